"""Reference of the colour conversion of dn_forward_frames (include/demonet_hip.h): the integer formulas in numpy, and a float64 statement of the
same matrices derived from Kr, Kb. Nothing here is fitted to device output.

    y = Y - yo, u = U - 128, v = V - 128
    R = clamp((cy y + crv v + 2^13) >> 14), G = clamp((cy y - cgu u - cgv v + 2^13) >> 14), B = clamp((cy y + cbu u + 2^13) >> 14)

Chroma of pixel (x, y) is the sample (x >> 1, y >> 1)."""
import numpy as np

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
VARIANTS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]
SHIFT = 14


def real_coeffs(matrix, full):
    """(cy, crv, cbu, cgu, cgv, yo) as real numbers"""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    cy, cs, yo = (1.0, 1.0, 0) if full else (255.0 / 219.0, 255.0 / 224.0, 16)
    return cy, 2 * (1 - kr) * cs, 2 * (1 - kb) * cs, 2 * kb * (1 - kb) / kg * cs, 2 * kr * (1 - kr) / kg * cs, yo


def int_coeffs(matrix, full):
    c = real_coeffs(matrix, full)
    return tuple(int(np.floor(x * (1 << SHIFT) + 0.5)) for x in c[:5]) + (c[5],)


def yuv_to_rgb_real(Y, U, V, matrix, full):
    """float64, not rounded, not clamped; [..., 3]"""
    cy, crv, cbu, cgu, cgv, yo = real_coeffs(matrix, full)
    y, u, v = np.asarray(Y, np.float64) - yo, np.asarray(U, np.float64) - 128.0, np.asarray(V, np.float64) - 128.0
    return np.stack([cy * y + crv * v, cy * y - cgu * u - cgv * v, cy * y + cbu * u], -1)


def yuv_to_rgb_int(Y, U, V, matrix, full, clamp=True, swap_uv=False, offset=128, truncate=False):
    """the integer formulas; the keyword mutants are the classic mistakes (tests only). [..., 3] int32 (uint8 values when clamped)"""
    cy, crv, cbu, cgu, cgv, yo = int_coeffs(matrix, full)
    if swap_uv:
        U, V = V, U
    y, u, v = np.asarray(Y, np.int32) - yo, np.asarray(U, np.int32) - offset, np.asarray(V, np.int32) - offset
    half = 1 << (SHIFT - 1)
    s = np.stack([cy * y + crv * v + half, cy * y - cgu * u - cgv * v + half, cy * y + cbu * u + half], -1).astype(np.int32)
    if truncate:
        out = np.trunc(s.astype(np.float64) / (1 << SHIFT)).astype(np.int32)        # toward zero: C's `/`
    else:
        out = s >> SHIFT                                                           # arithmetic: floor
    return np.clip(out, 0, 255) if clamp else out


def rgb_to_yuv_real(rgb, matrix, full):
    """the forward matrix in float64 (for encoding known colours); rgb in 0..255; returns (Y, U, V) real"""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    r, g, b = [np.asarray(rgb, np.float64)[..., i] / 255.0 for i in range(3)]
    y = kr * r + kg * g + kb * b
    pb, pr = (b - y) / (2 * (1 - kb)), (r - y) / (2 * (1 - kr))
    if full:
        return 255.0 * y, 128.0 + 255.0 * pb, 128.0 + 255.0 * pr
    return 16.0 + 219.0 * y, 128.0 + 224.0 * pb, 128.0 + 224.0 * pr


# ---------------------------------------------------------------------------------------------------------------- whole frames
def chroma_size(h, w):
    return (h + 1) // 2, (w + 1) // 2


def noise_yuv(seed, h, w):
    """(Y [h, w], U [ch, cw], V [ch, cw]) uint8 i.i.d. noise over the whole byte range (out-of-range codes included: the clamp is exercised)"""
    rng = np.random.default_rng(seed)
    ch, cw = chroma_size(h, w)
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8)


def noise_rgb(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def planes_to_rgb(Y, U, V, matrix, full):
    """[h, w, 3] uint8: chroma sample (x >> 1, y >> 1) for pixel (x, y), then the integer formulas"""
    h, w = Y.shape
    yy, xx = np.arange(h) >> 1, np.arange(w) >> 1
    return yuv_to_rgb_int(Y, U[yy][:, xx], V[yy][:, xx], matrix, full).astype(np.uint8)


def pitched(plane, pitch, gap=0):
    """plane [rows, payload] uint8 inside a [rows, pitch] buffer whose gap bytes are `gap`; returns the buffer"""
    rows, payload = plane.shape
    buf = np.full((rows, pitch), gap, dtype=np.uint8)
    buf[:, :payload] = plane
    return buf


def interleave(U, V):
    """NV12's UV plane [ch, 2 cw]"""
    return np.stack([U, V], -1).reshape(U.shape[0], -1)
