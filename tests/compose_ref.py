"""Reference of the surface composition (include/demonet_hip.h, dn_compose) in numpy, in exact integers: the area filter as two
weight matrices and one integer division, the colour conversions of tests/frames_ref.py on the way in and the forward matrix, derived here from Kr,
Kb in float64, on the way out. Nothing here is fitted to device output. The keyword `mistake` makes the classic wrong resamplers (tests only):

    nearest       the source sample at floor(j sw / dw), no filter
    bilinear      two-tap interpolation at pixel centres (F.interpolate(mode="bilinear") rounded half up)
    floor         the exact sums, divided without the D / 2
    chroma_luma   the chroma rectangles taken at the luma origin (x0, y0) instead of (x0 / 2, y0 / 2)
    pool          adaptive_avg_pool windows [floor(j sw / dw), ceil((j + 1) sw / dw)) with equal weights
    swap_uv       U and V exchanged on the way out
"""
import numpy as np

import frames_ref as fr

MISTAKES = ("nearest", "bilinear", "floor", "chroma_luma", "pool", "swap_uv")
SHIFT = 14
YUV = ("nv12", "i420")
DST_SIZES = [(128, 160), (67, 91)]          # (height, width) of the destinations of the scenes below: one even, one odd


def forward_coeffs(matrix, full):
    """((yr, yg, yb), (ur, ug, ub), (vr, vg, vb), yo): round(c 2^14) of the RGB -> YUV matrix"""
    kr, kb = fr.KR_KB[matrix]
    kg = 1.0 - kr - kb
    sy, sc, yo = (1.0, 1.0, 0) if full else (219.0 / 255.0, 224.0 / 255.0, 16)
    rows = ((kr * sy, kg * sy, kb * sy), (-kr / (2 * (1 - kb)) * sc, -kg / (2 * (1 - kb)) * sc, 0.5 * sc),
            (0.5 * sc, -kg / (2 * (1 - kr)) * sc, -kb / (2 * (1 - kr)) * sc))
    q = tuple(tuple(int(np.floor(c * (1 << SHIFT) + 0.5)) for c in row) for row in rows)
    return q[0], q[1], q[2], yo


def component(c, rgb, off):
    """clamp(((c0 R + c1 G + c2 B + 2^13) >> 14) + off) of an int64 [..., 3] array"""
    v = c[0] * rgb[..., 0] + c[1] * rgb[..., 1] + c[2] * rgb[..., 2] + (1 << (SHIFT - 1))
    return np.clip((v >> SHIFT) + off, 0, 255)


def weights(s, d):
    """[d, s] int64: the length of [j s, (j + 1) s) intersected with [c d, (c + 1) d); every row sums to s"""
    j = np.arange(d, dtype=np.int64)[:, None]
    c = np.arange(s, dtype=np.int64)[None, :]
    return np.maximum(np.minimum((j + 1) * s, (c + 1) * d) - np.maximum(j * s, c * d), 0)


def area(p, dh, dw, mistake=None):
    """[sh, sw] -> [dh, dw], int64 in, int64 out: (sum wy wx p + D / 2) / D with D = sw sh"""
    p = np.asarray(p, np.int64)
    sh, sw = p.shape
    if mistake == "nearest":
        return p[(np.arange(dh) * sh) // dh][:, (np.arange(dw) * sw) // dw]
    if mistake == "bilinear":
        def taps(s, d):
            x = np.clip((np.arange(d) + 0.5) * s / d - 0.5, 0, s - 1)
            lo = np.floor(x).astype(np.int64)
            return lo, np.minimum(lo + 1, s - 1), x - lo
        y0, y1, fy = taps(sh, dh)
        x0, x1, fx = taps(sw, dw)
        top = p[y0][:, x0] * (1 - fx) + p[y0][:, x1] * fx
        bot = p[y1][:, x0] * (1 - fx) + p[y1][:, x1] * fx
        return np.floor(top * (1 - fy)[:, None] + bot * fy[:, None] + 0.5).astype(np.int64)
    if mistake == "pool":
        wy, wx = (weights(sh, dh) > 0).astype(np.int64), (weights(sw, dw) > 0).astype(np.int64)
        n = wy.sum(1)[:, None] * wx.sum(1)[None, :]
        return (wy @ p @ wx.T + n // 2) // n
    acc = weights(sh, dh) @ p @ weights(sw, dw).T
    D = sw * sh
    assert D <= 1 << 24 and acc.max() <= 255 * D
    return acc // D if mistake == "floor" else (acc + D // 2) // D


# ---------------------------------------------------------------------------------------------------------------- surfaces as channels
def channels(fmt, planes):
    """the payload planes of a surface as three [rows, samples] arrays: Y, U, V or R, G, B"""
    if fmt == "nv12":
        return [planes[0], planes[1][:, 0::2], planes[1][:, 1::2]]
    if fmt == "i420":
        return list(planes)
    px = planes[0].reshape(planes[0].shape[0], -1, 3)
    return [px[..., i] for i in ((0, 1, 2) if fmt == "rgb24" else (2, 1, 0))]


def planes_of(fmt, chans):
    """the inverse of channels(): uint8 payload planes"""
    c = [np.asarray(x).astype(np.uint8) for x in chans]
    if fmt == "nv12":
        return [c[0], fr.interleave(c[1], c[2])]
    if fmt == "i420":
        return c
    px = np.stack(c if fmt == "rgb24" else c[::-1], -1)
    return [px.reshape(px.shape[0], -1)]


def rgb_of(fmt, matrix, full, chans):
    """[h, w, 3] int64 RGB8 of a surface's channels: frames_ref's integer formulas, chroma sample (x >> 1, y >> 1)"""
    if fmt in YUV:
        return fr.planes_to_rgb(chans[0], chans[1], chans[2], matrix, full).astype(np.int64)
    return np.stack(chans, -1).astype(np.int64)


def compose(src_planes, dst_planes, items, src, dst, mistake=None):
    """The destinations after dn_compose. src_planes / dst_planes: per surface the list of payload planes; items: (src, src_rect, dst, dst_rect)
    with rectangles (x0, y0, w, h); src, dst: (format, matrix, full_range). Returns new payload planes per destination surface."""
    sfmt, dfmt = src[0], dst[0]
    planewise = sfmt in YUV and dfmt in YUV and src[1:] == dst[1:]
    sc = [channels(sfmt, p) for p in src_planes]
    out = [[np.array(c, np.int64) for c in channels(dfmt, p)] for p in dst_planes]
    rgb_cache = {}
    half = lambda r: (r[0] // 2, r[1] // 2, (r[2] + 1) // 2, (r[3] + 1) // 2)      # noqa: E731
    for s, (sx0, sy0, sw, sh), d, (dx0, dy0, dw, dh) in items:
        if planewise:
            out[d][0][dy0:dy0 + dh, dx0:dx0 + dw] = area(sc[s][0][sy0:sy0 + sh, sx0:sx0 + sw], dh, dw, mistake)
            cx, cy, cw, ch = half((sx0, sy0, sw, sh))
            ex, ey, ew, eh = half((dx0, dy0, dw, dh))
            if mistake == "chroma_luma":
                CH, CW = sc[s][1].shape
                cx, cy = min(sx0, CW - cw), min(sy0, CH - ch)
            for k in (1, 2):
                out[d][3 - k if mistake == "swap_uv" else k][ey:ey + eh, ex:ex + ew] = area(sc[s][k][cy:cy + ch, cx:cx + cw], eh, ew, mistake)
            continue
        if s not in rgb_cache:
            rgb_cache[s] = rgb_of(sfmt, src[1], src[2], sc[s])
        crop = rgb_cache[s][sy0:sy0 + sh, sx0:sx0 + sw]
        rgb = np.stack([area(crop[..., c], dh, dw, mistake) for c in range(3)], -1)
        if dfmt not in YUV:
            for c in range(3):
                out[d][c][dy0:dy0 + dh, dx0:dx0 + dw] = rgb[..., c]
            continue
        cyc, cuc, cvc, yo = forward_coeffs(dst[1], dst[2])
        out[d][0][dy0:dy0 + dh, dx0:dx0 + dw] = component(cyc, rgb, yo)
        ex, ey, ew, eh = half((dx0, dy0, dw, dh))
        pad = np.zeros((2 * eh, 2 * ew, 3), np.int64)
        cnt = np.zeros((2 * eh, 2 * ew), np.int64)
        pad[:dh, :dw], cnt[:dh, :dw] = rgb, 1
        n = cnt.reshape(eh, 2, ew, 2).sum((1, 3))
        mean = (pad.reshape(eh, 2, ew, 2, 3).sum((1, 3)) + (n // 2)[..., None]) // n[..., None]
        u, v = component(cuc, mean, 128), component(cvc, mean, 128)
        if mistake == "swap_uv":
            u, v = v, u
        if mistake == "chroma_luma":
            CH, CW = out[d][1].shape
            ex, ey = min(dx0, CW - ew), min(dy0, CH - eh)
        out[d][1][ey:ey + eh, ex:ex + ew] = u
        out[d][2][ey:ey + eh, ex:ex + ew] = v
    return [planes_of(dfmt, c) for c in out]


def applies(mistake, src, dst):
    """whether a mistake can show on this pair: the chroma mistakes need a chroma plane to write (swap_uv) or a chroma rectangle (chroma_luma)"""
    if mistake in ("swap_uv", "chroma_luma"):
        return dst[0] in YUV
    return True


# ---------------------------------------------------------------------------------------------------------------- scenes
def whole(sizes, i):
    return (0, 0, sizes[i][1], sizes[i][0])


def mixed_items(src_sizes):
    """The mixed scene over sources of regions_ref.SIZES and destinations of DST_SIZES, legal for every format pair (even origins):
    (src, src_rect, dst, dst_rect). In destination 0: a non-integer downscale that ends at the odd column 97 with a 2:1 item beside it at 98, a 4:1
    item, a 1:1 copy, a 1.5 x upscale, a 20:1 by 8:1 item, a whole frame into one pixel; uncovered payload remains. In the odd destination 1 four
    items: two non-integer downscales (the second ends at the frame's odd last column), a 2:1 sub-rectangle and an upscale."""
    w0, w1 = whole(src_sizes, 0), whole(src_sizes, 1)
    return [(0, w0, 0, (0, 0, 97, 75)), (0, (0, 0, 120, 100), 0, (98, 0, 60, 50)), (0, (20, 40, 240, 160), 0, (98, 50, 60, 40)),
            (1, (10, 20, 40, 30), 0, (0, 76, 40, 30)), (1, (30, 10, 40, 20), 0, (42, 92, 60, 30)), (0, w0, 0, (104, 92, 13, 25)),
            (1, w1, 0, (120, 92, 1, 1)),
            (0, w0, 1, (0, 0, 45, 33)), (1, w1, 1, (46, 0, 45, 33)), (0, (100, 50, 90, 66), 1, (0, 34, 45, 33)), (1, (0, 0, 30, 22), 1, (46, 34, 45, 33))]


def second_items(src_sizes):
    """other items, and fewer of them: what the captured call is replayed on"""
    w0, w1 = whole(src_sizes, 0), whole(src_sizes, 1)
    return [(1, w1, 0, (2, 4, 77, 59)), (0, (60, 20, 150, 90), 0, (80, 4, 50, 45)), (0, w0, 1, (10, 2, 65, 50)), (1, (64, 32, 33, 33), 0, (90, 70, 33, 33)),
            (0, (0, 100, 64, 96), 1, (0, 54, 16, 12))]


def many_items(src_sizes, side=48, cell=34):
    """side x side items of 33 x 33 destination pixels (four tiles each, three of them ragged) on a grid of `cell` pixels in ONE destination of
    (side cell) x (side cell): 1:1 copies, every fifth a 2:1 downscale, every seventh a 1.5 x upscale, sources alternating. With side = 48 these
    are 2304 items and 9216 tiles: more than two tiles per workgroup of the kernel's grid, and runs of tiles that cross item boundaries."""
    items = []
    for n in range(side * side):
        r, c = divmod(n, side)
        s = n & 1
        h, w = src_sizes[s]
        k = 66 if n % 5 == 0 else (22 if n % 7 == 0 else 33)
        x0, y0 = 2 * ((n * 7) % ((w - k) // 2 + 1)), 2 * ((n * 3) % ((h - k) // 2 + 1))
        items.append((s, (x0, y0, k, k), 0, (c * cell, r * cell, 33, 33)))
    return items


def api_items(items):
    """the (src, dst, dst_rect, src_rect) tuples Compositor.set takes"""
    return [(s, d, dr, sr) for s, sr, d, dr in items]


def noise_planes(fmt, seed, h, w):
    """payload planes of a noise surface of any format"""
    if fmt in YUV:
        Y, U, V = fr.noise_yuv(seed, h, w)
        return [Y, fr.interleave(U, V)] if fmt == "nv12" else [Y, U, V]
    rgb = fr.noise_rgb(seed, h, w)
    return [rgb.reshape(h, 3 * w)]
