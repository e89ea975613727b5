"""float64 reference of the input resize (csrc/dense.hip resize_kernel, u8hwc_kernel) and the bound an fp32 evaluation must keep.

bilinear_ref restates aten's upsample_bilinear2d with align_corners=False, size= given and no scale factor -- what the reference's transform
calls with fixed_size (transform.py:52-53):
    ratio = in / out;  src = max(ratio * (dst + 0.5) - 0.5, 0);  i0 = floor(src);  i1 = i0 + (i0 < in - 1);  l = src - i0
    out = (1 - ly) * ((1 - lx) * a + lx * b) + ly * ((1 - lx) * c + lx * d)
tests/test_resize.py ties it to F.interpolate in float64, holds two fp32 evaluations to the bound and shows that the bound catches the usual
mistakes. Nothing here is fitted to device output.
"""
import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32


def _coords(n_in, n_out):
    """(src, i0, i1, lambda) of one axis in float64"""
    src = np.maximum((n_in / n_out) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    return src, i0, i1, src - i0


def bilinear_ref(img, oh, ow):
    """img [..., h, w] (any real dtype) -> [..., oh, ow] float64"""
    img = np.asarray(img, dtype=np.float64)
    h, w = img.shape[-2:]
    _, y0, y1, ly = _coords(h, oh)
    _, x0, x1, lx = _coords(w, ow)
    ly = ly[:, None]
    a, b = img[..., y0[:, None], x0[None, :]], img[..., y0[:, None], x1[None, :]]
    c, d = img[..., y1[:, None], x0[None, :]], img[..., y1[:, None], x1[None, :]]
    return (1.0 - ly) * ((1.0 - lx) * a + lx * b) + ly * ((1.0 - lx) * c + lx * d)


def bound(img, oh, ow):
    """Per-element bound E [..., oh, ow] on |fp32 evaluation - bilinear_ref(img, oh, ow)|, u = 2^-24.

    An fp32 evaluation computes, per axis, r' = fl(in / out), p = fl(r' * (dst + 0.5)) (dst + 0.5 is exact), s = fl(p - 0.5), src' = max(s, 0):
        |r' - r| <= u r;   |p - r t| <= (2u + u^2) r t with t = dst + 0.5;   |s - (p - 0.5)| <= u |p - 0.5|
    max(., 0) does not expand distances, and r t = src + 0.5 where the clamp is idle (r t < 0.5 where it is not), so
        |src' - src| <= 2u (src + 0.5) + u src + O(u^2) (src + 1) <= dc := 3u (src + 1)          (the spare 2u covers the second-order terms)
    i0' = floor(src') and l' = src' - i0' are exact in fp32. The evaluation therefore is the bilinear surface B -- continuous, linear inside
    each cell in either coordinate, constant beyond the last row / column -- at (sy', sx') instead of (sy, sx), plus its own arithmetic:
      coordinate term   |B(sy', sx') - B(sy, sx)| <= dcy Gy + dcx Gx. Going from sy to sy' at a fixed x the slope of B is a convex combination
                        of two vertical neighbour differences of the cell it is in; dc < 1, so that cell is y0 - 1, y0 or y0 + 1, and (the
                        x coordinate being off too) its columns are among x0 - 1 .. x0 + 2. Gy is the largest |img[i + 1, j] - img[i, j]|
                        over rows y0 - 1 .. y0 + 2 and those columns (indices clamped into the image); Gx likewise. An i0 that flips at an
                        integer coordinate is inside this term: B is continuous there.
      arithmetic term   every one of the four products w a reaches the result through fl(1 - lx), fl(1 - ly), the / 255 of the uint8 path,
                        two multiplications and two additions: seven roundings, (1 + u)^7 - 1 <= g7 := 7u / (1 - 7u) relative to
                        sum w |a| <= max |a, b, c, d| (the exact weights are non-negative and sum to 1). The maximum is taken over the same
                        4 x 4 window, since the cell may be a neighbour.
    E = dcy Gy + dcx Gx + g7 max|window|."""
    img = np.asarray(img, dtype=np.float64)
    h, w = img.shape[-2:]
    sy, y0, _, _ = _coords(h, oh)
    sx, x0, _, _ = _coords(w, ow)
    rows = np.clip(y0[:, None] + np.arange(-1, 3)[None, :], 0, h - 1)            # [oh, 4]
    cols = np.clip(x0[:, None] + np.arange(-1, 3)[None, :], 0, w - 1)            # [ow, 4]
    win = img[..., rows[:, None, :, None], cols[None, :, None, :]]                # [..., oh, ow, 4, 4]
    gy = np.abs(np.diff(win, axis=-2)).max(axis=(-2, -1))
    gx = np.abs(np.diff(win, axis=-1)).max(axis=(-2, -1))
    amax = np.abs(win).max(axis=(-2, -1))
    dcy = (3.0 * U * (sy + 1.0))[:, None]
    dcx = (3.0 * U * (sx + 1.0))[None, :]
    return dcy * gy + dcx * gx + (7.0 * U / (1.0 - 7.0 * U)) * amax


def emulate_fp32(img, oh, ow, half_pixel=True, swap_ratios=False, clamp_x1=True, clamp_src=True, nearest=False, align_corners=False):
    """resize_kernel's statements in numpy float32, same order, one rounding per operation. img [p, h, w] float32 -> [p, oh, ow] float32.
    The keyword arguments switch on one mistake each (the mutants of test_resize.py):
      half_pixel=False     src = ratio * dst
      align_corners=True   ratio = (in - 1) / (out - 1), src = ratio * dst
      swap_ratios=True     rh and rw exchanged
      clamp_x1=False       x1 = x0 + 1 always: at x0 = w - 1 it reads the next row's first pixel (flat addressing, as the kernel's)
      clamp_src=False      no max(src, 0) and no clamp of the weights: extrapolation above the first row / left of the first column
      nearest=True         the pixel at (y0, x0)"""
    img = np.ascontiguousarray(img, dtype=np.float32)
    p, h, w = img.shape
    f = np.float32
    rh, rw = f(h) / f(oh), f(w) / f(ow)
    if align_corners:
        rh, rw = f(h - 1) / f(max(oh - 1, 1)), f(w - 1) / f(max(ow - 1, 1))
    if swap_ratios:
        rh, rw = rw, rh
    oy, ox = np.arange(oh, dtype=np.float32), np.arange(ow, dtype=np.float32)
    if half_pixel and not align_corners:
        sy, sx = rh * (oy + f(0.5)) - f(0.5), rw * (ox + f(0.5)) - f(0.5)
    else:
        sy, sx = rh * oy, rw * ox
    if clamp_src:
        sy, sx = np.maximum(sy, f(0)), np.maximum(sx, f(0))
    y0, x0 = np.minimum(sy.astype(np.int64), h - 1), np.minimum(sx.astype(np.int64), w - 1)      # (int): truncation; the min guards the mutants' reads only
    y1 = y0 + (y0 < h - 1)
    x1 = x0 + ((x0 < w - 1) if clamp_x1 else 1)
    ly, lx = sy - y0.astype(np.float32), sx - x0.astype(np.float32)
    if clamp_src:
        ly, lx = np.minimum(np.maximum(ly, f(0)), f(1)), np.minimum(np.maximum(lx, f(0)), f(1))
    hy, hx = (f(1) - ly)[:, None], (f(1) - lx)[None, :]
    ly, lx = ly[:, None], lx[None, :]
    flat = img.reshape(p, h * w)
    at = lambda yy, xx: flat[:, np.minimum(yy[:, None] * w + xx[None, :], h * w - 1)]
    a, b, c, d = at(y0, x0), at(y0, x1), at(y1, x0), at(y1, x1)
    if nearest:
        return a
    t0, t1, b0, b1 = hx * a, lx * b, hx * c, lx * d
    top, bot = t0 + t1, b0 + b1
    u, v = hy * top, ly * bot
    out = u + v
    assert out.dtype == np.float32
    return out


def noise(seed, n, h, w):
    """[n, 3, h, w] float32: i.i.d. uniform noise in [0, 1] (rough: neighbouring pixels are unrelated) with exact 0.0 and 1.0 in the four corners"""
    x = np.random.default_rng(seed).random((n, 3, h, w), dtype=np.float32)
    x[..., 0, 0], x[..., -1, -1] = 0.0, 0.0
    x[..., 0, -1], x[..., -1, 0] = 1.0, 1.0
    return x


def noise_u8(seed, n, h, w):
    """[n, h, w, 3] uint8, uniform over 0 .. 255, with 0 and 255 in the corners"""
    x = np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    x[:, 0, 0], x[:, -1, -1] = 0, 0
    x[:, 0, -1], x[:, -1, 0] = 255, 255
    return x


# (name, h, w, n): the input sizes of tests/test_resize.py, resized to the network size of the model under test
CASES = [("up-97x131", 97, 131, 2), ("2x-320x320", 320, 320, 1), ("2x-640x480", 640, 480, 1), ("3x-480x480", 480, 480, 1),
         ("375x500", 375, 500, 1), ("500x375", 500, 375, 1), ("427x640", 427, 640, 1), ("1080x1920", 1080, 1920, 1),
         ("2160x3840", 2160, 3840, 1), ("1x1", 1, 1, 2), ("1x57", 1, 57, 2), ("57x1", 57, 1, 2), ("2x2", 2, 2, 2),
         ("48x64-n33", 48, 64, 33), ("48x64-n9", 48, 64, 9)]
