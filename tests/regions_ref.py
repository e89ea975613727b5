"""Reference of dn_forward_regions (include/demonet_hip.h): the network input of a region is what the uint8 path computes from the rectangle cut
out of the converted frame, mirrored when flagged. `crop` states that in numpy (converted frame -> crop -> optional mirror); `resize_u8` is the
uint8 path's resize in fp32, one rounding per operation; `sample` computes the same network input the way a kernel does -- tap by tap from the
planes -- and takes three deliberate mistakes, which the tests use to show that a set of regions can tell right from wrong. Nothing here is
fitted to device output."""
import numpy as np

import frames_ref as fr

F = np.float32

# (height, width) of the two test frames and the regions (frame, x0, y0, w, h, flip) the GPU tests run: odd origins, both flips, an upscale, a
# downscale, the identity size at an odd origin, one pixel more than it, whole frames, the odd frame's last row and column, a single pixel
SIZES = [(200, 260), (97, 131)]
REGIONS = [(0, 37, 21, 91, 67, 0), (0, 37, 21, 91, 67, 1), (0, 51, 33, 160, 160, 0), (0, 51, 33, 160, 160, 1), (0, 99, 39, 161, 161, 0),
           (0, 3, 5, 255, 193, 1), (0, 0, 0, 260, 200, 0), (1, 0, 0, 131, 97, 1), (1, 90, 60, 41, 37, 0), (1, 130, 96, 1, 1, 0), (1, 1, 1, 2, 3, 1)]


def crop(rgb, region):
    """rgb: [H, W, 3] uint8, the converted frame; region: (frame, x0, y0, w, h, flip) -> [h, w, 3] uint8, contiguous"""
    _, x0, y0, w, h, flip = region
    c = rgb[y0:y0 + h, x0:x0 + w]
    assert c.shape[:2] == (h, w)
    return np.ascontiguousarray(c[:, ::-1] if flip else c)


def _axis(n_in, n_out):
    """(i0, i1, l) of the bilinear resize n_in -> n_out (align_corners=False, no antialias) in fp32, one rounding per operation"""
    o = np.arange(n_out, dtype=F)
    r = F(n_in) / F(n_out)
    s = np.maximum(r * (o + F(0.5)) - F(0.5), F(0))
    assert s.dtype == F
    i0 = s.astype(np.int32)
    i1 = i0 + (i0 < n_in - 1)
    l = np.minimum(np.maximum(s - i0.astype(F), F(0)), F(1))
    return i0, i1, l


def _bilerp(a, b, c, d, lx, ly):
    """a, b, c, d: [oh, ow, 3] fp32 taps (top-left, top-right, bottom-left, bottom-right); lx [ow], ly [oh]"""
    hx, hy = (F(1) - lx)[None, :, None], (F(1) - ly)[:, None, None]
    lx, ly = lx[None, :, None], ly[:, None, None]
    top, bot = hx * a + lx * b, hx * c + lx * d
    out = hy * top + ly * bot
    assert out.dtype == F
    return out


def resize_u8(img, oh, ow):
    """img [h, w, 3] uint8 -> [3, oh, ow] fp32: x / 255, then the bilinear resize"""
    h, w, _ = img.shape
    y0, y1, ly = _axis(h, oh)
    x0, x1, lx = _axis(w, ow)
    v = img.astype(F) / F(255)
    out = _bilerp(v[y0][:, x0], v[y0][:, x1], v[y1][:, x0], v[y1][:, x1], lx, ly)
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def sample(Y, U, V, matrix, full, region, oh, ow, chroma_local=False, frame_clamp=False, ignore_flip=False):
    """The network input [3, oh, ow] fp32 of a region, tap by tap from the planes of its frame (Y [H, W], U, V [ceil(H/2), ceil(W/2)]).
    The mistakes: chroma_local -- the chroma sample taken at the region's chroma origin plus the region-local (xr >> 1, yr >> 1) instead of
    (X >> 1, Y >> 1) of the frame pixel; frame_clamp -- the second tap clamped at the frame's last row / column instead of the region's;
    ignore_flip -- the mirror flag not honoured."""
    _, rx, ry, w, h, flip = region
    H, W = Y.shape
    flip = bool(flip) and not ignore_flip
    y0, y1, ly = _axis(h, oh)
    x0, x1, lx = _axis(w, ow)
    if frame_clamp:
        y1 = y0 + (ry + y0 < H - 1)
        x1 = x0 + ((rx + (w - 1 - x0) > 0) if flip else (rx + x0 < W - 1))

    def tap(yr, xr):
        xl = (w - 1 - xr) if flip else xr
        X, Yp = rx + xl, ry + yr
        if chroma_local:
            cx, cy = (rx >> 1) + (xl >> 1), (ry >> 1) + (yr >> 1)
        else:
            cx, cy = X >> 1, Yp >> 1
        rgb = fr.yuv_to_rgb_int(Y[Yp][:, X], U[cy][:, cx], V[cy][:, cx], matrix, full)
        return rgb.astype(F) / F(255)

    out = _bilerp(tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1), lx, ly)
    return np.ascontiguousarray(out.transpose(2, 0, 1))


MISTAKES = ("chroma_local", "frame_clamp", "ignore_flip")
