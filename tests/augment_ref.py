"""float64 reference of the training augmentation (csrc/augment.hip, dn_augment_batch; demonet_amd/augment.py) and the tolerance an fp32 evaluation
must keep.

`reference` restates, literally and in numpy float64, what include/demonet_hip.h states for dn_augment_batch: torchvision's tensor formulas of
RandomPhotometricDistort (the reference's data/transforms.py:190-239 calls ColorJitter on a float tensor), then canvas, crop and flip as array
operations, then resize_ref.bilinear_ref. `boxes_ref` restates the reference's box statements (transforms.py:184-185, 121-126, 37;
transform.py:278-292) in numpy float32, one IEEE operation each, so the sampler's boxes must equal it bit for bit. `emulate_fp32` is the kernel's
photometric arithmetic in numpy float32, one rounding per operation (the style of resize_ref.emulate_fp32).

torchvision is not a dependency of this project and the reference's transforms.py imports it, so neither can run in the tests; the restatement is
pinned by closed forms instead (tests/test_augment.py: hue by 1/3 turns red into green, saturation 0 gives gray, ...), as tests/cocoeval_ref.py is.
Nothing here is fitted to device output.

One deliberate difference from torchvision's text: _hsv2rgb writes `i = floor(6 h) % 6`, which also wraps a hue that was never reduced into
[0, 1). After `h = (h + f) mod 1` the only value the `% 6` can still change is i = 6 at h == 1.0 exactly; `_hsv2rgb` below maps that one case to
sector 0 and lets every other i outside 0 .. 5 select no sector (all-zero mask, as torchvision's einsum would give): for every reduced hue the
two agree, and a missing `mod 1` shows (the hue_no_mod mutant) instead of being silently repaired.

The record objects are demonet_amd.augment.Params (read by attribute only).

Tolerance. An fp32 evaluation differs from `reference` by (a) the error of the resize of the image it gathered, bounded per element by
resize_ref.bound(V64, S_h, S_w) with V64 the float64 photometric, gathered image (that bound already covers the u8 / 255 conversion), plus (b) the
error of the photometric chain on each tap, which the convex bilinear weights do not amplify. (b) is not derived by hand (hue is a quotient of
differences); it is MEASURED on the host: the largest |emulate_fp32 - float64 photometric| over the inputs and parameters of the GPU cases
(tests/test_augment.py::test_photometric_tolerance prints it), times four because the device may contract or order a multiply-add differently
from the numpy emulation. It must stay under 1e-5: a larger value means the emulation is wrong, not that the tolerance should grow.
"""
import numpy as np

import resize_ref as rr

# largest |emulate_fp32 - float64 photometric| over tests/test_augment.py's GPU cases, measured on the host 2026-10-19: 9.313e-07
PHOTO_MEASURED = 9.32e-07
PHOTO_TOL = 4.0 * PHOTO_MEASURED


def _factor(v):
    return float(np.float32(v))


def gray(x):
    return 0.2989 * x[..., 0] + 0.587 * x[..., 1] + 0.114 * x[..., 2]


def blend(a, b, f):
    return np.clip(f * a + (1.0 - f) * b, 0.0, 1.0)


def rgb2hsv(x):
    """torchvision _rgb2hsv on [..., 3]"""
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    maxc, minc = x.max(axis=-1), x.min(axis=-1)
    eqc = maxc == minc
    cr = maxc - minc
    ones = np.ones_like(maxc)
    s = cr / np.where(eqc, ones, maxc)
    div = np.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = np.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    return np.stack((h, s, maxc), axis=-1)


def hsv2rgb(x):
    """torchvision _hsv2rgb on [..., 3]; the sector of h == 1.0 is 0, any other i outside 0 .. 5 selects nothing (see the module docstring)"""
    h, s, v = x[..., 0], x[..., 1], x[..., 2]
    i = np.floor(h * 6.0)
    f = h * 6.0 - i
    i = np.where(h == 1.0, 0, i.astype(np.int64))
    p = np.clip(v * (1.0 - s), 0.0, 1.0)
    q = np.clip(v * (1.0 - s * f), 0.0, 1.0)
    t = np.clip(v * (1.0 - s * (1.0 - f)), 0.0, 1.0)
    mask = (i[..., None] == np.arange(6)).astype(x.dtype)                        # [..., 6]
    a1 = np.stack((v, q, p, p, t, v), axis=-1)
    a2 = np.stack((t, v, v, q, p, p), axis=-1)
    a3 = np.stack((p, p, t, v, v, q), axis=-1)
    return np.stack(((mask * a1).sum(-1), (mask * a2).sum(-1), (mask * a3).sum(-1)), axis=-1)


def adjust_hue(x, f, no_mod=False):
    hsv = rgb2hsv(x)
    h = hsv[..., 0] + f
    if not no_mod:
        h = np.mod(h, 1.0)
    return hsv2rgb(np.stack((h, hsv[..., 1], hsv[..., 2]), axis=-1))


def photometric(u8, par, mean_before_brightness=False, hue_no_mod=False):
    """u8 [h, w, 3] uint8 -> [h, w, 3] float64, channels permuted. Mutants: mean_before_brightness = the contrast mean of the undistorted image;
    hue_no_mod = the hue shifted without the mod 1."""
    x = np.asarray(u8, dtype=np.float64) / 255.0
    m0 = gray(x).mean()

    def contrast(x):
        m = m0 if mean_before_brightness else gray(x).mean()
        return blend(x, m, _factor(par.contrast))

    if par.brightness is not None:
        x = blend(x, 0.0, _factor(par.brightness))
    if par.contrast is not None and par.contrast_before:
        x = contrast(x)
    if par.saturation is not None:
        x = blend(x, gray(x)[..., None], _factor(par.saturation))
    if par.hue is not None:
        x = adjust_hue(x, _factor(par.hue), hue_no_mod)
    if par.contrast is not None and not par.contrast_before:
        x = contrast(x)
    return x[..., list(par.perm)]


def gather(xp, par, permute_fill=False, flip_before_crop=False):
    """xp [h, w, 3] (any float dtype) -> [3, crop_h, crop_w] of the same dtype: canvas, crop and flip as array operations. Mutants: permute_fill = the
    fill goes through the channel permutation too; flip_before_crop = the canvas is flipped, then cropped."""
    h, w = xp.shape[:2]
    fill = np.array([np.float32(v) for v in par.fill], dtype=np.float32).astype(xp.dtype)
    if permute_fill:
        fill = fill[list(par.perm)]
    canvas = np.empty((par.canvas_h, par.canvas_w, 3), dtype=xp.dtype)
    canvas[:] = fill
    canvas[par.top:par.top + h, par.left:par.left + w] = xp
    if flip_before_crop and par.flip:
        canvas = canvas[:, ::-1]
    crop = canvas[par.crop_t:par.crop_t + par.crop_h, par.crop_l:par.crop_l + par.crop_w]
    if par.flip and not flip_before_crop:
        crop = crop[:, ::-1]
    assert crop.shape[:2] == (par.crop_h, par.crop_w)
    return np.ascontiguousarray(crop.transpose(2, 0, 1))


def reference(u8, par, oh, ow, **mutant):
    """(V64 [3, crop_h, crop_w], out [3, oh, ow]) float64"""
    pm = {k: v for k, v in mutant.items() if k in ("mean_before_brightness", "hue_no_mod")}
    gm = {k: v for k, v in mutant.items() if k in ("permute_fill", "flip_before_crop")}
    assert len(pm) + len(gm) == len(mutant)
    v64 = gather(photometric(u8, par, **pm), par, **gm)
    return v64, rr.bilinear_ref(v64, oh, ow)


def bound(v64, oh, ow):
    """per-element bound [3, oh, ow] on |fp32 evaluation - reference|"""
    return rr.bound(v64, oh, ow) + PHOTO_TOL


def boxes_ref(boxes, labels, par, out_hw):
    """The reference's box statements in numpy float32. boxes [G, 4] xyxy pixels of the source image -> (boxes, labels) in out_hw = (S_h, S_w)."""
    f = np.float32
    b = np.array(boxes, dtype=np.float32).reshape(-1, 4).copy()
    lab = np.array(labels).copy()
    b[:, 0::2] = b[:, 0::2] + f(par.left)                                        # transforms.py:184-185
    b[:, 1::2] = b[:, 1::2] + f(par.top)
    whole = (par.crop_l, par.crop_t, par.crop_w, par.crop_h) == (0, 0, par.canvas_w, par.canvas_h)
    assert par.option < 1.0 or whole, "a record whose crop is not its whole canvas must carry the IoU option it was drawn with (option < 1)"
    if par.option < 1.0:                                                         # transforms.py:107-126
        left, top, right, bottom = par.crop_l, par.crop_t, par.crop_l + par.crop_w, par.crop_t + par.crop_h
        cx = f(0.5) * (b[:, 0] + b[:, 2])
        cy = f(0.5) * (b[:, 1] + b[:, 3])
        within = (f(left) < cx) & (cx < f(right)) & (f(top) < cy) & (cy < f(bottom))
        b, lab = b[within], lab[within]
        b[:, 0::2] = np.clip(b[:, 0::2] - f(left), f(0), f(par.crop_w))
        b[:, 1::2] = np.clip(b[:, 1::2] - f(top), f(0), f(par.crop_h))
    if par.flip:                                                                 # transforms.py:37
        b[:, [0, 2]] = f(par.crop_w) - b[:, [2, 0]]
    rh, rw = f(out_hw[0]) / f(par.crop_h), f(out_hw[1]) / f(par.crop_w)          # transform.py:278-292
    out = np.stack((b[:, 0] * rw, b[:, 1] * rh, b[:, 2] * rw, b[:, 3] * rh), axis=1)
    assert out.dtype == np.float32
    return out, lab


# ---- the kernel's arithmetic in numpy float32 ----

def _gray32(r, g, b):
    f = np.float32
    return (f(0.2989) * r + f(0.587) * g) + f(0.114) * b


def _clamp32(v):
    return np.minimum(np.maximum(v, np.float32(0)), np.float32(1))


def _blend32(a, b, fac):
    f1 = np.float32(1) - fac
    return _clamp32(fac * a + f1 * b)


def _hue32(r, g, b, fac):
    f = np.float32
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    eqc = maxc == minc
    cr = maxc - minc
    one = np.ones_like(maxc)
    s = cr / np.where(eqc, one, maxc)
    div = np.where(eqc, one, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    zero = np.zeros_like(maxc)
    hr = np.where(maxc == r, bc - gc, zero)
    hg = np.where((maxc == g) & (maxc != r), (f(2) + rc) - bc, zero)
    hb = np.where((maxc != g) & (maxc != r), (f(4) + gc) - rc, zero)
    h = (hr + hg) + hb
    h = np.fmod(h / f(6) + f(1), f(1))
    h = h + fac
    h = h - np.floor(h)
    v = maxc
    h6 = h * f(6)
    fl = np.floor(h6)
    fr = h6 - fl
    i = fl.astype(np.int32)
    i = np.where(i >= 6, i - 6, i)
    p = _clamp32(v * (f(1) - s))
    q = _clamp32(v * (f(1) - s * fr))
    t = _clamp32(v * (f(1) - s * (f(1) - fr)))
    sel = lambda a, b_, c, d: np.where((i == a[0]) | (i == a[1]), v, np.where(i == b_, q, np.where(i == c, t, p)))
    out = sel((0, 5), 1, 4, None), sel((1, 2), 3, 0, None), sel((3, 4), 5, 2, None)
    assert all(o.dtype == np.float32 for o in out)
    return out


def emulate_fp32(u8, par):
    """augment.hip's photometric chain on a whole image: u8 [h, w, 3] -> [h, w, 3] float32 (channels permuted). The mean is the double sum of the
    fp32 grays (its order does not reach fp32), divided by the pixel count in double, rounded to fp32."""
    f = np.float32
    x = np.asarray(u8).astype(np.float32) / f(255)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    mean = lambda: f(_gray32(r, g, b).astype(np.float64).sum() / float(r.size))
    if par.brightness is not None:
        fac = f(par.brightness)
        r, g, b = _clamp32(fac * r), _clamp32(fac * g), _clamp32(fac * b)
    if par.contrast is not None and par.contrast_before:
        m, fac = mean(), f(par.contrast)
        r, g, b = _blend32(r, m, fac), _blend32(g, m, fac), _blend32(b, m, fac)
    if par.saturation is not None:
        fac, y = f(par.saturation), _gray32(r, g, b)
        r, g, b = _blend32(r, y, fac), _blend32(g, y, fac), _blend32(b, y, fac)
    if par.hue is not None:
        r, g, b = _hue32(r, g, b, f(par.hue))
    if par.contrast is not None and not par.contrast_before:
        m, fac = mean(), f(par.contrast)
        r, g, b = _blend32(r, m, fac), _blend32(g, m, fac), _blend32(b, m, fac)
    out = np.stack((r, g, b), axis=-1)[..., list(par.perm)]
    assert out.dtype == np.float32
    return out


def emulate_full(u8, par, oh, ow):
    """the whole call in numpy float32: emulate_fp32, the gather, resize_ref.emulate_fp32 -> [3, oh, ow] float32"""
    return rr.emulate_fp32(gather(emulate_fp32(u8, par), par), oh, ow)


# ---- the full-chain cases of tests/test_augment.py (GPU: every element against `bound`; CPU: PHOTO_MEASURED and the emulation against the same bound) ----

FULL_SIZES = [(37, 53), (97, 131), (375, 500)]       # 375 x 500 = 187 500 pixels: 46 reduction chunks of 4 096, the last one partial
FULL_OUTS = [(24, 40), (320, 320)]


def _zoomed(P, h, w, **kw):
    """a canvas 1.7 x 1.5 times the image, the image off-centre, a crop that holds fill on two sides and part of the image, flipped"""
    Hc, Wc = int(h * 1.7), int(w * 1.5)
    top, left = (Hc - h) // 3, (Wc - w) // 2
    return P(canvas_h=Hc, canvas_w=Wc, left=left, top=top, crop_l=left // 2, crop_t=top // 2, crop_w=left // 2 + (2 * w) // 3, crop_h=top // 2 + (3 * h) // 4,
             flip=True, **kw)


def chain_params(P, h, w):
    """[(name, Params)]: each photometric step alone, both contrast orders, all steps together with zoom, crop and flip. P = demonet_amd.augment.Params"""
    ident = lambda **kw: P.identity(h, w, **kw)
    return [("brightness", ident(brightness=1.125)), ("contrast-before", ident(contrast=1.5, contrast_before=True)),
            ("contrast-after", ident(contrast=0.5)), ("saturation", ident(saturation=1.5)), ("hue+", ident(hue=0.05)), ("hue-", ident(hue=-0.05)),
            ("hue-half", ident(hue=0.5)),
            ("all-before", _zoomed(P, h, w, brightness=0.875, contrast=1.5, contrast_before=True, saturation=0.5, hue=-0.05, perm=(2, 0, 1))),
            ("all-after", _zoomed(P, h, w, brightness=1.125, contrast=0.5, saturation=1.5, hue=0.05, perm=(1, 2, 0), fill=(0.1, 0.9, 0.3)))]


def full_cases(P):
    """[(name, images [n x uint8 [h, w, 3]], params [n], (oh, ow))]"""
    cases = []
    for k, (h, w) in enumerate(FULL_SIZES):
        img = rr.noise_u8(100 + k, 1, h, w)[0]
        named = chain_params(P, h, w)
        for oh, ow in FULL_OUTS:
            cases.append(("%dx%d-to-%dx%d" % (h, w, oh, ow), [img] * len(named), [p for _, p in named], (oh, ow)))
    # 33 images of mixed sizes, contrast on for every third one only (the others' workgroups of the mean launch exit at once)
    imgs, pars = [], []
    for i in range(33):
        h, w = 3 + (7 * i) % 41, 2 + (11 * i) % 59
        imgs.append(rr.noise_u8(200 + i, 1, h, w)[0])
        if i % 3 == 0:
            pars.append(_zoomed(P, h, w, brightness=1.1, contrast=0.7 + 0.02 * i, contrast_before=bool(i % 2), hue=0.03) if h > 4 and w > 4
                        else P.identity(h, w, contrast=1.3, contrast_before=bool(i % 2)))
        else:
            pars.append(P.identity(h, w, saturation=0.8 if i % 3 == 1 else None, flip=bool(i % 2), perm=(0, 2, 1)))
    cases.append(("n33-mixed", imgs, pars, (24, 40)))
    return cases
