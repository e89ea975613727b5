"""SSD training augmentation (demonet_amd/augment.py, csrc/augment.hip) against tests/augment_ref.py.

CPU: the ABI, closed-form pins of the float64 reference, the sampler over 2000 seeded draws, the photometric tolerance term (measured here, never on
the device) and the fp32 emulation inside the bound. GPU: geometry bit for bit, the full chain against the bound on every element, the bound
catching four mutants, determinism, rejections, and the preset in front of SSD.loss."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_ref as ar
import resize_ref as rr
from demonet_amd import _lib, augment
from demonet_amd.augment import Params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_RTOL = 2e-5            # tests/test_loss.py: model.loss against a second evaluation of the same loss


# ---------------------------------------------------------------- ABI

def test_abi_names_agree():
    hdr = open(os.path.join(ROOT, "include", "demonet_hip.h")).read()
    declared = set(re.findall(r"DN_API\s+[\w\s\*]+?\b(dn_\w+)\s*\(", hdr))
    if not os.path.exists(_lib.LIB_PATH):
        from demonet_amd import build
        build.build(verbose=False)
    L = C.CDLL(_lib.LIB_PATH)
    for name in ("dn_augment_workspace_bytes", "dn_augment_batch"):
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    # the record layout the Python side packs is the header's
    for name, val in re.findall(r"\b(DN_AUG_\w+) = (\d+)", hdr):
        py = name[len("DN_AUG_"):]
        assert getattr(augment, py) == int(val), name
    L.dn_augment_workspace_bytes.restype = C.c_size_t
    assert L.dn_augment_workspace_bytes(0) == 0 and L.dn_augment_workspace_bytes(3) == 3 * L.dn_augment_workspace_bytes(1) > 0


def test_pack_layout():
    p = Params(canvas_h=9, canvas_w=8, left=1, top=2, crop_l=3, crop_t=4, crop_w=5, crop_h=5, flip=True, hue=-0.05, contrast=1.5, contrast_before=True,
               perm=(2, 0, 1), fill=(0.25, 0.5, 0.75))
    r = augment.pack([p])
    assert r.shape == (1, 20) and r.dtype == np.int32
    f = r.view(np.float32)
    assert r[0, augment.FLAGS] == augment.F_CONTRAST | augment.F_HUE | augment.F_CONTRAST_BEFORE | augment.F_FLIP
    assert f[0, augment.HUE] == np.float32(-0.05) and f[0, augment.CONTRAST] == 1.5 and f[0, augment.BRIGHTNESS] == 1.0
    assert list(r[0, 5:12]) == [2, 0, 1, 9, 8, 1, 2] and list(f[0, 12:15]) == [0.25, 0.5, 0.75] and list(r[0, 15:20]) == [3, 4, 5, 5, 0]


# ---------------------------------------------------------------- reference pins

def _px(*rgb):
    return np.array(rgb, dtype=np.float64).reshape(1, 1, 3)


def test_ref_hue_closed_forms():
    assert np.allclose(ar.adjust_hue(_px(1, 0, 0), 1.0 / 3.0), _px(0, 1, 0), atol=1e-15)          # red -> green
    assert np.allclose(ar.adjust_hue(_px(0, 1, 0), 1.0 / 3.0), _px(0, 0, 1), atol=1e-15)          # green -> blue
    assert np.allclose(ar.adjust_hue(_px(0, 0, 1), -1.0 / 3.0), _px(0, 1, 0), atol=1e-15)         # and back, through the mod
    x = np.random.default_rng(0).random((7, 5, 3))
    assert np.allclose(ar.adjust_hue(x, 0.0), x, atol=1e-15)                                       # hue 0 is the identity
    g = np.repeat(np.random.default_rng(1).random((4, 4, 1)), 3, axis=2)
    for f in (-0.5, -0.05, 0.2, 0.5):
        assert np.array_equal(ar.adjust_hue(g, f), g)                                              # a gray pixel has no hue to shift
    # the sector of h == 1.0 is sector 0; a hue outside [0, 1] selects nothing (what the hue_no_mod mutant relies on)
    assert np.array_equal(ar.hsv2rgb(_px(1.0, 1.0, 1.0)), _px(1, 0, 0))
    assert np.array_equal(ar.hsv2rgb(_px(-0.1, 1.0, 1.0)), _px(0, 0, 0)) and np.array_equal(ar.hsv2rgb(_px(1.1, 1.0, 1.0)), _px(0, 0, 0))


def test_ref_blend_closed_forms():
    x = np.random.default_rng(2).integers(0, 256, (6, 8, 3), dtype=np.uint8)
    x64 = x / 255.0
    P = lambda **kw: Params.identity(6, 8, **kw)
    gray = ar.photometric(x, P(saturation=0.0))
    assert np.allclose(gray, ar.gray(x64)[..., None].repeat(3, 2), atol=1e-15)                     # saturation 0 gives gray
    assert np.allclose(ar.photometric(x, P(saturation=1.0)), x64, atol=1e-15)                      # saturation 1 is the identity
    black = np.zeros((5, 5, 3), dtype=np.uint8)
    for f in (0.5, 1.5):
        assert np.array_equal(ar.photometric(black, Params.identity(5, 5, contrast=f)), np.zeros((5, 5, 3)))      # (other constants: the next test)
    # half black, half white: mean gray = 0.9999 / 2; white -> clamp(1.5 - 0.5 * 0.49995), black -> clamp(-0.5 * 0.49995) = 0
    hw = np.zeros((2, 4, 3), dtype=np.uint8)
    hw[:, 2:] = 255
    out = ar.photometric(hw, Params.identity(2, 4, contrast=1.5))
    assert np.array_equal(out[:, :2], np.zeros((2, 2, 3))) and np.array_equal(out[:, 2:], np.ones((2, 2, 3)))
    out = ar.photometric(hw, Params.identity(2, 4, contrast=0.5))
    m = (0.2989 + 0.587 + 0.114) / 2.0
    assert np.allclose(out[:, :2], 0.5 * m, atol=1e-15) and np.allclose(out[:, 2:], 0.5 + 0.5 * m, atol=1e-15)
    assert ar.photometric(np.full((1, 1, 3), 250, np.uint8), Params.identity(1, 1, brightness=1.125)).max() == 1.0      # brightness clamps at 1
    assert np.allclose(ar.photometric(np.full((1, 1, 3), 100, np.uint8), Params.identity(1, 1, brightness=0.875)), 0.875 * 100 / 255.0, atol=1e-15)
    assert np.array_equal(ar.photometric(x, P(perm=(2, 1, 0))), x64[..., ::-1])                    # [2, 1, 0] swaps R and B
    # the contrast mean is the mean of the image as it stands: after brightness (and after saturation and hue when contrast comes last)
    a = ar.photometric(x, P(brightness=0.875, contrast=1.5, contrast_before=True))
    b = ar.blend(x64 * np.float32(0.875), ar.gray(x64 * np.float32(0.875)).mean(), 1.5)
    assert np.allclose(a, b, atol=1e-15)


def test_ref_constant_contrast_is_identity_up_to_the_gray_weights():
    """torchvision's gray weights sum to 0.9999, so the 'mean' of a constant image c is 0.9999 c: contrast f maps c to c (f + 0.9999 (1 - f))."""
    const = np.full((3, 3, 3), 200, dtype=np.uint8)
    c = 200 / 255.0
    out = ar.photometric(const, Params.identity(3, 3, contrast=1.5))
    assert np.allclose(out, c * (1.5 - 0.5 * 0.9999), atol=1e-15) and abs(out[0, 0, 0] - c) < 1e-4


def test_ref_geometry_equals_numpy_slicing():
    x = rr.noise_u8(5, 1, 6, 9)[0]
    x64 = x / 255.0
    fill = (0.25, 0.5, 0.75)
    for flip in (False, True):
        for perm in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
            p = Params(canvas_h=11, canvas_w=14, left=3, top=2, crop_l=1, crop_t=1, crop_w=12, crop_h=8, flip=flip, perm=perm, fill=fill)
            v64, out = ar.reference(x, p, 8, 12)
            want = np.pad(x64[..., list(perm)].transpose(2, 0, 1), ((0, 0), (2, 3), (3, 2)))
            for c in range(3):
                want[c][:2], want[c][8:], want[c][:, :3], want[c][:, 12:] = fill[c], fill[c], fill[c], fill[c]
            want = want[:, 1:9, 1:13]
            want = want[:, :, ::-1] if flip else want
            assert np.array_equal(v64, want) and np.array_equal(out, want)          # identity resize: weights exactly (1, 0)


def test_ref_resize_equals_interpolate():
    x = rr.noise_u8(6, 1, 13, 17)[0]
    p = Params(canvas_h=20, canvas_w=25, left=4, top=3, crop_l=2, crop_t=1, crop_w=19, crop_h=15, flip=True, hue=0.05, saturation=1.5)
    v64, out = ar.reference(x, p, 24, 40)
    want = F.interpolate(torch.from_numpy(v64)[None], size=(24, 40), mode="bilinear", align_corners=False)[0].numpy()
    assert np.abs(out - want).max() < 1e-14


# ---------------------------------------------------------------- sampler

H0, W0 = 240, 320
BOXES0 = torch.tensor([[10.0, 20.0, 110.0, 140.0], [150.5, 30.25, 300.0, 200.0], [60.0, 100.0, 90.0, 130.0], [200.0, 150.0, 319.0, 239.0],
                       [0.0, 0.0, 320.0, 240.0]])
LABELS0 = torch.tensor([3, 1, 4, 1, 5])


def _draws(n, seed, **kw):
    s = augment.AugmentSampler("ssd", size=(320, 320), **kw)
    g = torch.Generator().manual_seed(seed)
    tg = [{"boxes": BOXES0, "labels": LABELS0}] * n
    return s.sample([(H0, W0)] * n, tg, g)


@pytest.fixture(scope="module")
def draws():
    return _draws(2000, 1234)


def test_sampler_crops(draws):
    pars, tgs = draws
    seen = set()
    zoomed = 0
    for p in pars:
        seen.add(p.option)
        zoomed += (p.canvas_h, p.canvas_w) != (H0, W0)
        # the image sits inside its canvas
        assert p.left >= 0 and p.top >= 0 and p.left + W0 <= p.canvas_w and p.top + H0 <= p.canvas_h
        assert H0 <= p.canvas_h <= 4 * H0 and W0 <= p.canvas_w <= 4 * W0
        # the crop: integer sides, inside the canvas
        for v in (p.crop_l, p.crop_t, p.crop_w, p.crop_h):
            assert isinstance(v, int)
        assert p.crop_w >= 1 and p.crop_h >= 1 and p.crop_l >= 0 and p.crop_t >= 0
        assert p.crop_l + p.crop_w <= p.canvas_w and p.crop_t + p.crop_h <= p.canvas_h
        if p.option >= 1.0:
            assert (p.crop_l, p.crop_t, p.crop_w, p.crop_h) == (0, 0, p.canvas_w, p.canvas_h)
            continue
        assert 0.5 <= p.crop_w / p.crop_h <= 2.0
        assert 0.3 * p.canvas_w - 1 <= p.crop_w <= p.canvas_w and 0.3 * p.canvas_h - 1 <= p.crop_h <= p.canvas_h
        b = BOXES0.numpy() + np.array([p.left, p.top, p.left, p.top], dtype=np.float32)
        cx, cy = 0.5 * (b[:, 0] + b[:, 2]), 0.5 * (b[:, 1] + b[:, 3])
        inside = (p.crop_l < cx) & (cx < p.crop_l + p.crop_w) & (p.crop_t < cy) & (cy < p.crop_t + p.crop_h)
        assert inside.any()
        crop = np.array([p.crop_l, p.crop_t, p.crop_l + p.crop_w, p.crop_t + p.crop_h], dtype=np.float64)
        bb = b[inside].astype(np.float64)
        iw = np.clip(np.minimum(bb[:, 2], crop[2]) - np.maximum(bb[:, 0], crop[0]), 0, None)
        ih = np.clip(np.minimum(bb[:, 3], crop[3]) - np.maximum(bb[:, 1], crop[1]), 0, None)
        iou = iw * ih / ((bb[:, 2] - bb[:, 0]) * (bb[:, 3] - bb[:, 1]) + p.crop_w * p.crop_h - iw * ih)
        assert iou.max() >= p.option - 1e-6, (iou.max(), p.option)              # (the sampler compares in float32)
    assert seen == {0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0}
    assert 800 < zoomed < 1200 and 800 < sum(p.flip for p in pars) < 1200
    for k, (lo, hi) in (("brightness", (0.875, 1.125)), ("contrast", (0.5, 1.5)), ("saturation", (0.5, 1.5)), ("hue", (-0.05, 0.05))):
        vals = [getattr(p, k) for p in pars if getattr(p, k) is not None]
        assert 800 < len(vals) < 1200 and lo - 1e-6 <= min(vals) and max(vals) <= hi + 1e-6 and max(vals) - min(vals) > 0.9 * (hi - lo)
    assert 800 < sum(p.contrast_before for p in pars) < 1200
    assert {p.perm for p in pars} == {(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)}
    assert all(p.fill == tuple(float(np.float32(m / 255.0)) for m in (123.0, 117.0, 104.0)) for p in pars)


def test_sampler_boxes_equal_the_reference_statements_bit_for_bit(draws):
    pars, tgs = draws
    kept = 0
    for p, t in zip(pars, tgs):
        want_b, want_l = ar.boxes_ref(BOXES0.numpy(), LABELS0.numpy(), p, (320, 320))
        assert t["boxes"].dtype == torch.float32 and t["labels"].dtype == torch.int64
        assert np.array_equal(t["boxes"].numpy().view(np.uint32), want_b.view(np.uint32)) and np.array_equal(t["labels"].numpy(), want_l)
        kept += len(want_l)
    assert 2000 < kept < 10000          # some crops drop boxes, none drops all
    assert torch.equal(BOXES0, torch.tensor(BOXES0.tolist()))      # the caller's targets are not modified


def test_sampler_is_deterministic_and_policies(draws):
    a, ta = _draws(50, 7)
    b, tb = _draws(50, 7)
    assert a == b and all(torch.equal(x["boxes"], y["boxes"]) for x, y in zip(ta, tb))
    c, _ = _draws(50, 8)
    assert a != c
    # an image without boxes takes the as-is crop
    s = augment.AugmentSampler("ssd", size=(320, 320))
    g = torch.Generator().manual_seed(3)
    empty = {"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.int64)}
    pars, tgs = s.sample([(50, 60)] * 40, [empty] * 40, g)
    for p, t in zip(pars, tgs):
        assert p.option >= 1.0 and (p.crop_l, p.crop_t, p.crop_w, p.crop_h) == (0, 0, p.canvas_w, p.canvas_h)
        assert t["boxes"].shape == (0, 4) and t["labels"].shape == (0,)
    # 'hflip' draws nothing but the flip: one torch.rand(1) per image
    s = augment.AugmentSampler("hflip", size=(320, 320), hflip_prob=0.5)
    g, g2 = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    pars, tgs = s.sample([(H0, W0)] * 64, [{"boxes": BOXES0, "labels": LABELS0}] * 64, g)
    flips = [bool(torch.rand(1, generator=g2) < 0.5) for _ in range(64)]
    assert torch.equal(g.get_state(), g2.get_state())
    for p, fl in zip(pars, flips):
        assert p == Params.identity(H0, W0, flip=fl, fill=s.fill)
    assert 0 < sum(flips) < 64
    with pytest.raises(ValueError, match='Unknown data augmentation policy "mosaic"'):
        augment.DetectionPresetTrain("mosaic")
    with pytest.raises(ValueError):
        s.sample([(4, 4)], [], None)


def test_python_input_checks():
    preset = augment.DetectionPresetTrain("hflip", size=(8, 8))
    tg = {"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.int64)}
    ok = torch.zeros(4, 5, 3, dtype=torch.uint8)
    for bad in (ok, [], [ok.float()], [ok.permute(1, 0, 2)], [torch.zeros(3, 4, 5, dtype=torch.uint8)], [ok, "x"]):
        with pytest.raises(ValueError):
            preset(bad, [tg] * (len(bad) if isinstance(bad, list) else 1))
    with pytest.raises(ValueError):
        preset([ok, ok], [tg])
    with pytest.raises(ValueError):
        augment.augment_batch([ok], [], (8, 8))
    with pytest.raises(RuntimeError):          # CPU images: no fallback
        augment.augment_batch([ok], [Params.identity(4, 5)], (8, 8))


# ---------------------------------------------------------------- the tolerance term, measured on the host

@pytest.fixture(scope="module")
def full():
    """the full-chain cases with their float64 references: [(name, images, params, (oh, ow), [(V64, out64)])], computed once"""
    return [(name, imgs, pars, out, [ar.reference(im, p, *out) for im, p in zip(imgs, pars)]) for name, imgs, pars, out in ar.full_cases(Params)]


def test_photometric_tolerance(full):
    """PHOTO_TOL = 4 x the largest |emulate_fp32 - float64 photometric| over the GPU cases' inputs and parameters; the constant in augment_ref.py is
    that measurement and stays under 1e-5."""
    worst = 0.0
    for name, imgs, pars, out, _ in full:
        for im, p in zip(imgs, pars):
            worst = max(worst, float(np.abs(ar.emulate_fp32(im, p).astype(np.float64) - ar.photometric(im, p)).max()))
    print("largest |emulate_fp32 - float64 photometric| = %.3e (PHOTO_MEASURED = %.3e, PHOTO_TOL = %.3e)" % (worst, ar.PHOTO_MEASURED, ar.PHOTO_TOL))
    assert worst <= ar.PHOTO_MEASURED <= 1.05 * worst, worst
    assert ar.PHOTO_TOL == 4.0 * ar.PHOTO_MEASURED and ar.PHOTO_TOL < 1e-5


def test_emulation_stays_inside_the_bound(full):
    for name, imgs, pars, (oh, ow), refs in full:
        for k, (im, p, (v64, want)) in enumerate(zip(imgs, pars, refs)):
            got = ar.emulate_full(im, p, oh, ow).astype(np.float64)
            err, bnd = np.abs(got - want), ar.bound(v64, oh, ow)
            assert err.shape == bnd.shape == (3, oh, ow)
            assert (err <= bnd).all(), (name, k, float((err / bnd).max()))


# ---------------------------------------------------------------- GPU

def _dev(imgs):
    return [torch.from_numpy(np.ascontiguousarray(im)).cuda() for im in imgs]


def _torch_geometry(x, p):
    """u8 [h, w, 3] device tensor -> [3, crop_h, crop_w]: slicing, padding and flip of u8.float() / 255 with torch ops. The quotient is the correctly
    rounded one, computed on the host as the reference's ToTensor computes it (on the device torch divides by a Python scalar by multiplying with
    1 / 255, which differs in the last bit; tests/test_resize.py does the same for dn_forward_u8)."""
    h, w = x.shape[:2]
    v = (x.cpu().float() / 255).to(x.device).permute(2, 0, 1)[list(p.perm)]
    canvas = torch.tensor(p.fill, dtype=torch.float32, device=x.device).view(3, 1, 1).expand(3, p.canvas_h, p.canvas_w).clone()
    canvas[:, p.top:p.top + h, p.left:p.left + w] = v
    crop = canvas[:, p.crop_t:p.crop_t + p.crop_h, p.crop_l:p.crop_l + p.crop_w]
    return crop.flip(-1) if p.flip else crop


GEO_SIZES = [(1, 1), (2, 2), (1, 57), (57, 1), (37, 53)]


def _geo_records(h, w):
    """(canvas, placement, crops): no zoom and a zoom; crops touching each canvas edge, lying wholly in the fill, of one pixel, and the whole canvas"""
    recs = []
    for Hc, Wc, left, top in ((h, w, 0, 0), (h + 7, w + 9, 4, 3)):
        crops = [(0, 0, Wc, Hc), (0, 0, max(Wc // 2, 1), max(Hc // 2, 1)), (Wc - max(Wc // 2, 1), Hc - max(Hc // 2, 1), max(Wc // 2, 1), max(Hc // 2, 1)),
                 (left, top, 1, 1), (left + w - 1, top + h - 1, 1, 1), (0, Hc - 1, Wc, 1), (Wc - 1, 0, 1, Hc)]
        if Hc > h:
            crops += [(0, 0, 4, 3), (Wc - 5, Hc - 4, 5, 4), (0, 0, left, Hc), (left - 1, top - 1, 1, 1), (left + w, top + h, 1, 1)]      # in the fill
            crops += [(left - 1, top - 1, 2, 2), (left + w - 1, top + h - 1, 2, 2)]                                                       # across the image's corners
        recs += [(Hc, Wc, left, top, c) for c in crops]
    return recs


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", GEO_SIZES)
def test_geometry_is_exact(h, w):
    x = _dev([rr.noise_u8(h * 100 + w, 1, h, w)[0]])[0]
    runs = 0
    for Hc, Wc, left, top, (cl, ct, cw, ch) in _geo_records(h, w):
        for flip in (False, True):
            for perm in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
                p = Params(canvas_h=Hc, canvas_w=Wc, left=left, top=top, crop_l=cl, crop_t=ct, crop_w=cw, crop_h=ch, flip=flip, perm=perm,
                           fill=(0.1, 0.9, 0.3) if flip else Params.identity(1, 1).fill)
                got = augment.augment_batch([x], [p], (ch, cw))
                want = _torch_geometry(x, p)
                assert torch.equal(got[0], want), (Hc, Wc, left, top, cl, ct, cw, ch, flip, perm)
                runs += 1
    assert runs >= 7 * 6


@pytest.mark.gpu
def test_geometry_is_exact_nine_sizes_in_one_batch():
    sizes = [(1, 1), (2, 2), (1, 57), (57, 1), (37, 53), (3, 4), (16, 16), (5, 64), (64, 5)]
    xs = _dev([rr.noise_u8(300 + i, 1, h, w)[0] for i, (h, w) in enumerate(sizes)])
    perms = [(0, 1, 2), (2, 1, 0), (1, 2, 0), (0, 2, 1), (1, 0, 2), (2, 0, 1)]
    pars = []
    for i, (h, w) in enumerate(sizes):          # every image under its own canvas; all crops 6 x 7
        Hc, Wc = h + 6 + i, w + 7 + 2 * i
        left, top = i % 5, (2 * i) % 6
        pars.append(Params(canvas_h=Hc, canvas_w=Wc, left=left, top=top, crop_l=(3 * i) % (Wc - 6), crop_t=(5 * i) % (Hc - 5), crop_w=7, crop_h=6,
                           flip=bool(i % 2), perm=perms[i % 6]))
    got = augment.augment_batch(xs, pars, (6, 7))
    for i in range(9):
        assert torch.equal(got[i], _torch_geometry(xs[i], pars[i])), i
    out = torch.empty_like(got)
    assert augment.augment_batch(xs, pars, (6, 7), out=out) is out and torch.equal(out, got)


@pytest.mark.gpu
def test_full_chain_within_the_bound(full):
    for name, imgs, pars, (oh, ow), refs in full:
        got = augment.augment_batch(_dev(imgs), pars, (oh, ow)).cpu().numpy().astype(np.float64)
        assert got.shape == (len(imgs), 3, oh, ow)
        for k, (v64, want) in enumerate(refs):
            err, bnd = np.abs(got[k] - want), ar.bound(v64, oh, ow)
            ratio = float((err / bnd).max())
            print("%s image %d: max err %.3e, max err / bound %.3f" % (name, k, err.max(), ratio))
            assert (err <= bnd).all(), (name, k, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("mutant", ["mean_before_brightness", "permute_fill", "flip_before_crop", "hue_no_mod"])
def test_bound_catches_mutant(mutant):
    """The device result is inside the bound of the reference and OUTSIDE the bound of the reference with one mistake."""
    h, w, oh, ow = 37, 53, 24, 40
    im = rr.noise_u8(100, 1, h, w)[0]
    p = dict(ar.chain_params(Params, h, w))["all-before"]
    got = augment.augment_batch(_dev([im]), [p], (oh, ow))[0].cpu().numpy().astype(np.float64)
    v64, want = ar.reference(im, p, oh, ow)
    assert (np.abs(got - want) <= ar.bound(v64, oh, ow)).all()
    mv64, mwant = ar.reference(im, p, oh, ow, **{mutant: True})
    over = np.abs(got - mwant) > ar.bound(mv64, oh, ow)
    print("%s: %d of %d elements outside the mutant's bound" % (mutant, int(over.sum()), over.size))
    assert over.any()


@pytest.mark.gpu
def test_two_calls_are_bit_identical():
    h, w = 375, 500
    im = _dev([rr.noise_u8(102, 1, h, w)[0], rr.noise_u8(103, 1, 97, 131)[0]])
    named = dict(ar.chain_params(Params, h, w))
    pars = [named["all-after"], dict(ar.chain_params(Params, 97, 131))["all-before"]]
    a = augment.augment_batch(im, pars, (320, 320)).clone()
    b = augment.augment_batch(im, pars, (320, 320))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _raw_call(L, ptrs, sizes, rec, n, oh, ow, out, ws, ws_bytes):
    as_i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
    return L.dn_augment_batch(ptrs, as_i32(sizes), as_i32(rec), n, oh, ow, C.c_void_p(out) if out else None, C.c_void_p(ws) if ws else None, ws_bytes,
                              C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.gpu
def test_invalid_records_are_refused_before_any_launch():
    L = _lib.lib()
    h, w, oh, ow = 5, 6, 4, 4
    x = _dev([rr.noise_u8(1, 1, h, w)[0]] * 2)
    good = Params(canvas_h=9, canvas_w=10, left=2, top=1, crop_l=1, crop_t=1, crop_w=6, crop_h=5, contrast=1.2)
    out = torch.full((2, 3, oh, ow), -7.0, device="cuda")
    ws_bytes = L.dn_augment_workspace_bytes(2)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
    ptrs = (C.c_void_p * 2)(x[0].data_ptr(), x[1].data_ptr())
    sizes = np.array([[h, w], [h, w]], dtype=np.int32)
    rec = augment.pack([good, good])
    base = dict(ptrs=ptrs, sizes=sizes, rec=rec, n=2, oh=oh, ow=ow, out=out.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws_bytes)

    def word(i, v, image=1):
        r = rec.copy()
        if isinstance(v, float):
            r.view(np.float32)[image, i] = v
        else:
            r[image, i] = v
        return dict(rec=r)

    bad = {
        "null images": dict(ptrs=None), "null image 1": dict(ptrs=(C.c_void_p * 2)(x[0].data_ptr(), None)), "null sizes": dict(sizes=None),
        "null params": dict(rec=None), "null out": dict(out=0), "null workspace": dict(ws=0), "n = 0": dict(n=0), "n < 0": dict(n=-1),
        "out_h = 0": dict(oh=0), "out_w < 0": dict(ow=-3), "h = 0": dict(sizes=np.array([[h, w], [0, w]], dtype=np.int32)),
        "w < 0": dict(sizes=np.array([[h, -w], [h, w]], dtype=np.int32)),
        "crop right of the canvas": word(augment.CROP_L, 5), "crop below the canvas": word(augment.CROP_H, 9), "crop_l < 0": word(augment.CROP_L, -1),
        "crop_t < 0": word(augment.CROP_T, -1), "crop_w = 0": word(augment.CROP_W, 0), "crop_h < 0": word(augment.CROP_H, -2, image=0),
        "image right of the canvas": word(augment.LEFT, 5), "image below the canvas": word(augment.TOP, 5), "left < 0": word(augment.LEFT, -1),
        "top < 0": word(augment.TOP, -1, image=0), "canvas smaller than the image": word(augment.CANVAS_W, 5),
        "perm repeats": word(augment.PERM + 1, 0), "perm out of range": word(augment.PERM + 2, 3), "perm negative": word(augment.PERM, -1),
        "brightness NaN": word(augment.BRIGHTNESS, float("nan")), "contrast inf": word(augment.CONTRAST, float("inf")),
        "saturation -inf": word(augment.SATURATION, float("-inf"), image=0), "hue NaN": word(augment.HUE, float("nan")),
        "fill NaN": word(augment.FILL + 2, float("nan")), "unknown flag": word(augment.FLAGS, 64),
        "workspace too small": dict(ws_bytes=ws_bytes - 1), "workspace of 0": dict(ws_bytes=0),
    }
    assert _raw_call(L, **base) == 0
    torch.cuda.synchronize()
    assert bool((out != -7.0).all())
    for name, change in bad.items():
        out.fill_(-7.0)
        rc = _raw_call(L, **{**base, **change})
        torch.cuda.synchronize()
        assert rc == -1, (name, rc, L.dn_last_error())          # DN_E_INVALID
        assert bool((out == -7.0).all()), name
    # through the Python surface the refusal is a RuntimeError with the library's text
    with pytest.raises(RuntimeError, match="crop"):
        augment.augment_batch(x[:1], [Params(canvas_h=h, canvas_w=w, crop_l=1, crop_t=0, crop_w=w, crop_h=h)], (oh, ow))


@pytest.mark.gpu
def test_preset_feeds_the_loss():
    from demonet_amd import models
    m = models.load_synthetic(models.ssdlite320_mobilenet_v3_large(num_classes=21), 0).cuda()
    sizes = [(375, 500), (333, 500), (480, 360), (97, 131)]
    imgs = _dev([rr.noise_u8(400 + i, 1, h, w)[0] for i, (h, w) in enumerate(sizes)])
    rng = np.random.RandomState(5)
    targets = []
    for (h, w), gcount in zip(sizes, (3, 1, 4, 2)):
        xy = rng.uniform(0, 0.5, (gcount, 2)).astype(np.float32) * np.array([w, h], dtype=np.float32)
        wh = rng.uniform(0.2, 0.5, (gcount, 2)).astype(np.float32) * np.array([w, h], dtype=np.float32)
        targets.append({"boxes": torch.from_numpy(np.concatenate([xy, xy + wh], 1)).cuda(), "labels": torch.from_numpy(rng.randint(1, 21, (gcount,)).astype(np.int64)).cuda()})
    preset = m.train_preset()
    assert preset.size == (320, 320)
    batch, tg = preset(imgs, targets, generator=torch.Generator().manual_seed(21))
    assert batch.shape == (4, 3, 320, 320) and batch.dtype == torch.float32 and batch.is_cuda
    assert all(t["boxes"].is_cuda and t["labels"].is_cuda and t["boxes"].shape[0] == t["labels"].shape[0] >= 1 for t in tg)
    got = m.loss(batch, tg)
    assert all(bool(torch.isfinite(v)) for v in got.values())
    # the same records from the same seed, applied by augment_ref
    pars, _ = preset.sampler.sample(sizes, targets, torch.Generator().manual_seed(21))
    assert any(p.flags() & 15 for p in pars) and any((p.crop_h, p.crop_w) != s for p, s in zip(pars, sizes))
    ref = np.stack([ar.reference(im.cpu().numpy(), p, 320, 320)[1] for im, p in zip(imgs, pars)]).astype(np.float32)
    ref_t = []
    for t, p in zip(targets, pars):
        b, lab = ar.boxes_ref(t["boxes"].cpu().numpy(), t["labels"].cpu().numpy(), p, (320, 320))
        ref_t.append({"boxes": torch.from_numpy(b).cuda(), "labels": torch.from_numpy(lab).cuda()})
    for a, b in zip(tg, ref_t):
        assert torch.equal(a["boxes"], b["boxes"]) and torch.equal(a["labels"], b["labels"])
    want = m.loss(torch.from_numpy(ref).cuda(), ref_t)
    for k in want:
        print("%s: preset %.7f reference %.7f" % (k, got[k].item(), want[k].item()))
        assert abs(got[k].item() - want[k].item()) <= LOSS_RTOL * abs(want[k].item()) + 1e-7, k
    # ... and the whole input side of a fine-tuning step
    m.train_heads()
    losses = m.loss(*preset(imgs, targets, generator=torch.Generator().manual_seed(21)))
    (losses["bbox_regression"] + losses["classification"]).backward()
    for k, prm in m.head_parameters().items():
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), k
