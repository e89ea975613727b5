"""The first post-process step (csrc/post_math.h: softmax over the classes, decode + clip) where the synthetic heads never take it:
regressions past the log(1000/16) clamp, box centres far outside the image, logit gaps down to the cut of pp_exp_nonpos at -103.28 and
past it. dn_postprocess is called directly, under both DN_PP_FAST settings.

n = 2 images, K = 3 classes, A = 256 pairwise disjoint anchors on a 16 x 16 grid; score threshold 0, NMS threshold 1 (no IoU exceeds it),
top-k = A per class and detections_per_img = 2 A = 512: every (anchor, foreground class) with a positive score is kept, and a score of
exactly 0 never is a candidate (include/demonet_hip.h)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ssd_oracle as so
from demonet_amd import _lib, synth

pytestmark = pytest.mark.gpu

N, K, GRID = 2, 3, 16
A = GRID * GRID
TOPK, DETS = A, 2 * A
F32 = np.float32
CLIP32 = F32(math.log(1000.0 / 16.0))                   # PP_BBOX_XFORM_CLIP as the kernels hold it
EXP_CLIP32 = F32(math.exp(float(CLIP32)))               # fl32(exp(fl32(log(1000/16))))
TINY = 2.0 ** -126                                      # smallest normal float


@pytest.fixture(params=["1", "0"], ids=["cutoff-fast-path", "full-path"])
def pp_fast(request, monkeypatch):
    monkeypatch.setenv("DN_PP_FAST", request.param)
    return request.param


def _anchors(origin, pitch, w, h):
    """[A, 4] float32: a w x h box in every cell of a GRID x GRID grid of `pitch` pixels (w, h < pitch: pairwise disjoint)"""
    assert w < pitch and h < pitch
    iy, ix = np.divmod(np.arange(A), GRID)
    x0, y0 = origin + pitch * ix, origin + pitch * iy
    return np.stack([x0, y0, x0 + w, y0 + h], 1).astype(F32)


def _postprocess(logits, reg, anchors, hw):
    L = _lib.lib()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    lg, rg, an = dev(logits), dev(reg), dev(anchors)
    ws = torch.empty(L.dn_postprocess_workspace_bytes(N, A, K, TOPK, DETS), dtype=torch.uint8, device="cuda")
    boxes = torch.empty(N, DETS, 4, device="cuda")
    scores = torch.empty(N, DETS, device="cuda")
    labels = torch.empty(N, DETS, dtype=torch.int64, device="cuda")
    counts = torch.empty(N, dtype=torch.int32, device="cuda")
    kept = torch.empty(N, DETS, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = L.dn_postprocess(p(lg), p(rg), p(an), N, A, K, float(hw[0]), float(hw[1]), None, 0.0, 1.0, TOPK, DETS,
                          p(boxes), p(scores), p(labels), p(counts), p(kept), p(ws), ws.numel(),
                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "dn_postprocess")
    torch.cuda.synchronize()
    return boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy(), counts.cpu().numpy(), kept.cpu().numpy()


def _by_anchor(b, l, c, k):
    """[N, K - 1, A, 4] boxes by (image, foreground label, anchor); asserts that every anchor was kept once per label"""
    out = np.full((N, K - 1, A, 4), np.nan, dtype=F32)
    for i in range(N):
        assert int(c[i]) == DETS, f"image {i}: {int(c[i])} of {DETS} (anchor, class) pairs kept"
        for lab in range(1, K):
            sel = l[i] == lab
            assert np.array_equal(np.sort(k[i][sel]), np.arange(A)), f"image {i} label {lab}: not every anchor kept"
            out[i, lab - 1, k[i][sel]] = b[i][sel]
    return out


def _mild_logits(seed):
    return (synth.normal(seed, "post_extremes.logits", N * A * K) * F32(2.0)).reshape(N, A, K)


def test_the_clamp_is_a_clamp_exactly(pp_fast):
    """dw = min(reg[2] / 5, clip): rows whose reg[2] is 25, 1e4, 3e38 or +inf decode to the same bits, and so for reg[3] and for both. Image 1
    holds the same rows as image 0 with the next of the four values: the two images' boxes are equal bit for bit. Where reg[:2] is 0 the
    clamped extent is the closed form of post_math.h in float32: pcx = 0 * w + cx, pw = fl32(exp(clip)) * w, x = pcx -+ 0.5 * pw."""
    big = np.array([25.0, 1e4, 3e38, np.inf], dtype=F32)
    anchors = _anchors(4096.0, 64.0, 8.0, 16.0)
    hw = (16384.0, 16384.0)                                   # 62.5 x 16 = 1000 pixels at most: no box reaches a border
    a = np.arange(A)
    mode = (a // 4) % 3                                       # 0: reg[2] clamped, 1: reg[3], 2: both
    centred = (a // 12) % 2 == 0
    reg = np.zeros((N, A, 4), dtype=F32)
    shift = (synth.normal(5, "post_extremes.shift", A * 2) * F32(3.0)).reshape(A, 2)
    shift[centred] = 0.0
    for i in range(N):
        v = big[(a + i) % 4]
        reg[i, :, :2] = shift
        reg[i, :, 2] = np.where(mode != 1, v, F32(1.0))
        reg[i, :, 3] = np.where(mode != 0, v, F32(-2.0))
    b, s, l, c, k = _postprocess(_mild_logits(3), reg, anchors, hw)
    box = _by_anchor(b, l, c, k)
    assert np.isfinite(box).all()
    assert np.array_equal(box[0].view(np.uint32), box[1].view(np.uint32)), "the four values past the clamp decode to different bits"
    assert np.array_equal(box[:, 0].view(np.uint32), box[:, 1].view(np.uint32)), "the two labels of an anchor carry different boxes"
    w, h = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
    cx, cy = anchors[:, 0] + F32(0.5) * w, anchors[:, 1] + F32(0.5) * h
    pcx, pcy = F32(0.0) * w + cx, F32(0.0) * h + cy
    pw, ph = EXP_CLIP32 * w, EXP_CLIP32 * h
    assert pw.dtype == F32 and float(EXP_CLIP32) == pytest.approx(62.5, rel=1e-6)
    want = np.stack([pcx - F32(0.5) * pw, pcy - F32(0.5) * ph, pcx + F32(0.5) * pw, pcy + F32(0.5) * ph], 1)
    assert (want > 0).all() and (want < hw[0]).all()
    got = box[0, 0]
    xs, ys = centred & (mode != 1), centred & (mode != 0)
    assert xs.sum() >= 40 and ys.sum() >= 40
    assert np.array_equal(got[xs][:, 0::2].view(np.uint32), want[xs][:, 0::2].view(np.uint32)), \
        f"clamped width: got {got[xs][0, 0::2]!r}, closed form {want[xs][0, 0::2]!r}"
    assert np.array_equal(got[ys][:, 1::2].view(np.uint32), want[ys][:, 1::2].view(np.uint32)), \
        f"clamped height: got {got[ys][0, 1::2]!r}, closed form {want[ys][0, 1::2]!r}"
    # the clamp widens nothing below it: reg = 20 (dw = 4.0 < clip) gives a narrower box, the unclamped extents are the mild ones
    assert np.allclose(got[mode == 0][:, 3] - got[mode == 0][:, 1], math.exp(-0.4) * 16.0, rtol=0, atol=2e-3)       # (coordinates near 5000: ulp 5e-4)
    assert np.allclose(got[mode == 1][:, 2] - got[mode == 1][:, 0], math.exp(0.2) * 8.0, rtol=0, atol=2e-3)
    reg20 = reg.copy()
    reg20[:, :, 2] = 20.0
    b2, _, l2, c2, k2 = _postprocess(_mild_logits(3), reg20, anchors, hw)
    w20 = _by_anchor(b2, l2, c2, k2)[0, 0]
    assert np.allclose(w20[:, 2] - w20[:, 0], math.exp(4.0) * 8.0, rtol=1e-5, atol=2e-3) and ((w20[:, 2] - w20[:, 0]) < pw).all()


def test_boxes_far_outside_and_past_the_clamp_against_the_oracle(pp_fast):
    """reg[:2] ~ N(0, 30): centres up to hundreds of pixels outside a 320 x 320 image, boxes clipped to zero area at the border;
    reg[2:] ~ N(0, 15): dw, dh from exp(-9) to past the clamp. Against the oracle's decode in float64, at the tolerances the golden boxes
    are held to; the expected boxes are gathered by the device's kept indices, which equal the oracle's."""
    anchors = _anchors(2.0, 20.0, 12.0, 10.0)
    hw = (320.0, 320.0)
    reg = np.concatenate([(synth.normal(7, "post_extremes.ctr", N * A * 2) * F32(30.0)).reshape(N, A, 2),
                          (synth.normal(7, "post_extremes.size", N * A * 2) * F32(15.0)).reshape(N, A, 2)], 2).astype(F32)
    logits = _mild_logits(9)
    ref = so.postprocess_detections(torch.from_numpy(logits).double(), torch.from_numpy(reg).double(), torch.from_numpy(anchors).double(),
                                    hw, 0.0, 1.0, DETS, TOPK, return_intermediates=True)
    b, s, l, c, k = _postprocess(logits, reg, anchors, hw)
    _by_anchor(b, l, c, k)                                    # every anchor kept
    assert ((reg[..., 2:] / 5 > float(CLIP32)).mean() > 0.05)
    for i, d in enumerate(ref):
        dec = d["decoded"]
        area = (dec[:, 2] - dec[:, 0]) * (dec[:, 3] - dec[:, 1])
        assert (area == 0).sum() >= 10 and (area > 0).sum() >= 100, "the case must hold boxes clipped away and boxes left"
        assert d["anchor_idx"].shape[0] == DETS
        got_pairs = sorted(zip(l[i].tolist(), k[i].tolist()))
        assert got_pairs == sorted(zip(d["labels"].tolist(), d["anchor_idx"].tolist()))
        sc = d["scores"].astype(np.float64)
        if ((sc[:-1] - sc[1:]) / sc[:-1]).min() > 1e-5:      # no two adjacent scores within the softmax tolerance: the order is decided
            assert np.array_equal(k[i], d["anchor_idx"]) and np.array_equal(l[i], d["labels"])
        np.testing.assert_allclose(b[i], dec[k[i]], rtol=1e-5, atol=2e-3)
        assert (b[i] >= 0).all() and (b[i] <= 320).all()


def test_scores_down_to_the_exp_cut_and_below(pp_fast):
    """Logits x 30 (gaps to -200) and rows at the edges of pp_exp_nonpos: equal logits, one +80 among -80s, a gap straddling the cut at
    -103.28, gaps in [-103, -88] whose exponentials are fp32 subnormals. Against a float64 softmax at rtol 1e-5, atol 1e-7. A score below the
    float range is exactly 0 (then it is no candidate) or a subnormal; none is negative or NaN."""
    logits = (synth.normal(13, "post_extremes.hot", N * A * K) * F32(30.0)).reshape(N, A, K)
    u = synth.uniform(13, "post_extremes.sub", 2 * 64).reshape(64, 2)
    for i in range(N):
        logits[i, 0] = (7.0, 7.0, 7.0)
        logits[i, 1] = (-80.0, 80.0, -80.0)
        logits[i, 2] = (-80.0, -80.0, 80.0)
        logits[i, 3] = (80.0, -80.0, -80.0)
        logits[i, 4] = (0.0, -103.2, -103.4)
        logits[i, 5] = (-103.4, 0.0, -103.2)
        logits[i, 6] = (50.0, 50.0 - 103.2, 50.0 - 103.4)
        logits[i, 8:72, 0] = 0.0
        logits[i, 8:72, 1:] = -88.0 - 15.0 * u
    logits[1, 8:72] = logits[1, 8:72][:, [1, 0, 2]]          # (the maximum on a foreground class)
    logits = logits.astype(F32)
    x = logits.astype(np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    want = e / e.sum(-1, keepdims=True)
    assert (x.min(-1) - x.max(-1)).min() < -150 and ((want[..., 1:] > 0) & (want[..., 1:] < TINY)).sum() >= 64
    anchors = _anchors(2.0, 20.0, 12.0, 10.0)
    reg = np.zeros((N, A, 4), dtype=F32)
    b, s, l, c, k = _postprocess(logits, reg, anchors, (320.0, 320.0))
    seen_sub = 0
    for i in range(N):
        cnt = int(c[i])
        si, li, ki = s[i, :cnt], l[i, :cnt], k[i, :cnt]
        assert not np.isnan(s[i]).any() and (s[i] >= 0).all() and (si > 0).all() and (s[i, cnt:] == 0).all()
        assert ((li >= 1) & (li < K)).all() and ((ki >= 0) & (ki < A)).all()
        got = np.zeros((A, K), dtype=np.float64)
        hit = np.zeros((A, K), dtype=bool)
        got[ki, li] = si
        hit[ki, li] = True
        assert hit.sum() == cnt, "an (anchor, class) pair was reported twice"
        w = want[i]
        np.testing.assert_allclose(got[:, 1:], w[:, 1:], rtol=1e-5, atol=1e-7)
        # a pair that is no candidate has a score of exactly 0 on the device: only a value below the float range may become that
        assert (w[:, 1:][~hit[:, 1:]] < TINY).all(), float(w[:, 1:][~hit[:, 1:]].max())
        # ... and a value below the float range is 0 or a subnormal
        below = w[:, 1:] < TINY
        assert (got[:, 1:][below] < TINY).all()
        seen_sub += int(((got[:, 1:] > 0) & (got[:, 1:] < TINY)).sum())
        # the rows set by hand
        assert got[0, 1] == got[0, 2] and abs(got[0, 1] - 1.0 / 3.0) < 1e-7
        assert got[1, 1] == 1.0 and not hit[1, 2] and got[2, 2] == 1.0 and not hit[2, 1] and not hit[3, 1] and not hit[3, 2]
        assert got[4, 2] <= got[4, 1] < 2e-45 and got[5, 1] == 1.0 and got[6, 2] <= got[6, 1] < 2e-45      # (either side of the cut: 0 or the smallest subnormal)
    print(f"\nsubnormal scores reported: {seen_sub}")
