"""Soft-NMS as a post-process mode (dn_postprocess_soft, dn_set_nms, SSD.set_nms): the CPU part checks the ABI, the argument handling and
the verifier of tests/soft_nms_ref.py itself; the GPU part (-m gpu) holds the kernel to that verifier on every case, to bit-identical
repeats, to the hard path where the two must coincide, and the models' forwards to the stand-alone entry point bit for bit."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import post_select_ref as psr
import soft_nms_ref as sr
import ssd_oracle as so
from demonet_amd import _lib, models, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARD, LINEAR, GAUSSIAN = 0, 1, 2
METHOD = {"linear": LINEAR, "gaussian": GAUSSIAN}
NMS_THRESH, SIGMA = 0.5, 0.5

# (n, A, K, topk, dets, score_thresh)
OP_CASES = [
    (2, 200, 3, 64, 100, 0.01),
    (1, 700, 5, 300, 300, 0.001),       # the merge truncates
    (1, 1500, 2, 512, 512, 0.0005),     # candidate capacity
    (2, 500, 7, 40, 30, 0.05),
    (1, 128, 4, 100, 50, 0.9999),       # empty
    (1, 64, 300, 16, 64, 0.0),          # wide merge (more than 256 foreground classes)
    (11, 640, 6, 80, 40, 0.03),         # XCD mapping
]
# the shapes on which the float32 restatement was compared with float64 on the CPU (and the verifier is tested without a GPU)
CPU_CASES = [OP_CASES[0], OP_CASES[3]]


@functools.lru_cache(maxsize=None)
def _inputs(n, A, K):
    """Random inputs as tests/test_gpu_model.py::test_postprocess_random_vs_oracle generates them: duplicated rows (exact score ties) and
    duplicated anchors (identical boxes) included."""
    rng = np.random.default_rng(A * 7 + K)
    logits = rng.normal(0, 2.0, (n, A, K)).astype(np.float32)
    reg = rng.normal(0, 1.0, (n, A, 4)).astype(np.float32)
    ctr = rng.uniform(20, 300, (A, 2)).astype(np.float32)
    wh = rng.uniform(10, 120, (A, 2)).astype(np.float32)
    anchors = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)
    dup = rng.integers(0, A, A // 5)
    src = rng.integers(0, A, A // 5)
    logits[:, dup] = logits[:, src]
    reg[:, dup] = reg[:, src]
    anchors[dup[: len(dup) // 2]] = anchors[src[: len(dup) // 2]]
    return logits, reg, anchors


@functools.lru_cache(maxsize=None)
def _intermediates(n, A, K):
    """The reference's softmax scores [A, K] and decoded, clipped boxes [A, 4] per image (they do not depend on the selection settings)."""
    logits, reg, anchors = _inputs(n, A, K)
    d = so.postprocess_detections(torch.from_numpy(logits), torch.from_numpy(reg), torch.from_numpy(anchors), (320, 320), 0.5, 0.5, 1, 1,
                                  return_intermediates=True)
    return [(x["softmax"], x["decoded"]) for x in d]


def _lattice_inputs():
    """The exact-equality case: 12 x 12 square anchors of side 1.5 x pitch on a lattice (neighbours: IoU 0.2, diagonal 0.06) and 40 duplicated
    rows (IoU exactly 1), zero regression: every same-class pair has IoU <= nms_thresh or is an exact duplicate."""
    rng = np.random.default_rng(5)
    pitch, side, g = 24.0, 36.0, 12
    cy, cx = np.meshgrid(30.0 + pitch * np.arange(g), 30.0 + pitch * np.arange(g), indexing="ij")
    ctr = np.stack([cx.ravel(), cy.ravel()], 1)
    anchors = np.concatenate([ctr - side / 2, ctr + side / 2], 1).astype(np.float32)
    A0, ndup, K = g * g, 40, 4
    logits = rng.normal(0, 2.0, (2, A0, K)).astype(np.float32)
    src = rng.integers(0, A0, ndup)
    anchors = np.concatenate([anchors, anchors[src]], 0)
    logits = np.concatenate([logits, logits[:, src]], 1)
    perm = rng.permutation(A0 + ndup)
    anchors, logits = np.ascontiguousarray(anchors[perm]), np.ascontiguousarray(logits[:, perm])
    reg = np.zeros((2, A0 + ndup, 4), np.float32)
    return logits, reg, anchors


def _declared_symbols():
    txt = open(os.path.join(ROOT, "include", "demonet_hip.h")).read()
    return set(re.findall(r"DN_API\s+[\w\s\*]+?\b(dn_\w+)\s*\(", txt)), txt


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_soft_nms_entry_points():
    syms, txt = _declared_symbols()
    for name in ("dn_set_nms", "dn_postprocess_soft"):
        assert name in syms, name + " not declared in demonet_hip.h"
        assert name in _lib.EXPORTS, name + " not bound in _lib.py"
    if os.path.exists(_lib.LIB_PATH):
        L = C.CDLL(_lib.LIB_PATH)
        assert hasattr(L, "dn_set_nms") and hasattr(L, "dn_postprocess_soft")
    m = re.search(r"enum\s*\{\s*DN_NMS_HARD\s*=\s*0\s*,\s*DN_NMS_SOFT_LINEAR\s*=\s*1\s*,\s*DN_NMS_SOFT_GAUSSIAN\s*=\s*2\s*\}", txt)
    assert m, "the DN_NMS_* enum is missing from the header"
    assert _lib.DN_NMS == dict(hard=HARD, linear=LINEAR, gaussian=GAUSSIAN)
    assert "#define DN_ABI_VERSION 1" in txt
    # dn_postprocess_soft = dn_postprocess's signature with (int, float) behind nms_thresh
    base, soft = _lib._SIGNATURES["dn_postprocess"], _lib._SIGNATURES["dn_postprocess_soft"]
    assert soft[0] is base[0] and soft[1] == base[1][:11] + [C.c_int, C.c_float] + base[1][11:]


def test_set_nms_validates_and_round_trips_without_a_gpu():
    m = models.ssdlite320_mobilenet_v3_large(num_classes=5)
    assert (m.nms_method, m.nms_sigma) == ("hard", 0.5)
    gen = m._plan_gen
    assert m.set_nms("gaussian", sigma=0.3) is m
    assert (m.nms_method, m.nms_sigma) == ("gaussian", 0.3)
    assert m.set_nms("linear") is m and (m.nms_method, m.nms_sigma) == ("linear", 0.5)
    for bad in (dict(method="soft"), dict(method=1), dict(method=None), dict(method=["linear"]), dict(method="gaussian", sigma=0.0), dict(method="gaussian", sigma=-1.0),
                dict(method="gaussian", sigma=float("nan")), dict(method="gaussian", sigma=float("inf")), dict(method="linear", sigma="x")):
        with pytest.raises(ValueError):
            m.set_nms(**bad)
    assert (m.nms_method, m.nms_sigma) == ("linear", 0.5), "a rejected call must leave the setting alone"
    assert m.set_nms("hard").nms_method == "hard"
    assert m._plan_gen == gen and m._handle is None


def _restated(case, method, sigma=SIGMA, dtype=np.float32):
    n, A, K, topk, dets, st = case
    return [sr.soft_nms_image(sm, dec, method, NMS_THRESH, sigma, st, topk, dets, dtype) for sm, dec in _intermediates(n, A, K)]


@pytest.mark.parametrize("method", sr.METHODS)
@pytest.mark.parametrize("case", CPU_CASES, ids=str)
def test_verifier_accepts_the_float32_restatement_and_rejects_corrupted_ones(case, method):
    n, A, K, topk, dets, st = case
    args = (method, NMS_THRESH, SIGMA, st, topk, dets)
    inter = _intermediates(n, A, K)
    f32 = _restated(case, method)
    worst = dict(pick=0.0, score=0.0)
    for (out, _), (sm, dec) in zip(f32, inter):
        w = sr.verify_image(out, sm, dec, *args)
        worst = {k: max(worst[k], w[k]) for k in worst}
    print("float32 restatement %s %s: worst pick ratio %.3f, worst |got - ref| / bound %.3f" % (case, method, worst["pick"], worst["score"]))
    assert worst["pick"] <= 1 and worst["score"] <= 1
    (b, s, l, cnt, k), (sm, dec) = f32[0][0], inter[0]
    assert cnt >= 8
    # one score scaled by 1 + 1e-4 (a decayed one: far beyond any bound here)
    s2 = s.copy()
    s2[cnt // 2] *= np.float32(1 + 1e-4)
    with pytest.raises(AssertionError):
        sr.verify_image((b, s2, l, cnt, k), sm, dec, *args)
    # two emitted anchors of one class swapped across a large gap: the first and the last detection of the most frequent label
    lab = np.bincount(l[:cnt]).argmax()
    rows = np.nonzero(l[:cnt] == lab)[0]
    i, j = rows[0], rows[-1]
    assert s[i] > 1.05 * s[j], "the corrupted pair must be far apart (the bounds are below 1e-4)"
    k2, b2 = k.copy(), b.copy()
    k2[[i, j]] = k[[j, i]]
    b2[[i, j]] = b[[j, i]]
    with pytest.raises(AssertionError):
        sr.verify_image((b2, s, l, cnt, k2), sm, dec, *args)
    # a dropped detection (count one short): the candidate was never emitted although its score is above the threshold
    if cnt < dets:
        b3, s3, l3, k3 = b.copy(), s.copy(), l.copy(), k.copy()
        b3[cnt - 1] = 0; s3[cnt - 1] = 0; l3[cnt - 1] = 0; k3[cnt - 1] = -1
        if s[cnt - 1] > 1.01 * st:
            with pytest.raises(AssertionError):
                sr.verify_image((b3, s3, l3, cnt - 1, k3), sm, dec, *args)


def test_float32_restatement_agrees_with_the_float64_oracle_where_it_is_unambiguous():
    for case in CPU_CASES:
        for method in sr.METHODS:
            for (o32, _), (o64, info) in zip(_restated(case, method), _restated(case, method, dtype=np.float64)):
                if sr.order_is_unambiguous(info):
                    assert o32[3] == o64[3] and np.array_equal(o32[2], o64[2]) and np.array_equal(o32[4], o64[4])


def test_lattice_input_meets_the_condition_of_the_exact_equality_case():
    logits, reg, anchors = _lattice_inputs()
    d = so.postprocess_detections(torch.from_numpy(logits), torch.from_numpy(reg), torch.from_numpy(anchors), (320, 320), 0.0, NMS_THRESH, 1, 1,
                                  return_intermediates=True)
    for x in d:
        dec = x["decoded"]
        ar = sr.areas_of(dec)
        dups = 0
        for i in range(dec.shape[0]):
            u = sr.iou_row(dec[i], ar[i], dec, ar)
            assert ((u <= np.float32(NMS_THRESH)) | (u == 1)).all()
            dups += int((u == 1).sum()) - 1
        assert dups >= 40, "the case needs exact duplicates"      # hence: linear decay only ever multiplies by 1 or by 0, and soft == hard


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU, op level
# ------------------------------------------------------------------------------------------------------------------------------------
def _post_soft(logits, reg, anchors, st, nt, method, sigma, topk, dets, ws_bytes=None, hard_entry=False, want_inputs=False):
    """dn_postprocess_soft (hard_entry: dn_postprocess) on device tensors; returns (rc, numpy outputs)."""
    L = _lib.lib()
    n, A, K = logits.shape
    need = L.dn_postprocess_workspace_bytes(n, A, K, topk, dets)
    ws = torch.empty(need if ws_bytes is None else ws_bytes, dtype=torch.uint8, device="cuda")
    boxes = torch.full((n, dets, 4), -7.0, device="cuda")
    scores = torch.full((n, dets), -7.0, device="cuda")
    labels = torch.full((n, dets), -7, dtype=torch.int64, device="cuda")
    counts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    kept = torch.full((n, dets), -7, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if hard_entry:
        rc = L.dn_postprocess(p(logits), p(reg), p(anchors), n, A, K, 320.0, 320.0, None, float(st), float(nt), int(topk), int(dets),
                              p(boxes), p(scores), p(labels), p(counts), p(kept), p(ws), ws.numel(), stream)
    else:
        rc = L.dn_postprocess_soft(p(logits), p(reg), p(anchors), n, A, K, 320.0, 320.0, None, float(st), float(nt), int(method), float(sigma),
                                   int(topk), int(dets), p(boxes), p(scores), p(labels), p(counts), p(kept), p(ws), ws.numel(), stream)
    torch.cuda.synchronize()
    outs = tuple(t.cpu().numpy() for t in (boxes, scores, labels, counts, kept))
    if not want_inputs or rc != 0:
        return rc, outs
    # what the reduce worked on, left behind in the workspace, in the oracle's form: softmax [A, K] (background column unused), boxes [A, 4]
    # (tests/post_select_ref.py holds the one Python copy of csrc/postprocess.hip's post_buffers)
    return rc, outs, psr.read_workspace(ws.cpu().numpy(), n, A, K, topk)["inter"]


def _check_case(case, method, sigma):
    """The verifier replays the kernel's output on the scores and boxes the kernel itself selected from: the device's softmax and decode agree with
    the oracle's to an ulp or two (asserted here at the tolerance of test_postprocess_random_vs_oracle), not bit for bit, and the verifier's
    bounds cover the reduce alone -- its exact checks (boxes, untouched scores) and B = 0 bounds need the reduce's true inputs."""
    n, A, K, topk, dets, st = case
    logits, reg, anchors = (torch.from_numpy(x).cuda() for x in _inputs(n, A, K))
    rc, got, device_inter = _post_soft(logits, reg, anchors, st, NMS_THRESH, METHOD[method], sigma, topk, dets, want_inputs=True)
    _lib.check(rc, "dn_postprocess_soft")
    for (sm, dec), (rsm, rdec) in zip(device_inter, _intermediates(n, A, K)):
        np.testing.assert_allclose(sm[:, 1:], rsm[:, 1:], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(dec, rdec, rtol=1e-5, atol=2e-3)
    rc, again = _post_soft(logits, reg, anchors, st, NMS_THRESH, METHOD[method], sigma, topk, dets)
    _lib.check(rc, "dn_postprocess_soft")
    for x, y in zip(got, again):
        assert np.array_equal(x, y), "two calls must agree bit for bit"
    worst = dict(pick=0.0, score=0.0)
    outright = 0
    total = 0
    for i, (sm, dec) in enumerate(device_inter):
        out = tuple(x[i] for x in got)
        w = sr.verify_image(out, sm, dec, method, NMS_THRESH, sigma, st, topk, dets)
        worst = {k: max(worst[k], w[k]) for k in worst}
        ref, info = sr.soft_nms_image(sm, dec, method, NMS_THRESH, sigma, st, topk, dets)
        total += int(out[3])
        if sr.order_is_unambiguous(info):
            outright += 1
            assert int(out[3]) == ref[3]
            assert np.array_equal(out[2], ref[2]), "labels differ from the oracle's although no decision is ambiguous"
            assert np.array_equal(out[4], ref[4]), "anchors differ from the oracle's although no decision is ambiguous"
    print("soft-NMS case %s %s sigma %.2f: %d detections, worst pick ratio %.3f, worst |got - ref| / bound %.3f, %d of %d images compared outright"
          % (case, method, sigma, total, worst["pick"], worst["score"], outright, n))
    return total, outright


@pytest.mark.gpu
@pytest.mark.parametrize("method", sr.METHODS)
@pytest.mark.parametrize("case", OP_CASES, ids=str)
def test_soft_postprocess_against_the_replay_verifier(case, method):
    total, outright = _check_case(case, method, SIGMA)
    assert (total == 0) == (case[5] > 0.99), "only the empty case may come back empty"
    if case == OP_CASES[0] and method == "linear":
        # the comparison with the oracle's own anchor sequence must not be vacuous: on this case no decision of either image is within reach
        # of fp32 rounding (the exact ties of its duplicated rows are untouched scores, which both sides resolve by anchor)
        assert outright == case[0], "the outright comparison with the oracle ran on %d of %d images" % (outright, case[0])


@pytest.mark.gpu
def test_soft_postprocess_gaussian_with_a_narrow_sigma_drops_many():
    case = OP_CASES[1]
    n, A, K, topk, dets, st = case
    _check_case(case, "gaussian", 0.1)      # (the verifier's asserts are the test)
    logits, reg, anchors = (torch.from_numpy(x).cuda() for x in _inputs(n, A, K))
    narrow = _post_soft(logits, reg, anchors, st, NMS_THRESH, GAUSSIAN, 0.1, topk, dets)[1]
    wide = _post_soft(logits, reg, anchors, st, NMS_THRESH, GAUSSIAN, 50.0, topk, dets)[1]
    assert float(narrow[1].sum()) < float(wide[1].sum())


@pytest.mark.gpu
@pytest.mark.parametrize("fast", ["1", "0"])
def test_hard_method_through_the_soft_entry_is_dn_postprocess(fast, monkeypatch):
    monkeypatch.setenv("DN_PP_FAST", fast)
    for case in (OP_CASES[1], OP_CASES[5], OP_CASES[6]):
        n, A, K, topk, dets, st = case
        logits, reg, anchors = (torch.from_numpy(x).cuda() for x in _inputs(n, A, K))
        rc, a = _post_soft(logits, reg, anchors, st, NMS_THRESH, HARD, 0.0, topk, dets)      # (sigma is not read in hard mode)
        _lib.check(rc, "dn_postprocess_soft")
        rc, b = _post_soft(logits, reg, anchors, st, NMS_THRESH, HARD, 0.0, topk, dets, hard_entry=True)
        _lib.check(rc, "dn_postprocess")
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        assert int(a[3].sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("st", [0.0, 0.02])
def test_linear_mode_equals_the_hard_path_where_no_score_can_decay(st):
    """Every same-class pair has IoU <= nms_thresh (factor 1) or is an exact duplicate (IoU 1: factor 0, dropped at any score_thresh >= 0):
    linear soft-NMS emits what hard NMS keeps, with untouched scores -- bit for bit the reference-pinned hard path."""
    logits, reg, anchors = (torch.from_numpy(x).cuda() for x in _lattice_inputs())
    rc, soft = _post_soft(logits, reg, anchors, st, NMS_THRESH, LINEAR, SIGMA, 200, 300)
    _lib.check(rc, "dn_postprocess_soft")
    rc, hard = _post_soft(logits, reg, anchors, st, NMS_THRESH, HARD, 0.0, 200, 300, hard_entry=True)
    _lib.check(rc, "dn_postprocess")
    for x, y, what in zip(soft, hard, ("boxes", "scores", "labels", "counts", "kept anchors")):
        assert np.array_equal(x, y), what
    assert int(soft[3].min()) >= 144 and int(soft[3].max()) < 3 * 184      # the duplicates are gone, the lattice stays


@pytest.mark.gpu
def test_soft_postprocess_rejections():
    n, A, K, topk, dets, st = OP_CASES[0]
    logits, reg, anchors = (torch.from_numpy(x).cuda() for x in _inputs(n, A, K))
    for method, sigma in ((3, 0.5), (-1, 0.5), (GAUSSIAN, 0.0), (GAUSSIAN, float("nan")), (GAUSSIAN, float("inf")), (GAUSSIAN, -0.5)):
        rc, _ = _post_soft(logits, reg, anchors, st, NMS_THRESH, method, sigma, topk, dets)
        assert rc == -1, (method, sigma, rc)
    need = _lib.lib().dn_postprocess_workspace_bytes(n, A, K, topk, dets)
    for method in (LINEAR, GAUSSIAN):
        rc, _ = _post_soft(logits, reg, anchors, st, NMS_THRESH, method, SIGMA, topk, dets, ws_bytes=need - 256)
        assert rc == -3, rc
    rc, _ = _post_soft(logits, reg, anchors, st, NMS_THRESH, LINEAR, float("nan"), topk, dets)      # sigma is the Gaussian's alone
    assert rc == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU, model level
# ------------------------------------------------------------------------------------------------------------------------------------
def _model(name, ncls):
    m = getattr(models, name)(num_classes=ncls)
    models.load_synthetic(m, 0)
    return m.cuda()


def _op_on_heads(m, imgs, method, sigma):
    """dn_postprocess_soft on the model's own head outputs, in the padded form of forward_batch."""
    logits, reg = m.forward_heads(imgs)
    anchors = torch.from_numpy(m._lowered.anchors).cuda()
    W, H = m.graph.size
    L = _lib.lib()
    n, A, K = logits.shape
    D, topk = m.detections_per_img, m.topk_candidates
    ws = torch.empty(L.dn_postprocess_workspace_bytes(n, A, K, topk, D), dtype=torch.uint8, device="cuda")
    boxes = torch.empty(n, D, 4, device="cuda"); scores = torch.empty(n, D, device="cuda")
    labels = torch.empty(n, D, dtype=torch.int64, device="cuda"); counts = torch.empty(n, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(L.dn_postprocess_soft(p(logits), p(reg), p(anchors), n, A, K, float(H), float(W), None, float(m.score_thresh), float(m.nms_thresh),
                                     _lib.DN_NMS[method], float(sigma), int(topk), int(D), p(boxes), p(scores), p(labels), p(counts), None,
                                     p(ws), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dn_postprocess_soft")
    torch.cuda.synchronize()
    return boxes, scores, labels, counts


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,epilogue", [("ssdlite320_mobilenet_v3_large", 3, False), ("ssdlite320_mobilenet_v3_large", 37, True),
                                              ("ssd300_vgg16", 2, False)])
def test_model_forward_in_gaussian_mode_is_the_op_on_its_head_outputs(name, n, epilogue, monkeypatch):
    """model(images) == dn_postprocess_soft(forward_heads(images)) bit for bit: below the fused head epilogue's batch size, with it (37 images
    run as chains of 19 and 18: the epilogue's threshold is set to 16 images per chain), and on the VGG model (another level table, the
    anchor-major score layout)."""
    raw = C.CDLL(_lib.LIB_PATH)
    if epilogue:
        monkeypatch.setenv("DN_HEAD_SOFTMAX_MINN", "16")
    m = _model(name, 21).set_nms("gaussian", sigma=SIGMA)
    W, H = m.graph.size
    imgs = torch.from_numpy(synth.images(71, n, H, W)).cuda()
    before = raw.dn_debug_head_softmax_launches()
    got = [t.clone() for t in m.forward_batch(imgs)]
    assert (raw.dn_debug_head_softmax_launches() - before >= 1) == epilogue
    ref = _op_on_heads(m, imgs, "gaussian", SIGMA)
    for x, y, what in zip(got, ref, ("boxes", "scores", "labels", "counts")):
        assert torch.equal(x, y), what
    assert int(got[3].min()) > 0
    # the list form returns the same detections
    dets = m(list(imgs))
    for i, d in enumerate(dets):
        c = int(got[3][i])
        assert torch.equal(d["scores"], got[1][i, :c]) and torch.equal(d["labels"], got[2][i, :c]) and torch.equal(d["boxes"], got[0][i, :c])
    # and the soft result is not the hard one
    hard = [t.clone() for t in m.set_nms("hard").forward_batch(imgs)]
    assert not torch.equal(hard[1], got[1])


@pytest.mark.gpu
def test_uint8_packed_and_pipelined_forwards_follow_the_mode():
    from demonet_amd.dist import pack_detections
    from demonet_amd.pipeline import ForwardPipeline
    m = _model("ssdlite320_mobilenet_v3_large", 21).set_nms("gaussian", sigma=0.3)
    n = 4
    u8 = torch.from_numpy((synth.images(73, n, 320, 320) * 255).round().astype(np.uint8)).cuda().permute(0, 2, 3, 1).contiguous()
    imgs = (u8.cpu().permute(0, 3, 1, 2).float() / 255).contiguous().cuda()      # (true division, on the CPU: torch's GPU kernel multiplies by 1 / 255)
    D = m.detections_per_img
    packed = torch.empty(n, D + 1, 6, device="cuda")
    ref = [t.clone() for t in m.forward_batch(imgs, packed=packed)]
    assert torch.equal(packed[:, :D], pack_detections(ref[0], ref[1], ref[2])) and torch.equal(packed[:, D, 0].to(torch.int32), ref[3])
    hard = [t.clone() for t in _model("ssdlite320_mobilenet_v3_large", 21).forward_batch(imgs)]
    assert not torch.equal(hard[1], ref[1]), "the Gaussian mode must change the scores of this batch"
    for x, y in zip(ref, m.forward_uint8(u8)):
        assert torch.equal(x, y)
    with ForwardPipeline(m, n, depth=3) as pipe:
        tickets = [pipe.submit(imgs) for _ in range(4)]
        for t in tickets[-3:]:
            for x, y in zip(ref, pipe.result(t)):
                assert torch.equal(x, y)


@pytest.mark.gpu
def test_mode_switches_keep_the_plan_and_return_to_the_hard_result():
    imgs = torch.from_numpy(synth.images(79, 5, 320, 320)).cuda()
    never = [t.clone() for t in _model("ssdlite320_mobilenet_v3_large", 21).forward_batch(imgs)]
    m = _model("ssdlite320_mobilenet_v3_large", 21)
    first = [t.clone() for t in m.forward_batch(imgs)]
    gen, handle = m._plan_gen, m._handle
    soft = {}
    for method in ("gaussian", "linear", "gaussian"):
        out = [t.clone() for t in m.set_nms(method).forward_batch(imgs)]
        if method in soft:
            for x, y in zip(soft[method], out):
                assert torch.equal(x, y)
        soft[method] = out
        again = m.forward_batch(imgs)          # graph replay
        for x, y in zip(out, again):
            assert torch.equal(x, y)
    assert not torch.equal(soft["gaussian"][1], soft["linear"][1])
    back = m.set_nms("hard").forward_batch(imgs)
    for x, y, z in zip(never, first, back):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert (m._plan_gen, m._handle) == (gen, handle), "a mode switch must not rebuild the plan"
    # a rebuilt plan inherits the mode
    m.set_nms("gaussian")
    m.invalidate()
    out = m.forward_batch(imgs)
    assert m._plan_gen == gen + 1
    for x, y in zip(soft["gaussian"], out):
        assert torch.equal(x, y)
