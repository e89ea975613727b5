"""GPU tests (-m gpu) of vocabularies above 256 foreground classes (LVIS v1: 1 204 classes with the background, OpenImages: 601, Objects365:
366), up to DN_MAX_CLASSES = 2048: the wide softmax / decode kernel and the wide merge of csrc/postprocess.hip, the limit at the C boundary,
the fused-head epilogue's class bound, and the 64-bit offsets of head outputs above 2^31 bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import ssd_oracle as so
from demonet_amd import _lib, models, synth

pytestmark = pytest.mark.gpu

LOGIT_ATOL, LOGIT_RTOL = 6e-2, 1e-2       # the measured fp16-storage tolerance of tests/test_gpu_model.py (same synthetic heads)
LOSS_RTOL = 2e-5                          # tests/test_loss.py


def _risky(m):
    # a near-tie that 1-ulp softmax differences could flip (exact ties, gap 0, break canonically)
    return min(m["thresh_gap"], m["iou_gap"]) < 1e-5 or any(0 < m[k] < 1e-5 for k in ("topk_gap", "final_gap", "order_gap"))


def _pp_case(n, A, K, seed):
    """Logits whose passing scores are well separated: a background logit above a low baseline (foreground softmax far below the threshold),
    then on 8 % of the anchors one to three raised classes drawn with weight 1 / class (class 1 is heavy, classes above 256 occur), exact
    duplicate rows (score ties), partly with the same anchor box too (tied boxes)."""
    rng = np.random.default_rng(seed)
    logits = (-8.0 + rng.normal(0, 0.1, (n, A, K))).astype(np.float32)
    logits[:, :, 0] = 3.0
    w = 1.0 / np.arange(1, K)
    w /= w.sum()
    for i in range(n):
        hot = np.nonzero(rng.random(A) < 0.08)[0]
        for r in range(3):
            cls = 1 + rng.choice(K - 1, hot.size, p=w)
            on = rng.random(hot.size) < (1.0 if r == 0 else 0.4)
            a = hot[on]
            logits[i, a, cls[on]] = rng.uniform(2.0, 8.0, a.size).astype(np.float32)
    reg = rng.normal(0, 1.0, (n, A, 4)).astype(np.float32)
    ctr = rng.uniform(20, 300, (A, 2)).astype(np.float32)
    wh = rng.uniform(10, 120, (A, 2)).astype(np.float32)
    anchors = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)
    dup = rng.integers(0, A, A // 10)
    src = rng.integers(0, A, A // 10)
    logits[:, dup] = logits[:, src]
    reg[:, dup] = reg[:, src]
    anchors[dup[: len(dup) // 2]] = anchors[src[: len(dup) // 2]]
    return logits, reg, anchors


def _postprocess(logits, reg, anchors, hw, st, nt, topk, dets):
    L = _lib.lib()
    n, A, K = logits.shape
    ws = torch.empty(L.dn_postprocess_workspace_bytes(n, A, K, topk, dets), dtype=torch.uint8, device="cuda")
    boxes = torch.empty(n, dets, 4, device="cuda")
    scores = torch.empty(n, dets, device="cuda")
    labels = torch.empty(n, dets, dtype=torch.int64, device="cuda")
    counts = torch.empty(n, dtype=torch.int32, device="cuda")
    kept = torch.empty(n, dets, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = L.dn_postprocess(p(logits), p(reg), p(anchors), n, A, K, float(hw[0]), float(hw[1]), None, float(st), float(nt),
                          int(topk), int(dets), p(boxes), p(scores), p(labels), p(counts), p(kept), p(ws), ws.numel(),
                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "dn_postprocess")
    torch.cuda.synchronize()
    return boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy(), counts.cpu().numpy(), kept.cpu().numpy()


def _model(name, ncls, **kw):
    m = getattr(models, name)(num_classes=ncls, **kw)
    models.load_synthetic(m, 0)
    return m.cuda()


def _compare_to_oracle_post(m, logits, reg, dets_dev, picks, exact_min=0):
    """Detections of images `picks` (device tensors of forward_batch) against the oracle's post-process of the device's own head outputs
    (logits / reg: the rows of those images, CPU). Labels / boxes exact-order where no near-tie decides them; counts and sorted scores always."""
    g = m.graph
    p = g.post
    anchors = torch.from_numpy(m._lowered.anchors)
    ref = so.postprocess_detections(logits, reg, anchors, (g.size[1], g.size[0]), p["score_thresh"], p["nms_thresh"], p["detections_per_img"],
                                    p["topk_candidates"], return_intermediates=True)
    boxes, scores, labels, counts = [t.cpu().numpy() for t in dets_dev]
    exact = 0
    for j, i in enumerate(picks):
        d = ref[j]
        cnt = int(counts[i])
        assert cnt == d["labels"].shape[0] <= p["detections_per_img"], (i, cnt, d["labels"].shape[0])
        mg = so.selection_margins(d["softmax"], d["decoded"], p["score_thresh"], p["nms_thresh"], p["topk_candidates"], p["detections_per_img"])
        if not _risky(mg):
            assert np.array_equal(labels[i, :cnt], d["labels"]), i
            np.testing.assert_allclose(boxes[i, :cnt], d["boxes"], rtol=1e-5, atol=1e-3)
            exact += 1
        np.testing.assert_allclose(np.sort(scores[i, :cnt])[::-1], np.sort(d["scores"])[::-1], rtol=1e-5, atol=1e-7)
    assert exact >= exact_min
    return ref


@pytest.fixture(params=["1", "0"], ids=["cutoff-fast-path", "full-path"])
def pp_fast(request, monkeypatch):
    monkeypatch.setenv("DN_PP_FAST", request.param)
    return request.param


# (n, A, K, topk, dets, score_thresh, seed): seeds picked on the CPU with ssd_oracle.selection_margins so that no image has a near-tie
PP_CASES = [
    (3, 3234, 258, 300, 300, 0.001, 258),      # one class above the narrow kernel's 256
    (2, 3234, 366, 300, 300, 0.001, 366),      # Objects365
    (2, 3234, 1204, 300, 300, 0.001, 1204),    # LVIS v1
    (1, 8732, 1204, 400, 200, 0.01, 1204),     # LVIS v1 on the ssd300 anchor count, topk 400 (the 512-candidate variants)
    (2, 3234, 257, 300, 300, 0.001, 257),      # the narrow kernel at its largest K (a [64][257] tile: more than 64 KB of LDS)
]


@pytest.mark.parametrize("n,A,K,topk,dets,st,seed", PP_CASES, ids=[f"K{c[2]}-A{c[1]}" for c in PP_CASES])
def test_postprocess_above_256_classes_vs_oracle(n, A, K, topk, dets, st, seed, pp_fast):
    """dn_postprocess in isolation: kept labels and anchor indices of every image equal the oracle's exactly, scores and boxes to float
    tolerance, rows beyond the count zero."""
    logits, reg, anchors = _pp_case(n, A, K, seed)
    nt = 0.5
    ref = so.postprocess_detections(torch.from_numpy(logits), torch.from_numpy(reg), torch.from_numpy(anchors), (320, 320), st, nt, dets, topk,
                                    return_intermediates=True)
    b, s, l, c, k = _postprocess(torch.from_numpy(logits).cuda(), torch.from_numpy(reg).cuda(), torch.from_numpy(anchors).cuda(), (320, 320),
                                 st, nt, topk, dets)
    compared = 0
    for i, d in enumerate(ref):
        assert not _risky(so.selection_margins(d["softmax"], d["decoded"], st, nt, topk, dets)), "fixture has a near-tie: pick another seed"
        cnt = int(c[i])
        assert cnt == d["labels"].shape[0] > 0
        assert np.array_equal(l[i, :cnt], d["labels"]), i
        assert np.array_equal(k[i, :cnt], d["anchor_idx"]), i
        np.testing.assert_allclose(s[i, :cnt], d["scores"], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(b[i, :cnt], d["boxes"], rtol=1e-5, atol=2e-3)
        assert (s[i, cnt:] == 0).all() and (l[i, cnt:] == 0).all()
        compared += 1
    assert compared == n
    assert int(l.max()) > 256 or K < 366            # labels above 256 made it through the merge (uint16 label slots)


def test_ssdlite_lvis_batch64_against_the_cpu_path():
    """ssdlite320_mobilenet_v3_large(num_classes=1204) at batch 64 (1.0 GB of head outputs): head logits of images 0, 31, 32, 63 within the logit
    tolerance of the fp32 CPU path, detections equal to the oracle's post-process of the device's own head outputs, graph replay equal to eager."""
    name, n, picks = "ssdlite320_mobilenet_v3_large", 64, [0, 31, 32, 63]
    m = _model(name, 1204)
    try:
        imgs = torch.from_numpy(synth.images(2024, n, 320, 320)).cuda()
        o = so.OracleSSD(name, synth.state_dict(m.graph, 0), 1204)
        raw = o.forward_raw([imgs[i].cpu() for i in picks])
        logits, reg = m.forward_heads(imgs)
        assert tuple(logits.shape) == (n, m.graph.num_anchors(), 1204)
        lg, rg = logits[picks].cpu(), reg[picks].cpu()
        del logits, reg
        err = (lg - raw["cls_logits"]).abs()
        assert bool((err <= LOGIT_ATOL + LOGIT_RTOL * raw["cls_logits"].abs()).all()), err.max().item()
        assert bool(((rg - raw["bbox_regression"]).abs() <= 6e-2 + 1e-2 * raw["bbox_regression"].abs()).all())
        first = [t.clone() for t in m.forward_batch(imgs, persistent_input=True)]
        replay = [t.clone() for t in m.forward_batch(imgs, persistent_input=True)]
        m.set_graph_mode(False)
        eager = [t.clone() for t in m.forward_batch(imgs, persistent_input=True)]
        torch.cuda.synchronize()
        for q in range(4):
            assert torch.equal(first[q], replay[q]) and torch.equal(first[q], eager[q]), q
        assert int(first[2].max()) > 256
        _compare_to_oracle_post(m, lg, rg, first, picks)
    finally:
        m.release()


def test_vgg300_lvis_batch64_head_outputs_above_2gb():
    """ssd300_vgg16(num_classes=1204) at batch 64: 2.69 GB of class logits (> 2^31 bytes: every offset on the path is 64-bit). Detections of
    images 0 and 63 equal the oracle's post-process of the device's own head outputs."""
    n, picks = 64, [0, 63]
    m = _model("ssd300_vgg16", 1204)
    try:
        imgs = torch.from_numpy(synth.images(77, n, 300, 300)).cuda()
        logits, reg = m.forward_heads(imgs)
        assert logits.numel() * 4 > 2 ** 31
        lg, rg = logits[picks].cpu(), reg[picks].cpu()
        del logits, reg
        assert bool(torch.isfinite(lg).all()) and float(lg.abs().max()) > 0
        dets = [t.clone() for t in m.forward_batch(imgs)]
        torch.cuda.synchronize()
        assert int(dets[3][63]) > 0
        _compare_to_oracle_post(m, lg, rg, dets, picks)
    finally:
        m.release()


def test_v2_objects365_uint8_equals_float_path():
    """ssd_lite_mobilenet_v2(image_size=300, num_classes=366): the uint8 HWC entry equals the float path bit for bit."""
    m = _model("ssd_lite_mobilenet_v2", 366, image_size=300)
    try:
        g = torch.Generator().manual_seed(366)
        u8 = torch.randint(0, 256, (5, 300, 300, 3), dtype=torch.uint8, generator=g).cuda()
        ref_in = (u8.cpu().permute(0, 3, 1, 2).float() / 255).contiguous().cuda()
        ref = [t.clone() for t in m.forward_batch(ref_in, persistent_input=True)]
        for _ in range(2):
            got = [t.clone() for t in m.forward_uint8(u8)]
        torch.cuda.synchronize()
        for a, b in zip(ref, got):
            assert torch.equal(a, b)
    finally:
        m.release()


def test_pipeline_of_lvis_forwards_equals_forward_batch():
    """Three forwards of the K = 1204 model in flight through ForwardPipeline equal forward_batch of each batch."""
    from demonet_amd.pipeline import ForwardPipeline
    m = _model("ssdlite320_mobilenet_v3_large", 1204)
    try:
        batches = [torch.from_numpy(synth.images(300 + i, 16, 320, 320)).cuda() for i in range(3)]
        with ForwardPipeline(m, 16, depth=3) as pipe:
            ref = [[t.clone() for t in m.forward_batch(b)] for b in batches]
            for _ in range(2):
                ts = [pipe.submit(b) for b in batches]
                for k, t in enumerate(ts):
                    for a, b in zip(ref[k], pipe.result(t)):
                        assert torch.equal(a, b), k
        assert int(sum(int(r[3].sum()) for r in ref)) > 0
    finally:
        m.release()


def test_class_limit():
    """num_classes = DN_MAX_CLASSES (2048) builds and runs; 2049 is refused with a message that names the limit (dn_create and
    dn_postprocess alike)."""
    m = _model("ssdlite320_mobilenet_v3_large", 2048)
    try:
        img = torch.from_numpy(synth.images(7, 1, 320, 320)).cuda()
        boxes, scores, labels, counts = m.forward_batch(img)
        torch.cuda.synchronize()
        assert 0 <= int(counts[0]) <= m.graph.post["detections_per_img"] and int(labels.max()) < 2048
    finally:
        m.release()
    m = _model("ssdlite320_mobilenet_v3_large", 2049)
    with pytest.raises(RuntimeError, match="2048"):
        m.forward_batch(torch.from_numpy(synth.images(7, 1, 320, 320)).cuda())
    logits = torch.zeros(1, 64, 2049, device="cuda")
    reg = torch.zeros(1, 64, 4, device="cuda")
    anchors = torch.tensor([[0.0, 0.0, 10.0, 10.0]] * 64, device="cuda")
    with pytest.raises(RuntimeError, match="2048"):
        _postprocess(logits, reg, anchors, (320, 320), 0.01, 0.5, 100, 100)


def test_loss_lvis_vs_oracle():
    """dn_ssd_loss at K = 1204 against ssd_loss_oracle."""
    from demonet_amd.loss import ssd_loss
    n, A, K = 2, 3234, 1204
    rng = np.random.RandomState(1204)
    c = rng.uniform(0, 300, (A, 2)).astype(np.float32)
    wh = rng.uniform(10, 120, (A, 2)).astype(np.float32)
    anchors = torch.from_numpy(np.concatenate([c - wh / 2, c + wh / 2], 1))
    logits = torch.from_numpy(rng.randn(n, A, K).astype(np.float32) * 3)
    reg = torch.from_numpy(rng.randn(n, A, 4).astype(np.float32))
    targets = []
    for gcount in (6, 11):
        xy = rng.uniform(0, 250, (gcount, 2)).astype(np.float32)
        b = torch.from_numpy(np.concatenate([xy, xy + rng.uniform(8, 150, (gcount, 2)).astype(np.float32)], 1))
        targets.append({"boxes": b, "labels": torch.from_numpy(rng.randint(1, K, (gcount,)).astype(np.int64))})
    want, wm = so.ssd_loss_oracle(logits, reg, anchors, targets, 0.5, 3.0)
    got, gm = ssd_loss({"cls_logits": logits.cuda(), "bbox_regression": reg.cuda()}, [anchors.cuda()] * n, targets, 0.5, 3.0)
    assert np.array_equal(gm.cpu().numpy(), wm.numpy())
    for k in want:
        assert abs(got[k].item() - want[k].item()) <= LOSS_RTOL * abs(want[k].item()) + 1e-7, k


@pytest.mark.parametrize("ncls,epilogue", [(92, True), (93, False), (200, False)])
def test_fused_head_softmax_boundary(ncls, epilogue, monkeypatch):
    """The fused head launch computes softmax / decode in its epilogue for the factories' 6-anchor levels up to K = 92 (its LDS bound) and not
    above; either way the detections equal the logit-writing path bit for bit."""
    raw = C.CDLL(_lib.LIB_PATH)
    imgs = torch.from_numpy(synth.images(92, 8, 320, 320)).cuda()
    monkeypatch.setenv("DN_HEAD_SOFTMAX_MINN", "1")
    res, launches = {}, {}
    for flag in ("0", "1"):
        monkeypatch.setenv("DN_HEAD_SOFTMAX", flag)
        m = _model("ssdlite320_mobilenet_v3_large", ncls)
        try:
            before = raw.dn_debug_head_softmax_launches()
            res[flag] = [t.clone() for t in m.forward_batch(imgs)]
            launches[flag] = raw.dn_debug_head_softmax_launches() - before
        finally:
            m.release()
    assert launches["0"] == 0
    assert (launches["1"] >= 1) == epilogue, launches
    assert int(res["1"][3].sum()) > 0
    for q in range(4):
        assert torch.equal(res["0"][q], res["1"][q]), q
