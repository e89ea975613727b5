"""The backward through the SSDLite heads (csrc/headgrad.hip, demonet_amd/headgrad.py) against the float64 reference and the derived
per-element bound of tests/head_grad_ref.py. CPU part: the ABI, the parameter bookkeeping, the input condition of every case, the
new unit's resources. GPU part: dn_lite_head_backward on raw buffers, then SSD.loss(...).backward() on whole models."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import head_grad_ref as hr
from demonet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dn_lite_head_backward_workspace_bytes", "dn_lite_head_backward", "dn_level_features", "dn_forward_features")
REGIMES = ["small", "unit"]
_P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU
def test_symbols_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "demonet_hip.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for sym in NEW_SYMBOLS:
        assert sym in _lib.EXPORTS, sym
        assert re.search(r"DN_API\s+\w+\s+%s\(" % sym, header), sym
        assert hasattr(lib, sym), sym
    assert _lib.DN_ABI_VERSION == 1 and "#define DN_ABI_VERSION 1" in header


def test_headgrad_is_built_without_scratch_and_hazards(tmp_path):
    """the new unit as build.py compiles it: part of SOURCES, on the fp16 matrix cores, no scratch in any kernel, no inline-asm read of a
    matrix result inside its hazard window (tools/mfma_hazard_scan.py), no inline asm at all"""
    from demonet_amd import build
    assert "headgrad.hip" in build.SOURCES
    src = os.path.join(ROOT, "demonet_amd", "csrc", "headgrad.hip")
    assert "asm" not in re.sub(r"//.*", "", open(src).read())
    out = os.path.join(str(tmp_path), "headgrad.s")
    subprocess.check_call([build.HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-gpu-rdc", "--cuda-device-only", "-S",
                           *build.EXTRA.get("headgrad.hip", []), src, "-o", out])
    text = open(out).read()
    assert "v_mfma_f32_32x32x16_f16" in text
    scratch = [int(v) for v in re.findall(r"; ScratchSize: (\d+)", text)]
    assert len(scratch) >= 5 and all(v == 0 for v in scratch), scratch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from mfma_hazard_scan import asm_hazards
    assert not asm_hazards(text)


@pytest.mark.parametrize("i", range(len(hr.OP_CASES)))
@pytest.mark.parametrize("regime", REGIMES)
def test_op_case_input_condition(i, regime):
    x, wd, bd, w1, dy = hr.op_case(i, regime)
    assert hr.level_bound(x, wd, bd, w1, dy, False)["ambiguous"] <= hr.AMBIGUOUS_CAP


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU, op level
def _run_op(x, wd, bd, w1, dy, pad_rows=3):
    """dn_lite_head_backward on device copies of an op_case; dy is embedded in a larger [n][A][cols] array (rows in front of and behind
    the level) so that the in-place addressing (image stride, level offset) is exercised. Returns the four outputs on the CPU."""
    dev = torch.device("cuda")
    n, c, h, w = x.shape
    cout = w1.shape[0]
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)                                   # NHWC fp16
    wdd = wd.reshape(c, 9).t().contiguous().to(dev) if wd is not None else None         # [9][c]
    bdd = bd.float().to(dev) if bd is not None else None
    w1d = w1.contiguous().to(dev)
    stride = (h * w + 2 * pad_rows) * cout
    full = torch.full((n, stride), float("nan"), dtype=torch.float32, device=dev)
    full[:, pad_rows * cout:(pad_rows + h * w) * cout] = hr.rows(dy).reshape(n, h * w * cout).to(dev)
    L = _lib.lib()
    ws = torch.empty(int(L.dn_lite_head_backward_workspace_bytes(n, h, w, c, cout, int(wd is not None))), dtype=torch.uint8, device=dev)
    outs = []
    for _ in range(2):
        g = dict(g_wd=torch.full((9, c), float("nan"), device=dev) if wd is not None else None,
                 g_bd=torch.full((c,), float("nan"), device=dev) if wd is not None else None,
                 g_w1=torch.full((cout, c), float("nan"), device=dev), g_b1=torch.full((cout,), float("nan"), device=dev))
        ws.fill_(0xFF)
        dyp = C.c_void_p(full.data_ptr() + pad_rows * cout * 4)
        _lib.check(L.dn_lite_head_backward(_P(xd), _P(wdd), _P(bdd), _P(w1d), dyp, stride, n, h, w, c, cout, _P(g["g_wd"]), _P(g["g_bd"]),
                                           _P(g["g_w1"]), _P(g["g_b1"]), _P(ws), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "dn_lite_head_backward")
        torch.cuda.synchronize()
        outs.append({k: (v.cpu() if v is not None else None) for k, v in g.items()})
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(hr.OP_CASES)))
@pytest.mark.parametrize("regime", REGIMES)
def test_op_level_within_bound_and_deterministic(i, regime):
    x, wd, bd, w1, dy = hr.op_case(i, regime)
    first, second = _run_op(x, wd, bd, w1, dy)
    ref = hr.level_grads(x, wd, bd, w1, dy)
    bound = hr.level_bound(x, wd, bd, w1, dy, False)
    assert bound["ambiguous"] <= hr.AMBIGUOUS_CAP
    worst = {}
    for k in ("g_wd", "g_bd", "g_w1", "g_b1"):
        if ref[k] is None:
            continue
        worst[k] = hr.worst_ratio(first[k], ref[k], bound[k])
        assert torch.equal(first[k].view(torch.int32), second[k].view(torch.int32)), "%s: two runs differ" % k
    print("op case %s %s: worst |got - ref| / bound %s" % (hr.OP_CASES[i], regime, {k: "%.3f" % v for k, v in worst.items()}))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.gpu
def test_op_level_rejects_what_it_does_not_take():
    dev = torch.device("cuda")
    L = _lib.lib()
    t = torch.zeros(1 << 16, dtype=torch.float32, device=dev)
    p = _P(t)
    args = lambda n, h, w, c, cout: (p, p, p, p, p, h * w * cout, n, h, w, c, cout, p, p, p, p, p, t.numel() * 4, None)
    assert L.dn_lite_head_backward(*args(1, 2, 2, 12, 8)) == -4          # DN_E_UNSUPPORTED: c % 8
    assert L.dn_lite_head_backward(*args(1, 2, 2, 16, 6 * 2048 + 1)) == -4
    assert L.dn_lite_head_backward(*args(0, 2, 2, 16, 8)) == -1          # DN_E_INVALID
    assert L.dn_lite_head_backward(*args(1, 2, 2, 16, 0)) == -1
    bad = list(args(1, 2, 2, 16, 8))
    bad[5] = 1                                                           # image stride smaller than the level
    assert L.dn_lite_head_backward(*bad) == -1
    bad = list(args(1, 2, 2, 16, 8))
    bad[16] = 16                                                         # workspace too small
    assert L.dn_lite_head_backward(*bad) == -3


# ------------------------------------------------------------------------------------------------------------------------------------
# whole models
V3, V2 = hr.V3, hr.V2
LOSS_RTOL = 2e-5          # tests/test_loss.py


def _model(kind, K, seed=0):
    from demonet_amd import models
    m = models.ssdlite320_mobilenet_v3_large(num_classes=K) if kind == V3 else models.ssd_lite_mobilenet_v2(num_classes=K)
    return models.load_synthetic(m, seed)


def _targets(boxes_per_image, K, seed=3):
    rng = np.random.RandomState(seed)
    targets = []
    for gcount in boxes_per_image:
        xy = rng.uniform(0, 220, (gcount, 2)).astype(np.float32)
        targets.append({"boxes": torch.from_numpy(np.concatenate([xy, xy + rng.uniform(20, 90, (gcount, 2)).astype(np.float32)], 1)).reshape(-1, 4),
                        "labels": torch.from_numpy(rng.randint(1, K, (gcount,)).astype(np.int64))})
    return targets


@pytest.mark.parametrize("kind", [V3, V2])
def test_head_parameters_are_the_reference_head_keys(kind):
    m = _model(kind, 21)
    hp = m.head_parameters()
    assert list(hp) == [k for k, _ in m.named_parameters() if k.startswith("head.")]
    assert set(hp) == set(hr.head_param_keys(kind, 6)) == {k for k in m.state_dict() if k.startswith("head.") and "running_" not in k and "num_batches" not in k}
    assert len(hp) == (60 if kind == V3 else 64)
    assert not any(p.requires_grad for p in m.parameters())                      # default: nothing trains
    m.train_heads()
    assert all(p.requires_grad == k.startswith("head.") for k, p in m.named_parameters())
    m.train_heads(False)
    assert not any(p.requires_grad for p in m.parameters())


def test_training_mode_errors_name_train_heads():
    from demonet_amd import models
    m = _model(V3, 21).train()
    with pytest.raises(ValueError):
        m([torch.zeros(3, 320, 320)])
    with pytest.raises(NotImplementedError, match="train_heads"):
        m([torch.zeros(3, 320, 320)], _targets([1], 21))
    v = models.ssd300_vgg16(num_classes=5).train()
    with pytest.raises(NotImplementedError):
        v.train_heads()
    for p in v.parameters():
        p.requires_grad_(True)
    with pytest.raises(NotImplementedError):
        v([torch.zeros(3, 300, 300)], _targets([1], 5))


def _fold_matches_blob(kind, device):
    """headgrad.fold (float64 torch ops, fp16 by one rounding) against the folded weights of plan.py's blob, bit for bit"""
    from demonet_amd import headgrad
    from demonet_amd.plan import LoweredModel
    m = _model(kind, 21, seed=1)
    sd = {k: v.detach().float().cpu() if v.is_floating_point() else v.detach().cpu() for k, v in m.state_dict().items()}
    low = LoweredModel(m.graph, sd)
    blob = np.frombuffer(low.blob, dtype=np.uint8)
    at = lambda off, dt, count: torch.from_numpy(blob[off:off + count * np.dtype(dt).itemsize].view(dt).copy())
    by_key = {nd.conv_key: low.ops[i] for i, nd in enumerate(m.graph.nodes) if nd.conv_key}
    m = m.to(device)
    P, B = dict(m.named_parameters()), dict(m.named_buffers())
    for e in headgrad.entries(m.graph):
        wd, bd, w1, b1, s, inv = headgrad.fold(e, P, B)
        o = by_key[e.pw_w[:-len(".weight")]]
        assert torch.equal(w1.cpu().view(torch.int16).reshape(-1), at(o.w_off, np.float16, e.cout * e.c).view(torch.int16)), e.pw_w
        assert torch.equal(b1.cpu().view(torch.int32), at(o.b_off, np.float32, e.cout).view(torch.int32)), e.pw_b
        if e.dw_w:
            o = by_key[e.dw_w[:-len(".weight")]]
            assert torch.equal(wd.cpu().view(torch.int16).reshape(-1), at(o.w_off, np.float16, 9 * e.c).view(torch.int16)), e.dw_w
            assert torch.equal(bd.cpu().view(torch.int32), at(o.b_off, np.float32, e.c).view(torch.int32)), e.bn


@pytest.mark.parametrize("kind", [V3, V2])
def test_fold_equals_the_plan_blob_cpu(kind):
    _fold_matches_blob(kind, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [V3, V2])
def test_fold_equals_the_plan_blob_on_the_device(kind):
    _fold_matches_blob(kind, "cuda")


def _train_step(m, imgs, targets):
    """one differentiable loss through the library, keeping the gradient the loss sent into the heads: (losses, d_cls, d_reg, features)"""
    from demonet_amd import headgrad
    ho = headgrad.head_outputs(m, imgs)
    for t in ho.values():
        t.retain_grad()
    step = ho["cls_logits"].grad_fn.step
    losses = m.compute_loss(targets, ho)
    for p in m.parameters():
        p.grad = None
    (losses["bbox_regression"] + losses["classification"]).backward()
    feats = [torch.cat([x for x, _, _ in lv]).permute(0, 3, 1, 2).cpu() for lv in step.pieces]
    return losses, ho["cls_logits"].grad.cpu(), ho["bbox_regression"].grad.cpu(), feats


def _check_model(kind, K, imgs, targets, levels=None, tag=""):
    m = _model(kind, K).cuda()
    with torch.no_grad():
        plain = m.loss(imgs, targets)
    assert all(p.grad is None for p in m.parameters())
    m.train_heads()
    gen = m._plan_gen
    via_loss = m.loss(imgs, targets)
    assert via_loss["classification"].requires_grad and via_loss["bbox_regression"].requires_grad
    losses, d_cls, d_reg, feats = _train_step(m, imgs, targets)
    assert m._plan_gen == gen
    for k in plain:
        for got in (via_loss[k], losses[k]):
            assert abs(got.item() - plain[k].item()) <= LOSS_RTOL * abs(plain[k].item()) + 1e-7, (k, got.item(), plain[k].item())
    hp = m.head_parameters()
    for k, p in m.named_parameters():
        assert (p.grad is not None) == (k in hp), k
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ref, amb = hr.model_reference(kind, sd, feats, list(m.graph.anchors_per_loc), K, d_cls, d_reg, levels)
    assert amb <= hr.AMBIGUOUS_CAP, amb
    worst = {k: hr.worst_ratio(hp[k].grad.cpu(), g, b) for k, (g, b) in ref.items()}
    assert all(bool(torch.isfinite(p.grad).all()) for p in hp.values())
    top = max(worst, key=worst.get)
    fg = int((d_reg.abs().sum(-1) > 0).sum())
    print("model case %s %s K=%d n=%d: %d foreground anchors, ambiguous share %.4f %%, worst |got - ref| / bound %.3f (%s) over %d parameters"
          % (tag, kind, K, imgs.shape[0], fg, 100 * amb, worst[top], top, len(worst)))
    assert worst[top] <= 1.0, {k: v for k, v in worst.items() if v > 1.0}
    return m


def _images(n, size, seed):
    from demonet_amd import synth
    return torch.from_numpy(synth.images(seed, n, size, size)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,K,boxes", [(V3, 21, (2, 0, 5)), (V3, 91, (3, 6)), (V2, 21, (4, 2))])
def test_model_gradients_within_bound(kind, K, boxes):
    _check_model(kind, K, _images(len(boxes), 320, 91), _targets(boxes, K))


@pytest.mark.gpu
def test_model_gradients_batch64_two_chains():
    """64 images run as two sub-batch chains (a level tensor is two pieces); 5 - 12 boxes per image give several hundred foreground
    anchors: the loss gradient is then ~1e-3 and below, the small-dy regime"""
    boxes = tuple(5 + (i * 3) % 8 for i in range(64))
    m = _check_model(V3, 21, _images(64, 320, 7), _targets(boxes, 21, seed=5), tag="batch64")
    assert m.batch_split(64) >= 2


@pytest.mark.gpu
def test_model_gradients_large_vocabulary():
    _check_model(V3, 1204, _images(2, 320, 11), _targets((4, 7), 1204), levels=(0, 5), tag="lvis")


@pytest.mark.gpu
def test_sgd_on_the_heads_and_eval_afterwards():
    K = 21
    m = _model(V3, K).cuda()
    imgs, targets = _images(4, 320, 13), _targets((3, 1, 6, 2), K, seed=9)
    m.train()
    with pytest.raises(NotImplementedError, match="train_heads"):
        m(list(imgs), targets)
    m.train_heads()
    opt = torch.optim.SGD(m.head_parameters().values(), lr=0.02)
    history = []
    m.eval()
    m(list(imgs))                      # builds the plan
    m.train()
    gen = m._plan_gen
    for _ in range(20):
        losses = m(list(imgs), targets)
        opt.zero_grad(set_to_none=True)
        (losses["bbox_regression"] + losses["classification"]).backward()
        assert all(bool(torch.isfinite(p.grad).all()) for p in m.head_parameters().values())
        assert all(p.grad is None for k, p in m.named_parameters() if not k.startswith("head."))
        opt.step()
        history.append({k: v.item() for k, v in losses.items()})
        assert m._plan_gen == gen, "an optimizer step on the heads rebuilt the plan"
    print("SGD on the heads, 20 steps:", history[0], "->", history[-1])
    for k in ("bbox_regression", "classification"):
        assert history[-1][k] < history[0][k], (k, history[0][k], history[-1][k])
    m.eval()
    got = m(list(imgs))
    assert m._plan_gen == gen + 1       # the trained heads are lowered once
    m(list(imgs))
    assert m._plan_gen == gen + 1
    fresh = _model(V3, K, seed=5)
    fresh.load_state_dict(m.state_dict())
    want = fresh.cuda().eval()(list(imgs))
    for a, b in zip(got, want):
        for k in ("boxes", "scores", "labels"):
            assert torch.equal(a[k], b[k]), k
    # and the loss the trained plan reports is the last training state's
    with torch.no_grad():
        after = m.loss(imgs, targets)
    assert after["classification"].item() < history[0]["classification"]


@pytest.mark.gpu
def test_backward_after_another_forward_raises():
    m = _model(V3, 21).cuda().train_heads()
    imgs, targets = _images(2, 320, 3), _targets((2, 3), 21)
    losses = m.loss(imgs, targets)
    with torch.no_grad():
        m.loss(imgs, targets)
    with pytest.raises(RuntimeError, match="another forward"):
        losses["classification"].backward()
