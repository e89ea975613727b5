"""Gradient of the SSD training loss with respect to both head outputs (dn_ssd_loss_train / dn_ssd_loss_backward, the
autograd Function behind demonet_amd.loss.ssd_loss) against autograd of the oracle (oracle/ssd_oracle.py:ssd_loss_oracle) on the CPU
with logits and regressions in float64 and anchors and target boxes left in float32 (casting those too would move IoUs across the
matching threshold). Upstream gradients (0.7, 1.3).

Which rows carry a gradient is index work: exact. Values: max|g_hip - g64| <= 4 x max|g32 - g64| + 2^-22 max|g64| per tensor, where
g32 is the oracle's own float32 autograd on the same inputs (computed here, per case): a different but equally valid fp32 summation
order may lose a couple of bits more than torch's, a wrong 1/N or a missing log-sum-exp loses far more than 4 x."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ssd_oracle as so  # noqa: E402

G_BOX, G_CLS = 0.7, 1.3
NEW_SYMBOLS = ("dn_ssd_loss_state_bytes", "dn_ssd_loss_train", "dn_ssd_loss_backward")
# the four parameter sets of test_loss.py::test_hip_loss_vs_oracle_random, plus an LVIS-size vocabulary
RANDOM = [(2, 3234, 91, [3, 7], 3.0), (3, 777, 21, [0, 1, 40], 3.0), (1, 500, 5, [200], 3.0), (2, 3000, 21, [12, 5], 2.5),
          (4, 3234, 1204, [5, 9, 2, 30], 3.0)]
CASES = ["random%d" % i for i in range(len(RANDOM))] + ["golden%d" % i for i in range(4)]
# rows with a non-zero logit gradient, per case (the float32 and the float64 oracle agree on them: test_inputs_have_no_ties_at_the_cut)
SELECTED_ROWS = {"random0": 300, "random1": 340, "random2": 500, "random3": 438, "random4": 1452,
                 "golden0": 460, "golden1": 164, "golden2": 1108, "golden3": 2956}


def _random_case(n, A, K, gmaxs, ratio):
    """the construction of test_loss.py::test_hip_loss_vs_oracle_random"""
    rng = np.random.RandomState(n * 1000 + A)
    c = rng.uniform(0, 300, (A, 2)).astype(np.float32)
    wh = rng.uniform(10, 120, (A, 2)).astype(np.float32)
    anchors = torch.from_numpy(np.concatenate([c - wh / 2, c + wh / 2], 1))
    logits = torch.from_numpy(rng.randn(n, A, K).astype(np.float32) * 3)
    reg = torch.from_numpy(rng.randn(n, A, 4).astype(np.float32))
    targets = []
    for gcount in gmaxs:
        if gcount and A == 500:
            idx = rng.choice(A, gcount, replace=False)
            b = anchors[idx].clone()
        else:
            xy = rng.uniform(0, 250, (gcount, 2)).astype(np.float32)
            b = torch.from_numpy(np.concatenate([xy, xy + rng.uniform(8, 150, (gcount, 2)).astype(np.float32)], 1))
        targets.append({"boxes": b.reshape(-1, 4), "labels": torch.from_numpy(rng.randint(1, K, (gcount,)).astype(np.int64))})
    return anchors, logits, reg, targets, 0.5, ratio


@functools.lru_cache(maxsize=None)
def _case(name):
    """(anchors, logits, reg, targets, iou_thresh, neg_to_pos_ratio), all on the CPU"""
    if name.startswith("random"):
        return _random_case(*RANDOM[int(name[6:])])
    from test_loss import _cases
    for ci, g, anchors, logits, reg, targets in _cases():
        if ci == int(name[6:]):
            return anchors, logits, reg, targets, float(g["iou_thresh"]), float(g["neg_to_pos_ratio"])
    raise KeyError(name)


def _oracle_grads(case, dtype, g_box=G_BOX, g_cls=G_CLS):
    anchors, logits, reg, targets, iou, ratio = case
    lg = logits.to(dtype, copy=True).requires_grad_(True)           # a copy: the cached case tensors stay plain data
    rg = reg.to(dtype, copy=True).requires_grad_(True)
    losses, matched = so.ssd_loss_oracle(lg, rg, anchors, targets, iou, ratio)
    (g_box * losses["bbox_regression"] + g_cls * losses["classification"]).backward()
    glg = lg.grad if lg.grad is not None else torch.zeros_like(lg)
    grg = rg.grad if rg.grad is not None else torch.zeros_like(rg)
    return glg, grg, matched


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """float64 gradients, the float32 autograd's own error against them, and the row sets"""
    g64l, g64r, matched = _oracle_grads(_case(name), torch.float64)
    g32l, g32r, _ = _oracle_grads(_case(name), torch.float32)
    return dict(glg=g64l, grg=g64r, matched=matched, rows=(g64l != 0).any(-1), anchors=(g64r != 0).any(-1), rows32=(g32l != 0).any(-1),
                anchors32=(g32r != 0).any(-1), err_lg=(g32l.double() - g64l).abs().max().item(), err_rg=(g32r.double() - g64r).abs().max().item())


# ---- CPU -------------------------------------------------------------------------------------------------------------------------

def test_new_symbols_exported_and_declared():
    """the built library exports the training entry points, the header declares them, the binding lists them"""
    from demonet_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB]).decode()
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "demonet_hip.h")).read()
    declared = set(re.findall(r"DN_API\s+[\w\s\*]+?\b(dn_\w+)\s*\(", header))
    for sym in NEW_SYMBOLS:
        assert sym in exported, sym
        assert sym in declared, sym
        assert sym in _lib.EXPORTS, sym
    L = _lib.lib()
    assert L.dn_ssd_loss_state_bytes(2, 3234) >= 2 * 3234 * 9 + 4


@pytest.mark.parametrize("name", CASES)
def test_inputs_have_no_ties_at_the_cut(name):
    """Condition on the inputs of the parity tests: the float32 and the float64 oracle mine the same negatives, so 'which rows' is
    exact index work and not a matter of rounding."""
    o = _oracle(name)
    assert torch.equal(o["rows"], o["rows32"]) and torch.equal(o["anchors"], o["anchors32"])
    assert int(o["rows"].sum()) == SELECTED_ROWS[name]
    assert torch.equal(o["anchors"], o["matched"] >= 0)
    print(f"{name}: {int(o['rows'].sum())} rows, fp32 autograd error {o['err_lg']:.3e} (logits, max|g| {o['glg'].abs().max().item():.3e}) "
          f"{o['err_rg']:.3e} (regressions, max|g| {o['grg'].abs().max().item():.3e})")


def _row_weights(case, glg64, matched):
    """w per row, recovered from the oracle's gradient at the target class: g[target] = g_cls * w * (p[target] - 1) / N"""
    anchors, logits, reg, targets, iou, ratio = case
    N = max(1, int((matched >= 0).sum()))
    p = torch.softmax(logits.double(), -1)
    lab = torch.zeros(matched.shape, dtype=torch.int64)
    for i, t in enumerate(targets):
        fg = matched[i] >= 0
        lab[i, fg] = t["labels"][matched[i][fg]]
    w = glg64.gather(-1, lab[..., None])[..., 0] / ((p.gather(-1, lab[..., None])[..., 0] - 1.0) * G_CLS / N)
    return w.round().long()


def _partial_spill_case():
    """A = 500, 70 boxes that are exact anchors: 140 foreground anchors, 420 negatives wanted, 360 exist -- the first 60 foreground
    anchors by index count twice, the other 80 once"""
    rng = np.random.RandomState(570)
    A, K = 500, 5
    c = rng.uniform(0, 300, (A, 2)).astype(np.float32)
    wh = rng.uniform(10, 120, (A, 2)).astype(np.float32)
    anchors = torch.from_numpy(np.concatenate([c - wh / 2, c + wh / 2], 1))
    idx = rng.choice(A, 70, replace=False)
    targets = [{"boxes": anchors[idx].clone(), "labels": torch.from_numpy(rng.randint(1, K, (70,)).astype(np.int64))}]
    return (anchors, torch.from_numpy(rng.randn(1, A, K).astype(np.float32) * 3), torch.from_numpy(rng.randn(1, A, 4).astype(np.float32)), targets,
            0.5, 3.0)


def test_spill_cases_count_foreground_rows_twice_in_the_oracle():
    """random2 (A = 500, 200 boxes) is the spill corner with every foreground row at w = 2; the partial case has w = 2 on the first
    60 foreground anchors by index only. The GPU parity tests on these two therefore exercise w = 2 and where it stops."""
    o = _oracle("random2")
    w = _row_weights(_case("random2"), o["glg"], o["matched"])
    fg = o["matched"] >= 0
    assert int(fg.sum()) > 0 and (w[fg] == 2).all() and (w[~fg] == 1).all()
    case = _partial_spill_case()
    glg, _, matched = _oracle_grads(case, torch.float64)
    w = _row_weights(case, glg, matched)
    fg = torch.where(matched[0] >= 0)[0]
    assert fg.numel() == 140 and (w[0, fg[:60]] == 2).all() and (w[0, fg[60:]] == 1).all() and (w[matched < 0] == 1).all()


# ---- GPU -------------------------------------------------------------------------------------------------------------------------

def _pack_targets(targets, dev):
    n = len(targets)
    gmax = max(1, max(int(t["boxes"].shape[0]) for t in targets))
    gb = torch.zeros((n, gmax, 4), dtype=torch.float32, device=dev)
    gl = torch.zeros((n, gmax), dtype=torch.int64, device=dev)
    gc = torch.zeros((n,), dtype=torch.int32, device=dev)
    for i, t in enumerate(targets):
        g = int(t["boxes"].shape[0])
        if g:
            gb[i, :g] = t["boxes"].to(dev, torch.float32)
            gl[i, :g] = t["labels"].to(dev, torch.int64)
        gc[i] = g
    return gb, gl, gc, gmax


def _abi_run(case, g_box=G_BOX, g_cls=G_CLS, want_cls=True, want_box=True):
    """dn_ssd_loss, dn_ssd_loss_train and dn_ssd_loss_backward through the C ABI; the gradient buffers are pre-filled with NaN"""
    from demonet_amd import _lib
    anchors, logits, reg, targets, iou, ratio = case
    dev = torch.device("cuda")
    L = _lib.lib()
    lg, rg, an = logits.to(dev), reg.to(dev), anchors.to(dev)
    n, A, K = lg.shape
    gb, gl, gc, gmax = _pack_targets(targets, dev)
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(int(L.dn_ssd_loss_workspace_bytes(n, A)), dtype=torch.uint8, device=dev)
    state = torch.empty(int(L.dn_ssd_loss_state_bytes(n, A)), dtype=torch.uint8, device=dev)
    m0, m1 = torch.empty((n, A), dtype=torch.int64, device=dev), torch.empty((n, A), dtype=torch.int64, device=dev)
    l0, l1 = torch.empty(2, device=dev), torch.empty(2, device=dev)
    _lib.check(L.dn_ssd_loss(P(lg), P(rg), P(an), P(gb), P(gl), P(gc), n, A, K, gmax, iou, ratio, P(m0), P(l0), P(ws), ws.numel(), s), "dn_ssd_loss")
    _lib.check(L.dn_ssd_loss_train(P(lg), P(rg), P(an), P(gb), P(gl), P(gc), n, A, K, gmax, iou, ratio, P(m1), P(l1), P(ws), ws.numel(), P(state),
                                   state.numel(), s), "dn_ssd_loss_train")
    up = torch.tensor([g_box, g_cls], dtype=torch.float32, device=dev)
    glg = torch.full_like(lg, float("nan")) if want_cls else None
    grg = torch.full_like(rg, float("nan")) if want_box else None
    _lib.check(L.dn_ssd_loss_backward(P(lg), P(rg), P(an), P(gb), P(gl), P(state), state.numel(), P(up), n, A, K, gmax, P(glg), P(grg), s),
               "dn_ssd_loss_backward")
    torch.cuda.synchronize()
    return dict(l0=l0, l1=l1, m0=m0, m1=m1, glg=glg, grg=grg)


def _autograd_run(case, g_box=G_BOX, g_cls=G_CLS, logits_grad=True, reg_grad=True, prepare=None):
    """the public path: ssd_loss(...) then backward(); returns (losses, matched, logits leaf, reg leaf)"""
    from demonet_amd.loss import ssd_loss
    anchors, logits, reg, targets, iou, ratio = case
    lg = logits.cuda().requires_grad_(logits_grad)
    rg = reg.cuda().requires_grad_(reg_grad)
    ho = {"cls_logits": lg, "bbox_regression": rg}
    if prepare is not None:
        lg, rg, ho = prepare(lg, rg)
    losses, matched = ssd_loss(ho, anchors.cuda(), targets, iou, ratio)
    (g_box * losses["bbox_regression"] + g_cls * losses["classification"]).backward()
    torch.cuda.synchronize()
    return losses, matched, lg, rg


def _check_against_oracle(name, glg, grg):
    o = _oracle(name)
    glg, grg = glg.detach().cpu(), grg.detach().cpu()
    # 1. which rows: exact
    assert not torch.isnan(glg).any() and not torch.isnan(grg).any(), "a gradient buffer was not fully written"
    assert torch.equal((glg != 0).any(-1), o["rows"]), name
    assert torch.equal((grg != 0).any(-1), o["anchors"]), name
    assert (glg[~o["rows"]] == 0).all() and (grg[~o["anchors"]] == 0).all()
    # 2. values: 4 x the oracle's own float32 error + 1.5 ulp of the largest gradient
    for what, got, want, e32 in (("cls_logits", glg, o["glg"], o["err_lg"]), ("bbox_regression", grg, o["grg"], o["err_rg"])):
        err = (got.double() - want).abs().max().item()
        bound = 4.0 * e32 + 2.0 ** -22 * want.abs().max().item()
        print(f"{name} d/d{what}: max|g_hip - g64| {err:.3e}, oracle fp32 {e32:.3e}, ratio {err / e32 if e32 else float('nan'):.2f}, "
              f"bound {bound:.3e}, max|g64| {want.abs().max().item():.3e}")
        assert err <= bound, (name, what, err, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_gradients_vs_oracle(name):
    """(1) rows and (2) values through the C ABI with NaN pre-filled buffers; (5) dn_ssd_loss_train's losses and matched indices are
    bit-equal to dn_ssd_loss's."""
    r = _abi_run(_case(name))
    assert torch.equal(r["m0"], r["m1"]) and np.array_equal(r["m1"].cpu().numpy(), _oracle(name)["matched"].numpy())
    assert r["l0"].cpu().numpy().tobytes() == r["l1"].cpu().numpy().tobytes()
    _check_against_oracle(name, r["glg"], r["grg"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["random0", "random1", "random2", "golden3"])
def test_autograd_path_equals_abi(name):
    """ssd_loss(...).backward() hands over exactly what the C ABI computes, and its value is dn_ssd_loss's"""
    r = _abi_run(_case(name))
    losses, matched, lg, rg = _autograd_run(_case(name))
    assert losses["classification"].grad_fn is not None and losses["bbox_regression"].grad_fn is not None
    assert torch.equal(matched, r["m0"]) and not matched.requires_grad
    assert torch.stack([losses["bbox_regression"], losses["classification"]]).detach().cpu().numpy().tobytes() == r["l0"].cpu().numpy().tobytes()
    assert torch.equal(lg.grad, r["glg"]) and torch.equal(rg.grad, r["grg"])
    _check_against_oracle(name, lg.grad, rg.grad)


def _tie_case():
    rng = np.random.RandomState(777)
    A, K = 777, 21
    c = rng.uniform(0, 300, (A, 2)).astype(np.float32)
    wh = rng.uniform(10, 120, (A, 2)).astype(np.float32)
    anchors = torch.from_numpy(np.concatenate([c - wh / 2, c + wh / 2], 1))
    xy = rng.uniform(0, 250, (2, 2)).astype(np.float32)
    boxes = torch.from_numpy(np.concatenate([xy, xy + rng.uniform(8, 150, (2, 2)).astype(np.float32)], 1))
    targets = [{"boxes": boxes, "labels": torch.tensor([3, 17])}]
    return anchors, torch.zeros(1, A, K), torch.from_numpy(rng.randn(1, A, 4).astype(np.float32)), targets, 0.5, 3.0


def test_tie_case_oracle_takes_the_first_background_anchors():
    """constant logits: every cross entropy is equal; the stable sort mines the first 3 x #foreground background anchors by index"""
    glg, _, matched = _oracle_grads(_tie_case(), torch.float64)
    fg = matched[0] >= 0
    assert int(fg.sum()) >= 2
    want = torch.where(~fg)[0][:3 * int(fg.sum())]
    mined = torch.where((glg[0] != 0).any(-1) & ~fg)[0]
    assert torch.equal(mined, want)


@pytest.mark.gpu
def test_ties_are_mined_in_anchor_order():
    case = _tie_case()
    glg64, grg64, matched = _oracle_grads(case, torch.float64)
    r = _abi_run(case)
    fg = matched[0] >= 0
    rows = (r["glg"].cpu()[0] != 0).any(-1)
    assert torch.equal(torch.where(rows & ~fg)[0], torch.where(~fg)[0][:3 * int(fg.sum())])
    assert torch.equal(rows, (glg64[0] != 0).any(-1))
    assert (r["glg"].cpu().double() - glg64).abs().max().item() <= 2.0 ** -20 * glg64.abs().max().item()


def _small_case(n, A, K, gcounts, seed):
    rng = np.random.RandomState(seed)
    c = rng.uniform(0, 300, (A, 2)).astype(np.float32)
    wh = rng.uniform(10, 120, (A, 2)).astype(np.float32)
    anchors = torch.from_numpy(np.concatenate([c - wh / 2, c + wh / 2], 1))
    targets = []
    for g in gcounts:
        xy = rng.uniform(0, 250, (g, 2)).astype(np.float32)
        b = torch.from_numpy(np.concatenate([xy, xy + rng.uniform(8, 150, (g, 2)).astype(np.float32)], 1)).reshape(-1, 4)
        targets.append({"boxes": b, "labels": torch.from_numpy(rng.randint(1, K, (g,)).astype(np.int64))})
    return (anchors, torch.from_numpy(rng.randn(n, A, K).astype(np.float32) * 3), torch.from_numpy(rng.randn(n, A, 4).astype(np.float32)), targets,
            0.5, 3.0)


def _check_small(case):
    """rows exact, values within the module's bound, for a case built on the spot"""
    g64l, g64r, _ = _oracle_grads(case, torch.float64)
    g32l, g32r, _ = _oracle_grads(case, torch.float32)
    assert torch.equal((g64l != 0).any(-1), (g32l != 0).any(-1))
    r = _abi_run(case)
    for got, want, g32 in ((r["glg"].cpu(), g64l, g32l), (r["grg"].cpu(), g64r, g32r)):
        assert not torch.isnan(got).any()
        assert torch.equal((got != 0).any(-1), (want != 0).any(-1))
        err = (got.double() - want).abs().max().item()
        assert err <= 4.0 * (g32.double() - want).abs().max().item() + 2.0 ** -22 * want.abs().max().item()
    return r


@pytest.mark.gpu
def test_corner_no_boxes_at_all():
    """a batch without a single box: N = 1, nothing is foreground, nothing is mined -- both gradients are zero everywhere"""
    r = _check_small(_small_case(2, 300, 7, [0, 0], 11))
    assert (r["glg"] == 0).all() and (r["grg"] == 0).all() and r["l1"].cpu().tolist() == [0.0, 0.0]


@pytest.mark.gpu
def test_corner_partial_spill():
    _check_small(_partial_spill_case())


@pytest.mark.gpu
@pytest.mark.parametrize("n,A,K,gcounts", [(2, 999, 2, [4, 9]), (3, 65, 3, [1, 0, 2]), (1, 1000, 64, [6]), (1, 1000, 65, [6])])
def test_corner_shapes(n, A, K, gcounts):
    """K = 2; fewer rows than one tile and a ragged last tile; both sides of the 16-lane / 64-lane switch"""
    _check_small(_small_case(n, A, K, gcounts, 100 + K))


@pytest.mark.gpu
def test_corner_only_one_input_requires_grad():
    case = _case("random1")
    _, _, lg, rg = _autograd_run(case)
    _, _, lg1, rg1 = _autograd_run(case, reg_grad=False)
    _, _, lg2, rg2 = _autograd_run(case, logits_grad=False)
    assert rg1.grad is None and lg2.grad is None
    assert torch.equal(lg1.grad, lg.grad) and torch.equal(rg2.grad, rg.grad)
    r = _abi_run(case, want_box=False)
    assert torch.equal(r["glg"], lg.grad)
    r = _abi_run(case, want_cls=False)
    assert torch.equal(r["grg"], rg.grad)


@pytest.mark.gpu
def test_corner_one_upstream_gradient_zero():
    case = _case("random1")
    _, _, lg, rg = _autograd_run(case)
    _, _, lg0, rg0 = _autograd_run(case, g_box=0.0)
    assert (rg0.grad == 0).all() and torch.equal(lg0.grad, lg.grad)
    _, _, lg0, rg0 = _autograd_run(case, g_cls=0.0)
    assert (lg0.grad == 0).all() and torch.equal(rg0.grad, rg.grad)


@pytest.mark.gpu
def test_corner_fp16_and_non_contiguous_inputs():
    """dtype and layout conversion happen in torch ops outside the Function: the gradient arrives in the caller's dtype and layout"""
    case = _case("random1")
    anchors, logits, reg, targets, iou, ratio = case
    half_case = (anchors, logits.half().float(), reg, targets, iou, ratio)
    _, _, lg, rg = _autograd_run(half_case)

    def as_half(lg_leaf, rg_leaf):
        h = lg_leaf.detach().half().requires_grad_(True)
        return h, rg_leaf, {"cls_logits": h, "bbox_regression": rg_leaf}
    _, _, lgh, rgh = _autograd_run(half_case, prepare=as_half)
    assert lgh.grad.dtype == torch.float16 and torch.equal(lgh.grad, lg.grad.half()) and torch.equal(rgh.grad, rg.grad)

    def as_permuted(lg_leaf, rg_leaf):
        store = lg_leaf.detach().permute(0, 2, 1).contiguous().requires_grad_(True)           # [n, K, A] storage
        return store, rg_leaf, {"cls_logits": store.permute(0, 2, 1), "bbox_regression": rg_leaf}
    _, _, store, rgp = _autograd_run(half_case, prepare=as_permuted)
    assert store.grad.shape == store.shape and torch.equal(store.grad.permute(0, 2, 1), lg.grad) and torch.equal(rgp.grad, rg.grad)


@pytest.mark.gpu
def test_corner_non_default_stream_and_determinism():
    case = _case("random3")
    _, _, lg, rg = _autograd_run(case)
    _, _, lg2, rg2 = _autograd_run(case)
    assert lg.grad.cpu().numpy().tobytes() == lg2.grad.cpu().numpy().tobytes() and rg.grad.cpu().numpy().tobytes() == rg2.grad.cpu().numpy().tobytes()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        r = _abi_run(case)
        losses, _, lg3, rg3 = _autograd_run(case)
    s.synchronize()
    assert torch.equal(lg3.grad, lg.grad) and torch.equal(rg3.grad, rg.grad) and torch.equal(r["glg"], lg.grad) and torch.equal(r["grg"], rg.grad)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["random0", "golden1"])
def test_no_grad_paths_return_the_value_bits(name):
    """(5) with no input requiring grad, and under torch.no_grad(), ssd_loss is dn_ssd_loss: no grad_fn, the same bits"""
    from demonet_amd.loss import ssd_loss
    anchors, logits, reg, targets, iou, ratio = _case(name)
    r = _abi_run(_case(name))
    want = r["l0"].cpu().numpy().tobytes()
    losses, matched = ssd_loss({"cls_logits": logits.cuda(), "bbox_regression": reg.cuda()}, anchors.cuda(), targets, iou, ratio)
    with torch.no_grad():
        losses_ng, matched_ng = ssd_loss({"cls_logits": logits.cuda().requires_grad_(True), "bbox_regression": reg.cuda().requires_grad_(True)},
                                         anchors.cuda(), targets, iou, ratio)
    for ls, m in ((losses, matched), (losses_ng, matched_ng)):
        assert ls["classification"].grad_fn is None and ls["bbox_regression"].grad_fn is None
        assert not ls["classification"].requires_grad and not ls["bbox_regression"].requires_grad
        assert torch.stack([ls["bbox_regression"], ls["classification"]]).cpu().numpy().tobytes() == want
        assert torch.equal(m, r["m0"])


@pytest.mark.gpu
def test_it_trains():
    """(6) logits and regressions as free parameters, 20 plain SGD steps through SSD.compute_loss and backward(): both losses go down
    and every gradient is finite. A check of the wiring; parity is test_gradients_vs_oracle."""
    from demonet_amd import models
    anchors, _, _, targets, _, _ = _case("random0")
    m = models.ssdlite320_mobilenet_v3_large(num_classes=21)
    gen = torch.Generator().manual_seed(5)
    lg = (torch.randn(2, 3234, 21, generator=gen)).cuda().requires_grad_(True)
    rg = torch.randn(2, 3234, 4, generator=gen).cuda().requires_grad_(True)
    tg = [{"boxes": t["boxes"], "labels": t["labels"].clamp(max=20)} for t in targets]         # that case draws labels for K = 91
    history = []
    for step in range(21):
        losses = m.compute_loss(tg, {"cls_logits": lg, "bbox_regression": rg}, anchors.cuda())
        history.append((losses["bbox_regression"].item(), losses["classification"].item()))
        if step == 20:
            break
        (losses["bbox_regression"] + losses["classification"]).backward()
        assert torch.isfinite(lg.grad).all() and torch.isfinite(rg.grad).all()
        with torch.no_grad():
            lg -= 10.0 * lg.grad
            rg -= 10.0 * rg.grad
        lg.grad = None
        rg.grad = None
    print("loss (bbox, cls) before / after 20 SGD steps:", history[0], history[-1])
    assert history[-1][0] < history[0][0] and history[-1][1] < history[0][1]
