"""The SSD matcher on tie-rich targets, bit for bit against the real reference (tests/golden/ssd_match_ties.npz, written by
tests/golden/make_match_golden.py: SSDMatcher on box_iou and SSD.compute_loss of a reference model instance, on the default boxes
of all four models). The other loss tests draw boxes from continuous distributions, where two anchors almost never have nearly equal
IoU with a box and no IoU sits at the threshold. Here ground truth copies anchors, halves them (IoU 0.5 in real arithmetic), sits
midway between neighbours, repeats itself and is pixel-aligned: the match is decided by the last bit of an fp32 IoU, so the kernel has
to round inter / (area1 + area2 - inter) operation by operation as the reference's separate torch ops do.

That the fixture can tell is a condition on the fixture, checked on the CPU with a numpy emulation of the match whose union is
either rounded like the reference or once, as a fused multiply-add rounds it (test_single_rounding_emulation_differs_from_the_fixture):
it is stated on the emulation, never on the kernel under test.

Also here: hard negative mining when the cut falls inside a large class of exactly equal cross entropies (logits built from 6
prototype rows), and the 256-boxes-per-image capacity of the matcher.

Bounds: matched indices exact; losses LOSS_RTOL = 2e-5 of the reference's values (tests/test_loss.py); gradients the bound of
tests/test_loss_grad.py, 4 x the oracle's own fp32 error + 2^-22 max|g64|; which rows carry a gradient exact."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ssd_oracle as so  # noqa: E402
from test_loss import LOSS_RTOL  # noqa: E402
from test_loss_grad import G_BOX, G_CLS, _abi_run, _oracle_grads  # noqa: E402

MODELS = ["ssdlite320_mobilenet_v3_large", "ssd_lite_mobilenet_v2", "ssd300_vgg16", "ssd512_vgg16"]
NUM_ANCHORS = {"ssdlite320_mobilenet_v3_large": 3234, "ssd300_vgg16": 8732}
FAMILIES = ("copy", "half", "midpoint", "duplicate", "pixel", "shared")          # the codes of make_match_golden.py
GMAX = 256
DN_E_INVALID = -1


# ---- numpy emulation of the match ------------------------------------------------------------------------------------------------

def emulate_iou(boxes, anchors, fused):
    """[G, A] fp32 IoU, every operation rounded to fp32 as box_iou's separate torch ops round it; with `fused` the union
    (area1 + area2) - w * h is rounded once, as a fused multiply-add of the unrounded product does (float64 holds the product of two
    fp32 exactly)."""
    b, a = boxes.astype(np.float32)[:, None, :], anchors.astype(np.float32)[None]
    area1 = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    area2 = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    w = np.maximum(np.minimum(b[..., 2], a[..., 2]) - np.maximum(b[..., 0], a[..., 0]), np.float32(0))
    h = np.maximum(np.minimum(b[..., 3], a[..., 3]) - np.maximum(b[..., 1], a[..., 1]), np.float32(0))
    inter = w * h
    total = area1 + area2
    assert inter.dtype == np.float32 and total.dtype == np.float32
    union = (total.astype(np.float64) - w.astype(np.float64) * h.astype(np.float64)).astype(np.float32) if fused else total - inter
    return inter / union


def emulate_match(boxes, anchors, iou_thresh, fused):
    """SSDMatcher on emulate_iou: [A] int64"""
    if len(boxes) == 0:
        return np.full(anchors.shape[0], -1, np.int64)
    q = emulate_iou(boxes, anchors, fused)
    m = q.argmax(0).astype(np.int64)                  # first maximum over the gts
    m[q.max(0) < np.float32(iou_thresh)] = -1
    for g, a in enumerate(q.argmax(1)):               # every gt keeps its best anchor (the first maximum); later gts win
        m[a] = g
    return m


# ---- the fixture -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _fixture(golden_dir, name):
    """(case, fixture arrays): case = (anchors, logits, reg, targets, iou_thresh, neg_to_pos_ratio) on the CPU, as test_loss_grad"""
    g = np.load(os.path.join(golden_dir, "ssd_match_ties.npz"))
    anchors = torch.from_numpy(np.load(os.path.join(golden_dir, name + ".npz"))["anchors"].astype(np.float32))
    A, K = anchors.shape[0], int(g["num_classes"])
    cnt = g[name + "_gt_counts"]
    n = len(cnt)
    gen = torch.Generator().manual_seed(int(g[name + "_logits_seed"]))
    logits = torch.randn(n, A, K, generator=gen) * 2.0
    reg = torch.randn(n, A, 4, generator=gen)
    targets = [{"boxes": torch.from_numpy(g[name + "_gt_boxes"][i, :cnt[i]].copy()),
                "labels": torch.from_numpy(g[name + "_gt_labels"][i, :cnt[i]].copy())} for i in range(n)]
    fx = dict(matched=g[name + "_matched"].astype(np.int64), family=g[name + "_family"], counts=cnt,
              bbox_regression=float(g[name + "_bbox_regression"]), classification=float(g[name + "_classification"]))
    assert fx["matched"].shape == (n, A)
    return (anchors, logits, reg, targets, float(g["iou_thresh"]), float(g["neg_to_pos_ratio"])), fx


def _oracle_of(case):
    """float64 gradients, the float32 autograd's own error against them, and the row sets (test_loss_grad._oracle for any case)"""
    g64l, g64r, matched = _oracle_grads(case, torch.float64)
    g32l, g32r, _ = _oracle_grads(case, torch.float32)
    return dict(glg=g64l, grg=g64r, matched=matched, rows=(g64l != 0).any(-1), anchors=(g64r != 0).any(-1), rows32=(g32l != 0).any(-1),
                anchors32=(g32r != 0).any(-1), err_lg=(g32l.double() - g64l).abs().max().item(), err_rg=(g32r.double() - g64r).abs().max().item())


@functools.lru_cache(maxsize=None)
def _fixture_oracle(golden_dir, name):
    return _oracle_of(_fixture(golden_dir, name)[0])


def _check_gradients(what, o, glg, grg):
    """test_loss_grad._check_against_oracle against an oracle record: rows exact, values within 4 x the oracle's own fp32 error +
    2^-22 max|g64|"""
    glg, grg = glg.detach().cpu(), grg.detach().cpu()
    assert not torch.isnan(glg).any() and not torch.isnan(grg).any(), "a gradient buffer was not fully written"
    assert torch.equal((glg != 0).any(-1), o["rows"]), what
    assert torch.equal((grg != 0).any(-1), o["anchors"]), what
    for which, got, want, e32 in (("cls_logits", glg, o["glg"], o["err_lg"]), ("bbox_regression", grg, o["grg"], o["err_rg"])):
        err = (got.double() - want).abs().max().item()
        bound = 4.0 * e32 + 2.0 ** -22 * want.abs().max().item()
        print(f"{what} d/d{which}: max|g_hip - g64| {err:.3e}, oracle fp32 {e32:.3e}, bound {bound:.3e}, max|g64| {want.abs().max().item():.3e}")
        assert err <= bound, (what, which, err, bound)


# ---- CPU: the fixture is what the oracle computes, and it can tell the two roundings apart ---------------------------------------------

def test_fixture_covers_the_four_models(golden_dir):
    g = np.load(os.path.join(golden_dir, "ssd_match_ties.npz"))
    assert list(g["models"]) == MODELS
    for name in MODELS:
        case, fx = _fixture(golden_dir, name)
        A = case[0].shape[0]
        assert NUM_ANCHORS.get(name, A) == A
        cnt = sorted(int(c) for c in fx["counts"])
        assert len(cnt) <= 4 and cnt[0] == 0 and cnt[1] == 1 and cnt[-1] == GMAX          # family (g): a full image next to 0 and 1 box
        fam = fx["family"]
        for i, c in enumerate(fx["counts"]):
            assert (fam[i, c:] == -1).all()
        assert set(np.unique(fam[fam >= 0]).tolist()) == set(range(len(FAMILIES)))
        full = fam[int(np.argmax(fx["counts"]))]
        assert set(np.unique(full).tolist()) == set(range(len(FAMILIES))), "the full image mixes every family"


@pytest.mark.parametrize("name", MODELS)
def test_oracle_reproduces_the_fixture(golden_dir, name):
    (anchors, logits, reg, targets, iou, ratio), fx = _fixture(golden_dir, name)
    losses, matched = so.ssd_loss_oracle(logits, reg, anchors, targets, iou, ratio)
    assert np.array_equal(matched.numpy(), fx["matched"])
    for i, t in enumerate(targets):
        assert np.array_equal(so.ssd_match(t["boxes"], anchors, iou).numpy(), fx["matched"][i])
    for k in ("bbox_regression", "classification"):
        assert abs(losses[k].item() - fx[k]) <= 1e-6 * abs(fx[k]), (k, losses[k].item(), fx[k])


@pytest.mark.parametrize("name", MODELS)
def test_single_rounding_emulation_differs_from_the_fixture(golden_dir, name):
    """Sensitivity condition: with the union rounded operation by operation the emulation IS the fixture; with the union rounded once
    it differs on at least 20 anchors per model, in at least 3 box families. A differing anchor counts for the family of the box the
    fixture matches it to, or, where the fixture has none, of the box the emulation matches it to."""
    (anchors, _, _, targets, iou, _), fx = _fixture(golden_dir, name)
    an = anchors.numpy()
    per_family = np.zeros(len(FAMILIES), np.int64)
    per_image = []
    for i, t in enumerate(targets):
        boxes = t["boxes"].numpy()
        assert np.array_equal(emulate_match(boxes, an, iou, fused=False), fx["matched"][i]), (name, i)
        fused = emulate_match(boxes, an, iou, fused=True)
        d = np.where(fused != fx["matched"][i])[0]
        per_image.append(len(d))
        gt = np.where(fx["matched"][i][d] >= 0, fx["matched"][i][d], fused[d])
        per_family += np.bincount(fx["family"][i][gt], minlength=len(FAMILIES))
    print(f"{name}: single-rounding emulation differs on {int(per_family.sum())} anchors, per image {per_image}, per family "
          + ", ".join(f"{f} {c}" for f, c in zip(FAMILIES, per_family)))
    assert per_family.sum() >= 20
    assert (per_family > 0).sum() >= 3


@pytest.mark.parametrize("name", MODELS)
def test_fixture_has_no_ties_at_the_mining_cut(golden_dir, name):
    """the condition of test_loss_grad.test_inputs_have_no_ties_at_the_cut on the fixture's inputs: 'which rows' is index work"""
    o = _fixture_oracle(golden_dir, name)
    assert torch.equal(o["rows"], o["rows32"]) and torch.equal(o["anchors"], o["anchors32"])
    assert torch.equal(o["anchors"], o["matched"] >= 0)
    assert np.array_equal(o["matched"].numpy(), _fixture(golden_dir, name)[1]["matched"])
    print(f"{name}: {int(o['rows'].sum())} rows, fp32 autograd error {o['err_lg']:.3e} (logits) {o['err_rg']:.3e} (regressions)")


# ---- mining ties: the cut inside a class of equal cross entropies ---------------------------------------------------------------------

PROTOTYPES = 6
MINING = {2: ([40, 25], 4102), 3: ([40, 0, 25], 4103)}          # n -> (boxes per image, seed)


@functools.lru_cache(maxsize=None)
def _mining_case(golden_dir, n):
    """the real 3234 default boxes, K = 21, every anchor's logit row one of 6 prototype rows: a background anchor's cross entropy takes
    one of 6 values exactly, in any implementation that treats every row alike. Returns (case, prototype index [n, A])."""
    counts, seed = MINING[n]
    rng = np.random.RandomState(seed)
    anchors = torch.from_numpy(np.load(os.path.join(golden_dir, MODELS[0] + ".npz"))["anchors"].astype(np.float32))
    A, K = anchors.shape[0], 21
    protos = (rng.randn(PROTOTYPES, K) * 3).astype(np.float32)
    which = rng.randint(0, PROTOTYPES, (n, A))
    logits = torch.from_numpy(protos[which])
    reg = torch.from_numpy(rng.randn(n, A, 4).astype(np.float32))
    targets = []
    for c in counts:
        xy = rng.uniform(0, 250, (c, 2)).astype(np.float32)
        b = torch.from_numpy(np.concatenate([xy, xy + rng.uniform(8, 150, (c, 2)).astype(np.float32)], 1)).reshape(-1, 4)
        targets.append({"boxes": b, "labels": torch.from_numpy(rng.randint(1, K, (c,)).astype(np.int64))})
    return (anchors, logits, reg, targets, 0.5, 3.0), (protos, which)


@functools.lru_cache(maxsize=None)
def _mining_oracle(golden_dir, n):
    return _oracle_of(_mining_case(golden_dir, n)[0])


@pytest.mark.parametrize("n", sorted(MINING))
def test_mining_tie_inputs_cut_inside_a_large_class(golden_dir, n):
    """Condition on the inputs of test_mining_ties: the float32 and the float64 oracle select the same rows; in every image that has
    boxes (one without mines nothing) the cut falls strictly inside a class of equal cross entropies with at least 300 members, of
    which the first in anchor order are taken; in at least one image they reach past anchor 1024, the second pass of the 1024-thread
    kernels."""
    case, (protos, which) = _mining_case(golden_dir, n)
    o = _mining_oracle(golden_dir, n)
    assert torch.equal(o["rows"], o["rows32"]) and torch.equal(o["anchors"], o["anchors32"])
    ce = -torch.log_softmax(torch.from_numpy(protos).double(), -1)[:, 0].numpy()          # a background row's cross entropy per prototype
    assert np.diff(np.sort(ce)).min() > 1e-3
    last_taken = []
    for i, t in enumerate(case[3]):
        fg = o["matched"][i].numpy() >= 0
        rows = o["rows"][i].numpy()
        if len(t["boxes"]) == 0:
            assert not rows.any()
            continue
        want, have = 3 * int(fg.sum()), 0
        for p in np.argsort(-ce):
            members = np.where(~fg & (which[i] == p))[0]
            if have + len(members) >= want:
                break
            assert rows[members].all()
            have += len(members)
        taken = want - have
        assert 0 < taken < len(members) and len(members) >= 300, (i, taken, len(members))
        assert rows[members[:taken]].all() and not rows[members[taken:]].any()
        assert int(rows.sum()) == want + int(fg.sum())
        last_taken.append(int(members[taken - 1]))
        print(f"n={n} image {i}: {int(fg.sum())} foreground, tie class of {len(members)} members, {taken} taken, the last at anchor {members[taken - 1]}")
    assert max(last_taken) > 1024


# ---- GPU -------------------------------------------------------------------------------------------------------------------------

def _poisoned_targets(targets, gmax, dev):
    """rows behind gt_counts[i] hold 1e30 and NaN boxes and label -1: nothing may read them"""
    n = len(targets)
    gb = torch.full((n, gmax, 4), 1e30, dtype=torch.float32)
    gb[:, 1::2] = float("nan")
    gl = torch.full((n, gmax), -1, dtype=torch.int64)
    gc = torch.zeros((n,), dtype=torch.int32)
    for i, t in enumerate(targets):
        g = int(t["boxes"].shape[0])
        gb[i, :g], gl[i, :g], gc[i] = t["boxes"], t["labels"], g
    return gb.to(dev), gl.to(dev), gc.to(dev)


def _abi_forward(case, gmax):
    """dn_ssd_loss with matched_idxs given and dn_ssd_loss_train through the C ABI on poison-padded targets"""
    from demonet_amd import _lib
    anchors, logits, reg, targets, iou, ratio = case
    dev = torch.device("cuda")
    L = _lib.lib()
    lg, rg, an = logits.to(dev), reg.to(dev), anchors.to(dev)
    n, A, K = lg.shape
    gb, gl, gc = _poisoned_targets(targets, gmax, dev)
    P = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(int(L.dn_ssd_loss_workspace_bytes(n, A)), dtype=torch.uint8, device=dev)
    state = torch.empty(int(L.dn_ssd_loss_state_bytes(n, A)), dtype=torch.uint8, device=dev)
    m0, m1 = torch.full((n, A), -7, dtype=torch.int64, device=dev), torch.full((n, A), -7, dtype=torch.int64, device=dev)
    l0, l1 = torch.full((2,), float("nan"), device=dev), torch.full((2,), float("nan"), device=dev)
    _lib.check(L.dn_ssd_loss(P(lg), P(rg), P(an), P(gb), P(gl), P(gc), n, A, K, gmax, iou, ratio, P(m0), P(l0), P(ws), ws.numel(), s), "dn_ssd_loss")
    _lib.check(L.dn_ssd_loss_train(P(lg), P(rg), P(an), P(gb), P(gl), P(gc), n, A, K, gmax, iou, ratio, P(m1), P(l1), P(ws), ws.numel(), P(state),
                                   state.numel(), s), "dn_ssd_loss_train")
    torch.cuda.synchronize()
    return m0.cpu().numpy(), l0.cpu().numpy(), m1.cpu().numpy(), l1.cpu().numpy()


def _report_mismatch(name, what, got, fx):
    d = got != fx["matched"]
    if d.any():
        i, a = np.where(d)
        gt = np.where(fx["matched"][i, a] >= 0, fx["matched"][i, a], got[i, a])
        fam = np.bincount(fx["family"][i, np.clip(gt, 0, None)], minlength=len(FAMILIES))
        print(f"{name} {what}: matched differs from the reference on {int(d.sum())} anchors, per image {np.bincount(i, minlength=len(got)).tolist()}, "
              + "per family " + ", ".join(f"{f} {c}" for f, c in zip(FAMILIES, fam)))
    else:
        print(f"{name} {what}: matched equals the reference on all {got.size} anchors")
    return int(d.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_hip_matching_equals_the_reference_on_ties(golden_dir, name):
    """dn_ssd_loss (matched_idxs given), dn_ssd_loss_train and demonet_amd.loss.ssd_loss: matched bit for bit the reference's, both
    losses within LOSS_RTOL of the reference's, train and plain bit-equal; padding rows are poison. The full image is gmax = 256."""
    from demonet_amd.loss import ssd_loss
    case, fx = _fixture(golden_dir, name)
    anchors, logits, reg, targets, iou, ratio = case
    m0, l0, m1, l1 = _abi_forward(case, GMAX)
    losses, mp = ssd_loss({"cls_logits": logits.cuda(), "bbox_regression": reg.cuda()}, anchors.cuda(), targets, iou, ratio)
    lp = np.array([losses["bbox_regression"].item(), losses["classification"].item()], np.float32)
    wrong = [_report_mismatch(name, what, m, fx) for what, m in (("dn_ssd_loss", m0), ("dn_ssd_loss_train", m1), ("ssd_loss", mp.cpu().numpy()))]
    for what, l in (("dn_ssd_loss", l0), ("dn_ssd_loss_train", l1), ("ssd_loss", lp)):
        print(f"{name} {what}: bbox {l[0]:.7f} (reference {fx['bbox_regression']:.7f}) cls {l[1]:.7f} (reference {fx['classification']:.7f})")
    assert wrong == [0, 0, 0], (name, wrong)
    assert np.array_equal(m0, m1) and l0.tobytes() == l1.tobytes()
    for l in (l0, l1, lp):
        assert abs(float(l[0]) - fx["bbox_regression"]) <= LOSS_RTOL * abs(fx["bbox_regression"])
        assert abs(float(l[1]) - fx["classification"]) <= LOSS_RTOL * abs(fx["classification"])
    assert lp.tobytes() == l0.tobytes(), "zero padding and poison padding give the same bits"


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_hip_gradients_on_the_fixture(golden_dir, name):
    case, fx = _fixture(golden_dir, name)
    o = _fixture_oracle(golden_dir, name)
    assert torch.equal(o["rows"], o["rows32"]) and torch.equal(o["anchors"], o["anchors32"])          # no ties at the cut
    r = _abi_run(case)
    assert np.array_equal(r["m1"].cpu().numpy(), fx["matched"]) and torch.equal(r["m0"], r["m1"])
    _check_gradients(name, o, r["glg"], r["grg"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(MINING))
def test_mining_ties(golden_dir, n):
    """the cut inside a class of several hundred exactly equal cross entropies: the mined rows are the oracle's -- the first members in
    anchor order -- and the gradients hold the module's bound"""
    case, _ = _mining_case(golden_dir, n)
    o = _mining_oracle(golden_dir, n)
    r = _abi_run(case)
    assert np.array_equal(r["m1"].cpu().numpy(), o["matched"].numpy())
    rows = (r["glg"].cpu() != 0).any(-1)
    print(f"n={n}: rows selected per image {rows.sum(1).tolist()}, oracle {o['rows'].sum(1).tolist()}")
    assert torch.equal(rows, o["rows"])
    _check_gradients(f"mining ties n={n}", o, r["glg"], r["grg"])


@pytest.mark.gpu
def test_more_boxes_than_the_matcher_holds_is_an_error():
    """gmax = 257: DN_E_INVALID from all three entry points before anything is launched, dn_last_error names gmax; ssd_loss raises
    ValueError for an image with 257 boxes. gmax = 256 with a full image is test_hip_matching_equals_the_reference_on_ties."""
    from demonet_amd import _lib
    from demonet_amd.loss import ssd_loss
    L = _lib.lib()
    dev = torch.device("cuda")
    n, A, K, gmax = 1, 64, 3, GMAX + 1
    rng = np.random.RandomState(257)
    xy = rng.uniform(0, 200, (A, 2)).astype(np.float32)
    anchors = torch.from_numpy(np.concatenate([xy, xy + rng.uniform(10, 90, (A, 2)).astype(np.float32)], 1)).to(dev)
    bxy = rng.uniform(0, 200, (gmax, 2)).astype(np.float32)
    boxes = torch.from_numpy(np.concatenate([bxy, bxy + rng.uniform(10, 90, (gmax, 2)).astype(np.float32)], 1))
    labels = torch.from_numpy(rng.randint(1, K, (gmax,)).astype(np.int64))
    lg, rg = torch.zeros(n, A, K, device=dev), torch.zeros(n, A, 4, device=dev)
    gb, gl, gc = boxes[None].to(dev), labels[None].to(dev), torch.tensor([gmax], dtype=torch.int32, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(int(L.dn_ssd_loss_workspace_bytes(n, A)), dtype=torch.uint8, device=dev)
    state = torch.zeros(int(L.dn_ssd_loss_state_bytes(n, A)), dtype=torch.uint8, device=dev)
    m, l, up = torch.empty((n, A), dtype=torch.int64, device=dev), torch.empty(2, device=dev), torch.ones(2, device=dev)
    glg, grg = torch.empty_like(lg), torch.empty_like(rg)
    calls = {
        "dn_ssd_loss": lambda: L.dn_ssd_loss(P(lg), P(rg), P(anchors), P(gb), P(gl), P(gc), n, A, K, gmax, 0.5, 3.0, P(m), P(l), P(ws), ws.numel(), s),
        "dn_ssd_loss_train": lambda: L.dn_ssd_loss_train(P(lg), P(rg), P(anchors), P(gb), P(gl), P(gc), n, A, K, gmax, 0.5, 3.0, P(m), P(l), P(ws),
                                                         ws.numel(), P(state), state.numel(), s),
        "dn_ssd_loss_backward": lambda: L.dn_ssd_loss_backward(P(lg), P(rg), P(anchors), P(gb), P(gl), P(state), state.numel(), P(up), n, A, K, gmax,
                                                               P(glg), P(grg), s),
    }
    for what, call in calls.items():
        assert call() == DN_E_INVALID, what
        msg = L.dn_last_error().decode()
        assert "gmax" in msg and what in msg, (what, msg)
    with pytest.raises(ValueError):
        ssd_loss({"cls_logits": lg, "bbox_regression": rg}, anchors, [{"boxes": boxes, "labels": labels}])
    torch.cuda.synchronize()
