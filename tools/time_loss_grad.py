"""dev tool: value + gradient of the SSD loss through demonet_amd.loss.ssd_loss(...) and backward() (dn_ssd_loss_train +
dn_ssd_loss_backward) against a restatement of the reference's compute_loss in torch ops on the same device (cross_entropy, the two
sorts, smooth_l1_loss, autograd), given the same matched indices.
    python tools/time_loss_grad.py [--out FILE] [--reps R] [--rounds Q]
Per shape -- n=64 A=3234 K=91, n=64 A=3234 K=21, n=16 A=3234 K=1204 --:
  * the two versions are first checked against each other (loss values rtol 2e-5, gradients to 1e-5 of the largest gradient),
  * then timed in one process, alternated round by round: device events around R calls of value + backward each, Q rounds, the
    median round per version (the HIP path includes the host work of ssd_loss: target packing and validation),
  * the backward launch alone (dn_ssd_loss_backward through the C ABI, device events around R calls), with its ALGORITHMIC bytes from
    the shapes -- zeros written for the rows without a gradient, the selected rows read and written once, regressions read and their
    gradient written, matched indices and weights read -- and that figure's share of the 8 TB/s HBM peak. Bytes the kernel moves
    beyond those (the selected rows are read three times, from cache after the first) are not in it.
One JSON line on stdout (and in --out): {"shapes": [one record per shape]}."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from demonet_amd import _lib  # noqa: E402
from demonet_amd.loss import ssd_loss  # noqa: E402

SHAPES = [(64, 3234, 91), (64, 3234, 21), (16, 3234, 1204)]
HBM_PEAK_GBS = 8000.0


def make_inputs(n, A, K, seed=0):
    rng = np.random.RandomState(seed)
    c = rng.uniform(0, 300, (A, 2)).astype(np.float32)
    wh = rng.uniform(10, 120, (A, 2)).astype(np.float32)
    anchors = torch.from_numpy(np.concatenate([c - wh / 2, c + wh / 2], 1)).cuda()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    logits = torch.randn(n, A, K, generator=gen, device="cuda") * 3
    reg = torch.randn(n, A, 4, generator=gen, device="cuda")
    targets = []
    for i in range(n):
        g = 1 + (i * 7) % 12
        xy = rng.uniform(0, 250, (g, 2)).astype(np.float32)
        b = np.concatenate([xy, xy + rng.uniform(8, 150, (g, 2)).astype(np.float32)], 1)
        targets.append({"boxes": torch.from_numpy(b).cuda(), "labels": torch.from_numpy(rng.randint(1, K, (g,)).astype(np.int64)).cuda()})
    return anchors, logits, reg, targets


def encode(gt, anchors):
    ew, eh = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
    ecx, ecy = anchors[:, 0] + 0.5 * ew, anchors[:, 1] + 0.5 * eh
    gw, gh = gt[:, 2] - gt[:, 0], gt[:, 3] - gt[:, 1]
    gcx, gcy = gt[:, 0] + 0.5 * gw, gt[:, 1] + 0.5 * gh
    return torch.stack([10.0 * (gcx - ecx) / ew, 10.0 * (gcy - ecy) / eh, 5.0 * torch.log(gw / ew), 5.0 * torch.log(gh / eh)], dim=1)


def torch_loss(logits, reg, anchors, targets, matched, neg_to_pos_ratio=3.0):
    """SSD.compute_loss in torch ops: a Python loop per image, cross entropy over every row, two sorts of [n, A]"""
    n, A, K = logits.shape
    num_foreground, bbox_loss, cls_targets = 0, [], []
    for i, t in enumerate(targets):
        fg = torch.where(matched[i] >= 0)[0]
        mi = matched[i][fg]
        num_foreground += mi.numel()
        bbox_loss.append(F.smooth_l1_loss(reg[i][fg], encode(t["boxes"][mi], anchors[fg]), reduction="sum"))
        ct = torch.zeros((A,), dtype=torch.int64, device=logits.device)
        ct[fg] = t["labels"][mi]
        cls_targets.append(ct)
    cls_targets = torch.stack(cls_targets)
    cls_loss = F.cross_entropy(logits.reshape(-1, K), cls_targets.reshape(-1), reduction="none").view(n, A)
    fgm = cls_targets > 0
    num_negative = neg_to_pos_ratio * fgm.sum(1, keepdim=True)
    neg = cls_loss.clone()
    neg[fgm] = -float("inf")
    _, idx = neg.sort(1, descending=True)
    bgm = idx.sort(1)[1] < num_negative
    N = max(1, num_foreground)
    return {"bbox_regression": torch.stack(bbox_loss).sum() / N, "classification": (cls_loss[fgm].sum() + cls_loss[bgm].sum()) / N}


def _events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def backward_alg_bytes(n, A, K, selected_rows, matched_anchors):
    rows = n * A
    zeros = (rows - selected_rows) * K * 4
    selected = selected_rows * K * 4 * 2
    regressions = rows * 16 + matched_anchors * 16                    # gradient written everywhere, regressions read where matched
    index = rows * (8 + 1)                                            # matched index, weight
    return zeros + selected + regressions + index


def run(n, A, K, reps, rounds):
    anchors, logits, reg, targets = make_inputs(n, A, K)
    lg, rg = logits.clone().requires_grad_(True), reg.clone().requires_grad_(True)

    def hip_step():
        losses, _ = ssd_loss({"cls_logits": lg, "bbox_regression": rg}, anchors, targets)
        lg.grad = rg.grad = None
        (losses["bbox_regression"] + losses["classification"]).backward()
        return losses

    with torch.no_grad():
        _, matched = ssd_loss({"cls_logits": logits, "bbox_regression": reg}, anchors, targets)

    lt, rt = logits.clone().requires_grad_(True), reg.clone().requires_grad_(True)

    def torch_step():
        losses = torch_loss(lt, rt, anchors, targets, matched)
        lt.grad = rt.grad = None
        (losses["bbox_regression"] + losses["classification"]).backward()
        return losses

    # the two versions agree before either is timed
    a, b = hip_step(), torch_step()
    for k in a:
        assert abs(a[k].item() - b[k].item()) <= 2e-5 * abs(b[k].item()) + 1e-7, (k, a[k].item(), b[k].item())
    for got, want in ((lg.grad, lt.grad), (rg.grad, rt.grad)):
        assert (got - want).abs().max().item() <= 1e-5 * want.abs().max().item(), (got - want).abs().max().item()
    selected_rows = int((lg.grad != 0).any(-1).sum())
    matched_anchors = int((matched >= 0).sum())
    for _ in range(3):
        hip_step()
        torch_step()
    torch.cuda.synchronize()
    hip_ms, torch_ms = [], []
    for _ in range(rounds):
        hip_ms.append(_events_ms(hip_step, reps))
        torch_ms.append(_events_ms(torch_step, reps))

    # the backward launch alone, through the C ABI
    L = _lib.lib()
    P = lambda t: C.c_void_p(t.data_ptr())
    gmax = max(int(t["boxes"].shape[0]) for t in targets)
    gb = torch.zeros((n, gmax, 4), device="cuda")
    gl = torch.zeros((n, gmax), dtype=torch.int64, device="cuda")
    gc = torch.zeros((n,), dtype=torch.int32, device="cuda")
    for i, t in enumerate(targets):
        g = int(t["boxes"].shape[0])
        gb[i, :g], gl[i, :g], gc[i] = t["boxes"], t["labels"], g
    ws = torch.empty(int(L.dn_ssd_loss_workspace_bytes(n, A)), dtype=torch.uint8, device="cuda")
    state = torch.empty(int(L.dn_ssd_loss_state_bytes(n, A)), dtype=torch.uint8, device="cuda")
    losses = torch.empty(2, device="cuda")
    up = torch.ones(2, device="cuda")
    glg, grg = torch.empty_like(logits), torch.empty_like(reg)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    value = lambda: _lib.check(L.dn_ssd_loss_train(P(logits), P(reg), P(anchors), P(gb), P(gl), P(gc), n, A, K, gmax, 0.5, 3.0, None, P(losses), P(ws),
                                                   ws.numel(), P(state), state.numel(), s), "dn_ssd_loss_train")
    back = lambda: _lib.check(L.dn_ssd_loss_backward(P(logits), P(reg), P(anchors), P(gb), P(gl), P(state), state.numel(), P(up), n, A, K, gmax,
                                                     P(glg), P(grg), s), "dn_ssd_loss_backward")
    for _ in range(3):
        value()
        back()
    torch.cuda.synchronize()
    assert torch.equal(glg, lg.grad) and torch.equal(grg, rg.grad)
    value_ms = statistics.median(_events_ms(value, reps * 5) for _ in range(rounds))
    back_ms = statistics.median(_events_ms(back, reps * 5) for _ in range(rounds))
    alg = backward_alg_bytes(n, A, K, selected_rows, matched_anchors)
    gbs = alg / (back_ms * 1e-3) / 1e9
    return dict(n=n, anchors=A, num_classes=K, selected_rows=selected_rows, matched_anchors=matched_anchors, reps=reps, rounds=rounds,
                hip_value_and_grad_ms=round(statistics.median(hip_ms), 4), torch_value_and_grad_ms=round(statistics.median(torch_ms), 4),
                hip_rounds_ms=[round(x, 4) for x in hip_ms], torch_rounds_ms=[round(x, 4) for x in torch_ms],
                speedup=round(statistics.median(torch_ms) / statistics.median(hip_ms), 2), value_launches_ms=round(value_ms, 4),
                backward_launch_ms=round(back_ms, 4), backward_alg_bytes=alg, backward_alg_gbs=round(gbs, 1),
                backward_share_of_hbm_peak_on_alg_bytes=round(gbs / HBM_PEAK_GBS, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    rows = []
    for n, A, K in SHAPES:
        r = run(n, A, K, a.reps, a.rounds)
        print({k: r[k] for k in ("n", "num_classes", "hip_value_and_grad_ms", "torch_value_and_grad_ms", "backward_launch_ms")}, file=sys.stderr, flush=True)
        rows.append(r)
        torch.cuda.empty_cache()
    line = json.dumps({"tool": "tools/time_loss_grad.py", "device": torch.cuda.get_device_name(0), "shapes": rows})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
