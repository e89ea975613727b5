"""dev tool: one whole fine-tuning step on the SSDLite heads -- forward, loss, backward, optimizer step, finiteness check -- two ways on one build:
  ours    demonet_amd.optim.SGD and the loop body of engine.train_one_epoch: the loss terms gate the optimizer's launch, the per-step values go into
          a device ring, the host reads ring and gate once per round (print_freq = --reps);
  torch   torch.optim.SGD (its default implementation on the device) and the reference loop's check (demonet/engine.py:39-44): `.item()` on
          the summed loss every step, `math.isfinite`, then zero_grad / backward / step. What a user could write before optim.SGD existed.
    python tools/time_train_step.py [--out profiles/train_step_timing.json] [--reps R] [--rounds Q] [--n 64] [--classes 91] [--max-norm M]
Both sides run SGD with momentum 0.9 and weight decay 1e-4 at lr 1e-3 on their own copy of the model, from a batch already at the network size (the
augmentation is the same call on both sides and is timed by tools/time_augment.py). Timed in one process, alternated round by round: device events
AND the host clock around R steps each (the round ends with the side's own read of the device, so both clocks cover whole steps), Q rounds,
medians; `spread` = (max - min) / median over a side's rounds. Also the optimizer part alone (grad norm + update launches of ours, torch's
step) by device events around the bare calls on the last gradients. One JSON line on stdout (and in --out)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from demonet_amd import models, optim, synth  # noqa: E402


def make_case(n, K):
    m = models.load_synthetic(models.ssdlite320_mobilenet_v3_large(num_classes=K), 0).cuda().train_heads().train()
    imgs = torch.from_numpy(synth.images(17, n, 320, 320)).cuda()
    rng = np.random.RandomState(n + K)
    targets = []
    for i in range(n):
        g = 1 + (i * 7) % 12
        xy = rng.uniform(0, 220, (g, 2)).astype(np.float32)
        b = np.concatenate([xy, xy + rng.uniform(20, 90, (g, 2)).astype(np.float32)], 1)
        targets.append({"boxes": torch.from_numpy(b).cuda(), "labels": torch.from_numpy(rng.randint(1, K, (g,)).astype(np.int64)).cuda()})
    return m, imgs, targets


def _timed(fn, reps, finish):
    """(device ms per step, host ms per step) of reps calls and the side's closing read"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for i in range(reps):
        fn(i)
    finish()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps, (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--classes", type=int, default=91)
    ap.add_argument("--max-norm", type=float, default=None, help="also clip (ours: in the update launch; torch: clip_grad_norm_)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    cfg = dict(lr=1e-3, momentum=0.9, weight_decay=1e-4)
    ma, imgs, targets = make_case(a.n, a.classes)
    mb = make_case(a.n, a.classes)[0]
    ours = optim.SGD(ma.head_parameters().values(), max_norm=a.max_norm, **cfg)
    theirs = torch.optim.SGD(mb.head_parameters().values(), **cfg)
    ring = torch.zeros((a.reps, 4), dtype=torch.float32, device="cuda")

    def ours_step(i):
        loss_dict = ma(imgs, targets)
        losses = loss_dict["bbox_regression"] + loss_dict["classification"]
        row = ring[i % a.reps]
        torch.stack([v.detach() for v in loss_dict.values()] + [losses.detach()], out=row[1:])
        ours.zero_grad()
        losses.backward()
        ours.step(gate=row[1:], norm_out=row[0:1])

    def ours_read():
        host = ring.cpu()
        tripped, at = ours.status()
        assert not tripped and bool(torch.isfinite(host).all()), (tripped, at)

    def torch_step(i):
        loss_dict = mb(imgs, targets)
        losses = loss_dict["bbox_regression"] + loss_dict["classification"]
        loss_value = losses.item()
        assert math.isfinite(loss_value), loss_value
        theirs.zero_grad()
        losses.backward()
        if a.max_norm is not None:
            torch.nn.utils.clip_grad_norm_(list(mb.head_parameters().values()), a.max_norm)
        theirs.step()

    for i in range(3):
        ours_step(i)
        torch_step(i)
    ours_read()
    torch.cuda.synchronize()
    rebuilds0 = ours.table_builds
    dev = {"ours": [], "torch": []}
    host = {"ours": [], "torch": []}
    for _ in range(a.rounds):
        d, h = _timed(ours_step, a.reps, ours_read)
        dev["ours"].append(d)
        host["ours"].append(h)
        d, h = _timed(torch_step, a.reps, torch.cuda.synchronize)
        dev["torch"].append(d)
        host["torch"].append(h)
    # the optimizer part alone, on the gradients of the last step
    opt_only = {}
    for name, fn in (("ours", lambda i: ours.step(gate=ring[0, 1:], norm_out=ring[0, 0:1])), ("torch", lambda i: theirs.step())):
        fn(0)
        opt_only[name] = [round(_timed(fn, 50, torch.cuda.synchronize)[0] * 1e3, 2) for _ in range(5)]
    med = statistics.median
    spread = lambda v: (max(v) - min(v)) / med(v)
    elems = sum(p.numel() for p in ma.head_parameters().values())
    rec = {"tool": "tools/time_train_step.py", "device": torch.cuda.get_device_name(0), "n": a.n, "num_classes": a.classes, "reps": a.reps, "rounds": a.rounds,
           "max_norm": a.max_norm, "head_parameters": len(ma.head_parameters()), "head_parameter_elements": elems,
           "table_builds_while_timed": ours.table_builds - rebuilds0}
    for clock, d in (("device", dev), ("host", host)):
        rec[clock + "_ms_per_step"] = {k: round(med(v), 4) for k, v in d.items()}
        rec[clock + "_rounds_ms"] = {k: [round(x, 4) for x in v] for k, v in d.items()}
        rec[clock + "_spread"] = {k: round(spread(v), 4) for k, v in d.items()}
        rec[clock + "_torch_over_ours"] = round(med(d["torch"]) / med(d["ours"]), 4)
    rec["optimizer_only_us_per_step_rounds"] = opt_only
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
