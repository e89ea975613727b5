"""dev tool: one training step on the SSDLite heads -- features -> head forward -> loss -> backward to the head parameters -- through
SSD.loss(...).backward() (demonet_amd/headgrad.py: dn_forward_features, the launch-per-layer head, dn_ssd_loss_train / _backward,
dn_lite_head_backward) against the same step with the head restated in torch ops on the same device: the same features from the plan,
copied to NCHW fp32, F.conv2d / F.batch_norm(training=False) / F.relu6, autograd, the same loss call.
    python tools/time_head_grad.py [--out FILE] [--reps R] [--rounds Q] [--kernel-stats CSV]
    python tools/time_head_grad.py --profile-step N K [--steps S]      (S steps of one shape and nothing else: the run to put under
                                                                        rocprofv3 --kernel-trace --stats; its CSV is what --kernel-stats reads)
Per shape -- (64 images, K = 91), (64, 21), (16, 1204) --:
  * the hand-written gradients are first checked against the float64 reference within the derived bound of tests/head_grad_ref.py
    (levels 1 and 5 only at K = 1204: the bound of level 0 is minutes of float64 matrix products on the host), and the torch-ops
    gradients, for the same upstream gradient, against the same reference to 1e-3 of each tensor's largest gradient;
  * then both steps are timed in one process, alternated round by round: device events around R steps each, Q rounds, medians;
  * MFMA FLOPs the two matrix kernels issue per step, from the shapes (every 32x32x16 instruction counts 32768, zero padding included);
    with --kernel-stats also each new kernel's time per step and, for the two matrix kernels, their share of the fp16 MFMA peak that
    bench.py's roofline uses.
One JSON line on stdout (and in --out)."""
import argparse
import csv
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT):
    sys.path.insert(0, p)
import head_grad_ref as hr  # noqa: E402
from demonet_amd import headgrad, models, synth  # noqa: E402

SHAPES = [(64, 91), (64, 21), (16, 1204)]
NEW_KERNELS = ("hg_max_kernel", "hg_prep_kernel", "hg_w1_kernel", "hg_dz_kernel", "hg_reduce_kernel")


def mfma_peak_tflops():
    """bench.py's MFMA_PEAK_TFLOPS, read from its source (importing bench.py would run its argument parsing)"""
    for line in open(os.path.join(ROOT, "bench.py")):
        if line.startswith("MFMA_PEAK_TFLOPS"):
            return float(line.split("=")[1].split("#")[0])
    raise RuntimeError("MFMA_PEAK_TFLOPS not found in bench.py")


def make_case(n, K):
    m = models.load_synthetic(models.ssdlite320_mobilenet_v3_large(num_classes=K), 0).cuda()
    imgs = torch.from_numpy(synth.images(17, n, 320, 320)).cuda()
    rng = np.random.RandomState(n + K)
    targets = []
    for i in range(n):
        g = 1 + (i * 7) % 12
        xy = rng.uniform(0, 220, (g, 2)).astype(np.float32)
        b = np.concatenate([xy, xy + rng.uniform(20, 90, (g, 2)).astype(np.float32)], 1)
        targets.append({"boxes": torch.from_numpy(b).cuda(), "labels": torch.from_numpy(rng.randint(1, K, (g,)).astype(np.int64)).cuda()})
    return m, imgs, targets


def torch_heads(feats, P, B, ents, n, A, K):
    """the reference's SSDLiteHead in torch ops (ssd_mobilenetv3.py:27-36,65-95), head BN in eval mode"""
    logits, reg = [None] * 6, [None] * 6
    for e in ents:
        y = F.conv2d(feats[e.level], P[e.dw_w], None, 1, 1, 1, e.c)
        y = F.batch_norm(y, B[e.bn + ".running_mean"], B[e.bn + ".running_var"], P[e.bn + ".weight"], P[e.bn + ".bias"], False, 0.0, e.eps)
        y = F.conv2d(F.relu6(y), P[e.pw_w], P[e.pw_b])
        y = y.view(n, -1, e.cols, e.h, e.w).permute(0, 3, 4, 1, 2).reshape(n, -1, e.cols)
        (logits if e.kind == 1 else reg)[e.level] = y
    return {"cls_logits": torch.cat(logits, 1), "bbox_regression": torch.cat(reg, 1)}


def features_nchw(m, imgs):
    import ctypes as C
    from demonet_amd import _lib
    g = m.graph
    dev = imgs.device
    handle = m._plan(dev, heads_may_differ=True)
    n, _, h, w = imgs.shape
    b = m._buffers_for(n, h, w, dev)
    b["images"].copy_(imgs)
    L = _lib.lib()
    ws = b["ws"]
    _lib.check(L.dn_forward_features(C.c_void_p(handle), C.c_void_p(b["images"].data_ptr()), n, h, w, C.c_void_p(ws.data_ptr()), ws.numel(),
                                     C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "dn_forward_features")
    m._feat_gen += 1
    feats = []
    for lvl, f in enumerate(g.features):
        t = g.t(f)
        parts = []
        for k in range(m.batch_split(n)):
            p, first, im = C.c_void_p(), C.c_int(), C.c_int()
            _lib.check(L.dn_level_features(C.c_void_p(handle), C.c_void_p(ws.data_ptr()), n, lvl, k, C.byref(p), C.byref(first), C.byref(im)))
            off = p.value - ws.data_ptr()
            parts.append(ws[off:off + im.value * t.h * t.w * t.c * 2].view(torch.float16).view(im.value, t.h, t.w, t.c))
        feats.append(torch.cat(parts).permute(0, 3, 1, 2).float().contiguous())
    return feats


def mfma_flops(ents, pieces):
    """FLOPs of the matrix instructions hg_w1_kernel / hg_dz_kernel issue in one backward (csrc/headgrad.hip: 64 x 64 tiles, 32-deep stages,
    hg_split chunks), and the useful FLOPs 2 P c cout of each contraction"""
    cd = lambda a, b: -(-a // b)
    w1 = dz = useful = 0
    for e in ents:
        for _, _, im in pieces[e.level]:
            P = im * e.h * e.w
            tiles = cd(e.c, 64) * cd(e.cout, 64)
            sp = min(max(1, min(16, 1024 // tiles)), cd(P, 128))
            chunk = cd(cd(P, sp), 32) * 32
            stages = sum(cd(min(P, (z + 1) * chunk) - z * chunk, 32) for z in range(sp) if z * chunk < P)
            w1 += tiles * stages * 8 * 32768
            dz += cd(e.c, 64) * cd(P, 64) * cd(e.cout, 32) * 8 * 32768
            useful += 2 * P * e.c * e.cout
    return w1, dz, useful


def _events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def steps_for(n, K):
    m, imgs, targets = make_case(n, K)
    m.train_heads()
    g = m.graph
    ents = headgrad.entries(g)
    A = g.num_anchors()
    hp = m.head_parameters()

    def hip_step():
        losses = m.loss(imgs, targets)
        for p in hp.values():
            p.grad = None
        (losses["bbox_regression"] + losses["classification"]).backward()
        return losses

    tp = {k: p.detach().clone().requires_grad_(True) for k, p in hp.items()}
    B = dict(m.named_buffers())

    def torch_step():
        feats = features_nchw(m, imgs)
        losses = m.compute_loss(targets, torch_heads(feats, tp, B, ents, n, A, K))
        for p in tp.values():
            p.grad = None
        (losses["bbox_regression"] + losses["classification"]).backward()
        return losses

    return m, imgs, targets, ents, hp, tp, hip_step, torch_step


def run(n, K, reps, rounds, kstats, steps_profiled):
    m, imgs, targets, ents, hp, tp, hip_step, torch_step = steps_for(n, K)
    # correctness first: the library's gradients within the derived bound, the torch-ops gradients near the same reference
    ho = headgrad.head_outputs(m, imgs)
    for t in ho.values():
        t.retain_grad()
    step = ho["cls_logits"].grad_fn.step
    losses = m.compute_loss(targets, ho)
    for p in hp.values():
        p.grad = None
    (losses["bbox_regression"] + losses["classification"]).backward()
    feats = [torch.cat([x for x, _, _ in lv]).permute(0, 3, 1, 2).cpu() for lv in step.pieces]
    levels = (1, 5) if K > 256 else None
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ref, amb = hr.model_reference(hr.V3, sd, feats, list(m.graph.anchors_per_loc), K, ho["cls_logits"].grad.cpu(), ho["bbox_regression"].grad.cpu(), levels)
    worst = max(hr.worst_ratio(hp[k].grad.cpu(), g, b) for k, (g, b) in ref.items())
    assert worst <= 1.0 and amb <= hr.AMBIGUOUS_CAP, (worst, amb)
    # the torch-ops head, given the SAME upstream gradient (its own loss gradient differs a little: it runs unrounded fp32 weights, so its
    # logits and the negatives mined from them are not the library's)
    out = torch_heads(features_nchw(m, imgs), tp, dict(m.named_buffers()), ents, n, m.graph.num_anchors(), K)
    ((out["cls_logits"] * ho["cls_logits"].grad).sum() + (out["bbox_regression"] * ho["bbox_regression"].grad).sum()).backward()
    worst_torch = max(float((tp[k].grad.cpu().double() - g).abs().max() / g.abs().max().clamp_min(1e-30)) for k, (g, _) in ref.items())
    assert worst_torch <= 1e-3, worst_torch
    a, b = hip_step(), torch_step()
    for k in a:
        assert abs(a[k].item() - b[k].item()) <= 5e-3 * abs(b[k].item()), (k, a[k].item(), b[k].item())
    pieces = step.pieces
    for _ in range(3):
        hip_step()
        torch_step()
    torch.cuda.synchronize()
    hip_ms, torch_ms = [], []
    for _ in range(rounds):
        hip_ms.append(_events_ms(hip_step, reps))
        torch_ms.append(_events_ms(torch_step, reps))
    w1f, dzf, useful = mfma_flops(ents, pieces)
    rec = dict(n=n, num_classes=K, chains=m.batch_split(n), reps=reps, rounds=rounds, worst_ratio_to_bound=round(worst, 3), bound_levels=levels or "all",
               torch_grad_worst_rel=float("%.3g" % worst_torch), hip_step_ms=round(statistics.median(hip_ms), 4), torch_step_ms=round(statistics.median(torch_ms), 4),
               hip_rounds_ms=[round(x, 4) for x in hip_ms], torch_rounds_ms=[round(x, 4) for x in torch_ms],
               torch_over_hip=round(statistics.median(torch_ms) / statistics.median(hip_ms), 2),
               mfma_flops_issued=dict(hg_w1_kernel=w1f, hg_dz_kernel=dzf), useful_flops_per_contraction=useful)
    if kstats:
        peak = mfma_peak_tflops()
        rec["kernels"] = {}
        for name in NEW_KERNELS:
            ns = sum(v for k, v in kstats.items() if name in k)
            ms = ns / 1e6 / steps_profiled
            row = dict(ms_per_step=round(ms, 4))
            if name in rec["mfma_flops_issued"] and ms > 0:
                tf = rec["mfma_flops_issued"][name] / (ms * 1e-3) / 1e12
                row.update(issued_tflops=round(tf, 1), share_of_fp16_mfma_peak=round(tf / peak, 4))
            rec["kernels"][name] = row
    return rec


def read_kernel_stats(path):
    """rocprofv3 --stats kernel_stats.csv: kernel name -> total duration in ns"""
    out = {}
    for r in csv.DictReader(open(path)):
        out[r["Name"]] = out.get(r["Name"], 0) + int(float(r["TotalDurationNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--profile-step", type=int, nargs=2, default=None, metavar=("N", "K"))
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats.csv of a rocprofv3 run of --profile-step for the FIRST shape")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if a.profile_step:
        hip_step = steps_for(*a.profile_step)[6]
        for _ in range(a.steps):
            hip_step()
        torch.cuda.synchronize()
        return
    rows = []
    for i, (n, K) in enumerate(SHAPES):
        r = run(n, K, a.reps, a.rounds, read_kernel_stats(a.kernel_stats) if a.kernel_stats and i == 0 else None, a.steps)
        print({k: r[k] for k in ("n", "num_classes", "hip_step_ms", "torch_step_ms", "worst_ratio_to_bound")}, file=sys.stderr, flush=True)
        rows.append(r)
        torch.cuda.empty_cache()
    line = json.dumps({"tool": "tools/time_head_grad.py", "device": torch.cuda.get_device_name(0), "mfma_peak_tflops": mfma_peak_tflops(), "shapes": rows})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
