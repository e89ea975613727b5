"""dev tool: what COCO scoring costs with the matching on the device, against the host path.
    python tools/time_coco_eval.py [--out profiles/coco_eval_timing.json] [--batches 4] [--rounds 3] [--host-rounds 1] [--launches 200]
1. match_us: device time of the dn_coco_match launch alone -- HIP events around `launches` back-to-back calls on preallocated outputs after a
   warm-up, mean per launch, median over `rounds`: n = 64, d = 300, 8 ground truths per image, 3 labels, 4 area ranges with 1 and with 10
   thresholds, and n = 64 at the limits d = 512, gmax = 1024 (all rows live, 3 labels, 10 thresholds, 4 ranges, a tenth of `launches`).
2. seconds: ssdlite320_mobilenet_v3_large with 21 classes, batch 64, `batches` batches resident on the device (four distinct ones, cycled), 8
   ground truths per image made from a first forward's top detections (one in five crowd, area = the box's or half of it):
     host    engine.evaluate + engine.coco_records + tests/cocoeval_ref.coco_eval (the numpy restatement of pycocotools: Python loops)
     device  engine.evaluate_coco                     (matching on the device, two sorts + cumulative sums at the end)
   host clock around each whole call; the device path's loop and its summary are timed separately (`summarize_seconds`), and pad_targets per batch.
   The set is small because the host reference is slow; no ratio is promised. The loader repeats four batches, so scores tie across images; both
   paths keep (batch, image, slot) order among ties, and `stats_equal` records whether the twelve numbers came out the same.
One JSON document on stdout (and in --out)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cocoeval_ref  # noqa: E402
from demonet_amd import _lib, cocoeval, engine, models, synth  # noqa: E402

MODEL, K, BATCH, GT = "ssdlite320_mobilenet_v3_large", 21, 64, 8


def _match_case(n, d, g, gmax, seed=0):
    rng = np.random.default_rng(seed)
    ctr, wh = rng.uniform(50, 900, (n, gmax, 2)), rng.uniform(20, 120, (n, gmax, 2))
    gb = np.concatenate([ctr - wh / 2, ctr + wh / 2], -1).astype(np.float32)
    gl = rng.integers(1, 4, (n, gmax)).astype(np.int64)
    src = rng.integers(0, g, (n, d))
    boxes = (np.take_along_axis(gb, src[..., None], 1) + rng.normal(0, 5.0, (n, d, 4))).astype(np.float32)
    labels = np.take_along_axis(gl, src, 1)
    scores = rng.uniform(0.01, 1.0, (n, d)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).cuda()
    return dict(boxes=t(boxes), scores=t(scores), labels=t(labels), counts=torch.full((n,), d, dtype=torch.int32, device="cuda"), gt_boxes=t(gb),
                gt_labels=t(gl), gt_counts=torch.full((n,), g, dtype=torch.int32, device="cuda"), gt_crowd=t((rng.random((n, gmax)) < 0.1).astype(np.uint8)),
                gt_area=t(((gb[..., 2] - gb[..., 0]) * (gb[..., 3] - gb[..., 1])).astype(np.float32)))


def _match_us(case, thresholds, launches, rounds):
    n, d = case["scores"].shape
    gmax = case["gt_labels"].shape[1]
    R = len(cocoeval.AREA_RANGES)
    flags = torch.empty((n, d, R), dtype=torch.int32, device="cuda")
    rank = torch.empty((n, d), dtype=torch.int32, device="cuda")
    stats = torch.zeros((K, R), dtype=torch.int64, device="cuda")
    thr = (C.c_double * len(thresholds))(*thresholds)
    rng = (C.c_double * (2 * R))(*[v for r in cocoeval.AREA_RANGES for v in r])
    p = lambda x: C.c_void_p(x.data_ptr())
    L, st = _lib.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = [p(case[k]) for k in ("boxes", "scores", "labels", "counts", "gt_boxes", "gt_labels", "gt_counts", "gt_crowd", "gt_area")] + \
        [n, d, gmax, K, thr, len(thresholds), rng, R, 100, p(flags), p(rank), None, p(stats), st]
    out = []
    for r in range(rounds + 1):                                  # (round 0 is the warm-up)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(launches):
            _lib.check(L.dn_coco_match(*args), "dn_coco_match")
        e1.record()
        e1.synchronize()
        if r:
            out.append(e0.elapsed_time(e1) * 1e3 / launches)
    return round(statistics.median(out), 2)


def _host_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-rounds", type=int, default=1)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    ten = tuple(cocoeval.IOU_THRESHOLDS)
    match_us = {"n64_d300_g8_t1_r4": _match_us(_match_case(64, 300, GT, GT), (0.5,), a.launches, a.rounds),
                "n64_d300_g8_t10_r4": _match_us(_match_case(64, 300, GT, GT), ten, a.launches, a.rounds),
                "n64_d512_g1024_t10_r4": _match_us(_match_case(64, 512, 1024, 1024), ten, max(1, a.launches // 10), a.rounds)}

    m = models.load_synthetic(getattr(models, MODEL)(num_classes=K), 0).cuda()
    distinct = [torch.from_numpy(synth.images(3000 + i, BATCH, 320, 320)).cuda() for i in range(4)]
    rng = np.random.default_rng(0)
    targets = []
    for b in distinct:                                           # 8 ground truths per image: the top detections, jittered
        boxes, scores, labels, counts = (t.cpu() for t in m.forward_batch(b))
        tb = []
        for i in range(BATCH):
            k = min(GT, int(counts[i]))
            top = torch.argsort(scores[i, :int(counts[i])], descending=True, stable=True)[:k]
            gb = boxes[i, top] + torch.from_numpy(rng.integers(-3, 4, (k, 4)).astype(np.float32))
            area = (gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1]) * torch.from_numpy(rng.choice([1.0, 0.5], k).astype(np.float32))
            tb.append({"boxes": gb, "labels": labels[i, top].clone(), "area": area, "iscrowd": torch.from_numpy((rng.random(k) < 0.2).astype(np.uint8))})
        targets.append(tb)
    loader = [(distinct[i % 4], [dict(t, image_id=i * BATCH + j) for j, t in enumerate(targets[i % 4])]) for i in range(a.batches)]
    n_images = a.batches * BATCH

    def host_path():
        t0 = time.perf_counter()
        res, _ = engine.evaluate(m, loader)
        records = engine.coco_records(res)
        t1 = time.perf_counter()
        dets = [{k: v.numpy() for k, v in res[t["image_id"]].items()} for _, tg in loader for t in tg]
        gts = [{k: t[k].numpy() for k in ("boxes", "labels", "iscrowd", "area")} for _, tg in loader for t in tg]
        out = cocoeval_ref.coco_eval(dets, gts, K)
        return out["stats"], t1 - t0, time.perf_counter() - t1, len(records)

    def device_path():
        return engine.evaluate_coco(m, loader)

    device_path()                                                # warm-up of both loops' shapes
    engine.evaluate(m, loader[:4])
    t_dev, t_sum, t_host, t_host_loop, t_host_ref, same, n_records = [], [], [], [], [], [], 0
    for r in range(a.rounds):
        dt, (summary, stats) = _host_s(device_path)
        t_dev.append(dt)
        t_sum.append(stats["summarize_seconds"])
        if r < a.host_rounds:
            dt, (host_stats, loop_s, ref_s, n_records) = _host_s(host_path)
            t_host.append(dt)
            t_host_loop.append(loop_s)
            t_host_ref.append(ref_s)
            same.append(summary["stats"] == host_stats)
    t_pad = _host_s(lambda: [cocoeval.pad_targets(tg, "cuda") for _, tg in loader])[0] / a.batches
    med = statistics.median
    doc = dict(device=torch.cuda.get_device_name(0), match_us=match_us, launches=a.launches, rounds=a.rounds, model=MODEL, num_classes=K, batch=BATCH,
               batches=a.batches, images=n_images, detections=n_records, gt_per_image=GT, thresholds=10, area_ranges=4, max_dets=[1, 10, 100],
               seconds=dict(host=round(med(t_host), 3), host_evaluate_and_records=round(med(t_host_loop), 4), host_reference=round(med(t_host_ref), 3),
                            device=round(med(t_dev), 4), device_loop=round(med(t_dev) - med(t_sum), 4), device_summarize=round(med(t_sum), 4)),
               images_per_sec=dict(host=round(n_images / med(t_host), 1), device=round(n_images / med(t_dev), 1)),
               device_path_parts_ms=dict(pad_targets_per_batch=round(t_pad * 1e3, 3)), stats=summary["stats"], stats_equal=all(same))
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
