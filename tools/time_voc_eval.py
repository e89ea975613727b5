"""dev tool: what VOC scoring costs with the marking on the device, against the host path.
    python tools/time_voc_eval.py [--out profiles/voc_eval_timing.json] [--batches 32] [--rounds 3] [--host-rounds 2] [--launches 200]
1. match_us: device time of the dn_match_detections launch alone -- HIP events around `launches` back-to-back calls on preallocated outputs after
   a warm-up, mean per launch, median over `rounds`: n = 64, d = 300, 8 ground truths per image with 1 and with 10 thresholds, and n = 64 at the
   limits d = 512, gmax = 1024 (all rows live, 3 labels, 10 thresholds).
2. images_per_sec: ssdlite320_mobilenet_v3_large with 21 classes, batch 64, `batches` batches resident on the device (four distinct ones, cycled),
   8 ground truths per image made from a first forward's top detections, one threshold (0.5):
     host    engine.evaluate + evalrec.voc_mean_ap      (detections to the host, Python loop over every detection)
     device  engine.evaluate_voc                        (marking on the device, one sort + cumulative sum at the end)
   host clock around each whole call, the two alternated; plus where evaluate_voc's time goes: the forwards alone (engine.evaluate's loop with
   nothing collected: ForwardPipeline submit / drain), pad_targets per batch, summarize, and summarize with evalrec.voc_ap's Python loop in place of voceval._voc_ap (the same numbers).
   The loader repeats four batches, so scores tie across images: the host path orders ties by an unstable sort, the device path by batch, image,
   slot, and the two mAPs may differ in the last digits (map_abs_diff); tests/test_evalmatch.py holds them equal where no scores tie.
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
from demonet_amd import _lib, engine, evalrec, models, synth, voceval  # noqa: E402
from demonet_amd.pipeline import ForwardPipeline  # noqa: E402

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
                gt_labels=t(gl), gt_difficult=t((rng.random((n, gmax)) < 0.1).astype(np.uint8)), gt_counts=torch.full((n,), g, dtype=torch.int32, device="cuda"))


def _match_us(case, thresholds, launches, rounds):
    n, d = case["scores"].shape
    gmax = case["gt_labels"].shape[1]
    flags = torch.empty((n, d), dtype=torch.int32, device="cuda")
    stats = torch.zeros((K, 2), dtype=torch.int64, device="cuda")
    thr = (C.c_double * len(thresholds))(*thresholds)
    p = lambda x: C.c_void_p(x.data_ptr())
    L, st = _lib.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = [p(case[k]) for k in ("boxes", "scores", "labels", "counts", "gt_boxes", "gt_labels", "gt_difficult", "gt_counts")] + \
        [n, d, gmax, K, thr, len(thresholds), 1.0, p(flags), None, None, p(stats), st]
    out = []
    for r in range(rounds + 1):                                  # (round 0 is the warm-up)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(launches):
            _lib.check(L.dn_match_detections(*args), "dn_match_detections")
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
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-rounds", type=int, default=2)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    ten = voceval.COCO_THRESHOLDS
    match_us = {"n64_d300_g8_t1": _match_us(_match_case(64, 300, GT, GT), (0.5,), a.launches, a.rounds),
                "n64_d300_g8_t10": _match_us(_match_case(64, 300, GT, GT), ten, a.launches, a.rounds),
                "n64_d512_g1024_t10": _match_us(_match_case(64, 512, 1024, 1024), ten, a.launches, a.rounds)}

    m = models.load_synthetic(getattr(models, MODEL)(num_classes=K), 0).cuda()
    distinct = [torch.from_numpy(synth.images(3000 + i, BATCH, 320, 320)).cuda() for i in range(4)]
    rng = np.random.default_rng(0)
    targets = []
    for b in distinct:                                           # 8 ground truths per image: the top detections, jittered; one in five difficult
        boxes, scores, labels, counts = (t.cpu() for t in m.forward_batch(b))
        tb = []
        for i in range(BATCH):
            k = min(GT, int(counts[i]))
            top = torch.argsort(scores[i, :int(counts[i])], descending=True, stable=True)[:k]
            tb.append({"boxes": boxes[i, top] + torch.from_numpy(rng.integers(-3, 4, (k, 4)).astype(np.float32)), "labels": labels[i, top].clone(),
                       "difficult": torch.from_numpy((rng.random(k) < 0.2).astype(np.uint8))})
        targets.append(tb)
    loader = [(distinct[i % 4], [dict(t, image_id=i * BATCH + j) for j, t in enumerate(targets[i % 4])]) for i in range(a.batches)]
    n_images = a.batches * BATCH

    def host_path():
        res, _ = engine.evaluate(m, loader)
        dets = [{k: v.numpy() for k, v in res[t["image_id"]].items()} for _, tg in loader for t in tg]
        gts = [{k: t[k].numpy() for k in ("boxes", "labels", "difficult")} for _, tg in loader for t in tg]
        return evalrec.voc_mean_ap(dets, gts, 0.5)[0]

    def device_path():
        return engine.evaluate_voc(m, loader, thresholds=(0.5,))

    def forwards_only():
        with ForwardPipeline(m, BATCH, depth=3) as pipe:
            for images, _ in loader:
                pipe.submit(images)

    device_path()                                                # warm-up of both loops' shapes
    engine.evaluate(m, loader[:4])
    t_host, t_dev, t_fwd, maps = [], [], [], []
    for r in range(a.rounds):
        dt, (summary, stats) = _host_s(device_path)
        t_dev.append(dt)
        t_fwd.append(_host_s(forwards_only)[0])
        if r < a.host_rounds:
            dt, host_map = _host_s(host_path)
            t_host.append(dt)
            maps.append((summary["map"][0], host_map))
    t_pad = _host_s(lambda: [voceval.pad_targets(tg, "cuda") for _, tg in loader])[0] / a.batches
    acc = voceval.VocAccumulator(K)
    for images, tg in loader:
        acc.update(*m.forward_batch(images), tg)
    t_sum = _host_s(acc.summarize)[0]
    fast_ap = voceval._voc_ap
    voceval._voc_ap = evalrec.voc_ap                             # what summarize costs with evalrec.voc_ap's Python loop over the envelope
    try:
        t_sum_loop, looped = _host_s(acc.summarize)
    finally:
        voceval._voc_ap = fast_ap
    same_ap = looped == acc.summarize()
    med = statistics.median
    doc = dict(device=torch.cuda.get_device_name(0), match_us=match_us, launches=a.launches, rounds=a.rounds, model=MODEL, num_classes=K, batch=BATCH,
               batches=a.batches, images=n_images, gt_per_image=GT, thresholds=[0.5],
               seconds=dict(host=round(med(t_host), 3), device=round(med(t_dev), 4), forwards_only=round(med(t_fwd), 4)),
               images_per_sec=dict(host=round(n_images / med(t_host), 1), device=round(n_images / med(t_dev), 1), forwards_only=round(n_images / med(t_fwd), 1)),
               device_over_host=round(med(t_host) / med(t_dev), 1),
               device_path_parts_ms=dict(pad_targets_per_batch=round(t_pad * 1e3, 3), summarize=round(t_sum * 1e3, 2),
                                         summarize_with_evalrec_voc_ap=round(t_sum_loop * 1e3, 2)), summarize_equals_evalrec_voc_ap=same_ap,
               map_device_host=maps, map_abs_diff=max(abs(x - y) for x, y in maps))
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
