"""dev tool: what sliced inference costs on one full-HD frame, and what the hand-written crop and merge replace.
    python tools/time_sliced.py [--out profiles/sliced_timing.json] [--rounds 5] [--reps 20] [--host-reps 1]
ssdlite320_mobilenet_v3_large, K = 91, default thresholds, one 1080 x 1920 frame, tile 320, overlap 0.25 (40 tiles), full_image=True: 41 sources.
Device events around `reps` calls of each variant, the variants alternated over `rounds` rounds, medians reported (ms per call):
  whole         SSD.detect_sliced: crop, tile forward, whole-image forward, staging copies, merge, the counts' device-to-host copy
  forwards      the 40-tile forward and the whole-image forward alone (forward_batch on resident inputs): the floor
  crop          dn_crop_tiles alone (it reads the 40 origins back first: host-synchronous)
  merge         dn_merge_detections alone on the 41 staged sources (workspace and outputs allocated per call, no host copy)
  torch_crop    the same tiles by torch slicing + stack
  host_merge    device-to-host copy of the staged sources + tests/sliced_ref.merge_ref (numpy) on the host: host clock, `host-reps` calls a round
  today         what a user composes without this feature: torch_crop -> forwards -> host_merge
One JSON document on stdout (and in --out)."""
import argparse
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
import sliced_ref as sr  # noqa: E402
from demonet_amd import models, sliced, synth  # noqa: E402

MODEL, K, H, W, TILE, OVERLAP = "ssdlite320_mobilenet_v3_large", 91, 1080, 1920, 320, 0.25


def _events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def _host_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    m = models.load_synthetic(getattr(models, MODEL)(num_classes=K), 0).cuda()
    D = m.detections_per_img
    frame = torch.from_numpy(synth.images(1080, 1, H, W)[0]).cuda()
    origins, th, tw = sliced.tile_grid(H, W, TILE, TILE, OVERLAP)
    T = len(origins)
    origins_dev = torch.tensor(origins, dtype=torch.int32, device="cuda")
    offsets = np.asarray([(float(x), float(y)) for x, y in origins] + [(0.0, 0.0)], np.float32)
    offsets_dev = torch.from_numpy(offsets).cuda()
    tiles = torch.empty((T, 3, th, tw), device="cuda")
    whole1 = frame[None].contiguous()

    def torch_crop():
        return torch.stack([frame[:, y:y + th, x:x + tw] for x, y in origins], out=tiles)

    def forwards():
        to = m.forward_batch(tiles, persistent_input=True)
        fo = m.forward_batch(whole1, persistent_input=True)
        return to, fo

    def stage():
        to, fo = forwards()
        return [torch.cat([x, y], 0) for x, y in zip(to, fo)]

    def host_merge(st):
        b, s, l, c = (t.cpu().numpy() for t in st)
        return sr.merge_ref(b, s, l, c, offsets, [0, T + 1], sr.IOU, m.nms_thresh, 0, D)

    def today():
        torch_crop()
        return host_merge(stage())

    sliced.crop_tiles(frame, origins_dev, th, tw, out=tiles)
    staged = stage()
    torch.cuda.synchronize()
    variants = dict(
        whole=(lambda: m.detect_sliced(frame, tile=TILE, overlap=OVERLAP), _events_ms, a.reps),
        forwards=(forwards, _events_ms, a.reps),
        crop=(lambda: sliced.crop_tiles(frame, origins_dev, th, tw, out=tiles), _events_ms, a.reps),
        merge=(lambda: sliced.merge_detections(*staged, offsets_dev, [0, T + 1], m.nms_thresh, "iou", False, D), _events_ms, a.reps),
        torch_crop=(torch_crop, _events_ms, a.reps),
        host_merge=(lambda: host_merge(staged), _host_ms, a.host_reps),
        today=(today, _host_ms, a.host_reps),
    )
    # the two paths must agree before their times are compared
    got = m.detect_sliced(frame, tile=TILE, overlap=OVERLAP)[0]
    ob, os_, ol, oc, _, margin = today()
    n = int(oc[0])
    same = bool(n == got["scores"].numel() and np.array_equal(got["boxes"].cpu().numpy(), ob[0, :n]) and np.array_equal(got["scores"].cpu().numpy(), os_[0, :n])
                and np.array_equal(got["labels"].cpu().numpy(), ol[0, :n]))
    for name, (fn, timer, reps) in variants.items():      # warm-up of every shape
        if timer is _events_ms:
            for _ in range(3):
                fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for name, (fn, timer, reps) in variants.items():
            times[name].append(timer(fn, reps))
    doc = dict(model=MODEL, num_classes=K, frame=[H, W], tile=TILE, overlap=OVERLAP, tiles=T, sources=T + 1, rows_per_source=D,
               candidates=int(staged[3].sum()), merged=n, merge_margin=margin, whole_equals_composition=same, rounds=a.rounds, reps=a.reps,
               host_reps=a.host_reps, device=torch.cuda.get_device_name(0),
               median_ms={k: round(statistics.median(v), 4) for k, v in times.items()},
               min_ms={k: round(min(v), 4) for k, v in times.items()}, max_ms={k: round(max(v), 4) for k, v in times.items()})
    med = doc["median_ms"]
    doc["crop_plus_merge_share_of_whole"] = round((med["crop"] + med["merge"]) / med["whole"], 4)
    doc["whole_over_forwards"] = round(med["whole"] / med["forwards"], 3)
    doc["today_over_whole"] = round(med["today"] / med["whole"], 2)
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
