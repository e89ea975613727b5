"""dev tool: what flip test-time augmentation with weighted boxes fusion costs at batch 64, and what the device fusion replaces.
    python tools/time_tta.py [--out profiles/tta_timing.json] [--rounds 5] [--reps 20] [--host-reps 1] [--batch 64]
ssdlite320_mobilenet_v3_large, K = 91, default thresholds, synthetic weights, 64 synthetic 320 x 320 images: 128 sources of 300 rows, 64 groups.
Device events around `reps` calls of each variant, the variants alternated over `rounds` rounds, medians reported (ms per call):
  whole         SSD.detect_tta(fuse="wbf"): flip, one forward of 128, un-flip, staging copies, fusion, the counts' device-to-host copy
  forward_2n    the forward of the 128 images alone (forward_batch on a resident input): the floor of `whole`
  forwards      the plain and the flipped forward as two forward_batch calls of 64 on resident inputs: the floor of `today`
  fuse          dn_fuse_detections alone on the 128 staged sources (workspace and outputs allocated per call, no host copy): its six launches
  host_fuse     device-to-host copy of the staged sources + tests/wbf_ref.fuse (numpy float32) + upload of the result: host clock, `host-reps` calls
  today         what a user composes without this feature: forwards -> un-flip -> host_fuse
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
import wbf_ref as wr  # noqa: E402
from demonet_amd import fusion, models, synth  # noqa: E402

MODEL, K, H, W = "ssdlite320_mobilenet_v3_large", 91, 320, 320


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
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    m = models.load_synthetic(getattr(models, MODEL)(num_classes=K), 0).cuda().eval()
    D, N = m.detections_per_img, a.batch
    plain = torch.from_numpy(synth.images(64, N, H, W)).cuda()
    flipped = torch.flip(plain, [-1]).contiguous()
    both = torch.cat([plain, flipped], 0)
    gb = list(range(0, 2 * N + 1, 2))
    offsets = np.zeros((2 * N, 2), np.float32)
    offsets_dev = torch.from_numpy(offsets).cuda()

    def forwards():
        po = [t.clone() for t in m.forward_batch(plain, persistent_input=True)]
        fo = m.forward_batch(flipped, persistent_input=True)
        return po, fo

    def stage():
        """-> the 2 N sources, sources 2 g and 2 g + 1 = image g, the mirrored pass mapped back (on the device)."""
        po, fo = forwards()
        fb = fo[0]
        ub = torch.stack([float(W) - fb[..., 2], fb[..., 1], float(W) - fb[..., 0], fb[..., 3]], -1)
        return [torch.stack([x, y], 1).flatten(0, 1).contiguous() for x, y in zip(po, (ub, fo[1], fo[2], fo[3]))]

    def host_fuse(st):
        b, s, l, c = (t.cpu().numpy() for t in st)
        out = wr.fuse(b, s, l, c, offsets, gb, None, m.nms_thresh, m.score_thresh, D)
        return out, [torch.from_numpy(x).cuda() for x in out[:4]]

    def today():
        return host_fuse(stage())

    staged = stage()
    torch.cuda.synchronize()
    variants = dict(
        whole=(lambda: m.detect_tta(plain), _events_ms, a.reps),
        forward_2n=(lambda: m.forward_batch(both, persistent_input=True), _events_ms, a.reps),
        forwards=(forwards, _events_ms, a.reps),
        fuse=(lambda: fusion.fuse_detections(*staged, offsets_dev, gb, None, m.nms_thresh, m.score_thresh, D), _events_ms, a.reps),
        host_fuse=(lambda: host_fuse(staged), _host_ms, a.host_reps),
        today=(today, _host_ms, a.host_reps),
    )
    # the two paths must agree before their times are compared
    got = m.detect_tta(plain)
    (ob, os_, ol, oc, om, _), _ = today()
    same = all(int(oc[g]) == got[g]["scores"].numel() and np.array_equal(got[g]["boxes"].cpu().numpy(), ob[g, :oc[g]])
               and np.array_equal(got[g]["scores"].cpu().numpy(), os_[g, :oc[g]]) and np.array_equal(got[g]["labels"].cpu().numpy(), ol[g, :oc[g]])
               for g in range(N))
    for name, (fn, timer, reps) in variants.items():      # warm-up of every shape
        if timer is _events_ms:
            for _ in range(3):
                fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for name, (fn, timer, reps) in variants.items():
            times[name].append(timer(fn, reps))
    doc = dict(model=MODEL, num_classes=K, image=[H, W], batch=N, sources=2 * N, rows_per_source=D, candidates=int(staged[3].sum()),
               fused=int(oc.sum()), fused_rows_with_two_members=int((om == 2).sum()), whole_equals_composition=bool(same), rounds=a.rounds, reps=a.reps,
               host_reps=a.host_reps, device=torch.cuda.get_device_name(0),
               median_ms={k: round(statistics.median(v), 4) for k, v in times.items()},
               min_ms={k: round(min(v), 4) for k, v in times.items()}, max_ms={k: round(max(v), 4) for k, v in times.items()})
    med = doc["median_ms"]
    doc["fuse_share_of_whole"] = round(med["fuse"] / med["whole"], 4)
    doc["whole_over_forward_2n"] = round(med["whole"] / med["forward_2n"], 3)
    doc["today_over_whole"] = round(med["today"] / med["whole"], 2)
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
