"""dev tool: what the soft-NMS modes cost against hard NMS on the flagship workload.
    python tools/time_soft_nms.py [--out profiles/soft_nms_timing.json] [--warmup 20] [--steps 200]
ssdlite320_mobilenet_v3_large, K = 91, batch 64, one forward at a time (forward_batch on one stream, hipGraph replay, device events around
the timed steps), in hard, linear and Gaussian (sigma 0.5) mode of SSD.set_nms; then, per mode, the post-process segments of dn_profile_end
over 20 eager forwards: softmax / decode | cut-off + select / NMS (the soft reduce reports here) | merge | fallback select + merge. A forward of
64 images runs as two sub-batch chains; the profile times them back to back and adds their segments up.
One JSON document on stdout (and in --out)."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from demonet_amd import _lib, models, synth  # noqa: E402

MODEL, K, BATCH = "ssdlite320_mobilenet_v3_large", 91, 64
MODES = [("hard", 0.5), ("linear", 0.5), ("gaussian", 0.5)]


def _events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def run(method, sigma, warmup, steps):
    m = getattr(models, MODEL)(num_classes=K)
    models.load_synthetic(m, 0)
    m.cuda().set_nms(method, sigma=sigma)
    W, H = m.graph.size
    imgs = torch.from_numpy(synth.images(64, BATCH, H, W)).cuda()
    try:
        step = lambda: m.forward_batch(imgs, persistent_input=True)
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        ms = _events_ms(step, steps)
        counts = m.forward_batch(imgs, persistent_input=True)[3]
        dets = int(counts.sum())
        L = _lib.lib()
        h = C.c_void_p(m._handle)
        nseg = len(m.graph.nodes) + 4
        _lib.check(L.dn_profile_begin(h))
        for _ in range(20):
            step()
        buf = (C.c_float * nseg)()
        runs = _lib.check(L.dn_profile_end(h, buf, nseg))
        seg = [round(float(buf[len(m.graph.nodes) + q]), 4) for q in range(4)]
        chains = _lib.check(L.dn_batch_split(h, BATCH))
    finally:
        m.release()
    return dict(mode=method, sigma=sigma if method == "gaussian" else None, forward_ms=round(ms, 4), img_per_s=round(BATCH / ms * 1e3, 1),
                detections=dets, profiled_forwards=runs, chains=chains, softmax_decode_ms=seg[0], select_nms_ms=seg[1], merge_ms=seg[2],
                fallback_ms=seg[3])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    doc = dict(model=MODEL, num_classes=K, batch=BATCH, warmup=a.warmup, steps=a.steps, device=torch.cuda.get_device_name(0), modes=[])
    for method, sigma in MODES:
        doc["modes"].append(run(method, sigma, a.warmup, a.steps))
        torch.cuda.empty_cache()
    hard = doc["modes"][0]
    for r in doc["modes"][1:]:
        r["forward_vs_hard"] = round(r["forward_ms"] / hard["forward_ms"], 3)
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
