"""dev tool: what tracking 64 streams on the device costs behind a forward, and what it replaces.
    python tools/time_track.py [--out profiles/track_timing.json] [--rounds 5] [--host-frames 3] [--streams 64]
64 streams, about 100 detections per stream and frame (tests/track_ref.scene: 112 moving objects with dropouts, score dips and false positives in
160 rows), ByteTrack's default thresholds, 256 slots. The forward beside it: ssdlite320_mobilenet_v3_large, K = 91, synthetic weights, batch 64.
The tracker is warmed up over 10 frames; every round restarts from that state and steps through the next 50 frames. Medians over the rounds:
  update_us        one dn_track_update launch (device events around the 50 steps, divided by 50)
  update_empty_us  the same with no detection and no track in any stream: the launch, the state's round trip and the outputs
  update_full_us   the same at the limits: 256 live tracks and 512 rows per stream (a grid of disjoint boxes)
  forward_ms       forward_batch alone, batch 64, resident input
  device_ms        forward_batch + ByteTracker.update behind it on the same stream: a frame step of the product path
  host_track_ms    device-to-host copy of the frame's detections + tests/track_ref.RefTracker.update for all streams (host clock)
  today_ms         forward_ms + host_track_ms: what a user composes without this feature
The device tracker and the restatement are compared bit for bit over the warm-up and the first 10 timed frames before any time is taken. One JSON document on stdout
(and in --out)."""
import argparse
import copy
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
import track_ref as tr  # noqa: E402
from demonet_amd import models, synth  # noqa: E402
from demonet_amd.track import ByteTracker  # noqa: E402

MODEL, K, H, W = "ssdlite320_mobilenet_v3_large", 91, 320, 320
WARM, STEPS, D, CHECKED = 10, 50, 160, 10


def _events_ms(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=3)
    ap.add_argument("--streams", type=int, default=64)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    B = a.streams
    m = models.load_synthetic(getattr(models, MODEL)(num_classes=K), 0).cuda().eval()
    images = torch.from_numpy(synth.images(64, B, H, W)).cuda()
    frames, _ = tr.scene(64, WARM + STEPS, B, D, objects=112, size=2000.0, false_positives=5, exits=False)
    dev_frames = [[torch.from_numpy(x).cuda() for x in fr] for fr in frames]
    tracker = ByteTracker(B, "cuda")
    ref = tr.RefTracker(B, 256)

    # agreement first: the warm-up and the first CHECKED timed frames
    same = True
    for i, (fr, dfr) in enumerate(zip(frames, dev_frames)):
        if i == WARM:
            warm_state, warm_ref = tracker.state_dict(), copy.deepcopy(ref)
        got = [t.cpu().numpy() for t in tracker.update(*dfr)]
        if i < WARM + CHECKED:
            want = ref.update(*fr)
            same = same and all(x.tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(want, got))
    live = int((tracker.table()["state"] != 0).sum().item())
    out_rows = int(got[5].sum())

    def steps():
        for dfr in dev_frames[WARM:]:
            tracker.update(*dfr)

    def forward():
        return m.forward_batch(images, persistent_input=True)

    def device_frame(dfr):
        forward()
        tracker.update(*dfr)

    def device_steps():
        for dfr in dev_frames[WARM:]:
            device_frame(dfr)

    def host_track():
        r = copy.deepcopy(warm_ref)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for dfr in dev_frames[WARM:WARM + a.host_frames]:
            r.update(*[t.cpu().numpy() for t in dfr])
        return (time.perf_counter() - t0) * 1e3 / a.host_frames

    # the limits: 256 live tracks, 512 rows
    full = ByteTracker(B, "cuda")
    i = np.arange(512)
    grid = np.stack([(i % 32) * 44.0, (i // 32) * 44.0, (i % 32) * 44.0 + 30.0, (i // 32) * 44.0 + 30.0], 1).astype(np.float32)
    fb = torch.from_numpy(np.broadcast_to(grid, (B, 512, 4)).copy()).cuda()
    fs = torch.full((B, 512), 0.9, device="cuda")
    fl = torch.ones((B, 512), dtype=torch.int64, device="cuda")
    fc = torch.full((B,), 512, dtype=torch.int32, device="cuda")
    empty = ByteTracker(B, "cuda")
    ec = torch.zeros((B,), dtype=torch.int32, device="cuda")
    for _ in range(3):
        full.update(fb, fs, fl, fc)
        empty.update(fb, fs, fl, ec)
        forward()
    torch.cuda.synchronize()

    times = dict(update_us=[], update_empty_us=[], update_full_us=[], forward_ms=[], device_ms=[], host_track_ms=[])
    for _ in range(a.rounds):
        tracker.load_state_dict(warm_state)
        times["update_us"].append(_events_ms(steps) * 1e3 / STEPS)
        times["update_empty_us"].append(_events_ms(lambda: empty.update(fb, fs, fl, ec), 20) * 1e3)
        times["update_full_us"].append(_events_ms(lambda: full.update(fb, fs, fl, fc), 20) * 1e3)
        times["forward_ms"].append(_events_ms(forward, STEPS))
        tracker.load_state_dict(warm_state)
        times["device_ms"].append(_events_ms(device_steps) / STEPS)
        times["host_track_ms"].append(host_track())
    med = {k: round(statistics.median(v), 4) for k, v in times.items()}
    med["today_ms"] = round(med["forward_ms"] + med["host_track_ms"], 4)
    doc = dict(model=MODEL, num_classes=K, image=[H, W], streams=B, rows=D, detections_per_stream_and_frame=round(float(np.mean([f[3].mean() for f in frames])), 1),
               live_tracks_at_the_end=live, output_rows_last_frame=out_rows, device_equals_restatement=bool(same), frames_compared=WARM + CHECKED, warm_frames=WARM, steps=STEPS,
               rounds=a.rounds, host_frames=a.host_frames, device=torch.cuda.get_device_name(0), median=med,
               min={k: round(min(v), 4) for k, v in times.items()}, max={k: round(max(v), 4) for k, v in times.items()})
    doc["update_share_of_device_frame"] = round(med["update_us"] / 1e3 / med["device_ms"], 4)
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
