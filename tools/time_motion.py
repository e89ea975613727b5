"""dev tool: what camera-motion compensation costs, beside the tracker launch and beside what a user composes without it.
    python tools/time_motion.py [--out profiles/motion_timing.json] [--rounds 5] [--streams 64] [--host-streams 2]
The workload: 64 full-HD NV12 surfaces (rows 2048 bytes apart, as a hardware decoder hands them out) of a textured world under a camera that
pans by (16, 8) pixels per frame, and the detections of tools/time_track.py's scene (about 100 per stream and frame in 160 rows), which mask
the blocks under them. Defaults of MotionCompensator: thumbnails of 240 x 135 (k = 8), 98 blocks of 16 x 16 per stream, radius 16.
Every measurement is device events around STEPS calls, divided by STEPS; the measurements of a round alternate; median (min - max) over rounds:
  estimate_us      MotionCompensator.estimate with the frame's detections: thumbnails, block match, fit (three launches)
  reseed_us        estimate on a freshly reset state (the reset outside the events): the thumbnail launch, and a match and a fit launch that
                   find nothing to do -- an upper bound of the thumbnail launch, so luma_bytes / reseed_us is a LOWER bound of its read rate
  compensate_us    ByteTracker.compensate (dn_track_compensate)
  update_us        ByteTracker.update (dn_track_update) alone on the same detections, in the same run
  today_ms         the host composition of today, per frame step, measured on --host-streams streams and scaled to all (host clock): the copy
                   of the luma planes to the host + tests/motion_ref.RefCompensator.estimate + the edit of the filter through table()
Before any time is taken the device is compared with the reference on the host streams (bit for bit). One JSON document on stdout (and --out)."""
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
import motion_ref as mr  # noqa: E402
import track_ref as tr  # noqa: E402
from demonet_amd.frames import FrameBatch  # noqa: E402
from demonet_amd.motion import MotionCompensator  # noqa: E402
from demonet_amd.track import ByteTracker  # noqa: E402

H, W, PITCH, D, STEPS, WARM = 1080, 1920, 2048, 160, 20, 6
HBM_PEAK = 8.0e12          # bytes per second, the MI355X data sheet


def _events_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--host-streams", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    B, hs = a.streams, min(a.host_streams, a.streams)
    worlds = [mr.textured(500 + b % 4, H + 8 * 3, W + 16 * 3, 16) for b in range(4)]
    lumas = [[mr.window(worlds[b % 4], 16 * f, 8 * f, H, W) for b in range(B)] for f in range(3)]          # three camera positions, cycled
    surfaces = []
    uv = torch.full((H // 2, PITCH), 128, dtype=torch.uint8).cuda()[:, :W]           # (the chroma plane is never read: one for all)
    for f in range(3):
        per = []
        for b in range(B):
            y = torch.zeros((H, PITCH), dtype=torch.uint8)
            y[:, :W] = torch.from_numpy(lumas[f][b])
            per.append((y.cuda()[:, :W], uv))
        surfaces.append(per)
    batches = [FrameBatch(B, "cuda", "nv12").set(s) for s in surfaces]
    frames, _ = tr.scene(64, WARM + STEPS, B, D, objects=112, size=1000.0, false_positives=5, exits=False)
    dev = [[torch.from_numpy(x).cuda() for x in fr] for fr in frames]
    mc, tracker, plain = MotionCompensator(B, "cuda"), ByteTracker(B, "cuda"), ByteTracker(B, "cuda")
    ref = mr.RefCompensator(hs)

    same = True
    for i in range(WARM):
        motion, stats = mc.estimate(batches[i % 3], dev[i][0], dev[i][1], dev[i][3])
        tracker.compensate(motion)
        tracker.update(*dev[i])
        plain.update(*dev[i])
        if i < 3:
            wm, wst, wv = ref.estimate(lumas[i % 3][:hs], frames[i][0][:hs], frames[i][1][:hs], frames[i][3][:hs])
            same = same and motion[:hs].cpu().numpy().tobytes() == wm.tobytes() and np.array_equal(stats[:hs].cpu().numpy(), wst) \
                and np.array_equal(mc.vectors()[:hs].cpu().numpy(), wv)
    ok_after_warmup = int(mc.motion[:, 3].sum().item())
    warm = dict(mc=mc.state_dict(), tracker=tracker.state_dict(), plain=plain.state_dict())

    def estimates():
        for k in range(WARM, WARM + STEPS):
            mc.estimate(batches[k % 3], dev[k][0], dev[k][1], dev[k][3])

    def reseeds():
        total = 0.0
        for k in range(WARM, WARM + STEPS):
            mc.reset()
            total += _events_ms(lambda: mc.estimate(batches[k % 3], dev[k][0], dev[k][1], dev[k][3]))
        return total

    def compensates():
        for _ in range(STEPS):
            tracker.compensate(mc.motion)

    def updates():
        for k in range(WARM, WARM + STEPS):
            plain.update(*dev[k])

    def today():
        r = mr.RefCompensator(hs)
        r.estimate(lumas[0][:hs])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = [surfaces[1][b][0].cpu().numpy() for b in range(hs)]
        det = [t[:hs].cpu().numpy() for t in (dev[WARM][0], dev[WARM][1], dev[WARM][3])]
        motion, _, _ = r.estimate(host, *det)
        tab = tracker.table()
        flt, st = tab["filter"][:hs].cpu().numpy(), tab["state"][:hs].cpu().numpy()
        shim = tr.RefTracker(hs, 256)
        shim.filter, shim.state = flt, st
        mr.compensate(shim, motion)
        tab["filter"][:hs] = torch.from_numpy(shim.filter).cuda()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 * B / hs

    times = dict(estimate_us=[], reseed_us=[], compensate_us=[], update_us=[], today_ms=[])
    estimates()
    for _ in range(a.rounds):
        mc.load_state_dict(warm["mc"])
        times["estimate_us"].append(_events_ms(estimates) * 1e3 / STEPS)
        plain.load_state_dict(warm["plain"])
        times["update_us"].append(_events_ms(updates) * 1e3 / STEPS)
        tracker.load_state_dict(warm["tracker"])
        times["compensate_us"].append(_events_ms(compensates) * 1e3 / STEPS)
        times["reseed_us"].append(reseeds() * 1e3 / STEPS)
        tracker.load_state_dict(warm["tracker"])
        times["today_ms"].append(today())
    med = {k: round(statistics.median(v), 3) for k, v in times.items()}
    luma_bytes = B * H * W
    doc = dict(streams=B, frame=[H, W], pitch=PITCH, format="nv12", k=8, thumbnail=[H // 8, W // 8], blocks_per_stream=98, candidates_per_block=1089,
               rows=D, detections_per_stream_and_frame=round(float(np.mean([f[3].mean() for f in frames])), 1),
               streams_ok_after_warmup=ok_after_warmup, device_equals_reference=bool(same), streams_compared=hs, frames_compared=3,
               warm_frames=WARM, steps=STEPS, rounds=a.rounds, host_streams=hs, device=torch.cuda.get_device_name(0),
               luma_bytes_read_per_step=luma_bytes, absolute_differences_per_step=B * 98 * 1089 * 256,
               median=med, min={k: round(min(v), 3) for k, v in times.items()}, max={k: round(max(v), 3) for k, v in times.items()})
    doc["luma_bytes_per_second_lower_bound"] = round(luma_bytes / (med["reseed_us"] * 1e-6))
    doc["fraction_of_hbm_peak_lower_bound"] = round(doc["luma_bytes_per_second_lower_bound"] / HBM_PEAK, 4)
    doc["hbm_peak_bytes_per_second"] = HBM_PEAK
    doc["estimate_over_update"] = round(med["estimate_us"] / med["update_us"], 3)
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
