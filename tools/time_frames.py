"""dev tool: what 64 full-HD NV12 surfaces cost through SSD.forward_frames, and what a user composes without it.
    python tools/time_frames.py [--out profiles/frames_timing.json] [--rounds 5] [--frames 64]
64 surfaces of 1080 x 1920, each an allocation of its own with a row pitch of 2048 bytes (as a hardware decoder hands them out), BT.709 limited
range, noise content. The forward: ssdlite320_mobilenet_v3_large, K = 91, synthetic weights. Both sides run in this process on the same
device and are timed alternately, round by round, with device events around `reps` back-to-back calls after a warm-up; medians over the rounds:
  frames_ms         forward_frames on a FrameBatch that names the surfaces (the records are set once; the graph replays)
  frames_set_ms     the same with FrameBatch.set(surfaces) in front of every forward (validation + the upload of 64 records), host clock incl. sync
  today_ms          the composition without the feature: the SAME integer formulas in torch ops per surface -> torch.stack -> forward_uint8
  today_convert_ms  its conversion and stack alone
  uint8_ms          forward_uint8 alone on the stacked block (resident)
  resident_ms       forward_batch on a resident float batch at the network size: the forward without any input stage
Before any time is taken the torch composition is compared with tests/frames_ref.py on one surface and the two paths' detections with each other,
bit for bit. One JSON document on stdout (and in --out)."""
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
import frames_ref as fr  # noqa: E402
from demonet_amd import models, synth  # noqa: E402
from demonet_amd.frames import FrameBatch  # noqa: E402

MODEL, K = "ssdlite320_mobilenet_v3_large", 91
H, W, PITCH = 1080, 1920, 2048
MATRIX, FULL = "bt709", False


def _events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def torch_nv12_to_rgb(y, uv):
    """[h, w, 3] uint8 of one surface (y [h, w], uv [h / 2, w] views, any pitch): the integer formulas of include/demonet_hip.h in torch ops"""
    cy, crv, cbu, cgu, cgv, yo = fr.int_coeffs(MATRIX, FULL)
    c = uv.unflatten(1, (-1, 2)).to(torch.int32) - 128
    c = c.repeat_interleave(2, 0).repeat_interleave(2, 1)          # chroma sample (x >> 1, y >> 1)
    u, v = c[..., 0], c[..., 1]
    l = (y.to(torch.int32) - yo) * cy + (1 << 13)
    rgb = torch.stack([l + crv * v, l - cgu * u - cgv * v, l + cbu * u], -1) >> 14
    return rgb.clamp_(0, 255).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--today-reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    n = a.frames
    m = models.load_synthetic(getattr(models, MODEL)(num_classes=K), 0).cuda().eval()
    Wn, Hn = m.graph.size
    rng = np.random.default_rng(0)
    surfaces = []
    for i in range(n):
        ybuf = torch.from_numpy(rng.integers(0, 256, (H, PITCH), dtype=np.uint8)).cuda()
        cbuf = torch.from_numpy(rng.integers(0, 256, (H // 2, PITCH), dtype=np.uint8)).cuda()
        surfaces.append((ybuf[:, :W], cbuf[:, :W]))
    batch = FrameBatch(n, "cuda", "nv12", MATRIX, FULL).set(surfaces)
    resident = torch.from_numpy(synth.images(64, n, Hn, Wn)).cuda()

    def convert():
        return torch.stack([torch_nv12_to_rgb(y, uv) for y, uv in surfaces])

    def today():
        return m.forward_uint8(convert())

    def frames():
        return m.forward_frames(batch)

    # agreement first
    y0, c0 = surfaces[0][0].cpu().numpy(), surfaces[0][1].cpu().numpy()
    want = fr.planes_to_rgb(y0, c0[:, 0::2], c0[:, 1::2], MATRIX, FULL)
    conversion_equals_ref = bool(np.array_equal(torch_nv12_to_rgb(*surfaces[0]).cpu().numpy(), want))
    block = convert()
    ref = [t.clone() for t in m.forward_uint8(block)]
    got = [t.clone() for t in frames()]
    same = all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(got, ref))
    detections = int(ref[3].sum())

    def set_and_forward():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            m.forward_frames(batch.set(surfaces))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.reps

    for _ in range(3):      # every shape of the timed windows
        frames()
        m.forward_uint8(block)
        m.forward_batch(resident, persistent_input=True)
    today()
    torch.cuda.synchronize()

    times = dict(frames_ms=[], frames_set_ms=[], today_ms=[], today_convert_ms=[], uint8_ms=[], resident_ms=[])
    for _ in range(a.rounds):
        times["frames_ms"].append(_events_ms(frames, a.reps))
        times["today_ms"].append(_events_ms(today, a.today_reps))
        times["frames_set_ms"].append(set_and_forward())
        times["today_convert_ms"].append(_events_ms(convert, a.today_reps))
        times["uint8_ms"].append(_events_ms(lambda: m.forward_uint8(block), a.reps))
        times["resident_ms"].append(_events_ms(lambda: m.forward_batch(resident, persistent_input=True), a.reps))
    med = {k: round(statistics.median(v), 4) for k, v in times.items()}
    surface_bytes = H * W * 3 // 2
    doc = dict(model=MODEL, num_classes=K, frames=n, surface=[H, W], pitch=PITCH, format="nv12", matrix=MATRIX, full_range=FULL, network=[Hn, Wn],
               surface_bytes=surface_bytes, rgb_block_bytes=n * H * W * 3, network_input_bytes=n * 3 * Hn * Wn * 4,
               taps_per_forward=n * Hn * Wn * 4, tap_bytes=3,
               conversion_equals_ref=conversion_equals_ref, detections_equal_today=bool(same), detections=detections,
               rounds=a.rounds, reps=a.reps, today_reps=a.today_reps, device=torch.cuda.get_device_name(0), median=med,
               min={k: round(min(v), 4) for k, v in times.items()}, max={k: round(max(v), 4) for k, v in times.items()})
    doc["input_stage_ms"] = round(med["frames_ms"] - med["resident_ms"], 4)
    doc["speedup_over_today"] = round(med["today_ms"] / med["frames_ms"], 2)
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
