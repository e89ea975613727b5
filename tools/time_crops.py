"""dev tool: what cutting the tracked objects out of 64 full-HD NV12 surfaces costs through crops.ObjectCropper, and what a user composes without it.
    python tools/time_crops.py [--out profiles/crops_timing.json] [--rounds 7] [--streams 64] [--reps 200] [--today-reps 3]
64 surfaces of 1080 x 1920, each an allocation of its own with a row pitch of 2048 bytes, BT.709 limited range, noise content; 20 boxes per stream
at person-like sizes (40 .. 160 pixels wide, 2 .. 3 times as high, centres anywhere in the frame, so some hang over an edge) in 32 rows; fp16 patches
of 128 x 64 with the ImageNet mean and std, 2048 slots. Both sides run in this process on the same device and are timed alternately, round by round,
with device events around back-to-back calls after a warm-up; medians over the rounds with min and max:
  crop_us         one ObjectCropper call (two launches), `reps` calls back to back
  crop_graph_us   the same call captured once in a graph, `reps` replays
  today_ms        the composition without the feature, per step: every frame converted with the SAME integer formulas in torch ops
                  (tools/time_frames.py), the boxes and counts copied to the host, per box slice + F.interpolate(bilinear, align_corners=False) +
                  normalise, torch.stack
  today_crops_ms  the same without the conversion (the converted frames resident): the per-box part alone
Before any time is taken the device patches of streams 0 and 1 are compared bit for bit with tests/crops_ref.py, and the torch composition's patches
with the device's (largest difference; torch's resize multiplies in another order, so the bits differ). bytes: written = kept patches;
rectangle = every luma and chroma byte of the kept rectangles once (the least a gather must read); tap = the 12 bytes the four taps of every output
pixel ask for. One JSON document on stdout (and in --out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import crops_ref as cr  # noqa: E402
import frames_ref as fr  # noqa: E402
from demonet_amd.crops import ObjectCropper  # noqa: E402
from demonet_amd.frames import FrameBatch  # noqa: E402
from time_frames import torch_nv12_to_rgb  # noqa: E402

H, W, PITCH = 1080, 1920, 2048
MATRIX, FULL = "bt709", False
D, PER_STREAM, SIZE, CAPACITY = 32, 20, (128, 64), 2048


def _events(fn, reps):
    """milliseconds per call of `reps` back-to-back calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def scene(streams, seed=0):
    rng = np.random.default_rng(seed)
    boxes = np.zeros((streams, D, 4), dtype=np.float32)
    w = rng.uniform(40, 160, (streams, D))
    h = w * rng.uniform(2, 3, (streams, D))
    cx, cy = rng.uniform(0, W, (streams, D)), rng.uniform(0, H, (streams, D))
    boxes[:] = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1)
    return boxes, np.full((streams,), PER_STREAM, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--today-reps", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    n = a.streams
    rng = np.random.default_rng(0)
    surfaces = []
    for _ in range(n):
        ybuf = torch.from_numpy(rng.integers(0, 256, (H, PITCH), dtype=np.uint8)).cuda()
        cbuf = torch.from_numpy(rng.integers(0, 256, (H // 2, PITCH), dtype=np.uint8)).cuda()
        surfaces.append((ybuf[:, :W], cbuf[:, :W]))
    batch = FrameBatch(n, "cuda", "nv12", MATRIX, FULL).set(surfaces)
    boxes_np, counts_np = scene(n)
    boxes, counts = torch.from_numpy(boxes_np).cuda(), torch.from_numpy(counts_np).cuda()
    p = cr.params(SIZE, capacity=CAPACITY, fp16=True, mean=cr.IMAGENET_MEAN, std=cr.IMAGENET_STD)
    cropper = ObjectCropper(n, "cuda", size=SIZE, capacity=CAPACITY, dtype=torch.float16, mean=p.mean, std=p.std)
    mean = torch.tensor(p.mean, device="cuda").view(3, 1, 1)
    std = torch.tensor(p.std, device="cuda").view(3, 1, 1)

    def crop():
        return cropper(batch, boxes, counts)

    def today_crops(frames):
        hb, hc = boxes.cpu().numpy(), counts.cpu().numpy()          # the host round trip of every step
        index, kept, _ = cr.rects(hb, hc, [(H, W)] * n, None, p)      # (the rectangle rules on the host, as a user would write them)
        out = []
        for b, _, x0, y0, w, h in index[:kept, :6].tolist():
            c = frames[b][y0:y0 + h, x0:x0 + w].permute(2, 0, 1).unsqueeze(0).float().div_(255)
            c = Fn.interpolate(c, size=SIZE, mode="bilinear", align_corners=False)[0]
            out.append(((c - mean) / std).half())
        return torch.stack(out)

    def convert():
        return [torch_nv12_to_rgb(y, uv) for y, uv in surfaces]

    def today():
        return today_crops(convert())

    # agreement first
    patches, index, totals = (t.clone() for t in crop())
    torch.cuda.synchronize()
    kept, dropped = int(totals[0]), int(totals[1])
    hidx = index.cpu().numpy()
    want_index, want_kept, want_dropped = cr.rects(boxes_np, counts_np, [(H, W)] * n, None, p)
    index_equals_ref = bool(np.array_equal(hidx, want_index)) and (kept, dropped) == (want_kept, want_dropped)
    checked = int((hidx[:kept, 0] < 2).sum())
    rgbs = []
    for y, uv in surfaces[:2]:
        y0, c0 = y.cpu().numpy(), uv.cpu().numpy()
        rgbs.append(fr.planes_to_rgb(y0, c0[:, 0::2], c0[:, 1::2], MATRIX, FULL))
    want = cr.patches(rgbs, want_index, checked, p)
    patches_equal_ref = bool(patches[:checked].cpu().numpy().tobytes() == want.tobytes())
    resident = convert()
    composed = today_crops(resident)
    today_max_abs_diff = float((composed.float() - patches[:kept].float()).abs().max())

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        crop()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        crop()
    for _ in range(20):      # every shape of the timed windows
        crop()
        graph.replay()
    today()
    torch.cuda.synchronize()

    times = dict(crop_us=[], crop_graph_us=[], today_ms=[], today_crops_ms=[])
    for _ in range(a.rounds):
        times["crop_us"].append(_events(crop, a.reps) * 1e3)
        times["today_ms"].append(_events(today, a.today_reps))
        times["crop_graph_us"].append(_events(graph.replay, a.reps) * 1e3)
        times["today_crops_ms"].append(_events(lambda: today_crops(resident), a.today_reps))
    rect = hidx[:kept, 4].astype(np.int64) * hidx[:kept, 5]
    written = kept * 3 * SIZE[0] * SIZE[1] * 2
    rectangle = int(rect.sum() + (rect // 2).sum())
    taps = kept * SIZE[0] * SIZE[1] * 12
    med = {k: round(statistics.median(v), 3) for k, v in times.items()}
    sec = med["crop_graph_us"] * 1e-6
    doc = dict(streams=n, surface=[H, W], pitch=PITCH, format="nv12", matrix=MATRIX, full_range=FULL, rows=D, boxes_per_stream=PER_STREAM,
               patch=list(SIZE), dtype="float16", capacity=CAPACITY, patches=kept, dropped=dropped,
               mean_rectangle=[round(float(hidx[:kept, 5].mean()), 1), round(float(hidx[:kept, 4].mean()), 1)],
               index_equals_ref=index_equals_ref, patches_equal_ref=patches_equal_ref, patches_compared=checked,
               today_max_abs_diff=today_max_abs_diff, bytes_written=written, rectangle_bytes=rectangle, tap_bytes=taps,
               written_gb_per_s=round(written / sec / 1e9, 1), rectangle_gb_per_s=round(rectangle / sec / 1e9, 1),
               tap_gb_per_s=round(taps / sec / 1e9, 1), rounds=a.rounds, reps=a.reps, today_reps=a.today_reps,
               device=torch.cuda.get_device_name(0), median=med, min={k: round(min(v), 3) for k, v in times.items()},
               max={k: round(max(v), 3) for k, v in times.items()})
    doc["speedup_over_today"] = round(med["today_ms"] * 1e3 / med["crop_us"], 1)
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
