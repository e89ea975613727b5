"""dev tool: sliced inference on 8 full-HD NV12 surfaces through sliced.FrameSlicer, and what a user composes without it.
    python tools/time_sliced_frames.py [--out profiles/sliced_frames_timing.json] [--rounds 5] [--frames 8]
8 surfaces of 1080 x 1920, each an allocation of its own with a row pitch of 2048 bytes, BT.709 limited range, noise content. The forward:
ssdlite320_mobilenet_v3_large, K = 91, synthetic weights; default tile (320) and overlap: 40 tiles + the whole frame = 41 regions per frame.
Both sides run in this process on the same device and are timed alternately, round by round, with device events around `reps` back-to-back
steps after a warm-up; medians over the rounds:
  slicer_ms          slicer(batch): every region of every frame through shared forwards, one merge, padded device tensors (no host wait)
  list_ms            SSD.detect_sliced_frames(batch): the same plus the one host copy of the counts and the per-frame views
  track_ms           SSD.track_sliced_frames(batch, tracker, slicer): slicer(batch) + ByteTracker.update
  today_ms           the composition without the feature: per surface the SAME integer formulas in torch ops -> [3, H, W] float image ->
                     SSD.detect_sliced(image)
  today_convert_ms   its conversions alone
Before any time is taken the torch conversion is compared with tests/frames_ref.py on one surface and the two sides' detections with each
other, bit for bit (the float image is divided by a 255 held in a tensor: true division, as the kernel's). One JSON document on stdout (and in --out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import frames_ref as fr  # noqa: E402
from demonet_amd import models  # noqa: E402
from demonet_amd.frames import FrameBatch  # noqa: E402
from demonet_amd.sliced import FrameSlicer  # noqa: E402
from demonet_amd.track import ByteTracker  # noqa: E402
from time_frames import H, MATRIX, FULL, PITCH, W, _events_ms, torch_nv12_to_rgb  # noqa: E402

MODEL, K = "ssdlite320_mobilenet_v3_large", 91


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--today-reps", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    n = a.frames
    m = models.load_synthetic(getattr(models, MODEL)(num_classes=K), 0).cuda().eval()
    rng = np.random.default_rng(0)
    surfaces = []
    for i in range(n):
        ybuf = torch.from_numpy(rng.integers(0, 256, (H, PITCH), dtype=np.uint8)).cuda()
        cbuf = torch.from_numpy(rng.integers(0, 256, (H // 2, PITCH), dtype=np.uint8)).cuda()
        surfaces.append((ybuf[:, :W], cbuf[:, :W]))
    batch = FrameBatch(n, "cuda", "nv12", MATRIX, FULL).set(surfaces)
    slicer = FrameSlicer(m, batch.sizes)
    tracker = ByteTracker(n, "cuda")
    d255 = torch.tensor(255.0, device="cuda")

    def convert():
        return [torch_nv12_to_rgb(y, uv).permute(2, 0, 1).to(torch.float32).div(d255).contiguous() for y, uv in surfaces]

    def today():
        return [m.detect_sliced(img)[0] for img in convert()]

    # agreement first
    y0, c0 = surfaces[0][0].cpu().numpy(), surfaces[0][1].cpu().numpy()
    want = fr.planes_to_rgb(y0, c0[:, 0::2], c0[:, 1::2], MATRIX, FULL)
    conversion_equals_ref = bool(np.array_equal(torch_nv12_to_rgb(*surfaces[0]).cpu().numpy(), want))
    host = (want.transpose(2, 0, 1).astype(np.float32) / np.float32(255))
    float_image_equals_host_division = bool(np.array_equal(convert()[0].cpu().numpy().view(np.int32), host.view(np.int32)))
    ref = today()
    got = m.detect_sliced_frames(batch)
    same = all(torch.equal(_bits(x[k]), _bits(y[k])) if x[k].shape == y[k].shape else False for x, y in zip(got, ref) for k in ("boxes", "scores", "labels"))
    detections = sum(len(d["scores"]) for d in ref)

    for _ in range(3):      # every shape of the timed windows
        slicer(batch)
        m.detect_sliced_frames(batch)
        m.track_sliced_frames(batch, tracker, slicer)
    today()
    torch.cuda.synchronize()

    times = dict(slicer_ms=[], list_ms=[], track_ms=[], today_ms=[], today_convert_ms=[])
    for _ in range(a.rounds):
        times["slicer_ms"].append(_events_ms(lambda: slicer(batch), a.reps))
        times["today_ms"].append(_events_ms(today, a.today_reps))
        times["list_ms"].append(_events_ms(lambda: m.detect_sliced_frames(batch), a.reps))
        times["today_convert_ms"].append(_events_ms(convert, a.today_reps))
        times["track_ms"].append(_events_ms(lambda: m.track_sliced_frames(batch, tracker, slicer), a.reps))
    med = {k: round(statistics.median(v), 4) for k, v in times.items()}
    M = slicer.max_tiles_per_forward
    doc = dict(model=MODEL, num_classes=K, frames=n, surface=[H, W], pitch=PITCH, format="nv12", matrix=MATRIX, full_range=FULL, network=list(m.graph.size)[::-1],
               regions_per_frame=slicer.S // n, regions=slicer.S, max_tiles_per_forward=M, forwards_per_step=(slicer.S + M - 1) // M,
               today_forwards_per_step=2 * n, conversion_equals_ref=conversion_equals_ref, float_image_equals_host_division=float_image_equals_host_division,
               detections_equal_today=bool(same), detections=detections, rounds=a.rounds, reps=a.reps, today_reps=a.today_reps,
               device=torch.cuda.get_device_name(0), median=med, min={k: round(min(v), 4) for k, v in times.items()},
               max={k: round(max(v), 4) for k, v in times.items()})
    doc["today_over_list"] = round(med["today_ms"] / med["list_ms"], 2)
    doc["today_over_slicer"] = round(med["today_ms"] / med["slicer_ms"], 2)
    doc["track_ms_per_frame_step"] = med["track_ms"]
    doc["not_measured"] = ["the region kernel alone under a profiler", "I420 and the RGB formats", "other frame sizes and mixed sizes", "tiles that are resized (tile != network size)",
                           "other max_tiles_per_forward than 64", "detect_tta_frames against detect_tta", "trained weights (the merge sees synthetic-weight detections)"]
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
