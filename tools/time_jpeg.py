"""Times the baseline JPEG encoder (demonet_amd/jpeg.py) on the MI355X against the composition available without it, and writes
profiles/jpeg_timing.json.

    python tools/time_jpeg.py [--streams 64] [--steps 20] [--today-steps 3] [--rounds 5] [--out profiles/jpeg_timing.json]

Three workloads per step, 64 full-HD NV12 surfaces (pitch 2048) of a smooth synthetic picture with noise on it as the source:
    frames    the 64 whole frames at quality 85 from a BT.601 full-range batch (the plane-wise path)
    rgb       the same surfaces declared limited-range BT.709 (the RGB path)
    objects   1280 rectangles of about 128 x 64 (height x width) from an ObjectCropper's index table, quality 85 (encode_objects)
"today" is the same product made without the encoder: Compositor NV12 -> RGB24 of the whole frames, one copy of the RGB surfaces to the host, and
PIL save(format="JPEG", quality=85, subsampling=2) of every frame or every rectangle on 16 threads. Our times are device events around `steps`
calls after a warm-up, `rounds` times: median and range; today's are host wall times around the same number of rounds of `today-steps` steps, with a
synchronise at both ends. Before a workload is timed every file it produced is opened with PIL and its size checked, and the first file's luma is
compared with the source (`files_open`, `luma_mae`). The pixel rate is source pixels coded per second; it is set against the Compositor's wall rate
of profiles/compose_timing.json (bytes read per second / 1.5 bytes per NV12 pixel)."""
import argparse
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from demonet_amd import compose, jpeg  # noqa: E402
from demonet_amd.crops import ObjectCropper  # noqa: E402
from demonet_amd.frames import FrameBatch  # noqa: E402

DEV = "cuda:0"
H, W, PITCH = 1080, 1920, 2048
QUALITY = 85
THREADS = 16


def picture(seed):
    """(Y [H, PITCH], UV [H / 2, PITCH]) uint8 on the device: smooth gradients and discs with +-6 of noise, so that the files have the size of a
    camera picture's rather than of noise's"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, device=DEV, dtype=torch.float32), torch.arange(PITCH, device=DEV, dtype=torch.float32), indexing="ij")
    base = 128 + 70 * torch.sin(xx / (90.0 + seed)) * torch.cos(yy / (60.0 + 2 * seed)) + 30 * ((xx // 160 + yy // 120) % 2)
    y = (base + torch.randint(-6, 7, (H, PITCH), device=DEV, generator=g)).clamp_(0, 255).to(torch.uint8)
    cb = 128 + 40 * torch.sin(xx[::2] / 200.0 + seed) + torch.randint(-3, 4, (H // 2, PITCH), device=DEV, generator=g)
    return y, cb.clamp_(0, 255).to(torch.uint8)


def device_timed(fn, steps, rounds):
    fn()
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / steps)
    return dict(median_us=round(statistics.median(out), 1), min_us=round(min(out), 1), max_us=round(max(out), 1))


def host_timed(fn, steps, rounds):
    fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / steps)
    return dict(median_us=round(statistics.median(out), 1), min_us=round(min(out), 1), max_us=round(max(out), 1))


def main():
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--today-steps", type=int, default=3)
    ap.add_argument("--objects-per-stream", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_jpeg.py measures on the GPU; there is none here")
    n = args.streams
    full = [picture(s) for s in range(n)]
    sources = [(y[:, :W], uv[:, :W]) for y, uv in full]
    planes = FrameBatch(n, DEV, format="nv12", matrix="bt601", full_range=True).set(sources)
    limited = FrameBatch(n, DEV, format="nv12", matrix="bt709", full_range=False).set(sources)
    rgbs = [torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV) for _ in range(n)]
    rgb_batch = FrameBatch(n, DEV, format="rgb24").set(rgbs)
    pool = ThreadPoolExecutor(THREADS)
    result = dict(streams=n, frame=[H, W], pitch=PITCH, quality=QUALITY, steps=args.steps, rounds=args.rounds, today_steps=args.today_steps, threads=THREADS,
                  device=torch.cuda.get_device_name(0), workloads={})
    wall_rate = None
    comp_json = os.path.join(ROOT, "profiles", "compose_timing.json")
    if os.path.exists(comp_json):
        wall_rate = json.load(open(comp_json))["workloads"]["wall"]["read_bytes_per_second"] / 1.5
        result["compositor_wall_pixels_per_second"] = round(wall_rate)

    def save(arr):
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, format="JPEG", quality=QUALITY, subsampling=2)
        return buf.getbuffer().nbytes

    def today(batch, rects):
        comp = compose.Compositor(n, DEV).set([(i, i, (0, 0, W, H)) for i in range(n)], batch, rgb_batch)

        def step():
            comp(batch, rgb_batch)
            host = [t.cpu().numpy() for t in rgbs]
            if rects is None:
                return sum(pool.map(save, host))
            return sum(pool.map(lambda r: save(np.ascontiguousarray(host[r[0]][r[2]:r[2] + r[4], r[1]:r[1] + r[3]])), rects))
        return step

    def measure(name, enc, run, batch, rects, pixels):
        run()
        files = enc.files()
        written = [f for f in files if f is not None]
        want = [(W, H)] * n if rects is None else [(r[3], r[4]) for r in rects]
        assert len(written) == len(want), (name, len(written), len(want), enc.totals.tolist())
        for f, size in zip(written, want):
            im = Image.open(io.BytesIO(f))
            im.load()
            assert im.size == size, (name, im.size, size)
        luma_mae = None
        if rects is None:
            im = Image.open(io.BytesIO(written[0]))
            im.draft("YCbCr", im.size)
            got = np.asarray(im.convert("YCbCr"), np.int64)[..., 0]
            if name == "frames":
                luma_mae = round(float(np.abs(got - sources[0][0].cpu().numpy().astype(np.int64)).mean()), 3)
        ours = device_timed(run, args.steps, args.rounds)
        step = today(batch, rects)
        today_bytes = step()
        base = host_timed(step, args.today_steps, args.rounds)
        rate = pixels / (ours["median_us"] * 1e-6)
        result["workloads"][name] = dict(files=len(written), files_open=True, luma_mae=luma_mae, kernel=ours, today=base, bytes_produced=int(enc.totals[2]),
                                         bytes_of_files=sum(len(f) for f in written), today_bytes_of_files=int(today_bytes), source_pixels=pixels,
                                         pixels_per_second=round(rate), pixel_rate_over_compositor_wall=round(rate / wall_rate, 4) if wall_rate else None,
                                         today_over_kernel=round(base["median_us"] / ours["median_us"], 1))
        print(name, json.dumps(result["workloads"][name]), flush=True)

    items = [jpeg.Item(i) for i in range(n)]
    enc = jpeg.JpegEncoder(n, DEV, arena_bytes=n * (2 << 20), quality=QUALITY).set(items, planes)
    measure("frames", enc, lambda: enc.encode(planes), planes, None, n * H * W)
    enc2 = jpeg.JpegEncoder(n, DEV, arena_bytes=n * (2 << 20), quality=QUALITY).set(items, limited)
    measure("rgb", enc2, lambda: enc2.encode(limited), limited, None, n * H * W)
    # objects: boxes of about 64 x 128 on a grid, through a real cropper step
    d = args.objects_per_stream
    rng = np.random.default_rng(5)
    boxes = np.zeros((n, d, 4), np.float32)
    for b in range(n):
        for j in range(d):
            x0, y0 = 40 + (j % 10) * 180 + rng.integers(0, 40), 60 + (j // 10) * 400 + rng.integers(0, 200)
            boxes[b, j] = (x0, y0, x0 + 64 + rng.integers(-8, 9), y0 + 128 + rng.integers(-16, 17))
    cropper = ObjectCropper(n, DEV, size=(128, 64), capacity=n * d, dtype=torch.float16)
    _, index, totals = cropper(limited, torch.from_numpy(boxes).to(DEV), torch.full((n,), d, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    kept = int(totals[0])
    rows = index[:kept].cpu().numpy()
    rects = [(int(r[0]), int(r[2]) & ~1, int(r[3]) & ~1, int(r[4]) + (int(r[2]) & 1), int(r[5]) + (int(r[3]) & 1)) for r in rows]
    enc3 = jpeg.JpegEncoder(n * d, DEV, arena_bytes=n * d * (16 << 10), quality=QUALITY, max_segments=n * d * 12)
    measure("objects", enc3, lambda: enc3.encode_objects(limited, cropper), limited, rects, sum(r[3] * r[4] for r in rects))
    result["workloads"]["objects"]["rectangles"] = kept
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
