"""Times the surface composition (demonet_amd/compose.py) on the MI355X against the composition available without it, and writes
profiles/compose_timing.json.

    python tools/time_compose.py [--streams 64] [--steps 1000] [--today-steps 10] [--rounds 5] [--out profiles/compose_timing.json]

Three workloads per step, 64 full-HD NV12 surfaces (pitch 2048) as the source:
    wall      into one 3840 x 2160 NV12 surface, 8 x 8 cells of 480 x 270 (the plane-wise path, 4:1)
    previews  into 64 NV12 surfaces of 640 x 360 (the plane-wise path, 3:1)
    rgb       into 64 RGB24 surfaces of 1920 x 1080 (the RGB path, 1:1)
"today" is the same result made with torch on the same device: NV12 -> float RGB (chroma replicated, the matrix), F.interpolate(mode="area"),
RGB -> YUV with a 2 x 2 chroma mean where the destination is NV12, and one slice assignment per cell or surface. Times are device events around
`steps` calls after a warm-up, `rounds` times: median and range. Before a workload is timed its output is compared, byte for byte, with the
header's arithmetic written out in torch integers for these integer ratios (block sums, (sum + D / 2) / D; the integer YUV -> RGB formulas); the
result is recorded as `device_equals_exact`, and a mismatch ends the run. Bytes are the payload bytes a step must read and write, counted from the shapes.
The yardstick of the wall is the luma read rate of the motion thumbnail kernel in profiles/motion_timing.json (each source byte read once, little
written)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from demonet_amd import compose  # noqa: E402
from demonet_amd.frames import FrameBatch  # noqa: E402

DEV = "cuda:0"
H, W, PITCH = 1080, 1920, 2048
KR, KB = 0.2126, 0.0722


def nv12_surface(h, w, pitch, gen):
    y = torch.randint(0, 256, (h, pitch), dtype=torch.uint8, device=DEV, generator=gen)
    uv = torch.randint(0, 256, (h // 2, pitch), dtype=torch.uint8, device=DEV, generator=gen)
    return y[:, :w], uv[:, :w]


def to_rgb(y, uv):
    """[3, h, w] float RGB of a limited-range BT.709 NV12 surface, chroma replicated"""
    h, w = y.shape
    yy = (y.float() - 16.0) * (255.0 / 219.0)
    c = uv.reshape(h // 2, w // 2, 2).float() - 128.0
    c = c.repeat_interleave(2, 0).repeat_interleave(2, 1) * (255.0 / 224.0)
    u, v = c[..., 0], c[..., 1]
    kg = 1.0 - KR - KB
    r = yy + 2 * (1 - KR) * v
    b = yy + 2 * (1 - KB) * u
    g = yy - 2 * KB * (1 - KB) / kg * u - 2 * KR * (1 - KR) / kg * v
    return torch.stack([r, g, b]).clamp_(0, 255)


def to_nv12(rgb):
    """(Y [h, w], UV [h / 2, w]) uint8 of a [3, h, w] float RGB image, chroma from the 2 x 2 mean"""
    kg = 1.0 - KR - KB
    r, g, b = rgb[0], rgb[1], rgb[2]
    y = KR * r + kg * g + KB * b
    m = F.avg_pool2d(rgb[None], 2)[0]
    ym = KR * m[0] + kg * m[1] + KB * m[2]
    u = (m[2] - ym) / (2 * (1 - KB)) * (224.0 / 255.0) + 128.0
    v = (m[0] - ym) / (2 * (1 - KR)) * (224.0 / 255.0) + 128.0
    yq = (y * (219.0 / 255.0) + 16.5).clamp_(0, 255).to(torch.uint8)
    uvq = (torch.stack([u, v], -1) + 0.5).clamp_(0, 255).to(torch.uint8)
    return yq, uvq.reshape(uvq.shape[0], -1)


def today(sources, dests, rects, rgb_out):
    for (y, uv), dst, (x0, y0, w, h) in zip(sources, dests, rects):
        rgb = to_rgb(y, uv)
        if (h, w) != tuple(rgb.shape[1:]):
            rgb = F.interpolate(rgb[None], size=(h, w), mode="area")[0]
        if rgb_out:
            dst[y0:y0 + h, x0:x0 + w] = (rgb + 0.5).clamp_(0, 255).to(torch.uint8).permute(1, 2, 0)
        else:
            yq, uvq = to_nv12(rgb)
            dst[0][y0:y0 + h, x0:x0 + w] = yq
            dst[1][y0 // 2:(y0 + h) // 2, x0:x0 + w] = uvq


def block_mean(p, k):
    """(sum + D / 2) / D over k x k blocks of a [h, w] uint8 plane, D = k k: the header's area filter at an integer ratio"""
    h, w = p.shape
    s = p.to(torch.int32).reshape(h // k, k, w // k, k).sum((1, 3))
    return ((s + k * k // 2) // (k * k)).to(torch.uint8)


def exact(sources, dests, rects, rgb_out):
    """whether every destination rectangle holds what include/demonet_hip.h defines (integer ratios only)"""
    for (y, uv), dst, (x0, y0, w, h) in zip(sources, dests, rects):
        if rgb_out:             # 1:1, BT.709 limited: round(c 2^14) of the header, chroma sample (x >> 1, y >> 1)
            yy = (y.to(torch.int32) - 16) * 19077 + (1 << 13)
            c = uv.reshape(uv.shape[0], -1, 2).to(torch.int32).repeat_interleave(2, 0).repeat_interleave(2, 1) - 128
            u, v = c[..., 0], c[..., 1]
            want = torch.stack([(yy + 29372 * v) >> 14, (yy - 3494 * u - 8731 * v) >> 14, (yy + 34610 * u) >> 14], -1).clamp_(0, 255).to(torch.uint8)
            if not torch.equal(dst[y0:y0 + h, x0:x0 + w], want):
                return False
            continue
        k = y.shape[0] // h
        cuv = uv.reshape(uv.shape[0], -1, 2)
        want_uv = torch.stack([block_mean(cuv[..., 0], k), block_mean(cuv[..., 1], k)], -1).reshape(h // 2, w)
        if not (torch.equal(dst[0][y0:y0 + h, x0:x0 + w], block_mean(y, k)) and torch.equal(dst[1][y0 // 2:(y0 + h) // 2, x0:x0 + w], want_uv)):
            return False
    return True


def timed(fn, steps, rounds):
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
    return dict(median_us=round(statistics.median(out), 3), min_us=round(min(out), 3), max_us=round(max(out), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--today-steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compose_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_compose.py measures on the GPU; there is none here")
    n = args.streams
    gen = torch.Generator(device=DEV).manual_seed(7)
    sources = [nv12_surface(H, W, PITCH, gen) for _ in range(n)]
    src = FrameBatch(n, DEV, format="nv12").set(sources)
    src_bytes = n * H * W * 3 // 2
    result = dict(streams=n, frame=[H, W], pitch=PITCH, format="nv12", steps=args.steps, rounds=args.rounds, today_steps=args.today_steps,
                  device=torch.cuda.get_device_name(0), workloads={})

    def measure(name, dst_batch, dests, items, rects, rgb_out, written):
        comp = compose.Compositor(max(n, 1), DEV).set(items, src, dst_batch)
        comp(src, dst_batch)
        torch.cuda.synchronize()
        if not exact(sources, dests, rects, rgb_out):
            raise SystemExit("time_compose.py: the output of '{}' differs from the header's arithmetic; nothing was timed".format(name))
        ours = timed(lambda: comp(src, dst_batch), args.steps, args.rounds)
        base = timed(lambda: today(sources, dests, rects, rgb_out), args.today_steps, args.rounds)
        moved = src_bytes + written
        result["workloads"][name] = dict(device_equals_exact=True, kernel=ours, today=base, bytes_read_per_step=src_bytes, bytes_written_per_step=written, tiles=comp.tiles,
                                         bytes_per_second=round(moved / (ours["median_us"] * 1e-6)),
                                         read_bytes_per_second=round(src_bytes / (ours["median_us"] * 1e-6)),
                                         today_over_kernel=round(base["median_us"] / ours["median_us"], 1))
        print(name, json.dumps(result["workloads"][name]), flush=True)

    # (a) the wall
    cols = 8
    rows = (n + cols - 1) // cols
    wall = nv12_surface(270 * rows, 480 * cols, 480 * cols, gen)
    wall_batch = FrameBatch(1, DEV, format="nv12").set([wall])
    items = compose.grid(src.sizes, wall_batch.sizes[0], rows, cols)
    measure("wall", wall_batch, [wall] * n, items, [it.dst_rect for it in items], False, n * 480 * 270 * 3 // 2)
    # (b) previews
    previews = [nv12_surface(360, 640, 640, gen) for _ in range(n)]
    prev_batch = FrameBatch(n, DEV, format="nv12").set(previews)
    measure("previews", prev_batch, previews, [(i, i, (0, 0, 640, 360)) for i in range(n)], [(0, 0, 640, 360)] * n, False, n * 640 * 360 * 3 // 2)
    # (c) NV12 -> RGB24
    rgbs = [torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV) for _ in range(n)]
    rgb_batch = FrameBatch(n, DEV, format="rgb24").set(rgbs)
    measure("rgb", rgb_batch, rgbs, [(i, i, (0, 0, W, H)) for i in range(n)], [(0, 0, W, H)] * n, True, n * H * W * 3)

    motion = os.path.join(ROOT, "profiles", "motion_timing.json")
    if os.path.exists(motion):
        rate = json.load(open(motion)).get("luma_bytes_per_second_lower_bound")
        if rate:
            result["yardstick"] = dict(source="profiles/motion_timing.json: luma_bytes_per_second_lower_bound", bytes_per_second=rate,
                                       wall_read_rate_over_yardstick=round(result["workloads"]["wall"]["read_bytes_per_second"] / rate, 3))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
