"""Times the surface dewarping (demonet_amd/warp.py) on the MI355X against the composition available without it, and writes
profiles/warp_timing.json.

    python tools/time_warp.py [--steps 200] [--today-steps 3] [--rounds 5] [--out profiles/warp_timing.json]

Three workloads per step:
    fisheye    16 NV12 surfaces of 2880 x 2880 -> 64 NV12 views of 960 x 720, four per camera (90 degrees, tilt 50, pan 45 + 90 k)
    undistort  64 full-HD NV12 surfaces -> 64 of the same size through a Brown-Conrady mesh, 1:1
    rotate     64 full-HD RGB24 surfaces -> 64 of 1080 x 1920, turned by 90 degrees
Each is timed twice in the same process, alternating: as the library chooses (tiles whose source footprint fits are staged in LDS) and with
DN_WARP_STAGE=0 (every tile gathers). "today" is the same map made with torch on the same device: float planes, F.grid_sample with the dense grid
(built once, outside the timed loop), round, store. Times are device events around `steps` calls after a warm-up, `rounds` times: median and range.
Before a workload is timed its first output surface is compared, byte for byte, with the header's arithmetic written out in torch integers; the
result is recorded as `device_equals_exact`, and a mismatch ends the run. Bytes per step are the destination payload, the meshes and the source
bytes inside the union of the tiles' footprints (the bounding boxes of each tile's 25 control points plus the tap, clipped to the frame), computed
here from the meshes; which path each tile takes is computed from the same boxes by the kernel's rule. Yardsticks: the Compositor's wall rate
(profiles/compose_timing.json) and the luma read rate of the motion thumbnail kernel (profiles/motion_timing.json)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from demonet_amd import warp  # noqa: E402
from demonet_amd.frames import FrameBatch  # noqa: E402

DEV = "cuda:0"
ST_W = ST_H = 112            # csrc/warp.hip: WP_ST_W, WP_ST_H, WP_ST_CW, WP_ST_CH
ST_CW = ST_CH = 64


def surface(fmt, h, w, pitch, gen):
    if fmt == "nv12":
        y = torch.randint(0, 256, (h, pitch), dtype=torch.uint8, device=DEV, generator=gen)
        uv = torch.randint(0, 256, (h // 2, pitch), dtype=torch.uint8, device=DEV, generator=gen)
        return y[:, :w], uv[:, :w]
    return torch.randint(0, 256, (h, pitch), dtype=torch.uint8, device=DEV, generator=gen)[:, :3 * w].unflatten(1, (w, 3))


# ---------------------------------------------------------------------------------------------------------------- the header in torch integers
def positions(mesh, chroma):
    """q [h, w, 2] int64 on the device, in 1/32 sample, of the luma pixels or the chroma samples of the mesh's rectangle"""
    dh, dw = mesh.size
    m = torch.from_numpy(mesh.points.astype(np.int64)).to(DEV)
    if chroma:
        x, y = 2 * torch.arange((dw + 1) // 2, device=DEV), 2 * torch.arange((dh + 1) // 2, device=DEV)
        i, j, n = (2 * (x & 7) + 1)[None, :, None], (2 * (y & 7) + 1)[:, None, None], 16
    else:
        x, y = torch.arange(dw, device=DEV), torch.arange(dh, device=DEV)
        i, j, n = (x & 7)[None, :, None], (y & 7)[:, None, None], 8
    cx, cy = (x >> 3)[None, :], (y >> 3)[:, None]
    P = (n - j) * ((n - i) * m[cy, cx] + i * m[cy, cx + 1]) + j * ((n - i) * m[cy + 1, cx] + i * m[cy + 1, cx + 1])
    return (((P + 512) >> 10) - 8) if chroma else ((P + 64) >> 7)


def exact_plane(p, q, border):
    """[H, W] uint8 through q with a constant border byte: the header's taps and blend"""
    H, W = p.shape
    p = p.to(torch.int64)
    x0, fx, y0, fy = q[..., 0] >> 5, q[..., 0] & 31, q[..., 1] >> 5, q[..., 1] & 31

    def tap(x, y):
        xc, yc = x.clamp(0, W - 1), y.clamp(0, H - 1)
        return torch.where((x == xc) & (y == yc), p[yc, xc], torch.full_like(x, border))
    out = (32 - fx) * (32 - fy) * tap(x0, y0) + fx * (32 - fy) * tap(x0 + 1, y0) + (32 - fx) * fy * tap(x0, y0 + 1) + fx * fy * tap(x0 + 1, y0 + 1)
    return ((out + 512) >> 10).to(torch.uint8)


def exact(fmt, src, dst, mesh, border):
    """whether the destination surface holds what include/demonet_hip.h defines"""
    q = positions(mesh, False)
    if fmt == "nv12":
        qc = positions(mesh, True)
        uv = src[1].unflatten(1, (-1, 2))
        want_uv = torch.stack([exact_plane(uv[..., 0], qc, border[1]), exact_plane(uv[..., 1], qc, border[2])], -1).flatten(1)
        return torch.equal(dst[0], exact_plane(src[0], q, border[0])) and torch.equal(dst[1], want_uv)
    return torch.equal(dst, torch.stack([exact_plane(src[..., c], q, border[c]) for c in range(3)], -1))


# ---------------------------------------------------------------------------------------------------------------- today
def dense_grid(mesh, src_hw, chroma):
    """[1, h, w, 2] float32 grid of F.grid_sample(align_corners=True) from the mesh's own positions"""
    q = positions(mesh, chroma).to(torch.float32) / 32.0
    H, W = src_hw
    return torch.stack([2 * q[..., 0] / max(W - 1, 1) - 1, 2 * q[..., 1] / max(H - 1, 1) - 1], -1)[None]


def today(fmt, src, dst, grids):
    """one surface through its dense grid(s): float planes, grid_sample, round, store"""
    if fmt == "nv12":
        out = F.grid_sample(src[0].float()[None, None], grids[0], mode="bilinear", padding_mode="zeros", align_corners=True)
        dst[0].copy_((out[0, 0] + 0.5).clamp_(0, 255).to(torch.uint8))
        c = src[1].unflatten(1, (-1, 2)).permute(2, 0, 1).float()[None]
        out = F.grid_sample(c, grids[1], mode="bilinear", padding_mode="zeros", align_corners=True)
        dst[1].copy_((out[0] + 0.5).clamp_(0, 255).to(torch.uint8).permute(1, 2, 0).flatten(1))
    else:
        out = F.grid_sample(src.permute(2, 0, 1).float()[None], grids[0], mode="bilinear", padding_mode="zeros", align_corners=True)
        dst.copy_((out[0] + 0.5).clamp_(0, 255).to(torch.uint8).permute(1, 2, 0))


# ---------------------------------------------------------------------------------------------------------------- footprints
def tile_boxes(mesh):
    """per 32 x 32 tile of the mesh's rectangle the range of its 25 control points: [tiles, 4] = minX, maxX, minY, maxY in 1/64 pixel"""
    dh, dw = mesh.size
    m = mesh.points.astype(np.int64)
    mh, mw = m.shape[:2]
    out = []
    for ty in range((dh + 31) // 32):
        for tx in range((dw + 31) // 32):
            ys = np.minimum(np.arange(5) + 4 * ty, mh - 1)
            xs = np.minimum(np.arange(5) + 4 * tx, mw - 1)
            p = m[ys][:, xs]
            out.append((p[..., 0].min(), p[..., 0].max(), p[..., 1].min(), p[..., 1].max()))
    return np.array(out)


def footprint(mesh, src_hw, yuv):
    """(the mask of the source samples inside the tiles' luma boxes, clipped to the frame; tiles staged; tiles) by the kernel's rule"""
    H, W = src_hw
    mask = np.zeros((H, W), bool)
    staged = 0
    boxes = tile_boxes(mesh)
    for lo_x, hi_x, lo_y, hi_y in boxes:
        x0, x1, y0, y1 = lo_x >> 6, ((hi_x + 1) >> 6) + 1, lo_y >> 6, ((hi_y + 1) >> 6) + 1
        mask[max(y0, 0):max(min(y1, H - 1) + 1, 0), max(x0, 0):max(min(x1, W - 1) + 1, 0)] = True
        ok = x0 >= 0 and y0 >= 0 and x1 < W and y1 < H and x1 - x0 + 1 <= ST_W and y1 - y0 + 1 <= ST_H
        if yuv:
            c0, c1, r0, r1 = (lo_x - 33) >> 7, ((hi_x - 30) >> 7) + 1, (lo_y - 33) >> 7, ((hi_y - 30) >> 7) + 1
            ok = ok and c0 >= 0 and r0 >= 0 and c1 < (W + 1) // 2 and r1 < (H + 1) // 2 and c1 - c0 + 1 <= ST_CW and r1 - r0 + 1 <= ST_CH
        staged += int(ok)
    return mask, staged, len(boxes)


def timed_pair(fns, steps, rounds):
    """alternating rounds of the functions: [dict(median_us, min_us, max_us)] per function"""
    for fn in fns:
        fn()
        fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) * 1000.0 / steps)
    return [dict(median_us=round(statistics.median(o), 3), min_us=round(min(o), 3), max_us=round(max(o), 3)) for o in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--today-steps", type=int, default=3)
    ap.add_argument("--cameras", type=int, default=16)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_warp.py measures on the GPU; there is none here")
    gen = torch.Generator(device=DEV).manual_seed(7)
    result = dict(steps=args.steps, rounds=args.rounds, today_steps=args.today_steps, device=torch.cuda.get_device_name(0), workloads={})
    yard = {}
    for name, path, pick in (("compose_wall", "compose_timing.json", lambda j: j["workloads"]["wall"]["bytes_per_second"]),
                             ("motion_luma_read", "motion_timing.json", lambda j: j["luma_bytes_per_second_lower_bound"])):
        p = os.path.join(ROOT, "profiles", path)
        if os.path.exists(p):
            yard[name] = dict(source="profiles/" + path, bytes_per_second=pick(json.load(open(p))))
    result["yardsticks"] = yard

    def measure(name, fmt, src_hw, src_pitch, n_src, meshes, pairs, border):
        """pairs: (source, destination) per item, item k through meshes[k % len(meshes)]"""
        bpp = 1.5 if fmt == "nv12" else 3.0
        sources = [surface(fmt, src_hw[0], src_hw[1], src_pitch, gen) for _ in range(n_src)]
        dh, dw = meshes[0].size
        dests = [surface(fmt, dh, dw, (dw if fmt == "nv12" else 3 * dw), gen) for _ in pairs]
        sb = FrameBatch(n_src, DEV, format=fmt).set(sources)
        db = FrameBatch(len(pairs), DEV, format=fmt).set(dests)
        items = [warp.Item(s, d, meshes[k % len(meshes)], (0, 0), border) for k, (s, d) in enumerate(pairs)]
        w = warp.Warper(len(pairs), DEV).set(items, sb, db)
        os.environ["DN_WARP_STAGE"] = "1"
        w(sb, db)
        torch.cuda.synchronize()
        from demonet_amd.osd import to_surface
        b = to_surface(border, fmt, "bt709", False)
        if not exact(fmt, sources[pairs[0][0]], dests[0], meshes[0], b):
            raise SystemExit("time_warp.py: the first output of '{}' differs from the header's arithmetic; nothing was timed".format(name))
        first = [t.clone() for t in (dests[0] if fmt == "nv12" else (dests[0],))]
        os.environ["DN_WARP_STAGE"] = "0"
        w(sb, db)
        torch.cuda.synchronize()
        same = all(torch.equal(a, c) for a, c in zip(first, dests[0] if fmt == "nv12" else (dests[0],)))
        if not same:
            raise SystemExit("time_warp.py: the gather path of '{}' differs from the staged path; nothing was timed".format(name))

        def run(stage):
            def fn():
                os.environ["DN_WARP_STAGE"] = stage
                w(sb, db)
            return fn
        ours, gather = timed_pair([run("1"), run("0")], args.steps, args.rounds)
        os.environ["DN_WARP_STAGE"] = "1"
        grids = [(dense_grid(m, src_hw, False), dense_grid(m, ((src_hw[0] + 1) // 2, (src_hw[1] + 1) // 2), True)) if fmt == "nv12" else (dense_grid(m, src_hw, False),)
                 for m in meshes]

        def todays():
            for k, (s, d) in enumerate(pairs):
                today(fmt, sources[s], dests[d], grids[k % len(meshes)])
        base = timed_pair([todays], args.today_steps, args.rounds)[0]
        # bytes: per source the union of the footprints of its meshes, the meshes once, the destination payload
        foot = {id(m): footprint(m, src_hw, fmt == "nv12") for m in meshes}
        per_src = {}
        for k, (s, d) in enumerate(pairs):
            per_src.setdefault(s, set()).add(id(meshes[k % len(meshes)]))
        union = {}
        for ms in per_src.values():
            key = frozenset(ms)
            if key not in union:
                union[key] = int(np.logical_or.reduce([foot[m][0] for m in key]).sum())
        src_samples = sum(union[frozenset(ms)] for ms in per_src.values())
        staged = sum(foot[id(meshes[k % len(meshes)])][1] for k in range(len(pairs)))
        tiles = sum(foot[id(meshes[k % len(meshes)])][2] for k in range(len(pairs)))
        written = int(len(pairs) * dh * dw * bpp)
        mesh_bytes = w.points * 8
        read = int(src_samples * bpp)
        moved = written + mesh_bytes + read
        rate = moved / (ours["median_us"] * 1e-6)
        result["workloads"][name] = dict(
            format=fmt, sources=n_src, source=list(src_hw), source_pitch=src_pitch, items=len(pairs), destination=[dh, dw], device_equals_exact=True,
            gather_equals_staged=True, kernel=ours, gather_only=gather, today=base, tiles=tiles, tiles_staged=staged, tiles_gathered=tiles - staged,
            bytes_written_per_step=written, mesh_bytes_per_step=mesh_bytes, source_bytes_in_footprints_per_step=read, bytes_per_second=round(rate),
            gather_over_staged=round(gather["median_us"] / ours["median_us"], 3), today_over_kernel=round(base["median_us"] / ours["median_us"], 1),
            rate_over_yardstick={k: round(rate / v["bytes_per_second"], 3) for k, v in yard.items()})
        print(name, json.dumps(result["workloads"][name]), flush=True)
        del sources, dests, sb, db, w, grids
        torch.cuda.empty_cache()

    cams, n = args.cameras, args.streams
    views = [warp.fisheye_view((2880, 2880), (720, 960), fov=90, pan=45 + 90 * k, tilt=50) for k in range(4)]
    measure("fisheye", "nv12", (2880, 2880), 3072, cams, views, [(i // 4, i) for i in range(4 * cams)], (0, 0, 0))
    K = np.array([[1100.0, 0, 959.5], [0, 1100.0, 539.5], [0, 0, 1]])
    measure("undistort", "nv12", (1080, 1920), 2048, n, [warp.undistort(K, (-0.28, 0.09, 0.0005, -0.0003, -0.01), (1080, 1920))], [(i, i) for i in range(n)], (0, 0, 0))
    measure("rotate", "rgb24", (1080, 1920), 3 * 1920, n, [warp.rotate((1080, 1920), 1)], [(i, i) for i in range(n)], (0, 0, 0))
    result["not_measured"] = ["kernel time by rocprofv3 (these are device-event times of whole calls)", "I420 and BGR24 surfaces", "replicate borders",
                              "more than one destination rectangle per surface", "the upload of a new table or mesh by set()"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
