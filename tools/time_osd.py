"""dev tool: what painting the tracker's outputs into 64 full-HD NV12 surfaces costs through osd.Overlay, and what a user composes without it.
    python tools/time_osd.py [--out profiles/osd_timing.json] [--rounds 5] [--streams 64] [--reps 100] [--today-reps 1]
64 surfaces of 1080 x 1920, each an allocation of its own with a row pitch of 2048 bytes, BT.709 limited range, noise content; 100 tracks per
stream at person-like sizes (40 .. 160 pixels wide, 2 .. 3 times as high, centres anywhere in the frame) in 128 rows, 8 classes, ids and scores.
Two runs: "outline" (thickness 2, a class / id / score label per row) and "redact" (the rows of 2 classes of 8 -- a fifth to a quarter of the rows --
pixelated with block 16 instead). Both sides run in this process on the same device and are timed alternately, round by round, with device events
around back-to-back calls after a warm-up; medians over the rounds with min and max:
  paint_us        one Overlay.paint (two launches), `reps` calls back to back
  paint_graph_us  the same call captured once in a graph, `reps` replays
  today_ms        the composition without the feature, per step: every surface converted to RGB in torch ops (tools/time_frames.py), boxes, labels
                  and counts copied to the host, and per box on the device four slice assignments for the outline and one for the label's
                  background (the text itself is NOT drawn: it has no torch counterpart), or avg_pool2d + repeat_interleave for a pixelated box.
                  The painted RGB frames are not converted back to NV12 either, which a consumer of surfaces would still have to do
Before any time is taken the painted surface of stream 0 is compared bit for bit with tests/osd_ref.py. bytes: every plane byte of the tiles touched
is read once and written once (32 x 32 luma + 16 x 32 chroma bytes per full tile). One JSON document on stdout (and in --out)."""
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
import osd_ref as ref  # noqa: E402
from demonet_amd import osd, osd_font  # noqa: E402
from demonet_amd.frames import FrameBatch  # noqa: E402
from time_frames import torch_nv12_to_rgb  # noqa: E402

H, W, PITCH = 1080, 1920, 2048
MATRIX, FULL = "bt709", False
D, PER_STREAM, CLASSES = 128, 100, 8
NAMES = ["person", "bicycle", "car", "bus", "truck", "dog", "face", "plate"]


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
    w = rng.uniform(40, 160, (streams, D))
    h = w * rng.uniform(2, 3, (streams, D))
    cx, cy = rng.uniform(0, W, (streams, D)), rng.uniform(0, H, (streams, D))
    boxes = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1).astype(np.float32)
    scores = rng.uniform(0.3, 1.0, (streams, D)).astype(np.float32)
    labels = rng.integers(0, CLASSES, (streams, D)).astype(np.int64)
    ids = rng.integers(1, 100000, (streams, D)).astype(np.int64)
    return boxes, scores, labels, ids, np.full((streams,), PER_STREAM, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--today-reps", type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    n = a.streams
    rng = np.random.default_rng(0)
    pristine = [(torch.from_numpy(rng.integers(0, 256, (H, PITCH), dtype=np.uint8)).cuda(),
                 torch.from_numpy(rng.integers(0, 256, (H // 2, PITCH), dtype=np.uint8)).cuda()) for _ in range(n)]
    buffers = [(y.clone(), c.clone()) for y, c in pristine]
    surfaces = [(y[:, :W], c[:, :W]) for y, c in buffers]
    batch = FrameBatch(n, "cuda", "nv12", MATRIX, FULL).set(surfaces)
    boxes_np, scores_np, labels_np, ids_np, counts_np = scene(n)
    boxes, scores, labels, ids, counts = (torch.from_numpy(x).cuda() for x in (boxes_np, scores_np, labels_np, ids_np, counts_np))
    redacted = (6, 7)
    tile_bytes = 0
    doc = dict(streams=n, surface=[H, W], pitch=PITCH, format="nv12", matrix=MATRIX, full_range=FULL, rows=D, tracks_per_stream=PER_STREAM,
               classes=CLASSES, rounds=a.rounds, reps=a.reps, today_reps=a.today_reps, device=torch.cuda.get_device_name(0), runs={})

    for run in ("outline", "redact"):
        ov = osd.Overlay(n, "cuda", names=NAMES, scale=1, thickness=2)
        if run == "redact":
            ov.redact(redacted, block=16)
        styles = [(s.thickness, s.fill_alpha, s.pixelate, s.flags) for s in ov.styles]

        def restore():
            for (y, c), (py, pc) in zip(buffers, pristine):
                y.copy_(py)
                c.copy_(pc)

        def paint():
            return ov.paint(batch, boxes, scores, labels, counts, ids=ids)

        def today():
            frames = [torch_nv12_to_rgb(y, uv) for y, uv in surfaces]
            hb, hl, hc = boxes.cpu().numpy(), labels.cpu().numpy(), counts.cpu().numpy()      # the host round trip of every step
            colour = torch.tensor([230, 25, 75], dtype=torch.uint8, device="cuda")
            for b in range(n):
                f = frames[b]
                for j in range(int(hc[b])):
                    x0, y0 = int(max(np.floor(hb[b, j, 0]), 0)), int(max(np.floor(hb[b, j, 1]), 0))
                    x1, y1 = int(min(np.ceil(hb[b, j, 2]), W)), int(min(np.ceil(hb[b, j, 3]), H))
                    if x0 >= x1 or y0 >= y1:
                        continue
                    if run == "redact" and int(hl[b, j]) in redacted:
                        xa, ya = x0 // 16 * 16, y0 // 16 * 16
                        xb, yb = min(-(-x1 // 16) * 16, W // 16 * 16), min(-(-y1 // 16) * 16, H // 16 * 16)
                        if xa < xb and ya < yb:
                            blk = f[ya:yb, xa:xb].permute(2, 0, 1).unsqueeze(0).float()
                            m = Fn.avg_pool2d(blk, 16).repeat_interleave(16, 2).repeat_interleave(16, 3)[0].permute(1, 2, 0)
                            f[ya:yb, xa:xb] = m.round().to(torch.uint8)
                        continue
                    f[y0:y0 + 2, x0:x1] = colour
                    f[max(y1 - 2, y0):y1, x0:x1] = colour
                    f[y0:y1, x0:x0 + 2] = colour
                    f[y0:y1, max(x1 - 2, x0):x1] = colour
                    f[max(y0 - 8, 0):y0, x0:min(x0 + 8 * 16, W)] = colour
            return frames

        # agreement first: stream 0 against the numpy statement
        restore()
        stats = paint().clone()
        torch.cuda.synchronize()
        hs = stats.cpu().numpy()
        got = [surfaces[0][0].cpu().numpy(), surfaces[0][1].cpu().numpy()]
        chans, subs = ref.split("nv12", [pristine[0][0][:, :W].cpu().numpy(), pristine[0][1][:, :W].cpu().numpy()])
        rows = dict(boxes=boxes_np[0], scores=scores_np[0], labels=labels_np[0], ids=ids_np[0], count=int(counts_np[0]))
        pal = ref.palette_records(osd.PALETTE, "nv12", MATRIX, FULL)
        params = dict(colour_by_id=1, scale=1, label_alpha=255, line_thickness=2, zone_thickness=2, zone_alpha=255, line_colour=(0, 0, 0), zone_colour=(0, 0, 0))
        want, counted = ref.paint(chans, subs, rows, styles, None, CLASSES, ref.name_records(NAMES), pal, osd_font.table(), None, params)
        equal = all(np.array_equal(g, w) for g, w in zip(got, ref.join("nv12", want))) and tuple(hs[0, :2]) == counted

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            paint()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            paint()
        for _ in range(10):      # every shape of the timed windows
            paint()
            graph.replay()
        today()
        torch.cuda.synchronize()
        times = dict(paint_us=[], paint_graph_us=[], today_ms=[])
        for _ in range(a.rounds):
            times["paint_us"].append(_events(paint, a.reps) * 1e3)
            times["today_ms"].append(_events(today, a.today_reps))
            times["paint_graph_us"].append(_events(graph.replay, a.reps) * 1e3)
        tiles = int(hs[:, 2].sum())
        # (a frame of 1080 rows has a ragged last tile row of 24 luma rows; the average tile is the frame over its tiles)
        tile_bytes = H * W * 3 // 2 / (((H + 31) // 32) * ((W + 31) // 32))
        med = {k: round(statistics.median(v), 3) for k, v in times.items()}
        sec = med["paint_graph_us"] * 1e-6
        moved = tiles * tile_bytes
        doc["runs"][run] = dict(rows_painted=int(hs[:, 0].sum()), rows_skipped=int(hs[:, 1].sum()), tiles_touched=tiles, tiles_dropped=int(hs[:, 3].sum()),
                                tiles_of_all_frames=n * ((H + 31) // 32) * ((W + 31) // 32), stream_0_equals_ref=bool(equal),
                                bytes_read=int(moved), bytes_written=int(moved), read_gb_per_s=round(moved / sec / 1e9, 1),
                                written_gb_per_s=round(moved / sec / 1e9, 1), median=med, min={k: round(min(v), 3) for k, v in times.items()},
                                max={k: round(max(v), 3) for k, v in times.items()},
                                speedup_over_today=round(med["today_ms"] * 1e3 / med["paint_graph_us"], 1))
    track = os.path.join(ROOT, "profiles", "track_timing.json")
    if os.path.exists(track):
        with open(track) as f:
            t = json.load(f)["median"]
        doc["track_update_us"] = t["update_us"]
        doc["forward_ms"] = t["forward_ms"]
        for run in doc["runs"]:
            us = doc["runs"][run]["median"]["paint_graph_us"]
            doc["runs"][run]["share_of_forward_track_paint_step"] = round(us / (t["forward_ms"] * 1e3 + t["update_us"] + us), 4)
            doc["runs"][run]["times_track_update"] = round(us / t["update_us"], 2)
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
