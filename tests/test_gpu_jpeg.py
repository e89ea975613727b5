"""Baseline JPEG encoding on the device (dn_jpeg_encode, dn_jpeg_items_from_index, jpeg.JpegEncoder, SSD.track_frames(..., jpeg=))
against tests/jpeg_ref.py, BYTE FOR BYTE: every file, every result row, the totals, and the whole arena -- it is pre-filled with 0xA5, and the bytes
of the alignment gaps and everything beyond bytes_used must still be 0xA5 afterwards. tests/test_jpeg.py shows that the scenes used here tell eight
wrong encoders from the right one and that an independent decoder opens the reference's files."""
import ctypes as C

import numpy as np
import pytest
import torch

import compose_ref as cr
import crops_ref
import jpeg_ref as ref
import regions_ref as rr
import test_gpu_regions as tgr
from demonet_amd import _lib, compose, jpeg, models, osd
from demonet_amd.crops import ObjectCropper
from demonet_amd.frames import FrameBatch
from demonet_amd.track import ByteTracker

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GAP = 0xA5
FULL601, LIMITED709 = ("bt601", True), ("bt709", False)
_WANT = {}


# ---------------------------------------------------------------------------------------------------------------- helpers
def _batch(fmt, space, planes, pitch="w+1"):
    surfaces = [tgr._surface(fmt, p, pitch, GAP) for p in planes]
    return FrameBatch(len(planes), DEV, format=fmt, matrix=space[0], full_range=space[1]).set(surfaces)


def _noise(fmt, seed=940):
    return [cr.noise_planes(fmt, seed + i, h, w) for i, (h, w) in enumerate(rr.SIZES)]


def _want(key, fmt, space, planes, item):
    """the reference's file of item (frame, rect, quality) of the frames `planes`, computed once per key"""
    f, rect, q = item
    k = (key, fmt, space, f, rect, q)
    if k not in _WANT:
        _WANT[k] = ref.encode_item(fmt, space[0], space[1], planes[f], rect, q)[0]
    return _WANT[k]


def _encoder(items, arena_bytes=1 << 20, **kw):
    enc = jpeg.JpegEncoder(items, DEV, arena_bytes, **kw)
    enc._allocate()
    enc.arena.fill_(GAP)
    return enc


def _check(enc, files, what, statuses=None):
    """results, totals, files() and EVERY byte of the arena against the reference's placement of `files` (None: a slot without a file, its status
    in `statuses`)"""
    torch.cuda.synchronize()
    lengths = [len(f) if f is not None else -(statuses[i] if statuses else ref.EMPTY) for i, f in enumerate(files)]
    lengths += [-ref.EMPTY] * (enc.capacity - len(files))
    res, totals = ref.place(lengths, enc.arena_bytes)
    got_res, got_totals = enc.results.cpu().numpy(), enc.totals.cpu().numpy()
    assert np.array_equal(got_res, res), "{}: results\n{}\nwant\n{}".format(what, got_res[:len(files) + 1], res[:len(files) + 1])
    assert np.array_equal(got_totals, totals), "{}: totals {} want {}".format(what, got_totals, totals)
    padded = list(files) + [None] * (enc.capacity - len(files))
    want = ref.arena_after(np.full(enc.arena_bytes, GAP, np.uint8), [f or b"" for f in padded], res)
    got = enc.arena.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "{}: {} arena bytes differ, first at {} (got {:02x}, want {:02x}); results {}".format(
        what, bad.size, bad[0], got[bad[0]], want[bad[0]], res[:len(files)].tolist())
    out = enc.files()
    assert out == [f if st == ref.OK else None for f, st in zip(padded, res[:, 2])], what
    return res, totals


MIXED = [(0, None, 85), (1, None, 50), (1, (0, 0, 1, 1), 5), (1, (4, 2, 16, 16), 100), (1, (20, 30, 17, 15), 85), (1, (64, 48, 33, 47), 50), (0, (100, 60, 160, 140), 30)]
SECOND = [(1, (2, 4, 77, 59), 85), (0, None, 5), (0, (60, 20, 150, 90), 100)]


def _norm(items):
    return [(f, (0, 0, rr.SIZES[f][1], rr.SIZES[f][0]) if r is None else r, q) for f, r, q in items]


def _run(fmt, space, items, pitch="w+1", seed=940, capacity=16, what=""):
    planes = _noise(fmt, seed)
    batch = _batch(fmt, space, planes, pitch)
    enc = _encoder(capacity).set(items, batch)
    assert enc.items == _norm(items)
    arena, results, totals = enc.encode(batch)
    assert arena is enc.arena and results is enc.results and totals is enc.totals
    files = [_want(seed, fmt, space, planes, it) for it in _norm(items)]
    _check(enc, files, what or "{} {}".format(fmt, space))
    return files


# ---------------------------------------------------------------------------------------------------------------- 1. formats and colour spaces
@pytest.mark.parametrize("space", [FULL601, LIMITED709], ids=["bt601-full", "bt709-limited"])
@pytest.mark.parametrize("fmt", ["nv12", "i420", "rgb24", "bgr24"])
def test_every_format_and_both_paths_on_the_mixed_scene(fmt, space):
    first = _run(fmt, space, MIXED)
    planes = fmt in ref.YUV and space == FULL601
    assert ref.planewise(fmt, *space) == planes
    assert _lib.debug_last_kernel() == ("jpeg_planes_kernel" if planes else "jpeg_rgb_kernel") + "<{}>".format(_lib.DN_FRAME[fmt])
    again = _run(fmt, space, MIXED, pitch="256")
    assert first == again                       # other pitches (and other alignments of every row piece): the same files
    assert first == _run(fmt, space, MIXED, pitch="w")


# ---------------------------------------------------------------------------------------------------------------- 2. the scenes of the coder
@pytest.mark.parametrize("q", ref.QUALITIES)
def test_edge_restart_wide_row_checkerboard_and_flat_scenes(q):
    """the plane-wise scenes of tests/test_jpeg.py at one quality in ONE call: 1 x 1, 16 x 16, 17 x 15 and 33 x 47 rectangles (every partial MCU),
    13 MCU rows (RSTm wraps), 66 MCUs in a row (the bit remainder is carried over six groups of ten), category 11 / 10 values, all-EOB blocks"""
    scenes = ref.plane_scenes()
    names = ["noise0", "noise1", "gradient", "flat", "checkerboard"]
    planes = [scenes[n][1] for n in names]
    items = [(i, scenes[n][2], q) for i, n in enumerate(names)] + [(1, r, q) for r in ref.RECTS]
    for fmt in ("nv12", "i420"):
        mine = planes if fmt == "nv12" else [[p[0], p[1][:, 0::2], p[1][:, 1::2]] for p in planes]
        batch = _batch(fmt, FULL601, mine, "w+1")
        enc = _encoder(16, arena_bytes=1 << 19).set(items, batch)
        enc.encode(batch)
        files = [_want("scenes", "nv12", FULL601, planes, it) for it in items]
        _check(enc, files, "scenes at quality {} ({})".format(q, fmt))


def test_two_runs_give_the_same_bytes_and_items_carry_their_own_quality():
    planes = _noise("nv12")
    batch = _batch("nv12", LIMITED709, planes)
    items = [jpeg.Item(0, None, 10), jpeg.Item(0), jpeg.Item(0, quality=95)]
    enc = _encoder(4, quality=60).set(items, batch)
    enc.encode(batch)
    torch.cuda.synchronize()
    first = enc.arena.clone()
    enc.arena.fill_(GAP)
    enc.encode(batch)
    files = [_want(940, "nv12", LIMITED709, planes, (0, (0, 0, 260, 200), q)) for q in (10, 60, 95)]
    _check(enc, files, "second run")
    assert torch.equal(first, enc.arena) and len({len(f) for f in files}) == 3


# ---------------------------------------------------------------------------------------------------------------- 4. no space
def test_an_arena_one_byte_short_of_the_second_item():
    planes = _noise("i420")
    items = _norm([(1, (4, 2, 16, 16), 85), (1, None, 85), (1, (20, 30, 17, 15), 50)])
    files = [_want(940, "i420", FULL601, planes, it) for it in items]
    short = ref.align16(len(files[0])) + len(files[1]) - 1
    batch = _batch("i420", FULL601, planes)
    enc = _encoder(3, arena_bytes=short).set(items, batch)
    enc.encode(batch)
    res, totals = _check(enc, files, "one byte short")
    assert res[:, 2].tolist() == [0, 3, 3] and res[1].tolist() == [ref.align16(len(files[0])), 0, 3, 0] and totals.tolist() == [1, 2, len(files[0]), 0]
    # an arena that ends inside the gap behind the second: the third, judged by the rule, does not fit, the first two are written
    enc = _encoder(3, arena_bytes=short + 2).set(items, batch)
    enc.encode(batch)
    res, totals = _check(enc, files, "room for two")
    assert res[:, 2].tolist() == [0, 0, 3] and totals[0] == 2
    # ... and with the second item small, the third fits behind it
    items = [items[0], items[2], items[1]]
    files = [files[0], files[2], files[1]]
    enc = _encoder(3, arena_bytes=ref.align16(len(files[0])) + ref.align16(len(files[1])) + len(files[2])).set(items, batch)
    enc.encode(batch)
    res, totals = _check(enc, files, "exactly enough")
    assert res[:, 2].tolist() == [0, 0, 0] and totals[2] == enc.arena_bytes


# ---------------------------------------------------------------------------------------------------------------- 5. the device-built table
INDEX = [[0, 3, 11, 21, 30, 40, 0, 0], [-1, 0, 0, 0, 0, 0, 0, 0], [2, 0, 0, 0, 8, 8, 0, 0], [1, 1, 100, 90, 40, 8, 0, 0], [1, 2, 0, 0, 16, 16, 0, 0],
         [-7, 0, 0, 0, 8, 8, 0, 0], [1, 0, 3, 2, 0, 5, 0, 0], [1, 5, 129, 95, 2, 2, 0, 0], [1, 4, 130, 0, 2, 2, 0, 0], [0, 9, 0, 0, 260, 200, 0, 0],
         [1, 7, 8, 8, 16, 17, 0, 0]]
SELECT = [1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1]


@pytest.mark.parametrize("fmt,space", [("nv12", FULL601), ("nv12", LIMITED709), ("bgr24", FULL601)], ids=["planes", "yuv-rgb", "bgr"])
def test_encode_objects_from_a_hand_written_index(fmt, space):
    """odd origins, a row with stream -1, streams out of range, rectangles past the frame, an empty side, a deselected row, and a last row whose
    two MCU rows push the total past max_segments"""
    planes = _noise(fmt)
    batch = _batch(fmt, space, planes)
    yuv = fmt in ref.YUV
    everything = ref.items_from_index(INDEX, rr.SIZES, yuv, SELECT, 1 << 20)
    rows = sum((it[4] + 15) // 16 for st, it in everything if st == ref.OK)
    want = ref.items_from_index(INDEX, rr.SIZES, yuv, SELECT, rows - 1)
    assert [st for st, _ in want] == [0, 1, 2, 2, 1, 2, 2, 0, 2, 0, 3] and want[0][1] == ((0, 10, 20, 31, 41) if yuv else (0, 11, 21, 30, 40))
    enc = _encoder(16, max_segments=rows - 1)
    index = torch.tensor(INDEX, dtype=torch.int32, device=DEV)
    enc.encode_objects(batch, index, select=torch.tensor(SELECT, dtype=torch.bool, device=DEV), quality=70)
    assert _lib.debug_last_kernel().startswith("jpeg_")
    files = [_want(940, fmt, space, planes, (it[0], it[1:], 70)) if st == ref.OK else None for st, it in want]
    _check(enc, files, "hand-written index", [st for st, _ in want])
    # no select, room for every row, the encoder's own quality
    enc = _encoder(16, quality=40)
    enc.encode_objects(batch, index)
    files = [_want(940, fmt, space, planes, (it[0], it[1:], 40)) if st == ref.OK else None for st, it in ref.items_from_index(INDEX, rr.SIZES, yuv, None, 1 << 20)]
    _check(enc, files, "no select", [st for st, _ in ref.items_from_index(INDEX, rr.SIZES, yuv, None, 1 << 20)])
    with pytest.raises(ValueError, match="index rows"):
        _encoder(4).encode_objects(batch, index)
    with pytest.raises(ValueError, match="select must be"):
        enc.encode_objects(batch, index, select=torch.ones(3, dtype=torch.bool, device=DEV))


def test_encode_objects_behind_a_cropper_step():
    planes = _noise("nv12", 930)
    batch = _batch("nv12", LIMITED709, planes, "256")
    boxes, counts = crops_ref.boxes_array()
    cropper = ObjectCropper(2, DEV, size=(16, 8), capacity=64, dtype=torch.float16)
    _, index, totals = cropper(batch, torch.from_numpy(boxes).to(DEV), torch.from_numpy(counts).to(DEV))
    enc = _encoder(64, arena_bytes=1 << 20, max_segments=1024)
    enc.encode_objects(batch, cropper, quality=80)
    torch.cuda.synchronize()
    rows = index.cpu().numpy()
    kept = int(totals.cpu()[0])
    assert kept >= 8 and (rows[kept:, 0] == -1).all()
    want = ref.items_from_index(rows, rr.SIZES, True, None, 1024)
    assert [st for st, _ in want] == [0] * kept + [1] * (64 - kept)
    files = [_want(930, "nv12", LIMITED709, planes, (it[0], it[1:], 80)) if st == ref.OK else None for st, it in want]
    _check(enc, files, "behind the cropper", [st for st, _ in want])


# ---------------------------------------------------------------------------------------------------------------- 6. a captured call
def test_a_captured_call_follows_surfaces_items_and_the_item_count():
    fmt, space = "nv12", FULL601
    planes = [_noise(fmt, 940), _noise(fmt, 960)]
    batch = _batch(fmt, space, planes[0])
    enc = _encoder(8).set(MIXED, batch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enc.encode(batch)                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enc.encode(batch)
    tables = (batch.table.data_ptr(), enc.table.data_ptr(), enc.arena.data_ptr())
    for which, items in ((0, MIXED), (1, MIXED), (1, SECOND), (1, SECOND[:1]), (1, [])):
        batch.set([tgr._surface(fmt, p, "w+1", GAP) for p in planes[which]])          # other surfaces ...
        enc.set(items, batch)                                                        # ... other items, another count
        assert (batch.table.data_ptr(), enc.table.data_ptr(), enc.arena.data_ptr()) == tables
        enc.arena.fill_(GAP)
        graph.replay()
        files = [_want(940 + 20 * which, fmt, space, planes[which], it) for it in _norm(items)]
        _check(enc, files, "replay on {} items of surfaces {}".format(len(items), which))


# ---------------------------------------------------------------------------------------------------------------- 7. behind the tracker
def test_the_encoder_behind_paint_and_composition_of_a_tracking_step():
    m = models.load_synthetic(models.ssd_lite_mobilenet_v2(image_size=160, num_classes=3), 0).to(DEV)
    try:
        fmt = "nv12"
        sp = [tgr._source(fmt, "bt709", False, 930 + i, h, w)[0] for i, (h, w) in enumerate(rr.SIZES)]
        dp = [cr.noise_planes("i420", 950 + i, h, w) for i, (h, w) in enumerate(cr.DST_SIZES)]
        kw = dict(max_tracks=64, track_thresh=0.05, low_thresh=0.01, new_thresh=0.05)
        ov = osd.Overlay(2, DEV, names=["background", "thing", "other"], scale=1)
        items = cr.api_items(cr.mixed_items(rr.SIZES))
        trackers = [ByteTracker(2, DEV, **kw) for _ in range(3)]

        def fresh():
            ssurf = [tgr._surface(fmt, p, "256", GAP) for p in sp]
            dsurf = [tgr._surface("i420", p, "w+1", GAP) for p in dp]
            sb = FrameBatch(2, DEV, format=fmt).set(ssurf)
            db = FrameBatch(2, DEV, format="i420", matrix="bt601", full_range=True).set(dsurf)
            return sb, db, ssurf, dsurf
        a_sb, a_db, _, a_ds = fresh()
        b_sb, b_db, _, b_ds = fresh()
        c_sb, _, c_ss, _ = fresh()
        comp_a = compose.Compositor(16, DEV).set(items, a_sb, a_db)
        comp_b = compose.Compositor(16, DEV).set(items, b_sb, b_db)
        walls = [(0, None, 85), (1, (10, 2, 40, 33), 60)]
        wall_sizes = cr.DST_SIZES
        enc = _encoder(4).set(walls, a_db)
        on_batch = _encoder(4).set([(1, None, 50)], c_sb)
        outs_a = [t.clone() for t in m.track_frames(a_sb, trackers[0], osd=ov, compose=comp_a, wall=a_db, jpeg=enc)[:6]]
        outs_b = [t.clone() for t in m.track_frames(b_sb, trackers[1], osd=ov, compose=comp_b, wall=b_db, jpeg=None)[:6]]      # None: today's call
        outs_c = [t.clone() for t in m.track_frames(c_sb, trackers[2], jpeg=on_batch)[:6]]                                      # no wall: the batch
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(outs_a, outs_b)) and all(torch.equal(x, y) for x, y in zip(outs_a, outs_c))
        wall_a = [[v.cpu().numpy() for v in s] for s in a_ds]
        wall_b = [[v.cpu().numpy() for v in s] for s in b_ds]
        assert all(np.array_equal(x, y) for s, t in zip(wall_a, wall_b) for x, y in zip(s, t))            # the wall is what the step without jpeg= leaves
        assert any(not np.array_equal(x, y) for s, t in zip(wall_a, dp) for x, y in zip(s, t))
        norm = [(f, (0, 0, wall_sizes[f][1], wall_sizes[f][0]) if r is None else r, q) for f, r, q in walls]
        _check(enc, [ref.encode_item("i420", "bt601", True, wall_a[f], r, q)[0] for f, r, q in norm], "the wall as it stands after the step")
        frame = [v.cpu().numpy() for v in c_ss[1]]
        _check(on_batch, [ref.encode_item(fmt, "bt709", False, frame, (0, 0, rr.SIZES[1][1], rr.SIZES[1][0]), 50)[0]], "the batch, no wall")
        with pytest.raises(ValueError, match="stale sizes"):
            m.track_frames(a_sb, trackers[0], jpeg=enc)              # set() for the wall, used without one
        with pytest.raises(ValueError, match="expected a JpegEncoder"):
            m.track_frames(a_sb, trackers[0], jpeg=ov)
    finally:
        m.release()


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_every_error_code_of_the_entry_points():
    DN_E_INVALID, DN_E_UNSUPPORTED = -1, -4
    planes = _noise("nv12")
    batch = _batch("nv12", FULL601, planes)
    enc = _encoder(8).set(MIXED, batch)
    torch.cuda.synchronize()
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda v: C.c_void_p(v) if v else None      # noqa: E731
    table0 = enc.table.clone()

    def call(**kw):
        a = dict(frames=batch.table.data_ptr(), fmt=0, color=0x10, table=enc.table.data_ptr(), capacity=8, arena=enc.arena.data_ptr(), arena_bytes=enc.arena_bytes,
                 results=enc.results.data_ptr(), totals=enc.totals.data_ptr(), ws=enc.workspace.data_ptr(), ws_bytes=enc.workspace.numel())
        a.update(kw)
        return L.dn_jpeg_encode(p(a["frames"]), a["fmt"], a["color"], p(a["table"]), a["capacity"], p(a["arena"]), a["arena_bytes"], p(a["results"]),
                                p(a["totals"]), p(a["ws"]), a["ws_bytes"], stream)
    for kw in (dict(frames=0), dict(table=0), dict(arena=0), dict(results=0), dict(totals=0), dict(ws=0), dict(frames=batch.table.data_ptr() + 4),
               dict(table=enc.table.data_ptr() + 8), dict(results=enc.results.data_ptr() + 4), dict(totals=enc.totals.data_ptr() + 8),
               dict(ws=enc.workspace.data_ptr() + 4), dict(capacity=0), dict(capacity=-2), dict(arena_bytes=-1), dict(fmt=4), dict(fmt=-1), dict(color=2),
               dict(color=0x20), dict(color=0x13), dict(ws_bytes=0), dict(ws_bytes=int(L.dn_jpeg_workspace_bytes(8, 1)) - 1)):
        assert call(**kw) == DN_E_INVALID, kw
        assert L.dn_last_error()
    assert call(capacity=8193) == DN_E_UNSUPPORTED
    assert L.dn_jpeg_workspace_bytes(8193, 10) == 0 and L.dn_jpeg_workspace_bytes(0, 10) == 0 and L.dn_jpeg_workspace_bytes(8, 0) == 0
    assert L.dn_jpeg_workspace_bytes(8, 100) >= 8 * 8 + 100 * 4
    index = torch.tensor(INDEX, dtype=torch.int32, device=DEV)

    def from_index(**kw):
        a = dict(frames=batch.table.data_ptr(), n=2, fmt=0, index=index.data_ptr(), rows=len(INDEX), select=0, q=85, segs=100, table=enc.table.data_ptr())
        a.update(kw)
        return L.dn_jpeg_items_from_index(p(a["frames"]), a["n"], a["fmt"], p(a["index"]), a["rows"], p(a["select"]), a["q"], a["segs"], p(a["table"]), stream)
    for kw in (dict(frames=0), dict(index=0), dict(table=0), dict(frames=batch.table.data_ptr() + 4), dict(index=index.data_ptr() + 4), dict(table=enc.table.data_ptr() + 4),
               dict(n=0), dict(rows=0), dict(segs=0), dict(q=0), dict(q=101), dict(fmt=9)):
        assert from_index(**kw) == DN_E_INVALID, kw
    assert from_index(rows=8193) == DN_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert (enc.arena == GAP).all() and torch.equal(enc.table, table0) and enc.results[:, 2].eq(1).all()        # nothing was enqueued
    assert call() == 0
    _check(enc, [_want(940, "nv12", FULL601, planes, it) for it in _norm(MIXED)], "the call itself")
