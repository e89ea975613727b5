"""The on-screen display on the device (dn_osd_paint, osd.Overlay, SSD.track_frames(..., osd=)) against tests/osd_ref.py, bit for bit on
every plane's payload; the gap bytes of a pitched surface, filled with 0xA5, must stay. Frames are the noise surfaces of tests/regions_ref.SIZES
(200 x 260: 9 x 7 tiles; 97 x 131: odd sizes and a ragged last tile) built with the helpers of tests/test_gpu_regions.py. tests/test_osd.py shows
that the mixed scene used here tells six wrong painters from the right one."""
import ctypes as C

import numpy as np
import pytest
import torch

import frames_ref as fr
import osd_ref as ref
import regions_ref as rr
import test_gpu_regions as tgr
from demonet_amd import _lib, models, osd, osd_font
from demonet_amd.frames import FrameBatch
from demonet_amd.track import ByteTracker
from demonet_amd.zones import ZoneAnalytics

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GAP = 0xA5
FONT = osd_font.table()
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------------------- helpers
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sources(fmt, matrix, full, sizes=rr.SIZES, seeds=(930, 931, 932, 933)):
    return [tgr._source(fmt, matrix, full, seeds[i], h, w)[0] for i, (h, w) in enumerate(sizes)]


def _surfaces(fmt, srcs, pitch):
    return [tgr._surface(fmt, planes, pitch, GAP) for planes in srcs]


def _root(t):
    while t._base is not None:
        t = t._base
    return t


def _payloads(fmt, surface, planes):
    """the payload planes of a surface as numpy, after checking that its gap bytes are still GAP"""
    out = []
    for view, p in zip(surface if isinstance(surface, tuple) else (surface,), planes):
        full = _root(view).cpu().numpy()
        payload = p.shape[1]
        assert full.shape[0] == p.shape[0] and (full[:, payload:] == GAP).all(), "a gap byte changed"
        out.append(full[:, :payload])
    return out


def _cfg_record(cfg):
    rec = _lib.ZoneConfig()
    if cfg is not None:
        rec.n_lines, rec.n_zones = int(cfg["n_lines"]), int(cfg["n_zones"])
        for i in range(16):
            rec.nv[i] = int(cfg["nv"][i])
            for k in range(4):
                rec.lines[i][k] = float(cfg["lines"][i][k])
            for e in range(16):
                rec.verts[i][e][0], rec.verts[i][e][1] = float(cfg["verts"][i][e][0]), float(cfg["verts"][i][e][1])
    return rec


def _zones(cfgs):
    """a ZoneAnalytics whose device table holds these records as they are (out-of-range counts included)"""
    za = ZoneAnalytics(ByteTracker(len(cfgs), DEV, max_tracks=8))
    raw = b"".join(bytes(_cfg_record(c)) for c in cfgs)
    za.config.view(-1).copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
    return za


def _tensors(scenes, with_ids=True):
    d = max(len(r["boxes"]) for r, _ in scenes)
    B = len(scenes)
    boxes, scores = np.zeros((B, d, 4), np.float32), np.zeros((B, d), np.float32)
    labels, ids, counts = np.zeros((B, d), np.int64), np.zeros((B, d), np.int64), np.zeros(B, np.int32)
    for b, (r, _) in enumerate(scenes):
        n = len(r["boxes"])
        boxes[b, :n], scores[b, :n], labels[b, :n], counts[b] = r["boxes"], r["scores"], r["labels"], r["count"]
        if r["ids"] is not None:
            ids[b, :n] = r["ids"]
    padded = [dict(boxes=boxes[b], scores=scores[b], labels=labels[b], ids=ids[b] if with_ids else None, count=int(counts[b])) for b in range(B)]
    return padded, (_dev(boxes), _dev(scores), _dev(labels), _dev(counts), _dev(ids) if with_ids else None)


def _overlay(streams, styles, **kw):
    ov = osd.Overlay(streams, DEV, names=ref.NAMES, palette=ref.PALETTE_RGB, **kw)
    for label, (t, a, p, f) in enumerate(styles):
        ov.set_style(label, thickness=t, fill_alpha=a, pixelate=p, label=bool(f & ref.LABEL), score=bool(f & ref.SCORE), hide=bool(f & ref.HIDE))
    return ov


def _ref_params(ov, fmt, matrix, full):
    p = ov.params
    return dict(colour_by_id=p.color_by_id, scale=p.scale, label_alpha=p.label_alpha, line_thickness=p.line_thickness, zone_thickness=p.zone_thickness,
                zone_alpha=p.zone_alpha, line_colour=ref.to_surface(ov.line_colour, fmt, matrix, full),
                zone_colour=ref.to_surface(ov.zone_colour, fmt, matrix, full))


def _want(fmt, matrix, full, srcs, rows, cfgs, styles, ov):
    pal = ref.palette_records(ref.PALETTE_RGB, fmt, matrix, full)
    out = []
    for planes, r, cfg in zip(srcs, rows, cfgs):
        chans, subs = ref.split(fmt, planes)
        got, counted = ref.paint(chans, subs, r, styles, None, len(styles), ref.name_records(), pal, FONT, cfg, _ref_params(ov, fmt, matrix, full))
        out.append((ref.join(fmt, got), counted))
    return out


def _compare(fmt, surfaces, srcs, want, stats, what):
    for b, (surface, planes, (wp, counted)) in enumerate(zip(surfaces, srcs, want)):
        for i, (g, w) in enumerate(zip(_payloads(fmt, surface, planes), wp)):
            bad = np.argwhere(g != w)
            assert bad.size == 0, "{}: stream {} plane {}: {} bytes differ, first at {} (got {}, want {})".format(
                what, b, i, len(bad), tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])])
        assert tuple(stats[b, :2]) == counted, (what, b, stats[b], counted)
        assert stats[b, 3] == 0


def _run(fmt, matrix, full, scenes, styles, pitch="w+1", sizes=rr.SIZES, with_ids=True, what="", **okw):
    srcs = _sources(fmt, matrix, full, sizes)
    surfaces = _surfaces(fmt, srcs, pitch)
    batch = FrameBatch(len(sizes), DEV, format=fmt, matrix=matrix, full_range=full).set(surfaces)
    rows, tensors = _tensors(scenes, with_ids)
    cfgs = [c for _, c in scenes]
    ov = _overlay(len(sizes), styles, **okw)
    za = _zones(cfgs) if any(c is not None for c in cfgs) else None
    boxes, scores, labels, counts, ids = tensors
    stats = ov.paint(batch, boxes, scores, labels, counts, ids=ids, zones=za)
    torch.cuda.synchronize()
    stats = stats.cpu().numpy()
    want = _want(fmt, matrix, full, srcs, rows, cfgs, styles, ov)
    _compare(fmt, surfaces, srcs, want, stats, what or fmt)
    return stats, want, srcs


def _mixed():
    return [ref.mixed_scene(w, h, shift=i) for i, (h, w) in enumerate(rr.SIZES)]


# ---------------------------------------------------------------------------------------------------------------- 1. formats
@pytest.mark.parametrize("fmt,matrix,full", tgr.FORMATS, ids=tgr.IDS)
def test_format_sweep(fmt, matrix, full):
    for pitch in ("w", "256"):
        stats, want, srcs = _run(fmt, matrix, full, _mixed(), ref.MIXED_STYLES, pitch, what="{} pitch {}".format(fmt, pitch))
        assert (stats[:, 0] >= 6).all() and (stats[:, 2] >= 12).all()
        assert any(not np.array_equal(a, b) for a, b in zip(want[0][0], srcs[0]))


# ---------------------------------------------------------------------------------------------------------------- 2. geometry
EDGE_STYLES = [(1, 0, 0, 0), (2, 0, 0, 0), (3, 0, 0, 0), (5, 0, 0, 0), (16, 0, 0, 0), (2, 0, 0, ref.HIDE)]


@pytest.mark.parametrize("fmt", ["nv12", "bgr24"])
def test_geometry_edges_counts_and_labels_out_of_range(fmt):
    h, w = rr.SIZES[1]
    boxes = [(30.5, 30.5, 33.5, 33.5), (31.0, 2.0, 32.0, 40.0), (2.0, 32.0, 70.0, 33.0), (28.0, 60.0, 36.0, 68.0),       # the tile seams
             (0.0, 10.0, 9.0, 20.0), (w - 9.0, 10.0, float(w), 20.0), (50.0, 0.0, 60.0, 7.0), (50.0, h - 7.0, 60.0, float(h)),   # each edge
             (-40.0, -40.0, -1.0, -1.0), (w + 1.0, 5.0, w + 30.0, 20.0), (80.0, 40.0, 70.0, 50.0), (90.0, 50.0, 90.0, 60.0),   # outside, inverted, zero area
             (NAN, 1.0, 5.0, 5.0), (1.0, 1.0, INF, 5.0), (-INF, 1.0, 5.0, 5.0), (-1e30, -1e30, 1e30, 1e30),
             (100.0, 30.0, 126.0, 56.0), (64.2, 64.7, 96.1, 96.9), (40.0, 72.0, 44.0, 90.0), (10.0, 40.0, 20.0, 50.0), (12.0, 42.0, 30.0, 52.0)]
    labels = [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 0, 4, 3, 5, -1, 99]
    full = ref.make_rows(boxes, labels=labels, ids=list(range(len(boxes))), count=len(boxes) + 5)
    scenes = [(full, None), (dict(full, count=-3), None), (dict(full, count=0), None)]
    stats, want, srcs = _run(fmt, "bt601", True, scenes, EDGE_STYLES, "w+1", sizes=[(h, w)] * 3, what="edges " + fmt)
    assert stats[0, 0] >= 8 and stats[0, 0] + stats[0, 1] == len(boxes) and stats[0, 2] >= 8        # (_compare held both against the reference)
    assert (stats[1:] == 0).all()                    # nothing to paint: no row, no tile (and _compare saw the frames' bytes untouched)
    for b in (1, 2):
        assert all(np.array_equal(a, p) for a, p in zip(want[b][0], srcs[b]))


# ---------------------------------------------------------------------------------------------------------------- 3. order and blend
@pytest.mark.parametrize("fmt", ["i420", "rgb24"])
def test_order_and_blend(fmt):
    styles = [(0, 1, 0, 0), (0, 128, 0, 0), (0, 255, 0, 0), (0, 0, 8, 0), (2, 0, 0, ref.LABEL | ref.SCORE), (4, 200, 0, 0)]
    rows = ref.make_rows([(20.0, 20.0, 80.0, 70.0), (40.0, 30.0, 100.0, 80.0), (60.0, 10.0, 90.0, 50.0), (30.0, 40.0, 75.0, 75.0),      # fills, pixelate
                          (35.0, 60.0, 90.0, 90.0), (30.0, 45.0, 120.0, 65.0)],                         # a label (y 52 .. 60) under a LATER box
                         labels=[0, 1, 2, 3, 4, 5], ids=[1, 2, 3, 4, 5, 6], scores=[0.1, 0.2, 0.3, 0.4, 0.55, 0.6])
    _run(fmt, "bt709", False, [(rows, None), (rows, None)], styles, "256", what="order " + fmt)
    # alpha 0 through the default style: the fill paints nothing, the bytes stay
    _run(fmt, "bt709", False, [(ref.make_rows([(5.0, 5.0, 50.0, 50.0)]), None)] * 2, [(0, 0, 0, 0)] * 6, "w", what="alpha 0 " + fmt)


# ---------------------------------------------------------------------------------------------------------------- 4. pixelate
@pytest.mark.parametrize("fmt", ["nv12", "i420", "rgb24"])
def test_pixelate_blocks(fmt):
    styles = [(0, 0, 4, 0), (0, 0, 8, 0), (0, 0, 16, 0), (0, 0, 32, 0), (1, 0, 16, 0), (0, 90, 32, 0)]
    h, w = rr.SIZES[1]
    boxes = [(3.0, 3.0, 29.5, 21.5), (35.0, 5.0, 61.0, 27.0), (70.0, 3.0, 109.0, 40.0), (10.0, 35.0, 75.0, 75.0),          # boxes that cut blocks
             (w - 21.0, h - 30.0, w + 5.0, h + 5.0), (100.0, 45.0, float(w), 70.0), (0.0, h - 9.0, 40.0, float(h)), (80.0, 70.0, 95.0, 90.0)]
    rows = ref.make_rows(boxes, labels=[0, 1, 2, 3, 4, 5, 0, 1], ids=list(range(8)))
    _run(fmt, "bt601", False, [(rows, None), (rows, None)], styles, "w+1", what="pixelate " + fmt)


# ---------------------------------------------------------------------------------------------------------------- 5. labels
@pytest.mark.parametrize("scale", [1, 2, 3, 4])
def test_labels_at_every_scale(scale):
    k = 8 * scale
    styles = [(1, 0, 0, ref.LABEL | ref.SCORE), (1, 0, 0, ref.LABEL), (0, 0, 0, ref.LABEL | ref.SCORE), (2, 60, 0, ref.LABEL), (1, 0, 0, 0),
              (1, 0, 0, ref.LABEL | ref.SCORE)]
    boxes = [(10.0, k - 1.0, 60.0, k + 30.0), (70.0, float(k), 120.0, k + 20.0),           # the text inside (iy0 = 8k - 1) and above (iy0 = 8k)
             (200.0, 90.0, 250.0, 120.0), (20.0, 190.0, 80.0, 199.5),                        # cut at the right edge; a box near the bottom (its text is above it)
             (5.0, 100.0, 259.0, 150.0), (100.5, 160.2, 140.0, 180.0)]                       # the 31-character text
    rows = ref.make_rows(boxes, labels=[0, 1, 2, 3, 5, 2], ids=[0, 7, 999999999, 10 ** 9, 999999999, -1], scores=[0.0, 0.5, 0.994, 0.995, 1.0, NAN])
    small = ref.make_rows([(100.0, 80.0, 125.0, 92.0), (3.0, 90.0, 60.0, 96.5)], labels=[5, 0], ids=[999999999, 12], scores=[1.0, 2.0])   # cut at the right edge
    for with_ids, by in ((True, "id"), (True, "label"), (False, "id")):
        _run("nv12", "bt709", False, [(rows, None), (small, None)], styles, "w+1", with_ids=with_ids, scale=scale, colour_by=by, label_alpha=255 if by == "id" else 170,
             what="labels scale {} ids {} by {}".format(scale, with_ids, by))


@pytest.mark.parametrize("fmt", ["nv12", "rgb24"])
@pytest.mark.parametrize("scale", [1, 2, 3, 4])
def test_a_label_cut_at_the_bottom_edge(fmt, scale):
    """A label is 8 scale = k rows high and sits above its box when iy0 >= k, so its bottom passes H only in a frame lower than 2k rows: frames of
    regions_ref.SIZES cannot show it. Two short frames (same helpers): the text inside the box, cut at the bottom by one row, and cut at the
    bottom and the right at once. A score of -1 prints 0 %."""
    k = 8 * scale
    sizes = [(2 * k - 3, 100), (k + 5, 61)]
    a = ref.make_rows([(4.0, k - 2.0, 90.0, 2.0 * k - 3.0), (50.0, 1.0, 99.0, k - 3.0)], labels=[0, 1], ids=[12, 3], scores=[-1.0, 0.5])
    b = ref.make_rows([(20.5, k - 1.0, 60.0, k + 5.0)], labels=[5], ids=[999999999], scores=[1.0])
    for rows, (h, w) in ((a, sizes[0]), (b, sizes[1])):
        iy0 = int(np.floor(rows["boxes"][0][1]))
        assert iy0 < k and iy0 + k > h                      # inside its box, and its last rows lie beyond the frame
    assert ref.build_text(ref.name_records()[0], 12, True, -1.0) == b"person #12 0%"
    styles = [(1, 0, 0, ref.LABEL | ref.SCORE), (2, 0, 0, ref.LABEL), (1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 30, 0, ref.LABEL | ref.SCORE)]
    _run(fmt, "bt601", False, [(a, None), (b, None)], styles, "w+1", sizes=sizes, scale=scale, what="bottom cut {} scale {}".format(fmt, scale))


# ---------------------------------------------------------------------------------------------------------------- 6. segments
@pytest.mark.parametrize("thickness", [1, 6])
def test_segments(thickness):
    def cfg(lines, polys, n_lines=None, n_zones=None, nv=None):
        c = dict(n_lines=len(lines) if n_lines is None else n_lines, lines=np.zeros((16, 4), np.float32), n_zones=len(polys) if n_zones is None else n_zones,
                 nv=np.zeros(16, np.int32), verts=np.zeros((16, 16, 2), np.float32))
        for i, ln in enumerate(lines):
            c["lines"][i] = ln
        for z, poly in enumerate(polys):
            c["nv"][z] = len(poly) if nv is None else nv[z]
            c["verts"][z, :len(poly)] = np.asarray(poly, np.float32)
        return c
    a = cfg([(10.0, 50.5, 250.0, 50.5), (64.0, 3.0, 64.0, 190.0), (5.0, 5.0, 200.0, 180.0), (90.0, 90.0, 90.0, 90.0), (NAN, 5.0, 50.0, 60.0),
             (10.0, 10.0, INF, 40.0), (1e20, 1e20, -1e20, -1e20), (-50.0, 120.0, 400.0, 160.5), (31.5, 31.5, 32.5, 32.5)],
            [[(30.0, 100.0), (120.0, 110.0), (70.0, 140.0), (110.0, 185.0), (25.0, 170.0)], [(200.0, 20.0), (240.0, 20.0), (220.0, 60.0)]])
    # counts out of range in the table: n_lines 40 -> 16 (the rows behind the ninth are zero: degenerate), nv 99 -> 16, nv 1 -> 3, n_zones -2 -> 0
    b = cfg([(3.0, 90.0, 128.0, 4.0)], [[(10.0, 10.0), (60.0, 12.0), (40.0, 50.0)], [(70.0, 60.0), (120.0, 60.0), (100.0, 90.0), (80.0, 95.0)]],
            n_lines=40, nv=[99, 1])
    rows = ref.make_rows([(40.0, 40.0, 90.0, 80.0)], labels=[0], ids=[1])
    for alpha in (255, 100):
        _run("nv12", "bt709", False, [(rows, a), (rows, b)], [(2, 0, 0, ref.LABEL)] * 6, "w+1", line_thickness=thickness, zone_alpha=alpha,
             what="segments {} alpha {}".format(thickness, alpha))
    c = cfg([(1.0, 1.0, 50.0, 50.0)], [[(10.0, 10.0), (60.0, 12.0), (40.0, 50.0)]], n_zones=-2)
    _run("rgb24", "bt709", False, [(rows, c), (rows, a)], [(2, 0, 0, 0)] * 6, "w", sizes=[rr.SIZES[1], rr.SIZES[0]], line_thickness=thickness,
         what="segments rgb {}".format(thickness))


# ---------------------------------------------------------------------------------------------------------------- 7. a captured paint
def test_a_captured_paint_follows_surfaces_boxes_and_zones():
    fmt, matrix, full = "nv12", "bt709", False
    scenes = _mixed()
    rows, (boxes, scores, labels, counts, ids) = _tensors(scenes)
    first, second = _sources(fmt, matrix, full), _sources(fmt, matrix, full, seeds=(12, 13))
    batch = FrameBatch(2, DEV, format=fmt, matrix=matrix, full_range=full).set(_surfaces(fmt, first, "w+1"))
    ov = _overlay(2, ref.MIXED_STYLES)
    za = ZoneAnalytics(ByteTracker(2, DEV, max_tracks=8))
    lines, polys = [(5.0, 5.0, 120.0, 90.0)], [[(20.0, 15.0), (110.0, 20.0), (60.0, 45.0), (100.0, 85.0)]]
    za.set_all(lines, polys)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ov.paint(batch, boxes, scores, labels, counts, ids=ids, zones=za)        # warm-up outside the capture: tables and workspace
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stats = ov.paint(batch, boxes, scores, labels, counts, ids=ids, zones=za)
    moved = [dict(r, boxes=r["boxes"] + np.float32(7.5), count=max(r["count"] - 2, 0)) for r in rows]
    lines2, polys2 = [(3.0, 80.0, 128.0, 10.0), (64.5, 0.0, 64.5, 96.0)], [[(30.0, 30.0), (90.0, 35.0), (50.0, 80.0)]]

    def config_of(ln, pl):
        c = dict(n_lines=len(ln), lines=np.zeros((16, 4), np.float32), n_zones=len(pl), nv=np.zeros(16, np.int32), verts=np.zeros((16, 16, 2), np.float32))
        for i, l in enumerate(ln):
            c["lines"][i] = l
        for z, poly in enumerate(pl):
            c["nv"][z] = len(poly)
            c["verts"][z, :len(poly)] = np.asarray(poly, np.float32)
        return c
    got = []
    for src, rws, (ln, pl) in ((first, rows, (lines, polys)), (second, moved, (lines2, polys2)), (second, moved, (lines2, polys2))):
        surfaces = _surfaces(fmt, src, "w+1")
        table = batch.table.data_ptr()
        batch.set(surfaces)
        assert batch.table.data_ptr() == table
        boxes.copy_(torch.from_numpy(np.stack([r["boxes"] for r in rws])))
        counts.copy_(torch.from_numpy(np.asarray([r["count"] for r in rws], np.int32)))
        za.set_all(ln, pl)
        graph.replay()
        torch.cuda.synchronize()
        want = _want(fmt, matrix, full, src, rws, [config_of(ln, pl)] * 2, ref.MIXED_STYLES, ov)
        _compare(fmt, surfaces, src, want, stats.cpu().numpy(), "replay")
        got.append([p.copy() for s, planes in zip(surfaces, src) for p in _payloads(fmt, s, planes)])
    assert all(np.array_equal(a, b) for a, b in zip(got[1], got[2]))          # two replays on equal inputs: equal bits


# ---------------------------------------------------------------------------------------------------------------- 8. capacity
def _raw_call(ov, batch, tensors, rows_per_stream, workspace, za=None, **kw):
    boxes, scores, labels, counts, ids = tensors
    a = dict(frames=batch.table.data_ptr(), n=batch.n, format=batch.format_code, boxes=boxes.data_ptr(), scores=scores.data_ptr(), labels=labels.data_ptr(),
             ids=ids.data_ptr() if ids is not None else 0, counts=counts.data_ptr(), d=rows_per_stream, styles=ov._styles.data_ptr(), n_labels=ov.n_labels,
             names=ov._names.data_ptr(), palette=ov._palette.data_ptr(), font=ov._font.data_ptr(), zones=za.config.data_ptr() if za is not None else 0,
             params=ov.params, ws=workspace.data_ptr(), ws_bytes=workspace.numel(), stats=ov.stats.data_ptr())
    a.update(kw)
    p = lambda v: C.c_void_p(v) if v else None      # noqa: E731
    return _lib.lib().dn_osd_paint(p(a["frames"]), a["n"], a["format"], p(a["boxes"]), p(a["scores"]), p(a["labels"]), p(a["ids"]), p(a["counts"]), a["d"],
                                   p(a["styles"]), a["n_labels"], p(a["names"]), p(a["palette"]), p(a["font"]), p(a["zones"]),
                                   C.byref(a["params"]) if a["params"] is not None else None, p(a["ws"]), a["ws_bytes"], p(a["stats"]),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_tiles_beyond_the_capacity_are_dropped_counted_and_never_written():
    fmt, matrix, full = "i420", "bt601", False
    scenes = _mixed()
    rows, tensors = _tensors(scenes)
    d = tensors[0].shape[1]
    srcs = _sources(fmt, matrix, full)
    surfaces = _surfaces(fmt, srcs, "w+1")
    batch = FrameBatch(2, DEV, format=fmt, matrix=matrix, full_range=full).set(surfaces)
    ov = _overlay(2, ref.MIXED_STYLES)
    ov._set_space(batch)
    za = _zones([c for _, c in scenes])
    L = _lib.lib()
    capacity = 17
    fixed = L.dn_osd_workspace_bytes(2, d, 0)
    assert fixed > 0 and L.dn_osd_workspace_bytes(2, d, capacity) == fixed + 8 * capacity
    ws = torch.zeros(fixed + 8 * capacity, dtype=torch.uint8, device=DEV)
    assert _raw_call(ov, batch, tensors, d, ws, za) == 0
    torch.cuda.synchronize()
    stats = ov.stats.cpu().numpy()
    host = ws.cpu().numpy()
    marked = int(host[8:12].view(np.int32)[0])                                   # word 2: what the call marked; words 0 and 1 are zero again
    assert not host[:8].any()
    assert marked == stats[:, 2].sum() and marked > 2 * capacity
    assert stats[:, 3].sum() == marked - capacity
    kept = {tuple(e) for e in host[fixed:].view(np.int32).reshape(capacity, 2)}
    assert len(kept) == capacity                                                  # a set: the list's order is free
    want = _want(fmt, matrix, full, srcs, rows, [c for _, c in scenes], ref.MIXED_STYLES, ov)
    changed = 0
    for b, (surface, planes, (wp, _)) in enumerate(zip(surfaces, srcs, want)):
        h, w = rr.SIZES[b]
        tiles_x = (w + 31) // 32
        assert all(0 <= t < tiles_x * ((h + 31) // 32) for s, t in kept if s == b)
        got_c, _ = ref.split(fmt, _payloads(fmt, surface, planes))
        want_c, subs = ref.split(fmt, wp)
        orig_c, _ = ref.split(fmt, planes)
        for ty in range((h + 31) // 32):
            for tx in range(tiles_x):
                for g, wc, oc, s in zip(got_c, want_c, orig_c, subs):
                    e = 32 // s
                    sl = (slice(ty * e, ty * e + e), slice(tx * e, tx * e + e))
                    expect = wc[sl] if (b, ty * tiles_x + tx) in kept else oc[sl]
                    assert np.array_equal(g[sl], expect), (b, ty, tx)
                    changed += int((b, ty * tiles_x + tx) in kept and not np.array_equal(wc[sl], oc[sl]))
    assert changed >= 1


# ---------------------------------------------------------------------------------------------------------------- 9. behind the tracker
def test_paint_behind_the_tracker():
    m = models.load_synthetic(models.ssd_lite_mobilenet_v2(image_size=160, num_classes=3), 0).to(DEV)
    try:
        fmt, matrix, full = "nv12", "bt709", False
        srcs = _sources(fmt, matrix, full)
        kw = dict(max_tracks=64, track_thresh=0.05, low_thresh=0.01, new_thresh=0.05)
        tracker, twin = ByteTracker(2, DEV, **kw), ByteTracker(2, DEV, **kw)
        za, zb = ZoneAnalytics(tracker), ZoneAnalytics(twin)
        lines, polys = [(5.0, 5.0, 120.0, 90.0)], [[(20.0, 15.0), (110.0, 20.0), (60.0, 45.0), (100.0, 85.0)]]
        za.set_all(lines, polys)
        zb.set_all(lines, polys)
        names = ["background", "thing", "other"]
        styles = [(2, 0, 0, ref.LABEL | ref.SCORE), (2, 40, 0, ref.LABEL | ref.SCORE), (1, 0, 8, ref.LABEL)]
        ov = osd.Overlay(2, DEV, names=names, palette=ref.PALETTE_RGB, scale=1)
        for lb, (t, a, p, f) in enumerate(styles):
            ov.set_style(lb, thickness=t, fill_alpha=a, pixelate=p, label=bool(f & ref.LABEL), score=bool(f & ref.SCORE))
        cfg = dict(n_lines=1, lines=np.zeros((16, 4), np.float32), n_zones=1, nv=np.zeros(16, np.int32), verts=np.zeros((16, 16, 2), np.float32))
        cfg["lines"][0] = lines[0]
        cfg["nv"][0] = 4
        cfg["verts"][0, :4] = np.asarray(polys[0], np.float32)
        pal = ref.palette_records(ref.PALETTE_RGB, fmt, matrix, full)
        painted = 0
        for step in range(3):
            plain = FrameBatch(2, DEV, format=fmt, matrix=matrix, full_range=full).set(_surfaces(fmt, srcs, "256"))
            surfaces = _surfaces(fmt, srcs, "256")
            batch = FrameBatch(2, DEV, format=fmt, matrix=matrix, full_range=full).set(surfaces)
            want_outs = m.track_frames(plain, twin, analytics=zb)
            want_outs = [t.clone() for t in want_outs[:-1]] + [tuple(t.clone() for t in want_outs[-1])]
            outs = m.track_frames(batch, tracker, analytics=za, osd=ov)
            torch.cuda.synchronize()
            assert len(outs) == len(want_outs) == 8
            for a, b in zip(outs[:-1], want_outs[:-1]):
                assert torch.equal(a, b)
            assert all(torch.equal(a, b) for a, b in zip(outs[-1], want_outs[-1]))
            boxes, scores, labels, ids, _, counts = (t.cpu().numpy() for t in outs[:6])
            stats = ov.stats.cpu().numpy()
            for b in range(2):
                rows = dict(boxes=boxes[b], scores=scores[b], labels=labels[b], ids=ids[b], count=int(counts[b]))
                chans, subs = ref.split(fmt, srcs[b])
                got, counted = ref.paint(chans, subs, rows, styles, None, 3, [n.encode().ljust(16, b"\0") for n in names], pal, FONT, cfg,
                                         _ref_params(ov, fmt, matrix, full))
                for g, w in zip(_payloads(fmt, surfaces[b], srcs[b]), ref.join(fmt, got)):
                    assert np.array_equal(g, w), (step, b)
                assert tuple(stats[b, :2]) == counted
                painted += counted[0]
        assert painted >= 2
        with pytest.raises(ValueError, match="osd must be an Overlay"):
            m.track_frames(batch, tracker, osd=tracker)
    finally:
        m.release()


def test_paint_behind_the_sliced_and_the_appearance_steps():
    """osd= of track_sliced_frames and track_frames_appearance: after each step the surfaces equal osd_ref applied to what the step returned."""
    import crops_ref as cr
    from demonet_amd.crops import ObjectCropper
    from demonet_amd.sliced import FrameSlicer
    from demonet_amd.track import AppearanceTracker
    m = models.load_synthetic(models.ssd_lite_mobilenet_v2(image_size=160, num_classes=3), 0).to(DEV)
    try:
        fmt, matrix, full = "nv12", "bt709", False
        srcs = _sources(fmt, matrix, full)
        kw = dict(max_tracks=64, track_thresh=0.05, low_thresh=0.01, new_thresh=0.05)
        names = ["background", "thing", "other"]
        styles = [(2, 0, 0, ref.LABEL | ref.SCORE), (1, 0, 0, ref.LABEL | ref.SCORE), (2, 50, 0, ref.LABEL)]
        ov = osd.Overlay(2, DEV, names=names, palette=ref.PALETTE_RGB, scale=1)
        for lb, (t, a, p, f) in enumerate(styles):
            ov.set_style(lb, thickness=t, fill_alpha=a, pixelate=p, label=bool(f & ref.LABEL), score=bool(f & ref.SCORE))
        pal = ref.palette_records(ref.PALETTE_RGB, fmt, matrix, full)
        records = [n.encode().ljust(16, b"\0") for n in names]

        def check(step, surfaces, outs):
            torch.cuda.synchronize()
            boxes, scores, labels, ids, _, counts = (t.cpu().numpy() for t in outs[:6])
            stats = ov.stats.cpu().numpy()
            painted = 0
            for b in range(2):
                rows = dict(boxes=boxes[b], scores=scores[b], labels=labels[b], ids=ids[b], count=int(counts[b]))
                chans, subs = ref.split(fmt, srcs[b])
                got, counted = ref.paint(chans, subs, rows, styles, None, 3, records, pal, FONT, None, _ref_params(ov, fmt, matrix, full))
                for g, w in zip(_payloads(fmt, surfaces[b], srcs[b]), ref.join(fmt, got)):
                    assert np.array_equal(g, w), (step, b)
                assert tuple(stats[b, :2]) == counted
                painted += counted[0]
            return painted

        tracker = ByteTracker(2, DEV, **kw)
        slicer = FrameSlicer(m, rr.SIZES, max_tiles_per_forward=3)
        painted = 0
        for step in range(2):
            surfaces = _surfaces(fmt, srcs, "w+1")
            batch = FrameBatch(2, DEV, format=fmt, matrix=matrix, full_range=full).set(surfaces)
            painted += check(("sliced", step), surfaces, m.track_sliced_frames(batch, tracker, slicer, osd=ov))
        assert painted >= 1

        dim = 32
        app = AppearanceTracker(2, DEV, dim, **kw)
        cropper = ObjectCropper(2, DEV, size=(16, 8), capacity=128, dtype=torch.float16, mean=cr.IMAGENET_MEAN, std=cr.IMAGENET_STD)
        cropper.patches.zero_()
        W = torch.from_numpy(np.random.RandomState(9).normal(0, 1, (3 * 16 * 8, dim)).astype(np.float32)).to(DEV)
        embedder = lambda patches: patches.reshape(patches.shape[0], -1).float() @ W      # noqa: E731
        painted = 0
        for step in range(2):
            surfaces = _surfaces(fmt, srcs, "256")
            batch = FrameBatch(2, DEV, format=fmt, matrix=matrix, full_range=full).set(surfaces)
            painted += check(("appearance", step), surfaces, m.track_frames_appearance(batch, app, cropper, embedder, osd=ov))
        assert painted >= 1
    finally:
        m.release()


# ---------------------------------------------------------------------------------------------------------------- 10. refusals
def test_every_error_code_of_the_entry_point():
    DN_E_INVALID, DN_E_WORKSPACE, DN_E_UNSUPPORTED = -1, -3, -4
    fmt, matrix, full = "nv12", "bt709", False
    srcs = _sources(fmt, matrix, full)
    surfaces = _surfaces(fmt, srcs, "w+1")
    batch = FrameBatch(2, DEV, format=fmt, matrix=matrix, full_range=full).set(surfaces)
    rows, tensors = _tensors(_mixed())
    d = tensors[0].shape[1]
    ov = _overlay(2, ref.MIXED_STYLES)
    ov._set_space(batch)
    L = _lib.lib()
    for s, dd, cap in ((0, d, 1), (2, 0, 1), (2, d, -1), (65536, d, 1), (2, 513, 1)):
        assert L.dn_osd_workspace_bytes(s, dd, cap) == 0
    fixed = L.dn_osd_workspace_bytes(2, d, 0)
    ws = torch.zeros(fixed + 8 * 200, dtype=torch.uint8, device=DEV)
    big = torch.zeros(4096 * 16, dtype=torch.uint8, device=DEV)

    def with_params(**kw):
        rec = _lib.OsdParams.from_buffer_copy(ov.params)
        for k, v in kw.items():
            if k.startswith("style_"):
                setattr(rec.default_style, k[6:], v)
            elif k == "reserved":
                rec.reserved[2] = v
            else:
                setattr(rec, k, v)
        return rec
    invalid = [dict(frames=0), dict(boxes=0), dict(scores=0), dict(labels=0), dict(counts=0), dict(palette=0), dict(font=0), dict(params=None), dict(ws=0),
               dict(stats=0), dict(names=0), dict(n=0), dict(d=0), dict(n_labels=0), dict(format=4), dict(format=-1),
               dict(boxes=tensors[0].data_ptr() + 4), dict(ws=ws.data_ptr() + 8), dict(stats=ov.stats.data_ptr() + 4), dict(labels=tensors[2].data_ptr() + 4),
               dict(ids=tensors[4].data_ptr() + 4), dict(scores=tensors[1].data_ptr() + 2), dict(counts=tensors[3].data_ptr() + 1),
               dict(zones=big.data_ptr() + 8), dict(styles=ov._styles.data_ptr() + 4), dict(palette=ov._palette.data_ptr() + 4)]
    invalid += [dict(params=with_params(**kw)) for kw in (dict(scale=0), dict(scale=5), dict(line_thickness=0), dict(zone_thickness=65), dict(style_thickness=17),
                                                          dict(style_pixelate=5), dict(style_flags=8), dict(n_colors=0), dict(n_colors=257), dict(label_alpha=256),
                                                          dict(zone_alpha=-1), dict(color_by_id=2), dict(reserved=1), dict(reserved0=1))]
    before = [p.copy() for s, planes in zip(surfaces, srcs) for p in _payloads(fmt, s, planes)]
    for kw in invalid:
        assert _raw_call(ov, batch, tensors, d, ws, **kw) == DN_E_INVALID, kw
        assert L.dn_last_error()
    assert _raw_call(ov, batch, tensors, 513, ws) == DN_E_UNSUPPORTED
    assert _raw_call(ov, batch, tensors, d, ws, n=65536) == DN_E_UNSUPPORTED
    assert _raw_call(ov, batch, tensors, d, ws, ws_bytes=fixed + 7) == DN_E_WORKSPACE
    assert _raw_call(ov, batch, tensors, d, ws, ws_bytes=0) == DN_E_WORKSPACE
    torch.cuda.synchronize()
    after = [p for s, planes in zip(surfaces, srcs) for p in _payloads(fmt, s, planes)]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))               # every error is raised before anything is enqueued
    # the optional pointers may be null: no ids, no styles (the default style, here without a label), no zones, and then no names either
    quiet = with_params(style_flags=0)
    assert _raw_call(ov, batch, tensors, d, ws, ids=0, styles=0, zones=0, names=0, params=quiet) == 0
    torch.cuda.synchronize()
    assert _lib.debug_last_kernel() == "osd_paint_kernel<0>"
    assert (ov.stats.cpu().numpy()[:, 0] >= 6).all()
