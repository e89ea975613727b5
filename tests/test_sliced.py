"""Sliced inference: dn_crop_tiles, dn_merge_detections, demonet_amd/sliced.py and SSD.detect_sliced.

CPU part: the ABI, tile_grid, and the reference itself (tests/sliced_ref.py: pinned to the project's oracle NMS, idempotent, and every GPU case meets
the condition under which exact equality is the right demand -- no compared pair sits on the threshold). GPU part: the crop against torch slicing
bit for bit, the merge against merge_ref exactly, the rejections, and detect_sliced against the composition a user would write by hand."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import sliced_ref as sr
from demonet_amd import _lib, models, sliced, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dn_crop_tiles", "dn_merge_detections_workspace_bytes", "dn_merge_detections")
f32 = np.float32


# ----------------------------------------------------------------------------------------------------------------------------------
# merge cases: dict(boxes [S,d,4], scores [S,d], labels [S,d], counts [S], offsets [S,2], group_begin, metric, thresh, agnostic, d_out)
# ----------------------------------------------------------------------------------------------------------------------------------
def _clustered(seed, S, d, n_labels, n_clusters, counts, lattice=False, shuffle=False, extent=1500.0):
    """Boxes around n_clusters centres in image coordinates, reported by S sources through one offset each (the source's box = image box - offset),
    scores descending inside a source (shuffle: in random row order), rows at or beyond the count filled with plausible garbage."""
    rng = np.random.default_rng(seed)
    q = (lambda v: np.round(v * 4) / 4) if lattice else (lambda v: v)
    ctr = rng.uniform(100, extent, (n_clusters, 2))
    size = rng.uniform(30, 120, (n_clusters, 2))
    which = rng.integers(0, n_clusters, (S, d))
    c = ctr[which] + rng.normal(0, 4.0, (S, d, 2))
    wh = size[which] * rng.uniform(0.85, 1.15, (S, d, 2))
    img = q(np.concatenate([c - wh / 2, c + wh / 2], -1))
    off = q(rng.uniform(0, 64, (S, 2)))
    boxes = (img - np.concatenate([off, off], -1)[:, None, :]).astype(f32)
    scores = np.sort(rng.uniform(0.01, 1.0, (S, d)).astype(f32), axis=1)[:, ::-1].copy()
    if shuffle:
        scores = rng.permuted(scores, axis=1)
    labels = rng.integers(1, n_labels + 1, (S, d)).astype(np.int64)
    return dict(boxes=boxes, scores=scores, labels=labels, counts=np.asarray(counts, np.int32), offsets=off.astype(f32))


def _embed(case, before, after, seed=99):
    """The same sources inside larger arrays: `before` and `after` more sources, with full counts, that belong to no group."""
    d = case["scores"].shape[1]
    pad = _clustered(seed, before + after, d, 3, 5, [d] * (before + after))
    out = dict(case)
    for k in ("boxes", "scores", "labels", "counts", "offsets"):
        out[k] = np.concatenate([pad[k][:before], case[k], pad[k][before:]], 0)
    out["group_begin"] = [b + before for b in case["group_begin"]]
    return out


@functools.lru_cache(maxsize=None)
def merge_case(name):
    base = dict(metric=sr.IOU, thresh=0.5, agnostic=0)
    if name == "a_identity":            # one source, boxes that do not overlap: the output is the input
        g = np.arange(12)
        x, y = 40.0 * (g % 4), 40.0 * (g // 4)
        b = np.zeros((1, 16, 4), f32)
        b[0, :12] = np.stack([x, y, x + 30, y + 30], 1)
        b[0, 12:] = 7.0
        s = np.zeros((1, 16), f32)
        s[0, :12] = np.linspace(0.9, 0.1, 12, dtype=f32)
        s[0, 12:] = 0.99
        c = dict(base, boxes=b, scores=s, labels=np.full((1, 16), 3, np.int64), counts=np.array([12], np.int32), offsets=np.zeros((1, 2), f32),
                 group_begin=[0, 1], d_out=16)
        return _embed(c, 1, 1)
    if name in ("b_two_tiles", "c_equal_scores"):
        # 4 sources x 8 rows. The object at (100, 100, 160, 150) of the image is seen by source 0 (offset 0, 0) and by source 1 (offset 64, 0); with
        # b the second report has the higher score and survives, with c the scores are equal and the lower flattened index (source 0) survives
        c = _clustered(3, 4, 8, 2, 40, [5, 6, 8, 0])
        c["offsets"] = np.array([[0, 0], [64, 0], [0, 48], [64, 48]], f32)
        c["boxes"][0, 2] = (100, 100, 160, 150)
        c["boxes"][1, 1] = (100 - 64 + 1, 100, 160 - 64 + 1, 150)
        c["labels"][0, 2] = c["labels"][1, 1] = 1
        c["scores"][0, 2] = 0.80
        c["scores"][1, 1] = 0.90 if name == "b_two_tiles" else 0.80
        return _embed(dict(base, **c, group_begin=[0, 4], d_out=20), 0, 2)
    if name == "d_chunks":              # 6 x 300 over 5 labels: the walk spans several chunks and leaves with d_out kept
        return _embed(dict(base, **_clustered(11, 6, 300, 5, 70, [300] * 6), group_begin=[0, 6], d_out=300), 2, 0)
    if name == "d_lattice":             # the same on the quarter-pixel lattice: every sum, area and intersection is exact
        return dict(base, **_clustered(12, 6, 300, 5, 70, [300] * 6, lattice=True), group_begin=[0, 6], d_out=300)
    if name == "e_empty_group":         # two groups (CSR): the first has three sources with nothing in them, and one group has no source at all
        c = _clustered(13, 6, 40, 3, 30, [0, 0, 0, 40, 17, 1])
        return dict(base, **c, group_begin=[0, 3, 3, 6], d_out=64)
    if name == "f_agnostic":
        return dict(base, **_clustered(14, 5, 64, 4, 60, [64, 50, 64, 3, 64]), group_begin=[0, 5], d_out=100, agnostic=1)
    if name in ("g_nested_iou", "g_nested_ios"):
        # a 20 x 20 box inside a 100 x 100 one of the same label: IoU 0.04 keeps it, intersection over the smaller box is 1 and removes it
        c = _clustered(15, 2, 8, 2, 12, [4, 4], extent=600.0)
        c["offsets"] = np.array([[0, 0], [32, 16]], f32)
        c["boxes"][0, 0] = (700, 700, 800, 800)
        c["boxes"][1, 0] = (740 - 32, 740 - 16, 760 - 32, 760 - 16)
        c["labels"][0, 0] = c["labels"][1, 0] = 2
        c["scores"][0, 0], c["scores"][1, 0] = 0.95, 0.94
        return dict(base, **c, group_begin=[0, 2], d_out=16, metric=sr.IOS if name.endswith("ios") else sr.IOU)
    if name == "h_many_slots":          # 64 x 300 = 19 200 slots in one group; few clusters: fewer than d_out survive, the walk goes to the end
        cnt = np.random.default_rng(16).integers(0, 301, 64)
        return dict(base, **_clustered(16, 64, 300, 5, 30, cnt), group_begin=[0, 64], d_out=300)
    if name == "i_shuffled":
        return dict(base, **_clustered(17, 5, 48, 3, 40, [48, 20, 48, 31, 7], shuffle=True), group_begin=[0, 5], d_out=60)
    if name == "j_three_tables":
        # 131 groups: the library hands the kernels 64 groups per launch, so three tables, the second and third with a first group > 0. Two sources
        # of 4 rows per group on 3 centres (pairs across the sources overlap), ragged counts; group 64, the first of the second table, has no
        # source; source 260 belongs to no group
        gb = MANY_GROUPS
        cnt = np.random.default_rng(18).integers(0, 5, gb[-1] + 1)
        return dict(base, **_clustered(18, gb[-1] + 1, 4, 2, 3, cnt), group_begin=gb, d_out=6)
    raise KeyError(name)


MANY_GROUPS = [2 * g for g in range(65)] + [2 * g for g in range(64, 131)]      # 132 entries; [64] == [65] == 128; ends at 260
MERGE_CASES = ("a_identity", "b_two_tiles", "c_equal_scores", "d_chunks", "d_lattice", "e_empty_group", "f_agnostic", "g_nested_iou", "g_nested_ios",
               "h_many_slots", "i_shuffled", "j_three_tables")


@functools.lru_cache(maxsize=None)
def merge_expected(name):
    c = merge_case(name)
    return sr.merge_ref(c["boxes"], c["scores"], c["labels"], c["counts"], c["offsets"], c["group_begin"], c["metric"], c["thresh"], c["agnostic"],
                        c["d_out"])


# ----------------------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------------------
def test_the_three_symbols_are_exported_declared_and_bound():
    if not os.path.exists(_lib.LIB_PATH):
        from demonet_amd import build
        build.build(verbose=False)
    L = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "demonet_hip.h")).read()
    declared = set(re.findall(r"DN_API\s+[\w\s\*]+?\b(dn_\w+)\s*\(", header))
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in declared, n
        assert n in _lib.EXPORTS, n
    assert "DN_MERGE_IOU = 0" in header and "DN_MERGE_IOS = 1" in header and _lib.DN_MERGE == dict(iou=0, ios=1)
    assert "#define DN_ABI_VERSION 1" in header and _lib.DN_ABI_VERSION == 1
    L.dn_merge_detections_workspace_bytes.restype = C.c_size_t
    assert L.dn_merge_detections_workspace_bytes(41, 300, 1) >= 41 * 300 * 8       # pure host arithmetic
    assert L.dn_merge_detections_workspace_bytes(1, 513, 1) == 0 and L.dn_merge_detections_workspace_bytes(0, 8, 1) == 0


GRIDS = [(500, 700, 320, 320, 0.25),        # the worked example
         (200, 900, 320, 320, 0.25),        # smaller than the tile in one axis
         (640, 960, 320, 320, 0.0),         # an exact multiple, overlap 0
         (333, 517, 128, 96, 0.0),          # overlap 0, no multiple
         (1080, 1920, 320, 320, 0.25)]


def test_tile_grid_worked_example():
    origins, th, tw = sliced.tile_grid(500, 700, 320, 320, 0.25)
    assert (th, tw) == (320, 320)
    assert origins == [(0, 0), (240, 0), (380, 0), (0, 180), (240, 180), (380, 180)]
    assert len(sliced.tile_grid(1080, 1920, 320, 320, 0.25)[0]) == 40
    assert sliced.tile_grid(320, 320, 320, 320, 0.25) == ([(0, 0)], 320, 320)
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            sliced.tile_grid(500, 700, 320, 320, bad)
    with pytest.raises(ValueError):
        sliced.tile_grid(500, 700, 0, 320, 0.25)


@pytest.mark.parametrize("H,W,th,tw,overlap", GRIDS)
def test_tile_grid_covers_the_image_with_equal_tiles_inside_it(H, W, th, tw, overlap):
    origins, th2, tw2 = sliced.tile_grid(H, W, th, tw, overlap)
    assert (origins, th2, tw2) == sr.tile_grid_ref(H, W, th, tw, overlap)
    assert (th2, tw2) == (min(th, H), min(tw, W))
    cover = np.zeros((H, W), bool)
    for x0, y0 in origins:
        assert 0 <= x0 <= W - tw2 and 0 <= y0 <= H - th2                       # inside the image; one size for all
        cover[y0:y0 + th2, x0:x0 + tw2] = True
    assert cover.all()
    xs, ys = sorted({x for x, _ in origins}), sorted({y for _, y in origins})
    assert origins == [(x, y) for y in ys for x in xs]                          # a full grid, row-major
    for vals, tile in ((xs, tw2), (ys, th2)):
        stride = max(1, tile - int(round(overlap * tile)))
        assert vals[0] == 0 and all(0 < b - a <= stride for a, b in zip(vals, vals[1:]))


def test_merge_ref_keeps_what_the_oracle_nms_keeps():
    """One source, zero offset, IoU, per class: merge_ref keeps exactly the boxes oracle/nms_c.c (through fast_post) keeps on the same candidates
    sorted by class, then score."""
    import fast_post
    L = fast_post._nms()
    rng = np.random.default_rng(21)
    for trial in range(3):
        c = _clustered(30 + trial, 1, 400, 4, 50, [400])
        c["scores"] = rng.permutation(np.linspace(0.05, 0.95, 400).astype(f32))[None]       # tie-free
        thr = 0.5
        ob, os_, ol, oc, src, margin = sr.merge_ref(c["boxes"], c["scores"], c["labels"], c["counts"], np.zeros((1, 2), f32), [0, 1], sr.IOU, thr, 0, 400)
        assert margin > 0
        order = np.lexsort((-c["scores"][0], c["labels"][0]))                     # class-major, score-descending inside a class
        cb = np.ascontiguousarray(c["boxes"][0][order])
        lab = c["labels"][0][order]
        seg = np.searchsorted(lab, np.arange(1, 6)).astype(np.int32)              # labels 1 .. 4 -> 4 segments
        keep = np.zeros(400, np.uint8)
        kept = L.nms_segments(cb.ctypes.data, seg.ctypes.data, 4, C.c_float(thr), keep.ctypes.data)
        assert kept == int(oc[0]) and 0 < kept < 400
        assert sorted(order[np.nonzero(keep)[0]].tolist()) == sorted(src[0, :kept].tolist())
        assert np.all(np.diff(os_[0, :kept]) <= 0)                                # ... reported in global score order


@pytest.mark.parametrize("name", ["d_chunks", "f_agnostic", "g_nested_ios"])
def test_merging_a_merged_result_changes_nothing(name):
    c = merge_case(name)
    ob, os_, ol, oc, _, _ = merge_expected(name)
    G = len(c["group_begin"]) - 1
    again = sr.merge_ref(ob, os_, ol, oc, np.zeros((G, 2), f32), list(range(G + 1)), c["metric"], c["thresh"], c["agnostic"], c["d_out"])
    for x, y in zip((ob, os_, ol, oc), again[:4]):
        assert np.array_equal(x, y)
    assert int(oc.sum()) > 0


@pytest.mark.parametrize("name", MERGE_CASES)
def test_every_gpu_merge_case_meets_its_input_condition(name):
    """No compared pair sits on the threshold (margin > 0), and each case shows what it is there for."""
    c = merge_case(name)
    ob, os_, ol, oc, src, margin = merge_expected(name)
    assert margin > 0, margin
    d = c["scores"].shape[1]
    first = c["group_begin"][0]
    if name == "a_identity":
        assert int(oc[0]) == 12 and np.array_equal(src[0, :12], first * d + np.arange(12))
    if name == "b_two_tiles":
        assert (first + 1) * d + 1 in src[0] and first * d + 2 not in src[0]
    if name == "c_equal_scores":
        assert first * d + 2 in src[0] and (first + 1) * d + 1 not in src[0]
    if name in ("d_chunks", "d_lattice"):
        assert int(oc[0]) == 300
        rank_of_last = int((c["scores"][c["group_begin"][0]:c["group_begin"][-1]] >= os_[0, 299]).sum())
        assert 512 < rank_of_last < 1500                                          # several chunks of 256, and an early exit
    if name == "d_lattice":
        for k in ("boxes", "offsets"):
            assert np.array_equal(c[k] * 4, np.round(c[k] * 4)) and np.abs(c[k]).max() < 2048
    if name == "e_empty_group":
        assert oc.tolist()[:2] == [0, 0] and int(oc[2]) > 0
    if name == "f_agnostic":
        per_class = sr.merge_ref(c["boxes"], c["scores"], c["labels"], c["counts"], c["offsets"], c["group_begin"], c["metric"], c["thresh"], 0, c["d_out"])
        assert int(oc[0]) < int(per_class[3][0])
    if name == "g_nested_iou":
        assert d + 0 in src[0] and 0 in src[0]
    if name == "g_nested_ios":
        assert d + 0 not in src[0] and 0 in src[0]
    if name == "h_many_slots":
        assert c["scores"].shape == (64, 300) and 0 < int(oc[0]) < 300
    if name == "i_shuffled":
        assert any(np.any(np.diff(c["scores"][s, :c["counts"][s]]) > 0) for s in range(5))
    if name == "j_three_tables":
        gb = c["group_begin"]
        assert len(gb) - 1 == 131 and gb[64] == gb[65] and int(oc[64]) == 0 and gb[-1] < c["scores"].shape[0] and c["d_out"] > d
        cand = np.array([c["counts"][a:b].sum() for a, b in zip(gb, gb[1:])])
        for lo, hi in ((0, 64), (64, 128), (128, 131)):                           # every table keeps something and suppresses something
            assert (oc[lo:hi] > 0).any() and (oc[lo:hi] < cand[lo:hi]).any(), (lo, hi)
        assert len(set(c["counts"].tolist())) == 5                                # ragged: every count 0 .. 4


# ----------------------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------------------
def _crop(img, origins, th, tw):
    """-> (return code, output [t, 3, th, tw] pre-filled with NaN)"""
    t = len(origins)
    out = torch.full((t, 3, th, tw), float("nan"), dtype=torch.float32, device="cuda")
    o = torch.tensor(origins, dtype=torch.int32, device="cuda")
    rc = _lib.lib().dn_crop_tiles(C.c_void_p(img.data_ptr()), img.shape[1], img.shape[2], C.c_void_p(o.data_ptr()), t, th, tw,
                                  C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, out


CROPS = [(37, 53, 16, 24, [(0, 0), (12, 5), (29, 21), (29, 0), (7, 21), (1, 13)]),      # 29 = 53 - 24: the clamped last column; odd x0; scalar rows (w odd)
         (37, 53, 16, 22, [(0, 0), (13, 5), (31, 21)]),                                  # tw not a multiple of 4
         (40, 64, 16, 24, [(0, 0), (12, 5), (40, 24), (40, 0), (7, 21), (1, 13), (36, 3)]),   # 16-byte rows: aligned and unaligned x0 side by side
         (70, 64, 66, 64, [(0, 0), (0, 4), (0, 1)])]                                     # more than one workgroup per plane, 16-byte path


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,th,tw,origins", CROPS)
def test_crop_tiles_equals_torch_slicing_bit_for_bit(H, W, th, tw, origins):
    img = torch.from_numpy(synth.images(7, 1, H, W)[0]).cuda()
    rc, out = _crop(img, origins, th, tw)
    assert rc == 0, _lib.lib().dn_last_error()
    want = torch.stack([img[:, y:y + th, x:x + tw] for x, y in origins])
    assert torch.equal(out.view(torch.int32), want.contiguous().view(torch.int32))
    assert torch.equal(sliced.crop_tiles(img, torch.tensor(origins, dtype=torch.int32, device="cuda"), th, tw), want)


@pytest.mark.gpu
def test_crop_tiles_rejections():
    img = torch.from_numpy(synth.images(7, 1, 37, 53)[0]).cuda()
    for origins in ([(0, 0), (30, 5)], [(0, 22)], [(-1, 0)], [(0, 0), (0, -3)]):      # 30 + 24 > 53; 22 + 16 > 37; negative
        rc, out = _crop(img, origins, 16, 24)
        assert rc == -1, origins
        assert bool(torch.isnan(out).all())                                        # nothing was written
    assert _crop(img, [(0, 0)], 38, 24)[0] == -1 and _crop(img, [(0, 0)], 16, 54)[0] == -1      # a tile larger than the image
    L = _lib.lib()
    o = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    out = torch.empty((1, 3, 16, 24), device="cuda")
    p = C.c_void_p
    assert L.dn_crop_tiles(None, 37, 53, p(o.data_ptr()), 1, 16, 24, p(out.data_ptr()), None) == -1
    assert L.dn_crop_tiles(p(img.data_ptr()), 37, 53, None, 1, 16, 24, p(out.data_ptr()), None) == -1
    assert L.dn_crop_tiles(p(img.data_ptr()), 37, 53, p(o.data_ptr()), 1, 16, 24, None, None) == -1
    for t, th, tw in ((0, 16, 24), (1, 0, 24), (1, 16, -2)):                       # non-positive sizes
        assert L.dn_crop_tiles(p(img.data_ptr()), 37, 53, p(o.data_ptr()), t, th, tw, p(out.data_ptr()), None) == -1


def _merge(c, ws_bytes=None, want_src=True, **over):
    """One dn_merge_detections call on the case -> (return code, five numpy outputs). Workspace and outputs are pre-filled with 0xFF bytes (NaN)."""
    c = dict(c, **over)
    L = _lib.lib()
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("boxes", "scores", "labels", "counts", "offsets")}
    S, d = c["scores"].shape
    S, d = over.get("s_total", S), over.get("d", d)
    gb = c["group_begin"]
    G, d_out = len(gb) - 1, c["d_out"]
    need = L.dn_merge_detections_workspace_bytes(S, d, G)
    ws = torch.full((max(need if ws_bytes is None else ws_bytes, 16),), 0xFF, dtype=torch.uint8, device="cuda")
    rows = max(d_out, 1)
    ob = torch.full((G, rows, 4), float("nan"), dtype=torch.float32, device="cuda")
    os_ = torch.full((G, rows), float("nan"), dtype=torch.float32, device="cuda")
    ol = torch.full((G, rows), -1, dtype=torch.int64, device="cuda")
    oc = torch.full((G,), -1, dtype=torch.int32, device="cuda")
    src = torch.full((G, rows), -7, dtype=torch.int32, device="cuda")
    p = C.c_void_p
    rc = L.dn_merge_detections(p(t["boxes"].data_ptr()), p(t["scores"].data_ptr()), p(t["labels"].data_ptr()), p(t["counts"].data_ptr()),
                               p(t["offsets"].data_ptr()), S, d, (C.c_int32 * (G + 1))(*gb), G, c["metric"], c["thresh"], c["agnostic"], d_out,
                               p(ob.data_ptr()), p(os_.data_ptr()), p(ol.data_ptr()), p(oc.data_ptr()), p(src.data_ptr()) if want_src else None,
                               p(ws.data_ptr()), ws.numel() if ws_bytes is None else ws_bytes, p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, [x.cpu().numpy() for x in (ob, os_, ol, oc, src)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", MERGE_CASES)
def test_merge_detections_equals_the_reference_exactly(name):
    c = merge_case(name)
    want = merge_expected(name)
    rc, got = _merge(c)
    assert rc == 0, _lib.lib().dn_last_error()
    for w, g, what in zip(want[:5], got, ("boxes", "scores", "labels", "counts", "src")):
        if w.dtype == np.float32:
            w, g = w.view(np.int32), g.view(np.int32)
        assert np.array_equal(w, g), what
    rc, again = _merge(c)
    assert rc == 0
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()                                          # deterministic: the same bits on a second run
    rc, nosrc = _merge(c, want_src=False)                                          # src_out is optional
    assert rc == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(got[:4], nosrc[:4])) and bool((nosrc[4] == -7).all())


@pytest.mark.gpu
def test_merge_detections_rejections():
    INVALID, WORKSPACE, UNSUPPORTED = -1, -3, -4

    def tiny(S, d):
        return dict(boxes=np.zeros((S, d, 4), f32), scores=np.zeros((S, d), f32), labels=np.zeros((S, d), np.int64), counts=np.zeros(S, np.int32),
                    offsets=np.zeros((S, 2), f32), group_begin=[0, S], metric=sr.IOU, thresh=0.5, agnostic=0, d_out=8)
    assert _merge(tiny(1, 513))[0] == UNSUPPORTED                                  # d = 513
    assert _merge(tiny(1025, 1))[0] == UNSUPPORTED                                 # 1 025 sources in one group
    assert _merge(tiny(1024, 1))[0] == 0
    assert _merge(tiny(129, 512))[0] == UNSUPPORTED                                # 66 048 slots in one group
    assert _merge(dict(tiny(256, 512), group_begin=[0, 128, 256]))[0] == 0         # ... two groups of 65 536 are fine
    assert _merge(tiny(2, 8), d_out=0)[0] == INVALID
    assert _merge(tiny(2, 8), d_out=513)[0] == UNSUPPORTED
    assert _merge(dict(tiny(4, 8), group_begin=[0, 3, 2, 4]))[0] == INVALID        # a decreasing group_begin
    assert _merge(dict(tiny(4, 8), group_begin=[0, 5]))[0] == INVALID              # beyond s_total
    assert _merge(tiny(2, 8), ws_bytes=16)[0] == WORKSPACE
    assert _merge(tiny(2, 8), metric=2)[0] == INVALID
    assert _merge(tiny(2, 8), agnostic=2)[0] == INVALID
    assert _merge(tiny(2, 8), thresh=float("nan"))[0] == INVALID
    assert _merge(tiny(2, 8))[0] == 0


IMG_SEED = 1008


@pytest.fixture(scope="module")
def model():
    return models.load_synthetic(models.ssdlite320_mobilenet_v3_large(num_classes=21), 0).cuda()


def _image(h, w, seed=IMG_SEED):
    return torch.from_numpy(synth.images(seed, 1, h, w)[0]).cuda()


def _compose(model, img, full_image, origins=((0, 0), (240, 0), (0, 80), (240, 80))):
    """What a user writes by hand today: slice with torch, forward the crops as one batch, forward the whole image, merge on the host."""
    D = model.detections_per_img
    crops = torch.stack([img[:, y:y + 320, x:x + 320] for x, y in origins])
    parts = [[t.cpu().numpy().copy() for t in model.forward_batch(crops)]]
    offsets = [(float(x), float(y)) for x, y in origins]
    if full_image:
        parts.append([t.cpu().numpy().copy() for t in model.forward_batch(img[None])])
        offsets.append((0.0, 0.0))
    b, s, l, c = (np.concatenate([p[i] for p in parts], 0) for i in range(4))
    ob, os_, ol, oc, _, margin = sr.merge_ref(b, s, l, c, np.asarray(offsets, f32), [0, len(offsets)], sr.IOU, model.nms_thresh, 0, D)
    n = int(oc[0])
    return ob[0, :n], os_[0, :n], ol[0, :n], margin, int(c.sum())


def _same(det, boxes, scores, labels):
    return (np.array_equal(det["boxes"].cpu().numpy().view(np.int32), boxes.view(np.int32))
            and np.array_equal(det["scores"].cpu().numpy().view(np.int32), scores.view(np.int32)) and np.array_equal(det["labels"].cpu().numpy(), labels))


@pytest.mark.gpu
@pytest.mark.parametrize("full_image", [True, False])
def test_detect_sliced_equals_the_hand_written_composition(model, full_image):
    img = _image(400, 560)
    assert len(sliced.tile_grid(400, 560, 320, 320, 0.25)[0]) == 4
    boxes, scores, labels, margin, candidates = _compose(model, img, full_image)
    print("candidates", candidates, "kept", len(scores), "margin", margin)
    assert margin > 0 and candidates > len(scores) > 0                            # the input condition of exact equality; and the merge had work
    out = model.detect_sliced(img, full_image=full_image)
    assert len(out) == 1 and len(scores) <= model.detections_per_img
    assert _same(out[0], boxes, scores, labels)
    split = model.detect_sliced([img], full_image=full_image, max_tiles_per_forward=3)      # sub-batches of 3 + 1 tiles
    assert _same(split[0], boxes, scores, labels)


@pytest.mark.gpu
def test_detect_sliced_of_one_tile_is_the_plain_forward(model):
    img = _image(320, 320)
    plain = model([img])[0]
    out = model.detect_sliced(img, full_image=False)[0]
    assert plain["scores"].numel() > 0
    for k in ("boxes", "scores", "labels"):
        assert torch.equal(out[k], plain[k]), k


@pytest.mark.gpu
def test_detect_sliced_list_of_different_sizes_equals_single_calls(model):
    a, b = _image(400, 560), _image(330, 500, seed=IMG_SEED + 1)
    both = model.detect_sliced([a, b])
    one = [model.detect_sliced(a)[0], model.detect_sliced(b)[0]]
    assert len(both) == 2
    for x, y in zip(both, one):
        assert x["scores"].numel() > 0
        for k in ("boxes", "scores", "labels"):
            assert torch.equal(x[k], y[k]), k


@pytest.mark.gpu
def test_detect_sliced_leaves_the_plain_forward_as_it_was(model):
    imgs = [_image(320, 320), _image(300, 420, seed=IMG_SEED + 2)]
    before = model(imgs)
    gen, handle = model._plan_gen, model._handle
    model.detect_sliced(_image(400, 560), metric="ios", class_agnostic=True, merge_thresh=0.3)
    after = model(imgs)
    assert (model._plan_gen, model._handle) == (gen, handle)                      # the plan was not rebuilt
    for x, y in zip(before, after):
        for k in ("boxes", "scores", "labels"):
            assert torch.equal(x[k], y[k]), k


@pytest.mark.gpu
def test_detect_sliced_argument_errors(model):
    img = _image(400, 560)
    for kw in (dict(overlap=1.0), dict(overlap=-0.5), dict(metric="giou"), dict(tile=0), dict(max_tiles_per_forward=0), dict(merge_thresh=float("nan"))):
        with pytest.raises(ValueError):
            model.detect_sliced(img, **kw)
    with pytest.raises(ValueError):
        model.detect_sliced(img[0])                                               # not [3, H, W]
    with pytest.raises(ValueError, match="65536"):
        model.detect_sliced(_image(400, 560), tile=16, overlap=0.0)               # 875 tiles x 300 rows: beyond the merge's slots
    model.train()
    try:
        with pytest.raises(ValueError):
            model.detect_sliced(img)
    finally:
        model.eval()
