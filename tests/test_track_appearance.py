"""Appearance association in the tracker, without a GPU (demonet_amd/track.py AppearanceTracker, csrc/trackapp.hip).

tests/track_appearance_ref.py restates include/demonet_hip.h (dn_track_update_appearance) on top of tests/track_ref.py. Here it is pinned by
closed forms of the fused pair value worked out by hand, by scenes built so that one rule decides them (a crossing that plain ByteTrack gets
wrong, a lost track found again without overlap, e exactly at its threshold, a low-score row), by four planted defects, and by its equality
with RefTracker when there are no embeddings. The C entry points refuse bad arguments before anything is enqueued, so every refusal is
exercised here, with made-up addresses. tests/test_gpu_track_appearance.py holds the device to the reference.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import track_appearance_ref as ar
import track_ref as tr
from demonet_amd import _lib, models
from demonet_amd import track as dtrack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ("dn_track_feature_bytes", "dn_track_appearance_workspace_bytes", "dn_track_feature_reset", "dn_track_update_appearance")
DN_E_INVALID, DN_E_UNSUPPORTED, DN_E_WORKSPACE = -1, -4, -3


def _library():
    if not os.path.exists(_lib.LIB_PATH):
        from demonet_amd import build
        build.build(verbose=False)
    return _lib.lib()


def test_the_symbols_are_exported_declared_and_bound_and_the_struct_mirror_matches_gcc(tmp_path):
    L = _library()
    header = open(os.path.join(ROOT, "include", "demonet_hip.h")).read()
    declared = set(re.findall(r"DN_API\s+[\w\s\*]+?\b(dn_\w+)\s*\(", header))
    assert set(NAMES) <= set(_lib.EXPORTS)
    for n in NAMES:
        assert hasattr(L, n) and n in declared, n
    codes = dict(re.findall(r"(DN_E_\w+)\s*=\s*(-?\d+)", header))
    assert (int(codes["DN_E_INVALID"]), int(codes["DN_E_UNSUPPORTED"]), int(codes["DN_E_WORKSPACE"])) == (DN_E_INVALID, DN_E_UNSUPPORTED, DN_E_WORKSPACE)
    names = [n for n, _ in _lib.TrackAppearanceParams._fields_]
    src = tmp_path / "ap.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "demonet_hip.h"\nint main(){printf("%zu %zu", sizeof(dn_track_appearance_params), '
                   'sizeof(dn_track_params));' + "".join('printf(" %zu", offsetof(dn_track_appearance_params, {}));'.format(n) for n in names)
                   + "return 0;}\n")
    exe = tmp_path / "ap"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert a[0] == C.sizeof(_lib.TrackAppearanceParams) == 32
    assert a[1] == C.sizeof(_lib.TrackParams) == 40                       # dn_track_params is untouched
    assert a[2:] == [getattr(_lib.TrackAppearanceParams, n).offset for n in names]
    assert "static_assert(sizeof(dn_track_appearance_params) == 32" in header


def test_buffer_sizes_are_host_arithmetic_and_match_the_python_layout():
    L = _library()
    fb, wb = L.dn_track_feature_bytes, L.dn_track_appearance_workspace_bytes
    assert fb(1, 256, 512) == 256 * 4 * (1 + 512) and fb(3, 5, 32) == 3 * 8 * 4 * 33 and fb(64, 1, 64) == 64 * 4 * 4 * 65
    for bad in ((0, 4, 32), (1, 0, 32), (1, 257, 32), (1, 4, 0), (1, 4, 48), (1, 4, 544), (1, 4, 31)):
        assert fb(*bad) == 0, bad
    up = lambda v: (v + 15) & ~15
    for B, T, d, E, dim in ((1, 1, 1, 1, 32), (3, 5, 7, 3, 96), (64, 256, 160, 8192, 256), (2, 17, 512, 5, 512)):
        tp = (T + 3) & ~3
        want = up(E * dim * 2) + up(E * 4) + up(B * d * 4) + B * tp * d * 4
        assert wb(B, T, d, E, dim) == want
        fields = dtrack.workspace_fields(B, T, d, E, dim)
        assert fields["total"][0] == want and fields["S"][0] + B * tp * d * 4 == want and fields["S"][2] == (B, tp, d)
        assert all(off % 16 == 0 for off, _, _ in fields.values())
    for bad in ((0, 4, 8, 1, 32), (1, 257, 8, 1, 32), (1, 4, 0, 1, 32), (1, 4, 513, 1, 32), (1, 4, 8, 0, 32), (1, 4, 8, 8193, 32), (1, 4, 8, 1, 40)):
        assert wb(*bad) == 0, bad
    # the tracker's own state block does not grow by a byte
    assert L.dn_track_state_bytes(3, 5) == 3 * (16 + 112 * 8)


def _call(L, params=None, app=None, **kw):
    """dn_track_update_appearance on made-up, suitably aligned addresses: only for calls that must be refused before anything is enqueued."""
    a = dict(boxes=0x10000, scores=0x20000, labels=0x30000, counts=0x40000, streams=2, d=8, emb=0x50000, index=0x60000, E=4, state=0x70000,
             state_bytes=None, features=0x80000, feature_bytes=None, workspace=0x90000, workspace_bytes=None, outs=[0xA0000 + 0x1000 * i for i in range(7)])
    a.update(kw)
    p = params if params is not None else _lib.TrackParams(0.5, 0.1, 0.6, 0.8, 0.5, 0.7, 30, 0, 4, 0)
    q = app if app is not None else _lib.TrackAppearanceParams(dim=64, alpha=0.9, appearance_thresh=0.25, proximity_thresh=0.5, emb_fp16=0)
    if a["state_bytes"] is None:
        a["state_bytes"] = 2 * (16 + 112 * 4)
    if a["feature_bytes"] is None:
        a["feature_bytes"] = 2 * 4 * 4 * 65
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = 1 << 20
    v = C.c_void_p
    return L.dn_track_update_appearance(v(a["boxes"]), v(a["scores"]), v(a["labels"]), v(a["counts"]), a["streams"], a["d"], C.byref(p) if p else None,
                                        C.byref(q) if q else None, v(a["emb"]), v(a["index"]), a["E"], v(a["state"]), a["state_bytes"], v(a["features"]),
                                        a["feature_bytes"], v(a["workspace"]), a["workspace_bytes"], *[v(o) for o in a["outs"]], None)


def _app(**kw):
    base = dict(dim=64, alpha=0.9, appearance_thresh=0.25, proximity_thresh=0.5, emb_fp16=0)
    base.update(kw)
    return _lib.TrackAppearanceParams(**base)


REFUSALS = [
    ("null features", dict(features=0), None, DN_E_INVALID),
    ("null embeddings with E > 0", dict(emb=0), None, DN_E_INVALID),
    ("null index with E > 0", dict(index=0), None, DN_E_INVALID),
    ("null workspace with E > 0", dict(workspace=0), None, DN_E_INVALID),
    ("embeddings with E = 0", dict(E=0, index=0), None, DN_E_INVALID),
    ("negative E", dict(E=-1), None, DN_E_INVALID),
    ("null boxes", dict(boxes=0), None, DN_E_INVALID),
    ("streams 0", dict(streams=0), None, DN_E_INVALID),
    ("misaligned embeddings", dict(emb=0x50004), None, DN_E_INVALID),
    ("misaligned index", dict(index=0x60008), None, DN_E_INVALID),
    ("misaligned features", dict(features=0x80004), None, DN_E_INVALID),
    ("misaligned workspace", dict(workspace=0x90008), None, DN_E_INVALID),
    ("misaligned state", dict(state=0x70008), None, DN_E_INVALID),
    ("dim 0", {}, dict(dim=0), DN_E_INVALID),
    ("alpha NaN", {}, dict(alpha=float("nan")), DN_E_INVALID),
    ("alpha above 1", {}, dict(alpha=1.5), DN_E_INVALID),
    ("alpha negative", {}, dict(alpha=-0.1), DN_E_INVALID),
    ("appearance_thresh NaN", {}, dict(appearance_thresh=float("nan")), DN_E_INVALID),
    ("proximity_thresh negative", {}, dict(proximity_thresh=-1.0), DN_E_INVALID),
    ("emb_fp16 2", {}, dict(emb_fp16=2), DN_E_INVALID),
    ("reserved", {}, dict(reserved=(C.c_int32 * 3)(0, 1, 0)), DN_E_INVALID),
    ("dim 48", {}, dict(dim=48), DN_E_UNSUPPORTED),
    ("dim 544", {}, dict(dim=544), DN_E_UNSUPPORTED),
    ("E 8193", dict(E=8193), None, DN_E_UNSUPPORTED),
    ("d 513", dict(d=513), None, DN_E_UNSUPPORTED),
    ("small state", dict(state_bytes=2 * (16 + 112 * 4) - 1), None, DN_E_WORKSPACE),
    ("small features", dict(feature_bytes=2 * 4 * 4 * 65 - 1), None, DN_E_WORKSPACE),
    ("small workspace", dict(workspace_bytes=4 * 64 * 2 + 16 + 2 * 8 * 4 + 2 * 4 * 8 * 4 - 1), None, DN_E_WORKSPACE),
]


@pytest.mark.parametrize("what,kw,app,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_step_refuses_before_anything_is_enqueued(what, kw, app, code):
    """Every refusal comes back with its code and a dn_last_error text that names the entry point; the addresses are made up, so a call that got
    as far as a launch would not come back at all."""
    L = _library()
    rc = _call(L, app=_app(**app) if app else None, **kw)
    assert rc == code, (what, rc)
    assert L.dn_last_error().decode().startswith("dn_track_update_appearance:"), L.dn_last_error()


def test_the_other_entry_points_and_the_python_layer_refuse_without_a_device():
    L = _library()
    v = C.c_void_p
    assert L.dn_track_feature_reset(v(0), 2, 4, 64, None, None) == DN_E_INVALID
    assert L.dn_track_feature_reset(v(0x1008), 2, 4, 64, None, None) == DN_E_INVALID
    assert L.dn_track_feature_reset(v(0x1000), 0, 4, 64, None, None) == DN_E_INVALID
    assert L.dn_track_feature_reset(v(0x1000), 2, 4, 48, None, None) == DN_E_UNSUPPORTED
    assert L.dn_track_feature_reset(v(0x1000), 2, 257, 64, None, None) == DN_E_UNSUPPORTED
    assert L.dn_last_error().decode().startswith("dn_track_feature_reset:")
    _call(L, params=_lib.TrackParams(0.5, 0.1, 0.6, 1.5, 0.5, 0.7, 30, 0, 4, 0))
    assert "dn_track_update_appearance: match_thresh" in L.dn_last_error().decode()        # dn_track_update's checks, under this entry's name
    with pytest.raises(RuntimeError):
        dtrack.AppearanceTracker(2, "cpu", 64)
    for kw in (dict(dim=0), dict(dim=48), dict(dim=544), dict(dim=64.0), dict(alpha=float("nan")), dict(alpha=1.5), dict(alpha=-0.5),
               dict(appearance_thresh=-0.1), dict(appearance_thresh=float("nan")), dict(proximity_thresh=-1.0), dict(streams=0), dict(max_tracks=257),
               dict(match_thresh=1.5), dict(track_buffer=-1)):
        args = dict(streams=2, device="cuda", dim=64)
        args.update(kw)
        with pytest.raises(ValueError):
            dtrack.AppearanceTracker(**args)
    assert issubclass(dtrack.AppearanceTracker, dtrack.ByteTracker)
    m = models.ssdlite320_mobilenet_v3_large(num_classes=3)
    with pytest.raises(ValueError):
        m.track_frames_appearance(None, object(), None, lambda x: x)
    m.train()
    with pytest.raises(ValueError):
        m.track_frames_appearance(None, None, None, None)


# ----------------------------------------------------------------------------------------------------------------------------------
# the fused value, by hand
# ----------------------------------------------------------------------------------------------------------------------------------
def test_closed_forms_of_the_fused_value():
    at, pt = f32(0.25), f32(0.5)
    F = lambda u, s, a=at, p=pt: ar.fused(f32(u), f32(s), a, p)
    # S = 0.75: e = 0.125 <= 0.25; u = 0.625: 1 - u = 0.375 <= 0.5 -> admissible, v = max(0.625, 0.875)
    assert F(0.625, 0.75) == f32(0.875)
    # ... and the IoU wins when it is the larger: S = 0.5 -> e = 0.25, 1 - e = 0.75 < u = 0.875
    assert F(0.875, 0.5) == f32(0.875)
    # e exactly AT the appearance threshold is admissible (S = 0.5 -> e = 0.25), just above it is not
    assert F(0.625, 0.5) == f32(0.75)
    assert F(0.625, 0.5 - 2.0 ** -20) == f32(0.625)                  # e = 0.25 + 2^-21, exact in fp32
    # 1 - u exactly AT the proximity threshold is admissible (u = 0.5), just beyond it is not
    assert F(0.5, 0.75) == f32(0.875)
    assert F(0.5 - 2.0 ** -20, 0.75) == f32(0.5 - 2.0 ** -20)         # 1 - u = 0.5 + 2^-20, exact in fp32
    # no overlap: admissible only with proximity_thresh = 1
    assert F(0.0, 1.0) == f32(0) and F(0.0, 1.0, at, f32(1)) == f32(1)
    # S slightly above 1 (fp16 operands, fp32 sum): e is clamped at 0, v = 1 exactly, never above
    assert F(0.625, 1.0 + 2.0 ** -10) == f32(1) and F(0.625, 1.5) == f32(1)
    # a NaN S is never admissible; a NaN u stays a NaN (and passes no gate)
    assert F(0.625, np.nan) == f32(0.625)
    assert np.isnan(F(np.nan, 1.0))
    # S = -1 (opposite): e = 1 > any sensible threshold
    assert F(0.625, -1.0) == f32(0.625)
    # the planted deviations move exactly the equalities
    assert ar.fused(f32(0.625), f32(0.5), at, pt, "lt") == f32(0.625) and ar.fused(f32(0.5), f32(0.75), at, pt, "lt") == f32(0.5)
    assert ar.fused(f32(0.0), f32(1.0), at, pt, "no_proximity") == f32(1)


def test_normalise_and_the_row_map():
    x = np.zeros((6, 32), f32)
    x[0, :4] = (3, 0, 4, 0)
    x[1, 0] = np.nan
    x[2, 5] = np.inf
    x[4, :] = 1e-30                                  # the squares underflow: norm 0
    x[5, :] = 1e30                                   # the squares overflow: norm inf
    ok, en = ar.normalise(x)
    assert ok.tolist() == [True, False, False, False, False, False]
    assert en[0, :4].astype(f32).tolist() == [f32(np.float16(0.6)), 0, f32(np.float16(0.8)), 0] and not en[1:].any()
    index = np.zeros((6, 8), np.int32)
    index[:, 0] = (0, 0, 1, -1, 2, 1)
    index[:, 1] = (1, 1, 0, 0, 0, 3)
    m = ar.row_map(index, np.array([2, 3], np.int32), 2, 4)
    assert m.tolist() == [[-1, 1, -1, -1], [2, -1, -1, -1]]        # slot 1 beats slot 0; stream -1, stream 2 and row 3 >= count 3 are ignored
    assert ar.row_map(index, np.array([2 ** 31 - 1, -5], np.int32), 2, 4).tolist() == [[-1, 1, -1, -1], [-1, -1, -1, -1]]


# ----------------------------------------------------------------------------------------------------------------------------------
# scenes
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes():
    return ar.scene_set()


@pytest.fixture(scope="module")
def good(scenes):
    return {name: ar.run(*sc) for name, sc in scenes.items()}


def test_the_crossing_scene_swaps_ids_without_appearance_and_keeps_them_with_it(scenes, good):
    B, T, dim, kw, frames, embs = scenes["crossing"]
    assert np.array_equal(frames[10][0][0, 0], frames[10][0][0, 1])                      # the boxes coincide at the crossing
    a, b = embs[0][0].astype(np.float64)
    assert abs(a @ b) / (np.linalg.norm(a) * np.linalg.norm(b)) < 0.11                   # near-orthogonal
    plain = tr.RefTracker(B, T)
    ids = [plain.update(*fr)[6][0, :2].tolist() for fr in frames]
    assert ids[:11] == [[1, 2]] * 11 and ids[11:] == [[2, 1]] * 13                       # IoU alone: the ids swap after the crossing
    t, outs = good["crossing"]
    assert [o[6][0, :2].tolist() for o in outs] == [[1, 2]] * 24                         # with appearance every row keeps its id
    assert t.fvalid[0].tolist() == [True, True, False, False] and t.next_id[0] == 3


def test_a_lost_track_is_found_again_without_overlap_only_with_proximity_1(good):
    t1, o1 = good["refind_prox1"]
    t5, o5 = good["refind_prox05"]
    assert [int(o[6][0, 0]) for o in o1] == [1, 1, 1, -1, -1, -1, 1, 1] and t1.state[0].tolist() == [tr.TRACKED, 0, 0, 0]
    assert [int(o[6][0, 0]) for o in o5] == [1, 1, 1, -1, -1, -1, -1, 2] and t5.state[0].tolist() == [tr.LOST, tr.TRACKED, 0, 0]
    log = [l for l in t1.assoc_log if l["stage"] == 1 and l["rows"] and l["slots"]][-2]      # frame 7: u = 0, v = 1 - e = 1
    assert log["iou"][0, 0] == f32(1) and log["matches"] == [(0, 0)]


def test_e_at_the_threshold_and_stage_2_ignoring_appearance(good):
    t, outs = good["equality"]
    assert [int(o[6][0, 0]) for o in outs] == [1, 1, 1]
    log = [l for l in t.assoc_log if l["stage"] == 1 and l["rows"] and l["slots"]][0]        # frame 2
    assert log["iou"][0, 0] == f32(0.75) and t._S is not None                                # S = 0.5 exactly, e = 0.25, v = 0.75
    t, outs = good["low_row"]
    assert [int(o[6][0, 0]) for o in outs] == [1, -1, -1] and t.state[0, 0] == tr.LOST
    log = [l for l in t.assoc_log if l["stage"] == 2 and l["rows"] and l["slots"]][0]
    assert abs(float(log["iou"][0, 0]) - 1.0 / 3.0) < 1e-6 and log["matches"] == []          # the value is the IoU alone


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("defect,where", [("lt", "equality"), ("no_proximity", "refind_prox05"), ("no_renorm", "random0"), ("stage2_fused", "low_row")])
def test_a_planted_defect_moves_the_result_of_the_scene_set(scenes, good, defect, where):
    """Each deviation changes what the scene set of the GPU association test yields: the table or the outputs for three of them; for the EMA
    without renormalisation the features, by far more than the GPU test's bound on them (about dim * 2^-24)."""
    t, outs = good[where]
    bad, bo = ar.run(*scenes[where], app_defect=defect)
    if defect == "no_renorm":
        both = t.fvalid & bad.fvalid
        assert both.any() and np.abs(t.feat[both].astype(np.float64) - bad.feat[both]).max() > 1e-4
        n = np.linalg.norm(bad.feat[both].astype(np.float64), axis=1)
        assert n.min() < 1 - 1e-4 and np.abs(np.linalg.norm(t.feat[both].astype(np.float64), axis=1) - 1).max() < 1e-6
        return
    same = all(_same(t.table()[k], bad.table()[k]) for k in t.FIELDS) and all(_same(x, y) for a, b in zip(outs, bo) for x, y in zip(a, b))
    assert not same


@pytest.mark.parametrize("seed", [1, 2])
def test_without_embeddings_the_reference_is_reftracker(seed):
    frames, _ = tr.scene(100 + seed, 25, 2, 32, objects=6)
    a = tr.RefTracker(2, 16, track_buffer=3, class_agnostic=bool(seed & 1))
    b = ar.AppRefTracker(2, 64, max_tracks=16, track_buffer=3, class_agnostic=bool(seed & 1))
    garbage = (np.full((3, 64), np.nan, f32), np.full((3, 8), -1, np.int32))
    for i, fr in enumerate(frames):
        wa = a.update(*fr)
        wb = b.update(*fr) if i % 2 else b.update(*fr, emb=garbage[0], index=garbage[1])      # none at all, or none that counts
        assert all(_same(x, y) for x, y in zip(wa, wb)), i
        assert all(_same(a.table()[k], b.table()[k]) for k in a.FIELDS), i
    assert not b.fvalid.any() and a.next_id.min() > 6


def test_the_random_scenes_exercise_what_they_are_meant_to(scenes, good):
    """Matches whose value is the appearance term's (above 0.99: the boxes jitter, an IoU does not get there), rows of objects without an
    embedding, and index rows that name nobody."""
    by_appearance = without = 0
    for name in ("random0", "random1", "random2", "random3"):
        t, _ = good[name]
        B, T, dim, kw, frames, embs = scenes[name]
        for l in t.assoc_log:
            for s, j in l["matches"]:
                by_appearance += int(l["stage"] != 2 and l["iou"][l["slots"].index(s), l["rows"].index(j)] > f32(0.99))
        for fr, (emb, index) in zip(frames, embs):
            named = {(int(r[0]), int(r[1])) for r in index if r[0] >= 0}
            without += sum(1 for b in range(B) for j in range(int(fr[3][b])) if (b, j) not in named)
            assert (index[:, 0] < 0).any()
    assert by_appearance > 50 and without > 50
