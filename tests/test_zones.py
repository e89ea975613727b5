"""Line-crossing and zone analytics behind the tracker (demonet_amd/zones.py, csrc/zones.hip): what can be shown without a GPU.

tests/zones_ref.py restates the rules of include/demonet_hip.h (dn_zone_update) in numpy float32. Here it is pinned by closed forms worked out by
hand, the library's symbols and the struct layout are checked against the header, the host-side refusals are covered, and the scenes the GPU tests
run (tests/test_gpu_zones.py) are shown to produce events of every kind.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import track_ref as tr
import zones_ref as zr
from demonet_amd import _lib
from demonet_amd import zones as dzones

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ("dn_zone_state_bytes", "dn_zone_reset", "dn_zone_update")
W, H = 60.0, 80.0          # a = 0.75: every mean <-> box conversion is exact for integer centres


def table_of(frame, tracks, T=4):
    """One stream's tracker table of a frame: tracks = {slot: dict(id, cx, cy[, state, label, last_frame])}; a track is tracked and seen in
    this frame unless told otherwise."""
    t = dict(frame=np.array([frame], np.int32), state=np.zeros((1, T), np.int32), id=np.zeros((1, T), np.int32), label=np.zeros((1, T), np.int64),
             filter=np.zeros((1, 20, T), f32), last_frame=np.zeros((1, T), np.int32))
    for s, k in tracks.items():
        t["state"][0, s], t["id"][0, s], t["label"][0, s] = k.get("state", 2), k["id"], k.get("label", 1)
        t["last_frame"][0, s] = k.get("last_frame", frame)
        t["filter"][0, 0, s], t["filter"][0, 5, s], t["filter"][0, 10, s], t["filter"][0, 15, s] = k["cx"], k["cy"], W / H, H
    return t


def walk(path, lines=(), zones=(), anchor=0, T=4, max_events=64, class_bin=None, **track):
    """One track with id 1 in slot 0 at the given centres, one per frame -> (state, [events of every frame as tuples])."""
    st = zr.new_state(1, T)
    cfg = [zr.config(lines, zones)]
    log = []
    for i, (cx, cy) in enumerate(path):
        st, ev, n = zr.step(table_of(i + 1, {0: dict(id=1, cx=cx, cy=cy, **track)}, T), cfg, st, class_bin, anchor, max_events)
        log.append([tuple(int(v) for v in r) for r in ev[0, :n[0]]])
    return st, log


SQUARE = [(100, 100), (200, 100), (200, 200), (100, 200)]


# ----------------------------------------------------------------------------------------------------------------------------------
def test_the_three_symbols_are_exported_declared_and_bound_and_the_struct_matches_the_header(tmp_path):
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
    q = L.dn_zone_state_bytes
    q.restype, q.argtypes = C.c_size_t, [C.c_int, C.c_int]
    assert q(1, 256) == 4 * (1156 + 22 * 256) and q(3, 5) == 3 * 4 * (1156 + 22 * 8) and q(64, 1) == 64 * 4 * (1156 + 22 * 4)      # host arithmetic
    assert q(0, 8) == 0 and q(1, 0) == 0 and q(1, 257) == 0
    for T in (1, 5, 256):
        fields = dzones.state_fields(T)
        assert fields["dwell_sum"][0] + 8 * 128 == q(1, T) and fields["dwell_sum"][0] % 8 == 0 and fields["line_count"][0] % 16 == 0
        ends = sorted((off, off + int(np.prod(shape)) * (8 if name == "dwell_sum" else 4)) for name, (off, _, shape) in fields.items())
        assert ends[0][0] == 0 and all(a[1] == b[0] for a, b in zip(ends, ends[1:]))             # the fields tile the block without gaps
    # the struct mirror against the header compiled with gcc
    names = [n for n, _ in _lib.ZoneConfig._fields_]
    src = tmp_path / "zc.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "demonet_hip.h"\nint main(){printf("%zu", sizeof(dn_zone_config));'
                   + "".join('printf(" %zu", offsetof(dn_zone_config, {}));'.format(n) for n in names)
                   + 'printf(" %d %d %d %d", DN_ZONE_CROSS, DN_ZONE_ENTER, DN_ZONE_EXIT, DN_ZONE_VANISH);return 0;}\n')
    exe = tmp_path / "zc"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    n = len(names)
    assert a[0] == C.sizeof(_lib.ZoneConfig) == 2384 and a[0] % 16 == 0
    assert a[1:1 + n] == [getattr(_lib.ZoneConfig, k).offset for k in names] == [0, 4, 260, 264, 328, 2376]
    assert a[1 + n:] == [_lib.DN_ZONE[k] for k in ("cross", "enter", "exit", "vanish")] == [zr.CROSS, zr.ENTER, zr.EXIT, zr.VANISH]
    assert "#define DN_ABI_VERSION 1" in header
    rec = dzones.config_record([(1, 2, 3, 4)], [[(0, 0), (8, 0), (8, 8)]])
    ref = zr.config([(1, 2, 3, 4)], [[(0, 0), (8, 0), (8, 8)]])
    assert rec.n_lines == 1 and rec.n_zones == 1 and list(rec.nv)[:2] == [3, 0]
    assert np.array_equal(np.ctypeslib.as_array(rec.lines), ref["lines"]) and np.array_equal(np.ctypeslib.as_array(rec.verts), ref["verts"])


def test_a_track_walking_straight_through_a_square_zone_enters_once_leaves_once_and_dwells_k_frames():
    """Centres x = 50, 80, ... by 30 a frame at y = 150 through the square 100 .. 200: inside at x = 110, 140, 170 (frames 3, 4, 5), outside again
    at x = 200 exactly (px < 200 is false): entered in frame 3, left in frame 6, dwell 3 = the frames spent inside."""
    st, log = walk([(50 + 30 * i, 150) for i in range(8)], zones=[SQUARE])
    assert [len(e) for e in log] == [0, 0, 1, 0, 0, 1, 0, 0]
    assert log[2] == [(zr.ENTER, 0, 1, 1, 0, 3, 0, 0)] and log[5] == [(zr.EXIT, 0, 1, 1, 0, 6, 3, 0)]
    assert st["entries"][0, 0, 0] == 1 and st["exits"][0, 0, 0] == 1 and st["dwell_sum"][0, 0, 0] == 3 and st["dwell_max"][0, 0, 0] == 3
    assert st["entries"].sum() == 1 and st["exits"].sum() == 1 and not st["vanished"].any() and not st["occupancy"].any()
    # the occupancy while inside, and the first observation inside a zone counts as an entry
    st, log = walk([(150, 150), (150, 150)], zones=[SQUARE])
    assert log[0] == [(zr.ENTER, 0, 1, 1, 0, 1, 0, 0)] and log[1] == [] and st["occupancy"][0, 0, 0] == 1
    # the bottom anchor: the same walk 40 pixels higher gives the same answer
    st, log = walk([(50 + 30 * i, 110) for i in range(8)], zones=[SQUARE], anchor=1)
    assert [len(e) for e in log] == [0, 0, 1, 0, 0, 1, 0, 0] and st["dwell_sum"][0, 0, 0] == 3
    st, log = walk([(50 + 30 * i, 50) for i in range(8)], zones=[SQUARE], anchor=1)      # bottom at y = 90: above the square
    assert not any(log)


def test_a_track_crossing_a_line_and_coming_back_counts_once_in_each_direction():
    """The line (100, 0) -> (100, 300): side = 300 * (px - 100) * -1 ... = -(by - ay) * (px - ax) = -300 (px - 100): >= 0 left of it. Stepping
    from x = 80 to x = 120 ends at side < 0: direction 1; back: direction 0."""
    line = (100, 0, 100, 300)
    st, log = walk([(80, 150), (120, 150), (140, 150), (90, 150)], lines=[line])
    assert log == [[], [(zr.CROSS, 0, 1, 1, 0, 2, 0, 1)], [], [(zr.CROSS, 0, 1, 1, 0, 4, 0, 0)]]
    assert st["line_count"][0, 0].sum(1).tolist() == [1, 1] and st["line_count"].sum() == 2
    # the reversed line reverses the directions
    st, log = walk([(80, 150), (120, 150), (90, 150)], lines=[(100, 300, 100, 0)])
    assert [e[0][7] for e in log[1:]] == [0, 1]
    # a step that ends exactly on the line is on the >= 0 side: from the negative side it crosses, and leaving to the positive side does not again
    st, log = walk([(120, 150), (100, 150), (80, 150)], lines=[line])
    assert [len(e) for e in log] == [0, 1, 0] and log[1][0][7] == 0


def test_a_path_that_rounds_the_end_of_a_line_and_a_stationary_track_cross_nothing():
    line = (100, 100, 100, 200)
    st, log = walk([(90, 210), (110, 210), (110, 90), (90, 90), (90, 150)], lines=[line])      # around both ends: the sides change, the segment is not met
    assert not any(log) and not st["line_count"].any()
    st, log = walk([(100, 150)] * 4 + [(140, 150)] * 3, lines=[line])                            # standing on the line, then standing beside it
    assert [len(e) for e in log] == [0, 0, 0, 0, 1, 0, 0]        # (on the line is the >= 0 side: leaving it to the negative side is the one crossing)
    st, log = walk([(100, 150)] * 2 + [(60, 150)] * 2, lines=[line])                             # ... and leaving it to the >= 0 side is none
    assert not any(log)
    st, log = walk([(60, 150)] * 5, lines=[line])
    assert not any(log)
    # ... and a track that is not observed for a frame keeps its previous anchor: lost on one side, found on the other, it counts
    st = zr.new_state(1, 4)
    cfg = [zr.config([line])]
    seen = []
    for fr, k in enumerate([dict(cx=80, cy=150), dict(cx=80, cy=150, state=3, last_frame=1), dict(cx=130, cy=150)]):
        st, ev, n = zr.step(table_of(fr + 1, {0: dict(id=7, **k)}), cfg, st, None, 0, 8)
        seen.append(int(n[0]))
    assert seen == [0, 0, 1] and tuple(ev[0, 0]) == (zr.CROSS, 0, 7, 1, 0, 3, 0, 1)


def test_a_concave_polygon_and_an_anchor_exactly_on_a_vertex_ray():
    ell = [(0, 0), (300, 0), (300, 100), (100, 100), (100, 300), (0, 300)]          # an L: the notch 100 .. 300 x 100 .. 300 is outside
    pts = {(50, 50): True, (250, 50): True, (50, 250): True, (200, 200): False, (150, 150): False, (350, 50): False, (99, 299): True, (100, 200): False}
    for (x, y), want in pts.items():
        assert zr.inside(zr.config(zones=[ell])["verts"][0], 6, f32(x), f32(y)) == want, (x, y)
    # a diamond: the ray to the right of (100, 100) runs exactly through the vertex (150, 100), that of (20, 100) through two vertices. The rule
    # (yi > py) != (yj > py) gives a vertex on the ray to exactly one of its two edges when they lie on different sides and to both or none
    # otherwise: one toggle at (150, 100) -- inside --, two toggles for (20, 100) -- outside.
    dia = zr.config(zones=[[(100, 50), (150, 100), (100, 150), (50, 100)]])["verts"][0]
    assert zr.inside(dia, 4, f32(100), f32(100)) and not zr.inside(dia, 4, f32(20), f32(100)) and not zr.inside(dia, 4, f32(160), f32(100))
    assert not zr.inside(dia, 4, f32(100), f32(50)) and not zr.inside(dia, 4, f32(100), f32(150))      # the top and the bottom vertex themselves
    # a vertex on the ray whose two edges lie on the same side (a spike touching the ray from above) toggles twice or not at all
    spike = zr.config(zones=[[(0, 0), (200, 0), (200, 100), (150, 50), (100, 100), (0, 100)]])["verts"][0]
    assert zr.inside(spike, 6, f32(50), f32(50)) and zr.inside(spike, 6, f32(120), f32(50)) and not zr.inside(spike, 6, f32(150), f32(60))
    st, log = walk([(100, 100), (20, 100)], zones=[[(100, 50), (150, 100), (100, 150), (50, 100)]])
    assert [e[0][0] for e in log] == [zr.ENTER, zr.EXIT]


def test_closing_an_entry_ignored_classes_tentative_tracks_and_the_event_limit():
    cfg = [zr.config([(100, 0, 100, 300)], [SQUARE, [(0, 0), (400, 0), (400, 400), (0, 400)]])]
    st = zr.new_state(1, 4)
    st, ev, n = zr.step(table_of(1, {0: dict(id=1, cx=80, cy=150), 1: dict(id=2, cx=150, cy=150, label=2)}), cfg, st, None, 0, 8)
    assert [tuple(r[:3]) for r in ev[0, :n[0]]] == [(zr.ENTER, 1, 1), (zr.ENTER, 0, 2), (zr.ENTER, 1, 2)]
    # frame 4: slot 0 holds another track beyond the line, slot 1 is free. No crossing from the old position; VANISH first, slot by slot
    st, ev, n = zr.step(table_of(4, {0: dict(id=3, cx=150, cy=150, label=4)}), cfg, st, None, 0, 8)
    assert [tuple(int(v) for v in r) for r in ev[0, :n[0]]] == [(zr.VANISH, 1, 1, -1, 0, 4, 3, 0), (zr.ENTER, 0, 3, 4, 0, 4, 0, 0), (zr.ENTER, 1, 3, 4, 0, 4, 0, 0),
                                                              (zr.VANISH, 0, 2, -1, 0, 4, 3, 0), (zr.VANISH, 1, 2, -1, 0, 4, 3, 0)]
    assert st["vanished"][0, :2, 0].tolist() == [1, 2] and not st["line_count"].any() and st["id"][0].tolist() == [3, 0, 0, 0]
    assert st["occupancy"][0, :2, 0].tolist() == [1, 1] and not st["exits"].any() and not st["dwell_sum"].any()
    # the event limit: the first max_events in order, the excess counted
    full = zr.step(table_of(1, {s: dict(id=s + 1, cx=150, cy=150) for s in range(4)}), cfg, zr.new_state(1, 4), None, 0, 64)
    cut = zr.step(table_of(1, {s: dict(id=s + 1, cx=150, cy=150) for s in range(4)}), cfg, zr.new_state(1, 4), None, 0, 5)
    assert full[2][0] == 8 and cut[2][0] == 5 and cut[0]["events_dropped"][0] == 3 and np.array_equal(cut[1][0], full[1][0, :5])
    assert all(np.array_equal(full[0][k], cut[0][k]) for k in zr.FIELDS if k != "events_dropped")      # the counters do not depend on the limit
    # a class map: label 3 ignored, label 9 beyond the map ignored, label 2 in bin 1; a tentative track is not observed
    bins = [255, 0, 1, 255]
    tracks = {0: dict(id=1, cx=150, cy=150, label=3), 1: dict(id=2, cx=150, cy=150, label=9), 2: dict(id=3, cx=150, cy=150, label=2),
              3: dict(id=4, cx=150, cy=150, label=1, state=1)}
    st, ev, n = zr.step(table_of(1, tracks), cfg, zr.new_state(1, 4), bins, 0, 8)
    assert n[0] == 2 and [int(r[4]) for r in ev[0, :2]] == [1, 1] and st["entries"][0, :2].sum(0).tolist() == [0, 2, 0, 0, 0, 0, 0, 0]
    assert st["id"][0].tolist() == [1, 2, 3, 4] and st["has_prev"][0].tolist() == [0, 0, 1, 0]
    # a filter mean that is not finite: not observed
    t = table_of(1, {0: dict(id=1, cx=np.nan, cy=150), 1: dict(id=2, cx=150, cy=np.inf)})
    st, ev, n = zr.step(t, cfg, zr.new_state(1, 4), None, 1, 8)
    assert n[0] == 0 and not st["has_prev"].any() and st["id"][0].tolist() == [1, 2, 0, 0]


def test_host_side_refusals():
    ok_line, ok_zone = (0, 0, 10, 10), [(0, 0), (10, 0), (10, 10)]
    dzones.config_record([ok_line] * 16, [ok_zone] * 16)
    dzones.config_record([], [[(i, i * i) for i in range(16)]])
    for lines, zones in (([ok_line] * 17, []), ([], [ok_zone] * 17), ([(0, 0, 0, 0)], []), ([(1.5, 2, 1.5, 2)], []), ([(0, 0, float("nan"), 1)], []),
                         ([(0, 0, float("inf"), 1)], []), ([(0, 0, 1)], []), ([], [ok_zone[:2]]), ([], [[(i, i * i) for i in range(17)]]),
                         ([], [[(0, 0), (1, float("nan")), (2, 2)]]), ([], [[(0, 0), (1, 1, 1), (2, 2)]]), ([("a", 0, 1, 1)], []),
                         ([(0, 0, 1e-46, 0)], [])):          # (the two ends coincide once rounded to float32)
        with pytest.raises(ValueError):
            dzones.config_record(lines, zones)
    with pytest.raises(ValueError):
        dzones.ZoneAnalytics(object())
    with pytest.raises(ValueError):
        dzones.check_analytics(object(), None, "track")
    dzones.check_analytics(None, None, "track")


@pytest.mark.parametrize("case", range(len(zr.SCENE_CASES)))
def test_the_scenes_of_the_gpu_tests_produce_at_least_five_events_of_every_kind(case):
    """The input condition of tests/test_gpu_zones.py::test_scenes_bit_for_bit: a comparison of empty event lists would show nothing."""
    T, anchor, bins = zr.SCENE_CASES[case]
    B = zr.SCENE_STREAMS
    tracker = tr.RefTracker(B, T, track_buffer=zr.SCENE_TRACK_BUFFER)
    st = zr.new_state(B, T)
    cfg = [zr.config(zr.SCENE_LINES, zr.SCENE_ZONES)] * B
    total = dict(cross0=0, cross1=0, enter=0, exit=0, vanish=0)
    for fr in zr.scene_frames():
        tracker.update(*fr)
        st, ev, n = zr.step(tracker.table(), cfg, st, bins, anchor, 256)
        for k, v in zr.event_census(ev, n).items():
            total[k] += v
    print(zr.SCENE_CASES[case], total)
    assert all(v >= 5 for v in total.values()), total
    assert st["events_dropped"].sum() == 0 and st["line_count"].sum() == total["cross0"] + total["cross1"]
    assert st["entries"].sum() == total["enter"] and st["exits"].sum() == total["exit"] and st["vanished"].sum() == total["vanish"]
    if bins is not None:
        assert st["entries"][:, :, 0].sum() > 0 and st["entries"][:, :, 1].sum() > 0 and not st["entries"][:, :, 2:].any()
