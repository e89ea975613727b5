"""ByteTrack on the device (demonet_amd/track.py, csrc/track.hip).

tests/track_ref.py restates include/demonet_hip.h (dn_track_update) in numpy float32. Without a GPU it is pinned by closed forms worked out by hand,
by a float64 restatement of the published 8 x 8 filter applied one step from the float32 state, by scipy's optimal assignment on scenes whose
objects do not compete, and by six planted defects. On the GPU every comparison of the device with it is bit for bit: every output and every
field of the state, after every frame.
"""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import track_ref as tr
from demonet_amd import _lib, models, synth
from demonet_amd import track as dtrack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ("dn_track_state_bytes", "dn_track_reset", "dn_track_update")


def frame_of(rows, d=8, B=1):
    """rows: per stream a list of (box, score, label) -> one frame's padded arrays."""
    if B == 1 and (not rows or not isinstance(rows[0], list)):
        rows = [rows]
    bx, sc, lb, ct = np.zeros((B, d, 4), f32), np.zeros((B, d), f32), np.zeros((B, d), np.int64), np.zeros(B, np.int32)
    for b, rs in enumerate(rows):
        for j, (box, s, l) in enumerate(rs):
            bx[b, j], sc[b, j], lb[b, j] = box, s, l
        ct[b] = len(rs)
    return bx, sc, lb, ct


BOX = (100.0, 100.0, 160.0, 180.0)          # w = 60, h = 80: a = 0.75 and every mean <-> box conversion is exact


def shifted(dx, dy=0.0, box=BOX):
    return (box[0] + dx, box[1] + dy, box[2] + dx, box[3] + dy)


# ----------------------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------------------
def test_the_three_symbols_are_exported_declared_and_bound(tmp_path):
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
    q = L.dn_track_state_bytes
    q.restype, q.argtypes = C.c_size_t, [C.c_int, C.c_int]
    assert q(1, 256) == 16 + 112 * 256 and q(3, 5) == 3 * (16 + 112 * 8) and q(64, 1) == 64 * (16 + 112 * 4)      # pure host arithmetic
    assert q(0, 8) == 0 and q(1, 0) == 0 and q(1, 257) == 0
    fields = dtrack.state_fields(5)
    assert fields["det"][0] + 4 * 8 == q(1, 5)
    # the struct mirror against the header compiled with gcc
    names = [n for n, _ in _lib.TrackParams._fields_]
    src = tmp_path / "tp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "demonet_hip.h"\nint main(){printf("%zu", sizeof(dn_track_params));'
                   + "".join('printf(" %zu", offsetof(dn_track_params, {}));'.format(n) for n in names) + "return 0;}\n")
    exe = tmp_path / "tp"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert a[0] == C.sizeof(_lib.TrackParams)
    assert a[1:] == [getattr(_lib.TrackParams, n).offset for n in names]
    assert "dn_debug_track" not in header and "#define DN_ABI_VERSION 1" in header


def _exact_step(box0, box1):
    """init from box0, predict, update with box1, in exact rational arithmetic with the float32 weights."""
    wp, wv = Fraction(float(tr.WP)), Fraction(float(tr.WV))

    def meas(b):
        b = [Fraction(float(f32(v))) for v in b]
        w, h = b[2] - b[0], b[3] - b[1]
        return [b[0] + w / 2, b[1] + h / 2, w / h, h]
    z0, z1 = meas(box0), meas(box1)
    h = z0[3]
    out = []
    for k in range(4):
        a = k == 2
        x, v = z0[k], Fraction(0)
        pxx = Fraction(float(tr.A_P0)) if a else (2 * wp * h) ** 2
        pvv = Fraction(float(tr.A_V0)) if a else (10 * wv * h) ** 2
        pxv = Fraction(0)
        qp = Fraction(float(tr.A_QP)) if a else (wp * h) ** 2
        qv = Fraction(float(tr.A_QV)) if a else (wv * h) ** 2
        x, pxx, pxv, pvv = x + v, pxx + 2 * pxv + pvv + qp, pxv + pvv, pvv + qv
        out.append([x, v, pxx, pxv, pvv])
    hp = out[3][0]
    for k in range(4):
        x, v, pxx, pxv, pvv = out[k]
        r = Fraction(float(tr.A_R)) if k == 2 else (wp * hp) ** 2
        S = pxx + r
        kx, kv = pxx / S, pxv / S
        y = z1[k] - x
        out[k] = [x + kx * y, v + kv * y, pxx - kx * S * kx, pxv - kx * S * kv, pvv - kv * S * kv]
    return [float(v) for row in out for v in row]


def test_one_object_seen_in_frames_1_to_3():
    """An object present from a stream's first frame is confirmed at once with id 1; the same object behind one empty frame is tentative first and
    confirmed by its second detection. After init, one predict and one update the 20 filter floats equal the exact rational result within 2^-17
    relative: each value is the end of at most 12 float32 operations of 2^-24 each, and the only cancelling step, P - (k S) k = P (1 - k),
    magnifies what it is given by 1 / (1 - k): after init and one predict Pxx = (4 / 400 + 1 / 256 + 1 / 400) h^2 = 6.56 r with r = h^2 / 400, so
    k = 0.868 and 1 / (1 - k) < 7.6: 12 x 7.6 x 2^-24 < 2^-17."""
    boxes = [BOX, shifted(4, 2, (100.0, 100.0, 161.0, 182.0)), shifted(8, 4)]
    t = tr.RefTracker(1, 4)
    for i, bx in enumerate(boxes):
        out = t.update(*frame_of([(bx, 0.9, 3)]))
        assert t.state[0].tolist() == [tr.TRACKED, 0, 0, 0] and t.id[0, 0] == 1 and t.next_id[0] == 2 and t.frame[0] == i + 1
        assert out[5][0] == 1 and out[3][0, 0] == 1 and out[4][0, 0] == 0 and out[2][0, 0] == 3 and out[6][0, 0] == 1
        if i == 0:
            assert out[0][0, 0].tolist() == list(BOX)                   # (exact: a = 0.75)
        if i == 1:
            want = np.array(_exact_step(boxes[0], boxes[1]))
            got = t.filter[0, :, 0].astype(np.float64)
            assert np.all(np.abs(got - want) <= 2.0 ** -17 * np.abs(want)), np.max(np.abs(got - want) / np.abs(want))
            assert 100.0 < out[0][0, 0, 0] < 104.0                      # the filtered box lies between the prediction and the measurement
    t = tr.RefTracker(1, 4)
    seq = []
    for rows in ([], [(BOX, 0.9, 3)], [(shifted(3), 0.9, 3)], [(shifted(6), 0.9, 3)]):
        out = t.update(*frame_of(rows))
        seq.append((int(t.state[0, 0]), int(out[5][0]), int(out[6][0, 0])))
    assert seq == [(tr.FREE, 0, -1), (tr.TENTATIVE, 0, -1), (tr.TRACKED, 1, 1), (tr.TRACKED, 1, 1)]
    assert t.start_frame[0, 0] == 2 and t.last_frame[0, 0] == 4 and t.id[0, 0] == 1


def test_lost_and_found_with_the_same_id_and_removed_after_track_buffer_exactly():
    t = tr.RefTracker(1, 4, track_buffer=3)
    t.update(*frame_of([(BOX, 0.9, 1)]))
    t.update(*frame_of([(BOX, 0.9, 1)]))                # frame 2: last_frame = 2
    for fr in (3, 4, 5):
        out = t.update(*frame_of([]))
        assert t.state[0, 0] == tr.LOST and out[5][0] == 0 and t.frame[0] == fr      # 5 - 2 = 3 is not > 3
    u = tr.RefTracker(1, 4, track_buffer=3)
    u.__dict__.update({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in t.__dict__.items()})
    out = u.update(*frame_of([(BOX, 0.9, 1)]))          # found again in frame 6
    assert u.state[0, 0] == tr.TRACKED and out[3][0, 0] == 1 and out[5][0] == 1 and u.next_id[0] == 2
    out = t.update(*frame_of([]))                       # frame 6: 6 - 2 > 3
    assert t.state[0, 0] == tr.FREE and not t.filter[0].any() and t.id[0, 0] == 0 and t.det[0, 0] == 0
    out = t.update(*frame_of([(BOX, 0.9, 1)]))          # the same object now starts a new track
    assert t.state[0, 0] == tr.TENTATIVE and t.id[0, 0] == 2


def test_an_iou_equal_to_the_gate_does_not_match():
    """match_thresh = 0.5: the gate is 0.5 exactly, and the lower half of the box has IoU 2400 / 4800 = 0.5 exactly with it."""
    half = (100.0, 100.0, 160.0, 140.0)
    t = tr.RefTracker(1, 4, match_thresh=0.5)
    t.update(*frame_of([(BOX, 0.9, 1)]))
    t.update(*frame_of([(half, 0.9, 1)]))
    assert t.assoc_log[-3]["iou"][0, 0] == f32(0.5) and t.assoc_log[-3]["matches"] == []
    assert t.state[0].tolist()[:2] == [tr.LOST, tr.TENTATIVE] and t.id[0].tolist()[:2] == [1, 2]
    g = tr.RefTracker(1, 4, match_thresh=0.5, defect="ge")
    g.update(*frame_of([(BOX, 0.9, 1)]))
    g.update(*frame_of([(half, 0.9, 1)]))
    assert g.state[0].tolist()[:2] == [tr.TRACKED, tr.FREE]


def test_a_low_score_detection_rescues_a_tracked_track_but_not_a_lost_one():
    t = tr.RefTracker(1, 4)
    t.update(*frame_of([(BOX, 0.9, 1)]))
    out = t.update(*frame_of([(BOX, 0.3, 1)]))           # tracked: stage 2 takes the low row
    assert t.state[0, 0] == tr.TRACKED and out[5][0] == 1 and out[1][0, 0] == f32(0.3) and out[6][0, 0] == 1
    t.update(*frame_of([]))
    assert t.state[0, 0] == tr.LOST
    out = t.update(*frame_of([(BOX, 0.3, 1)]))           # lost: the low row is not offered to it, and a low row starts nothing
    assert t.state[0, 0] == tr.LOST and out[5][0] == 0 and out[6][0, 0] == -1 and t.next_id[0] == 2
    out = t.update(*frame_of([(BOX, 0.05, 1)]))          # below low_thresh: nobody's
    assert out[5][0] == 0
    out = t.update(*frame_of([(BOX, 0.55, 1)]))          # high, but a lost track is in stage 1
    assert t.state[0, 0] == tr.TRACKED and out[3][0, 0] == 1


def test_the_frame_1_rule_new_thresh_and_the_slot_overflow_counter():
    far = [shifted(100.0 * i) for i in range(4)]
    t = tr.RefTracker(1, 2)
    out = t.update(*frame_of([(far[0], 0.9, 1), (far[1], 0.55, 1), (far[2], 0.7, 2), (far[3], 0.8, 1)]))
    # row 1 is high but below new_thresh = 0.6: it starts nothing and is not counted; rows 0 and 2 take the two slots; row 3 is dropped
    assert t.state[0].tolist() == [tr.TRACKED, tr.TRACKED] and t.id[0].tolist() == [1, 2] and t.label[0].tolist() == [1, 2]
    assert t.dropped[0] == 1 and t.next_id[0] == 3 and out[5][0] == 2 and out[6][0, :4].tolist() == [1, -1, 2, -1] and out[4][0].tolist() == [0, 2]
    out = t.update(*frame_of([(far[0], 0.9, 1), (far[3], 0.8, 1)]))
    assert t.dropped[0] == 2 and t.state[0].tolist() == [tr.TRACKED, tr.LOST]
    t = tr.RefTracker(1, 4)
    t.update(*frame_of([(far[0], 0.9, 1)]))
    t.update(*frame_of([(far[0], 0.9, 1), (far[2], 0.9, 1)]))
    assert t.state[0].tolist()[:2] == [tr.TRACKED, tr.TENTATIVE]          # after frame 1 a new track is tentative


def _slots(t, b=0):
    return {int(t.id[b, s]): s for s in range(t.T) if t.state[b, s] != tr.FREE}


def test_the_float32_filter_agrees_with_the_published_8x8_filter_one_step_at_a_time():
    """From the float32 state before each predict and each update of a 40-frame scene, the published filter in float64 with the full 8 x 8
    matrices gives what the float32 arithmetic gives, within a bound counted from the operations (eps = 2^-24, one rounding each):
      predict: x + v: 1 op; Pxx: 2 (weight, square) for q and 3 additions of non-negative terms: 5 eps relative; Pxv 1; Pvv 3.
      update: S 3 ops (r 2, sum 1); k 1 more: 4; k y: 6 (y itself 1, absolute eps |z| + eps |x|); P - (k S) k: the products carry 4 + 1 + 4 + 1 = 10 eps
      of P k <= P, the difference 1 more: absolute 11 eps P.
    So: means within 8 eps (|x| + |z| + |v|), covariance entries within 12 eps of sqrt(Pii Pjj) of the state before the step (which dominates every
    term). The entries outside the four 2 x 2 blocks are exactly 0 in float64: the block-diagonal argument of the header."""
    eps = 2.0 ** -24
    frames, _ = tr.scene(11, 40, 1, 16, separated=True)
    t = tr.RefTracker(1, 16)
    block = np.zeros((8, 8), bool)
    for k in range(4):
        block[np.ix_([k, 4 + k], [k, 4 + k])] = True
    checked = 0
    for bx, sc, lb, ct in frames:
        pre = t.filter[0].copy()
        state = t.state[0].copy()
        t.update(bx, sc, lb, ct)
        for s in range(t.T):
            if state[s] == tr.FREE or t.state[0, s] == tr.FREE:
                continue
            f = pre[:, s].copy()
            if state[s] in (tr.TRACKED, tr.LOST):
                if state[s] == tr.LOST:
                    f[16] = 0
                m, P = tr.predict64(*tr.to64(f))
                g = tr.kf_predict(f)
                gm, gP = tr.to64(g)
                scale = np.sqrt(np.outer(np.diag(P), np.diag(P)))
                assert np.all(np.abs(gm - m) <= 8 * eps * (np.abs(m) + np.abs(tr.to64(f)[0]))), (gm - m)
                assert np.all(np.abs(gP - P) <= 12 * eps * scale)
                assert not P[~block].any()
                f = g
                checked += 1
            if t.last_frame[0, s] == t.frame[0] and t.start_frame[0, s] != t.frame[0]:
                z = tr.measure(bx[0, t.det[0, s]]).astype(np.float64)
                m0, P0 = tr.to64(f)
                m, P = tr.update64(m0, P0, z)
                gm, gP = tr.to64(t.filter[0, :, s])
                assert np.array_equal(tr.kf_update(f, bx[0, t.det[0, s]]), t.filter[0, :, s])
                zz = np.concatenate([np.abs(z), np.abs(z)])
                assert np.all(np.abs(gm - m) <= 8 * eps * (np.abs(m0) + zz + np.abs(m))), (gm - m)
                assert np.all(np.abs(gP - P) <= 12 * eps * np.sqrt(np.outer(np.diag(P0), np.diag(P0))))
                assert not P[~block].any()
                checked += 1
    assert checked > 200


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_greedy_equals_the_optimal_assignment_where_objects_do_not_compete_and_every_object_keeps_one_id(seed):
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    frames, truth = tr.scene(seed, 40, 2, 16, separated=True, max_dropout=5)
    t = tr.RefTracker(2, 16)
    ids = {}
    n_assoc = 0
    for (bx, sc, lb, ct), tru in zip(frames, truth):
        t.assoc_log = []
        out = t.update(bx, sc, lb, ct)
        for a in t.assoc_log:
            if not a["slots"] or not a["rows"]:
                assert a["matches"] == []
                continue
            cost = np.where(a["ok"], 1.0 - a["iou"].astype(np.float64), 1e6)
            r, c = lsa(cost)
            best = {(a["slots"][i], a["rows"][j]) for i, j in zip(r, c) if a["ok"][i, j]}
            assert best == set(a["matches"])
            n_assoc += len(best)
        for b in range(2):
            for row, obj in tru[b].items():
                if out[6][b, row] >= 0:
                    ids.setdefault((b, obj), set()).add(int(out[6][b, row]))
    assert n_assoc > 150 and len(ids) == 12
    assert all(len(v) == 1 for v in ids.values()), ids
    assert len({(b, next(iter(v))) for (b, _), v in ids.items()}) == 12          # and no two objects of a stream share one


def _defect_case(defect):
    """-> (constructor arguments, frames) of a scene built so that this deviation shows."""
    grow = [(100.0, 100.0, 160.0, 180.0 + 6.0 * i) for i in range(6)]
    if defect == "ge":
        return dict(match_thresh=0.5), [[(BOX, 0.9, 1)], [((100.0, 100.0, 160.0, 140.0), 0.9, 1)]]
    if defect == "lost_stage2":
        return {}, [[(BOX, 0.9, 1)], [], [(BOX, 0.3, 1)]]
    if defect == "keep_vh":                 # a box that grows acquires a velocity of h; lost, it must stop growing
        return {}, [[(g, 0.9, 1)] for g in grow] + [[], [], []]
    if defect == "predict_tentative":
        return {}, [[], [(BOX, 0.9, 1)], [(shifted(2), 0.9, 1)]]
    if defect == "tie_high_slot":           # two tracks with the same box: the detection goes to the lower slot
        return {}, [[(BOX, 0.9, 1), (BOX, 0.8, 1)], [(BOX, 0.9, 1)]]
    if defect == "id_score_order":
        return {}, [[(BOX, 0.7, 1), (shifted(200), 0.9, 1)]]
    raise AssertionError(defect)


def _run_ref(kw, frames, defect=None, T=4):
    t = tr.RefTracker(1, T, defect=defect, **kw)
    outs = [t.update(*frame_of(rows)) for rows in frames]
    return t, outs


def _same_arrays(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize("defect", tr.DEFECTS)
def test_a_planted_defect_moves_the_restatement(defect):
    kw, frames = _defect_case(defect)
    good, go = _run_ref(kw, frames)
    bad, bo = _run_ref(kw, frames, defect)
    same = all(_same_arrays(x, y) for x, y in zip(go[-1], bo[-1])) and all(_same_arrays(good.table()[k], bad.table()[k]) for k in good.FIELDS)
    assert not same
    if defect == "tie_high_slot":
        assert go[-1][3][0, 0] == 1 and bo[-1][3][0, 0] == 2
    if defect == "id_score_order":
        assert go[-1][6][0, :2].tolist() == [1, 2] and bo[-1][6][0, :2].tolist() == [2, 1]
    if defect == "keep_vh":
        assert good.filter[0, 16, 0] == 0 and good.filter[0, 15, 0] < bad.filter[0, 15, 0]


def test_argument_errors_without_a_gpu():
    with pytest.raises(RuntimeError):
        dtrack.ByteTracker(2, "cpu")
    for kw in (dict(streams=0), dict(max_tracks=0), dict(max_tracks=257), dict(track_thresh=float("nan")), dict(low_thresh=-0.1),
               dict(match_thresh=1.5), dict(track_buffer=-1)):
        args = dict(streams=2, device="cuda")
        args.update(kw)
        with pytest.raises(ValueError):
            dtrack.ByteTracker(**args)
    m = models.ssdlite320_mobilenet_v3_large(num_classes=3)
    with pytest.raises(ValueError):
        m.track(torch.zeros(1, 3, 320, 320), object())
    m.train()
    with pytest.raises(ValueError):
        m.track(torch.zeros(1, 3, 320, 320), None)


# ----------------------------------------------------------------------------------------------------------------------------------
# GPU: the device against the restatement, bit for bit
# ----------------------------------------------------------------------------------------------------------------------------------
OUT_NAMES = ("boxes", "scores", "labels", "ids", "det", "counts", "det_ids")


def _dev(frame):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in frame]


def _assert_step(ref, want, dev, got, where):
    for name, w, g in zip(OUT_NAMES, want, got):
        g = g.cpu().numpy()
        assert _same_arrays(w, g), "{}: output {} differs\nwant {}\ngot  {}".format(where, name, w[w != g][:8] if w.shape == g.shape else w.shape,
                                                                                  g[w != g][:8] if w.shape == g.shape else g.shape)
    tab = dev.table()
    for k in ref.FIELDS:
        w, g = ref.table()[k], tab[k].cpu().numpy()
        assert _same_arrays(w, g), "{}: state field {} differs at {}".format(where, k, np.argwhere(w != g)[:8].tolist())


def _run_both(frames, B, T, between=None, **kw):
    """Steps the device tracker and the restatement through the frames and compares everything after every frame."""
    ref = tr.RefTracker(B, T, **kw)
    dev = dtrack.ByteTracker(B, "cuda", max_tracks=T, **kw)
    for i, fr in enumerate(frames):
        if between is not None:
            between(i, ref, dev)
        want = ref.update(*fr)
        got = dev.update(*_dev(fr))
        _assert_step(ref, want, dev, got, "frame {}".format(i + 1))
    return ref, dev


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(6))
def test_random_scenes_bit_for_bit(seed):
    frames, _ = tr.scene(100 + seed, 40, 3, 64, objects=7)
    ref, _ = _run_both(frames, 3, 32, track_buffer=3, class_agnostic=bool(seed & 1))
    assert ref.next_id.min() > 8 and ref.frame.tolist() == [40] * 3        # tracks were removed and restarted along the way


def _grid(n, per_row=32, pitch=44.0, side=30.0):
    i = np.arange(n)
    x, y = (i % per_row) * pitch, (i // per_row) * pitch
    return np.stack([x, y, x + side, y + side], 1).astype(f32)


def _grid_frames(counts, d, frames=3, drift=1.0):
    """Disjoint boxes on a grid, count[b] of them in stream b, all high, drifting by `drift` pixels a frame."""
    out = []
    rng = np.random.RandomState(5)
    for f in range(frames):
        bx = rng.uniform(0, 500, (len(counts), d, 4)).astype(f32)
        sc = rng.uniform(0.6, 1, (len(counts), d)).astype(f32)
        lb = np.ones((len(counts), d), np.int64)
        for b, c in enumerate(counts):
            bx[b, :c] = _grid(c) + f32(drift * f)
        out.append((bx, sc, lb, np.asarray(counts, np.int32)))
    return out


@pytest.mark.gpu
def test_the_sizes_at_which_the_kernel_changes_path():
    """Row counts around the wave and the workgroup size and at the limit; track tables around them; a 257th track that must be dropped and counted."""
    ref, _ = _run_both(_grid_frames([0, 1, 63, 64, 65, 512], 512), 6, 256)
    assert ref.dropped.tolist() == [0, 0, 0, 0, 0, 256 * 3] and (ref.state[5] == tr.TRACKED).sum() == 256
    ref, _ = _run_both(_grid_frames([255, 256, 257], 300), 3, 256)
    assert ref.dropped.tolist() == [0, 0, 3]
    ref, _ = _run_both(_grid_frames([63, 64, 65, 66], 80), 4, 65)
    assert ref.dropped.tolist() == [0, 0, 0, 3] and [(s != tr.FREE).sum() for s in ref.state] == [63, 64, 65, 65]
    ref, _ = _run_both(_grid_frames([3], 8), 1, 1)                                                     # max_tracks = 1
    assert ref.dropped[0] == 6
    frames, _ = tr.scene(7, 6, 65, 16, objects=4)                                                      # B = 65
    _run_both(frames, 65, 7, track_buffer=2)
    frames, _ = tr.scene(8, 6, 1, 16, objects=4)                                                       # B = 1
    _run_both(frames, 1, 7, track_buffer=2)


@pytest.mark.gpu
def test_a_chain_takes_as_many_rounds_as_it_has_tracks():
    """k tracks and k + 1 detections on a line, every weight along the path D0 - T0 - D1 - T1 - ... - Dk larger than the one before: every track's
    best detection is the one to its right, and only the last pair is mutual. The sequential answer gives every track its right neighbour, one
    pair per round; every detection taking its best track would hand D1 .. Dk-1 to the wrong side."""
    k = 7
    gaps = [30.0 - g for g in range(2 * k)]
    tx, dx, x = [], [], 0.0
    for i in range(k):
        dx.append(x)
        x += gaps[2 * i]
        tx.append(x)
        x += gaps[2 * i + 1]
    dx.append(x)
    sq = lambda x0: (x0, 50.0, x0 + 60.0, 110.0)      # noqa: E731
    f1 = frame_of([(sq(v), 0.9, 1) for v in tx], d=16)
    f2 = frame_of([(sq(v), 0.9, 1) for v in dx], d=16)
    ref, _ = _run_both([f1, f2], 1, 8)
    assert ref.assoc_log[-3]["matches"] == [(i, i + 1) for i in reversed(range(k))]
    assert ref.det[0, :k].tolist() == list(range(1, k + 1))


@pytest.mark.gpu
def test_nan_frames_an_empty_stream_beside_a_full_one_and_reset_in_mid_sequence():
    frames, _ = tr.scene(21, 14, 3, 32, objects=6)
    for bx, sc, lb, ct in frames:
        ct[1] = 0                                              # stream 1 never sees anything
        bx[2, 20:] = np.nan                                    # garbage rows beyond the count: NaN as well
    frames[5][1][:] = np.nan                                   # one frame in which every score is NaN
    frames[6][0][:] = np.nan                                   # ... and one in which every box is

    def between(i, ref, dev):
        if i == 9:
            ref.reset([0])
            dev.reset([0])
    ref, dev = _run_both(frames, 3, 16, between=between, track_buffer=2)
    assert ref.frame.tolist() == [5, 14, 14] and ref.next_id[1] == 1 and not ref.state[1].any()


@pytest.mark.gpu
def test_two_runs_give_the_same_bits_and_state_dict_resumes_a_run():
    frames, _ = tr.scene(31, 12, 2, 32, objects=6)
    a = dtrack.ByteTracker(2, "cuda", max_tracks=16, track_buffer=2)
    b = dtrack.ByteTracker(2, "cuda", max_tracks=16, track_buffer=2)
    c = dtrack.ByteTracker(2, "cuda", max_tracks=16, track_buffer=30, class_agnostic=True)
    for i, fr in enumerate(frames):
        if i == 6:
            sd = a.state_dict()
            assert sd["state"].device.type == "cpu" and sd["params"]["track_buffer"] == 2
            c.load_state_dict(sd)
        oa = [t.cpu().numpy() for t in a.update(*_dev(fr))]
        ob = [t.cpu().numpy() for t in b.update(*_dev(fr))]
        assert all(_same_arrays(x, y) for x, y in zip(oa, ob))
        assert torch.equal(a.state, b.state)
        if i >= 6:
            oc = [t.cpu().numpy() for t in c.update(*_dev(fr))]
            assert all(_same_arrays(x, y) for x, y in zip(oa, oc)) and torch.equal(a.state, c.state)


@pytest.mark.gpu
def test_a_captured_update_replays_like_the_eager_one():
    frames, _ = tr.scene(41, 5, 2, 32, objects=5)
    eager = dtrack.ByteTracker(2, "cuda", max_tracks=16)
    want = [[t.cpu().numpy().copy() for t in eager.update(*_dev(fr))] for fr in frames]
    cap = dtrack.ByteTracker(2, "cuda", max_tracks=16)
    static = _dev(frames[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap.update(*static)                                    # warm-up outside the capture: allocates the outputs
    torch.cuda.current_stream().wait_stream(side)
    cap.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = cap.update(*static)
    cap.reset()                                                # (the capture itself ran nothing)
    for fr, w in zip(frames, want):
        for dst, src in zip(static, fr):
            dst.copy_(torch.from_numpy(np.ascontiguousarray(src)))
        graph.replay()
        assert all(_same_arrays(x, y.cpu().numpy()) for x, y in zip(w, outs))
    assert torch.equal(cap.state, eager.state)


@pytest.mark.gpu
def test_rejections():
    t = dtrack.ByteTracker(2, "cuda", max_tracks=8)
    ok = _dev(frame_of([[(BOX, 0.9, 1)], []], d=8, B=2))
    t.update(*ok)
    bad = _dev(frame_of([[], []], d=513, B=2))
    with pytest.raises(ValueError):
        t.update(*bad)                                         # d = 513
    with pytest.raises(ValueError):
        t.update(*[x.cpu() for x in ok])                       # CPU tensors
    with pytest.raises(ValueError):
        t.update(ok[0], ok[1], ok[2].int(), ok[3])             # labels int32
    with pytest.raises(ValueError):
        t.update(ok[0].double(), ok[1], ok[2], ok[3])
    with pytest.raises(ValueError):
        t.update(ok[0][:1], ok[1][:1], ok[2][:1], ok[3][:1])   # one stream for a tracker of two
    with pytest.raises(ValueError):
        t.reset([2])
    # the C entry point itself
    L = _lib.lib()
    p = C.c_void_p
    outs = t.update(*ok)
    state_before = t.state.clone()

    def call(params, d=8, state_bytes=None, boxes=None):
        return L.dn_track_update(p((boxes if boxes is not None else ok[0]).data_ptr()), p(ok[1].data_ptr()), p(ok[2].data_ptr()), p(ok[3].data_ptr()),
                                 2, d, C.byref(params), p(t.state.data_ptr()), t.state.numel() if state_bytes is None else state_bytes,
                                 *[p(o.data_ptr()) for o in outs], None)

    def params(**kw):
        q = _lib.TrackParams.from_buffer_copy(t.params)
        for k, v in kw.items():
            setattr(q, k, v)
        return q
    assert call(params(max_tracks=257)) == -4 and call(params(), d=513) == -4                            # DN_E_UNSUPPORTED
    assert call(params(track_thresh=float("nan"))) == -1 and call(params(low_thresh=-1.0)) == -1          # DN_E_INVALID
    assert call(params(match_thresh=float("nan"))) == -1 and call(params(track_buffer=-1)) == -1 and call(params(), d=0) == -1
    assert call(params(max_tracks=16)) == -3 and call(params(), state_bytes=16) == -3                     # DN_E_WORKSPACE
    assert call(params(), boxes=ok[0].view(-1)[1:]) == -1                                                  # boxes not 16-byte aligned
    assert L.dn_track_reset(None, 2, 8, None, None) == -1 and L.dn_track_reset(p(t.state.data_ptr()), 2, 257, None, None) == -4
    torch.cuda.synchronize()
    assert torch.equal(t.state, state_before)                                                              # nothing was launched


# ----------------------------------------------------------------------------------------------------------------------------------
# model level
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return models.load_synthetic(models.ssdlite320_mobilenet_v3_large(num_classes=21, score_thresh=0.4), 0).cuda().eval()


def _video(frames=6, streams=4, h=300, w=420, step=3):
    base = torch.from_numpy(synth.images(2024, streams, h, w)).cuda()
    return [torch.roll(base, shifts=step * f, dims=3).contiguous() for f in range(frames)]


@pytest.mark.gpu
def test_ssd_track_equals_forward_batch_followed_by_the_restatement(model):
    video = _video()
    D = model.detections_per_img
    dev = dtrack.ByteTracker(4, "cuda", max_tracks=64)
    ref = tr.RefTracker(4, 64)
    seen = 0
    for i, imgs in enumerate(video):
        got = model.track(imgs, dev)
        det = [t.cpu().numpy().copy() for t in model.forward_batch(imgs)]
        assert det[1].shape == (4, D)
        want = ref.update(*det)
        _assert_step(ref, want, dev, got, "frame {}".format(i + 1))
        seen += int(want[5].sum())
    print("tracks output over the sequence:", seen, "ids handed out per stream:", (ref.next_id - 1).tolist())
    assert seen > 0


@pytest.mark.gpu
def test_update_on_a_pipeline_ticket_equals_update_on_forward_batch_outputs(model):
    from demonet_amd.pipeline import ForwardPipeline
    video = _video(frames=4)
    a = dtrack.ByteTracker(4, "cuda", max_tracks=64)
    b = dtrack.ByteTracker(4, "cuda", max_tracks=64)
    want = []
    for imgs in video:
        want.append([t.cpu().numpy().copy() for t in a.update(*model.forward_batch(imgs))])
    pipe = ForwardPipeline(model, 4, depth=2, height=300, width=420)
    try:
        for imgs, w in zip(video, want):
            ticket = pipe.submit(imgs)
            st = pipe.stream_of(ticket)
            b.state.record_stream(st)
            got = b.update(*pipe.outputs(ticket), stream=st)
            st.synchronize()
            assert all(_same_arrays(x, y.cpu().numpy()) for x, y in zip(w, got))
    finally:
        pipe.close()
    assert torch.equal(a.state, b.state)
