"""Appearance association in the tracker, on the device (demonet_amd/track.py AppearanceTracker, csrc/trackapp.hip).

The reference (tests/track_appearance_ref.py) is TEACHER-FORCED: at each frame it associates with the device's own similarity matrix S and starts
features from the device's own normalised rows en, both read back. Nothing it decides then depends on how the matrix cores or the norm's sum
round, so every output and every field of the tracker's state must agree BIT FOR BIT after every frame. S and en themselves are held to error
bounds derived in the tests that check them, and S to exact equality where the data makes every partial sum exact.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import track_appearance_ref as ar
import track_ref as tr
from demonet_amd import _lib, models
from demonet_amd import track as dtrack

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32, f16 = np.float32, np.float16
U = 2.0 ** -24                          # the unit roundoff of fp32
OUT_NAMES = ("boxes", "scores", "labels", "ids", "det", "counts", "det_ids")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _step(dev, fr, emb=None, index=None):
    out = dev.update(*[_dev(a) for a in fr], None if emb is None else _dev(emb), None if index is None else _dev(index))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _grid(n, per_row=32, pitch=44.0, side=30.0):
    i = np.arange(n)
    x, y = (i % per_row) * pitch, (i // per_row) * pitch
    return np.stack([x, y, x + side, y + side], 1).astype(f32)


def _frame(B, d, counts, boxes=None, score=0.9):
    bx = np.zeros((B, d, 4), f32)
    bx[:] = _grid(d) if boxes is None else boxes
    return bx, np.full((B, d), score, f32), np.ones((B, d), np.int64), np.asarray(counts, np.int32)


def _table_of(rows, dim, vectors):
    """rows: list of (stream, row) -> (emb [E, dim] f32, index [E, 8] i32), slot e for rows[e]."""
    index = np.zeros((len(rows), 8), np.int32)
    index[:, :2] = rows
    return np.asarray(vectors, f32).reshape(len(rows), dim), index


# ---------------------------------------------------------------------------------------------------------------- 1. the normalised rows
@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=["fp16", "fp32"])
def test_normalised_rows_against_float64(dtype):
    """en[e][k] = fp16(fl(x_k / n)) with n = fl(sqrt(ss)), ss the fp32 sum of the fp32 squares in SOME order. Every term of ss is >= 0, so
    whatever the order ss = sum x_k^2 (1 + t), |t| <= gamma_dim ~ dim U (one rounding per square, at most dim - 1 per addition chain); the square
    root halves that and adds its own rounding, the division adds one: the fp32 quotient is exact (1 + r), |r| <= (dim / 2 + 2) U + O(U^2), which
    (dim / 2 + 4) U covers for dim <= 512. The conversion to fp16 rounds to nearest: half a unit in the last place of the fp16 grid at the
    value. So |en - exact| <= ulp16 / 2 + (dim / 2 + 4) U |exact|, the ulp taken at the larger of |en| and |exact|."""
    rng = np.random.RandomState(7)
    for dim in (32, 96, 512):
        E = 130
        x = (rng.normal(0, 1, (E, dim)) * rng.choice([1e-3, 1.0, 30.0], (E, 1))).astype(dtype)
        x[3, 5], x[4, 0], x[5], x[6, dim - 1] = np.nan, np.inf, 0, -np.inf
        x[7, 1:] = 0                                                       # one element carries the whole norm: +-1 exactly
        dev = dtrack.AppearanceTracker(1, DEV, dim, max_tracks=4)
        index = np.full((E, 8), -1, np.int32)
        _step(dev, _frame(1, 4, [0]), x, index)
        en = dev.normalised().cpu().numpy()
        present = dev._ws_view("present").cpu().numpy()
        absent = [3, 4, 5, 6]
        assert en.dtype == np.float16 and en.shape == (E, dim)
        assert not en[absent].any() and not present[absent].any() and present.sum() == E - 4
        keep = np.setdiff1d(np.arange(E), absent)
        x64 = x[keep].astype(np.float64)
        exact = x64 / np.linalg.norm(x64, axis=1, keepdims=True)
        got = en[keep].astype(np.float64)
        half_ulp = 0.5 * np.spacing(np.maximum(np.abs(en[keep]), np.abs(exact).astype(np.float16))).astype(np.float64)
        bound = half_ulp + (dim / 2 + 4) * U * np.abs(exact)
        err = np.abs(got - exact)
        assert np.all(err <= bound), (dim, float((err / bound).max()))
        assert float((err / bound).max()) > 0.3                            # (the bound is not idle)
        assert abs(float(en[7, 0])) == 1.0


# ---------------------------------------------------------------------------------------------------------------- 2. the similarity matrix
def _started(B, T, dim, vectors, drop=()):
    """A tracker whose T slots per stream were started in frame 1 from `vectors` [B, T, dim] (slots in `drop` from rows without an embedding)."""
    dev = dtrack.AppearanceTracker(B, DEV, dim, max_tracks=T)
    rows = [(b, j) for b in range(B) for j in range(T) if (b, j) not in drop]
    emb, index = _table_of(rows, dim, [vectors[b, j] for b, j in rows])
    out = _step(dev, _frame(B, T, [T] * B), emb, index)
    assert out[5].tolist() == [T] * B                                      # frame 1: every row starts a confirmed track, slot = row
    return dev


def test_similarity_within_the_summation_bound():
    """Against the float64 dot of the device's OWN fp16 operands (the features as the device holds them, rounded to fp16 by torch's
    round-to-nearest-even conversion, and the device's en): the products of two fp16 values are exact in fp32, so the only error is the
    accumulation's. For K terms added in ANY order with round-to-nearest, |err| <= gamma_(K-1) sum|a_k b_k| with gamma_n = n U / (1 - n U); the
    test uses gamma_K and a factor 2 for a matrix-instruction accumulate that may not round to nearest (truncation doubles the per-step error)."""
    rng = np.random.RandomState(11)
    B, T, d, dim = 2, 17, 40, 96
    dev = _started(B, T, dim, rng.normal(0, 1, (B, T, dim)), drop={(0, 3), (1, 16)})
    for it in range(3):                                                    # frame 2 reads started features, frames 3 and 4 smoothed ones
        valid, feat = [t.cpu().numpy().copy() for t in dev.features()]
        counts = [d, 23]
        rows = [(b, j) for b in range(B) for j in range(counts[b]) if (b + j) % 5]
        emb, index = _table_of(rows, dim, rng.normal(0, 1, (len(rows), dim)))
        fr = _frame(B, d, counts, boxes=_grid(d) + f32(2.0 * it))
        _step(dev, fr, emb, index)
        S = dev.similarity().cpu().numpy()
        en = dev.normalised().cpu().numpy().astype(np.float64)
        a = torch.from_numpy(feat).half().numpy().astype(np.float64)
        rmap = ar.row_map(index, np.asarray(counts), B, d)
        assert S.shape == (B, T, d) and S.dtype == np.float32
        gamma = dim * U / (1 - dim * U)
        worst = 0.0
        for b in range(B):
            for j in range(d):
                if rmap[b, j] < 0:
                    assert not S[b, :, j].any()
                    continue
                prod = a[b] * en[rmap[b, j]][None, :]
                want, mag = prod.sum(1), np.abs(prod).sum(1)
                on = valid[b] != 0
                assert not S[b, ~on, j].any()
                err = np.abs(S[b, on, j].astype(np.float64) - want[on])
                assert np.all(err <= 2 * gamma * mag[on]), (it, b, j, float((err / (2 * gamma * mag[on])).max()))
                worst = max(worst, float(np.abs(S[b, on, j]).max()))
        assert worst > 0.1 and valid.sum() >= B * T - 2


EXACT = [(32, 1, 1), (64, 3, 15), (96, 15, 16), (512, 16, 17), (64, 17, 512), (512, 256, 512), (96, 256, 1), (32, 16, 16), (512, 3, 17)]


@pytest.mark.parametrize("dim,T,rows", EXACT, ids=["dim{}-T{}-rows{}".format(*c) for c in EXACT])
def test_similarity_exact_on_quarter_vectors(dim, T, rows):
    """Embeddings with 16 non-zero entries of +-1/4: the norm is exactly 1, en = x, a started feature = x, every product is +-1/16 and every
    partial sum a multiple of 1/16 below 2: nothing rounds, in any order. S of frame 2 equals the integer answer bit for bit -- across the
    slot paddings (max_tracks 1 and 3 -> 4, 15 / 16 / 17, 256), the row tails (1, 15 / 16 / 17, 512) and K = 32 .. 512. A wrong lane map, a
    K-slice that is not summed or a tail tile stored in the wrong place shows here."""
    B = 2
    tv = ar.quarter_vectors(B * T, dim, 3).reshape(B, T, dim)
    drop = {(1, T - 1)} if T > 1 else set()
    dev = _started(B, T, dim, tv, drop)
    counts = [rows, max(rows - 3, 1)]
    cand = [(b, j) for b in range(B) for j in range(counts[b])]
    keep = [r for i, r in enumerate(cand) if i % 7 != 3 or len(cand) < 4]
    ev = ar.quarter_vectors(len(keep), dim, 4)
    emb, index = _table_of(keep, dim, ev * f32(3.0))                       # (a power-of-two-free scale: the step normalises; 0.75^2 * 16 = 9)
    need = _lib.lib().dn_track_appearance_workspace_bytes(B, T, rows, len(keep), dim)
    big = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    dev._ws[(rows, len(keep))] = big[:need]
    big[:need] = 0xFF
    _step(dev, _frame(B, rows, counts, boxes=_grid(rows) + f32(1.0)), emb, index)
    assert bool((big[need:] == 0xA5).all())                               # nothing behind the documented workspace
    S = dev.similarity().cpu().numpy()
    en = dev.normalised().cpu().numpy()
    assert _same(en, ev.astype(f16))
    want = np.zeros((B, T, rows), f32)
    ti = np.rint(tv * 4).astype(np.int64)
    ei = np.rint(ev * 4).astype(np.int64)
    for e, (b, j) in enumerate(keep):
        want[b, :, j] = (ti[b] @ ei[e]).astype(f32) / f32(16)
    for b, j in drop:
        want[b, j, :] = 0
    assert _same(S, want), np.argwhere(S != want)[:8].tolist()
    assert np.abs(want).max() > 0


# ---------------------------------------------------------------------------------------------------------------- 3. the association
def _feature_bound(prev, x, alpha, beta, dim):
    """What a smoothed feature may differ from float64 by. v = alpha s + beta x in three roundings: |dv_k| <= 2 U (|alpha s_k| + |beta x_k|);
    the norm n of the computed v is off by (dim / 2 + 2) U relative (see test_normalised_rows_against_float64) and the division adds U. With
    exact e = v / |v|: |got_k - e_k| <= |dv_k| / |v| + |e_k| (|dv| / |v| + (dim / 2 + 3) U), |dv| <= 2 U (alpha + beta) as |s|, |x| <= 1 + 2^-10;
    second-order terms are covered by the factor 1 + 2^-10."""
    s, x = prev.astype(np.float64), x.astype(np.float64)
    a, b = float(alpha), float(beta)
    v = a * s + b * x
    n = np.linalg.norm(v)
    dv = 2 * U * (np.abs(a * s) + np.abs(b * x))
    e = v / n
    return e, (dv / n + np.abs(e) * (2 * U * (a + b) * (1 + 2.0 ** -10) / n + (dim / 2 + 3) * U)) * (1 + 2.0 ** -10)


def _assert_features(ref, dev, before, en, rmap, rowhas, where):
    """flags exact; a started feature is float(en) exactly, a smoothed one within _feature_bound of float64 from the DEVICE's previous one; the
    reference then continues from the device's features (teacher-forced like S)."""
    valid, feat = [t.cpu().numpy() for t in dev.features()]
    pv, pf = before
    assert np.array_equal(valid != 0, ref.fvalid), "{}: feature flags differ at {}".format(where, np.argwhere((valid != 0) != ref.fvalid)[:8].tolist())
    smoothed = 0
    for b in range(ref.B):
        frame = int(ref.frame[b])
        for s in range(ref.T):
            if not ref.fvalid[b, s]:
                continue
            j = int(ref.det[b, s])
            seen = ref.last_frame[b, s] == frame and j >= 0 and rowhas[b, j]
            if not seen:
                assert _same(feat[b, s], pf[b, s]), "{}: an untouched feature moved ({}, {})".format(where, b, s)
            elif ref.start_frame[b, s] == frame or not pv[b, s]:
                assert _same(feat[b, s], en[rmap[b, j]].astype(f32)), "{}: a started feature is not float(en) ({}, {})".format(where, b, s)
            else:
                e, bound = _feature_bound(pf[b, s], en[rmap[b, j]], ref.alpha, ref.beta, ref.dim)
                err = np.abs(feat[b, s].astype(np.float64) - e)
                assert np.all(err <= bound), "{}: feature ({}, {}) off by {} of its bound".format(where, b, s, float((err / bound).max()))
                smoothed += 1
    ref.feat[:] = feat
    return smoothed


def _run_scene(B, T, dim, kw, frames, embs, fp16=False):
    ref = ar.AppRefTracker(B, dim, max_tracks=T, **kw)
    dev = dtrack.AppearanceTracker(B, DEV, dim, max_tracks=T, **kw)
    smoothed = nofeat = 0
    for i, (fr, (emb, index)) in enumerate(zip(frames, embs)):
        where = "frame {}".format(i + 1)
        before = [t.cpu().numpy().copy() for t in dev.features()]
        emb = emb.astype(f16) if fp16 else emb
        got = _step(dev, fr, emb, index)
        S, en = dev.similarity().cpu().numpy(), dev.normalised().cpu().numpy()
        d = fr[1].shape[1]
        rmap = ar.row_map(index, fr[3], B, d)
        present = dev._ws_view("present").cpu().numpy() != 0
        assert np.array_equal(dev._ws_view("map").cpu().numpy(), rmap), where
        assert np.array_equal(present, ar.normalise(emb)[0]), where
        rowhas = (rmap >= 0) & present[np.maximum(rmap, 0)]
        want = ref.update(*fr, emb=emb, index=index, S=S, en=en)
        for name, w, g in zip(OUT_NAMES, want, got):
            assert _same(w, g), "{}: output {} differs at {}".format(where, name, np.argwhere(w != g)[:8].tolist())
        tab = dev.table()
        for k in ref.FIELDS:
            w, g = ref.table()[k], tab[k].cpu().numpy()
            assert _same(w, g), "{}: state field {} differs at {}".format(where, k, np.argwhere(w != g)[:8].tolist())
        smoothed += _assert_features(ref, dev, before, en, rmap, rowhas, where)
        nofeat += int(((ref.state != tr.FREE) & ~ref.fvalid).sum())
    return ref, dev, smoothed, nofeat


@pytest.fixture(scope="module")
def scenes():
    return ar.scene_set()


@pytest.mark.parametrize("name", ["random0", "random1", "random2", "random3", "crossing", "refind_prox1", "refind_prox05", "equality", "low_row"])
def test_scenes_bit_for_bit(scenes, name):
    ref, dev, smoothed, nofeat = _run_scene(*scenes[name], fp16=name == "random1")
    if name.startswith("random"):
        assert smoothed > 100 and nofeat > 0 and ref.fvalid.any()      # smoothed features, and live tracks that have none
    if name == "crossing":
        assert ref.id[0, :2].tolist() == [1, 2] and smoothed >= 40
        assert dev.table()["det"][0, :2].tolist() == [0, 1]               # after the crossing each track still holds its own row
    if name == "refind_prox1":
        assert ref.state[0].tolist() == [tr.TRACKED, 0, 0, 0] and ref.next_id[0] == 2      # found again without overlap: the same id
    if name == "refind_prox05":
        assert ref.state[0].tolist() == [tr.LOST, tr.TRACKED, 0, 0]
    if name == "low_row":
        assert ref.state[0, 0] == tr.LOST


# ---------------------------------------------------------------------------------------------------------------- 4. untrusted input
def test_garbage_index_rows_duplicates_and_embeddings_that_are_not_numbers():
    rng = np.random.RandomState(5)
    B, T, d, dim, E = 2, 8, 16, 64, 64
    frames, truth = tr.scene(77, 6, B, d, objects=5)
    ref = ar.AppRefTracker(B, dim, max_tracks=T, proximity_thresh=1.0)
    dev = dtrack.AppearanceTracker(B, DEV, dim, max_tracks=T, proximity_thresh=1.0)
    base = rng.normal(0, 1, (B, 8, dim))
    for i, fr in enumerate(frames):
        fr = tuple(a.copy() for a in fr)
        if i == 3:
            fr[3][0] = 2 ** 31 - 1                                         # a count far beyond d: clamped to d
        if i == 4:
            fr[3][1] = -7
        emb = rng.normal(0, 1, (E, dim)).astype(f32)
        index = rng.randint(-2 ** 31, 2 ** 31 - 1, (E, 8), dtype=np.int64).astype(np.int32)      # random bits
        slots = rng.permutation(E)
        k = 0
        for b in range(B):
            for j, o in truth[i][b].items():
                for rep in range(2 if j % 3 == 0 else 1):                  # duplicates: two slots name the row, the higher one wins
                    e = slots[k]
                    k += 1
                    index[e, :2] = (b, j)
                    emb[e] = base[b, o] + rng.normal(0, 0.02, dim)
        index[slots[k], :2], index[slots[k + 1], :2], index[slots[k + 2], :2] = (-1, 0), (0, d), (B, 0)
        index[slots[k + 3], :2] = (1, int(np.clip(fr[3][1], 0, d)))        # row == the clamped count: ignored
        bad = slots[:k:4]
        emb[bad[0::3], 7], emb[bad[1::3], 0], emb[bad[2::3]] = np.nan, np.inf, 0
        ins = [_dev(a) for a in fr] + [_dev(emb), _dev(index)]
        copies = [t.clone() for t in ins]
        outs = dev._outs.get(d)
        if outs is not None:
            for o in outs:
                o.view(torch.uint8).fill_(255)
        if dev._last is not None:
            dev._ws[dev._last].fill_(255)                                  # S, en, present and map all start as 0xFF
        got = [o.cpu().numpy() for o in dev.update(*ins)]
        torch.cuda.synchronize()
        assert all(torch.equal(a.view(torch.uint8), c.view(torch.uint8)) for a, c in zip(ins, copies))      # the inputs are only read
        S, en = dev.similarity().cpu().numpy(), dev.normalised().cpu().numpy()
        assert np.isfinite(S).all() and np.isfinite(en.astype(f32)).all() and np.abs(S).max() <= 1.0 + 2.0 ** -9
        rmap = ar.row_map(index, fr[3], B, d)
        assert np.array_equal(dev._ws_view("map").cpu().numpy(), rmap)
        present = dev._ws_view("present").cpu().numpy() != 0
        assert np.array_equal(present, ar.normalise(emb)[0]) and not present[bad].any()
        rowhas = (rmap >= 0) & present[np.maximum(rmap, 0)]
        assert not S[~np.broadcast_to(rowhas[:, None, :], S.shape)].any()
        want = ref.update(*fr, emb=emb, index=index, S=S, en=en)
        for name, w, g in zip(OUT_NAMES, want, got):
            assert _same(w, g), (i, name)
        for f in ref.FIELDS:
            assert _same(ref.table()[f], dev.table()[f].cpu().numpy()), (i, f)
        valid, feat = [t.cpu().numpy() for t in dev.features()]
        assert np.array_equal(valid != 0, ref.fvalid)
        ref.feat[:] = feat
    assert ref.fvalid.any() and ref.frame.tolist() == [6, 6]


# ---------------------------------------------------------------------------------------------------------------- 5. equivalence, repeatability
def test_no_embeddings_is_bytetracker_and_two_runs_give_the_same_bits(scenes):
    B, T, dim, kw, frames, embs = scenes["random2"]
    base_kw = {k: v for k, v in kw.items() if k != "proximity_thresh"}
    plain = dtrack.ByteTracker(B, DEV, max_tracks=T, **base_kw)
    none = dtrack.AppearanceTracker(B, DEV, dim, max_tracks=T, **kw)
    empty = dtrack.AppearanceTracker(B, DEV, dim, max_tracks=T, **kw)
    one, two = dtrack.AppearanceTracker(B, DEV, dim, max_tracks=T, **kw), dtrack.AppearanceTracker(B, DEV, dim, max_tracks=T, **kw)
    for i, (fr, (emb, index)) in enumerate(zip(frames[:14], embs)):
        ins = [_dev(a) for a in fr]
        want = [o.cpu().numpy() for o in plain.update(*ins)]
        nobody = np.full_like(index, -1)
        for t, args in ((none, ()), (empty, (_dev(emb), _dev(nobody)))):
            got = [o.cpu().numpy() for o in t.update(*ins, *args)]
            assert all(_same(w, g) for w, g in zip(want, got)), i
            assert torch.equal(t.state, plain.state), i
            assert not t.features()[0].any()
        a = [o.cpu().numpy() for o in one.update(*ins, _dev(emb), _dev(index))]
        b = [o.cpu().numpy() for o in two.update(*ins, _dev(emb), _dev(index))]
        assert all(_same(x, y) for x, y in zip(a, b)), i
        assert torch.equal(one.state, two.state) and torch.equal(one.features_buf, two.features_buf), i
        assert torch.equal(one._ws[one._last], two._ws[two._last]), i       # S, en, present and map
    assert one.features()[0].any() and one.similarity().abs().max() > 0.5


# ---------------------------------------------------------------------------------------------------------------- 6. state, replay, reset
def test_state_dict_round_trip_graph_replay_and_reset_of_one_stream(scenes):
    B, T, dim, kw, frames, embs = scenes["random3"]
    mk = lambda: dtrack.AppearanceTracker(B, DEV, dim, max_tracks=T, **kw)
    eager, resumed, captured = mk(), mk(), mk()
    static = [_dev(a) for a in frames[0]] + [_dev(embs[0][0]), _dev(embs[0][1])]
    for i in range(8):
        ins = [_dev(a) for a in frames[i]] + [_dev(embs[i][0]), _dev(embs[i][1])]
        eager.update(*ins)
        captured.update(*ins)
    sd = eager.state_dict()
    assert set(sd) >= {"state", "features", "appearance", "params"} and sd["features"].device.type == "cpu"
    resumed.load_state_dict(sd)
    with pytest.raises(ValueError):
        dtrack.AppearanceTracker(B, DEV, 32, max_tracks=T, **kw).load_state_dict(sd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    snap = (captured.state.clone(), captured.features_buf.clone())
    with torch.cuda.stream(side):
        captured.update(*static)                                           # warm-up: allocates the outputs and the workspace of this (d, E)
    torch.cuda.current_stream().wait_stream(side)
    captured.state.copy_(snap[0])
    captured.features_buf.copy_(snap[1])
    with torch.cuda.graph(graph):
        cap_out = captured.update(*static)
    captured.state.copy_(snap[0])                                          # (the capture enqueued nothing; the warm-up step is undone)
    captured.features_buf.copy_(snap[1])
    for i in range(8, 13):                                                 # 5 frames on new detections and embeddings
        new = list(frames[i]) + [embs[i][0], embs[i][1]]
        for s, a in zip(static, new):
            s.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        graph.replay()
        ins = [_dev(a) for a in new]
        want = [o.cpu().numpy() for o in eager.update(*ins)]
        again = [o.cpu().numpy() for o in resumed.update(*ins)]
        torch.cuda.synchronize()
        got = [o.cpu().numpy() for o in cap_out]
        for name, w, g, r in zip(OUT_NAMES, want, got, again):
            assert _same(w, g) and _same(w, r), (i, name)
        for t in (captured, resumed):
            assert torch.equal(t.state, eager.state) and torch.equal(t.features_buf, eager.features_buf), i
    assert eager.features()[0].any()
    keep = [t.clone() for t in eager.features()]
    eager.reset([1])
    torch.cuda.synchronize()
    valid, feat = eager.features()
    assert not valid[1].any() and not feat[1].any() and torch.equal(valid[0], keep[0][0]) and torch.equal(feat[2], keep[1][2])
    tab = eager.table()
    assert tab["frame"].tolist() == [13, 0, 13] and tab["next_id"][1] == 1
    eager.reset()
    assert not eager.features_buf.any()


# ---------------------------------------------------------------------------------------------------------------- 7. behind other objects
def test_zone_analytics_behind_an_appearance_tracker(scenes):
    from demonet_amd import zones as dzones
    B, T, dim, kw, frames, embs = scenes["random0"]
    base_kw = {k: v for k, v in kw.items() if k != "proximity_thresh"}
    app, plain = dtrack.AppearanceTracker(B, DEV, dim, max_tracks=T, **kw), dtrack.ByteTracker(B, DEV, max_tracks=T, **base_kw)
    square = [(0, 0), (640, 0), (640, 640), (0, 640)]
    za = dzones.ZoneAnalytics(app, anchor="center").set_all([(320, 0, 320, 640)], [square])
    zp = dzones.ZoneAnalytics(plain, anchor="center").set_all([(320, 0, 320, 640)], [square])
    dzones.check_analytics(za, app, "test")
    events = 0
    for i, fr in enumerate(frames[:12]):
        ins = [_dev(a) for a in fr]
        app.update(*ins)                                                    # no embeddings: the tracks are ByteTracker's, so are the events
        plain.update(*ins)
        (ea, na), (ep, npl) = za.update(), zp.update()
        assert torch.equal(ea, ep) and torch.equal(na, npl), i
        events += int(na.sum())
    assert events > 10 and torch.equal(za.state, zp.state)
    app.update(*[_dev(a) for a in frames[12]], _dev(embs[12][0]), _dev(embs[12][1]))
    ev, n = za.update()                                                     # ... and behind a step with embeddings it reads the same state block
    assert int(n.sum()) >= 0 and ev.shape[0] == B


def test_ssd_track_frames_appearance_equals_the_composition_by_hand():
    import crops_ref as cr
    import regions_ref as rr
    import test_gpu_regions as tgr
    from demonet_amd.crops import ObjectCropper
    from demonet_amd.frames import FrameBatch
    m = models.load_synthetic(models.ssd_lite_mobilenet_v2(image_size=160, num_classes=3), 0).to(DEV)
    try:
        fmt, matrix, full = "nv12", "bt709", False
        dim, cap = 64, 128
        mk_t = lambda: dtrack.AppearanceTracker(2, DEV, dim, max_tracks=64, track_thresh=0.05, low_thresh=0.01, new_thresh=0.05)
        mk_c = lambda: ObjectCropper(2, DEV, size=(16, 8), capacity=cap, dtype=torch.float16, mean=cr.IMAGENET_MEAN, std=cr.IMAGENET_STD)
        ta, tb, ca, cb = mk_t(), mk_t(), mk_c(), mk_c()
        for c in (ca, cb):
            c.patches.zero_()                                              # (slots never written hold the same bytes in both croppers)
        W = torch.from_numpy(np.random.RandomState(9).normal(0, 1, (3 * 16 * 8, dim)).astype(f32)).to(DEV)
        embedder = lambda patches: patches.reshape(patches.shape[0], -1).float() @ W
        batch = FrameBatch(2, DEV, fmt, matrix, full)
        with_feature = 0
        for i in range(4):
            src = [tgr._source(fmt, matrix, full, 940 + 2 * i + b, h, w) for b, (h, w) in enumerate(rr.SIZES)]
            batch.set([tgr._surface(fmt, planes, "256") for planes, _ in src])
            got = [o.clone() for o in m.track_frames_appearance(batch, ta, ca, embedder)]
            boxes, scores, labels, counts = m.forward_frames(batch)
            patches, index, totals = cb(batch, boxes, counts, scores >= tb.params.track_thresh)
            want = tb.update(boxes, scores, labels, counts, embedder(patches), index)
            torch.cuda.synchronize()
            for name, w, g in zip(OUT_NAMES, want, got):
                assert torch.equal(w, g), (i, name)
            assert torch.equal(ta.state, tb.state) and torch.equal(ta.features_buf, tb.features_buf), i
            assert torch.equal(ca.index, cb.index) and int(totals[0]) >= 2, i
            with_feature += int(ta.features()[0].sum())
        assert with_feature > 0 and ta.similarity().shape == (2, 64, boxes.shape[1])
        with pytest.raises(ValueError, match="tracker must be an AppearanceTracker"):
            m.track_frames_appearance(batch, dtrack.ByteTracker(2, DEV), ca, embedder)
        with pytest.raises(ValueError, match="must return"):
            m.track_frames_appearance(batch, ta, ca, lambda p: p)
    finally:
        m.release()


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_every_refusal_returns_its_code_with_nothing_launched():
    import test_track_appearance as cpu
    B, T, d, dim, E = 2, 4, 8, 64, 4
    dev = dtrack.AppearanceTracker(B, DEV, dim, max_tracks=T)
    fr = _frame(B, d, [3, 2])
    emb, index = _table_of([(0, 0), (0, 1), (1, 0), (1, 1)], dim, ar.quarter_vectors(4, dim, 1))
    _step(dev, fr, emb, index)
    ins = [_dev(a) for a in fr] + [_dev(emb), _dev(index)]
    outs = dev._outs[d]
    ws = dev._ws[(d, E)]
    watched = [dev.state, dev.features_buf, ws] + list(outs)
    for t in watched[2:]:
        t.view(torch.uint8).fill_(0x5A)
    torch.cuda.synchronize()
    before = [t.clone() for t in watched]
    L = _lib.lib()
    real = dict(boxes=ins[0].data_ptr(), scores=ins[1].data_ptr(), labels=ins[2].data_ptr(), counts=ins[3].data_ptr(), streams=B, d=d,
                emb=ins[4].data_ptr(), index=ins[5].data_ptr(), E=E, state=dev.state.data_ptr(), state_bytes=dev.state.numel(),
                features=dev.features_buf.data_ptr(), feature_bytes=dev.features_buf.numel(), workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
                outs=[o.data_ptr() for o in outs])
    _lib.debug_last_kernel()
    mark = "track_update_app_kernel"
    assert _lib.debug_last_kernel() == mark
    for what, kw, app, code in cpu.REFUSALS:
        args = dict(real)
        for k, v in kw.items():                                           # the made-up addresses of the CPU test become real ones, moved the same way
            if k in ("emb", "index", "state", "features", "workspace", "boxes") and v:
                args[k] = real[k] + (v & 0xF)
            elif k == "state_bytes":
                args[k] = real[k] - 1
            elif k == "feature_bytes":
                args[k] = real[k] - 1
            elif k == "workspace_bytes":
                args[k] = real[k] - 1
            else:
                args[k] = v
        rc = cpu._call(L, app=cpu._app(**app) if app else None, **args)
        assert rc == code, (what, rc)
        assert _lib.debug_last_kernel() == mark, what                      # no launcher got as far as naming a kernel
    torch.cuda.synchronize()
    for t, b in zip(watched, before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8))
    for bad in (dict(embeddings=ins[4][:, :32]), dict(embeddings=ins[4].double()), dict(embeddings=ins[4], index=ins[5][:2]),
                dict(embeddings=ins[4], index=ins[5].long()), dict(embeddings=None, index=ins[5]), dict(embeddings=ins[4].cpu(), index=ins[5]),
                dict(embeddings=ins[4], index=None)):
        with pytest.raises(ValueError):
            dev.update(*ins[:4], **bad)
    with pytest.raises(RuntimeError):
        dtrack.AppearanceTracker(B, DEV, dim, max_tracks=T).similarity()
