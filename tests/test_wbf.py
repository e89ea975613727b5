"""Weighted boxes fusion: dn_fuse_detections, demonet_amd/fusion.py, SSD.detect_tta and ensemble_detect.

CPU part: the ABI, and the float32 restatement itself (tests/wbf_ref.py), pinned three ways: closed forms, a float64 restatement of the published
algorithm that recomputes every fused box from its whole member list (memberships equal; boxes within (2 T + 3) 2^-24 max|coord|, scores within
(T + 2) 2^-24: the fp32 rounding of T products, T - 1 additions twice and a division), and planted defects that must each show. GPU part: the
device against wbf_ref.fuse bit for bit -- boxes, scores, labels, counts, members --, the sizes at which the walk changes path, determinism, the
rejections, and detect_tta / ensemble_detect against the composition a user would write by hand."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import wbf_ref as wr
from demonet_amd import _lib, fusion, models, sliced, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dn_fuse_detections_workspace_bytes", "dn_fuse_detections")
f32 = np.float32
EPS = 2.0 ** -24


# ----------------------------------------------------------------------------------------------------------------------------------
# cases: dict(boxes [S,d,4], scores [S,d], labels [S,d], counts [S], offsets [S,2], group_begin, weights [S] or None, thresh, skip, d_out)
# ----------------------------------------------------------------------------------------------------------------------------------
def _case(boxes, scores, labels, counts=None, offsets=None, group_begin=None, weights=None, thresh=0.55, skip=0.0, d_out=None):
    boxes, scores, labels = np.asarray(boxes, f32), np.asarray(scores, f32), np.asarray(labels, np.int64)
    S, d = scores.shape
    return dict(boxes=boxes, scores=scores, labels=labels, counts=np.asarray([d] * S if counts is None else counts, np.int32),
                offsets=np.zeros((S, 2), f32) if offsets is None else np.asarray(offsets, f32), group_begin=[0, S] if group_begin is None else group_begin,
                weights=None if weights is None else np.asarray(weights, f32), thresh=thresh, skip=skip, d_out=d if d_out is None else d_out)


def _two(b0, s0, b1, s1, l0=1, l1=1, **kw):
    """Two sources of one row each."""
    return _case([[b0], [b1]], [[s0], [s1]], [[l0], [l1]], d_out=4, **kw)


def _jittered(seed, S, d, counts, n_centres=12, n_labels=3, sigma=1.5, weights=None, **kw):
    """Boxes jittered around n_centres centres (a centre has one label; one box in ten gets a random one), reported by S sources through one
    offset each, scores in random row order, rows at or beyond the count filled with plausible garbage."""
    rng = np.random.default_rng(seed)
    ctr = rng.uniform(60, 900, (n_centres, 2))
    size = rng.uniform(40, 140, (n_centres, 2))
    clab = rng.integers(1, n_labels + 1, n_centres)
    which = rng.integers(0, n_centres, (S, d))
    c = ctr[which] + rng.normal(0, sigma, (S, d, 2))
    wh = size[which] * rng.uniform(0.94, 1.06, (S, d, 2))
    img = np.concatenate([c - wh / 2, c + wh / 2], -1)
    off = rng.uniform(0, 32, (S, 2))
    boxes = (img - np.concatenate([off, off], -1)[:, None, :]).astype(f32)
    scores = rng.uniform(0.05, 1.0, (S, d)).astype(f32)
    labels = np.where(rng.uniform(size=(S, d)) < 0.1, rng.integers(1, n_labels + 1, (S, d)), clab[which]).astype(np.int64)
    return _case(boxes, scores, labels, counts=counts, offsets=off.astype(f32), weights=weights, **kw)


SEEDS = (101, 102, 103, 104, 105, 106)
RANDOM = tuple("r{}_{}".format(seed, w) for seed in SEEDS for w in ("w111", "w211"))


def _grid_boxes(n, pitch=40.0, side=30.0, per_row=128):
    g = np.arange(n)
    x, y = pitch * (g % per_row), pitch * (g // per_row)
    return np.stack([x, y, x + side, y + side], 1).astype(f32)


SIZES = {63: (3, 21), 64: (2, 32), 65: (5, 13), 255: (5, 51), 256: (4, 64), 257: (1, 257), 8192: (16, 512)}      # candidates: (sources, d)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "cf_pair":               # (0,0,10,10) at 0.9 and (1,0,11,10) at 0.6: IoU 9/11, one row: score 0.75, x1 = 0.4, 2 members
        return _two((0, 0, 10, 10), 0.9, (1, 0, 11, 10), 0.6)
    if name == "cf_apart":              # the same two 50 px apart: each seen by one source of two: 0.45 and 0.3
        return _two((0, 0, 10, 10), 0.9, (51, 0, 61, 10), 0.6)
    if name == "cf_single":             # one source of one: its own score and its own box bit for bit
        return _case([[(3.3, 7.7, 20.1, 31.9)]], [[0.3]], [[5]])
    if name == "cf_on_thresh":          # IoU = 50 / 100 = 0.5 = thresh exactly: strict, no fusion
        return _two((0, 0, 10, 10), 0.9, (0, 0, 10, 5), 0.6, thresh=0.5)
    if name == "cf_labels":             # the pair of cf_pair with different labels does not fuse
        return _two((0, 0, 10, 10), 0.9, (1, 0, 11, 10), 0.6, l0=1, l1=2)
    if name == "cf_best":               # clusters A (0..10) and B (5..15), IoU 1/3; the candidate (3..13) has 7/13 with A and 8/12 with B: B, not A
        return _case([[(0, 0, 10, 10), (5, 0, 15, 10)], [(3, 0, 13, 10), (0, 0, 0, 0)]], [[0.9, 0.8], [0.5, 0.0]], [[1, 1], [1, 1]], counts=[2, 1],
                     thresh=0.5)
    if name in RANDOM:                  # 3 sources x 64 rows, full counts
        seed = int(name[1:4])
        return _jittered(seed, 3, 64, [64, 64, 64], weights=(2, 1, 1) if name.endswith("w211") else (1, 1, 1))
    if name.startswith("ragged_"):      # the same six seeds: ragged counts, one source with count 0, a second group whose sources are all empty
        seed = int(name[7:])
        return _jittered(seed, 6, 64, [64, 0, 37, 51, 0, 0], group_begin=[0, 4, 6], d_out=40)
    if name == "nan_scores":
        c = _jittered(111, 3, 64, [64, 50, 64])
        c["scores"][0, 3:40:7] = np.nan
        c["scores"][2, 5] = np.nan
        return c
    if name == "weights_skip":          # unequal weights and a skip_thresh that removes candidates; 0.2 <= score < 0.4 of source 0 pass only weighted
        return _jittered(112, 3, 64, [64, 60, 33], weights=(2, 1, 0.5), skip=0.4)
    if name == "two_groups_outside":    # sources 0 and 6 belong to no group
        return _jittered(113, 7, 48, [48, 48, 20, 48, 31, 48, 48], group_begin=[1, 4, 6], weights=(9, 1, 2, 1, 3, 1, 9), d_out=64)
    if name == "same_source_twice":     # exact ties of v and IoUs of exactly 1
        c = _jittered(114, 1, 64, [64])
        return _case(np.concatenate([c["boxes"]] * 2), np.concatenate([c["scores"]] * 2), np.concatenate([c["labels"]] * 2),
                     offsets=np.concatenate([c["offsets"]] * 2))
    if name == "three_tables":
        # 131 groups: the library hands the kernels 64 groups per launch, so three tables, the second and third with a first group > 0. Two sources
        # of 4 rows per group on 3 centres, ragged counts, unequal weights; group 64, the first of the second table, has no source; source 260
        # belongs to no group
        gb = [2 * g for g in range(65)] + [2 * g for g in range(64, 131)]
        rng = np.random.default_rng(116)
        return _jittered(116, gb[-1] + 1, 4, rng.integers(0, 5, gb[-1] + 1), n_centres=3, n_labels=2, group_begin=gb,
                         weights=rng.choice([0.5, 1.0, 2.0, 3.0], gb[-1] + 1), d_out=6)
    if name.startswith("disjoint_"):   # one label, boxes that do not touch: clusters = candidates
        n = int(name[9:])
        S, d = SIZES[n]
        rng = np.random.default_rng(n)
        scores = rng.permutation(np.linspace(0.05, 0.95, n).astype(f32)).reshape(S, d)
        return _case(_grid_boxes(n).reshape(S, d, 4), scores, np.full((S, d), 7, np.int64), d_out=512)
    if name == "long_clusters":         # 2 048 candidates of one label on 8 sites: clusters of about 256 members
        return _jittered(115, 4, 512, [512] * 4, n_centres=8, n_labels=1, sigma=0.8)
    raise KeyError(name)


def _fuse_ref(c, d_out=None, defect=None):
    return wr.fuse(c["boxes"], c["scores"], c["labels"], c["counts"], c["offsets"], c["group_begin"], c["weights"], c["thresh"], c["skip"],
                   c["d_out"] if d_out is None else d_out, defect=defect)


@functools.lru_cache(maxsize=None)
def expected(name):
    return _fuse_ref(case(name))


@functools.lru_cache(maxsize=None)
def expected64(name):
    c = case(name)
    return wr.fuse64(c["boxes"], c["scores"], c["labels"], c["counts"], c["offsets"], c["group_begin"], c["weights"], c["thresh"], c["skip"])


def _truncated(want, d_out):
    """The outputs of a reference run at a larger d_out, cut to d_out rows."""
    ob, os_, ol, oc, om = want[:5]
    return ob[:, :d_out], os_[:, :d_out], ol[:, :d_out], np.minimum(oc, d_out).astype(np.int32), om[:, :d_out]


# ----------------------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------------------
def test_the_two_symbols_are_exported_declared_and_bound():
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
    q = L.dn_fuse_detections_workspace_bytes
    q.restype, q.argtypes = C.c_size_t, [C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int]
    gb = lambda *v: (C.c_int32 * len(v))(*v)      # noqa: E731
    assert q(16, 512, gb(0, 16), 1) >= 16 * 512 * 60                       # pure host arithmetic
    assert q(17, 512, gb(0, 17), 1) == 0 and q(17, 512, gb(0, 16, 17), 2) > 0      # 8 704 slots in one group; 8 192 + 512
    assert q(1, 513, gb(0, 1), 1) == 0 and q(0, 8, gb(0, 0), 1) == 0 and q(4, 8, gb(0, 3, 2), 2) == 0 and q(4, 8, None, 1) == 0


def _rows(name):
    ob, os_, ol, oc, om, mem = expected(name)
    n = int(oc[0])
    return ob[0, :n], os_[0, :n], ol[0, :n], om[0, :n]


def test_closed_forms():
    b, s, l, m = _rows("cf_pair")
    assert len(s) == 1 and m.tolist() == [2] and l.tolist() == [1]
    assert s[0] == f32(f32(f32(f32(0.9) + f32(0.6)) / f32(2)) * f32(2)) / f32(2) and abs(float(s[0]) - 0.75) < 2 * EPS
    assert np.allclose(b[0], [0.4, 0.0, 10.4, 10.0], rtol=0, atol=11 * 4 * EPS)
    b, s, l, m = _rows("cf_apart")
    assert m.tolist() == [1, 1] and np.array_equal(s, np.array([f32(0.9) / f32(2), f32(0.6) / f32(2)], f32))
    assert np.array_equal(b, np.array([(0, 0, 10, 10), (51, 0, 61, 10)], f32))
    c = case("cf_single")
    b, s, l, m = _rows("cf_single")
    assert m.tolist() == [1] and l.tolist() == [5]
    assert s.tobytes() == c["scores"][0].tobytes() and b.tobytes() == c["boxes"][0].tobytes()      # bit for bit
    b, s, l, m = _rows("cf_on_thresh")
    assert wr.iou32(np.array([(0, 0, 10, 10)], f32), np.array((0, 0, 10, 5), f32))[0] == f32(0.5) == f32(case("cf_on_thresh")["thresh"])
    assert m.tolist() == [1, 1]
    assert _rows("cf_labels")[3].tolist() == [1, 1] and _rows("cf_labels")[2].tolist() == [1, 2]
    b, s, l, m = _rows("cf_best")
    assert sorted(expected("cf_best")[5][0]) == [[0], [1, 2]]             # the candidate (flattened index 2) joined B (index 1)


@pytest.mark.parametrize("name", RANDOM)
def test_every_random_case_meets_the_input_condition_of_the_float64_comparison(name):
    groups, margin = expected64(name)
    sizes = [len(c["members"]) for c in groups[0]]
    print(name, "clusters", len(sizes), "largest", max(sizes), "margin", margin)
    assert margin >= 1e-4, margin
    assert len(sizes) >= 12 and max(sizes) >= 8 and min(sizes) == 1      # long clusters and singletons


@pytest.mark.parametrize("name", RANDOM)
def test_the_float32_restatement_agrees_with_the_float64_algorithm(name):
    c = case(name)
    ob, os_, ol, oc, om, mem = _fuse_ref(c, d_out=192)
    groups, _ = expected64(name)
    clusters = groups[0]
    assert int(oc[0]) == len(clusters) == len(mem[0])
    by_first = {cl["members"][0]: cl for cl in clusters}                   # (output order may differ between scores a rounding apart)
    worst_box = worst_score = 0.0
    for r in range(int(oc[0])):
        cl = by_first[mem[0][r][0]]
        assert mem[0][r] == cl["members"]                                  # the same boxes, joined in the same order
        T = len(cl["members"])
        assert int(om[0, r]) == T and int(ol[0, r]) == cl["label"]
        eb = np.abs(ob[0, r].astype(np.float64) - cl["box"]).max()
        es = abs(float(os_[0, r]) - cl["score"])
        worst_box, worst_score = max(worst_box, eb), max(worst_score, es)
        assert eb <= (2 * T + 3) * EPS * np.abs(cl["box"]).max(), (r, T, eb)
        assert es <= (T + 2) * EPS, (r, T, es)
    print(name, "worst box difference", worst_box, "worst score difference", worst_score)


DEFECT_CASES = ("cf_pair", "cf_apart", "cf_single", "cf_on_thresh", "cf_labels", "cf_best", "r101_w111", "r102_w211", "weights_skip")


@pytest.mark.parametrize("defect", wr.DEFECTS)
def test_a_planted_defect_moves_the_restatement(defect):
    moved = []
    for name in DEFECT_CASES:
        good, bad = expected(name), _fuse_ref(case(name), defect=defect)
        if any(x.tobytes() != y.tobytes() for x, y in zip(good[:5], bad[:5])):
            moved.append(name)
    print(defect, "visible on", moved)
    assert moved, defect


def test_argument_errors_without_a_gpu():
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt)      # noqa: E731
    args = (z(2, 8, 4), z(2, 8), z(2, 8, dt=torch.int64), z(2, dt=torch.int32), z(2, 2), [0, 2])
    with pytest.raises(ValueError, match="GPU"):
        fusion.fuse_detections(*args)                                              # CPU tensors
    for kw in (dict(thresh=float("nan")), dict(thresh=-0.1), dict(skip_thresh=float("nan")), dict(skip_thresh=-1.0)):
        with pytest.raises(ValueError, match="thresh"):
            fusion.fuse_detections(*args, **kw)
    with pytest.raises(ValueError, match="8192"):
        fusion.check_fuse_limits(17, 512)
    with pytest.raises(ValueError, match="512"):
        fusion.check_fuse_limits(1, 513)
    m = models.ssdlite320_mobilenet_v3_large(num_classes=21)
    other = models.ssdlite320_mobilenet_v3_large(num_classes=5)
    m.eval(), other.eval()
    img = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match="nothing to fuse"):
        m.detect_tta(img, hflip=False)
    with pytest.raises(ValueError, match="nothing to fuse"):
        fusion.ensemble_detect([m], img)
    for kw in (dict(fuse="soft"), dict(thresh=float("nan")), dict(skip_thresh=-0.5)):
        with pytest.raises(ValueError):
            m.detect_tta(img, **kw)
    for bad in (torch.zeros(3, 64, 64), [torch.zeros(1, 64, 64)], [torch.zeros(3, 64, 64, dtype=torch.uint8)]):
        with pytest.raises(ValueError):
            m.detect_tta(bad)
    with pytest.raises(ValueError, match="num_classes"):
        fusion.ensemble_detect([m, other], img)
    for w in ((1.0,), (1.0, -1.0), (1.0, float("nan")), (0.0, 1.0)):
        with pytest.raises(ValueError, match="weights"):
            fusion.ensemble_detect([m, m], img, weights=w)
    with pytest.raises(ValueError):
        fusion.ensemble_detect([], img)
    m.train()
    with pytest.raises(ValueError, match="eval"):
        m.detect_tta(img)


# ----------------------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------------------
def _fuse(c, ws_bytes=None, want_members=True, **over):
    """One dn_fuse_detections call on the case -> (return code, five numpy outputs). Workspace and outputs are pre-filled with 0xFF bytes (NaN)."""
    c = dict(c, **over)
    L = _lib.lib()
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("boxes", "scores", "labels", "counts", "offsets")}
    w = torch.from_numpy(c["weights"]).cuda() if c["weights"] is not None else None
    S, d = c["scores"].shape
    S, d = over.get("s_total", S), over.get("d", d)
    gb = c["group_begin"]
    G, d_out = len(gb) - 1, c["d_out"]
    gb_c = (C.c_int32 * (G + 1))(*gb)
    need = L.dn_fuse_detections_workspace_bytes(S, d, gb_c, G)
    ws = torch.full((max(need if ws_bytes is None else ws_bytes, 16),), 0xFF, dtype=torch.uint8, device="cuda")
    rows = max(d_out, 1)
    ob = torch.full((G, rows, 4), float("nan"), dtype=torch.float32, device="cuda")
    os_ = torch.full((G, rows), float("nan"), dtype=torch.float32, device="cuda")
    ol = torch.full((G, rows), -1, dtype=torch.int64, device="cuda")
    oc = torch.full((G,), -1, dtype=torch.int32, device="cuda")
    om = torch.full((G, rows), -7, dtype=torch.int32, device="cuda")
    p = C.c_void_p
    ptr = {k: p(v.data_ptr()) for k, v in t.items()}
    ptr.update({k: None for k in over.get("null", ())})
    rc = L.dn_fuse_detections(ptr["boxes"], ptr["scores"], ptr["labels"], ptr["counts"], ptr["offsets"], p(w.data_ptr()) if w is not None else None,
                              S, d, gb_c, G, c["thresh"], c["skip"], d_out, p(ob.data_ptr()), p(os_.data_ptr()), p(ol.data_ptr()), p(oc.data_ptr()),
                              p(om.data_ptr()) if want_members else None, p(ws.data_ptr()), ws.numel() if ws_bytes is None else ws_bytes,
                              p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, [x.cpu().numpy() for x in (ob, os_, ol, oc, om)], need


def _assert_same(want, got):
    for w, g, what in zip(want[:5], got, ("boxes", "scores", "labels", "counts", "members")):
        assert w.shape == g.shape, what
        if w.dtype == np.float32:
            w, g = np.ascontiguousarray(w).view(np.int32), g.view(np.int32)
        assert np.array_equal(w, g), what


SMALL = ("cf_pair", "cf_apart", "cf_single", "cf_on_thresh", "cf_labels", "cf_best") + tuple("ragged_{}".format(s) for s in SEEDS) + (
    "nan_scores", "weights_skip", "two_groups_outside", "same_source_twice", "three_tables")


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_fuse_detections_equals_the_restatement_bit_for_bit(name):
    c = case(name)
    want = expected(name)
    if name.startswith("ragged_"):
        assert int(want[3][0]) > 0 and int(want[3][1]) == 0
    if name == "same_source_twice":
        assert (want[4][0, :int(want[3][0])] % 2 == 0).all()               # every box met its duplicate
    if name == "three_tables":
        gb, oc, om = c["group_begin"], want[3], want[4]
        assert len(gb) - 1 == 131 and gb[64] == gb[65] and int(oc[64]) == 0 and gb[-1] < c["scores"].shape[0] and c["d_out"] > c["scores"].shape[1]
        for lo, hi in ((0, 64), (64, 128), (128, 131)):                    # every table fuses a pair and leaves a box alone
            assert (om[lo:hi] >= 2).any() and (om[lo:hi] == 1).any(), (lo, hi)
        assert len(set(c["counts"].tolist())) == 5 and len(set(c["weights"].tolist())) == 4
    rc, got, _ = _fuse(c)
    assert rc == 0, _lib.lib().dn_last_error()
    _assert_same(want, got)
    rc, plain, _ = _fuse(c, want_members=False)                             # members_out is optional
    assert rc == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(got[:4], plain[:4])) and bool((plain[4] == -7).all())


@pytest.mark.gpu
def test_fuse_detections_through_the_tensor_api():
    c = case("two_groups_outside")
    t = [torch.from_numpy(c[k]).cuda() for k in ("boxes", "scores", "labels", "counts", "offsets")]
    out = fusion.fuse_detections(*t, c["group_begin"], torch.from_numpy(c["weights"]).cuda(), c["thresh"], c["skip"], c["d_out"], return_members=True)
    _assert_same(expected("two_groups_outside"), [x.cpu().numpy() for x in out])
    assert len(fusion.fuse_detections(*t, c["group_begin"], None, c["thresh"], c["skip"], c["d_out"])) == 4
    with pytest.raises(ValueError):
        fusion.fuse_detections(*t, [0, 8])                                  # beyond S
    with pytest.raises(ValueError):
        fusion.fuse_detections(*t, c["group_begin"], torch.ones(3, device="cuda"))      # weights of the wrong length


@pytest.mark.gpu
@pytest.mark.parametrize("d_out", [512, 7])
@pytest.mark.parametrize("n", sorted(SIZES))
def test_fuse_detections_where_every_candidate_is_a_cluster(n, d_out):
    """63, 64, 65: the owner lane wraps; 255 .. 257: the ranking's blocks; 8 192: the limit, clusters beyond the walk's LDS table."""
    name = "disjoint_{}".format(n)
    want = expected(name)
    assert (want[4][0, :min(n, 512)] == 1).all() and int(want[3][0]) == min(n, 512)
    rc, got, _ = _fuse(case(name), d_out=d_out)
    assert rc == 0, _lib.lib().dn_last_error()
    _assert_same(_truncated(want, d_out), got)


@pytest.mark.gpu
def test_fuse_detections_long_clusters():
    want = expected("long_clusters")
    n = int(want[3][0])
    assert 8 <= n <= 64 and int(want[4][0, :n].max()) >= 200 and int(want[4][0, :n].sum()) == 2048
    rc, got, _ = _fuse(case("long_clusters"))
    assert rc == 0, _lib.lib().dn_last_error()
    _assert_same(want, got)


@pytest.mark.gpu
def test_fuse_detections_is_deterministic():
    c = case("disjoint_8192")
    rc, a, _ = _fuse(c)
    rc2, b, _ = _fuse(c)
    assert rc == 0 and rc2 == 0
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    c = case("long_clusters")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(_fuse(c)[1], _fuse(c)[1]))


@pytest.mark.gpu
def test_fuse_detections_rejections():
    INVALID, WORKSPACE, UNSUPPORTED = -1, -3, -4

    def tiny(S, d, **kw):
        return _case(np.zeros((S, d, 4), f32), np.zeros((S, d), f32), np.zeros((S, d), np.int64), counts=[0] * S, d_out=8, **kw)
    for refused, code in ((tiny(1, 513), UNSUPPORTED),                              # d = 513
                          (tiny(17, 512), UNSUPPORTED),                             # 8 704 slots in one group
                          (tiny(8193, 1), UNSUPPORTED),                             # 8 193 slots in one group
                          (tiny(4, 8, group_begin=[0, 3, 2, 4]), INVALID),          # a decreasing group_begin
                          (tiny(4, 8, group_begin=[0, 5]), INVALID),                # beyond s_total
                          (tiny(4, 8, group_begin=[-1, 4]), INVALID)):
        rc, _, need = _fuse(refused)
        assert rc == code and need == 0, (refused["scores"].shape, refused["group_begin"], rc, need)
    assert _fuse(tiny(8192, 1))[0] == 0
    assert _fuse(tiny(32, 512, group_begin=[0, 16, 32]))[0] == 0                    # ... two groups of 8 192 are fine
    assert _fuse(tiny(2, 8), d_out=0)[0] == INVALID
    assert _fuse(tiny(2, 8), d_out=513)[0] == UNSUPPORTED
    assert _fuse(tiny(2, 8), ws_bytes=16)[0] == WORKSPACE
    rc, _, need = _fuse(tiny(2, 8))
    assert rc == 0 and need > 0 and _fuse(tiny(2, 8), ws_bytes=need - 1)[0] == WORKSPACE
    for kw in (dict(thresh=float("nan")), dict(thresh=-0.25), dict(skip=float("nan")), dict(skip=-0.25)):
        assert _fuse(tiny(2, 8), **kw)[0] == INVALID, kw
    for k in ("boxes", "scores", "labels", "counts", "offsets"):
        assert _fuse(tiny(2, 8), null=(k,))[0] == INVALID, k
    # misalignment, as the merge checks it: boxes 16 bytes, labels 8 bytes
    L, p = _lib.lib(), C.c_void_p
    c = tiny(2, 8)
    t = {k: torch.from_numpy(c[k]).cuda() for k in ("boxes", "scores", "labels", "counts", "offsets")}
    gb_c = (C.c_int32 * 2)(0, 2)
    ws = torch.empty(L.dn_fuse_detections_workspace_bytes(2, 8, gb_c, 1) + 16, dtype=torch.uint8, device="cuda")
    ob, os_, ol, oc = (torch.zeros(s, dtype=dt, device="cuda") for s, dt in (((1, 9, 4), torch.float32), ((1, 8), torch.float32), ((1, 9), torch.int64),
                                                                             ((1,), torch.int32)))
    for shift in (dict(boxes=4), dict(labels=4), dict(ob=4), dict(ol=4), dict(ws=4), dict(offsets=4), dict()):
        rc = L.dn_fuse_detections(p(t["boxes"].data_ptr() + shift.get("boxes", 0)), p(t["scores"].data_ptr()), p(t["labels"].data_ptr() + shift.get("labels", 0)),
                                  p(t["counts"].data_ptr()), p(t["offsets"].data_ptr() + shift.get("offsets", 0)), None, 2, 8, gb_c, 1, 0.5, 0.0,
                                  8, p(ob.data_ptr() + shift.get("ob", 0)), p(os_.data_ptr()), p(ol.data_ptr() + shift.get("ol", 0)), p(oc.data_ptr()), None,
                                  p(ws.data_ptr() + shift.get("ws", 0)), ws.numel() - 16, None)
        torch.cuda.synchronize()
        assert rc == (INVALID if shift else 0), shift


# ----------------------------------------------------------------------------------------------------------------------------------
# model level
# ----------------------------------------------------------------------------------------------------------------------------------
IMG_SEED = 2024
SCORE_THRESH = 0.4           # synthetic weights, K = 21: 24 .. 48 detections per pass on these images (300, the cap, at 0.2; under 10 at 0.5)


@pytest.fixture(scope="module")
def model():
    return models.load_synthetic(models.ssdlite320_mobilenet_v3_large(num_classes=21, score_thresh=SCORE_THRESH), 0).cuda().eval()


@functools.lru_cache(maxsize=None)
def _images(n=3, h=300, w=420, seed=IMG_SEED):
    return torch.from_numpy(synth.images(seed, n, h, w)).cuda()


def _np(outs):
    return [t.cpu().numpy().copy() for t in outs]


def _compose_tta(model, imgs):
    """What a user writes by hand today: the two forwards, detections to the host, un-flip and fusion there."""
    n, W = imgs.shape[0], f32(imgs.shape[3])
    pb, ps, pl, pc = _np(model.forward_batch(imgs))
    fb, fs, fl, fc = _np(model.forward_batch(torch.flip(imgs, [-1])))
    ub = np.stack([W - fb[..., 2], fb[..., 1], W - fb[..., 0], fb[..., 3]], -1).astype(f32)
    il = lambda a, b: np.stack([a, b], 1).reshape((2 * n,) + a.shape[1:])      # noqa: E731  sources 2 g, 2 g + 1 = group g
    return il(pb, ub), il(ps, fs), il(pl, fl), il(pc, fc)


def _same(det, boxes, scores, labels):
    return (np.array_equal(det["boxes"].cpu().numpy().view(np.int32), np.ascontiguousarray(boxes).view(np.int32))
            and np.array_equal(det["scores"].cpu().numpy().view(np.int32), np.ascontiguousarray(scores).view(np.int32))
            and np.array_equal(det["labels"].cpu().numpy(), labels))


@pytest.mark.gpu
def test_detect_tta_equals_the_hand_written_composition(model):
    imgs = _images()
    n, D = imgs.shape[0], model.detections_per_img
    b, s, l, c = _compose_tta(model, imgs)
    print("counts per source", c.tolist())
    assert 10 <= c.min() and c.max() < D                                          # dozens, and the forward's own cap is not in play
    gb = list(range(0, 2 * n + 1, 2))
    ob, os_, ol, oc, om, _ = wr.fuse(b, s, l, c, np.zeros((2 * n, 2), f32), gb, None, model.nms_thresh, model.score_thresh, D)
    print("fused counts", oc.tolist(), "rows with two members", [int((om[g] == 2).sum()) for g in range(n)])
    assert (om == 2).any() and (om == 1).any()
    out = model.detect_tta(imgs)
    assert len(out) == n
    for g in range(n):
        k = int(oc[g])
        assert _same(out[g], ob[g, :k], os_[g, :k], ol[g, :k]), g
    # fuse="nms": merge_detections on the same staging
    t = [torch.from_numpy(x).cuda() for x in (b, s, l, c)]
    mb, ms, ml, mc = _np(sliced.merge_detections(*t, torch.zeros((2 * n, 2), device="cuda"), gb, model.nms_thresh, "iou", False, D))
    out = model.detect_tta(list(imgs), fuse="nms")
    for g in range(n):
        k = int(mc[g])
        assert k > 0 and _same(out[g], mb[g, :k], ms[g, :k], ml[g, :k]), g


@pytest.mark.gpu
def test_detect_tta_list_of_two_sizes_equals_the_single_calls(model):
    a, b = _images()[0], _images(1, 260, 350, IMG_SEED + 1)[0]
    both = model.detect_tta([a, b, a])
    one = [model.detect_tta([a])[0], model.detect_tta(b[None])[0]]
    assert len(both) == 3
    for x, y in zip(both, one + one[:1]):
        assert x["scores"].numel() > 0
        for k in ("boxes", "scores", "labels"):
            assert torch.equal(x[k], y[k]), k


@pytest.mark.gpu
def test_ensemble_of_a_model_with_itself_returns_its_own_detections(model):
    imgs = _images()
    pb, ps, pl, pc = _np(model.forward_batch(imgs))
    out = fusion.ensemble_detect([model, model], imgs, weights=(1, 1))
    for g in range(imgs.shape[0]):
        k = int(pc[g])
        assert k > 0 and out[g]["scores"].numel() == k                             # same rows, same order
        assert np.array_equal(out[g]["scores"].cpu().numpy().view(np.int32), ps[g, :k].view(np.int32))      # (v + v) / 2 * 2 / 2 = v
        assert np.array_equal(out[g]["labels"].cpu().numpy(), pl[g, :k])
        got, want = out[g]["boxes"].cpu().numpy(), pb[g, :k]
        assert (np.abs(got - want) <= 2 * np.spacing(np.abs(want))).all()           # (v x + v x) / (v + v) rounds twice
    t = [torch.from_numpy(np.repeat(x, 2, 0)).cuda() for x in (pb, ps, pl, pc)]     # ... and every row has two members
    n = imgs.shape[0]
    om = fusion.fuse_detections(*t, torch.zeros((2 * n, 2), device="cuda"), list(range(0, 2 * n + 1, 2)), None, model.nms_thresh, model.score_thresh,
                                return_members=True)[4].cpu().numpy()
    for g in range(n):
        assert (om[g, :pc[g]] == 2).all() and (om[g, pc[g]:] == 0).all()


@pytest.mark.gpu
def test_fusing_a_single_forward_returns_it_bit_for_bit(model):
    """The per-class NMS has left no same-label pair above nms_thresh: every detection is a cluster of its own."""
    imgs = _images()
    n = imgs.shape[0]
    outs = [t.clone() for t in model.forward_batch(imgs)]
    fb, fs, fl, fc, fm = fusion.fuse_detections(*outs, torch.zeros((n, 2), device="cuda"), list(range(n + 1)), None, model.nms_thresh, 0.0,
                                                return_members=True)
    assert torch.equal(fc, outs[3]) and int(fc.min()) > 0
    for g, k in enumerate(fc.tolist()):
        assert torch.equal(fb[g, :k].view(torch.int32), outs[0][g, :k].view(torch.int32))
        assert torch.equal(fs[g, :k].view(torch.int32), outs[1][g, :k].view(torch.int32)) and torch.equal(fl[g, :k], outs[2][g, :k])
        assert bool((fm[g, :k] == 1).all()) and bool((fm[g, k:] == 0).all())


@pytest.mark.gpu
def test_detect_tta_and_ensemble_leave_the_plain_forward_as_it_was(model):
    imgs = [_images()[0], _images(1, 260, 350, IMG_SEED + 1)[0]]
    before = model(imgs)
    gen, handle = model._plan_gen, model._handle
    model.detect_tta(imgs)
    model.detect_tta(imgs, fuse="nms", hflip=False)
    fusion.ensemble_detect([model, model], imgs, weights=(2, 1), hflip=True)
    after = model(imgs)
    assert (model._plan_gen, model._handle) == (gen, handle)                       # the plan was not rebuilt
    for x, y in zip(before, after):
        for k in ("boxes", "scores", "labels"):
            assert torch.equal(x[k], y[k]), k
