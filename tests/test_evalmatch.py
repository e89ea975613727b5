"""VOC scoring on the device: dn_match_detections, demonet_amd/voceval.py and engine.evaluate_voc.

CPU part: the reference (tests/evalmatch_ref.py, the sequential walk) is held to the vectors the reference project's own voc_eval produced
(tests/golden/voc_eval.npz) through VocAccumulator.append + summarize, and to evalrec.voc_class_pr / voc_mean_ap on random tie-free sets.
GPU part: the kernel against that reference, exactly -- flags and best_gt for equality, best_ov by bit pattern, outputs pre-filled with 0xFF
bytes -- on the golden set, on designed edges, on every rejection, and end to end through engine.evaluate_voc."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import evalmatch_ref as er
from demonet_amd import _lib, evalrec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voc_eval.npz")
f32 = np.float32


# ----------------------------------------------------------------------------------------------------------------------------------
# the golden set as one padded image set
# ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden_set():
    """voc_eval.npz as one set: class ci becomes label ci + 1, detections and scores rounded to fp32, d = 16"""
    z = np.load(GOLDEN)
    n = max(int(z["ve_num_images"]), 1 + max(int(z[f"ve_{w}_img_{ci}"].max()) for ci in range(3) for w in ("det", "gt")))
    dets = [dict(boxes=[], scores=[], labels=[]) for _ in range(n)]
    gts = [dict(boxes=[], labels=[], difficult=[]) for _ in range(n)]
    for ci in range(3):
        for img, s, b in zip(z[f"ve_det_img_{ci}"], z[f"ve_det_score_{ci}"], z[f"ve_det_box_{ci}"]):
            dets[img]["boxes"].append(b.astype(f32)); dets[img]["scores"].append(f32(s)); dets[img]["labels"].append(ci + 1)
        for img, df, b in zip(z[f"ve_gt_img_{ci}"], z[f"ve_gt_diff_{ci}"], z[f"ve_gt_box_{ci}"]):
            gts[img]["boxes"].append(b.astype(f32)); gts[img]["labels"].append(ci + 1); gts[img]["difficult"].append(int(df))
    assert max(len(r["scores"]) for r in dets) <= 14
    return dict(det=er.pad_records(dets, 16), gt=er.pad_gt(gts), thresholds=(0.5, 0.3), num_classes=4, z={k: z[k] for k in z.files if k.startswith("ve_")})


def _accumulate(scores, labels, counts, flags, stats, num_classes, thresholds):
    from demonet_amd import voceval
    acc = voceval.VocAccumulator(num_classes, thresholds)
    acc.append(torch.from_numpy(scores), torch.from_numpy(labels), torch.from_numpy(counts), torch.from_numpy(flags.view(np.int32)), torch.from_numpy(stats))
    return acc


def _assert_golden(acc, z):
    """the accumulator's per-class vectors and APs are the reference voc_eval's, exactly"""
    for use07, key in ((False, "ve_ap"), (True, "ve_ap07")):
        s = acc.summarize(use_07_metric=use07)
        assert sorted(s["ap"]) == [1, 2, 3]
        for ci in range(3):
            for b, tag in enumerate(("t50", "t30")):
                assert s["ap"][ci + 1][b] == 100.0 * float(z[f"{key}_{ci}_{tag}"]), (key, ci, tag)
        for b in range(2):
            assert s["map"][b] == float(np.mean([s["ap"][c][b] for c in (1, 2, 3)]))
        assert s["map_avg"] == float(np.mean(s["map"]))
    for ci in range(3):
        for b, tag in enumerate(("t50", "t30")):
            rec, prec = acc.class_pr(ci + 1, b)
            np.testing.assert_array_equal(rec, z[f"ve_rec_{ci}_{tag}"])
            np.testing.assert_array_equal(prec, z[f"ve_prec_{ci}_{tag}"])


# ----------------------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------------------
def test_binding_exists_and_pad_targets_refuses_1025_boxes():
    from demonet_amd import voceval
    assert "dn_match_detections" in _lib.EXPORTS
    for name in ("pad_targets", "match_detections", "VocAccumulator"):
        assert callable(getattr(voceval, name))
    assert hasattr(C.CDLL(_lib.LIB_PATH), "dn_match_detections")
    t = {"boxes": torch.zeros(1025, 4), "labels": torch.ones(1025, dtype=torch.int64)}
    with pytest.raises(ValueError):
        voceval.pad_targets([t], "cpu")
    gb, gl, gd, gc = voceval.pad_targets([{"boxes": torch.ones(2, 4), "labels": torch.tensor([3, 4]), "difficult": torch.tensor([0, 1])},
                                          {"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.int64)},
                                          {"boxes": torch.full((3, 4), 2.0), "labels": torch.tensor([5, 6, 7])}], "cpu")
    assert tuple(gb.shape) == (3, 3, 4) and gb.dtype == torch.float32 and gl.dtype == torch.int64 and gd.dtype == torch.uint8 and gc.dtype == torch.int32
    assert gc.tolist() == [2, 0, 3] and gl.tolist() == [[3, 4, 0], [0, 0, 0], [5, 6, 7]] and gd.tolist() == [[0, 1, 0], [0, 0, 0], [0, 0, 0]]
    assert gb[0].tolist() == [[1.0] * 4, [1.0] * 4, [0.0] * 4] and gb[2].tolist() == [[2.0] * 4] * 3


def test_reference_reproduces_the_golden_voc_eval_vectors():
    g = golden_set()
    boxes, scores, labels, counts = g["det"]
    flags, _, _, stats = er.match_ref(boxes, scores, labels, counts, *g["gt"], g["thresholds"], 1.0, g["num_classes"])
    assert flags[np.arange(16)[None, :] >= counts[:, None]].max() == 0
    _assert_golden(_accumulate(scores, labels, counts, flags, stats, g["num_classes"], g["thresholds"]), g["z"])


def _random_set(seed):
    """A small tie-free image set: labels 1 .. 4 at random, class 5 with difficult ground truths only, class 6 with ground truth and no detection"""
    rng = np.random.default_rng(seed)
    n, d = int(rng.integers(1, 6)), 12
    all_scores = rng.permutation(np.linspace(0.02, 0.98, n * d).astype(f32)).reshape(n, d)
    dets, gts = [], []
    for i in range(n):
        g = int(rng.integers(0, 6))
        xy = rng.uniform(0, 200, (g, 2))
        gb = np.concatenate([xy, xy + rng.uniform(10, 80, (g, 2))], 1).astype(f32)
        gl = rng.integers(1, 5, g)
        gd = rng.random(g) < 0.25
        extra = int(rng.integers(0, 3))                       # the two special classes
        xy = rng.uniform(0, 200, (2 * extra, 2))
        gb = np.concatenate([gb, np.concatenate([xy, xy + 40], 1).astype(f32)])
        gl = np.concatenate([gl, [5] * extra, [6] * extra]).astype(np.int64)
        gd = np.concatenate([gd, [True] * extra, [False] * extra])
        c = int(rng.integers(0, d + 1))
        src = rng.integers(0, max(len(gl), 1), c)
        db = np.zeros((c, 4), f32)
        dl = np.zeros(c, np.int64)
        for j in range(c):
            if len(gl) and rng.random() < 0.7 and gl[src[j]] != 6:        # near a ground truth (duplicates happen), else anywhere
                db[j] = gb[src[j]] + rng.normal(0, 4, 4).astype(f32)
                dl[j] = gl[src[j]]
            else:
                xy = rng.uniform(0, 200, 2)
                db[j] = np.concatenate([xy, xy + rng.uniform(10, 80, 2)])
                dl[j] = rng.integers(1, 6)
        dets.append(dict(boxes=db, scores=all_scores[i, :c], labels=dl))
        gts.append(dict(boxes=gb, labels=gl, difficult=gd))
    return dets, gts


def test_reference_and_summarize_equal_evalrec_on_random_tie_free_sets():
    thresholds = (0.5, 0.3)
    seen_only_difficult = seen_no_detection = n_flags = 0
    for seed in range(200):
        dets, gts = _random_set(seed)
        boxes, scores, labels, counts = er.pad_records(dets, 12)
        flags, _, _, stats = er.match_ref(boxes, scores, labels, counts, *er.pad_gt(gts), thresholds, 1.0, 8)
        acc = _accumulate(scores, labels, counts, flags, stats, 8, thresholds)
        n_flags += int(counts.sum())
        # the marking: recall / precision per detection in confidence order are voc_class_pr's, number for number -- the two cumulative sums
        # fix every TP and FP flag
        for c in sorted({int(x) for g in gts for x in g["labels"]}):
            ids = [i for i, r in enumerate(dets) for l in r["labels"] if l == c]
            if not ids:
                continue
            ds = np.concatenate([r["scores"][r["labels"] == c] for r in dets])
            db = np.concatenate([r["boxes"][r["labels"] == c] for r in dets])
            gt = {i: (g["boxes"][g["labels"] == c], g["difficult"][g["labels"] == c]) for i, g in enumerate(gts)}
            for b, t in enumerate(thresholds):
                rec, prec = evalrec.voc_class_pr(ids, ds, db, gt, t)
                got_rec, got_prec = acc.class_pr(c, b)
                np.testing.assert_array_equal(got_rec, rec)
                np.testing.assert_array_equal(got_prec, prec)
        for use07 in (False, True):
            s = acc.summarize(use_07_metric=use07)
            for b, t in enumerate(thresholds):
                want_map, want_ap = evalrec.voc_mean_ap(dets, gts, t, use07)
                assert s["map"][b] == want_map and {c: v[b] for c, v in s["ap"].items()} == want_ap, (seed, t, use07)
        seen_only_difficult += int(stats[5, 1] > 0 and stats[5, 0] == 0)
        seen_no_detection += int(stats[6, 0] > 0)
    assert seen_only_difficult > 50 and seen_no_detection > 50 and n_flags > 3000


# ----------------------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _call(dev, n_, d_, gmax_, classes_, thr_host, offset_, outs, **override):
    """dn_match_detections through ctypes; dev: dict of device tensors (None = NULL); override: replace any raw argument"""
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    thr = (C.c_double * len(thr_host))(*thr_host)
    a = dict(boxes=p(dev["boxes"]), scores=p(dev["scores"]), labels=p(dev["labels"]), counts=p(dev["counts"]), gt_boxes=p(dev["gt_boxes"]),
             gt_labels=p(dev["gt_labels"]), gt_difficult=p(dev["gt_difficult"]), gt_counts=p(dev["gt_counts"]), n=n_, d=d_, gmax=gmax_, num_classes=classes_,
             thresholds=thr, n_thresh=len(thr_host), offset=float(offset_), flags=p(outs["flags"]), best_gt=p(outs["best_gt"]), best_ov=p(outs["best_ov"]),
             gt_stats=p(outs["gt_stats"]), stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    a.update(override)
    return _lib.lib().dn_match_detections(*a.values())


def _outputs(n, d, num_classes, stats=True):
    """every output pre-filled with 0xFF bytes, except gt_stats (which the call adds to): zero"""
    ff = lambda shape, dt: torch.full(shape, -1, dtype=dt, device="cuda:0")
    return dict(flags=ff((n, d), torch.int32), best_gt=ff((n, d), torch.int32), best_ov=ff((n, d), torch.int64),
                gt_stats=torch.zeros((num_classes, 2), dtype=torch.int64, device="cuda:0") if stats else None)


def _run_and_compare(case, null_difficult=False):
    boxes, scores, labels, counts = case["det"]
    gb, gl, gd, gc = case["gt"]
    thr, off, K = case["thresholds"], case.get("offset", 1.0), case["num_classes"]
    n, d = scores.shape
    dev = dict(boxes=_dev(boxes), scores=_dev(scores), labels=_dev(labels), counts=_dev(counts), gt_boxes=_dev(gb), gt_labels=_dev(gl),
               gt_difficult=None if null_difficult else _dev(gd), gt_counts=_dev(gc))
    outs = _outputs(n, d, K)
    assert _call(dev, n, d, gb.shape[1], K, thr, off, outs) == 0, _lib.lib().dn_last_error()
    torch.cuda.synchronize()
    want = er.match_ref(boxes, scores, labels, counts, gb, gl, None if null_difficult else gd, gc, thr, off, K)
    got_flags = outs["flags"].cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(got_flags, want[0])
    np.testing.assert_array_equal(outs["best_gt"].cpu().numpy(), want[1])
    np.testing.assert_array_equal(outs["best_ov"].cpu().numpy(), want[2].view(np.int64))      # by bit pattern (NaN, -inf, -0 included)
    np.testing.assert_array_equal(outs["gt_stats"].cpu().numpy(), want[3])
    return got_flags, want


@pytest.mark.gpu
def test_gpu_golden_set_gives_the_reference_voc_eval_vectors():
    """the kernel against the reference project's own voc_eval: flags from dn_match_detections, accumulated on the device, give ve_* exactly"""
    from demonet_amd import voceval
    g = golden_set()
    _run_and_compare(g)
    acc = voceval.VocAccumulator(g["num_classes"], g["thresholds"])
    det = [_dev(a) for a in g["det"]]
    acc.update(*det, tuple(_dev(a) for a in g["gt"]))
    _assert_golden(acc, g["z"])
    # and through the reference's target dicts
    gb, gl, gd, gc = g["gt"]
    targets = [dict(boxes=torch.from_numpy(gb[i, :gc[i]]), labels=torch.from_numpy(gl[i, :gc[i]]), difficult=torch.from_numpy(gd[i, :gc[i]])) for i in range(len(gc))]
    acc2 = voceval.VocAccumulator(g["num_classes"], g["thresholds"])
    acc2.update(*det, targets)
    assert acc2.summarize() == acc.summarize()


def _clutter(seed, cg, d, gmax, n_labels=3, shuffle=True, ties=False, diff=0.2):
    """images with (c, g) from cg: ground truths around a few centres, candidates = jittered ground truths and strays, rows beyond the counts garbage"""
    rng = np.random.default_rng(seed)
    n = len(cg)
    ctr = rng.uniform(50, 900, (n, gmax, 2))
    wh = rng.uniform(20, 120, (n, gmax, 2))
    gb = np.concatenate([ctr - wh / 2, ctr + wh / 2], -1).astype(f32)
    gl = rng.integers(1, n_labels + 1, (n, gmax)).astype(np.int64)
    gd = (rng.random((n, gmax)) < diff).astype(np.uint8)
    src = rng.integers(0, gmax, (n, d))
    boxes = np.take_along_axis(gb, src[..., None], 1) + rng.normal(0, 5.0, (n, d, 4)).astype(f32)
    labels = np.take_along_axis(gl, src, 1)
    for i, (c, g) in enumerate(cg):                       # candidates point at live ground truths where there are some
        if g:
            s = src[i] % g
            boxes[i] = gb[i, s] + rng.normal(0, 5.0, (d, 4)).astype(f32)
            labels[i] = gl[i, s]
    stray = rng.random((n, d)) < 0.2
    labels[stray] = rng.integers(1, n_labels + 2, int(stray.sum()))      # (label n_labels + 1 has no ground truth)
    scores = rng.uniform(0.01, 1.0, (n, d)).astype(f32)
    if ties:
        scores = (np.round(scores * 8) / 8).astype(f32)
    if not shuffle:
        scores = np.sort(scores, 1)[:, ::-1].copy()
    return dict(det=(boxes.astype(f32), scores, labels, np.array([c for c, _ in cg], np.int32)), gt=(gb, gl, gd, np.array([g for _, g in cg], np.int32)),
                thresholds=(0.5,), num_classes=n_labels + 1)


SIZES = [(c, g) for c in (63, 64, 65, 257, 512) for g in (1, 255, 257, 1024)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_thresh", [1, 16])
def test_gpu_sizes_around_the_workgroup(n_thresh):
    """c = 63, 64, 65, 257, 512 with g = 1, 255, 257, 1024 (one image each, one call), shuffled slots, heavy score ties, 1 and 16 thresholds"""
    case = _clutter(5, SIZES + [(0, 7), (9, 0), (0, 0)], 512, 1024, ties=True)
    case["thresholds"] = (0.5,) if n_thresh == 1 else tuple(np.linspace(0.05, 0.95, 16))
    flags, _ = _run_and_compare(case)
    assert (flags & 0xFFFF).any() and (flags >> 16).any() and ((flags[:20, :63] & 0x10001) == 0).any()      # TP, FP and ignored (at the first threshold) all occur


@pytest.mark.gpu
def test_gpu_designed_edges():
    one = lambda *rows: np.array([rows], f32)
    # c = 0 ; g = 0 (every candidate FP, best_ov = -inf) ; d = 1
    f, w = _run_and_compare(_clutter(1, [(0, 5), (6, 0), (8, 8)], 8, 8))
    assert (f[0] == 0).all() and (f[1, :6] == 1 << 16).all() and np.isneginf(w[2][1, :6]).all()
    _run_and_compare(_clutter(2, [(1, 3), (0, 2), (1, 0)], 1, 4))
    _run_and_compare(_clutter(3, [(20, 6)] * 3, 24, 6, shuffle=False), null_difficult=True)          # gt_difficult_dev = NULL, sorted rows
    _run_and_compare(dict(_clutter(4, [(30, 9), (17, 2)], 32, 9), offset=0.0, thresholds=(0.5, 0.7)))      # pixel_offset = 0
    # five candidates on one ground truth with tied scores: the lowest slot is the TP
    gt = (one((10, 10, 50, 50)), np.array([[1]], np.int64), np.zeros((1, 1), np.uint8), np.array([1], np.int32))
    det = (np.tile(one((11, 11, 50, 50)), (1, 5, 1)) + np.arange(5, dtype=f32)[None, :, None] * 0.25, np.full((1, 5), 0.5, f32), np.ones((1, 5), np.int64),
           np.array([5], np.int32))
    f, _ = _run_and_compare(dict(det=det, gt=gt, thresholds=(0.5,), num_classes=2))
    assert f[0].tolist() == [1] + [1 << 16] * 4
    # two identical ground truths: the lower index wins, the second is never claimed
    gt2 = (one((10, 10, 50, 50), (10, 10, 50, 50)), np.array([[1, 1]], np.int64), np.zeros((1, 2), np.uint8), np.array([2], np.int32))
    f, w = _run_and_compare(dict(det=(det[0], np.linspace(0.9, 0.5, 5, dtype=f32)[None], det[2], det[3]), gt=gt2, thresholds=(0.5,), num_classes=2))
    assert (w[1][0] == 0).all() and f[0].tolist() == [1] + [1 << 16] * 4
    # a difficult best match: neither flag ; a candidate whose label has no ground truth ; labels >= num_classes in gt_stats (and negative)
    gt3 = (one((10, 10, 50, 50), (100, 100, 150, 150), (200, 200, 240, 240)), np.array([[1, 2, 7]], np.int64), np.array([[0, 1, 0]], np.uint8), np.array([3], np.int32))
    det3 = (one((101, 99, 150, 151), (14, 14, 50, 50), (12, 12, 50, 50), (200, 200, 240, 240)), np.array([[0.9, 0.8, 0.7, 0.6]], f32),
            np.array([[2, 1, 3, 7]], np.int64), np.array([4], np.int32))
    f, w = _run_and_compare(dict(det=det3, gt=gt3, thresholds=(0.5, 0.9), num_classes=3))
    assert f[0].tolist() == [0, 1 | 1 << 17, 3 << 16, 3] and w[1][0].tolist() == [1, 0, -1, 2] and w[3].tolist() == [[0, 0], [1, 0], [0, 1]]
    gt3n = (gt3[0], np.array([[-1, 2, 1 << 40]], np.int64), gt3[2], gt3[3])
    _run_and_compare(dict(det=det3, gt=gt3n, thresholds=(0.5,), num_classes=3))
    # IoU exactly at the threshold: inter 50, union 100 -> 0.5: FP at 0.5, TP at 0.49
    gt4 = (one((0, 0, 9, 9)), np.array([[1]], np.int64), np.zeros((1, 1), np.uint8), np.array([1], np.int32))
    det4 = (one((0, 0, 9, 4)), np.array([[0.9]], f32), np.array([[1]], np.int64), np.array([1], np.int32))
    f, w = _run_and_compare(dict(det=det4, gt=gt4, thresholds=(0.5, 0.49), num_classes=2))
    assert w[2][0, 0] == 0.5 and f[0, 0] == (1 << 16 | 1 << 1)
    # a NaN coordinate (FP at every threshold, best_ov NaN, best_gt -1) and a NaN score (ranks last: the duplicate with a number wins)
    det5 = (one((12, 12, np.nan, 50), (11, 11, 50, 50), (10, 10, 50, 50), (300, 300, 320, 320)), np.array([[0.9, np.nan, 0.1, np.nan]], f32), np.ones((1, 4), np.int64),
            np.array([4], np.int32))
    f, w = _run_and_compare(dict(det=det5, gt=gt, thresholds=(0.5, 0.1), num_classes=2))
    assert np.isnan(w[2][0, 0]) and w[1][0, 0] == -1 and f[0].tolist() == [3 << 16, 3 << 16, 3, 3 << 16]


@pytest.mark.gpu
def test_gpu_gt_stats_accumulates_over_two_calls():
    case = _clutter(6, [(10, 7), (3, 12), (0, 1)], 16, 12)
    boxes, scores, labels, counts = case["det"]
    gb, gl, gd, gc = case["gt"]
    dev = dict(boxes=_dev(boxes), scores=_dev(scores), labels=_dev(labels), counts=_dev(counts), gt_boxes=_dev(gb), gt_labels=_dev(gl), gt_difficult=_dev(gd),
               gt_counts=_dev(gc))
    outs = _outputs(3, 16, 4)
    for _ in range(2):
        assert _call(dev, 3, 16, 12, 4, (0.5,), 1.0, outs) == 0
    want = er.match_ref(boxes, scores, labels, counts, gb, gl, gd, gc, (0.5,), 1.0, 4)[3]
    assert want.sum() == 20
    np.testing.assert_array_equal(outs["gt_stats"].cpu().numpy(), 2 * want)
    # the optional outputs may be NULL
    only = dict(_outputs(3, 16, 4), best_gt=None, best_ov=None, gt_stats=None)
    assert _call(dev, 3, 16, 12, 0, (0.5,), 1.0, only) == 0
    assert torch.equal(only["flags"], outs["flags"])


@pytest.mark.gpu
def test_gpu_rejections_leave_the_outputs_untouched():
    case = _clutter(7, [(10, 7), (3, 12)], 16, 12)
    boxes, scores, labels, counts = case["det"]
    gb, gl, gd, gc = case["gt"]
    dev = dict(boxes=_dev(boxes), scores=_dev(scores), labels=_dev(labels), counts=_dev(counts), gt_boxes=_dev(gb), gt_labels=_dev(gl), gt_difficult=_dev(gd),
               gt_counts=_dev(gc))
    outs = _outputs(2, 16, 4)
    outs["gt_stats"].fill_(-1)
    off = lambda t, k: C.c_void_p(t.data_ptr() + k)
    INVALID, UNSUPPORTED = -1, -4
    nan, inf = float("nan"), float("inf")
    bad = [(dict([(k, None)]), INVALID) for k in ("boxes", "scores", "labels", "counts", "gt_boxes", "gt_labels", "gt_counts", "thresholds", "flags")]
    bad += [(dict([(k, v)]), INVALID) for k in ("n", "d", "gmax", "n_thresh") for v in (0, -3)]
    bad += [(dict(num_classes=0), INVALID), (dict(num_classes=-1), INVALID)]
    bad += [(dict(thresholds=(C.c_double * 2)(0.5, nan), n_thresh=2), INVALID)]
    bad += [(dict(offset=v), INVALID) for v in (nan, inf, -inf, -1.0)]
    bad += [(dict(boxes=off(dev["boxes"], 4)), INVALID), (dict(gt_boxes=off(dev["gt_boxes"], 8)), INVALID), (dict(labels=off(dev["labels"], 4)), INVALID),
            (dict(gt_labels=off(dev["gt_labels"], 4)), INVALID), (dict(best_ov=off(outs["best_ov"], 4)), INVALID), (dict(gt_stats=off(outs["gt_stats"], 4)), INVALID)]
    bad += [(dict(d=513), UNSUPPORTED), (dict(gmax=1025), UNSUPPORTED), (dict(thresholds=(C.c_double * 17)(*([0.5] * 17)), n_thresh=17), UNSUPPORTED),
            (dict(n=65536), UNSUPPORTED)]
    for override, code in bad:
        assert _call(dev, 2, 16, 12, 4, (0.5,), 1.0, outs, **override) == code, override
        assert _lib.lib().dn_last_error()
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == -1).all()), k
    # the limits themselves are taken: n_thresh = 16 ran above; num_classes is not looked at without gt_stats
    assert _call(dev, 2, 16, 12, 0, (0.5,), 0.0, dict(outs, gt_stats=None)) == 0
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_evaluate_voc_end_to_end():
    """engine.evaluate_voc against the reference matcher + summarize on engine.evaluate's host records: three batches of 4 at two image sizes and one
    mixed-size batch, targets = a first forward's top detections jittered by a few pixels, some difficult; thresholds (0.5, 0.75)."""
    from demonet_amd import engine, models, synth, voceval
    model = models.load_synthetic(models.ssdlite320_mobilenet_v3_large(num_classes=21), 0).to("cuda:0")
    D = model.detections_per_img
    sizes = [[(320, 320)] * 4, [(320, 320)] * 4, [(256, 384)] * 4, [(320, 320), (240, 320), (256, 384), (300, 200)]]
    batches, iid = [], 0
    for bi, hw in enumerate(sizes):
        imgs = [torch.from_numpy(synth.images(2000 + 10 * bi + k, 1, h, w)[0]) for k, (h, w) in enumerate(hw)]
        batches.append((imgs, [{"image_id": iid + k} for k in range(4)]))
        iid += 4
    first, _ = engine.evaluate(model, batches)
    rng = np.random.default_rng(0)
    loader = []
    for imgs, tg in batches:
        targets = []
        for t in tg:
            r = first[t["image_id"]]
            k = min(6, len(r["scores"]))
            top = torch.argsort(r["scores"], descending=True, stable=True)[:k]
            jitter = torch.from_numpy(rng.integers(-3, 4, (k, 4)).astype(f32))
            targets.append({"image_id": t["image_id"], "boxes": r["boxes"][top] + jitter, "labels": r["labels"][top].clone(),
                            "difficult": torch.from_numpy((rng.random(k) < 0.3).astype(np.uint8))})
        loader.append((imgs, targets))
    thresholds = (0.5, 0.75)
    summary, stats = engine.evaluate_voc(model, loader, thresholds=thresholds)
    assert set(stats) == {"images", "seconds", "images_per_sec", "model_seconds"} and stats["images"] == 16
    records, _ = engine.evaluate(model, loader)
    dets = [{k: v.numpy() for k, v in records[t["image_id"]].items()} for _, tg in loader for t in tg]
    gts = [{k: t[k].numpy() for k in ("boxes", "labels", "difficult")} for _, tg in loader for t in tg]
    boxes, scores, labels, counts = er.pad_records(dets, D)
    flags, _, _, gstats = er.match_ref(boxes, scores, labels, counts, *er.pad_gt(gts), thresholds, 1.0, 21)
    live = flags[np.arange(D)[None, :] < counts[:, None]]
    assert (live & 0xFFFF).any() and (live >> 16).any() and (live == 0).any()          # TP, FP and ignored all occur
    want = _accumulate(scores, labels, counts, flags, gstats, 21, thresholds).summarize()
    assert summary == want
    assert want["map"][0] > 0 and len(want["ap"]) >= 1
    is_live = np.arange(D)[None, :] < counts[:, None]
    tie_free = all(len(np.unique(scores[is_live & (labels == c)])) == int((is_live & (labels == c)).sum()) for c in range(21))
    if tie_free:
        for b, t in enumerate(thresholds):
            m, ap = evalrec.voc_mean_ap(dets, gts, t)
            assert summary["map"][b] == m and {c: v[b] for c, v in summary["ap"].items()} == ap
