"""Exact tests of the hard-NMS post-process (csrc/postprocess.hip) at every capacity bucket, boundary and chain.

Every case goes through the public entry point dn_postprocess and is compared with tests/post_select_ref.py's verifier, which recomputes the
selection with the oracle's own functions FROM THE DEVICE'S scores and boxes (read back from the workspace): labels, anchors, counts, score bits
and boxes must be equal for every image. The front half (softmax, decode) is held to the oracle separately, at the tolerances of
test_gpu_model.py::test_postprocess_random_vs_oracle.

The designed cases state the regime they are built to hit (`expect`): the CPU test test_designed_case_hits_its_regime proves it from the torch
softmax of the case's logits, and the GPU test asserts it again from what the kernels left in the workspace (tauKey, needFull, keptCount, the
per-class count of keys >= tauKey). A case that misses its regime fails; nothing is skipped."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import post_select_ref as psr
import ssd_oracle as so
from demonet_amd import _lib, models, synth

HALF_DOWN = float(np.nextafter(np.float32(0.5), np.float32(0)))      # the float below 0.5


# ------------------------------------------------------------------------------------------------------------------------------------
# designed cases
# ------------------------------------------------------------------------------------------------------------------------------------
CASES = {}


def case(name, regime, scene, topk, dets, st=0.01, nt=0.5, hw=(320, 320), scale=None, env=None, expect=None, fasts=("1", "0")):
    """scene: a function returning the psr.Scene. expect: what psr.analyse_image must report on the cut-off path (DN_PP_FAST=1), per image:
    need_full [n], tau_zero [n], walk [n], merge_total [n], merge_ties [n], merge_whole [n], in_lds [n], counted (bool), and per
    (image, label): cnt (keys >= tau), M, kept, sel_ties."""
    assert name not in CASES, name
    CASES[name] = dict(name=name, regime=regime, scene=scene, topk=topk, dets=dets, st=st, nt=nt, hw=hw, scale=scale, env=env or {},
                       expect=expect or {}, fasts=fasts)


def full_bins(count):
    """`count` lattice scores whose LOWEST histogram bin is full (64 scores): once the image holds `want` scores the cut-off falls at or below it."""
    return psr.lattice_scores((count + 63) // 64 * 64)[-count:] if count else np.zeros(0, np.float32)


def cells(counts, K=None, n=1, A=None):
    """counts: {(image, label): number of disjoint cells with distinct lattice scores}"""
    def build():
        s = psr.Scene(n, K or 1 + max(l for _, l in counts))
        for (img, label), c in sorted(counts.items()):
            s.add_cells(full_bins(c), img, label)
        return s.pad_to(A) if A else s
    return build


# ---- counts against topk and the fast kernel's list limit, in every capacity bucket -------------------------------------------------------
# D is chosen so that want = 4 D exceeds the passing scores (tau = 0: the fast kernel lists every passing score) -- except in the bucket of 8
# words, where CAP = 2048 = want at D = 512: 2047 scores are `total < want`, 2048 are `total == want`, 2049 cross in the lowest (full) bin.
BUCKET_DETS = {1: 64, 2: 128, 4: 512, 5: 512, 8: 512}
BUCKET_TOPK = {1: (1, 63, 64), 2: (65, 128), 4: (129, 256), 5: (257, 320), 8: (321, 512)}
for _nw, _topks in BUCKET_TOPK.items():
    _cap = psr.fast_cap(_nw)
    for _topk in _topks:
        assert psr.nw_bucket(_topk) == _nw
        _counts = {_topk - 1, _topk, _topk + 1}
        if _topk == _topks[-1]:
            _counts |= {_cap - 1, _cap, _cap + 1}
        for _c in sorted(c for c in _counts if c >= 1):
            case("count-nw%d-topk%d-cnt%d" % (_nw, _topk, _c),
                 "bucket NW=%d (CAP %d), topk %d: %d keys >= tau in the class%s" % (_nw, _cap, _topk, _c, " -> needFull" if _c > _cap else ""),
                 cells({(0, 1): _c}), _topk, BUCKET_DETS[_nw],
                 expect=dict(cnt={(0, 1): _c}, need_full=[_c > _cap], M={(0, 1): min(_c, _topk)}, kept={(0, 1): min(_c, _topk)},
                             tau_zero=[_c < 4 * BUCKET_DETS[_nw]]))
case("count-two-classes-one-overflows", "NW=2: label 1 holds CAP + 1 keys, label 2 holds 10; the image beside it holds CAP and 10 and stays in the fast kernel",
     cells({(0, 1): 257, (0, 2): 10, (1, 1): 256, (1, 2): 10}, n=2), 128, 128,
     expect=dict(cnt={(0, 1): 257, (0, 2): 10, (1, 1): 256, (1, 2): 10}, need_full=[True, False], M={(0, 1): 128, (0, 2): 10, (1, 1): 128}))
case("count-fallback-between-two-fast-images", "NW=1: the middle of three images overflows the 64-entry list",
     cells({(0, 1): 64, (1, 1): 65, (2, 1): 63, (2, 2): 64}, n=3), 64, 64,
     expect=dict(need_full=[False, True, False], cnt={(0, 1): 64, (1, 1): 65, (2, 1): 63, (2, 2): 64}))


# ---- ties at the top-k cut ------------------------------------------------------------------------------------------------------------------
def tied(higher, ties, lower, spread=1, A=None):
    """One class: `higher` distinct scores, then `ties` anchors sharing ONE score, then `lower` distinct ones; the tied anchors stand `spread`
    anchors apart (the anchors between them carry the other scores or nothing), all on disjoint cells."""
    def build():
        sc = psr.lattice_scores(higher + 1 + lower)
        s = psr.Scene(1, 2)
        rest = list(sc[:higher]) + list(sc[higher + 1:])
        for t in range(ties):
            s.add(s.cell(), {(0, 1): float(sc[higher])})
            for _ in range(spread - 1):
                s.add(s.cell(), {(0, 1): float(rest.pop())} if rest else None)
        for v in rest:
            s.add(s.cell(), {(0, 1): float(v)})
        return s.pad_to(A) if A else s
    return build


case("tie-cut-2-fast", "NW=2, fast kernel: the score at rank topk is shared by 2 anchors (126 above it): the lower anchor goes in",
     tied(127, 2, 20), 128, 128, expect=dict(sel_ties={(0, 1): 2}, need_full=[False], cnt={(0, 1): 149}, M={(0, 1): 128}))
case("tie-cut-2-full", "NW=1: 63 above the cut, 2 share it, 65 keys overflow the list: the radix select of the full kernel splits the tie (quota 1)",
     tied(63, 2, 0), 64, 64, expect=dict(sel_ties={(0, 1): 2}, need_full=[True], cnt={(0, 1): 65}, M={(0, 1): 64}))
case("tie-cut-100-over-scan-blocks", "NW=1: 30 above the cut, 100 anchors six apart (three 256-anchor scan blocks) share it, quota 34; fallback by list overflow",
     tied(30, 100, 200, spread=6), 64, 16, expect=dict(sel_ties={(0, 1): 100}, need_full=[True], M={(0, 1): 64}))
case("tie-cut-100-fast", "NW=2, fast kernel (rank sort on (score, anchor) keys): 30 above the cut, 100 share it, 20 below",
     tied(30, 100, 20, spread=3), 128, 128, expect=dict(sel_ties={(0, 1): 100}, need_full=[False], cnt={(0, 1): 150}, M={(0, 1): 128}))
case("tie-all-equal-full", "NW=1: all 300 passing scores are equal: the 64 lowest anchors are the candidates (full kernel, via overflow)",
     tied(0, 300, 0, spread=2), 64, 64, expect=dict(sel_ties={(0, 1): 300}, need_full=[True], M={(0, 1): 64}))
case("tie-all-equal-fast", "NW=4: all 300 passing scores are equal, topk 256, inside the 1024-entry list",
     tied(0, 300, 0), 256, 512, expect=dict(sel_ties={(0, 1): 300}, need_full=[False], cnt={(0, 1): 300}, M={(0, 1): 256}))
case("tie-cnt-eq-topk", "NW=1: exactly topk passing scores, all equal: no select at all", tied(0, 64, 0), 64, 64,
     expect=dict(cnt={(0, 1): 64}, M={(0, 1): 64}, need_full=[False]))
case("tie-cnt-eq-topk-plus-1", "NW=1: topk + 1 equal scores: the highest anchor is cut (full kernel)", tied(0, 65, 0), 64, 64,
     expect=dict(sel_ties={(0, 1): 65}, need_full=[True], M={(0, 1): 64}))


# ---- mask words -------------------------------------------------------------------------------------------------------------------------------
def mask_pairs(M):
    """Suppressing pairs (i, j), i < j, no candidate in two pairs: (0, M-1); diagonal neighbours; a row of word 0 with a column of every later word;
    the last two candidates that are free (at odd M the row pair of the row-pair loop whose second row is beyond M follows it)."""
    want = [(0, M - 1), (2, 3), (61, 62), (63, 64)] + [(10 + w, 64 * w + 1) for w in range(1, (M + 63) // 64)] + [(M - 3, M - 2), (M - 5, M - 4)]
    used, out = set(), []
    for i, j in want:
        if 0 <= i < j < M and not ({i, j} & used):
            used |= {i, j}
            out.append((i, j))
    return out


def mask_scene(M):
    def build():
        s = psr.Scene(1, 2)
        sc = psr.lattice_scores(M)
        boxes = [s.cell() for _ in range(M)]
        for i, j in mask_pairs(M):
            boxes[j] = boxes[i]            # identical boxes: IoU 1
        for b, v in zip(boxes, sc):        # candidate rank == anchor index
            s.add(b, {(0, 1): float(v)})
        return s
    return build


for _nw, _mc in ((1, 64), (2, 128), (4, 256), (5, 320), (8, 512)):
    for _M in sorted({1, 2, 63, 64, 65, 127, 128, 129, _mc - 1, _mc}):
        if _M <= _mc:
            case("mask-nw%d-M%d" % (_nw, _M), "bucket NW=%d, M = %d candidates (%d mask words), %d suppressing pairs: %s"
                 % (_nw, _M, (_M + 63) // 64, len(mask_pairs(_M)), mask_pairs(_M)),
                 mask_scene(_M), _mc, 512, expect=dict(cnt={(0, 1): _M}, M={(0, 1): _M}, kept={(0, 1): _M - len(mask_pairs(_M))}, need_full=[False],
                                                      tau_zero=[True]))


# ---- chains -----------------------------------------------------------------------------------------------------------------------------------
def chain_scene(length, lead=0, clique=False):
    """`lead` disjoint cells with the highest scores, then a chain (or a clique of identical boxes) of `length`; candidate rank == anchor index."""
    def build():
        s = psr.Scene(1, 2)
        sc = psr.lattice_scores(lead + length)
        for v in sc[:lead]:
            s.add(s.cell(), {(0, 1): float(v)})
        for i, v in enumerate(sc[lead:]):
            s.add((10, 300, 14, 304) if clique else psr.chain_box(i, y=310), {(0, 1): float(v)})
        return s
    return build


for _L in (6, 7, 8, 63, 64):
    case("chain-%d" % _L, "NW=1: each of %d boxes suppresses its successor only: dependency depth %d, the fixed point %s in %d rounds"
         % (_L, _L - 1, "settles" if _L <= psr.FIXED_POINT_ROUNDS else "does not settle", psr.FIXED_POINT_ROUNDS),
         chain_scene(_L), 64, 64, expect=dict(walk=[_L > psr.FIXED_POINT_ROUNDS], M={(0, 1): _L}, kept={(0, 1): (_L + 1) // 2}, need_full=[False]))
case("chain-across-chunks", "NW=2: candidates 60 .. 70 form a chain across the boundary of the 64-candidate chunks: 4 links settle in chunk 0, the 7 of chunk 1 are walked",
     chain_scene(11, lead=60), 128, 128, expect=dict(M={(0, 1): 71}, kept={(0, 1): 66}, walk=[True], need_full=[False]))
case("chain-128", "NW=2: one chain of 128 over two chunks, both walked", chain_scene(128), 128, 128,
     expect=dict(M={(0, 1): 128}, kept={(0, 1): 64}, walk=[True], need_full=[False]))
case("chain-512", "NW=8: one chain of 200 behind 312 disjoint candidates", chain_scene(200, lead=312), 512, 512,
     expect=dict(M={(0, 1): 512}, kept={(0, 1): 412}, walk=[True], need_full=[False]))
case("clique-64", "NW=1: 64 identical boxes: the first suppresses all others (settles in two rounds)", chain_scene(64, clique=True), 64, 64,
     expect=dict(M={(0, 1): 64}, kept={(0, 1): 1}, walk=[False]))


# ---- threshold edges --------------------------------------------------------------------------------------------------------------------------
def boxes_scene(boxes, K=2, labels=None):
    def build():
        s = psr.Scene(1, K)
        for b, v, l in zip(boxes, psr.lattice_scores(len(boxes)), labels or [1] * len(boxes)):
            s.add(b, {(0, l): float(v)})
        return s
    return build


case("iou-exactly-half", "IoU exactly 0.5 at nms_thresh 0.5 (strict >): [0,0,3,1] and [1,0,4,1], and 2 x 2 against 2 x 4: all kept",
     boxes_scene([(0, 0, 3, 1), (1, 0, 4, 1), (20, 20, 22, 22), (20, 20, 22, 24)]), 64, 64, expect=dict(kept={(0, 1): 4}))
case("iou-half-threshold-one-float-lower", "the same pairs with nms_thresh the float below 0.5: the exact division decides, each pair loses its second box",
     boxes_scene([(0, 0, 3, 1), (1, 0, 4, 1), (20, 20, 22, 22), (20, 20, 22, 24)]), 64, 64, nt=HALF_DOWN, expect=dict(kept={(0, 1): 2}))
case("iou-one-lattice-step-above", "the pairs one lattice step closer: IoU 3/5 and 4/6 > 0.5", boxes_scene([(0, 0, 4, 1), (1, 0, 5, 1), (20, 20, 22, 22), (20, 20, 22, 23)]),
     64, 64, expect=dict(kept={(0, 1): 2}))
case("nms-thresh-0", "nms_thresh 0: touching boxes (IoU 0) are kept, any overlap is suppressed",
     boxes_scene([(0, 0, 2, 2), (2, 0, 4, 2), (10, 0, 13, 2), (12, 0, 15, 2), (40, 40, 50, 50), (49, 49, 60, 60)]), 64, 64, nt=0.0, expect=dict(kept={(0, 1): 4}))
case("nms-thresh-1", "nms_thresh 1: identical boxes (IoU exactly 1) are kept", boxes_scene([(5, 5, 9, 9)] * 3 + [(5, 5, 9, 10)]), 64, 64, nt=1.0,
     expect=dict(kept={(0, 1): 4}))
case("zero-area-outside", "anchors wholly outside the image clip to zero area: 0/0 is not > nms_thresh, all are kept (as in the oracle)",
     boxes_scene([(400, 10, 420, 30), (400, 10, 420, 30), (330, 10, 350, 30), (10, 400, 30, 420), (300, 10, 340, 30), (300, 10, 340, 30)]), 64, 64,
     expect=dict(kept={(0, 1): 5}))


# ---- merge ------------------------------------------------------------------------------------------------------------------------------------
for _t in (0, 1, 63, 64, 65):
    case("merge-total-%d" % _t, "D = 64, %d survivors over two classes" % _t,
         cells({(0, 1): (_t + 1) // 2, (0, 2): _t // 2}, K=3, A=max(_t, 4)), 64, 64, expect=dict(merge_total=[_t], need_full=[False]))


def merge_tie_scene():
    s = psr.Scene(1, 4)
    sc = psr.lattice_scores(9)
    for i in range(8):
        s.add(s.cell(), {(0, 1 + i % 3): float(sc[i])})
    for label in (3, 1, 2, 2, 3, 1):          # (added out of class order: the merge must order by class, then by emission)
        s.add(s.cell(), {(0, label): float(sc[8])})
    return s


case("merge-tie-three-classes", "D = 10: 8 survivors above the rank-D key, which 6 survivors of three classes share (quota 2: class 1's two)",
     merge_tie_scene, 64, 10, expect=dict(merge_total=[14], merge_ties=[6], merge_whole=[None]))


def whole_scene():
    s = psr.Scene(1, 3)
    for i, v in enumerate(psr.lattice_scores(10, top=0.2)):       # top byte of the key 0x3E: [0.125, 0.5)
        s.add(s.cell(), {(0, 1 + i % 2): float(v)})
    for i, v in enumerate(psr.lattice_scores(10, top=0.1)):       # top byte 0x3D
        s.add(s.cell(), {(0, 1 + i % 2): float(v)})
    return s


case("merge-whole-bin", "D = 10 and exactly 10 of 20 survivors in the radix bin of the top byte: the `whole` shortcut at shift 24",
     whole_scene, 64, 10, expect=dict(merge_total=[20], merge_whole=[24]))


def wide_merge_scene():
    s = psr.Scene(1, 9)
    sc = full_bins(512)
    for label in range(1, 9):
        s.add_cells(sc, 0, label)
    return s


case("merge-4096-survivors", "8 classes x 512 disjoint boxes, topk 512: 4096 survivors > MERGE_LCAP, the merge works from global memory "
     "(cut-off path: DN_PP_WANT=8 makes want = 4096 = total, tau at the lowest bin)", wide_merge_scene, 512, 512, env=dict(DN_PP_WANT="8"),
     expect=dict(merge_total=[4096], in_lds=[False], need_full=[False], cnt={(0, 1): 512, (0, 8): 512}, merge_whole=[16]))
case("merge-D1", "D = 1", cells({(0, 1): 5, (0, 2): 7}), 64, 1, expect=dict(merge_total=[12], tau_zero=[False]))


def few_scene():
    s = psr.Scene(2, 3)
    sc = psr.lattice_scores(64 + 20)
    for img in (0, 1):
        for v in sc[:50]:
            s.add((100, 100, 104, 104), {(img, 1): float(v)})        # a clique in the highest bin
        for i, v in enumerate(sc[64:]):
            s.add(s.cell(), {(img, 1 + (i + img) % 2): float(v)})
    return s


FEW = dict(tau_zero=[False, False], need_full=[True, True], cnt={(0, 1): 50, (0, 2): 0}, merge_total=[21, 21])
case("merge-mode0-fallback", "D = 10, want 40: 50 scores of one clique above a non-zero tau leave 1 survivor < D: the merge raises needFull",
     few_scene, 64, 10, expect=FEW)
case("merge-mode0-fallback-two-launches", "the same with DN_PP_FUSE_FALLBACK=0 (full selection, then a merge launch)", few_scene, 64, 10,
     env=dict(DN_PP_FUSE_FALLBACK="0"), expect=FEW, fasts=("1",))


def edge_scene():
    s = psr.Scene(2, 3)
    boxes = [(190, 10, 210, 30), (10, 90, 30, 110), (150, 50, 170, 70), (150, 52, 170, 72), (195, 95, 230, 130), (0, 0, 200, 100), (120, 20, 140, 40)]
    sc = psr.lattice_scores(2 * len(boxes))
    for i, b in enumerate(boxes):
        s.add(b, {(0, 1 + i % 2): float(sc[2 * i]), (1, 2 - i % 2): float(sc[2 * i + 1])})
    return s


case("scale-xy-per-image", "scale_xy with another (w, h) ratio per image", edge_scene, 64, 64,
     scale=[[1.5, 0.75], [0.4000000059604645, 2.0]], expect=dict(merge_total=[7, 7]))
case("image-100x200", "image_h 100, image_w 200 with anchors over the right and the lower edge (and one over both): clipping must not mix the two up",
     edge_scene, 64, 64, hw=(100, 200), scale=[[2.0, 3.0], [1.0, 1.0]], expect=dict(merge_total=[7, 7]))


# ---- the cut-off ------------------------------------------------------------------------------------------------------------------------------
def magnitudes_scene():
    """Scores from 0.9 down to 1e-10 and exact zeros, two classes."""
    s = psr.Scene(1, 3)
    i = 0
    for top in (0.9, 0.3, 0.02, 1e-3, 2e-5, 3e-6, 1e-7, 1e-10):
        for v in psr.lattice_scores(6, top=top):
            s.add(s.cell(), {(0, 1 + i % 2): float(v)})
            i += 1
    return s.pad_to(64)


case("thresh-0", "score_thresh 0: the clamped table (bin 0 holds every score below 2^-16), exact zeros do not pass", magnitudes_scene, 64, 7, st=0.0,
     expect=dict(tau_zero=[False], cnt={(0, 1): 15, (0, 2): 15}))
case("thresh-0-want-all", "score_thresh 0 and want = 48 = all passing scores: the crossing bin is the clamped bin 0 -> tau 0", magnitudes_scene, 64, 12, st=0.0,
     expect=dict(tau_zero=[True], cnt={(0, 1): 24, (0, 2): 24}))
case("thresh-1e-6", "score_thresh 1e-6 (below 2^-16: clamped table)", magnitudes_scene, 64, 9, st=1e-6,
     expect=dict(tau_zero=[True], cnt={(0, 1): 18, (0, 2): 18}))
case("thresh-0.01", "score_thresh 0.01", magnitudes_scene, 64, 4, st=0.01, expect=dict(tau_zero=[False], merge_total=[18]))


def top_bin_scene():
    s = psr.Scene(1, 2)
    for v in (0.998, 0.996, 0.994, 0.992, 0.9895, 0.985, 0.97, 0.5):
        s.add(s.cell(), {(0, 1): v})
    return s


case("thresh-0.99", "score_thresh 0.99 lies in the top histogram bin below 1.0, [0.96875, 1) (the table is that bin and the bin of 1.0 itself), which also holds scores below the threshold",
     top_bin_scene, 64, 1, st=0.99, expect=dict(tau_zero=[False], cnt={(0, 1): 4}, merge_total=[4]))
case("want-in-one-bin", "D = 8: all 40 scores of the image in one bin, want = 32: tau is that bin's edge", cells({(0, 1): 40}), 64, 8,
     expect=dict(tau_zero=[False], cnt={(0, 1): 40}))


def many_classes_scene(K):
    def build():
        s = psr.Scene(2, K)
        sc = psr.lattice_scores(40)
        for i, v in enumerate(sc):
            label = (1, 2, 77, K - 1, K - 1, 2, K - 1)[i % 7]
            s.add(s.cell(), {(0, label): float(v), (1, K - label): float(v)})
        return s.pad_to(200)
    return build


_NB001 = psr.hist_range(0.01)[1]
case("order-counted-largest-K", "score_thresh 0.01 (%d bins): K - 1 = %d is the largest with nb + K - 1 <= HBINS: the class order is counted" % (_NB001, psr.HBINS - _NB001),
     many_classes_scene(psr.HBINS - _NB001 + 1), 64, 64, expect=dict(counted=True, merge_total=[40, 40]))
case("order-identity-next-K", "one class more: no room for the counts, the class order is the identity", many_classes_scene(psr.HBINS - _NB001 + 2), 64, 64,
     expect=dict(counted=False, merge_total=[40, 40]))


def mixed_scene():
    """Two images, three classes: a chain, a clique, ties, disjoint cells -- the scene of the knob cases."""
    s = psr.Scene(2, 4)
    sc = psr.lattice_scores(200)
    for img in (0, 1):
        k = iter(sc[img:])
        for i in range(20):
            s.add(psr.chain_box(i, y=200 + 2 * img), {(img, 1): float(next(k))})
        for i in range(40):
            s.add((50, 50, 58, 58), {(img, 2): float(next(k))})
        t = float(next(k))
        for i in range(9):
            s.add(s.cell(), {(img, 3): t, (img, 1): float(next(k))})
        for i in range(60):
            s.add(s.cell(), {(img, 1 + i % 3): float(next(k))})
    return s


case("knob-default", "the mixed scene with default knobs", mixed_scene, 64, 30, expect=dict(walk=[True, True]))
for _w in (1, 4, 8):
    case("knob-want-%d" % _w, "DN_PP_WANT=%d" % _w, mixed_scene, 64, 30, env=dict(DN_PP_WANT=str(_w)), fasts=("1",),
         expect=dict(need_full=[_w == 1, _w == 1]))
case("knob-order-0", "DN_PP_ORDER=0: classes in class order", mixed_scene, 64, 30, env=dict(DN_PP_ORDER="0"), fasts=("1",))
case("knob-fuse-fallback-0", "DN_PP_FUSE_FALLBACK=0 with a falling back image (DN_PP_WANT=1)", mixed_scene, 64, 30,
     env=dict(DN_PP_FUSE_FALLBACK="0", DN_PP_WANT="1"), fasts=("1",), expect=dict(need_full=[True, True]))
case("knob-fuse-fallback-1", "DN_PP_FUSE_FALLBACK=1 with a falling back image (DN_PP_WANT=1)", mixed_scene, 64, 30,
     env=dict(DN_PP_FUSE_FALLBACK="1", DN_PP_WANT="1"), fasts=("1",), expect=dict(need_full=[True, True]))


# ---- shapes -----------------------------------------------------------------------------------------------------------------------------------
def shape_scene(A, n):
    def build():
        s = psr.Scene(n, 2)
        sc = psr.lattice_scores(3 * n + 40)
        s.add(s.cell(), {(img, 1): float(sc[img]) for img in range(n)})
        for i in range(1, min(A - 1, 31)):
            s.add(s.cell(), {(img, 1): float(sc[n + i + img]) for img in range(n) if (i + img) % 3})
        s.pad_to(max(A - 1, 1))
        if A > 1:
            s.add(s.cell(), {(img, 1): float(sc[2 * n + 32 + img]) for img in range(n)})       # the last anchor is a candidate
        return s
    return build


for _A in (1, 63, 64, 65, 257, 4097):
    for _n in (1, 9):
        case("shape-A%d-n%d" % (_A, _n), "A = %d anchors (K = 2), %d images, the first and the last anchor are candidates" % (_A, _n), shape_scene(_A, _n), 64, 64,
             expect=dict(need_full=[False] * _n))

NAMES = list(CASES)
NAMES_FAST = [(name, fast) for name in NAMES for fast in CASES[name]["fasts"]]      # (a case about a knob of the cut-off path has no full-path run)


@functools.lru_cache(maxsize=None)
def _arrays(name):
    return CASES[name]["scene"]().arrays()


def _scales(c, n):
    return [(1.0, 1.0)] * n if c["scale"] is None else [tuple(np.float32(v) for v in row) for row in c["scale"]]


def _check_regime(c, infos):
    """The case's `expect` against the predictor's report per image."""
    e = c["expect"]
    per_image = dict(need_full="need_full", walk="walk", merge_total="merge_total", merge_ties="merge_ties", merge_whole="merge_whole", in_lds="merge_in_lds")
    for key, field in per_image.items():
        if key in e:
            got = [r[field] for r in infos]
            assert got == list(e[key]), "%s: %s is %s, the case is built for %s" % (c["name"], key, got, e[key])
    if "tau_zero" in e:
        got = [r["tau"] == 0 for r in infos]
        assert got == list(e["tau_zero"]), "%s: tau == 0 is %s, the case is built for %s (tau %s)" % (c["name"], got, e["tau_zero"], [hex(r["tau"]) for r in infos])
    if "counted" in e:
        assert all(r["counted"] == e["counted"] for r in infos)
    for key, field in (("cnt", "cnt_tau"), ("M", "M"), ("kept", "kept"), ("sel_ties", "sel_ties")):
        for (img, label), v in e.get(key, {}).items():
            got = int(infos[img][field][label - 1])
            assert got == v, "%s: %s of image %d label %d is %d, the case is built for %d" % (c["name"], key, img, label, got, v)
    for r in infos:      # what the flag MEANS: a list overflow, or too few survivors above a non-zero cut-off
        assert r["need_full"] == bool((r["cnt_tau"] > r["cap"]).any() or r["why"] == "few")


def _want(c):
    return int(c["env"].get("DN_PP_WANT", psr.WANT_DEFAULT))


def _oracle_intermediates(logits, reg, anchors, hw):
    d = so.postprocess_detections(torch.from_numpy(logits), torch.from_numpy(reg), torch.from_numpy(anchors), hw, 0.5, 0.5, 1, 1, return_intermediates=True)
    return [(x["softmax"], x["decoded"]) for x in d]


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the mirrors, the helper itself, the input conditions
# ------------------------------------------------------------------------------------------------------------------------------------
def test_mirrors_follow_the_source_text():
    src = psr.source_constants()
    for name in ("HSHIFT", "HBINS", "MERGE_LCAP", "FIXED_POINT_ROUNDS", "FAST_CAP_MAX", "WANT_DEFAULT"):
        assert src[name] == getattr(psr, name), name
    assert src["nw_bucket"] == "w <= 2 ? w : w <= 4 ? 4 : w <= 5 ? 5 : 8"
    assert [psr.nw_bucket(t) for t in (40, 64, 80, 100, 300, 400)] == [1, 1, 2, 2, 5, 8]
    assert [psr.nw_bucket(t) for t in (1, 64, 65, 128, 129, 256, 257, 320, 321, 512)] == [1, 1, 2, 2, 4, 4, 5, 5, 8, 8]
    assert [psr.fast_cap(w) for w in (1, 2, 4, 5, 8)] == [64, 256, 1024, 1600, 2048]
    post = psr.source("postprocess.hip")
    # post_hist_range and the workspace layout, statement by statement
    for line in ("const float t = score_thresh > 0.f ? score_thresh : 0.f, one = 1.0f;", "const int top = (int)(one_bits >> HSHIFT);",
                 "const int hb_thr = (int)(thr_bits >> HSHIFT);", "const int hb0 = hb_thr > top + 1 - HBINS ? hb_thr : top + 1 - HBINS;",
                 "*nb_out = top + 1 - hb0;", "*clamped_out = hb_thr < hb0;",
                 "b.scoresT = reinterpret_cast<float*>(p);\n    p += align256((size_t)n * Km1 * A * 4);\n    b.boxes = reinterpret_cast<float4*>(p);\n"
                 "    p += align256((size_t)n * A * 16);\n    b.keptScore = reinterpret_cast<float*>(p);\n    p += align256((size_t)n * Km1 * topk * 4);\n"
                 "    b.keptAnchor = reinterpret_cast<int*>(p);\n    p += align256((size_t)n * Km1 * topk * 4);\n    b.keptCount = reinterpret_cast<int*>(p);\n"
                 "    p += align256((size_t)n * Km1 * 4);\n    b.tiles = dn_cdiv(A, 64);\n    b.phist = reinterpret_cast<unsigned*>(p);",
                 "b.tauKey = b.phist + (size_t)n * b.tiles * HBINS;", "b.needFull = reinterpret_cast<int*>(b.tauKey + n);", "b.order = b.needFull + n;",
                 "constexpr int HSHIFT = DN_PP_HSHIFT;", "constexpr int HBINS = DN_PP_HBINS;", "if (nb + Km1 <= HBINS) {",
                 "const bool in_lds = total <= (unsigned)LCAP;", "if (cnt > (unsigned)CAP) {", "if (whole && shift > 0) {",
                 "if (mode == 0 && total < (unsigned)D && tauKey[n] != 0u) {", "size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }"):
        assert line in post, "postprocess.hip no longer reads: " + line
    assert psr.hist_range(0.01) == (1924, 109, 0) and psr.hist_range(0.0)[1:] == (256, 1) and psr.hist_range(1e-6)[2] == 1 and psr.hist_range(0.99)[1] == 2
    lay = psr.workspace_layout(2, 100, 3, 64)
    assert lay["boxes"] == 1792 and lay["keptScore"] == 1792 + 3328 and lay["tauKey"] - lay["phist"] == 2 * 2 * 256 * 4


def test_logit_construction_reproduces_the_target_scores_within_4_ulp():
    worst = 0
    for name in ("count-nw2-topk128-cnt257", "count-nw8-topk512-cnt2049", "order-counted-largest-K", "merge-4096-survivors", "thresh-0.99", "merge-tie-three-classes"):
        logits, _, _, p = _arrays(name)
        sm = torch.softmax(torch.from_numpy(logits), -1).numpy()[..., 1:]
        on = p > 0
        assert (sm[~on] == 0).all(), "an OFF logit must give exactly 0.0"
        assert (p[on] >= 2.0 ** -6).all()
        ulp = np.abs(psr.bits(sm[on]).astype(np.int64) - psr.bits(p[on]).astype(np.int64))
        worst = max(worst, int(ulp.max()))
    print("target scores reproduced within %d ulp" % worst)
    assert worst <= 4


def test_lattice_scores_sit_mid_bin_and_apart():
    v = psr.lattice_scores(2049)
    b = psr.bits(v).astype(np.int64)
    assert (np.diff(b) <= -(1 << 12)).all() and (np.diff(v) < 0).all()
    frac = (b & ((1 << psr.HSHIFT) - 1)) / float(1 << psr.HSHIFT)
    assert frac.min() >= 0.25 and frac.max() < 0.75
    assert np.bincount((b >> psr.HSHIFT) - (b >> psr.HSHIFT).min()).tolist() == [1] + [64] * 32


@pytest.mark.parametrize("name", NAMES)
def test_designed_case_hits_its_regime(name):
    """The input condition of the GPU case, provable without a GPU: on the torch softmax of its logits the predictor reports the regime the case
    is built for; its boxes decode to the integer anchors exactly; its scores are reproduced on their lattice."""
    c = CASES[name]
    logits, reg, anchors, p = _arrays(name)
    n, A, K = logits.shape
    assert c["expect"] or c["env"], "a designed case states what it pins"
    inter = _oracle_intermediates(logits, reg, anchors, c["hw"])
    H, W = c["hw"]
    clipped = np.stack([np.clip(anchors[:, 0], 0, W), np.clip(anchors[:, 1], 0, H), np.clip(anchors[:, 2], 0, W), np.clip(anchors[:, 3], 0, H)], 1)
    for (sm, dec), pi in zip(inter, p):
        assert np.array_equal(dec, clipped), "zero regression must decode to the anchor exactly"
        on = pi > 0
        assert (sm[:, 1:][~on] == 0).all()
        assert (np.abs(psr.bits(sm[:, 1:][on]).astype(np.int64) - psr.bits(pi[on]).astype(np.int64)) <= psr.ulp_bound(pi[on])).all()
    infos = [psr.analyse_image(sm, dec, c["st"], c["nt"], c["topk"], c["dets"], _want(c), fast=True) for sm, dec in inter]
    _check_regime(c, infos)


def _two_cpu_cases():
    for name in ("merge-tie-three-classes", "chain-across-chunks"):
        c = CASES[name]
        logits, reg, anchors, _ = _arrays(name)
        sm, dec = _oracle_intermediates(logits, reg, anchors, c["hw"])[0]
        d = so.postprocess_detections(torch.from_numpy(logits), torch.from_numpy(reg), torch.from_numpy(anchors), c["hw"], c["st"], c["nt"], c["dets"],
                                      c["topk"], return_intermediates=True)[0]
        yield c, sm, dec, d


def test_verifier_accepts_the_oracle_and_rejects_corruptions():
    for c, sm, dec, d in _two_cpu_cases():
        D, scale = c["dets"], (np.float32(1.5), np.float32(0.75))
        cnt = d["labels"].shape[0]
        assert 4 <= cnt <= D
        pad = lambda x, fill: np.concatenate([x, np.full((D - cnt,) + x.shape[1:], fill, x.dtype)])
        b = pad(d["boxes"] * np.array([1.5, 0.75, 1.5, 0.75], np.float32), 0)
        s, l, k = pad(d["scores"], 0), pad(d["labels"], 0), pad(d["anchor_idx"].astype(np.int32), -1)
        args = (sm, dec, c["st"], c["nt"], c["topk"], D, scale)
        assert psr.verify_image((b, s, l, cnt, k), *args) == cnt
        bad = {}
        # a swapped tie: two detections with equal scores change places (labels, anchors and boxes with them)
        ties = [i for i in range(cnt - 1) if s[i] == s[i + 1]]
        if c["name"] == "merge-tie-three-classes":
            assert ties, "the case has tied detections"
        if ties:
            i = ties[0]
            sw = lambda x: np.concatenate([x[:i], x[i + 1:i + 2], x[i:i + 1], x[i + 2:]])
            bad["swapped tie"] = (sw(b), sw(s), sw(l), cnt, sw(k))
        # a dropped survivor: detection 1 is missing, the rest moved up
        dr = lambda x, fill: np.concatenate([x[:1], x[2:], np.full((1,) + x.shape[1:], fill, x.dtype)])
        bad["dropped survivor"] = (dr(b, 0), dr(s, 0), dr(l, 0), cnt - 1, dr(k, -1))
        bad["count one short"] = (b, s, l, cnt - 1, k)
        bad["count one over"] = (b, s, l, cnt + 1, k)
        bad["unscaled box"] = (pad(d["boxes"], 0), s, l, cnt, k)
        s2 = s.copy()
        s2[0] = np.nextafter(s2[0], np.float32(0))
        bad["score one ulp off"] = (b, s2, l, cnt, k)
        k2 = k.copy()
        k2[cnt:] = 0
        if cnt < D:
            bad["padding not -1"] = (b, s, l, cnt, k2)
        for what, out in bad.items():
            with pytest.raises(AssertionError):
                psr.verify_image(out, *args)
            print("rejected:", c["name"], what)


def test_serial_phase_restatement_takes_the_walk_only_on_deep_chains():
    for L in range(1, 12):
        mask = np.zeros((L, L), bool)
        mask[np.arange(L - 1), np.arange(1, L)] = True
        kept, walks = psr.serial_phase(mask)
        assert kept.tolist() == [i % 2 == 0 for i in range(L)] and walks == [L > psr.FIXED_POINT_ROUNDS]


def test_radix_select_restatement():
    rng = np.random.default_rng(3)
    keys = rng.integers(1, 2 ** 31, 500, dtype=np.int64).astype(np.uint32)
    keys[100:140] = keys[7]
    for need in (1, 7, 250, 499):
        for whole in (False, True):
            T, quota, shift = psr.radix_select(keys, need, whole)
            srt = np.sort(keys)[::-1]
            if shift is None:
                assert T == srt[need - 1] and (keys > T).sum() + quota == need
            else:
                assert (keys > np.uint32(T)).sum() == need


# ---- random inputs ------------------------------------------------------------------------------------------------------------------------------
def random_inputs(n, A, K, seed=None):
    """The generator of test_gpu_model.py::test_postprocess_random_vs_oracle, duplicated rows (exact score ties) and anchors included."""
    rng = np.random.default_rng(A * 7 + K if seed is None else seed)
    logits = rng.normal(0, 2.0, (n, A, K)).astype(np.float32)
    reg = rng.normal(0, 1.0, (n, A, 4)).astype(np.float32)
    ctr = rng.uniform(20, 300, (A, 2)).astype(np.float32)
    wh = rng.uniform(10, 120, (A, 2)).astype(np.float32)
    anchors = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)
    dup = rng.integers(0, A, A // 5)
    src = rng.integers(0, A, A // 5)
    logits[:, dup] = logits[:, src]
    reg[:, dup] = reg[:, src]
    anchors[dup[: len(dup) // 2]] = anchors[src[: len(dup) // 2]]
    return logits, reg, anchors


# (n, A, K, topk, dets, score_thresh, (image_h, image_w), seed): every capacity bucket, a non-square image, a scale_xy table. The seeds were
# picked on the CPU (test_random_case_input_condition): the oracle's iou_gap is at least 1e-4 on each.
RANDOM_CASES = [
    (2, 900, 4, 60, 100, 0.01, (240, 320), None),
    (2, 1200, 3, 128, 100, 0.01, (320, 200), None),
    (2, 1500, 3, 200, 200, 0.005, (240, 320), None),
    (1, 2500, 3, 256, 100, 0.002, (300, 320), None),
    (2, 2000, 4, 300, 300, 0.002, (200, 320), 3),
    (1, 6000, 2, 512, 512, 0.001, (320, 256), None),
]
# the nine parameter sets of test_postprocess_random_vs_oracle (square image, no scale table), through the verifier
OLD_RANDOM_CASES = [(3, 500, 7, 40, 30, 0.05), (2, 3234, 21, 400, 100, 0.02), (1, 70, 3, 300, 300, 0.0), (2, 200, 5, 64, 512, 0.01), (1, 128, 4, 100, 50, 0.9999),
                    (11, 640, 6, 80, 40, 0.03), (2, 5000, 3, 300, 300, 0.01), (1, 9000, 2, 400, 200, 0.01), (1, 20000, 2, 400, 100, 0.0)]
# (their seeds where the generator's own misses the input condition; the 21-class set has 3.2 million candidate pairs: the best of 780 seeds
#  tried on the CPU leaves 5.3e-5, fifty times the 1e-6 the device's boxes are held to, and is asked for 5e-5)
OLD_SEEDS = {0: 1, 1: 763, 5: 1, 6: 3}
IOU_GAP_MIN = {(2, 3234, 21, 400, 100, 0.02): 5e-5}
ALL_RANDOM = RANDOM_CASES + [c + ((320, 320), OLD_SEEDS.get(i)) for i, c in enumerate(OLD_RANDOM_CASES)]


def _random_scale(n):
    return [(np.float32(1.0 + 0.25 * i), np.float32(2.0 - 0.375 * i)) for i in range(n)]


@pytest.mark.parametrize("rc", ALL_RANDOM, ids=str)
def test_random_case_input_condition(rc):
    n, A, K, topk, dets, st, hw, seed = rc
    logits, reg, anchors = random_inputs(n, A, K, seed)
    gaps = [so.selection_margins(sm, dec, st, 0.5, topk, dets)["iou_gap"] for sm, dec in _oracle_intermediates(logits, reg, anchors, hw)]
    print("iou_gap", gaps)
    assert min(gaps) >= IOU_GAP_MIN.get(rc[:6], 1e-4)
    assert psr.nw_bucket(topk) in (1, 2, 4, 5, 8)


def test_random_cases_cover_every_bucket():
    assert sorted({psr.nw_bucket(rc[3]) for rc in RANDOM_CASES}) == [1, 2, 4, 5, 8] and [rc[3] for rc in RANDOM_CASES] == [60, 128, 200, 256, 300, 512]


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------------
def _run(logits, reg, anchors, hw, scale, st, nt, topk, dets):
    """dn_postprocess on numpy inputs -> (rc, outputs as numpy, psr.read_workspace(...))."""
    L = _lib.lib()
    n, A, K = logits.shape
    dl, dr, da = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (logits, reg, anchors))
    ws = torch.zeros(L.dn_postprocess_workspace_bytes(n, A, K, topk, dets), dtype=torch.uint8, device="cuda")
    boxes = torch.full((n, dets, 4), -7.0, device="cuda")
    scores = torch.full((n, dets), -7.0, device="cuda")
    labels = torch.full((n, dets), -7, dtype=torch.int64, device="cuda")
    counts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    kept = torch.full((n, dets), -7, dtype=torch.int32, device="cuda")
    sc = None if scale is None else torch.tensor([[float(a), float(b)] for a, b in scale], dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = L.dn_postprocess(p(dl), p(dr), p(da), n, A, K, float(hw[0]), float(hw[1]), None if sc is None else p(sc), float(st), float(nt), int(topk), int(dets),
                          p(boxes), p(scores), p(labels), p(counts), p(kept), p(ws), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    outs = tuple(t.cpu().numpy() for t in (boxes, scores, labels, counts, kept))
    return rc, outs, (psr.read_workspace(ws.cpu().numpy(), n, A, K, topk) if rc == 0 else None)


def _verify_all(outs, back, st, nt, topk, dets, scales):
    total = 0
    for i, (sm, dec) in enumerate(back["inter"]):
        total += psr.verify_image(tuple(x[i] for x in outs), sm, dec, st, nt, topk, dets, scales[i])
    return total


def _front_half(back, logits, reg, anchors, hw):
    """scoresT and boxes against the oracle's softmax and decode, at the tolerances of test_postprocess_random_vs_oracle's neighbours."""
    for (sm, dec), (rsm, rdec) in zip(back["inter"], _oracle_intermediates(logits, reg, anchors, hw)):
        np.testing.assert_allclose(sm[:, 1:], rsm[:, 1:], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(dec, rdec, rtol=1e-5, atol=2e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fast", NAMES_FAST, ids=["%s-fast%s" % nf for nf in NAMES_FAST])
def test_designed_case_is_exact_and_in_its_regime(name, fast, monkeypatch):
    c = CASES[name]
    monkeypatch.setenv("DN_PP_FAST", fast)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    logits, reg, anchors, p = _arrays(name)
    n, A, K = logits.shape
    rc, outs, back = _run(logits, reg, anchors, c["hw"], c["scale"], c["st"], c["nt"], c["topk"], c["dets"])
    _lib.check(rc, "dn_postprocess")
    _front_half(back, logits, reg, anchors, c["hw"])
    H, W = c["hw"]
    clipped = np.stack([np.clip(anchors[:, 0], 0, W), np.clip(anchors[:, 1], 0, H), np.clip(anchors[:, 2], 0, W), np.clip(anchors[:, 3], 0, H)], 1)
    for (sm, dec), pi in zip(back["inter"], p):      # the designed inputs arrived as designed: exact zeros, exact boxes
        assert (sm[:, 1:][pi == 0] == 0).all() and np.array_equal(dec, clipped)
    total = _verify_all(outs, back, c["st"], c["nt"], c["topk"], c["dets"], _scales(c, n))
    # the regime, from what the kernels left behind
    if fast == "1":
        infos = []
        for i, (sm, dec) in enumerate(back["inter"]):
            predicted = psr.tau_key(sm, c["st"], _want(c) * c["dets"])
            assert int(back["tauKey"][i]) == predicted, "tauKey[%d] = %#x, the histogram of scoresT gives %#x" % (i, int(back["tauKey"][i]), predicted)
            infos.append(psr.analyse_image(sm, dec, c["st"], c["nt"], c["topk"], c["dets"], _want(c), fast=True, tau=int(back["tauKey"][i])))
        assert back["needFull"].tolist() == [int(r["need_full"]) for r in infos], "needFull %s" % back["needFull"].tolist()
        _check_regime(c, infos)
    else:
        # the cut-off path was off: nobody wrote its words of the (zero-filled) workspace
        assert not back["tauKey"].any() and not back["needFull"].any(), "DN_PP_FAST=0 ran the cut-off path"
        infos = [psr.analyse_image(sm, dec, c["st"], c["nt"], c["topk"], c["dets"], fast=False) for sm, dec in back["inter"]]
    for i, r in enumerate(infos):
        assert back["keptCount"][i].tolist() == r["kept"].tolist(), "survivors per class of image %d: %s, expected %s" % (i, back["keptCount"][i].tolist(), r["kept"].tolist())
    print("%s fast=%s: %d detections; per image: tau %s cnt>=tau %s CAP %d needFull %s M %s kept %s walk %s merge %s"
          % (name, fast, total, [hex(r["tau"]) for r in infos], [r.get("cnt_tau", r["cnt_pass"]).tolist()[:4] for r in infos], infos[0]["cap"],
             back["needFull"].tolist() if fast == "1" else "-", [r["M"].tolist()[:4] for r in infos], [r["kept"].tolist()[:4] for r in infos],
             [r["walk"] for r in infos], [(r["merge_total"], r["merge_ties"], r["merge_whole"]) for r in infos]))


@pytest.mark.gpu
@pytest.mark.parametrize("fast", ["1", "0"])
def test_negative_score_thresh_is_rejected_and_zero_keeps_no_zero_score(fast, monkeypatch):
    """The reference keeps a score that underflowed to exactly 0.0 when the threshold is negative; the kernels encode `not passing` as key 0 and
    could not: dn_postprocess has always refused a negative threshold at its entry (plan.hip; demonet_hip.h now says why), which this pins.
    At threshold 0 neither side keeps a zero score."""
    monkeypatch.setenv("DN_PP_FAST", fast)
    logits, reg, anchors, p = _arrays("thresh-0")
    assert (p == 0).sum() > 64
    for st in (-1e-3, -1.0):
        rc, _, _ = _run(logits, reg, anchors, (320, 320), None, st, 0.5, 64, 64)
        assert rc == -1, rc
    rc, outs, back = _run(logits, reg, anchors, (320, 320), None, 0.0, 0.5, 64, 64)
    _lib.check(rc, "dn_postprocess")
    assert _verify_all(outs, back, 0.0, 0.5, 64, 64, [(1.0, 1.0)]) == 48 and (outs[1][0][:48] > 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("fast", ["1", "0"])
@pytest.mark.parametrize("rc", ALL_RANDOM, ids=str)
def test_random_case_against_the_verifier(rc, fast, monkeypatch):
    """Random logits, every image compared in full (no `risky` images: the verifier starts from the device's scores). The input condition that
    makes the fp32 IoU comparison safe is asserted, not skipped on."""
    n, A, K, topk, dets, st, hw, seed = rc
    monkeypatch.setenv("DN_PP_FAST", fast)
    logits, reg, anchors = random_inputs(n, A, K, seed)
    scales = None if hw == (320, 320) else _random_scale(n)
    code, outs, back = _run(logits, reg, anchors, hw, scales, st, 0.5, topk, dets)
    _lib.check(code, "dn_postprocess")
    _front_half(back, logits, reg, anchors, hw)
    gap = min(psr.iou_band_gap(sm, dec, st, 0.5, topk) for sm, dec in back["inter"])
    print("random %s fast=%s: min |IoU - nms_thresh| over the device's candidate pairs %.3g, needFull %s" % (rc, fast, gap, back["needFull"].tolist()))
    if fast == "0":
        assert not back["tauKey"].any() and not back["needFull"].any(), "DN_PP_FAST=0 ran the cut-off path"
    assert gap >= 1e-6, "input condition: a candidate pair within 1e-6 of the NMS threshold"
    total = _verify_all(outs, back, st, 0.5, topk, dets, scales or [(1.0, 1.0)] * n)
    assert (total == 0) == (st > 0.99)


# ---- the paths only a model forward reaches (level table: PERM; fused head epilogue: scores_ready) ------------------------------------------------
def _model(name, ncls, **kw):
    m = getattr(models, name)(num_classes=ncls, **kw)
    models.load_synthetic(m, 0)
    return m.cuda()


def _hard_op_on_heads(m, imgs):
    logits, reg = m.forward_heads(imgs)
    anchors = torch.from_numpy(m._lowered.anchors).cuda()
    W, H = m.graph.size
    L = _lib.lib()
    n, A, K = logits.shape
    D, topk = m.detections_per_img, m.topk_candidates
    ws = torch.empty(L.dn_postprocess_workspace_bytes(n, A, K, topk, D), dtype=torch.uint8, device="cuda")
    boxes = torch.empty(n, D, 4, device="cuda"); scores = torch.empty(n, D, device="cuda")
    labels = torch.empty(n, D, dtype=torch.int64, device="cuda"); counts = torch.empty(n, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(L.dn_postprocess(p(logits), p(reg), p(anchors), n, A, K, float(H), float(W), None, float(m.score_thresh), float(m.nms_thresh),
                                int(topk), int(D), p(boxes), p(scores), p(labels), p(counts), None, p(ws), ws.numel(),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dn_postprocess")
    torch.cuda.synchronize()
    return boxes, scores, labels, counts


# the V2 model at other network sizes, the epilogue allowed from one image per chain: it engages where the levels of >= 32 pixels are the
# pyramid levels 0 .. k of the fused head launch (at 160 level 0 alone: level 1 is 5 x 5) and not at 512, whose 32-wide level 0 is outside it
_V2_SIZES = [(160, True), (192, True), (301, True), (496, True), (512, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,n,minn,epilogue",
                         [("ssdlite320_mobilenet_v3_large", {}, 3, None, False), ("ssdlite320_mobilenet_v3_large", {}, 37, 16, True),
                          ("ssd_lite_mobilenet_v2", dict(image_size=300, score_thresh=0.01), 3, None, False), ("ssd300_vgg16", {}, 3, None, False)]
                         + [("ssd_lite_mobilenet_v2", dict(image_size=s, score_thresh=0.01), 3, 1, e) for s, e in _V2_SIZES],
                         ids=["v3-n3", "v3-n37-epilogue", "v2-300-n3", "vgg300-n3"] + [f"v2-{s}-n3-minn1" for s, _ in _V2_SIZES])
def test_model_forward_in_hard_mode_is_the_op_on_its_head_outputs(name, kw, n, minn, epilogue, monkeypatch):
    """model.forward_batch == dn_postprocess(forward_heads) bit for bit (labels, scores, boxes, counts): the forward's post-process reads scores
    stored through the plan's level table, and with the fused head epilogue (37 images: chains of 19 and 18 at a threshold of 16) scores the
    head launch computed -- neither can be reached through dn_postprocess, whose exactness the rest of this module holds."""
    raw = C.CDLL(_lib.LIB_PATH)
    if minn is not None:
        monkeypatch.setenv("DN_HEAD_SOFTMAX_MINN", str(minn))
    m = _model(name, 21, **kw)
    assert m.nms_method == "hard"
    W, H = m.graph.size
    imgs = torch.from_numpy(synth.images(71, n, H, W)).cuda()
    before = raw.dn_debug_head_softmax_launches()
    got = [t.clone() for t in m.forward_batch(imgs)]
    assert (raw.dn_debug_head_softmax_launches() - before >= 1) == epilogue
    ref = _hard_op_on_heads(m, imgs)
    for x, y, what in zip(got, ref, ("boxes", "scores", "labels", "counts")):
        assert torch.equal(x, y), what
    assert int(got[3].sum()) > 0
