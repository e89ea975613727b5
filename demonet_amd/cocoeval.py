"""COCO detection metrics with the per-image work on the device.

The reference's `CocoEvaluator` (demonet/data/coco_eval.py:23-64) hands every batch to pycocotools' `COCOeval`: `evaluateImg` matches the
detections of one (image, category) greedily against its ground truths, per IoU threshold and area range, `accumulate` orders a category's
detections over the whole set and interpolates precision at 101 recalls, `summarize` averages the twelve numbers. Matches only interact inside
one image and one category, so the matching runs per image on the device (`dn_coco_match`, csrc/cocomatch.hip) on the arrays the forward just
wrote, in the forward's stream, for all thresholds and area ranges at once. What needs the whole image set runs once, in
`CocoAccumulator.summarize`: two stable sorts and the cumulative sums on the device, then recall, precision and the interpolation in float64
on the host. pycocotools is not installed where this project runs; its arithmetic is restated in tests/cocoeval_ref.py.

Flags: one 32-bit word per (detection slot, area range), bit b = matched at thresholds[b], bit 16 + b = ignored at thresholds[b]; a true positive
is matched and not ignored, a false positive neither. The library writes uint32; the tensors here are int32 with the same bits.
"""
import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib

MAX_D = 512                 # detection slots per image
MAX_GT = 1024               # ground-truth boxes per image
MAX_THRESHOLDS = 16
MAX_RANGES = 4
MAX_DET = 128               # the largest maxDets
MAX_IMAGES = 65535          # images per call

IOU_THRESHOLDS = np.linspace(.5, .95, 10)
RECALL_THRESHOLDS = np.linspace(0, 1, 101)
AREA_RANGES = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))      # all, small, medium, large
STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")


def pad_targets(targets: Sequence[Dict[str, Tensor]], device):
    """The reference's target dicts (`boxes` [k, 4] xyxy, `labels` [k], optional `iscrowd` [k], optional `area` [k]) as the padded arrays
    dn_coco_match takes: (gt_boxes [n, gmax, 4] fp32, gt_labels [n, gmax] int64, gt_counts [n] int32, gt_crowd [n, gmax] uint8, gt_area
    [n, gmax] fp32) on `device`, gmax = the largest count (at least 1). A target without `area` gets fp32 w * h of its box (w, h subtracted in
    fp32). No host synchronisation: the sizes come from the shapes. ValueError above 1 024 boxes."""
    device = torch.device(device)
    lens = [int(t["boxes"].reshape(-1, 4).shape[0]) for t in targets]
    if not lens:
        raise ValueError("pad_targets: no targets")
    if max(lens) > MAX_GT:
        raise ValueError("pad_targets: an image with {} ground-truth boxes, at most {} are taken".format(max(lens), MAX_GT))
    n, gmax = len(lens), max(1, max(lens))
    boxes = torch.zeros((n * gmax, 4), dtype=torch.float32, device=device)
    labels = torch.zeros((n * gmax,), dtype=torch.int64, device=device)
    crowd = torch.zeros((n * gmax,), dtype=torch.uint8, device=device)
    area = torch.zeros((n * gmax,), dtype=torch.float32, device=device)
    counts = torch.tensor(lens, dtype=torch.int32).to(device, non_blocking=True)
    if sum(lens):
        rows = torch.tensor([i * gmax + k for i, c in enumerate(lens) for k in range(c)], dtype=torch.int64).to(device, non_blocking=True)
        live = [t for t, c in zip(targets, lens) if c]

        def cat(parts, dtype):                                # joined where the parts lie, then moved once
            parts = [torch.as_tensor(p) for p in parts]
            if len({p.device for p in parts}) > 1:
                parts = [p.to(device) for p in parts]
            return torch.cat([p.to(dtype) for p in parts]).to(device, non_blocking=True)

        def box_area(t):
            b = torch.as_tensor(t["boxes"]).reshape(-1, 4).to(torch.float32)
            return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])

        boxes.index_copy_(0, rows, cat([t["boxes"].reshape(-1, 4) for t in live], torch.float32))
        labels.index_copy_(0, rows, cat([t["labels"].reshape(-1) for t in live], torch.int64))
        if any("iscrowd" in t for t in live):
            parts = [torch.as_tensor(t["iscrowd"]).reshape(-1) != 0 if "iscrowd" in t else torch.zeros(c, dtype=torch.bool)
                     for t, c in zip(targets, lens) if c]
            crowd.index_copy_(0, rows, cat(parts, torch.uint8))
        area.index_copy_(0, rows, cat([torch.as_tensor(t["area"]).reshape(-1) if "area" in t else box_area(t) for t in live], torch.float32))
    return boxes.view(n, gmax, 4), labels.view(n, gmax), counts, crowd.view(n, gmax), area.view(n, gmax)


def _thresholds(thresholds):
    thr = [float(t) for t in thresholds]
    if not 1 <= len(thr) <= MAX_THRESHOLDS:
        raise ValueError("{} thresholds, 1 .. {} are taken".format(len(thr), MAX_THRESHOLDS))
    if any(t != t for t in thr):
        raise ValueError("a threshold is NaN")
    return thr


def _ranges(area_ranges):
    rng = [(float(lo), float(hi)) for lo, hi in area_ranges]
    if not 1 <= len(rng) <= MAX_RANGES:
        raise ValueError("{} area ranges, 1 .. {} are taken".format(len(rng), MAX_RANGES))
    if any(v != v for r in rng for v in r):
        raise ValueError("an area range holds a NaN")
    return rng


def coco_match(boxes: Tensor, scores: Tensor, labels: Tensor, counts: Tensor, gt_boxes: Tensor, gt_labels: Tensor, gt_counts: Tensor,
               gt_crowd: Optional[Tensor] = None, gt_area: Optional[Tensor] = None, thresholds=IOU_THRESHOLDS, area_ranges=AREA_RANGES,
               max_det: int = 100, gt_stats: Optional[Tensor] = None, return_match: bool = False):
    """dn_coco_match on tensors, one call on the current stream: boxes [n, d, 4] fp32, scores [n, d] fp32, labels [n, d] int64, counts [n] int32
    (what forward_batch returns) against gt_boxes [n, gmax, 4] fp32, gt_labels [n, gmax] int64, gt_counts [n] int32, gt_crowd [n, gmax] uint8 (or
    None), gt_area [n, gmax] fp32 (or None: w * h of the box) (`pad_targets`). gt_stats, when given ([num_classes, R] int64 on the same device), is
    ADDED to: per label and area range the number of ground truths that are not ignored. Returns (flags [n, d, R] int32, rank [n, d] int32), with
    return_match=True also match_gt [n, d, R, T] int32. Semantics: include/demonet_hip.h."""
    thr, rng = _thresholds(thresholds), _ranges(area_ranges)
    T, R = len(thr), len(rng)
    if not 1 <= int(max_det) <= MAX_DET:
        raise ValueError("coco_match: max_det={} (1 .. {})".format(max_det, MAX_DET))
    if scores.dim() != 2 or gt_labels.dim() != 2:
        raise ValueError("coco_match: scores must be [n, d] and gt_labels [n, gmax], got {} and {}".format(tuple(scores.shape), tuple(gt_labels.shape)))
    n, d = scores.shape
    gmax = gt_labels.shape[1]
    dev = scores.device
    want = [("boxes", boxes, (n, d, 4), torch.float32), ("scores", scores, (n, d), torch.float32), ("labels", labels, (n, d), torch.int64),
            ("counts", counts, (n,), torch.int32), ("gt_boxes", gt_boxes, (n, gmax, 4), torch.float32), ("gt_labels", gt_labels, (n, gmax), torch.int64),
            ("gt_counts", gt_counts, (n,), torch.int32)]
    if gt_crowd is not None:
        want.append(("gt_crowd", gt_crowd, (n, gmax), torch.uint8))
    if gt_area is not None:
        want.append(("gt_area", gt_area, (n, gmax), torch.float32))
    if gt_stats is not None:
        if gt_stats.dim() != 2 or gt_stats.shape[1] != R:
            raise ValueError("coco_match: gt_stats must be [num_classes, {}], got {}".format(R, tuple(gt_stats.shape)))
        want.append(("gt_stats", gt_stats, tuple(gt_stats.shape), torch.int64))
    for name, t, shape, dtype in want:
        if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev or dev.type != "cuda":
            raise ValueError("coco_match: {} must be a contiguous {} tensor of shape {} on the GPU, got {} {} on {}".format(
                name, dtype, shape, t.dtype, tuple(t.shape), t.device))
    if n < 1 or d < 1 or gmax < 1 or d > MAX_D or gmax > MAX_GT or n > MAX_IMAGES:
        raise ValueError("coco_match: n={} (1 .. {}), d={} (1 .. {}), gmax={} (1 .. {})".format(n, MAX_IMAGES, d, MAX_D, gmax, MAX_GT))
    flags = torch.empty((n, d, R), dtype=torch.int32, device=dev)
    rank = torch.empty((n, d), dtype=torch.int32, device=dev)
    match_gt = torch.empty((n, d, R, T), dtype=torch.int32, device=dev) if return_match else None
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    flat = [v for r in rng for v in r]
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dn_coco_match(p(boxes), p(scores), p(labels), p(counts), p(gt_boxes), p(gt_labels), p(gt_counts), p(gt_crowd), p(gt_area),
                                            n, d, gmax, int(gt_stats.shape[0]) if gt_stats is not None else 0, (C.c_double * T)(*thr), T,
                                            (C.c_double * (2 * R))(*flat), R, int(max_det), p(flags), p(rank), p(match_gt), p(gt_stats),
                                            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "dn_coco_match")
    return (flags, rank, match_gt) if return_match else (flags, rank)


class CocoAccumulator:
    """Detections of an image set, matched per image, and their COCO numbers.

        acc = CocoAccumulator(num_classes=91)
        for images, targets in loader:
            acc.update(*model.forward_batch(images), targets)      # matched on the device, nothing comes to the host
        print(acc.summarize()["stats"][0])                          # AP @ [.50 : .05 : .95]

    Categories are the labels 0 .. num_classes - 1; detections and ground truths with other labels are not scored."""

    def __init__(self, num_classes: int, iou_thresholds=IOU_THRESHOLDS, area_ranges=AREA_RANGES, max_dets=(1, 10, 100)):
        if num_classes < 1:
            raise ValueError("num_classes must be positive")
        self.num_classes = int(num_classes)
        self.thresholds = _thresholds(iou_thresholds)
        self.area_ranges = _ranges(area_ranges)
        self.max_dets = [int(m) for m in max_dets]
        if not self.max_dets or any(m < 1 or m > MAX_DET for m in self.max_dets) or sorted(self.max_dets) != self.max_dets:
            raise ValueError("max_dets must be ascending and lie in 1 .. {}".format(MAX_DET))
        self._chunks = []           # (scores [n, d], labels [n, d], counts [n], flags [n, d, R], rank [n, d]), where they were produced
        self._gt_stats = []         # one [num_classes, R] int64 tensor per device seen

    def _stats_on(self, device) -> Tensor:
        for t in self._gt_stats:
            if t.device == device:
                return t
        t = torch.zeros((self.num_classes, len(self.area_ranges)), dtype=torch.int64, device=device)
        self._gt_stats.append(t)
        return t

    def update(self, boxes: Tensor, scores: Tensor, labels: Tensor, counts: Tensor, targets):
        """One batch: the padded outputs of a forward and the reference's target dicts of the same images (or the tuple `pad_targets`
        returns). Matches on the device on the current stream and keeps copies of scores, labels, counts, the flags and the ranks there; no
        host synchronisation, so the forward's own output buffers may be overwritten by whatever is enqueued after this call."""
        gt = targets if isinstance(targets, tuple) else pad_targets(targets, scores.device)
        flags, rank = coco_match(boxes, scores, labels, counts, *gt, thresholds=self.thresholds, area_ranges=self.area_ranges,
                                 max_det=self.max_dets[-1], gt_stats=self._stats_on(scores.device))
        self._chunks.append((scores.clone(), labels.clone(), counts.clone(), flags, rank))

    def append(self, scores: Tensor, labels: Tensor, counts: Tensor, flags: Tensor, rank: Tensor, gt_stats: Tensor):
        """The bookkeeping of `update` without the kernel, for flags made elsewhere (CPU tensors too): scores [n, d], labels [n, d], counts [n],
        flags [n, d, R] int32, rank [n, d] int32, gt_stats [num_classes, R] = this batch's not-ignored ground truths. The tensors are kept,
        not copied."""
        n, d = scores.shape
        R = len(self.area_ranges)
        if (tuple(labels.shape) != (n, d) or tuple(flags.shape) != (n, d, R) or tuple(rank.shape) != (n, d) or tuple(counts.shape) != (n,)
                or tuple(gt_stats.shape) != (self.num_classes, R)):
            raise ValueError("append: expected scores, labels, rank [n, d], flags [n, d, {}], counts [n] and gt_stats [{}, {}]".format(R, self.num_classes, R))
        self._chunks.append((scores, labels.to(torch.int64), counts, flags.to(torch.int32), rank.to(torch.int32)))
        self._stats_on(scores.device).add_(gt_stats.to(device=scores.device, dtype=torch.int64))

    def summarize(self) -> dict:
        """pycocotools' accumulate + summarize: {"stats": the twelve numbers in pycocotools' order (`STAT_NAMES`: AP, AP50, AP75, APs, APm, APl
        at the largest maxDets; AR at each of the three maxDets; ARs, ARm, ARl), "precision" [T, 101, K, A, M], "recall" [T, K, A, M]} as float64
        arrays, K = num_classes indexed by label, -1 where a (category, range) has no ground truth that counts. A stat is the mean of its slice's
        entries > -1, or -1 without any; AP50 / AP75 are found by value among the thresholds (-1 if absent); the size stats need the four area
        ranges in the order all, small, medium, large and the AR stats three maxDets (-1 otherwise).
        The detections of rank < maxDets are ordered by one stable descending sort on the score and one stable sort by label (NaN last, as
        np.argsort(-score, kind='mergesort') puts them); ties across images keep (batch, image, slot) order, which is pycocotools' order when
        the images arrive by ascending image id. tp = matched and not ignored, fp = neither, summed cumulatively in int64 on the device; recall =
        tp / npig, precision = tp / (fp + tp + spacing(1)), the precision envelope (a reversed running maximum) and its values at
        `RECALL_THRESHOLDS` (searchsorted 'left'; 0 beyond the last recall) follow on the host in float64."""
        T, A, M, K = len(self.thresholds), len(self.area_ranges), len(self.max_dets), self.num_classes
        Rn = len(RECALL_THRESHOLDS)
        precision = -np.ones((T, Rn, K, A, M))
        recall = -np.ones((T, K, A, M))
        npig = np.zeros((K, A), dtype=np.int64)
        for t in self._gt_stats:
            npig += t.cpu().numpy()
        populated = npig > 0
        precision[:, :, populated, :] = 0.0                    # a category with ground truth and no detection scores 0
        recall[:, populated, :] = 0.0
        if self._chunks and populated.any():
            dev = self._chunks[-1][0].device
            s, lab, fl, rk = [], [], [], []
            for scores, labels, counts, flags, rank in self._chunks:
                live = (torch.arange(scores.shape[1], device=scores.device)[None, :] < counts[:, None].to(torch.int64)).reshape(-1)
                live &= (rank.reshape(-1) >= 0) & (rank.reshape(-1) < self.max_dets[-1])
                live &= (labels.reshape(-1) >= 0) & (labels.reshape(-1) < K)
                s.append(scores.reshape(-1)[live].to(dev))
                lab.append(labels.reshape(-1)[live].to(dev))
                fl.append(flags.reshape(-1, A)[live].to(dev))
                rk.append(rank.reshape(-1)[live].to(dev))
            s, lab, fl, rk = torch.cat(s), torch.cat(lab), torch.cat(fl), torch.cat(rk)
            by_score = torch.sort(-s, stable=True).indices             # descending, stable
            by_class = torch.sort(lab[by_score], stable=True)          # categories ascending, each in confidence order
            order = by_score[by_class.indices]
            fl, rk, lab = fl[order], rk[order], by_class.values
            shifts = torch.arange(T, device=dev, dtype=torch.int32)[:, None]
            for m, max_det in enumerate(self.max_dets):
                keep = torch.nonzero(rk < max_det).reshape(-1)
                lab_m = lab[keep].cpu().numpy()
                for a in range(A):
                    w = fl[keep, a][None, :]
                    matched, ignored = ((w >> shifts) & 1) != 0, ((w >> (shifts + 16)) & 1) != 0
                    tp_all = torch.cumsum((matched & ~ignored).to(torch.int64), dim=1).cpu().numpy()
                    fp_all = torch.cumsum((~matched & ~ignored).to(torch.int64), dim=1).cpu().numpy()
                    for k in np.nonzero(populated[:, a])[0]:
                        lo, hi = np.searchsorted(lab_m, k, "left"), np.searchsorted(lab_m, k, "right")
                        if hi == lo:
                            continue
                        tp = (tp_all[:, lo:hi] - (tp_all[:, lo - 1:lo] if lo else 0)).astype(np.float64)
                        fp = (fp_all[:, lo:hi] - (fp_all[:, lo - 1:lo] if lo else 0)).astype(np.float64)
                        rc = tp / float(npig[k, a])
                        pr = tp / (fp + tp + np.spacing(1))
                        recall[:, k, a, m] = rc[:, -1]
                        pr = np.concatenate((np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1], np.zeros((T, 1))), axis=1)      # envelope; 0 off the end
                        for b in range(T):
                            precision[b, :, k, a, m] = pr[b, np.searchsorted(rc[b], RECALL_THRESHOLDS, side="left")]

        def mean(x):
            x = x[x > -1]
            return float(np.mean(x)) if x.size else -1.0

        thr = np.asarray(self.thresholds)

        def ap(value=None, a=0):
            if a >= A:
                return -1.0
            rows = precision if value is None else precision[np.where(value == thr)[0]]
            return mean(rows[:, :, :, a, M - 1])

        def ar(a=0, m=M - 1):
            return mean(recall[:, :, a, m]) if a < A else -1.0

        stats = [ap(), ap(.5), ap(.75), ap(a=1), ap(a=2), ap(a=3), ar(m=0) if M == 3 else -1.0, ar(m=1) if M == 3 else -1.0, ar(), ar(a=1), ar(a=2), ar(a=3)]
        return {"stats": stats, "precision": precision, "recall": recall}
