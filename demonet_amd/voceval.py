"""PASCAL VOC scoring with the per-image work on the device.

The reference's `voc_eval` (demonet/data/voc_eval.py:116-155, restated on the host in `evalrec.voc_class_pr`) marks every detection of a
class as a true or a false positive. Claims on a ground truth only interact inside one image and one class, so that marking runs per image
on the device (`dn_match_detections`, csrc/evalmatch.hip) on the arrays the forward just wrote, in the forward's stream, for several overlap
thresholds at once. What needs the whole image set -- the per-class order by confidence and the cumulative sums -- runs once, in
`VocAccumulator.summarize`: one stable sort and one cumulative sum on the device, then precision / recall and `evalrec.voc_ap` in float64 on
the host. On tie-free scores the result is `evalrec.voc_mean_ap`'s, number for number.

Flags: one 32-bit word per detection slot, bit b = true positive at thresholds[b], bit 16 + b = false positive at thresholds[b], neither = the
best match is a "difficult" ground truth (ignored, voc_eval.py:140). The library writes uint32; the tensors here are int32 with the same bits.
"""
import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib, evalrec

MAX_D = 512                 # detection slots per image
MAX_GT = 1024               # ground-truth boxes per image
MAX_THRESHOLDS = 16
MAX_IMAGES = 65535          # images per call

COCO_THRESHOLDS = tuple(round(0.5 + 0.05 * i, 2) for i in range(10))      # 0.5 : 0.05 : 0.95, for `map_avg`


def pad_targets(targets: Sequence[Dict[str, Tensor]], device):
    """The reference's target dicts (`boxes` [k, 4] xyxy, `labels` [k], optional `difficult` [k]) as the padded arrays dn_ssd_loss and
    dn_match_detections take: (gt_boxes [n, gmax, 4] fp32, gt_labels [n, gmax] int64, gt_difficult [n, gmax] uint8, gt_counts [n] int32) on
    `device`, gmax = the largest count (at least 1). No host synchronisation: the sizes come from the shapes. ValueError above 1 024 boxes."""
    device = torch.device(device)
    lens = [int(t["boxes"].reshape(-1, 4).shape[0]) for t in targets]
    if not lens:
        raise ValueError("pad_targets: no targets")
    if max(lens) > MAX_GT:
        raise ValueError("pad_targets: an image with {} ground-truth boxes, at most {} are taken".format(max(lens), MAX_GT))
    n, gmax = len(lens), max(1, max(lens))
    boxes = torch.zeros((n * gmax, 4), dtype=torch.float32, device=device)
    labels = torch.zeros((n * gmax,), dtype=torch.int64, device=device)
    difficult = torch.zeros((n * gmax,), dtype=torch.uint8, device=device)
    counts = torch.tensor(lens, dtype=torch.int32).to(device, non_blocking=True)
    if sum(lens):
        rows = torch.tensor([i * gmax + k for i, c in enumerate(lens) for k in range(c)], dtype=torch.int64).to(device, non_blocking=True)
        live = [t for t, c in zip(targets, lens) if c]

        def cat(parts, dtype):                                # joined where the parts lie, then moved once
            parts = [torch.as_tensor(p) for p in parts]
            if len({p.device for p in parts}) > 1:
                parts = [p.to(device) for p in parts]
            return torch.cat([p.to(dtype) for p in parts]).to(device, non_blocking=True)

        boxes.index_copy_(0, rows, cat([t["boxes"].reshape(-1, 4) for t in live], torch.float32))
        labels.index_copy_(0, rows, cat([t["labels"].reshape(-1) for t in live], torch.int64))
        if any("difficult" in t for t in live):
            diff = [torch.as_tensor(t["difficult"]).reshape(-1) != 0 if "difficult" in t else torch.zeros(c, dtype=torch.bool)
                    for t, c in zip(targets, lens) if c]
            difficult.index_copy_(0, rows, cat(diff, torch.uint8))
    return boxes.view(n, gmax, 4), labels.view(n, gmax), difficult.view(n, gmax), counts


def _voc_ap(rec: np.ndarray, prec: np.ndarray, use_07_metric: bool) -> float:
    """`evalrec.voc_ap`, number for number, with the precision envelope (voc_eval.py:50-51, a Python loop over every detection there) as one
    reversed running maximum: a maximum does not round, so the order of taking it does not matter. The loop is 97 % of `summarize` on 600 k
    detections (profiles/voc_eval_timing.json); tests/test_evalmatch.py holds every AP to `evalrec.voc_ap` with ==."""
    if use_07_metric:
        return evalrec.voc_ap(rec, prec, True)
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.maximum.accumulate(np.concatenate(([0.0], prec, [0.0]))[::-1])[::-1]
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


def _thresholds(thresholds) -> List[float]:
    thr = [float(t) for t in thresholds]
    if not 1 <= len(thr) <= MAX_THRESHOLDS:
        raise ValueError("{} thresholds, 1 .. {} are taken".format(len(thr), MAX_THRESHOLDS))
    if any(t != t for t in thr):
        raise ValueError("a threshold is NaN")
    return thr


def match_detections(boxes: Tensor, scores: Tensor, labels: Tensor, counts: Tensor, gt_boxes: Tensor, gt_labels: Tensor,
                     gt_difficult: Optional[Tensor], gt_counts: Tensor, thresholds=(0.5,), pixel_offset: float = 1.0,
                     gt_stats: Optional[Tensor] = None, return_best: bool = False):
    """dn_match_detections on tensors, one call on the current stream: boxes [n, d, 4] fp32, scores [n, d] fp32, labels [n, d] int64, counts [n]
    int32 (what forward_batch returns) against gt_boxes [n, gmax, 4] fp32, gt_labels [n, gmax] int64, gt_difficult [n, gmax] uint8 (or None),
    gt_counts [n] int32 (`pad_targets`). gt_stats, when given ([num_classes, 2] int64 on the same device), is ADDED to: per class the number of
    (not difficult, difficult) ground truths. Returns flags [n, d] int32 (see the module's docstring), with return_best=True
    (flags, best_gt [n, d] int32, best_ov [n, d] float64). Semantics: include/demonet_hip.h."""
    thr = _thresholds(thresholds)
    if scores.dim() != 2 or gt_labels.dim() != 2:
        raise ValueError("match_detections: scores must be [n, d] and gt_labels [n, gmax], got {} and {}".format(tuple(scores.shape), tuple(gt_labels.shape)))
    n, d = scores.shape
    gmax = gt_labels.shape[1]
    dev = scores.device
    want = [("boxes", boxes, (n, d, 4), torch.float32), ("scores", scores, (n, d), torch.float32), ("labels", labels, (n, d), torch.int64),
            ("counts", counts, (n,), torch.int32), ("gt_boxes", gt_boxes, (n, gmax, 4), torch.float32), ("gt_labels", gt_labels, (n, gmax), torch.int64),
            ("gt_counts", gt_counts, (n,), torch.int32)]
    if gt_difficult is not None:
        want.append(("gt_difficult", gt_difficult, (n, gmax), torch.uint8))
    if gt_stats is not None:
        if gt_stats.dim() != 2 or gt_stats.shape[1] != 2:
            raise ValueError("match_detections: gt_stats must be [num_classes, 2], got {}".format(tuple(gt_stats.shape)))
        want.append(("gt_stats", gt_stats, tuple(gt_stats.shape), torch.int64))
    for name, t, shape, dtype in want:
        if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev or dev.type != "cuda":
            raise ValueError("match_detections: {} must be a contiguous {} tensor of shape {} on the GPU, got {} {} on {}".format(
                name, dtype, shape, t.dtype, tuple(t.shape), t.device))
    if n < 1 or d < 1 or gmax < 1 or d > MAX_D or gmax > MAX_GT or n > MAX_IMAGES:
        raise ValueError("match_detections: n={} (1 .. {}), d={} (1 .. {}), gmax={} (1 .. {})".format(n, MAX_IMAGES, d, MAX_D, gmax, MAX_GT))
    flags = torch.empty((n, d), dtype=torch.int32, device=dev)
    best_gt = torch.empty((n, d), dtype=torch.int32, device=dev) if return_best else None
    best_ov = torch.empty((n, d), dtype=torch.float64, device=dev) if return_best else None
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dn_match_detections(p(boxes), p(scores), p(labels), p(counts), p(gt_boxes), p(gt_labels), p(gt_difficult), p(gt_counts),
                                                  n, d, gmax, int(gt_stats.shape[0]) if gt_stats is not None else 0,
                                                  (C.c_double * len(thr))(*thr), len(thr), float(pixel_offset), p(flags), p(best_gt), p(best_ov),
                                                  p(gt_stats), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "dn_match_detections")
    return (flags, best_gt, best_ov) if return_best else flags


class VocAccumulator:
    """Detections of an image set, marked per image, and their PASCAL VOC score.

        acc = VocAccumulator(num_classes=21, thresholds=(0.5, 0.75))
        for images, targets in loader:
            acc.update(*model.forward_batch(images), targets)      # matched on the device, nothing comes to the host
        print(acc.summarize()["map"])

    `map_avg` with thresholds 0.5 : 0.05 : 0.95 (`COCO_THRESHOLDS`) is a convenience under VOC matching rules. It is NOT COCOeval: no crowd
    regions, no area ranges, no maxDets, a detection is compared only with the ground truth it overlaps most."""

    def __init__(self, num_classes: int, thresholds=(0.5,), pixel_offset: float = 1.0):
        if num_classes < 1:
            raise ValueError("num_classes must be positive")
        self.num_classes = int(num_classes)
        self.thresholds = _thresholds(thresholds)
        self.pixel_offset = float(pixel_offset)
        if not (0.0 <= self.pixel_offset < float("inf")):
            raise ValueError("pixel_offset must be finite and not negative")
        self._chunks = []           # (scores, labels, counts, flags): [n, d], [n, d], [n], [n, d], where they were produced
        self._gt_stats = []         # one [num_classes, 2] int64 tensor per device seen

    def _stats_on(self, device) -> Tensor:
        for t in self._gt_stats:
            if t.device == device:
                return t
        t = torch.zeros((self.num_classes, 2), dtype=torch.int64, device=device)
        self._gt_stats.append(t)
        return t

    def update(self, boxes: Tensor, scores: Tensor, labels: Tensor, counts: Tensor, targets):
        """One batch: the padded outputs of a forward and the reference's target dicts of the same images (or the tuple `pad_targets`
        returns). Matches on the device on the current stream and keeps copies of scores, labels, counts and the flags there; no host
        synchronisation, so the forward's own output buffers may be overwritten by whatever is enqueued after this call."""
        gt = targets if isinstance(targets, tuple) else pad_targets(targets, scores.device)
        flags = match_detections(boxes, scores, labels, counts, *gt, thresholds=self.thresholds, pixel_offset=self.pixel_offset,
                                 gt_stats=self._stats_on(scores.device))
        self._chunks.append((scores.clone(), labels.clone(), counts.clone(), flags))

    def append(self, scores: Tensor, labels: Tensor, counts: Tensor, flags: Tensor, gt_stats: Tensor):
        """The bookkeeping of `update` without the kernel, for flags made elsewhere (CPU tensors too): scores [n, d], labels [n, d], counts [n],
        flags [n, d] int32, gt_stats [num_classes, 2] = this batch's ground-truth counts. The tensors are kept, not copied."""
        n, d = scores.shape
        if tuple(labels.shape) != (n, d) or tuple(flags.shape) != (n, d) or tuple(counts.shape) != (n,) or tuple(gt_stats.shape) != (self.num_classes, 2):
            raise ValueError("append: expected scores, labels, flags [n, d], counts [n] and gt_stats [{}, 2]".format(self.num_classes))
        self._chunks.append((scores, labels.to(torch.int64), counts, flags.to(torch.int32)))
        self._stats_on(scores.device).add_(gt_stats.to(device=scores.device, dtype=torch.int64))

    def summarize(self, use_07_metric: bool = False) -> dict:
        """{"map": [mean AP in percent per threshold], "ap": {class: [AP in percent per threshold]}, "map_avg": the mean of "map"} over the
        classes that occur in the ground truth, difficult boxes included (as evalrec.voc_mean_ap chooses them). Per class the detections are
        ordered by one stable descending sort on the score (ties keep batch, image, slot order; NaN last, as np.argsort(-score) puts them), the
        TP / FP bits are summed cumulatively in int64, and recall, precision (voc_eval.py:157-161) and evalrec.voc_ap's numbers (`_voc_ap`)
        follow on the host in float64. A class without detections scores 0."""
        T = len(self.thresholds)
        stats = np.zeros((self.num_classes, 2), dtype=np.int64)
        for t in self._gt_stats:
            stats += t.cpu().numpy()
        classes = [int(c) for c in np.nonzero(stats.sum(1) > 0)[0]]
        ap = {c: [0.0] * T for c in classes}
        if self._chunks and classes:
            dev = self._chunks[-1][0].device
            s, lab, fl = [], [], []
            for scores, labels, counts, flags in self._chunks:
                live = (torch.arange(scores.shape[1], device=scores.device)[None, :] < counts[:, None].to(torch.int64)).reshape(-1)
                s.append(scores.reshape(-1)[live].to(dev))
                lab.append(labels.reshape(-1)[live].to(dev))
                fl.append(flags.reshape(-1)[live].to(dev))
            s, lab, fl = torch.cat(s), torch.cat(lab), torch.cat(fl)
            by_score = torch.sort(-s, stable=True).indices           # descending, stable
            by_class = torch.sort(lab[by_score], stable=True)                          # classes ascending, each in confidence order
            fl = fl[by_score[by_class.indices]]
            shifts = torch.arange(T, device=dev, dtype=torch.int32)[:, None]
            tp = torch.cumsum(((fl[None, :] >> shifts) & 1).to(torch.int64), dim=1).cpu().numpy()
            fp = torch.cumsum(((fl[None, :] >> (shifts + 16)) & 1).to(torch.int64), dim=1).cpu().numpy()
            lab_sorted = by_class.values.cpu().numpy()
            for c in classes:
                lo, hi = np.searchsorted(lab_sorted, c, "left"), np.searchsorted(lab_sorted, c, "right")
                if hi == lo:
                    continue
                npos = int(stats[c, 0])
                for b in range(T):
                    tpc = (tp[b, lo:hi] - (tp[b, lo - 1] if lo else 0)).astype(np.float64)
                    fpc = (fp[b, lo:hi] - (fp[b, lo - 1] if lo else 0)).astype(np.float64)
                    rec = tpc / float(npos) if npos > 0 else np.zeros_like(tpc)
                    prec = tpc / np.maximum(tpc + fpc, np.finfo(np.float64).eps)
                    ap[c][b] = 100.0 * _voc_ap(rec, prec, use_07_metric)
        maps = [float(np.mean([ap[c][b] for c in classes])) if classes else 0.0 for b in range(T)]
        return {"map": maps, "ap": ap, "map_avg": float(np.mean(maps))}

    def class_pr(self, cls: int, threshold_index: int = 0):
        """(recall, precision) per detection of one class in confidence order, as evalrec.voc_class_pr returns them (float64, host)."""
        s, fl = [], []
        for scores, labels, counts, flags in self._chunks:
            live = (torch.arange(scores.shape[1], device=scores.device)[None, :] < counts[:, None].to(torch.int64)) & (labels == cls)
            s.append(scores[live].cpu())
            fl.append(flags[live].cpu())
        s, fl = (torch.cat(s), torch.cat(fl)) if s else (torch.zeros(0), torch.zeros(0, dtype=torch.int32))
        fl = fl[torch.sort(-s, stable=True).indices]
        tp = torch.cumsum(((fl >> threshold_index) & 1).to(torch.int64), 0).numpy().astype(np.float64)
        fp = torch.cumsum(((fl >> (16 + threshold_index)) & 1).to(torch.int64), 0).numpy().astype(np.float64)
        npos = sum(int(t[cls, 0]) for t in self._gt_stats)
        rec = tp / float(npos) if npos > 0 else np.zeros_like(tp)
        return rec, tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
