"""The semantics of dn_match_detections (include/demonet_hip.h) as a literal numpy loop: per image the candidates, the best ground
truth of each by numpy's float64 arithmetic, a stable rank, and THE SEQUENTIAL WALK of voc_eval (data/voc_eval.py:116-155 of the reference) with
one "claimed" bit per ground truth -- not the min-table formulation the kernel uses. `pixel_offset` is a parameter (the reference has 1)."""
import numpy as np

TP0, FP0 = 0, 16      # bit of threshold 0 in a flags word


def match_ref(boxes, scores, labels, counts, gt_boxes, gt_labels, gt_difficult, gt_counts, thresholds, pixel_offset=1.0, num_classes=0):
    """boxes [n,d,4] f32, scores [n,d] f32, labels [n,d] i64, counts [n]; gt_boxes [n,gmax,4] f32, gt_labels [n,gmax] i64, gt_difficult [n,gmax] or
    None, gt_counts [n] -> (flags [n,d] uint32, best_gt [n,d] int32, best_ov [n,d] float64, gt_stats [num_classes,2] int64)."""
    n, d = scores.shape
    o = np.float64(pixel_offset)
    flags = np.zeros((n, d), np.uint32)
    best_gt = np.full((n, d), -1, np.int32)
    best_ov = np.zeros((n, d), np.float64)
    stats = np.zeros((max(int(num_classes), 0), 2), np.int64)
    for i in range(n):
        c, g = int(counts[i]), int(gt_counts[i])
        gb = gt_boxes[i, :g].astype(np.float64)
        gl = gt_labels[i, :g]
        gd = np.zeros(g, bool) if gt_difficult is None else gt_difficult[i, :g].astype(bool)
        for k in range(g):                                            # 5. ground-truth counts
            if 0 <= gl[k] < num_classes:
                stats[gl[k], 1 if gd[k] else 0] += 1
        with np.errstate(all="ignore"):
            for j in range(c):                                        # 1., 2. best ground truth of every candidate
                bb = boxes[i, j].astype(np.float64)
                ks = np.nonzero(gl == labels[i, j])[0]
                if ks.size == 0:
                    best_ov[i, j], best_gt[i, j] = -np.inf, -1
                    continue
                q = gb[ks]
                iw = np.maximum(np.minimum(q[:, 2], bb[2]) - np.maximum(q[:, 0], bb[0]) + o, 0.0)
                ih = np.maximum(np.minimum(q[:, 3], bb[3]) - np.maximum(q[:, 1], bb[1]) + o, 0.0)
                inter = iw * ih
                union = (bb[2] - bb[0] + o) * (bb[3] - bb[1] + o) + (q[:, 2] - q[:, 0] + o) * (q[:, 3] - q[:, 1] + o) - inter
                ov = inter / union
                if np.isnan(ov).any():
                    best_ov[i, j], best_gt[i, j] = np.nan, -1
                else:
                    best_ov[i, j], best_gt[i, j] = ov.max(), ks[int(np.argmax(ov))]
        s = scores[i, :c].astype(np.float64)                          # 3. score descending, NaN last, ties by ascending slot
        nan = np.isnan(s)
        order = np.lexsort((np.arange(c), np.where(nan, 0.0, -s), nan))
        for b, t in enumerate(thresholds):                            # 4. the walk
            t = np.float64(t)
            claimed = np.zeros(g, bool)
            for j in order:
                k = int(best_gt[i, j])
                if best_ov[i, j] > t:
                    if not gd[k]:
                        if not claimed[k]:
                            flags[i, j] |= np.uint32(1 << (TP0 + b))
                            claimed[k] = True
                        else:
                            flags[i, j] |= np.uint32(1 << (FP0 + b))
                else:
                    flags[i, j] |= np.uint32(1 << (FP0 + b))
    return flags, best_gt, best_ov, stats


def pad_records(dets, d):
    """[{boxes [k,4], scores [k], labels [k]}, ...] (numpy or tensors) -> padded (boxes [n,d,4] f32, scores [n,d] f32, labels [n,d] i64, counts [n] i32)"""
    n = len(dets)
    boxes, scores, labels = np.zeros((n, d, 4), np.float32), np.zeros((n, d), np.float32), np.zeros((n, d), np.int64)
    counts = np.zeros(n, np.int32)
    for i, r in enumerate(dets):
        c = len(r["scores"])
        assert c <= d
        counts[i] = c
        boxes[i, :c], scores[i, :c], labels[i, :c] = np.asarray(r["boxes"]).reshape(-1, 4), np.asarray(r["scores"]), np.asarray(r["labels"])
    return boxes, scores, labels, counts


def pad_gt(gts, gmax=None):
    """[{boxes [k,4], labels [k], optional difficult [k]}, ...] -> (gt_boxes [n,gmax,4] f32, gt_labels [n,gmax] i64, gt_difficult [n,gmax] u8, gt_counts)"""
    n = len(gts)
    gmax = gmax or max(1, max(len(g["labels"]) for g in gts))
    boxes, labels, diff = np.zeros((n, gmax, 4), np.float32), np.zeros((n, gmax), np.int64), np.zeros((n, gmax), np.uint8)
    counts = np.zeros(n, np.int32)
    for i, g in enumerate(gts):
        k = len(g["labels"])
        counts[i] = k
        boxes[i, :k], labels[i, :k] = np.asarray(g["boxes"]).reshape(-1, 4), np.asarray(g["labels"])
        if "difficult" in g:
            diff[i, :k] = np.asarray(g["difficult"]).astype(np.uint8)
    return boxes, labels, diff, counts
