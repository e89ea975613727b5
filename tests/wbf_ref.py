"""TEST INFRASTRUCTURE: the reference of weighted boxes fusion (demonet_amd/fusion.py, csrc/fuse.hip).

`fuse` restates the eight sentences of include/demonet_hip.h (dn_fuse_detections) in numpy float32, statement by statement, as a Python loop over
the candidates in rank order; only the comparison of one candidate with the clusters of its label is a numpy expression -- elementwise float32, so
every value is what the scalar formula gives. A correct device implementation must agree with it bit for bit. `defect` plants one deviation from
the text at a time (tests/test_wbf.py shows that each of them is visible).

`fuse64` is the published algorithm (Solovyev, Wang, Gabruseva 2019; ensemble_boxes.weighted_boxes_fusion, conf_type 'avg') in float64 on the same
candidates: every cluster keeps its member list and its fused box is recomputed from the whole list after every append. It also returns the
smallest |IoU - thresh| it met: `fuse` and `fuse64` can only be asked to agree on an input where that margin is comfortably positive.
"""
import numpy as np

f32 = np.float32
DEFECTS = ("single_div", "ge", "first", "nolabel", "nomin", "late_weight")


def iou32(fb, b):
    """IoU of the fused boxes fb [k, 4] with the candidate box b [4]: float32, the operation order of dn_merge_detections (DN_MERGE_IOU)."""
    aa = (fb[:, 2] - fb[:, 0]) * (fb[:, 3] - fb[:, 1])
    ab = (b[2] - b[0]) * (b[3] - b[1])
    xx1 = np.where(fb[:, 0] > b[0], fb[:, 0], b[0])
    yy1 = np.where(fb[:, 1] > b[1], fb[:, 1], b[1])
    xx2 = np.where(fb[:, 2] < b[2], fb[:, 2], b[2])
    yy2 = np.where(fb[:, 3] < b[3], fb[:, 3], b[3])
    w = xx2 - xx1
    h = yy2 - yy1
    w = np.where(w < 0, f32(0), w)
    h = np.where(h < 0, f32(0), h)
    inter = w * h
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = inter / (aa + ab - inter)
    assert u.dtype == np.float32
    return u


def group_weight(weights, s0, s1):
    """1. W = the weights of the group's sources added in source order."""
    W = f32(0)
    for s in range(s0, s1):
        W = f32(W + weights[s])
    return W


def candidates(boxes, scores, labels, counts, offsets, weights, s0, s1, skip_thresh, late_weight=False):
    """2. + 3. -> the group's candidates in rank order: (flattened index, v, shifted box [4] f32, label)."""
    d = scores.shape[1]
    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(s0, s1):
            for j in range(min(int(counts[s]), d)):
                v = f32(scores[s, j] * weights[s])
                t = scores[s, j] if late_weight else v
                if np.isnan(v) or np.isnan(t) or not (t >= skip_thresh) or not (t > 0) or not (v > 0):
                    continue
                o = offsets[s]
                b = np.array([boxes[s, j, 0] + o[0], boxes[s, j, 1] + o[1], boxes[s, j, 2] + o[0], boxes[s, j, 3] + o[1]], f32)
                out.append((s * d + j, v, b, int(labels[s, j])))
    out.sort(key=lambda c: (-float(c[1]), c[0]))
    return out


def _prepare(boxes, scores, labels, counts, offsets, weights):
    boxes, scores, offsets = np.asarray(boxes, f32), np.asarray(scores, f32), np.asarray(offsets, f32)
    labels, counts = np.asarray(labels, np.int64), np.asarray(counts, np.int32)
    weights = np.ones(scores.shape[0], f32) if weights is None else np.asarray(weights, f32)
    return boxes, scores, labels, counts, offsets, weights


def _rank_key(score, c):
    """8. score descending, a NaN behind every number, ties by creation order."""
    return (1, 0.0, c) if np.isnan(score) else (0, -float(score), c)


def fuse(boxes, scores, labels, counts, offsets, group_begin, weights, thresh, skip_thresh, d_out, defect=None):
    """-> (boxes_out [G, d_out, 4] f32, scores_out [G, d_out] f32, labels_out [G, d_out] i64, counts_out [G] i32, members_out [G, d_out] i32,
    memberships): memberships[g] = the member lists (flattened indices, in the order they joined) of group g's clusters in OUTPUT order, all of
    them (not only the first d_out)."""
    assert defect is None or defect in DEFECTS, defect
    boxes, scores, labels, counts, offsets, weights = _prepare(boxes, scores, labels, counts, offsets, weights)
    G = len(group_begin) - 1
    thresh, skip_thresh = f32(thresh), f32(skip_thresh)
    ob, os_, ol = np.zeros((G, d_out, 4), f32), np.zeros((G, d_out), f32), np.zeros((G, d_out), np.int64)
    oc, om = np.zeros(G, np.int32), np.zeros((G, d_out), np.int32)
    memberships = []
    for g in range(G):
        s0, s1 = int(group_begin[g]), int(group_begin[g + 1])
        W = group_weight(weights, s0, s1)
        cand = candidates(boxes, scores, labels, counts, offsets, weights, s0, s1, skip_thresh, late_weight=defect == "late_weight")
        cap = max(len(cand), 1)
        fb, A, lab = np.zeros((cap, 4), f32), np.zeros((cap, 4), f32), np.zeros(cap, np.int64)
        Sv, T = np.zeros(cap, f32), np.zeros(cap, np.int32)
        mem = []
        nc = 0
        for idx, v, b, l in cand:                                # 4. the walk
            win = -1
            if nc:
                sel = np.arange(nc) if defect == "nolabel" else np.nonzero(lab[:nc] == l)[0]      # creation order
                if sel.size:
                    u = iou32(fb[sel], b)
                    ok = (u >= thresh) if defect == "ge" else (u > thresh)      # (a NaN u compares false)
                    if ok.any():
                        if defect == "first":
                            win = int(sel[np.nonzero(ok)[0][0]])
                        else:
                            win = int(sel[np.argmax(np.where(ok, u, f32(-1)))])   # the largest u; argmax returns the first on a tie
            if win < 0:                                          # 5. a new cluster
                T[nc], Sv[nc], lab[nc] = 1, v, l
                A[nc] = v * b
                fb[nc] = A[nc] / Sv[nc] if defect == "single_div" else b
                mem.append([idx])
                nc += 1
            else:                                                # 6. the candidate joins
                T[win] += 1
                Sv[win] = Sv[win] + v
                A[win] = A[win] + v * b
                fb[win] = A[win] / Sv[win]
                mem[win].append(idx)
        assert A.dtype == np.float32 and fb.dtype == np.float32 and Sv.dtype == np.float32
        sc = np.zeros(nc, f32)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            for c in range(nc):                                  # 7. the score
                t = f32(T[c])
                m = t if defect == "nomin" else (W if W < t else t)
                sc[c] = f32(f32(f32(Sv[c] / t) * m) / W)
        order = sorted(range(nc), key=lambda c: _rank_key(sc[c], c))      # 8.
        n = min(nc, d_out)
        for r, c in enumerate(order[:n]):
            ob[g, r], os_[g, r], ol[g, r], om[g, r] = fb[c], sc[c], lab[c], T[c]
        oc[g] = n
        memberships.append([mem[c] for c in order])
    return ob, os_, ol, oc, om, memberships


def iou64(a, b):
    iw = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    ih = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    inter = iw * ih
    den = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    return inter / den if den > 0 else 0.0


def fuse64(boxes, scores, labels, counts, offsets, group_begin, weights, thresh, skip_thresh):
    """The published algorithm in float64 on the candidates of `fuse` (v and the shifted boxes are inputs here: their float32 values, exactly).
    -> (per group: the clusters in output order as dicts(box [4] f64, score f64, label, members [flattened indices]), margin = the smallest
    |IoU - thresh| over every IoU the walk evaluated)."""
    boxes, scores, labels, counts, offsets, weights = _prepare(boxes, scores, labels, counts, offsets, weights)
    thresh = float(f32(thresh))
    margin = np.inf
    groups = []
    for g in range(len(group_begin) - 1):
        s0, s1 = int(group_begin[g]), int(group_begin[g + 1])
        W = float(np.sum(weights[s0:s1].astype(np.float64)))
        clusters = []
        for idx, v, b, l in candidates(boxes, scores, labels, counts, offsets, weights, s0, s1, f32(skip_thresh)):
            v, b = float(v), b.astype(np.float64)
            best, best_u = None, thresh
            for c in clusters:
                if c["label"] != l:
                    continue
                u = iou64(c["box"], b)
                margin = min(margin, abs(u - thresh))
                if u > best_u:
                    best, best_u = c, u
            if best is None:
                clusters.append(dict(label=l, members=[idx], v=[v], boxes=[b], box=b))
            else:
                best["members"].append(idx)
                best["v"].append(v)
                best["boxes"].append(b)
                vs = np.asarray(best["v"])
                best["box"] = (vs[:, None] * np.asarray(best["boxes"])).sum(0) / vs.sum()      # from the whole list, every time
        for c in clusters:
            t = len(c["members"])
            c["score"] = sum(c["v"]) / t * min(t, W) / W
        order = sorted(range(len(clusters)), key=lambda i: (-clusters[i]["score"], i))
        groups.append([clusters[i] for i in order])
    return groups, margin
