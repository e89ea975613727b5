"""Numpy oracle and verifier of the soft-NMS post-process (include/demonet_hip.h: DN_NMS_SOFT_LINEAR / DN_NMS_SOFT_GAUSSIAN).

Semantics, per image and foreground class, on the reference's softmax scores s and decoded, clipped boxes b
(oracle/ssd_oracle.postprocess_detections(..., return_intermediates=True)):
  1. candidates: s > score_thresh (strict), the topk_candidates best by (score desc, anchor asc);
  2. while candidates remain: pick the one with the largest CURRENT score (ties: lower anchor), emit (anchor, current score), multiply
     the score of every remaining j by f(u), u = IoU(picked, j) in fp32 = inter / ((a_i + a_j) - inter), 0 when the union is 0:
         linear   f = u > nms_thresh ? 1 - u : 1          gaussian   f = exp(-(u * u) / sigma)
     and drop every remaining j whose score is now <= score_thresh;
  3. the emitted lists of all classes -> global top detections_per_img by (score desc, label asc, emission order).

The oracle carries the scores in float64 (on the fp32 IoU) and, per candidate, a bound B on the relative error of an fp32
implementation: the sum over its non-unit factors of eps(u),
    linear    eps = 2 * 2^-24                    (1 - u and the product: one rounding each)
    gaussian  eps = (3 + 2 u^2 / sigma) * 2^-24  (u * u, the division and the product: one rounding each; expf within 1 ulp; the
                                                  argument's error of 2 roundings amplified by |argument| = u^2 / sigma).
Near-tied decayed scores make the oracle's own ORDER ambiguous, so verify_image does not compare orders: it replays the
implementation's output, in its emission order, in float64, and checks every decision against those bounds.
"""
import numpy as np

U = 2.0 ** -24          # half an ulp of fp32, relative
SLACK = 2.0 ** -23      # one more rounding each way (the stored fp32 score against its float64 twin)
METHODS = ("linear", "gaussian")


def candidates(softmax: np.ndarray, score_thresh: float, topk: int):
    """Per foreground class: (anchor indices, fp32 scores), sorted by (score desc, anchor asc). softmax: [A, K] float32."""
    thr = np.float32(score_thresh)
    out = []
    for label in range(1, softmax.shape[1]):
        sc = softmax[:, label]
        idx = np.nonzero(sc > thr)[0]
        order = np.argsort(-sc[idx], kind="stable")[:min(topk, idx.size)]
        out.append((idx[order].astype(np.int64), sc[idx[order]].astype(np.float32)))
    return out


def iou_row(box: np.ndarray, area: np.float32, boxes: np.ndarray, areas: np.ndarray) -> np.ndarray:
    """fp32 IoU of one box against many, in the implementation's op order; 0 where the union is 0."""
    f = np.float32
    iw = np.maximum(f(0), np.minimum(box[2], boxes[:, 2]) - np.maximum(box[0], boxes[:, 0]))
    ih = np.maximum(f(0), np.minimum(box[3], boxes[:, 3]) - np.maximum(box[1], boxes[:, 1]))
    inter = (iw * ih).astype(f)
    uni = ((area + areas).astype(f) - inter).astype(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (inter / uni).astype(f)
    return np.where(uni == 0, f(0), u).astype(f)


def areas_of(boxes: np.ndarray) -> np.ndarray:
    return ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])).astype(np.float32)


def factor(u: np.ndarray, method: str, nms_thresh: float, sigma: float, dtype):
    """(f, eps, nonunit) for fp32 IoUs u; f in `dtype` (float64: the oracle; float32: the restatement of the kernel's arithmetic)."""
    sg = np.float32(sigma)
    if method == "linear":
        non = u > np.float32(nms_thresh)
        f = np.where(non, dtype(1) - u.astype(dtype), dtype(1)).astype(dtype)
        eps = np.where(non, 2 * U, 0.0)
    elif method == "gaussian":
        non = u > 0
        if dtype is np.float32:
            f = np.exp((-(u * u).astype(np.float32) / sg).astype(np.float32)).astype(np.float32)
        else:
            f = np.exp(-(u.astype(np.float64) ** 2) / np.float64(sg))
        eps = np.where(non, (3 + 2 * u.astype(np.float64) ** 2 / np.float64(sg)) * U, 0.0)
    else:
        raise ValueError(method)
    return f, eps, non


def soft_nms_class(anchors, scores, boxes, method, nms_thresh, sigma, score_thresh, dtype=np.float64):
    """The algorithm on one class. anchors / scores: candidates(); boxes: [A, 4] fp32 decoded boxes.
    Returns dict(anchors, scores (dtype), B: per emitted candidate; min_gap: the smallest relative margin of any decision (argmax
    or drop) that fp32 rounding could turn, exact ties of untouched scores excluded (both sides resolve them by anchor); max_B)."""
    thr = dtype(np.float32(score_thresh))
    cb = boxes[anchors]
    ca = areas_of(cb)
    s = scores.astype(dtype)
    B = np.zeros(len(anchors))
    alive = np.ones(len(anchors), dtype=bool)
    out_a, out_s, out_B = [], [], []
    min_gap, max_B = np.inf, 0.0
    while alive.any():
        live = np.nonzero(alive)[0]
        top = s[live].max()
        ties = live[s[live] == top]
        i = ties[np.argmin(anchors[ties])]
        others = live[live != i]
        if others.size:
            exact = (s[others] == top) & (B[others] == 0) & (B[i] == 0)
            rest = others[~exact]
            if rest.size:
                min_gap = min(min_gap, float((top - s[rest].max()) / top))
        out_a.append(int(anchors[i])); out_s.append(s[i]); out_B.append(B[i])
        max_B = max(max_B, float(B[i]))
        alive[i] = False
        if others.size:
            u = iou_row(cb[i], ca[i], cb[others], ca[others])
            f, eps, non = factor(u, method, nms_thresh, sigma, dtype)
            s[others] = (s[others] * f).astype(dtype)
            B[others] += eps
            drop = s[others] <= thr
            if thr > 0:
                touched = others[non]
                if touched.size:
                    min_gap = min(min_gap, float(np.abs(s[touched].astype(np.float64) - float(thr)).min() / float(thr)))
            max_B = max(max_B, float(B[others].max()))
            alive[others[drop]] = False
    return dict(anchors=np.asarray(out_a, dtype=np.int64), scores=np.asarray(out_s, dtype=dtype), B=np.asarray(out_B), min_gap=min_gap, max_B=max_B)


def merge(per_class, boxes, dets):
    """Global top `dets` of the per-class emitted lists by (score desc, label asc, emission order), in the output form of
    dn_postprocess: (boxes [dets,4] f32, scores [dets] f32, labels [dets] i64, count, kept_anchor [dets] i32; rows >= count zero, anchor -1).
    Also returns the smallest relative gap between neighbours of different labels around and inside the cut (order ambiguity of the merge)."""
    rows = []
    for c, r in enumerate(per_class):
        for e, (a, sc, b) in enumerate(zip(r["anchors"], r["scores"], r["B"])):
            rows.append((-float(sc), c + 1, e, int(a), float(b)))
    rows.sort()
    gap = np.inf
    for k in range(min(len(rows) - 1, dets)):
        p, q = rows[k], rows[k + 1]
        if p[1] != q[1] and not (p[0] == q[0] and p[4] == 0 and q[4] == 0):
            gap = min(gap, (q[0] - p[0]) / -p[0])
    rows = rows[:dets]
    cnt = len(rows)
    ob = np.zeros((dets, 4), np.float32); os_ = np.zeros(dets, np.float32); ol = np.zeros(dets, np.int64); ok = np.full(dets, -1, np.int32)
    for k, (ns, lab, _, a, _) in enumerate(rows):
        ob[k] = boxes[a]; os_[k] = np.float32(-ns); ol[k] = lab; ok[k] = a
    return (ob, os_, ol, cnt, ok), gap


def soft_nms_image(softmax, decoded, method, nms_thresh, sigma, score_thresh, topk, dets, dtype=np.float64):
    """The whole post-process of one image behind softmax / decode. Returns (output tuple as merge(), info) with
    info = dict(min_gap, max_B) over all classes and the merge."""
    per_class = [soft_nms_class(a, s, decoded, method, nms_thresh, sigma, score_thresh, dtype) for a, s in candidates(softmax, score_thresh, topk)]
    out, mgap = merge(per_class, decoded, dets)
    info = dict(min_gap=min([mgap] + [r["min_gap"] for r in per_class]), max_B=max([0.0] + [r["max_B"] for r in per_class]))
    return out, info


def order_is_unambiguous(info) -> bool:
    """No decision of the oracle lies within reach of fp32 rounding: an implementation's anchor sequence must then equal the oracle's."""
    return info["min_gap"] > 2 * (info["max_B"] + SLACK)


def verify_image(out, softmax, decoded, method, nms_thresh, sigma, score_thresh, topk, dets):
    """Replays one image's output (boxes, scores, labels, count, kept_anchor) in float64, class by class in its own emission order.
    AssertionError on the first violated property; returns dict(pick=, score=): the worst ratios of (a) and (b), <= 1 by the checks.
      (a) every pick is a valid argmax:   s_i (1 + B_i + 2^-23) >= s_j (1 - B_j - 2^-23) for all remaining j
      (b) scores:                         |score - s_i| <= s_i (B_i + 2^-23)
      (c) drops:                          a candidate never emitted ends with s <= score_thresh (1 + B); none emitted has s < score_thresh (1 - B)
      (d) the cut (count == dets):        each class's list is a prefix, and nothing left could be emitted above the last output's score (1 + B + 2^-23)
      (e) form:                           labels in range, anchors are candidates of their class, boxes exact, scores non-increasing, rows >= count zero."""
    boxes, scores, labels, count, kept = out
    cnt = int(count)
    K = softmax.shape[1]
    thr = float(np.float32(score_thresh))
    assert 0 <= cnt <= dets
    assert (boxes[cnt:] == 0).all() and (scores[cnt:] == 0).all() and (labels[cnt:] == 0).all(), "rows >= count must be zero"
    assert ((labels[:cnt] >= 1) & (labels[:cnt] < K)).all(), "label out of range"
    assert (np.diff(scores[:cnt]) <= 0).all(), "scores must be non-increasing"
    assert ((kept[:cnt] >= 0) & (kept[:cnt] < softmax.shape[0])).all(), "anchor out of range"
    assert np.array_equal(boxes[:cnt], decoded[kept[:cnt]]), "boxes must be the decoded boxes of the kept anchors, exactly"
    truncated = cnt == dets
    last = float(scores[cnt - 1]) if cnt else 0.0
    worst_pick, worst_score = 0.0, 0.0
    for c, (anchors, sc) in enumerate(candidates(softmax, score_thresh, topk)):
        rows = np.nonzero(labels[:cnt] == c + 1)[0]
        where = {int(a): k for k, a in enumerate(anchors)}
        cb = decoded[anchors]
        ca = areas_of(cb)
        s = sc.astype(np.float64)
        B = np.zeros(len(anchors))
        alive = np.ones(len(anchors), dtype=bool)
        for r in rows:
            a, g = int(kept[r]), float(scores[r])
            assert a in where, "class %d: anchor %d is not a candidate" % (c + 1, a)
            i = where[a]
            assert alive[i], "class %d: anchor %d emitted twice or after it was certainly dropped (s = %g)" % (c + 1, a, s[i])
            others = np.nonzero(alive)[0]
            others = others[others != i]
            lhs = s[i] * (1 + B[i] + SLACK)
            if others.size:
                rhs = (s[others] * (1 - B[others] - SLACK)).max()
                worst_pick = max(worst_pick, rhs / lhs)
                assert lhs >= rhs, "class %d: anchor %d (s = %.9g, B = %.3g) emitted while %.9g remains" % (c + 1, a, s[i], B[i], s[others].max())
            bound = s[i] * (B[i] + SLACK)
            worst_score = max(worst_score, abs(g - s[i]) / bound)
            assert abs(g - s[i]) <= bound, "class %d anchor %d: score %.9g, replay %.9g, bound %.3g" % (c + 1, a, g, s[i], bound)
            assert s[i] >= thr * (1 - B[i]), "class %d: anchor %d emitted below the score threshold (%.9g)" % (c + 1, a, s[i])
            alive[i] = False
            if others.size:
                u = iou_row(cb[i], ca[i], cb[others], ca[others])
                f, eps, _ = factor(u, method, nms_thresh, sigma, np.float64)
                s[others] *= f
                B[others] += eps
                alive[others[s[others] <= thr * (1 - B[others])]] = False      # certainly dropped; the ambiguous ones stay: they may be emitted or not
        left = np.nonzero(alive)[0]
        if truncated:
            if left.size:
                over = s[left] / (last * (1 + B[left] + SLACK))
                assert (over <= 1).all(), "class %d: %.9g left behind the cut at %.9g" % (c + 1, s[left].max(), last)
        else:
            assert (s[left] <= thr * (1 + B[left])).all(), "class %d: a candidate with s = %.9g > score_thresh was never emitted" % (c + 1, s[left].max() if left.size else 0)
    return dict(pick=worst_pick, score=worst_score)
