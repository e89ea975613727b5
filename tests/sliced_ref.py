"""TEST INFRASTRUCTURE: the reference of the sliced-inference pieces (demonet_amd/sliced.py, csrc/sliced.hip), numpy float32.

`merge_ref` follows the five sentences of include/demonet_hip.h (dn_merge_detections) literally, as a Python loop over the candidates in rank order;
only the comparison of one candidate with the list of kept ones is a numpy expression -- elementwise float32, so every value is what the scalar
formula of oracle/nms_c.c gives. It also returns the smallest |m - thresh| over all pairs it compared: an input whose margin is > 0 has no pair on
the threshold, and a correct implementation must then agree with it exactly. tests/test_sliced.py pins it to the project's oracle NMS.
"""
import numpy as np

IOU, IOS = 0, 1
f32 = np.float32


def axis_ref(extent, tile, overlap):
    stride = max(1, tile - int(round(overlap * tile)))
    xs = [k * stride for k in range(extent) if k * stride + tile < extent]
    return xs + [extent - tile], stride


def tile_grid_ref(H, W, th, tw, overlap):
    if not (0.0 <= overlap < 1.0):
        raise ValueError("overlap")
    th, tw = min(th, H), min(tw, W)
    xs, _ = axis_ref(W, tw, overlap)
    ys, _ = axis_ref(H, th, overlap)
    return [(x, y) for y in ys for x in xs], th, tw


def overlaps(kb, ka, b, a, metric):
    """m of the kept boxes kb [k, 4] (areas ka) with the candidate b (area a): float32, the operation order of oracle/nms_c.c."""
    xx1 = np.where(kb[:, 0] > b[0], kb[:, 0], b[0])
    yy1 = np.where(kb[:, 1] > b[1], kb[:, 1], b[1])
    xx2 = np.where(kb[:, 2] < b[2], kb[:, 2], b[2])
    yy2 = np.where(kb[:, 3] < b[3], kb[:, 3], b[3])
    w = xx2 - xx1
    h = yy2 - yy1
    w = np.where(w < 0, f32(0), w)
    h = np.where(h < 0, f32(0), h)
    inter = w * h
    with np.errstate(divide="ignore", invalid="ignore"):
        if metric == IOS:
            m = inter / np.where(ka < a, ka, a)
        else:
            m = inter / (ka + a - inter)
    assert m.dtype == np.float32
    return m


def merge_ref(boxes, scores, labels, counts, offsets, group_begin, metric, thresh, class_agnostic, d_out):
    """-> (boxes_out [G, d_out, 4] f32, scores_out [G, d_out] f32, labels_out [G, d_out] i64, counts_out [G] i32, src_out [G, d_out] i32, margin)."""
    boxes, scores, offsets = np.asarray(boxes, f32), np.asarray(scores, f32), np.asarray(offsets, f32)
    labels, counts = np.asarray(labels, np.int64), np.asarray(counts, np.int32)
    S, d = scores.shape
    G = len(group_begin) - 1
    thresh = f32(thresh)
    ob, os_, ol = np.zeros((G, d_out, 4), f32), np.zeros((G, d_out), f32), np.zeros((G, d_out), np.int64)
    oc, src = np.zeros(G, np.int32), np.full((G, d_out), -1, np.int32)
    margin = np.inf
    for g in range(G):
        # 1. candidates  2. shifted boxes
        cand = [(s, j) for s in range(group_begin[g], group_begin[g + 1]) for j in range(min(int(counts[s]), d)) if not np.isnan(scores[s, j])]
        # 3. rank: score descending, ties by ascending flattened index
        cand.sort(key=lambda sj: (-float(scores[sj]), sj[0] * d + sj[1]))
        kb, ka, kl = np.zeros((d_out, 4), f32), np.zeros(d_out, f32), np.zeros(d_out, np.int64)
        nk = 0
        for s, j in cand:                                       # 4. the walk
            off = offsets[s]
            b = np.array([boxes[s, j, 0] + off[0], boxes[s, j, 1] + off[1], boxes[s, j, 2] + off[0], boxes[s, j, 3] + off[1]], f32)
            a = (b[2] - b[0]) * (b[3] - b[1])
            keep = True
            if nk:
                sel = slice(0, nk) if class_agnostic else np.nonzero(kl[:nk] == labels[s, j])[0]
                m = overlaps(kb[sel], ka[sel], b, a, metric)
                ok = ~np.isnan(m)
                if ok.any():
                    margin = min(margin, float(np.abs(m[ok].astype(np.float64) - np.float64(thresh)).min()))
                keep = not bool((m > thresh).any())             # (a NaN m compares false: it does not suppress)
            if keep:
                kb[nk], ka[nk], kl[nk] = b, a, labels[s, j]
                ob[g, nk], os_[g, nk], ol[g, nk], src[g, nk] = b, scores[s, j], labels[s, j], s * d + j
                nk += 1
                if nk == d_out:                                 # 5. the first d_out kept ones; the walk may stop there
                    break
        oc[g] = nk
    return ob, os_, ol, oc, src, margin
