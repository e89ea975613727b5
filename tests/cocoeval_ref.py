"""pycocotools' COCOeval for bounding boxes (useCats = 1) restated in numpy, function for function as published: maskApi.c `bbIou`,
`computeIoU`, `evaluateImg`, `accumulate`, `summarize`. Per-(image, category) lists of dicts, the ground truths sorted by their ignore flag with
a stable sort, the `break` rule of the inner loop, `np.argsort(-score, kind='mergesort')` -- NOT the one-sweep, two-candidate, bit-flag form of
csrc/cocomatch.hip or the sorted-tensor form of demonet_amd/cocoeval.py. pycocotools itself is not installed where this project runs and the
reference project only imports it, so this arithmetic is UNPINNED third-party code (the standing of torchvision's NMS in DESIGN 2); what pins the
restatement is tests/test_cocoeval.py: closed forms worked out by hand and a cross-pin to the VOC matcher, which is held to the reference
project's own voc_eval vectors.

Images are evaluated in the order given (pycocotools: ascending image id); detection ids and ground-truth ids are 1-based, as loadRes makes them.
"""
import numpy as np

IOU_THRESHOLDS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)      # Params.setDetParams
RECALL_THRESHOLDS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RANGES = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
MAX_DETS = [1, 10, 100]


def bb_iou(dt, gt, iscrowd):
    """maskApi.c bbIou: dt [m][4], gt [n][4] as (x, y, w, h) doubles -> o [m][n]"""
    m, n = len(dt), len(gt)
    dt, gt = np.asarray(dt, np.float64).reshape(m, 4), np.asarray(gt, np.float64).reshape(n, 4)
    o = np.zeros((m, n), np.float64)
    for g in range(n):
        G = gt[g]
        ga = G[2] * G[3]
        crowd = bool(iscrowd[g])
        for d in range(m):
            D = dt[d]
            da = D[2] * D[3]
            o[d, g] = 0
            w = np.fmin(D[2] + D[0], G[2] + G[0]) - np.fmax(D[0], G[0])
            if w <= 0:
                continue
            h = np.fmin(D[3] + D[1], G[3] + G[1]) - np.fmax(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            u = da if crowd else da + ga - i
            o[d, g] = i / u
    return o


def compute_iou(gt, dt, max_det_last):
    if len(gt) == 0 and len(dt) == 0:
        return []
    inds = np.argsort([-d['score'] for d in dt], kind='mergesort')
    dt = [dt[i] for i in inds]
    if len(dt) > max_det_last:
        dt = dt[0:max_det_last]
    g = [g['bbox'] for g in gt]
    d = [d['bbox'] for d in dt]
    iscrowd = [int(o['iscrowd']) for o in gt]
    if len(d) == 0 or len(g) == 0:                          # maskUtils.iou of an empty list is an empty list
        return []
    return bb_iou(d, g, iscrowd)


def evaluate_img(gt, dt, ious, aRng, maxDet, iouThrs):
    """evaluateImg for one (image, category, area range). gt / dt: lists of dicts (gt: id, bbox, area, iscrowd, ignore; dt: id, bbox, area,
    score), in annotation order. Returns None or the dict of evaluateImg (the fields accumulate reads, and dtIds / gtIds)."""
    if len(gt) == 0 and len(dt) == 0:
        return None
    gt = [dict(g) for g in gt]
    for g in gt:
        if g['ignore'] or (g['area'] < aRng[0] or g['area'] > aRng[1]):
            g['_ignore'] = 1
        else:
            g['_ignore'] = 0
    # sort dt highest score first, sort gt ignore last
    gtind = np.argsort([g['_ignore'] for g in gt], kind='mergesort')
    gt = [gt[i] for i in gtind]
    dtind = np.argsort([-d['score'] for d in dt], kind='mergesort')
    dt = [dt[i] for i in dtind[0:maxDet]]
    iscrowd = [int(o['iscrowd']) for o in gt]
    ious = ious[:, gtind] if len(ious) > 0 else ious
    T, G, D = len(iouThrs), len(gt), len(dt)
    gtm = np.zeros((T, G))
    dtm = np.zeros((T, D))
    gtIg = np.array([g['_ignore'] for g in gt])
    dtIg = np.zeros((T, D))
    if not len(ious) == 0:
        for tind, t in enumerate(iouThrs):
            for dind, d in enumerate(dt):
                # information about best match so far (m=-1 -> unmatched)
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind, g in enumerate(gt):
                    # if this gt already matched, and not a crowd, continue
                    if gtm[tind, gind] > 0 and not iscrowd[gind]:
                        continue
                    # if dt matched to reg gt, and on ignore gt, stop
                    if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                        break
                    # continue to next gt unless better match made
                    if ious[dind, gind] < iou:
                        continue
                    # if match successful and best so far, store appropriately
                    iou = ious[dind, gind]
                    m = gind
                # if match made store id of match for both dt and gt
                if m == -1:
                    continue
                dtIg[tind, dind] = gtIg[m]
                dtm[tind, dind] = gt[m]['id']
                gtm[tind, m] = d['id']
    # set unmatched detections outside of area range to ignore
    a = np.array([d['area'] < aRng[0] or d['area'] > aRng[1] for d in dt]).reshape((1, len(dt)))
    dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
    return {'dtIds': [d['id'] for d in dt], 'gtIds': [g['id'] for g in gt], 'dtMatches': dtm, 'gtMatches': gtm,
            'dtScores': [d['score'] for d in dt], 'gtIgnore': gtIg, 'dtIgnore': dtIg}


def accumulate(evalImgs, K, I, iouThrs, recThrs, areaRng, maxDets):
    """evalImgs: the flat list of evaluate(), ordered [category][area range][image]"""
    T, R, A, M = len(iouThrs), len(recThrs), len(areaRng), len(maxDets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k in range(K):
        Nk = k * A * I
        for a in range(A):
            Na = a * I
            for m, maxDet in enumerate(maxDets):
                E = [evalImgs[Nk + Na + i] for i in range(I)]
                E = [e for e in E if e is not None]
                if len(E) == 0:
                    continue
                dtScores = np.concatenate([e['dtScores'][0:maxDet] for e in E])
                inds = np.argsort(-dtScores, kind='mergesort')
                dtScoresSorted = dtScores[inds]
                dtm = np.concatenate([e['dtMatches'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                dtIg = np.concatenate([e['dtIgnore'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                gtIg = np.concatenate([e['gtIgnore'] for e in E])
                npig = np.count_nonzero(gtIg == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dtIg))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp = np.array(tp)
                    fp = np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    if nd:
                        recall[t, k, a, m] = rc[-1]
                    else:
                        recall[t, k, a, m] = 0
                    pr = pr.tolist()
                    q = q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds2 = np.searchsorted(rc, recThrs, side='left')
                    try:
                        for ri, pi in enumerate(inds2):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
    return precision, recall


def summarize(precision, recall, iouThrs, areaRng, maxDets):
    """the twelve numbers of summarize()._summarizeDets; area ranges in the order all, small, medium, large"""
    iouThrs = np.asarray(iouThrs)

    def _summarize(ap=1, iouThr=None, aind=0, maxDets=100):
        mind = [i for i, mDet in enumerate(maxDetsList) if mDet == maxDets]
        if ap == 1:
            s = precision
            if iouThr is not None:
                t = np.where(iouThr == iouThrs)[0]
                s = s[t]
            s = s[:, :, :, [aind], mind]
        else:
            s = recall
            if iouThr is not None:
                t = np.where(iouThr == iouThrs)[0]
                s = s[t]
            s = s[:, :, [aind], mind]
        if len(s[s > -1]) == 0:
            return -1.0
        return float(np.mean(s[s > -1]))

    maxDetsList = list(maxDets)
    stats = [_summarize(1, maxDets=maxDetsList[2]), _summarize(1, iouThr=.5, maxDets=maxDetsList[2]), _summarize(1, iouThr=.75, maxDets=maxDetsList[2]),
             _summarize(1, aind=1, maxDets=maxDetsList[2]), _summarize(1, aind=2, maxDets=maxDetsList[2]), _summarize(1, aind=3, maxDets=maxDetsList[2]),
             _summarize(0, maxDets=maxDetsList[0]), _summarize(0, maxDets=maxDetsList[1]), _summarize(0, maxDets=maxDetsList[2]),
             _summarize(0, aind=1, maxDets=maxDetsList[2]), _summarize(0, aind=2, maxDets=maxDetsList[2]), _summarize(0, aind=3, maxDets=maxDetsList[2])]
    return stats


# ----------------------------------------------------------------------------------------------------------------------------------
# the data set around those functions: what COCO.loadRes / COCOeval._prepare build from records
# ----------------------------------------------------------------------------------------------------------------------------------
def _xywh(box):
    """xyxy fp32 -> [x, y, w, h] as Python floats with w, h subtracted in fp32: what engine.coco_records hands to pycocotools"""
    b = np.asarray(box, np.float32)
    return [float(b[0]), float(b[1]), float(np.float32(b[2] - b[0])), float(np.float32(b[3] - b[1]))]


def image_lists(det, gt, image_index):
    """One image's records -> ({label: [gt dicts]}, {label: [dt dicts]}), ids = slot + 1 (+ a per-image base so they are unique in a set).
    det: dict(boxes [c,4], scores [c], labels [c]); gt: dict(boxes [g,4], labels [g], optional iscrowd [g], optional area [g])."""
    gts, dts = {}, {}
    base = image_index * 100000
    for k in range(len(gt["labels"])):
        bbox = _xywh(gt["boxes"][k])
        crowd = int(gt["iscrowd"][k]) if gt.get("iscrowd") is not None else 0
        area = float(np.float32(gt["area"][k])) if gt.get("area") is not None else bbox[2] * bbox[3]
        gts.setdefault(int(gt["labels"][k]), []).append({'id': base + k + 1, 'slot': k, 'bbox': bbox, 'area': area, 'iscrowd': crowd, 'ignore': crowd})
    for j in range(len(det["scores"])):
        bbox = _xywh(det["boxes"][j])
        dts.setdefault(int(det["labels"][j]), []).append({'id': base + j + 1, 'slot': j, 'bbox': bbox, 'area': bbox[2] * bbox[3],
                                                          'score': float(det["scores"][j])})
    return gts, dts


def coco_eval(dets, gts, num_classes, iouThrs=IOU_THRESHOLDS, recThrs=RECALL_THRESHOLDS, areaRng=AREA_RANGES, maxDets=MAX_DETS):
    """COCOeval.evaluate + accumulate + summarize over lists of per-image records (see image_lists), categories = labels 0 .. num_classes - 1
    -> dict(stats [12], precision [T,101,K,A,M], recall [T,K,A,M])"""
    I = len(dets)
    lists = [image_lists(d, g, i) for i, (d, g) in enumerate(zip(dets, gts))]
    maxDet = maxDets[-1]
    ious = {(i, k): compute_iou(lists[i][0].get(k, []), lists[i][1].get(k, []), maxDet) for i in range(I) for k in range(num_classes)}
    evalImgs = [evaluate_img(lists[i][0].get(k, []), lists[i][1].get(k, []), ious[i, k], aRng, maxDet, iouThrs)
                for k in range(num_classes) for aRng in areaRng for i in range(I)]
    precision, recall = accumulate(evalImgs, num_classes, I, iouThrs, recThrs, areaRng, maxDets)
    return dict(stats=summarize(precision, recall, iouThrs, areaRng, maxDets), precision=precision, recall=recall)


def match_ref(boxes, scores, labels, counts, gt_boxes, gt_labels, gt_counts, gt_crowd, gt_area, thresholds, area_ranges, max_det, num_classes=0):
    """dn_coco_match's outputs from evaluate_img: padded arrays as the entry point takes them (gt_crowd / gt_area may be None) ->
    (flags [n,d,R] uint32, rank [n,d] int32, match_gt [n,d,R,T] int32, gt_stats [num_classes,R] int64). Counts are clamped to the arrays."""
    n, d = scores.shape
    gmax = gt_labels.shape[1]
    T, R = len(thresholds), len(area_ranges)
    flags = np.zeros((n, d, R), np.uint32)
    rank = np.full((n, d), -1, np.int32)
    match_gt = np.full((n, d, R, T), -1, np.int32)
    stats = np.zeros((max(int(num_classes), 0), R), np.int64)
    for i in range(n):
        c, g = min(max(int(counts[i]), 0), d), min(max(int(gt_counts[i]), 0), gmax)
        det = dict(boxes=boxes[i, :c], scores=scores[i, :c], labels=labels[i, :c])
        gt = dict(boxes=gt_boxes[i, :g], labels=gt_labels[i, :g], iscrowd=None if gt_crowd is None else (gt_crowd[i, :g] != 0),
                  area=None if gt_area is None else gt_area[i, :g])
        gts, dts = image_lists(det, gt, 0)
        for lb, glist in gts.items():
            for r, aRng in enumerate(area_ranges):
                e = evaluate_img(glist, [], [], aRng, max_det, thresholds)
                if 0 <= lb < num_classes:
                    stats[lb, r] += int(np.count_nonzero(e['gtIgnore'] == 0))
        for lb, dlist in dts.items():
            glist = gts.get(lb, [])
            order = np.argsort([-x['score'] for x in dlist], kind='mergesort')
            for q, at in enumerate(order):
                rank[i, dlist[at]['slot']] = q
            ious = compute_iou(glist, dlist, max_det)
            for r, aRng in enumerate(area_ranges):
                e = evaluate_img(glist, dlist, ious, aRng, max_det, thresholds)
                for q, did in enumerate(e['dtIds']):
                    j = did - 1
                    for b in range(T):
                        if e['dtMatches'][b, q]:
                            flags[i, j, r] |= np.uint32(1 << b)
                            match_gt[i, j, r, b] = int(e['dtMatches'][b, q]) - 1
                        if e['dtIgnore'][b, q]:
                            flags[i, j, r] |= np.uint32(1 << (16 + b))
    return flags, rank, match_gt, stats


def pad_records(dets, d):
    """[{boxes [k,4], scores [k], labels [k]}, ...] -> padded (boxes [n,d,4] f32, scores [n,d] f32, labels [n,d] i64, counts [n] i32)"""
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
    """[{boxes [k,4], labels [k], optional iscrowd [k], optional area [k]}, ...] -> (gt_boxes [n,gmax,4] f32, gt_labels [n,gmax] i64, gt_counts [n]
    i32, gt_crowd [n,gmax] u8, gt_area [n,gmax] f32); a missing area is fp32(w) * fp32(h) rounded to fp32"""
    n = len(gts)
    gmax = gmax or max(1, max(len(g["labels"]) for g in gts))
    boxes, labels = np.zeros((n, gmax, 4), np.float32), np.zeros((n, gmax), np.int64)
    crowd, area = np.zeros((n, gmax), np.uint8), np.zeros((n, gmax), np.float32)
    counts = np.zeros(n, np.int32)
    for i, g in enumerate(gts):
        k = len(g["labels"])
        counts[i] = k
        boxes[i, :k], labels[i, :k] = np.asarray(g["boxes"]).reshape(-1, 4), np.asarray(g["labels"])
        if g.get("iscrowd") is not None:
            crowd[i, :k] = np.asarray(g["iscrowd"]).astype(np.uint8)
        if g.get("area") is not None:
            area[i, :k] = np.asarray(g["area"], np.float32)
        else:
            area[i, :k] = (boxes[i, :k, 2] - boxes[i, :k, 0]) * (boxes[i, :k, 3] - boxes[i, :k, 1])
    return boxes, labels, counts, crowd, area


def records_of(padded_det, padded_gt, with_area=True):
    """the padded arrays back as per-image record lists for coco_eval"""
    boxes, scores, labels, counts = padded_det
    gb, gl, gc, gcrowd, garea = padded_gt
    dets = [dict(boxes=boxes[i, :counts[i]], scores=scores[i, :counts[i]], labels=labels[i, :counts[i]]) for i in range(len(counts))]
    gts = [dict(boxes=gb[i, :gc[i]], labels=gl[i, :gc[i]], iscrowd=gcrowd[i, :gc[i]], area=garea[i, :gc[i]] if with_area else None) for i in range(len(gc))]
    return dets, gts
