"""The Python copy of the post-process workspace layout (csrc/postprocess.hip post_buffers), an exact verifier of the hard-NMS selection that
starts from the device's own scores and boxes, a predictor of the regime a given input drives the kernels into (which capacity bucket, which
cut-off, fallback or not, deep chain or not, which merge branch), and the construction of designed inputs (target scores -> logits, integer
boxes). No GPU in here and no torch of its own (the oracle it calls imports torch): everything works on numpy arrays read back by the caller.

Why the verifier is exact: from the fp32 scores and the decoded boxes on, the selection is integer work on score bits plus the fp32 IoU
inter / ((a_i + a_j) - inter) > nms_thresh, which numpy evaluates in the same operation order (the kernels are built without contraction). So
labels, anchors, counts and score bits of every image are compared for equality -- there is no near-tie that has to be excused."""
import os
import re

import numpy as np

import ssd_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "demonet_amd", "csrc")

# mirrors of the kernels' constants (held to the source text by tests/test_post_select.py::test_mirrors_follow_the_source_text)
HSHIFT = 19               # common.h DN_PP_HSHIFT
HBINS = 256               # common.h DN_PP_HBINS
MERGE_LCAP = 3072         # postprocess.hip: survivors the merge keeps in LDS
FIXED_POINT_ROUNDS = 6    # postprocess.hip nms_serial_phase: rounds before the sequential walk
FAST_CAP_MAX = 2048       # postprocess.hip select_nms_fast_kernel: CAP = min(64 NW^2, 2048)
WANT_DEFAULT = 4          # postprocess.hip DN_PP_WANT
OFF_LOGIT = -200.0        # a foreground logit whose softmax is exactly 0.0 (expf underflows below -103.3) on the device and in torch


def nw_bucket(topk):
    """choice.h post_nw_bucket"""
    w = (topk + 63) // 64
    return w if w <= 2 else 4 if w <= 4 else 5 if w <= 5 else 8


def fast_cap(nw):
    return min(64 * nw * nw, FAST_CAP_MAX)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def hist_range(score_thresh):
    """postprocess.hip post_hist_range -> (hb0, nb, clamped)"""
    t = np.float32(score_thresh if score_thresh > 0 else 0.0)
    top = int(bits(np.float32(1.0))) >> HSHIFT
    hb_thr = int(bits(t)) >> HSHIFT
    hb0 = max(hb_thr, top + 1 - HBINS)
    return hb0, top + 1 - hb0, int(hb_thr < hb0)


# ------------------------------------------------------------------------------------------------------------------------------------
# the workspace
# ------------------------------------------------------------------------------------------------------------------------------------
def _align256(x):
    return (x + 255) // 256 * 256


def workspace_layout(n, A, K, topk):
    """Byte offsets of post_buffers(ws, n, A, K, topk)."""
    km1 = K - 1
    off, p = {}, 0
    for name, size in (("scoresT", n * km1 * A * 4), ("boxes", n * A * 16), ("keptScore", n * km1 * topk * 4), ("keptAnchor", n * km1 * topk * 4),
                       ("keptCount", n * km1 * 4)):
        off[name] = p
        p += _align256(size)
    off["phist"] = p
    off["tauKey"] = p + n * ((A + 63) // 64) * HBINS * 4
    off["needFull"] = off["tauKey"] + n * 4
    off["order"] = off["needFull"] + n * 4
    return off


def read_workspace(buf, n, A, K, topk):
    """buf: the workspace after dn_postprocess as a numpy uint8 array. Returns what the selection worked on and left behind:
    inter [(softmax [A, K] with an unused background column, boxes [A, 4])] per image (the oracle's form), tauKey [n], needFull [n],
    keptCount [n, K-1]. tauKey / needFull are written on the cut-off path (DN_PP_FAST=1, hard NMS) only."""
    off, km1 = workspace_layout(n, A, K, topk), K - 1
    view = lambda name, count, dt: buf[off[name]:off[name] + 4 * count].view(dt)
    sc = view("scoresT", n * km1 * A, np.float32).reshape(n, km1, A)
    bx = view("boxes", n * A * 4, np.float32).reshape(n, A, 4)
    inter = [(np.ascontiguousarray(np.concatenate([np.zeros((A, 1), np.float32), sc[i].T], 1)), bx[i].copy()) for i in range(n)]
    return dict(inter=inter, tauKey=view("tauKey", n, np.uint32).copy(), needFull=view("needFull", n, np.int32).copy(),
                keptCount=view("keptCount", n * km1, np.int32).reshape(n, km1).copy())


# ------------------------------------------------------------------------------------------------------------------------------------
# the verifier
# ------------------------------------------------------------------------------------------------------------------------------------
def expected_image(sm, dec, score_thresh, nms_thresh, topk, dets, scale=(1.0, 1.0)):
    """The oracle's selection on given scores [A, K] and boxes [A, 4]: (boxes [D, 4], scores [D], labels [D], count, anchors [D]), padded as
    the merge pads (zeros, anchor -1)."""
    a_idx, labels, cs = so.select_candidates(sm, score_thresh, topk)
    cb = dec[a_idx]
    keep = so.batched_nms(cb, cs, labels, nms_thresh)[:dets]
    c = int(keep.size)
    sx, sy = np.float32(scale[0]), np.float32(scale[1])
    boxes = np.zeros((dets, 4), np.float32)
    scores = np.zeros(dets, np.float32)
    lab = np.zeros(dets, np.int64)
    anc = np.full(dets, -1, np.int32)
    if c:
        boxes[:c] = cb[keep].astype(np.float32) * np.array([sx, sy, sx, sy], np.float32)
        scores[:c] = cs[keep]
        lab[:c] = labels[keep]
        anc[:c] = a_idx[keep]
    return boxes, scores, lab, c, anc


def verify_image(out, sm, dec, score_thresh, nms_thresh, topk, dets, scale=(1.0, 1.0)):
    """out = (boxes [D, 4], scores [D], labels [D], count, kept anchors [D]) of one image must BE the oracle's selection on (sm, dec)."""
    b, s, l, cnt, k = out
    eb, es, el, ec, ek = expected_image(sm, dec, score_thresh, nms_thresh, topk, dets, scale)
    assert int(cnt) == ec, "count %d, expected %d" % (int(cnt), ec)
    assert np.array_equal(np.asarray(l), el), "labels differ at rows %s" % np.nonzero(np.asarray(l) != el)[0][:8]
    assert np.array_equal(np.asarray(k), ek), "anchors differ at rows %s" % np.nonzero(np.asarray(k) != ek)[0][:8]
    assert np.array_equal(bits(s), bits(es)), "scores are not the bits of scoresT at rows %s" % np.nonzero(bits(s) != bits(es))[0][:8]
    assert np.array_equal(bits(b), bits(eb)), "boxes are not the device boxes times scale_xy at rows %s" % np.nonzero((bits(b) != bits(eb)).any(1))[0][:8]
    return ec


def iou_band_gap(sm, dec, score_thresh, nms_thresh, topk):
    """min |IoU - nms_thresh| over the same-class candidate pairs (inf: none). Below 1e-6 the division's last bit could decide."""
    gap = np.inf
    a_idx, labels, _ = so.select_candidates(sm, score_thresh, topk)
    for c in np.unique(labels):
        sel = a_idx[labels == c]
        if sel.size >= 2:
            iou = so.box_iou_np(dec[sel], dec[sel])[np.triu_indices(sel.size, 1)]
            d = np.abs(iou - np.float32(nms_thresh))
            d = d[np.isfinite(d)]
            if d.size:
                gap = min(gap, float(d.min()))
    return gap


# ------------------------------------------------------------------------------------------------------------------------------------
# the regime predictor: a restatement of the kernels' control decisions (not of their arithmetic)
# ------------------------------------------------------------------------------------------------------------------------------------
def tau_key(sm, score_thresh, want):
    """tau_body: the cut-off key of an image."""
    s = sm[:, 1:]
    hb0, nb, clamped = hist_range(score_thresh)
    passing = s[s > np.float32(score_thresh)]
    hist = np.bincount(np.clip((bits(passing) >> HSHIFT).astype(np.int64) - hb0, 0, nb - 1), minlength=nb)
    if hist.sum() < want:
        return 0
    above = 0
    for b in range(nb - 1, -1, -1):
        if above + hist[b] >= want:
            return 0 if (clamped and b == 0) else (hb0 + b) << HSHIFT
        above += int(hist[b])
    raise AssertionError("unreachable")


def radix_select(keys, need, whole_shortcut):
    """The 4 x 8-bit radix select of select_candidates / merge_body on uint32 keys (len(keys) > need): (T, quota, shift at which merge_body's
    `whole` shortcut fired or None)."""
    keys = np.asarray(keys, np.uint32).astype(np.int64)
    prefix = 0
    for shift in (24, 16, 8, 0):
        sel = keys if shift == 24 else keys[(keys >> (shift + 8)) == (prefix >> (shift + 8))]
        hist = np.bincount((sel >> shift) & 255, minlength=256)
        acc = 0
        for d in range(255, -1, -1):
            if acc + hist[d] >= need:
                break
            acc += int(hist[d])
        prefix |= d << shift
        need, size = need - acc, int(hist[d])
        if whole_shortcut and need == size and shift > 0:
            return prefix - 1, 0, shift
    return prefix, need, None


def serial_phase(mask):
    """nms_serial_phase on a strictly upper triangular bool matrix mask[i, j] (i suppresses j): (kept [M] bool, [chunk took the walk])."""
    M = mask.shape[0]
    removed = np.zeros(M, bool)
    kept = np.zeros(M, bool)
    walks = []
    for c0 in range(0, M, 64):
        c1 = min(M, c0 + 64)
        ext, sub = removed[c0:c1].copy(), mask[c0:c1, c0:c1]
        cur, settled = ext.copy(), False
        for _ in range(FIXED_POINT_ROUNDS):
            new = ext | sub[~cur].any(0)
            if np.array_equal(new, cur):
                settled = True
                break
            cur = new
        if not settled:
            cur = ext.copy()
            for l in range(c1 - c0):
                if not cur[l]:
                    cur |= sub[l]
        walks.append(not settled)
        kept[c0:c1] = ~cur
        if c1 < M:
            removed[c1:] |= mask[c0:c1][~cur][:, c1:].any(0)
    return kept, walks


def _class_pass(s, key, dec, take, topk, nms_thresh):
    """One class on one path: candidates `take` (bool [A]) -> dict(M, kept, walk, ties at the cut key, kept score bits in emission order)."""
    idx = np.nonzero(take)[0]
    order = idx[np.argsort(-s[idx], kind="stable")]
    ties = 0
    if order.size > topk:
        T = key[order[topk - 1]]
        ties = int((key[idx] == T).sum())
    sel = order[:topk]
    M = int(sel.size)
    if M == 0:
        return dict(M=0, kept=0, walk=False, ties=ties, keys=np.zeros(0, np.uint32))
    with np.errstate(divide="ignore", invalid="ignore"):
        mask = np.triu(so.box_iou_np(dec[sel], dec[sel]) > np.float32(nms_thresh), 1)
    kept, walks = serial_phase(mask)
    ref = so.nms_single_class(dec[sel], s[sel], nms_thresh)
    assert np.array_equal(np.nonzero(kept)[0], np.sort(ref)), "the restated serial phase disagrees with the oracle's greedy NMS"
    return dict(M=M, kept=int(kept.sum()), walk=bool(any(walks)), ties=ties, keys=key[sel][kept])


def analyse_image(sm, dec, score_thresh, nms_thresh, topk, dets, want_mult=WANT_DEFAULT, fast=True, tau=None):
    """Which way one image takes through the kernels. tau: the device's tauKey (None: predicted). Returns a dict:
      nw, cap            capacity bucket and the fast kernel's list limit
      tau                cut-off key (0: everything above the threshold); counted: the class-order row is counted, not the identity
      cnt_pass [K-1]     scores above the threshold;  cnt_tau [K-1]: of those, keys >= tau (what the fast kernel lists)
      need_full, why     the fallback flag of the cut-off path and its cause ('cap' / 'few' / None)
      M, kept [K-1]      candidates entering NMS and survivors per class ON THE DECIDING PATH (fast unless need_full or fast is off)
      walk               some 64-candidate chunk of the deciding path needed the sequential walk; sel_ties [K-1]: anchors sharing a class's cut key
      merge_total        survivors entering the merge; merge_ties: survivors sharing the rank-D key; merge_whole: shift of the `whole` shortcut
      merge_in_lds       total <= MERGE_LCAP"""
    km1 = sm.shape[1] - 1
    s = np.ascontiguousarray(sm[:, 1:])
    passing = s > np.float32(score_thresh)
    key = np.where(passing, bits(s), 0).astype(np.uint32)
    nw = nw_bucket(topk)
    cap = fast_cap(nw)
    hb0, nb, clamped = hist_range(score_thresh)
    r = dict(nw=nw, cap=cap, cnt_pass=passing.sum(0), counted=nb + km1 <= HBINS, need_full=False, why=None, tau=0)
    full = not fast
    if fast:
        r["tau"] = tau_key(sm, score_thresh, want_mult * dets) if tau is None else int(tau)
        above = passing & (key >= np.uint32(r["tau"]))
        r["cnt_tau"] = above.sum(0)
        if (r["cnt_tau"] > cap).any():
            r["need_full"], r["why"] = True, "cap"
        else:
            per = [_class_pass(s[:, c], key[:, c], dec, above[:, c], topk, nms_thresh) for c in range(km1)]
            if sum(p["kept"] for p in per) < dets and r["tau"] != 0:
                r["need_full"], r["why"] = True, "few"
        full = r["need_full"]
    if full:
        per = [_class_pass(s[:, c], key[:, c], dec, passing[:, c], topk, nms_thresh) for c in range(km1)]
    r["M"] = np.array([p["M"] for p in per])
    r["kept"] = np.array([p["kept"] for p in per])
    r["walk"] = any(p["walk"] for p in per)
    r["sel_ties"] = np.array([p["ties"] for p in per])
    keys = np.concatenate([p["keys"] for p in per]) if per else np.zeros(0, np.uint32)
    r["merge_total"] = int(keys.size)
    r["merge_in_lds"] = keys.size <= MERGE_LCAP
    r["merge_ties"], r["merge_whole"] = 0, None
    if keys.size > dets:
        T, quota, whole = radix_select(keys, dets, True)
        r["merge_whole"] = whole
        if whole is None:
            r["merge_ties"] = int((keys == np.uint32(T)).sum())
            assert (keys > np.uint32(T)).sum() + quota == dets
    return r


# ------------------------------------------------------------------------------------------------------------------------------------
# designed inputs
# ------------------------------------------------------------------------------------------------------------------------------------
def lattice_scores(count, top=0.11, per_bin=64):
    """`count` distinct float32 scores, descending from just below `top`: in every histogram bin (float bits >> HSHIFT) `per_bin` values between
    a quarter and three quarters of the bin, 2^(HSHIFT - 1) / per_bin units in the last place apart (per_bin 64: 2^12 ulp, a relative 2^-11 at
    least 2^-12) -- a device softmax a few ulp off reproduces their order and their bins."""
    step = (1 << (HSHIFT - 1)) // per_bin
    assert step >= 1 << 11
    h = (int(bits(np.float32(top))) >> HSHIFT) - 1
    out = np.empty(count, np.uint32)
    for i in range(count):
        b, j = divmod(i, per_bin)
        out[i] = ((h - b) << HSHIFT) + (1 << (HSHIFT - 2)) + (per_bin - 1 - j) * step
    return out.view(np.float32)


def logits_from_scores(p):
    """p [..., A, K-1]: target foreground scores, 0 = exactly zero (OFF_LOGIT); rows sum to less than 1. Logits [..., A, K] float32 whose softmax
    is p: background 0, foreground log(p / (1 - sum p))."""
    p = np.asarray(p, np.float64)
    bg = 1.0 - p.sum(-1, keepdims=True)
    assert (bg > 1e-3).all(), "the target scores of an anchor must leave room for the background"
    with np.errstate(divide="ignore"):
        fg = np.where(p > 0, np.log(np.where(p > 0, p, 1.0) / bg), OFF_LOGIT)
    return np.concatenate([np.zeros_like(bg), fg], -1).astype(np.float32)


def ulp_bound(p):
    """How far (in units of the last place) a softmax may be from the target p it was built for. The logit log(p / bg) is rounded to float32:
    half an ulp of a logit below 4.2 in magnitude (p >= 2^-6 here) is 1.2e-7, two ulp of p at worst, and the softmax adds its own one or two: 4.
    Smaller targets (the cases about the clamped histogram go down to 1e-10, a logit of -23, half an ulp 9.5e-7: 16 ulp of p): 40. The lattice
    is 2048 ulp apart at least, so either keeps order and bin."""
    return np.where(np.asarray(p) >= 2.0 ** -6, 4, 40)


class Scene:
    """Anchors with integer coordinates (zero regression: the decoded box IS the anchor, every IoU is exact in fp32) and target scores per
    (image, label). add() returns the anchor's index; anchors are numbered in the order they are added."""

    def __init__(self, n=1, K=2):
        self.n, self.K = n, K
        self.boxes, self.rows = [], []
        self._cell = 0

    def add(self, box, scores=None):
        """scores: {(image, label): p} (label 1 .. K-1)"""
        self.boxes.append(tuple(float(v) for v in box))
        self.rows.append(dict(scores or {}))
        return len(self.boxes) - 1

    def cell(self):
        """The next of 6400 pairwise disjoint (touching at most) 4 x 4 boxes inside 320 x 320."""
        i = self._cell
        self._cell += 1
        assert i < 6400
        x, y = 4 * (i % 80), 4 * (i // 80)
        return (x, y, x + 4, y + 4)

    def add_cells(self, scores, img=0, label=1):
        return [self.add(self.cell(), {(img, label): float(v)}) for v in scores]

    def pad_to(self, A):
        assert len(self.boxes) <= A
        while len(self.boxes) < A:
            self.add((300, 300, 310, 310))
        return self

    def arrays(self):
        A = len(self.boxes)
        p = np.zeros((self.n, A, self.K - 1), np.float64)
        for a, row in enumerate(self.rows):
            for (img, label), v in row.items():
                p[img, a, label - 1] = v
        anchors = np.asarray(self.boxes, np.float32).reshape(A, 4)
        return logits_from_scores(p), np.zeros((self.n, A, 4), np.float32), anchors, p.astype(np.float32)


def chain_box(i, y=0, x0=0):
    """Box i of a row in which each box suppresses its successor only, at nms_thresh 0.5: width 4, pitch 1 -- IoU(i, i+1) = 3/5,
    IoU(i, i+2) = 2/6. Greedy NMS keeps every other box, and box i's fate depends on all i boxes before it."""
    return (x0 + i, y, x0 + i + 4, y + 1)


# ------------------------------------------------------------------------------------------------------------------------------------
# source text the mirrors are held to
# ------------------------------------------------------------------------------------------------------------------------------------
def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def source_constants():
    common, choice, post = source("common.h"), source("choice.h"), source("postprocess.hip")
    num = lambda pat, txt: int(re.search(pat, txt).group(1))
    return dict(HSHIFT=num(r"constexpr int DN_PP_HSHIFT = (\d+);", common), HBINS=num(r"constexpr int DN_PP_HBINS = (\d+);", common),
                MERGE_LCAP=num(r"constexpr int MERGE_LCAP = (\d+);", post),
                FIXED_POINT_ROUNDS=num(r"for \(int it = 0; it < (\d+); \+\+it\)", post),
                FAST_CAP_MAX=num(r"constexpr int CAP = \(64 \* NW \* NW < (\d+)\) \? 64 \* NW \* NW : \1;", post),
                WANT_DEFAULT=num(r'dn_knob\("DN_PP_WANT", (\d+)\)', post),
                nw_bucket=re.search(r"constexpr int post_nw_bucket\(int topk\) \{\s*const int w = \(topk \+ 63\) / 64;\s*return (.*?);\s*\}", choice).group(1))
