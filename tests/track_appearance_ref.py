"""TEST INFRASTRUCTURE: the reference of the tracker's appearance step (demonet_amd/track.py AppearanceTracker, csrc/trackapp.hip).

`AppRefTracker` restates the text of include/demonet_hip.h (dn_track_update_appearance) on top of tests/track_ref.RefTracker, through its
`_associate` hook: the association is RefTracker's sequential greedy walk with the fused value v in place of u. The features are updated from
what a step did to each slot (started, matched, freed), read off the state after RefTracker.update.

On the GPU the reference is TEACHER-FORCED: update(..., S=..., en=...) associates with the device's own similarity matrix and starts features
from the device's own normalised rows, so nothing it decides depends on how the matrix cores or the norm's sum round, and the association must
agree bit for bit. Without them it computes both itself (float64 dot of the fp16 operands, rounded to float32).
`app_defect` plants one deviation from the text at a time (tests/test_track_appearance.py shows that each of them is visible).
"""
import numpy as np

import track_ref as tr

f32, f16 = np.float32, np.float16
APP_DEFECTS = ("lt", "no_proximity", "no_renorm", "stage2_fused")
ONE, HALF, ZERO = f32(1), f32(0.5), f32(0)


def fused(u, s, app_thresh, prox_thresh, defect=None):
    """The pair value of pairs whose track and row both have a feature: float32 scalars or arrays, one operation per line."""
    u, s = np.asarray(u, f32), np.asarray(s, f32)
    with np.errstate(all="ignore"):
        h = ONE - s
        h = h * HALF
        e = np.where(h < ZERO, ZERO, h)                   # (a NaN stays)
        far = ONE - u
        if defect == "lt":
            adm = (e < app_thresh) & (far < prox_thresh)
        elif defect == "no_proximity":
            adm = e <= app_thresh
        else:
            adm = (e <= app_thresh) & (far <= prox_thresh)      # (a NaN compares false)
        w = ONE - e
        v = np.where(adm, np.where(u > w, u, w), u)
    assert v.dtype == np.float32
    return v[()]


def normalise(emb):
    """-> (present [E] bool, en [E, dim] float16): the rows divided by their float32 norm, rounded to fp16; absent rows are 0."""
    x = np.asarray(emb).astype(f32)
    with np.errstate(all="ignore"):
        fin = np.all(np.isfinite(x), axis=1)
        nrm = np.sqrt(np.sum(x * x, axis=1, dtype=f32))
        ok = fin & (nrm > 0) & np.isfinite(nrm)
        en = np.where(ok[:, None], x / np.where(ok, nrm, ONE)[:, None], ZERO).astype(f16)
    return ok, en


def row_map(index, counts, B, d):
    """[B, d] int: the highest slot whose index row names (stream, row) validly, or -1."""
    m = np.full((B, d), -1, np.int64)
    if index is None:
        return m
    for e, row in enumerate(np.asarray(index)):
        b, j = int(row[0]), int(row[1])
        if 0 <= b < B and j >= 0 and j < min(max(int(counts[b]), 0), d):
            m[b, j] = e                                   # (ascending e: the highest wins)
    return m


class AppRefTracker(tr.RefTracker):
    def __init__(self, streams, dim, alpha=0.9, appearance_thresh=0.25, proximity_thresh=0.5, app_defect=None, **kw):
        assert app_defect is None or app_defect in APP_DEFECTS, app_defect
        super().__init__(streams, **kw)
        self.dim, self.app_defect = dim, app_defect
        self.alpha = f32(alpha)
        self.beta = ONE - self.alpha
        self.app_thresh, self.prox_thresh = f32(appearance_thresh), f32(proximity_thresh)
        self.fvalid = np.zeros((self.B, self.T), bool)
        self.feat = np.zeros((self.B, self.T, dim), f32)
        self._S = self._rowhas = None

    def reset(self, streams=None):
        super().reset(streams)
        for b in (range(self.B) if streams is None else streams):
            self.fvalid[b] = False
            self.feat[b] = 0

    def similarity(self, en, rmap):
        """S [B, T, d] float32 of the features as they stand: the float64 dot of the fp16 operands (exact products), rounded once."""
        B, T = self.B, self.T
        d = rmap.shape[1]
        S = np.zeros((B, T, d), f32)
        a = self.feat.astype(f16).astype(np.float64)
        for b in range(B):
            for j in range(d):
                if self._rowhas[b, j]:
                    S[b, :, j] = np.where(self.fvalid[b], a[b] @ en[rmap[b, j]].astype(np.float64), 0.0).astype(f32)
        return S

    def _associate(self, b, stage, slots, rows, tbox, dboxes, dlabels):
        if self._rowhas is None or (stage == 2 and self.app_defect != "stage2_fused"):
            return super()._associate(b, stage, slots, rows, tbox, dboxes, dlabels)
        gate = self.gate[stage]
        pairs = []
        val = np.zeros((len(slots), len(rows)), f32)
        ok = np.zeros((len(slots), len(rows)), bool)
        if rows:
            for i, s in enumerate(slots):
                v = tr.iou_row(tbox[s], dboxes[rows]).copy()
                if self.fvalid[b, s]:
                    v = np.where(self._rowhas[b, rows], fused(v, self._S[b, s, rows], self.app_thresh, self.prox_thresh, self.app_defect), v)
                val[i] = v
                same = np.ones(len(rows), bool) if self.agnostic else dlabels[rows] == self.label[b, s]
                with np.errstate(invalid="ignore"):
                    ok[i] = same & (v > gate)
                for c in np.nonzero(ok[i])[0]:
                    pairs.append((v[c], s, rows[c]))
        matches = tr.greedy(pairs)
        self.assoc_log.append(dict(stream=b, stage=stage, slots=list(slots), rows=list(rows), iou=val, ok=ok, gate=gate, matches=matches))
        return matches

    def update(self, boxes, scores, labels, counts, emb=None, index=None, S=None, en=None):
        counts = np.asarray(counts, np.int32)
        B, T = self.B, self.T
        d = np.asarray(scores).shape[1]
        if emb is None:
            rmap = np.full((B, d), -1, np.int64)
            self._rowhas = np.zeros((B, d), bool)
            self._S = np.zeros((B, T, d), f32)
        else:
            present, own = normalise(emb)
            en = own if en is None else np.asarray(en)
            rmap = row_map(index, counts, B, d)
            self._rowhas = (rmap >= 0) & present[np.maximum(rmap, 0)]
            self._S = self.similarity(en, rmap) if S is None else np.asarray(S, f32)
        out = super().update(boxes, scores, labels, counts)
        for b in range(B):
            frame = int(self.frame[b])
            for s in range(T):
                if self.state[b, s] == tr.FREE:
                    self.fvalid[b, s] = False
                    continue
                if self.last_frame[b, s] != frame:
                    continue                                   # not seen in this frame
                j = int(self.det[b, s])
                if self.start_frame[b, s] == frame:            # started
                    self.fvalid[b, s] = bool(self._rowhas[b, j])
                    if self._rowhas[b, j]:
                        self.feat[b, s] = en[rmap[b, j]].astype(f32)
                elif self._rowhas[b, j]:                       # matched with a row that has an embedding
                    x = en[rmap[b, j]].astype(f32)
                    if not self.fvalid[b, s]:
                        self.feat[b, s], self.fvalid[b, s] = x, True
                        continue
                    with np.errstate(all="ignore"):
                        t0 = self.alpha * self.feat[b, s]
                        t1 = self.beta * x
                        v = t0 + t1
                        nrm = np.sqrt(np.sum(v * v, dtype=f32))
                        good = bool(nrm > 0) and bool(np.isfinite(nrm))
                        self.feat[b, s] = v if self.app_defect == "no_renorm" else v / nrm
                    assert self.feat.dtype == np.float32
                    self.fvalid[b, s] = good
        self._rowhas = None
        return out


# ---------------------------------------------------------------------------------------------------------- scenes
def embed_scene(truth, counts, dim, seed, E, drop=0.2, noise=0.05, fp=0.5):
    """Embeddings for the frames of track_ref.scene: object o of stream b has a fixed random unit direction; a row that shows it gets that
    direction plus noise, except that a fraction `drop` of the rows gets none; a fraction `fp` of the other rows below the count gets a random
    one. The E slots are shuffled; the unused ones hold random numbers behind an index row of -1.
    -> per frame (emb [E, dim] float32, index [E, 8] int32)."""
    rng = np.random.RandomState(seed)
    base = {}
    out = []
    for f, per_stream in enumerate(truth):
        rows = []
        for b, t in enumerate(per_stream):
            for j in range(int(counts[f][b])):
                if j in t:
                    if rng.uniform() < drop:
                        continue
                    key = (b, t[j])
                    if key not in base:
                        v = rng.normal(0, 1, dim)
                        base[key] = v / np.linalg.norm(v)
                    rows.append((b, j, base[key] + rng.normal(0, noise / np.sqrt(dim), dim)))
                elif rng.uniform() < fp:
                    rows.append((b, j, rng.normal(0, 1, dim)))
        assert len(rows) <= E, (len(rows), E)
        emb = rng.normal(0, 1, (E, dim)).astype(f32)
        index = np.zeros((E, 8), np.int32)
        index[:, 0] = -1
        for e, (b, j, v) in zip(rng.permutation(E)[:len(rows)], rows):
            emb[e] = (v * rng.uniform(0.5, 20.0)).astype(f32)      # (any length: the step normalises)
            index[e, :2] = (b, j)
            index[e, 2:6] = rng.randint(0, 100, 4)                 # (the cropper's rectangle words: not read)
        out.append((emb, index))
    return out


def crossing_scene(dim=64, frames=24, cross=10):
    """Two objects of one class on one line meet, their boxes COINCIDE in frame `cross`, and they turn back the way they came, a little slower: to
    a tracker that sees boxes only they appear to pass through each other, so plain ByteTrack swaps their ids; their embeddings, two
    near-orthogonal directions, say who is who. One stream, d = 4; row 0 is object A, row 1 object B.
    -> (frames of (boxes, scores, labels, counts), per frame (emb [2, dim] float32, index [2, 8] int32))."""
    a = np.zeros(dim)
    b = np.zeros(dim)
    a[0], a[1] = 1.0, 0.05
    b[1], b[0] = 1.0, 0.05
    out, embs = [], []
    x0 = 300.0
    for f in range(frames):
        k = f - cross
        off = 6.0 * k if k <= 0 else -4.0 * k                # A comes from the left and goes back to the left
        bx = np.zeros((1, 4, 4), f32)
        sc = np.zeros((1, 4), f32)
        lb = np.zeros((1, 4), np.int64)
        bx[0, 0] = (x0 + off, 300.0, x0 + off + 60.0, 380.0)
        bx[0, 1] = (x0 - off, 300.0, x0 - off + 60.0, 380.0)
        sc[0, :2] = 0.9
        lb[0, :2] = 1
        out.append((bx, sc, lb, np.array([2], np.int32)))
        index = np.zeros((2, 8), np.int32)
        index[:, 1] = (0, 1)
        embs.append((np.stack([a, b]).astype(f32), index))
    return out, embs


def quarter_vectors(n, dim, seed):
    """n vectors with 16 non-zero entries of +-1/4: norm exactly 1, and every partial sum of a product of two of them is a multiple of 1/16."""
    rng = np.random.RandomState(seed)
    v = np.zeros((n, dim), f32)
    for i in range(n):
        v[i, rng.permutation(dim)[:16]] = rng.choice([-0.25, 0.25], 16)
    return v


BOX = (100.0, 100.0, 160.0, 180.0)          # w = 60, h = 80: every mean <-> box conversion is exact


def _one_stream(rows_per_frame, embs_per_frame, dim, d=4):
    """rows: per frame a list of (box, score, label); embs: per frame a list of (row, vector) -> (frames, embeddings) of one stream."""
    frames, embs = [], []
    for rows, es in zip(rows_per_frame, embs_per_frame):
        bx, sc, lb = np.zeros((1, d, 4), f32), np.zeros((1, d), f32), np.zeros((1, d), np.int64)
        for j, (box, s, l) in enumerate(rows):
            bx[0, j], sc[0, j], lb[0, j] = box, s, l
        frames.append((bx, sc, lb, np.array([len(rows)], np.int32)))
        E = max(len(es), 1)
        emb, index = np.zeros((E, dim), f32), np.zeros((E, 8), np.int32)
        index[:, 0] = -1
        for e, (j, v) in enumerate(es):
            emb[e], index[e, 0], index[e, 1] = v, 0, j
        embs.append((emb, index))
    return frames, embs


def _moved(dx, dy=0.0):
    return (BOX[0] + dx, BOX[1] + dy, BOX[2] + dx, BOX[3] + dy)


def refind_scene(dim=64):
    """An object is seen for three frames, is gone for three, and comes back 300 pixels away -- no overlap with where its lost track is -- with
    the same embedding. With proximity_thresh = 1 the lost track takes it (the same id); with 0.5 a new track starts."""
    f = quarter_vectors(1, dim, 5)[0]
    seen, back = [(BOX, 0.9, 1)], [(_moved(300.0), 0.9, 1)]
    return _one_stream([seen, seen, seen, [], [], [], back, back], [[(0, f)]] * 3 + [[]] * 3 + [[(0, f)]] * 2, dim)


def equality_scene(dim=64):
    """e EXACTLY at appearance_thresh = 0.25: the track's feature is sixteen +1/4, the second frame's embedding has twelve +1/4 and four -1/4 on the
    same support, so S = 8 / 16 = 0.5 and e = 0.25 with no rounding anywhere. The second box does not overlap the first (proximity_thresh = 1):
    the match exists through `e <= appearance_thresh` alone."""
    f = np.zeros(dim, f32)
    f[:16] = 0.25
    g = f.copy()
    g[:4] = -0.25
    return _one_stream([[(BOX, 0.9, 1)], [(_moved(100.0), 0.9, 1)], [(_moved(100.0), 0.9, 1)]], [[(0, f)], [(0, g)], [(0, g)]], dim)


def low_row_scene(dim=64):
    """Stage 2 is IoU alone: a LOW row (score 0.3) with the track's own embedding but an IoU of 1 / 3, below the stage's gate of 0.5, matches
    nothing even with proximity_thresh = 1, and the track is lost."""
    f = quarter_vectors(1, dim, 6)[0]
    return _one_stream([[(BOX, 0.9, 1)], [(_moved(30.0), 0.3, 1)], []], [[(0, f)], [(0, f)], []], dim)


def scene_set():
    """The scenes of the association test on the GPU, and of the planted defects on the CPU:
    name -> (streams, max_tracks, dim, tracker arguments, frames, embeddings)."""
    out = {}
    for seed in range(4):
        frames, truth = tr.scene(300 + seed, 30, 3, 64, objects=7)
        embs = embed_scene(truth, [fr[3] for fr in frames], 64, 400 + seed, 96)
        kw = dict(track_buffer=6, class_agnostic=bool(seed & 1), proximity_thresh=0.5 if seed < 2 else 1.0)
        out["random{}".format(seed)] = (3, 32, 64, kw, frames, embs)
    out["crossing"] = (1, 4, 64, {}) + crossing_scene()
    out["refind_prox1"] = (1, 4, 64, dict(proximity_thresh=1.0)) + refind_scene()
    out["refind_prox05"] = (1, 4, 64, dict(proximity_thresh=0.5)) + refind_scene()
    out["equality"] = (1, 4, 64, dict(proximity_thresh=1.0)) + equality_scene()
    out["low_row"] = (1, 4, 64, dict(proximity_thresh=1.0)) + low_row_scene()
    return out


def run(streams, max_tracks, dim, kw, frames, embs, app_defect=None):
    """Steps an AppRefTracker through a scene -> (tracker, the outputs of every frame)."""
    t = AppRefTracker(streams, dim, max_tracks=max_tracks, app_defect=app_defect, **kw)
    outs = [t.update(*fr, emb=e, index=i) for fr, (e, i) in zip(frames, embs)]
    return t, outs
