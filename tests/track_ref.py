"""TEST INFRASTRUCTURE: the reference of the device tracker (demonet_amd/track.py, csrc/track.hip).

`RefTracker` restates the text of include/demonet_hip.h (dn_track_update) in numpy float32, one operation per line: the filter as scalar float32
arithmetic, the association as the sequential greedy walk over the admissible pairs in the total order (IoU descending, slot ascending, row
ascending). A correct device implementation must agree with it bit for bit: every output and every field of the state, after every frame.
`defect` plants one deviation from the text at a time (tests/test_track.py shows that each of them is visible).

`predict64` / `update64` are the published filter (ByteTrack's KalmanFilter: 8 x 8 matrices, F, H, Q, R) in float64. `scene` is the seeded scene
generator of the tests and of tools/time_track.py.
"""
import numpy as np

f32 = np.float32
DEFECTS = ("ge", "lost_stage2", "keep_vh", "predict_tentative", "tie_high_slot", "id_score_order")
FREE, TENTATIVE, TRACKED, LOST = 0, 1, 2, 3
WP, WV = f32(0.05), f32(0.00625)          # 1 / 20 and 1 / 160 rounded to float32
A_P0, A_V0, A_QP, A_QV, A_R = f32(1e-2) * f32(1e-2), f32(1e-5) * f32(1e-5), f32(1e-2) * f32(1e-2), f32(1e-5) * f32(1e-5), f32(1e-1) * f32(1e-1)
HALF, TWO, TEN = f32(0.5), f32(2), f32(10)


def iou_row(a, b):
    """IoU of the track box a [4] with the detection boxes b [n, 4]: float32, the operation order of dn_merge_detections (the track as a_i)."""
    xx1 = np.where(a[0] > b[:, 0], a[0], b[:, 0])
    yy1 = np.where(a[1] > b[:, 1], a[1], b[:, 1])
    xx2 = np.where(a[2] < b[:, 2], a[2], b[:, 2])
    yy2 = np.where(a[3] < b[:, 3], a[3], b[:, 3])
    with np.errstate(all="ignore"):
        w = xx2 - xx1
        h = yy2 - yy1
        w = np.where(w < 0, f32(0), w)
        h = np.where(h < 0, f32(0), h)
        inter = w * h
        aa = (a[2] - a[0]) * (a[3] - a[1])
        ab = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        u = inter / ((aa + ab) - inter)
    assert u.dtype == np.float32
    return u


def measure(b):
    """box -> measurement (cx, cy, a, h)."""
    w = b[2] - b[0]
    h = b[3] - b[1]
    cx = b[0] + w * HALF
    cy = b[1] + h * HALF
    a = w / h
    return np.array([cx, cy, a, h], f32)


def mean_box(f):
    """mean -> box; f = the 20 filter floats of one track, f[5 k + (0 x, 1 v, 2 Pxx, 3 Pxv, 4 Pvv)]."""
    h = f[15]
    w = f[10] * h
    x1 = f[0] - w * HALF
    y1 = f[5] - h * HALF
    x2 = x1 + w
    y2 = y1 + h
    return np.array([x1, y1, x2, y2], f32)


def kf_init(b):
    z = measure(b)
    H = z[3]
    sp = WP * H
    sv = WV * H
    p2 = TWO * sp
    v10 = TEN * sv
    f = np.zeros(20, f32)
    for k in range(4):
        f[5 * k + 0] = z[k]
        f[5 * k + 1] = f32(0)
        f[5 * k + 2] = A_P0 if k == 2 else p2 * p2
        f[5 * k + 3] = f32(0)
        f[5 * k + 4] = A_V0 if k == 2 else v10 * v10
    return f


def kf_predict(f):
    f = f.copy()
    H = f[15]
    sp = WP * H
    sv = WV * H
    for k in range(4):
        qp = A_QP if k == 2 else sp * sp
        qv = A_QV if k == 2 else sv * sv
        x, v, pxx, pxv, pvv = f[5 * k:5 * k + 5]
        f[5 * k + 0] = x + v
        t = TWO * pxv
        t = pxx + t
        t = t + pvv
        f[5 * k + 2] = t + qp
        f[5 * k + 3] = pxv + pvv
        f[5 * k + 4] = pvv + qv
    return f


def kf_update(f, b):
    f = f.copy()
    z = measure(b)
    H = f[15]
    sp = WP * H
    for k in range(4):
        r = A_R if k == 2 else sp * sp
        x, v, pxx, pxv, pvv = f[5 * k:5 * k + 5]
        S = pxx + r
        kx = pxx / S
        kv = pxv / S
        y = z[k] - x
        f[5 * k + 0] = x + kx * y
        f[5 * k + 1] = v + kv * y
        ks = kx * S
        vs = kv * S
        f[5 * k + 2] = pxx - ks * kx
        f[5 * k + 3] = pxv - ks * kv
        f[5 * k + 4] = pvv - vs * kv
    assert f.dtype == np.float32
    return f


def greedy(pairs, high_slot=False):
    """The sequential walk: pairs (u, slot, row) in the order (u descending, slot ascending, row ascending); a pair is taken when both are free."""
    taken_t, taken_d, out = set(), set(), []
    for u, s, j in sorted(pairs, key=lambda p: (-float(p[0]), -p[1] if high_slot else p[1], p[2])):
        if s in taken_t or j in taken_d:
            continue
        taken_t.add(s)
        taken_d.add(j)
        out.append((s, j))
    return out


class RefTracker:
    def __init__(self, streams, max_tracks=256, track_thresh=0.5, low_thresh=0.1, new_thresh=None, match_thresh=0.8, second_thresh=0.5,
                 unconfirmed_thresh=0.7, track_buffer=30, class_agnostic=False, defect=None):
        assert defect is None or defect in DEFECTS, defect
        self.B, self.T, self.defect = streams, max_tracks, defect
        self.track_thresh, self.low_thresh = f32(track_thresh), f32(low_thresh)
        self.new_thresh = f32(float(track_thresh) + 0.1 if new_thresh is None else new_thresh)
        self.gate = {1: f32(1) - f32(match_thresh), 2: f32(1) - f32(second_thresh), 3: f32(1) - f32(unconfirmed_thresh)}
        self.track_buffer, self.agnostic = int(track_buffer), bool(class_agnostic)
        B, T = streams, max_tracks
        self.frame, self.next_id, self.dropped = np.zeros(B, np.int32), np.ones(B, np.int32), np.zeros(B, np.int32)
        self.state, self.id, self.label = np.zeros((B, T), np.int32), np.zeros((B, T), np.int32), np.zeros((B, T), np.int64)
        self.score, self.filter = np.zeros((B, T), f32), np.zeros((B, 20, T), f32)
        self.start_frame, self.last_frame, self.det = np.zeros((B, T), np.int32), np.zeros((B, T), np.int32), np.zeros((B, T), np.int32)
        self.assoc_log = []          # per update, stream and stage: dict(stream, stage, slots, rows, iou [len(slots), len(rows)], ok, gate, matches)

    FIELDS = ("frame", "next_id", "dropped", "state", "id", "label", "score", "filter", "start_frame", "last_frame", "det")

    def table(self):
        return {k: getattr(self, k) for k in self.FIELDS}

    def reset(self, streams=None):
        for b in (range(self.B) if streams is None else streams):
            self.frame[b], self.next_id[b], self.dropped[b] = 0, 1, 0
            for k in self.FIELDS[3:]:
                getattr(self, k)[b] = 0

    def _clear(self, b, s):
        for k in self.FIELDS[3:]:
            getattr(self, k)[b][..., s] = 0

    def _associate(self, b, stage, slots, rows, tbox, dboxes, dlabels):
        gate = self.gate[stage]
        pairs = []
        iou = np.zeros((len(slots), len(rows)), f32)
        ok = np.zeros((len(slots), len(rows)), bool)
        if rows:
            for i, s in enumerate(slots):
                u = iou_row(tbox[s], dboxes[rows])
                iou[i] = u
                same = np.ones(len(rows), bool) if self.agnostic else dlabels[rows] == self.label[b, s]
                with np.errstate(invalid="ignore"):
                    ok[i] = same & ((u >= gate) if self.defect == "ge" else (u > gate))      # (a NaN compares false)
                for c in np.nonzero(ok[i])[0]:
                    pairs.append((u[c], s, rows[c]))
        matches = greedy(pairs, high_slot=self.defect == "tie_high_slot")
        self.assoc_log.append(dict(stream=b, stage=stage, slots=list(slots), rows=list(rows), iou=iou, ok=ok, gate=gate, matches=matches))
        return matches

    def update(self, boxes, scores, labels, counts):
        boxes, scores = np.asarray(boxes, f32), np.asarray(scores, f32)
        labels, counts = np.asarray(labels, np.int64), np.asarray(counts, np.int32)
        B, T = self.B, self.T
        d = scores.shape[1]
        assert scores.shape[0] == B
        ob, os_, ol = np.zeros((B, T, 4), f32), np.zeros((B, T), f32), np.zeros((B, T), np.int64)
        oi, od, oc = np.zeros((B, T), np.int64), np.full((B, T), -1, np.int32), np.zeros(B, np.int32)
        det_ids = np.full((B, d), -1, np.int64)
        for b in range(B):
            self.frame[b] += 1                                                     # 1.
            frame = int(self.frame[b])
            n = min(max(int(counts[b]), 0), d)
            high, low = [], []                                                     # 2.
            for j in range(n):
                s, bx = scores[b, j], boxes[b, j]
                if np.isnan(s) or not np.all(np.isfinite(bx)):
                    continue
                with np.errstate(all="ignore"):
                    if not (bx[2] - bx[0] > 0) or not (bx[3] - bx[1] > 0):
                        continue
                if s >= self.track_thresh:
                    high.append(j)
                elif s > self.low_thresh and s < self.track_thresh:
                    low.append(j)
            before = self.state[b].copy()
            for s in range(T):                                                     # 3.
                if before[s] != FREE:
                    self.det[b, s] = -1
                predicted = before[s] in (TRACKED, LOST) or (self.defect == "predict_tentative" and before[s] == TENTATIVE)
                if before[s] == LOST and self.defect != "keep_vh":
                    self.filter[b, 16, s] = f32(0)
                if predicted:
                    self.filter[b, :, s] = kf_predict(self.filter[b, :, s])
            tbox = {s: mean_box(self.filter[b, :, s]) for s in range(T) if before[s] != FREE}
            taken = {}                                                             # row -> slot
            matched = set()

            def apply(matches):
                for s, j in matches:
                    self.filter[b, :, s] = kf_update(self.filter[b, :, s], boxes[b, j])
                    self.score[b, s] = scores[b, j]
                    self.state[b, s] = TRACKED
                    self.last_frame[b, s] = frame
                    self.det[b, s] = j
                    taken[j] = s
                    matched.add(s)
                    det_ids[b, j] = self.id[b, s]

            apply(self._associate(b, 1, [s for s in range(T) if before[s] in (TRACKED, LOST)], high, tbox, boxes[b], labels[b]))      # 4.
            second = [s for s in range(T) if s not in matched and (before[s] == TRACKED or (self.defect == "lost_stage2" and before[s] == LOST))]
            apply(self._associate(b, 2, second, low, tbox, boxes[b], labels[b]))                                                        # 5.
            for s in range(T):
                if before[s] == TRACKED and s not in matched:
                    self.state[b, s] = LOST
            rest = [j for j in high if j not in taken]
            apply(self._associate(b, 3, [s for s in range(T) if before[s] == TENTATIVE], rest, tbox, boxes[b], labels[b]))             # 6.
            for s in range(T):
                if before[s] == TENTATIVE and s not in matched:
                    self._clear(b, s)
            starts = [j for j in high if j not in taken and scores[b, j] >= self.new_thresh]                                            # 7.
            if self.defect == "id_score_order":
                starts.sort(key=lambda j: (-float(scores[b, j]), j))
            free = [s for s in range(T) if self.state[b, s] == FREE]
            for r, j in enumerate(starts):
                if r >= len(free):
                    self.dropped[b] += 1
                    continue
                s = free[r]
                self.filter[b, :, s] = kf_init(boxes[b, j])
                self.state[b, s] = TRACKED if frame == 1 else TENTATIVE
                self.id[b, s] = self.next_id[b]
                self.next_id[b] += 1
                self.label[b, s], self.score[b, s] = labels[b, j], scores[b, j]
                self.start_frame[b, s] = self.last_frame[b, s] = frame
                self.det[b, s] = j
                if frame == 1:
                    det_ids[b, j] = self.id[b, s]
            for s in range(T):                                                     # 8.
                if self.state[b, s] == LOST and frame - int(self.last_frame[b, s]) > self.track_buffer:
                    self._clear(b, s)
            r = 0                                                                  # 9.
            for s in range(T):
                if self.state[b, s] == TRACKED and self.last_frame[b, s] == frame:
                    ob[b, r], os_[b, r], ol[b, r] = mean_box(self.filter[b, :, s]), self.score[b, s], self.label[b, s]
                    oi[b, r], od[b, r] = self.id[b, s], self.det[b, s]
                    r += 1
            oc[b] = r
        return ob, os_, ol, oi, od, oc, det_ids


# ---------------------------------------------------------------------------------------------------------- the published filter, float64
def _matrices():
    F = np.eye(8)
    for i in range(4):
        F[i, 4 + i] = 1.0
    return F, np.eye(4, 8)


def to64(f):
    """The 20 floats of a track -> (mean [8], covariance [8, 8]) in float64, ByteTrack's order (cx, cy, a, h, vcx, vcy, va, vh)."""
    f = np.asarray(f, np.float64)
    mean, cov = np.zeros(8), np.zeros((8, 8))
    for k in range(4):
        mean[k], mean[4 + k] = f[5 * k], f[5 * k + 1]
        cov[k, k], cov[k, 4 + k], cov[4 + k, k], cov[4 + k, 4 + k] = f[5 * k + 2], f[5 * k + 3], f[5 * k + 3], f[5 * k + 4]
    return mean, cov


def predict64(mean, cov):
    """KalmanFilter.predict of the published tracker."""
    F, _ = _matrices()
    wp, wv = float(WP), float(WV)          # (the float32 weights, exactly: the comparison is about the arithmetic, not about 1 / 20 in binary)
    std = [wp * mean[3], wp * mean[3], 1e-2, wp * mean[3], wv * mean[3], wv * mean[3], 1e-5, wv * mean[3]]
    Q = np.diag(np.square(std))
    return F @ mean, F @ cov @ F.T + Q


def update64(mean, cov, z):
    """KalmanFilter.update of the published tracker (project, gain by a linear solve, correct)."""
    _, H = _matrices()
    wp = float(WP)
    R = np.diag(np.square([wp * mean[3], wp * mean[3], 1e-1, wp * mean[3]]))
    pm, S = H @ mean, H @ cov @ H.T + R
    K = np.linalg.solve(S, (cov @ H.T).T).T
    return mean + K @ (z - pm), cov - K @ S @ K.T


# ---------------------------------------------------------------------------------------------------------- scenes
def scene(seed, frames, streams, d, objects=6, size=640.0, separated=False, max_dropout=5, false_positives=2, garbage=True, exits=True):
    """A seeded sequence: `objects` boxes per stream move at constant velocity with box jitter; dropouts of 1 .. max_dropout frames, score dips
    into the low band, entries and exits, two crossing objects (objects 0 and 1, same label), false positives, garbage in the rows at or beyond
    the count, NaN scores and degenerate boxes among the rows (exits=False: nobody leaves). separated=True: objects on lanes that never overlap, no crossing, no false positives.
    -> (list of per-frame (boxes [B, d, 4] f32, scores [B, d] f32, labels [B, d] i64, counts [B] i32), truth): truth[f][b] = {row: object}."""
    rng = np.random.RandomState(seed)
    out, truth = [], []
    objs = []
    for b in range(streams):
        lst = []
        for o in range(objects):
            w, h = rng.uniform(40, 90), rng.uniform(50, 110)
            if separated:
                lane = size / objects
                h = min(h, lane * 0.6)
                p = np.array([rng.uniform(50, 120), lane * o + lane / 2 - h / 2])
                v = np.array([rng.uniform(2, 6), 0.0])
            else:
                p = rng.uniform(60, size - 160, 2)
                v = rng.uniform(-5, 5, 2)
            lst.append(dict(p=p, v=v, w=w, h=h, label=int(rng.randint(1, 4)), enter=int(rng.randint(0, 4)) if o >= 2 else 0,
                            leave=int(rng.randint(frames // 2, frames + 10)) if o >= 3 and exits else frames + 10, off=0))
        if not separated and objects >= 2:      # the crossing pair: towards each other on one line
            lst[0].update(p=np.array([100.0, 300.0]), v=np.array([6.0, 0.0]), w=60.0, h=80.0, label=1)
            lst[1].update(p=np.array([100.0 + 6.0 * frames, 300.0]), v=np.array([-6.0, 0.0]), w=60.0, h=80.0, label=1)
        objs.append(lst)
    for fr in range(frames):
        bx = rng.uniform(-50, 700, (streams, d, 4)).astype(f32)      # garbage everywhere; the rows below the count are overwritten
        sc = rng.uniform(0, 1, (streams, d)).astype(f32)
        lb = rng.randint(0, 5, (streams, d)).astype(np.int64)
        ct = np.zeros(streams, np.int32)
        tr = []
        if not garbage:
            bx[:], sc[:], lb[:] = 0, 0, 0
        for b in range(streams):
            rows = []
            for o, ob in enumerate(objs[b]):
                ob["p"] = ob["p"] + ob["v"]
                if fr < ob["enter"] or fr >= ob["leave"]:
                    continue
                if ob["off"] > 0:
                    ob["off"] -= 1
                    continue
                if fr > 2 and rng.uniform() < 0.06 and max_dropout > 0:
                    ob["off"] = int(rng.randint(1, max_dropout + 1)) - 1
                    continue
                jit = rng.normal(0, 1.0, 4)
                x1, y1 = ob["p"][0] + jit[0], ob["p"][1] + jit[1]
                box = [x1, y1, x1 + ob["w"] + jit[2], y1 + ob["h"] + jit[3]]
                s = rng.uniform(0.75, 0.98) if rng.uniform() > 0.12 else rng.uniform(0.15, 0.45)      # a dip into the low band
                rows.append((box, s, ob["label"], o))
            if not separated:
                for _ in range(int(rng.randint(0, false_positives + 1))):
                    x1, y1 = rng.uniform(0, size - 100, 2)
                    rows.append(([x1, y1, x1 + rng.uniform(20, 80), y1 + rng.uniform(20, 80)], rng.uniform(0.05, 0.9), int(rng.randint(1, 4)), -1))
                if rng.uniform() < 0.3:
                    rows.append(([10, 10, 50, 50], np.nan, 1, -1))                                     # a NaN score
                if rng.uniform() < 0.3:
                    rows.append(([200, 200, 200, 260], 0.9, 2, -1))                                    # w = 0
                if rng.uniform() < 0.2:
                    rows.append(([300, 300, 280, 340], 0.9, 2, -1))                                    # w < 0
                if rng.uniform() < 0.2:
                    rows.append(([np.inf, 0, 50, 50], 0.9, 1, -1))                                     # a coordinate that is not finite
                if rng.uniform() < 0.2:
                    rows.append(([np.nan, 0, 50, 50], 0.9, 1, -1))
            order = rng.permutation(len(rows))[:d]
            t = {}
            for r, k in enumerate(order):
                box, s, l, o = rows[k]
                bx[b, r], sc[b, r], lb[b, r] = np.asarray(box, f32), f32(s), l
                if o >= 0:
                    t[r] = o
            ct[b] = len(order)
            tr.append(t)
        out.append((bx, sc, lb, ct))
        truth.append(tr)
    return out, truth
