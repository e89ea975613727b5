"""TEST INFRASTRUCTURE: the reference of the device analytics behind the tracker (demonet_amd/zones.py, csrc/zones.hip).

`step` restates the seven rules of include/demonet_hip.h (dn_zone_update) in numpy float32, one operation per line and one rounding per operation.
It takes the tracker's per-slot arrays of a frame -- `ByteTracker.table()` brought to the host, or `RefTracker.table()` --, the per-stream
configurations and the previous zone state, and returns the new state and the events. A correct device implementation must agree with it bit for
bit: every field of the state, every event row and every count, after every frame.
"""
import numpy as np

f32 = np.float32
HALF = f32(0.5)
MAX_LINES, MAX_ZONES, MAX_VERTS, BINS = 16, 16, 16, 8
CROSS, ENTER, EXIT, VANISH = 1, 2, 3, 4
KINDS = {CROSS: "cross", ENTER: "enter", EXIT: "exit", VANISH: "vanish"}
TRACKED = 2
COUNTERS = ("line_count", "entries", "exits", "vanished", "occupancy", "dwell_max", "dwell_sum")
SLOT_FIELDS = ("id", "bin", "has_prev", "px", "py", "inside", "enter_frame")
FIELDS = ("events_dropped",) + SLOT_FIELDS + COUNTERS


def config(lines=(), zones=()):
    """One stream's record: lines = [(ax, ay, bx, by)], zones = [[(x, y), ...]] -> dict(n_lines, lines [16, 4], n_zones, nv [16], verts [16, 16, 2])."""
    c = dict(n_lines=len(lines), lines=np.zeros((MAX_LINES, 4), f32), n_zones=len(zones), nv=np.zeros(MAX_ZONES, np.int32),
             verts=np.zeros((MAX_ZONES, MAX_VERTS, 2), f32))
    for i, ln in enumerate(lines):
        c["lines"][i] = ln
    for z, poly in enumerate(zones):
        c["nv"][z] = len(poly)
        c["verts"][z, :len(poly)] = np.asarray(poly, f32)
    return c


def new_state(streams, max_tracks):
    B, T = streams, max_tracks
    z = lambda *shape, dtype=np.int32: np.zeros(shape, dtype)      # noqa: E731
    return dict(events_dropped=z(B), id=z(B, T), bin=z(B, T), has_prev=z(B, T), px=z(B, T, dtype=f32), py=z(B, T, dtype=f32),
                inside=z(B, T, dtype=np.uint32), enter_frame=z(B, MAX_ZONES, T), line_count=z(B, MAX_LINES, 2, BINS), entries=z(B, MAX_ZONES, BINS),
                exits=z(B, MAX_ZONES, BINS), vanished=z(B, MAX_ZONES, BINS), occupancy=z(B, MAX_ZONES, BINS), dwell_max=z(B, MAX_ZONES, BINS),
                dwell_sum=z(B, MAX_ZONES, BINS, dtype=np.int64))


def reset(state, streams=None):
    for b in (range(state["id"].shape[0]) if streams is None else streams):
        for k in FIELDS:
            state[k][b] = 0


def anchor_point(f, anchor):
    """The tracker's mean -> box in its operation order, then the anchor: 0 the box centre, 1 the bottom centre. f = the slot's 20 filter floats."""
    with np.errstate(all="ignore"):
        h = f[15]
        w = f[10] * h
        t = w * HALF
        x1 = f[0] - t
        t = h * HALF
        y1 = f[5] - t
        x2 = x1 + w
        y2 = y1 + h
        ax = x1 + x2
        ax = ax * HALF
        if anchor == 0:
            ay = y1 + y2
            ay = ay * HALF
        else:
            ay = y2
    assert ax.dtype == np.float32 and ay.dtype == np.float32
    return ax, ay


def side(ax, ay, bx, by, px, py):
    with np.errstate(all="ignore"):
        l = bx - ax
        r = py - ay
        l = l * r
        r = by - ay
        q = px - ax
        r = r * q
        s = l - r
    assert s.dtype == np.float32
    return s


def crossing(line, prev, p):
    """-> None, or the direction 0 / 1 of the step prev -> p over the segment line = (ax, ay, bx, by)."""
    ax, ay, bx, by = line
    a = side(ax, ay, bx, by, prev[0], prev[1])
    c = side(ax, ay, bx, by, p[0], p[1])
    u = side(prev[0], prev[1], p[0], p[1], ax, ay)
    v = side(prev[0], prev[1], p[0], p[1], bx, by)
    if np.isnan(a) or np.isnan(c) or np.isnan(u) or np.isnan(v):
        return None
    if (a >= 0) != (c >= 0) and (u >= 0) != (v >= 0):
        return 0 if c >= 0 else 1
    return None


def inside(verts, nv, px, py):
    """Even-odd rule over the nv vertices."""
    c = False
    for e in range(nv):
        xi, yi = verts[e]
        xj, yj = verts[e - 1 if e else nv - 1]
        if (yi > py) != (yj > py):
            with np.errstate(all="ignore"):
                t = xj - xi
                q = py - yi
                t = t * q
                q = yj - yi
                t = t / q
                t = t + xi
            assert t.dtype == np.float32
            if px < t:
                c = not c
    return c


def bin_of(label, class_bin):
    if class_bin is None:
        return 0
    if label < 0 or label >= len(class_bin):
        return 255
    v = int(class_bin[int(label)])
    return v if v < BINS else 255


def _clamp(v, lo, hi):
    return min(max(int(v), lo), hi)


def step(table, configs, state, class_bin=None, anchor=1, max_events=256):
    """One analytics step behind a tracker step. table: frame [B], state, id, label, last_frame [B, T], filter [B, 20, T] of the tracker AFTER its
    update; configs: one `config` per stream; state: the previous zone state (not modified). -> (new state, events [B, max_events, 8] int32,
    counts [B] int32)."""
    assert anchor in (0, 1)
    Z = {k: v.copy() for k, v in state.items()}
    B, T = Z["id"].shape
    events = np.zeros((B, max_events, 8), np.int32)
    counts = np.zeros(B, np.int32)
    for b in range(B):
        cfg = configs[b]
        f = int(table["frame"][b])
        n_lines, n_zones = _clamp(cfg["n_lines"], 0, MAX_LINES), _clamp(cfg["n_zones"], 0, MAX_ZONES)
        nv = [_clamp(v, 3, MAX_VERTS) for v in cfg["nv"]]
        Z["occupancy"][b] = 0
        evs = []
        for s in range(T):
            t_state, t_id, t_label = int(table["state"][b, s]), int(table["id"][b, s]), int(table["label"][b, s])
            lab32 = int(np.array(t_label, np.int64).astype(np.int32))
            # 1. a slot that is free or holds another track: the old entry is closed
            if t_state == 0 or t_id != Z["id"][b, s]:
                old_bin = int(Z["bin"][b, s]) & 7
                for z in range(MAX_ZONES):
                    if (int(Z["inside"][b, s]) >> z) & 1:
                        Z["vanished"][b, z, old_bin] += 1
                        evs.append((VANISH, z, int(Z["id"][b, s]), -1, old_bin, f, f - int(Z["enter_frame"][b, z, s]), 0))
                Z["id"][b, s] = t_id if t_state else 0
                Z["has_prev"][b, s] = 0
                Z["inside"][b, s] = 0
            # 2. observed?
            bn = bin_of(t_label, class_bin)
            if t_state != TRACKED or int(table["last_frame"][b, s]) != f or bn == 255:
                continue
            px, py = anchor_point(table["filter"][b, :, s].astype(f32), anchor)
            if not (np.isfinite(px) and np.isfinite(py)):
                continue
            Z["bin"][b, s] = bn
            # 3. lines
            if Z["has_prev"][b, s]:
                prev = (Z["px"][b, s], Z["py"][b, s])
                for i in range(n_lines):
                    d = crossing(cfg["lines"][i], prev, (px, py))
                    if d is not None:
                        Z["line_count"][b, i, d, bn] += 1
                        evs.append((CROSS, i, t_id, lab32, bn, f, 0, d))
            # 4. zones: the zones at or beyond n_zones hold nobody
            old = int(Z["inside"][b, s])
            new = 0
            for z in range(n_zones):
                if inside(cfg["verts"][z], nv[z], px, py):
                    new |= 1 << z
            for z in range(MAX_ZONES):
                o, n = (old >> z) & 1, (new >> z) & 1
                if n and not o:
                    Z["entries"][b, z, bn] += 1
                    Z["enter_frame"][b, z, s] = f
                    evs.append((ENTER, z, t_id, lab32, bn, f, 0, 0))
                if o and not n:
                    dwell = f - int(Z["enter_frame"][b, z, s])
                    Z["exits"][b, z, bn] += 1
                    Z["dwell_sum"][b, z, bn] += dwell
                    Z["dwell_max"][b, z, bn] = max(int(Z["dwell_max"][b, z, bn]), dwell)
                    evs.append((EXIT, z, t_id, lab32, bn, f, dwell, 0))
                if n:
                    Z["occupancy"][b, z, bn] += 1
            Z["inside"][b, s] = new
            # 5.
            Z["px"][b, s], Z["py"][b, s], Z["has_prev"][b, s] = px, py, 1
        # 6. / 7. the first max_events in order; the excess is counted
        keep = min(len(evs), max_events)
        if keep:
            events[b, :keep] = np.asarray(evs[:keep], np.int64).astype(np.int32)
        counts[b] = keep
        Z["events_dropped"][b] += len(evs) - keep
    return Z, events, counts


# ---------------------------------------------------------------------------------------------------------- the scenes of the tests
# Lines and zones inside the 640-pixel field of track_ref.scene: tests/test_zones.py asserts on the CPU that every configuration below yields at
# least five events of every kind and crossings in both directions, so the GPU comparison (tests/test_gpu_zones.py) never compares empty lists.
SCENE_LINES = [(250, 0, 250, 640), (0, 330, 640, 330), (0, 0, 640, 640), (400, 100, 100, 500)]
SCENE_ZONES = [[(100, 100), (540, 100), (540, 540), (100, 540)],
               [(50, 50), (400, 50), (400, 250), (250, 250), (250, 450), (50, 450)],          # concave
               [(320, 150), (600, 600), (60, 600)],
               [(200, 280), (330, 280), (330, 420), (200, 420)]]
SCENE_BINS = [255, 0, 1, 255, 0]            # label -> bin: background and label 3 ignored, two bins
SCENE_SEED, SCENE_FRAMES, SCENE_STREAMS, SCENE_D, SCENE_TRACK_BUFFER = 200, 40, 3, 32, 3
# (max_tracks, anchor, class map)
SCENE_CASES = [(8, 1, None), (8, 0, SCENE_BINS), (256, 1, SCENE_BINS), (256, 0, None)]


def scene_frames():
    import track_ref
    return track_ref.scene(SCENE_SEED, SCENE_FRAMES, SCENE_STREAMS, SCENE_D, objects=8)[0]


def event_census(events, counts):
    """-> {"cross0": n, "cross1": n, "enter": n, "exit": n, "vanish": n} of one step's events."""
    out = dict(cross0=0, cross1=0, enter=0, exit=0, vanish=0)
    for b in range(events.shape[0]):
        for r in events[b, :counts[b]]:
            out[KINDS[int(r[0])] + (str(int(r[7])) if r[0] == CROSS else "")] += 1
    return out
