"""Line-crossing and zone analytics behind the tracker, on the GPU (demonet_amd/zones.py, csrc/zones.hip).

Every comparison of the device with tests/zones_ref.py is bit for bit: every field of the zone state, every event row and every count, after every
frame. The reference is driven from the DEVICE tracker's state of the frame, so a difference in the tracker cannot leak in (tests/test_track.py
holds the tracker to its own reference). tests/test_zones.py shows on the CPU that the scenes used here produce events of every kind.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import zones_ref as zr
from demonet_amd import _lib, models, synth
from demonet_amd import track as dtrack
from demonet_amd import zones as dzones

pytestmark = pytest.mark.gpu
f32 = np.float32
ANCHOR = {0: "center", 1: "bottom"}
W, H = 60.0, 80.0


def _dev(frame):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in frame]


def _host_table(tracker):
    return {k: v.cpu().numpy() for k, v in tracker.table().items()}


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _assert_step(want_state, want_ev, want_n, za, got, where):
    ev, n = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert _same(want_n, n), "{}: event counts {} want {}".format(where, n.tolist(), want_n.tolist())
    assert _same(want_ev, ev), "{}: events differ at {}\nwant {}\ngot  {}".format(where, np.argwhere(want_ev != ev)[:4].tolist(), want_ev[want_ev != ev][:16],
                                                                                  ev[want_ev != ev][:16])
    tab = za.table()
    for k in zr.FIELDS:
        w, g = want_state[k], tab[k].cpu().numpy()
        if k == "inside":
            g = g.view(np.uint32)
        assert _same(w, g), "{}: zone state field {} differs at {}".format(where, k, np.argwhere(w != g)[:8].tolist())


class Pair:
    """A device ZoneAnalytics and the reference's state side by side, with one configuration per stream."""

    def __init__(self, tracker, configs, anchor=1, bins=None, max_events=256):
        self.tracker, self.anchor, self.bins, self.max_events = tracker, anchor, bins, max_events
        self.za = dzones.ZoneAnalytics(tracker, anchor=ANCHOR[anchor], class_bins=bins, max_events=max_events)
        self.cfg = []
        for b, (lines, zones) in enumerate(configs):
            self.za.set_lines(b, lines)
            self.za.set_zones(b, zones)
            self.cfg.append(zr.config(lines, zones))
        self.st = zr.new_state(tracker.streams, tracker.max_tracks)

    def step(self, where):
        before = self.tracker.state.clone()
        got = self.za.update()
        self.st, ev, n = zr.step(_host_table(self.tracker), self.cfg, self.st, self.bins, self.anchor, self.max_events)
        _assert_step(self.st, ev, n, self.za, got, where)
        assert torch.equal(self.tracker.state, before), "{}: the tracker's state was written".format(where)
        return ev, n


# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(zr.SCENE_CASES)))
def test_scenes_bit_for_bit(case):
    T, anchor, bins = zr.SCENE_CASES[case]
    B = zr.SCENE_STREAMS
    tracker = dtrack.ByteTracker(B, "cuda", max_tracks=T, track_buffer=zr.SCENE_TRACK_BUFFER)
    pair = Pair(tracker, [(zr.SCENE_LINES, zr.SCENE_ZONES)] * B, anchor, bins)
    total = dict(cross0=0, cross1=0, enter=0, exit=0, vanish=0)
    for i, fr in enumerate(zr.scene_frames()):
        tracker.update(*_dev(fr))
        ev, n = pair.step("frame {}".format(i + 1))
        for k, v in zr.event_census(ev, n).items():
            total[k] += v
    print(zr.SCENE_CASES[case], total)
    assert all(v >= 5 for v in total.values()), total
    c = {k: v.cpu().numpy() for k, v in pair.za.counters().items()}
    assert c["line_count"].shape == (B, 16, 2, 8) and c["dwell_sum"].dtype == np.int64 and c["entries"].sum() == total["enter"]


# ----------------------------------------------------------------------------------------------------------------------------------
# crafted tracker states, written through state_fields
# ----------------------------------------------------------------------------------------------------------------------------------
def _write(tracker, frame, tracks):
    """tracks: per stream {slot: dict(id, cx, cy[, state, label, last_frame, w, h])} -> the tracker's device state of that frame."""
    tracker.state.zero_()
    tab = tracker.table()
    host = {k: np.zeros(tuple(v.shape), {torch.int32: np.int32, torch.int64: np.int64, torch.float32: np.float32}[v.dtype]) for k, v in tab.items()}
    host["frame"][:] = frame
    host["next_id"][:] = 1000
    for b, slots in enumerate(tracks):
        for s, k in slots.items():
            host["state"][b, s], host["id"][b, s], host["label"][b, s] = k.get("state", 2), k["id"], k.get("label", 1)
            host["last_frame"][b, s], host["start_frame"][b, s], host["score"][b, s] = k.get("last_frame", frame), 1, 0.9
            w, h = k.get("w", W), k.get("h", H)
            host["filter"][b, 0, s], host["filter"][b, 5, s], host["filter"][b, 10, s], host["filter"][b, 15, s] = k["cx"], k["cy"], f32(w) / f32(h), h
    for k, v in tab.items():
        v.copy_(torch.from_numpy(host[k]))


SQUARE = [(100, 100), (200, 100), (200, 200), (100, 200)]
BIG = [(0, 0), (400, 0), (400, 400), (0, 400)]
LINE = (100, 0, 100, 300)


def _rows(ev, n, b=0):
    return [tuple(int(v) for v in r) for r in ev[b, :n[b]]]


def test_a_slot_whose_id_changes_a_lost_track_found_again_a_tentative_track_and_a_mean_that_is_not_finite():
    tracker = dtrack.ByteTracker(2, "cuda", max_tracks=6)                    # (6: not a multiple of 4)
    pair = Pair(tracker, [([LINE], [SQUARE, BIG])] * 2, anchor=0)
    nan, inf = float("nan"), float("inf")
    seq = [
        [{0: dict(id=1, cx=80, cy=150), 5: dict(id=2, cx=150, cy=150, label=2)}, {1: dict(id=1, cx=80, cy=150), 2: dict(id=2, cx=150, cy=150, state=1)}],
        # stream 0: slot 0 now holds track 3 beyond the line, slot 5 is free. stream 1: track 1 is lost, the tentative track is confirmed
        [{0: dict(id=3, cx=150, cy=150, label=4)}, {1: dict(id=1, cx=85, cy=150, state=3, last_frame=1), 2: dict(id=2, cx=150, cy=150)}],
        # stream 0: track 3's mean is NaN, a new track with an infinite one. stream 1: track 1 found again on the other side of the line
        [{0: dict(id=3, cx=nan, cy=150, label=4), 3: dict(id=4, cx=150, cy=inf)}, {1: dict(id=1, cx=130, cy=150), 2: dict(id=2, cx=150, cy=150)}],
        [{0: dict(id=3, cx=90, cy=150, label=4), 3: dict(id=4, cx=150, cy=150, h=nan)}, {1: dict(id=1, cx=130, cy=150), 2: dict(id=2, cx=90, cy=150)}],
    ]
    out = []
    for i, tracks in enumerate(seq):
        _write(tracker, i + 1, tracks)
        out.append(pair.step("crafted frame {}".format(i + 1)))
    # what the frames were built to show (the reference's events, which the device has just been held to)
    assert _rows(*out[0], b=1) == [(zr.ENTER, 1, 1, 1, 0, 1, 0, 0)]                                             # the tentative track: ignored
    assert _rows(*out[1], b=0) == [(zr.VANISH, 1, 1, -1, 0, 2, 1, 0), (zr.ENTER, 0, 3, 4, 0, 2, 0, 0), (zr.ENTER, 1, 3, 4, 0, 2, 0, 0),
                                   (zr.VANISH, 0, 2, -1, 0, 2, 1, 0), (zr.VANISH, 1, 2, -1, 0, 2, 1, 0)]      # no CROSS from the old track's position
    assert _rows(*out[1], b=1) == [(zr.ENTER, 0, 2, 1, 0, 2, 0, 0), (zr.ENTER, 1, 2, 1, 0, 2, 0, 0)]            # the lost track: nothing
    assert _rows(*out[2], b=0) == []                                                                            # NaN and inf: not observed
    assert _rows(*out[2], b=1) == [(zr.CROSS, 0, 1, 1, 0, 3, 0, 1), (zr.ENTER, 0, 1, 1, 0, 3, 0, 0)]            # found again beyond the line: it counts
    assert _rows(*out[3], b=0) == [(zr.CROSS, 0, 3, 4, 0, 4, 0, 0), (zr.EXIT, 0, 3, 4, 0, 4, 2, 0)]             # from the anchor of frame 2
    assert pair.st["occupancy"][0, :2, 0].tolist() == [0, 1] and pair.st["line_count"][1, 0, :, 0].tolist() == [1, 1]


def _ring(cx, cy, r, n=16, phase=0.0):
    a = phase + 2 * np.pi * np.arange(n) / n
    return [(float(f32(cx + r * np.cos(t))), float(f32(cy + r * np.sin(t)))) for t in a]


@pytest.mark.parametrize("T", [7, 64, 253, 256])
def test_sixteen_lines_sixteen_zones_of_sixteen_vertices_and_more_events_than_rows(T):
    """Every limit at once, on table sizes around the wave size and not multiples of 4: tracks jump about the field, so every frame emits far more
    than max_events events for T >= 64 -- the first max_events in order are kept and events_dropped takes the excess."""
    rng = np.random.RandomState(T)
    B = 2
    lines = [tuple(float(v) for v in rng.uniform(0, 600, 4).astype(f32)) for _ in range(16)]
    zones = [_ring(rng.uniform(150, 450), rng.uniform(150, 450), rng.uniform(80, 250), 16, rng.uniform(0, 1)) for _ in range(15)]
    zones.append([(float(x), float(y)) for x, y in rng.uniform(0, 600, (16, 2)).astype(f32)])      # a self-intersecting one: even-odd all the same
    tracker = dtrack.ByteTracker(B, "cuda", max_tracks=T)
    max_events = 37 if T >= 64 else 1024
    pair = Pair(tracker, [(lines, zones), (lines[:3], zones[:2])], anchor=1, bins=[1, 0, 7, 255, 3], max_events=max_events)
    dropped = 0
    for fr in range(4):
        tracks = []
        for b in range(B):
            live = rng.permutation(T)[:max(1, (T * 3) // 4)]
            tracks.append({int(s): dict(id=int(s) + 1 + (100 if fr == 2 and s % 5 == 0 else 0), cx=float(rng.uniform(0, 600)), cy=float(rng.uniform(0, 600)),
                                        label=int(rng.randint(0, 6)), w=float(rng.uniform(20, 90)), h=float(rng.uniform(20, 90))) for s in live})
        _write(tracker, fr + 1, tracks)
        ev, n = pair.step("T={} frame {}".format(T, fr + 1))
        dropped = pair.st["events_dropped"].copy()
        assert n.max() <= max_events and not ev[0, n[0]:].any()
    if T >= 64:
        assert dropped[0] > 4 * max_events and pair.za.event_counts.cpu().numpy()[0] == max_events
    else:
        assert dropped.sum() == 0 and n[0] > 16
    assert pair.st["vanished"].sum() > 0 and pair.st["exits"].sum() > 0 and pair.st["line_count"][0].sum() > 0 and (pair.st["dwell_max"] > 0).any()


# ----------------------------------------------------------------------------------------------------------------------------------
def _scene_run(analytics_factory, frames, tracker_kw, between=None):
    tracker = dtrack.ByteTracker(zr.SCENE_STREAMS, "cuda", **tracker_kw)
    za = analytics_factory(tracker)
    outs = []
    for i, fr in enumerate(frames):
        if between is not None:
            between(i, tracker, za)
        tracker.update(*_dev(fr))
        ev, n = za.update()
        outs.append((ev.cpu().numpy().copy(), n.cpu().numpy().copy()))
    return tracker, za, outs


def _factory(tracker):
    return dzones.ZoneAnalytics(tracker, anchor="bottom", class_bins=zr.SCENE_BINS, max_events=64).set_all(zr.SCENE_LINES, zr.SCENE_ZONES)


def test_two_runs_give_the_same_bits_and_state_dict_resumes_a_run():
    frames = zr.scene_frames()[:16]
    kw = dict(max_tracks=16, track_buffer=3)
    ta, za, oa = _scene_run(_factory, frames, kw)
    tb, zb, ob = _scene_run(_factory, frames, kw)
    assert all(_same(x[0], y[0]) and _same(x[1], y[1]) for x, y in zip(oa, ob)) and torch.equal(za.state, zb.state) and torch.equal(za.config, zb.config)
    assert sum(int(x[1].sum()) for x in oa) > 20
    # resume from the middle of the run in fresh objects
    tc, zc, _ = _scene_run(_factory, frames[:8], kw)
    td = dtrack.ByteTracker(zr.SCENE_STREAMS, "cuda", **kw)
    zd = dzones.ZoneAnalytics(td, anchor="bottom", class_bins=zr.SCENE_BINS, max_events=64)
    td.load_state_dict(tc.state_dict())
    sd = zc.state_dict()
    assert sd["state"].device.type == "cpu" and sd["anchor"] == "bottom"
    zd.load_state_dict(sd)
    for fr, want in zip(frames[8:], oa[8:]):
        td.update(*_dev(fr))
        ev, n = zd.update()
        assert _same(want[0], ev.cpu().numpy()) and _same(want[1], n.cpu().numpy())
    assert torch.equal(zd.state, za.state)
    zd.set_lines(1, zr.SCENE_LINES[:1])                       # the host mirror came with the state: the zones of stream 1 stay
    assert torch.equal(zd.config[1, 260:2376].cpu(), za.config[1, 260:2376].cpu()) and int(zd.config[1, :4].view(torch.int32)) == 1
    with pytest.raises(ValueError):
        dzones.ZoneAnalytics(td, anchor="center", class_bins=zr.SCENE_BINS, max_events=64).load_state_dict(sd)
    with pytest.raises(ValueError):
        dzones.ZoneAnalytics(dtrack.ByteTracker(zr.SCENE_STREAMS, "cuda", max_tracks=8), class_bins=zr.SCENE_BINS).load_state_dict(sd)


def test_partial_reset_of_streams():
    frames = zr.scene_frames()[:14]
    B = zr.SCENE_STREAMS
    tracker = dtrack.ByteTracker(B, "cuda", max_tracks=16, track_buffer=3)
    pair = Pair(tracker, [(zr.SCENE_LINES, zr.SCENE_ZONES)] * B, anchor=1)
    for i, fr in enumerate(frames):
        if i == 8:
            assert pair.st["entries"][1].sum() > 0
            pair.za.reset([1])
            zr.reset(pair.st, [1])
        if i == 11:                                             # the tracker's stream restarts: its slots turn free, the analytics closes them
            tracker.reset([0])
        tracker.update(*_dev(fr))
        ev, n = pair.step("frame {}".format(i + 1))
        if i == 8:
            assert (ev[1, :n[1], 0] == zr.ENTER).all() and n[1] > 0 and pair.st["entries"][1].sum() == n[1]      # everybody enters anew
        if i == 11:
            assert (ev[0, :n[0], 0] == zr.VANISH).sum() > 0 and (ev[0, :n[0], 5] == 1).all()
    with pytest.raises(ValueError):
        pair.za.reset([B])
    pair.za.reset()
    torch.cuda.synchronize()
    assert not pair.za.state.any() and pair.za.config.any()


def test_a_captured_tracker_step_plus_analytics_step_replays_like_the_eager_run():
    frames = zr.scene_frames()[:10]
    edit = [(300, 0, 300, 640)]                                  # stream 1's lines from frame 5 on

    def between(i, tracker, za):
        if i == 5:
            za.set_lines(1, edit)
    _, eager, want = _scene_run(_factory, frames, dict(max_tracks=16, track_buffer=3), between)

    tracker = dtrack.ByteTracker(zr.SCENE_STREAMS, "cuda", max_tracks=16, track_buffer=3)
    za = _factory(tracker)
    static = _dev(frames[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tracker.update(*static)                                  # warm-up outside the capture: allocates the tracker's outputs
        za.update()
    torch.cuda.current_stream().wait_stream(side)
    tracker.reset()
    za.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tracker.update(*static)
        ev, n = za.update()
    tracker.reset()                                              # (the capture itself ran nothing)
    za.reset()
    for i, (fr, w) in enumerate(zip(frames, want)):
        between(i, tracker, za)                                  # the record is edited in place: the captured launch reads it where it lies
        for dst, src in zip(static, fr):
            dst.copy_(torch.from_numpy(np.ascontiguousarray(src)))
        graph.replay()
        assert _same(w[0], ev.cpu().numpy()) and _same(w[1], n.cpu().numpy()), "frame {}".format(i + 1)
    assert torch.equal(za.state, eager.state) and torch.equal(za.config, eager.config)
    assert sum(int(w[1][1]) for w in want[5:]) > 0


def test_refusals_each_with_its_error_code():
    tracker = dtrack.ByteTracker(2, "cuda", max_tracks=8)
    za = dzones.ZoneAnalytics(tracker, max_events=16).set_all([LINE], [SQUARE])
    _write(tracker, 1, [{0: dict(id=1, cx=150, cy=110)}, {}])
    za.update()
    for kw in (dict(anchor="top"), dict(max_events=0), dict(max_events=1025), dict(class_bins=[0, 8]), dict(class_bins=[]), dict(class_bins=[-1])):
        with pytest.raises(ValueError):
            dzones.ZoneAnalytics(tracker, **kw)
    for bad in (2, -1, "0", None):
        with pytest.raises(ValueError):
            za.set_lines(bad, [LINE])
    with pytest.raises(ValueError):
        za.set_zones(0, [SQUARE[:2]])
    other = dtrack.ByteTracker(2, "cuda", max_tracks=8)
    m = models.ssdlite320_mobilenet_v3_large(num_classes=3)
    with pytest.raises(ValueError):
        dzones.check_analytics(za, other, "track")               # bound to another tracker
    with pytest.raises(ValueError):
        m.track(torch.zeros(2, 3, 320, 320), other, analytics=za)
    with pytest.raises(ValueError):
        m.track(torch.zeros(2, 3, 320, 320), tracker, analytics=object())
    torch.cuda.synchronize()
    state_before, tstate_before, ev_before = za.state.clone(), tracker.state.clone(), za.events.clone()
    # the C entry points themselves
    L = _lib.lib()
    p = C.c_void_p
    bins = torch.zeros(4, dtype=torch.uint8, device="cuda")

    def call(track=tracker.state.data_ptr(), tbytes=tracker.state.numel(), streams=2, T=8, config=za.config.data_ptr(), cb=None, n_labels=0, anchor=1,
             z=za.state.data_ptr(), zbytes=za.state.numel(), ev=za.events.data_ptr(), n=za.event_counts.data_ptr(), max_events=16):
        return L.dn_zone_update(p(track), tbytes, streams, T, p(config), p(cb) if cb else None, n_labels, anchor, p(z), zbytes, p(ev), p(n), max_events, None)
    INVALID, WORKSPACE, UNSUPPORTED = -1, -3, -4
    assert call(T=257) == UNSUPPORTED and call(max_events=1025) == UNSUPPORTED
    for kw in (dict(track=0), dict(config=0), dict(z=0), dict(ev=0), dict(n=0), dict(streams=0), dict(T=0), dict(max_events=0), dict(anchor=2),
               dict(anchor=-1), dict(cb=bins.data_ptr(), n_labels=0), dict(track=tracker.state.data_ptr() + 4), dict(z=za.state.data_ptr() + 8),
               dict(config=za.config.data_ptr() + 4), dict(ev=za.events.data_ptr() + 4), dict(n=za.event_counts.data_ptr() + 2),
               dict(tbytes=tracker.state.numel() - 1), dict(T=9)):                                       # (T = 9: the tracker's state is too small for it)
        assert call(**kw) == INVALID, kw
        assert L.dn_last_error()
    assert call(zbytes=za.state.numel() - 1) == WORKSPACE and call(zbytes=16) == WORKSPACE
    assert L.dn_zone_reset(None, 2, 8, None, None) == INVALID and L.dn_zone_reset(p(za.state.data_ptr()), 0, 8, None, None) == INVALID
    assert L.dn_zone_reset(p(za.state.data_ptr() + 4), 2, 8, None, None) == INVALID and L.dn_zone_reset(p(za.state.data_ptr()), 2, 257, None, None) == UNSUPPORTED
    assert L.dn_zone_state_bytes(2, 257) == 0 and L.dn_zone_state_bytes(0, 8) == 0
    torch.cuda.synchronize()
    assert torch.equal(za.state, state_before) and torch.equal(tracker.state, tstate_before) and torch.equal(za.events, ev_before)      # nothing was launched
    assert call(cb=bins.data_ptr(), n_labels=4) == 0 and call() == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------------------
# model level
# ----------------------------------------------------------------------------------------------------------------------------------
def test_ssd_track_without_analytics_is_todays_call_and_with_it_gains_the_events_pair():
    model = models.load_synthetic(models.ssdlite320_mobilenet_v3_large(num_classes=21, score_thresh=0.4), 0).cuda().eval()
    base = torch.from_numpy(synth.images(2024, 2, 300, 420)).cuda()
    video = [torch.roll(base, shifts=3 * f, dims=3).contiguous() for f in range(3)]
    plain, none, with_za = (dtrack.ByteTracker(2, "cuda", max_tracks=64) for _ in range(3))
    za = dzones.ZoneAnalytics(with_za, anchor="center").set_all([(210, 0, 210, 300)], [[(0, 0), (420, 0), (420, 300), (0, 300)]])
    st = zr.new_state(2, 64)
    cfg = [zr.config([(210, 0, 210, 300)], [[(0, 0), (420, 0), (420, 300), (0, 300)]])] * 2
    events = 0
    for i, imgs in enumerate(video):
        want = [t.cpu().numpy().copy() for t in plain.update(*model.forward_batch(imgs))]
        got = model.track(imgs, none, analytics=None)
        assert len(got) == 7 and all(_same(w, g.cpu().numpy()) for w, g in zip(want, got))
        got = model.track(imgs, with_za, analytics=za)
        assert len(got) == 8 and all(_same(w, g.cpu().numpy()) for w, g in zip(want, got[:7]))
        st, ev, n = zr.step(_host_table(with_za), cfg, st, None, 0, 256)
        _assert_step(st, ev, n, za, got[7], "frame {}".format(i + 1))
        events += int(n.sum())
    assert torch.equal(plain.state, none.state) and torch.equal(plain.state, with_za.state)
    print("events over the sequence:", events)
    assert events > 0
