"""dev tool: what the analytics step behind the tracker costs on 64 streams, and what it replaces.
    python tools/time_zones.py [--out profiles/zones_timing.json] [--rounds 5] [--host-frames 2] [--streams 64] [--parent-tree PATH]
64 streams, about 100 live tracks per stream (tests/track_ref.scene as in tools/time_track.py: 112 moving objects in 160 rows, 256 slots, ByteTrack's
default thresholds), 4 lines and 4 zones per stream, the bottom-centre anchor, a class map with two bins. The tracker and the analytics are warmed
up over 10 frames; every round restarts from that state and steps through the next 50 frames. Rounds are alternated; medians with min and max:
  track_parent_us   one dn_track_update launch per step with the PARENT commit's tree and library (--parent-tree: a checkout of the parent with its
                    library built; a child process of this tool that imports that tree). Without --parent-tree the entry is null.
  track_us          the same launch with this tree, measured by the same child code
  track_zones_us    dn_track_update + dn_zone_update behind it on the same stream, per step (this process)
  zones_alone_us    dn_zone_update alone on the recorded tracker states of the 50 frames (this process)
  host_ms           what a user composes without this feature, per step: the tracker step, its table copied to the host, tests/zones_ref.step
                    for all streams (host clock, --host-frames steps)
The device analytics and the reference are compared bit for bit over the warm-up and the first 10 timed frames before any time is taken. One JSON
document on stdout (and in --out)."""
import argparse
import copy
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, STEPS, D, CHECKED, OBJECTS, SIZE = 10, 50, 160, 10, 112, 2000.0
LINES = [(1000, 0, 1000, 2100), (0, 1000, 2100, 1000), (0, 0, 2000, 2000), (1500, 200, 300, 1800)]
ZONES = [[(300, 300), (1700, 300), (1700, 1700), (300, 1700)],
         [(100, 100), (1300, 100), (1300, 800), (800, 800), (800, 1500), (100, 1500)],
         [(1000, 400), (1900, 1900), (150, 1900)],
         [(700, 800), (1200, 800), (1200, 1400), (700, 1400)]]
BINS = [255, 0, 1, 0, 1]


def _scene(streams):
    sys.path.insert(0, os.path.join(ROOT, "tests"))      # (the scene generator is the same file in both trees)
    import track_ref as tr
    return tr.scene(64, WARM + STEPS, streams, D, objects=OBJECTS, size=SIZE, false_positives=5, exits=False)[0]


def _events_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def child(tree, streams):
    """The tracker step alone with the package of `tree`: answers every line on stdin with one round's microseconds per step."""
    sys.path.insert(0, tree)
    import torch
    from demonet_amd import _lib
    from demonet_amd.track import ByteTracker
    assert os.path.abspath(_lib.LIB_PATH).startswith(os.path.abspath(tree)), _lib.LIB_PATH
    frames = [[torch.from_numpy(x).cuda() for x in fr] for fr in _scene(streams)]
    tracker = ByteTracker(streams, "cuda")
    for fr in frames[:WARM]:
        tracker.update(*fr)
    warm = tracker.state_dict()

    def steps():
        for fr in frames[WARM:]:
            tracker.update(*fr)
    steps()
    print("ready", flush=True)
    for _ in sys.stdin:
        tracker.load_state_dict(warm)
        print(_events_ms(torch, steps) * 1e3 / STEPS, flush=True)


class Child:
    def __init__(self, tree, streams):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--role", "child", "--tree", tree, "--streams", str(streams)],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=tree)
        line = self.p.stdout.readline().strip()
        if line != "ready":
            raise RuntimeError("the child for {} did not start: {!r}".format(tree, line))

    def round(self):
        self.p.stdin.write("go\n")
        self.p.stdin.flush()
        return float(self.p.stdout.readline())

    def close(self):
        self.p.stdin.close()
        self.p.wait(timeout=60)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=2)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--role", default="main")
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    if a.role == "child":
        return child(os.path.abspath(a.tree), a.streams)
    sys.path.insert(0, ROOT)
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from demonet_amd.track import ByteTracker
    from demonet_amd.zones import ZoneAnalytics
    frames = _scene(a.streams)
    import zones_ref as zr
    B = a.streams
    dev_frames = [[torch.from_numpy(x).cuda() for x in fr] for fr in frames]
    tracker = ByteTracker(B, "cuda")
    za = ZoneAnalytics(tracker, anchor="bottom", class_bins=BINS, max_events=256).set_all(LINES, ZONES)
    cfg = [zr.config(LINES, ZONES)] * B
    st = zr.new_state(B, 256)

    # agreement first: the warm-up and the first CHECKED timed frames; the tracker's states of the timed frames are recorded on the way
    same, census, recorded = True, dict(cross0=0, cross1=0, enter=0, exit=0, vanish=0), []
    for i, dfr in enumerate(dev_frames):
        if i == WARM:
            warm_t, warm_z, warm_ref = tracker.state_dict(), za.state_dict(), copy.deepcopy(st)
        tracker.update(*dfr)
        ev, n = za.update()
        if i >= WARM:
            recorded.append(tracker.state.clone())
        if i < WARM + CHECKED:
            st, rev, rn = zr.step({k: v.cpu().numpy() for k, v in tracker.table().items()}, cfg, st, BINS, 1, 256)
            tab = za.table()
            same = same and rev.tobytes() == ev.cpu().numpy().tobytes() and rn.tobytes() == n.cpu().numpy().tobytes()
            same = same and all(np.ascontiguousarray(st[k]).tobytes() == tab[k].cpu().numpy().tobytes() for k in zr.FIELDS)
            for k, v in zr.event_census(rev, rn).items():
                census[k] += v
    live = int((tracker.table()["state"] != 0).sum().item())
    counters = {k: int(v.sum().item()) for k, v in za.counters().items()}

    def both():
        for dfr in dev_frames[WARM:]:
            tracker.update(*dfr)
            za.update()

    stand_ins = []
    for s in recorded:                       # one stand-in tracker per recorded state: the analytics reads `tracker.state` where it lies
        t = copy.copy(tracker)
        t.state = s
        stand_ins.append(t)

    def zones_alone():
        for t in stand_ins:
            za.tracker = t
            za.update()
        za.tracker = tracker

    def host():
        r = copy.deepcopy(warm_ref)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for dfr in dev_frames[WARM:WARM + a.host_frames]:
            tracker.update(*dfr)
            r = zr.step({k: v.cpu().numpy() for k, v in tracker.table().items()}, cfg, r, BINS, 1, 256)[0]
        return (time.perf_counter() - t0) * 1e3 / a.host_frames

    here = Child(ROOT, B)
    parent = Child(os.path.abspath(a.parent_tree), B) if a.parent_tree else None
    times = dict(track_parent_us=[], track_us=[], track_zones_us=[], zones_alone_us=[], host_ms=[])
    try:
        for _ in range(a.rounds):
            if parent is not None:
                times["track_parent_us"].append(parent.round())
            times["track_us"].append(here.round())
            tracker.load_state_dict(warm_t)
            za.load_state_dict(warm_z)
            times["track_zones_us"].append(_events_ms(torch, both) * 1e3 / STEPS)
            za.load_state_dict(warm_z)
            times["zones_alone_us"].append(_events_ms(torch, zones_alone) * 1e3 / STEPS)
            tracker.load_state_dict(warm_t)
            times["host_ms"].append(host())
    finally:
        here.close()
        if parent is not None:
            parent.close()
    stat = lambda f: {k: (round(f(v), 3) if v else None) for k, v in times.items()}      # noqa: E731
    doc = dict(streams=B, rows=D, slots=256, lines=len(LINES), zones=len(ZONES), class_bins=BINS, anchor="bottom", live_tracks_at_the_end=live,
               live_tracks_per_stream=round(live / B, 1), device_equals_reference=bool(same), frames_compared=WARM + CHECKED,
               events_in_the_compared_frames=census, counters_after_all_frames=counters, warm_frames=WARM, steps=STEPS, rounds=a.rounds,
               host_frames=a.host_frames, parent_tree=bool(a.parent_tree), device=torch.cuda.get_device_name(0), median=stat(statistics.median),
               min=stat(min), max=stat(max))
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
