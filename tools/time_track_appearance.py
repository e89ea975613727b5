"""dev tool: what the tracker's appearance step costs, beside the plain tracker launch and beside what a user composes without it.
    python tools/time_track_appearance.py [--out profiles/track_appearance_timing.json] [--rounds 5] [--host-frames 2] [--streams 64]
The workload of tools/time_track.py (64 streams, about 100 detections per stream and frame in 160 rows, 256 slots, ByteTrack's thresholds) with
embeddings of dimension 256 for the HIGH rows (score >= track_thresh) in a table of 8192 slots, as an ObjectCropper of that capacity hands them
on: every object has a fixed random direction, a row shows it with noise, the other HIGH rows get random vectors.
Both trackers are warmed up over 10 frames; every round restarts from that state and steps through the next 50 frames. The measurements of a
round alternate; median (min - max) over the rounds, device events around the 50 steps divided by 50:
  appearance_us       AppearanceTracker.update with embeddings: the fill, the norms, the similarity, the step (four graph nodes)
  appearance_none_us  AppearanceTracker.update without embeddings: the step alone
  update_us           ByteTracker.update (dn_track_update) on the same detections, the same library: the tracker launch this step extends
  torch_sim_us        what a user composes today for the similarity alone: F.normalize of the table, a gather into [B, d, dim], F.normalize of
                      the features kept as a torch tensor, torch.bmm in fp16 -> S [B, 256, d] fp32
  today_ms            torch_sim + the copy of S and of the detections to the host + tests/track_appearance_ref.AppRefTracker.update given S (host
                      clock, --host-frames frames)
Before any time is taken the device is compared with the teacher-forced reference over the warm-up frames (bit for bit). One JSON document on
stdout (and in --out)."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import track_appearance_ref as ar  # noqa: E402
import track_ref as tr  # noqa: E402
from demonet_amd.track import AppearanceTracker, ByteTracker  # noqa: E402

WARM, STEPS, D, DIM, E, T = 10, 50, 160, 256, 8192, 256


def _events_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def embeddings(frames, truth, seed):
    """per frame (emb [E, DIM] f32, index [E, 8] i32): the HIGH rows, in (stream, row) order as a cropper numbers them."""
    rng = np.random.RandomState(seed)
    base = {}
    out = []
    for fr, per_stream in zip(frames, truth):
        emb = np.zeros((E, DIM), np.float32)
        index = np.zeros((E, 8), np.int32)
        index[:, 0] = -1
        e = 0
        for b, t in enumerate(per_stream):
            for j in range(int(fr[3][b])):
                if not (fr[1][b, j] >= 0.5) or e >= E:
                    continue
                if j in t:
                    if (b, t[j]) not in base:
                        v = rng.normal(0, 1, DIM)
                        base[(b, t[j])] = v / np.linalg.norm(v)
                    emb[e] = base[(b, t[j])] + rng.normal(0, 0.05 / np.sqrt(DIM), DIM)
                else:
                    emb[e] = rng.normal(0, 1, DIM)
                index[e, :2] = (b, j)
                e += 1
        out.append((emb, index, e))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=2)
    ap.add_argument("--streams", type=int, default=64)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    B = a.streams
    frames, truth = tr.scene(64, WARM + STEPS, B, D, objects=112, size=2000.0, false_positives=5, exits=False)
    embs = embeddings(frames, truth, 65)
    dev_frames = [[torch.from_numpy(x).cuda() for x in fr] for fr in frames]
    dev_embs = [(torch.from_numpy(e).cuda(), torch.from_numpy(i).cuda()) for e, i, _ in embs]
    app, none, plain = AppearanceTracker(B, "cuda", DIM), AppearanceTracker(B, "cuda", DIM), ByteTracker(B, "cuda")
    ref = ar.AppRefTracker(B, DIM, max_tracks=T)

    same = True
    for i in range(WARM):
        got = [t.cpu().numpy() for t in app.update(*dev_frames[i], *dev_embs[i])]
        none.update(*dev_frames[i])
        plain.update(*dev_frames[i])
        want = ref.update(*frames[i], emb=embs[i][0], index=embs[i][1], S=app.similarity().cpu().numpy(), en=app.normalised().cpu().numpy())
        same = same and all(x.tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(want, got))
        same = same and bool(np.array_equal(app.features()[0].cpu().numpy() != 0, ref.fvalid))
    warm = dict(app=app.state_dict(), none=none.state_dict(), plain=plain.state_dict())
    warm_ref = copy.deepcopy(ref)
    live = int((app.table()["state"] != 0).sum().item()) / B
    with_feature = int(app.features()[0].sum().item()) / B

    feat_t = app.features()[1].clone()                       # the composition keeps its features as a torch tensor [B, T, DIM]

    def torch_sim(k):
        emb, index = dev_embs[k]
        en = F.normalize(emb, dim=1).half()
        rows = torch.zeros((B, D, DIM), dtype=torch.float16, device="cuda")
        ok = index[:, 0] >= 0
        rows[index[ok, 0].long(), index[ok, 1].long()] = en[ok]
        return torch.bmm(F.normalize(feat_t, dim=2).half(), rows.transpose(1, 2)).float()

    def run(tracker, with_emb):
        for k in range(WARM, WARM + STEPS):
            if with_emb:
                tracker.update(*dev_frames[k], *dev_embs[k])
            else:
                tracker.update(*dev_frames[k])

    def sims():
        for k in range(WARM, WARM + STEPS):
            torch_sim(k)

    def today():
        r = copy.deepcopy(warm_ref)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(WARM, WARM + a.host_frames):
            S = torch_sim(k).cpu().numpy()
            host = [t.cpu().numpy() for t in dev_frames[k]]
            r.update(*host, emb=embs[k][0], index=embs[k][1], S=S)
        return (time.perf_counter() - t0) * 1e3 / a.host_frames

    for _ in range(2):
        sims()
    times = dict(appearance_us=[], appearance_none_us=[], update_us=[], torch_sim_us=[], today_ms=[])
    for _ in range(a.rounds):
        app.load_state_dict(warm["app"])
        times["appearance_us"].append(_events_ms(lambda: run(app, True)) * 1e3 / STEPS)
        plain.load_state_dict(warm["plain"])
        times["update_us"].append(_events_ms(lambda: run(plain, False)) * 1e3 / STEPS)
        none.load_state_dict(warm["none"])
        times["appearance_none_us"].append(_events_ms(lambda: run(none, False)) * 1e3 / STEPS)
        times["torch_sim_us"].append(_events_ms(sims) * 1e3 / STEPS)
        times["today_ms"].append(today())
    med = {k: round(statistics.median(v), 3) for k, v in times.items()}
    tp = (T + 3) & ~3
    doc = dict(streams=B, rows=D, slots=T, dim=DIM, table_slots=E, embeddings_per_frame=round(float(np.mean([n for _, _, n in embs])), 1),
               detections_per_stream_and_frame=round(float(np.mean([f[3].mean() for f in frames])), 1), live_tracks_per_stream_after_warmup=live,
               tracks_with_a_feature_per_stream_after_warmup=with_feature, device_equals_teacher_forced_reference=bool(same), frames_compared=WARM,
               warm_frames=WARM, steps=STEPS, rounds=a.rounds, host_frames=a.host_frames, device=torch.cuda.get_device_name(0),
               S_bytes_written_per_step=B * tp * D * 4, en_bytes_written_per_step=E * DIM * 2, feature_bytes_read_per_similarity=B * tp * DIM * 4,
               median=med, min={k: round(min(v), 3) for k, v in times.items()}, max={k: round(max(v), 3) for k, v in times.items()})
    doc["appearance_over_update"] = round(med["appearance_us"] / med["update_us"], 3)
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
