"""dev tool: timings of large class vocabularies (K above 256 foreground classes: the wide softmax / decode kernel and the wide merge).
    python tools/time_large_vocab.py [--out FILE] [--reps R]
Per configuration -- ssdlite320_mobilenet_v3_large at batch 64 with K in {91, 366, 1204}, ssd300_vgg16 at batch 64 with K = 1204 --:
  * forward_batch one at a time (device events around R forwards, graph replay),
  * three forwards in flight through ForwardPipeline (depth 3, one chain each),
  * dn_postprocess alone on the device's own head outputs (R calls),
  * the wide kernel's algorithmic bytes from the shapes: logits read once, scores written once (class-major), regressions + anchors read,
    boxes written. Its kernel time comes from a separate `rocprofv3 --kernel-trace --stats` run (softmax_decode_wide_kernel).
One JSON line per configuration on stdout (and in --out)."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from demonet_amd import _lib, models, synth  # noqa: E402
from demonet_amd.pipeline import ForwardPipeline  # noqa: E402

CONFIGS = [("ssdlite320_mobilenet_v3_large", 91, 64), ("ssdlite320_mobilenet_v3_large", 366, 64),
           ("ssdlite320_mobilenet_v3_large", 1204, 64), ("ssd300_vgg16", 1204, 64)]


def _events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def wide_bytes(n, A, K):
    # logits [n][A][K] read once, scores [n][K-1][A] written, regressions [n][A][4] + anchors [A][4] read, boxes [n][A][4] written (fp32)
    return 4 * (n * A * K + n * (K - 1) * A + n * A * 4 + A * 4 + n * A * 4)


def run(name, K, n, reps):
    m = getattr(models, name)(num_classes=K)
    models.load_synthetic(m, 0)
    m.cuda()
    size = m.graph.size
    imgs = torch.from_numpy(synth.images(64, n, size[1], size[0])).cuda()
    try:
        for _ in range(3):
            m.forward_batch(imgs, persistent_input=True)
        torch.cuda.synchronize()
        fwd_ms = _events_ms(lambda: m.forward_batch(imgs, persistent_input=True), reps)
        with ForwardPipeline(m, n, depth=3) as pipe:
            for _ in range(3):
                pipe.result(pipe.submit(imgs, persistent_input=True))
            torch.cuda.synchronize()
            tickets = []

            def one():
                tickets.append(pipe.submit(imgs, persistent_input=True))
            pipe_ms = _events_ms(one, reps * 3)
            for t in tickets[-3:]:
                pipe.result(t)
        torch.cuda.synchronize()
        logits, reg = m.forward_heads(imgs)
        A = logits.shape[1]
        p = m.graph.post
        anchors = torch.from_numpy(m._lowered.anchors).cuda()
        L = _lib.lib()
        topk, dets = p["topk_candidates"], p["detections_per_img"]
        ws = torch.empty(L.dn_postprocess_workspace_bytes(n, A, K, topk, dets), dtype=torch.uint8, device="cuda")
        boxes = torch.empty(n, dets, 4, device="cuda")
        scores = torch.empty(n, dets, device="cuda")
        labels = torch.empty(n, dets, dtype=torch.int64, device="cuda")
        counts = torch.empty(n, dtype=torch.int32, device="cuda")
        P = lambda t: C.c_void_p(t.data_ptr())
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        call = lambda: _lib.check(L.dn_postprocess(P(logits), P(reg), P(anchors), n, A, K, float(size[1]), float(size[0]), None,
                                                   float(p["score_thresh"]), float(p["nms_thresh"]), topk, dets, P(boxes), P(scores), P(labels),
                                                   P(counts), None, P(ws), ws.numel(), s), "dn_postprocess")
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        post_ms = _events_ms(call, reps)
        del logits, reg, ws
    finally:
        m.release()
    return dict(model=name, num_classes=K, batch=n, anchors=A, forward_ms=round(fwd_ms, 3), forward_img_per_s=round(n / fwd_ms * 1e3, 1),
                pipeline3_ms_per_batch=round(pipe_ms, 3), pipeline3_img_per_s=round(n / pipe_ms * 1e3, 1), postprocess_ms=round(post_ms, 3),
                wide_kernel=K - 1 > 256, softmax_alg_bytes=wide_bytes(n, A, K))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    rows = []
    for name, K, n in CONFIGS:
        r = run(name, K, n, a.reps)
        print(json.dumps(r), flush=True)
        rows.append(r)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
