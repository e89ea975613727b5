"""Authoring-time tool: the per-conv multipliers of tests/trained_like.py (tests/golden/trained_like_calib.json).

Walks the op IR with oracle/op_ref.py (fp16-rounded weights) on synth.images(11, 1, H, W), the "spread" edits applied and no multipliers
yet. At every conv it sets one scalar so that
  a conv followed by BN     has median over the live channels of std(conv output) / sqrt(running_var + eps) equal to 1: the statistics a
                            trained BN would hold;
  a VGG conv (no BN)        has an output rms of 32 before the bias;
  a head's last conv        has the output std the graph builder intended (Param.target).
Then prints the figures of the regime conditions (trained_like.measure). The result is a small table of floats, committed as data.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from demonet_amd import spec, synth  # noqa: E402
import op_ref  # noqa: E402
import trained_like  # noqa: E402

MODELS = {"ssdlite320_mobilenet_v3_large": 91, "ssd_lite_mobilenet_v2": 21, "ssd300_vgg16": 91, "ssd512_vgg16": 91}
VGG_RMS = 32.0


def calibrate(name):
    g = spec.GRAPHS[name](num_classes=MODELS[name])
    sd = trained_like.state_dict(g, "spread", 0, calib={})
    target = {p.key[:-len(".weight")]: p.target for p in g.params if p.kind == "conv_w"}
    ref = op_ref.OpRef(g, sd, bound=False, round_se=False)
    W, H = g.size
    val = {g.nodes[0].inp: op_ref.stem_input(g, torch.from_numpy(synth.images(11, 1, H, W)))}
    mult = {}
    for i, nd in enumerate(g.nodes):
        if nd.op in ("stem", "pw", "dw", "conv"):
            x = val[nd.inp]
            if nd.op == "pw" and nd.se >= 0:
                x = x * val[nd.se][:, :, None, None]
            z = ref._conv(nd, x, ref.w[i][0]).double()              # the folded conv without its bias
            if nd.bn_key:
                s = torch.from_numpy(sd[nd.bn_key + ".weight"].astype(np.float64) /
                                     np.sqrt(sd[nd.bn_key + ".running_var"].astype(np.float64) + nd.bn_eps))
                live = torch.from_numpy(sd[nd.bn_key + ".running_var"] > 1e-6)
                u = z / s.view(1, -1, 1, 1)                           # conv output / sqrt(var + eps)
                n_el = u.shape[0] * u.shape[2] * u.shape[3]
                d = u.std(dim=(0, 2, 3), unbiased=False)
                # (maps of a few pixels: the second moment over all live channels stands in for the per-channel deviation)
                m = 1.0 / float(d[live].median() if n_el >= 8 else (u[:, live] ** 2).mean().sqrt())
            elif nd.head:
                m = float(np.sqrt(target[nd.conv_key])) / float(z.std(unbiased=False))
            else:
                m = VGG_RMS / float((z ** 2).mean().sqrt())
            m = round(m, 5)
            mult[nd.conv_key] = m
            sd[nd.conv_key + ".weight"] = (sd[nd.conv_key + ".weight"].astype(np.float64) * m).astype(np.float32)
            w, b = op_ref.folded(nd, sd)
            ref.w[i] = (w, b, w.abs(), b.abs())
        y, _ = ref.op(nd, val)
        if nd.head and nd.op in ("pw", "conv"):
            continue
        if nd.op == "dw" and nd.pool >= 0:
            val[nd.pool] = op_ref.pool_sum(y)[0]
        val[nd.out] = y
    return mult


def report(name, table):
    g = spec.GRAPHS[name](num_classes=MODELS[name])
    for regime in trained_like.REGIMES:
        m = trained_like.measure(g, trained_like.state_dict(g, regime, 0, calib=table))
        print(name, regime, {k: v for k, v in m.items() if k not in ("subnormal", "const")})
        for k, v in trained_like.conditions(m, regime == "hot_heads").items():
            print("    %-70s %s" % (k, "holds" if v else "FAILS"))


if __name__ == "__main__":
    torch.set_num_threads(8)
    which = sys.argv[1:] or list(MODELS)
    table = json.load(open(trained_like.CALIB_PATH)) if os.path.exists(trained_like.CALIB_PATH) else {}
    with torch.no_grad():
        for name in which:
            table[name] = calibrate(name)
            report(name, table[name])
    json.dump(table, open(trained_like.CALIB_PATH, "w"), indent=0, sort_keys=True)
    print("wrote", trained_like.CALIB_PATH)
