"""dev tool (CPU only): where does the fp16 path's logit error come from?  Evaluates the op IR in torch with the device's rounding points
emulated -- BN folded into fp16 weights, every activation tensor rounded to fp16 where the kernels store it, the SE product rounded to
fp16 (it is an MFMA operand), fp32 accumulation -- and switches single rounding sources off:

    python tools/emulate_fp16.py [model]

    all-fp16         what the kernels do (should land near the measured device error, profiles/r0x_layer_errors.txt)
    res-fp32         the residual-stream tensors (block outputs: linear projections) kept in fp32
    w-fp32           weights not rounded to fp16
    exp-fp32         expanded / depthwise tensors kept in fp32 (everything but the residual stream)
The reference is the same IR in fp32 (oracle/op_ref.py, pinned to the reference's head outputs by tests/test_op_ref.py)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from demonet_amd import models, synth  # noqa: E402

import op_ref  # noqa: E402  (oracle/op_ref.py: the op IR evaluator, its weight fold and rounding points)


def run(name, mode, imgs, g, sd):
    is_res = set()                      # residual-stream tensors: outputs of backbone projections (pw, act none, not head)
    for nd in g.nodes:
        if nd.op == "pw" and nd.act == 0 and not nd.head:
            is_res.add(nd.out)

    def store(nd, y):
        if mode == "fp32" or nd.op == "maxpool":
            return y
        if mode == "res-fp32" and nd.out in is_res:
            return y
        if mode == "exp-fp32" and nd.out not in is_res:
            return y
        return op_ref.h16(y)

    # weights (SE FCs included) fp16 unless fp32 / w-fp32; the stem always runs on fp32 weights; the SE product is an fp16 MFMA operand
    return op_ref.chain(g, sd, imgs, round_w=mode not in ("fp32", "w-fp32"), round_se=mode != "fp32", store=store)


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "ssdlite320_mobilenet_v3_large"
    ncls = 21 if name == "ssd_lite_mobilenet_v2" else 91
    m = getattr(models, name)(num_classes=ncls)
    g = m.graph
    sd = {k: torch.from_numpy(v.copy()) for k, v in synth.state_dict(g, 0).items()}
    W, H = g.size
    imgs = torch.from_numpy(synth.images(1, 2, H, W))
    torch.set_num_threads(8)
    with torch.no_grad():
        ref_l, ref_r, ref_v = run(name, "fp32", imgs, g, sd)
        print(f"{name}: max|logit| {ref_l.abs().max():.2f}")
        for mode in ("all-fp16", "res-fp32", "w-fp32", "exp-fp32"):
            l, r, v = run(name, mode, imgs, g, sd)
            d = (l - ref_l).abs()
            dr = (r - ref_r).abs()
            last = [nd.out for nd in g.nodes if not nd.head and nd.out in v and nd.out in ref_v and v[nd.out].dim() == 4][-12]
            print(f"  {mode:9s} logits max {d.max():.4f} mean {d.mean():.5f}   regression max {dr.max():.4f} mean {dr.mean():.5f}")


if __name__ == "__main__":
    main()
