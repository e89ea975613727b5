"""CPU tests (-m "not gpu") of oracle/op_ref.py, the fp32 reference and error bound that tests/test_gpu_launch_parity.py holds every
kernel launch to: the fp32 chain equals the reference's head outputs, and the bound passes what a correct kernel may do while it fails
the defects kernels have had or risk (each mutant below is a CPU emulation of a kernel with that one defect)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import op_ref
import ssd_oracle as so
from demonet_amd import spec, synth

V3 = "ssdlite320_mobilenet_v3_large"


def _golden_images(g, seeds):
    W, H = g.size
    return torch.from_numpy(np.stack([synth.images(int(s), 1, H, W)[0] for s in seeds]))


@pytest.mark.parametrize("name", [V3, "ssd_lite_mobilenet_v2", "ssd300_vgg16", "ssd512_vgg16"])
def test_fp32_chain_matches_golden(golden_dir, name):
    """the op IR in fp32 (op_ref, weights folded there) against the reference's recorded head outputs and features, at
    test_oracle.py's tolerances"""
    if name == "ssd512_vgg16" and not os.environ.get("DEMONET_SLOW"):
        pytest.skip("100 GMAC/img on CPU; set DEMONET_SLOW=1")
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    g = spec.GRAPHS[name](num_classes=int(z["num_classes"]))
    sd = synth.state_dict(g, int(z["weight_seed"]))
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    with torch.no_grad():
        lg, rg, val = op_ref.chain(g, sd, _golden_images(g, z["image_seeds"]))
    np.testing.assert_allclose(rg.numpy(), z["bbox_regression"], rtol=1e-4, atol=2e-4)
    for i in range(int(z["n_images"])):
        if f"cls_logits_full_{i}" in z:
            np.testing.assert_allclose(lg[i].numpy(), z[f"cls_logits_full_{i}"], rtol=1e-4, atol=2e-4)
        np.testing.assert_allclose(lg[i].numpy()[::7], z[f"cls_logits_rows_{i}"], rtol=1e-4, atol=2e-4)
    for lvl, f in enumerate(g.features):
        fn = val[f].numpy()
        assert tuple(fn.shape) == tuple(z[f"feat{lvl}_shape"])
        samp = fn.reshape(fn.shape[0], -1)[:, ::max(1, fn[0].size // 4096)]
        np.testing.assert_allclose(samp, z[f"feat{lvl}_sample"], rtol=1e-4, atol=2e-4)


def _v2_chain_against_the_oracle(size):
    g = spec.ssd_lite_mobilenet_v2_graph(image_size=size, num_classes=21)
    sd = synth.state_dict(g, 0)
    imgs = torch.from_numpy(synth.images(3, 2, size, size))
    with torch.no_grad():
        lg, rg, _ = op_ref.chain(g, sd, imgs)
    raw = so.OracleSSD("ssd_lite_mobilenet_v2", sd, 21, size=(size, size)).forward_raw(list(imgs))
    np.testing.assert_allclose(lg.numpy(), raw["cls_logits"].numpy(), rtol=1e-4, atol=2e-4)
    np.testing.assert_allclose(rg.numpy(), raw["bbox_regression"].numpy(), rtol=1e-4, atol=2e-4)


def test_fp32_chain_matches_oracle_v2_at_300():
    """BASELINE config C3: the V2 hub model at 300 x 300 (ragged maps down the pyramid) against the oracle"""
    _v2_chain_against_the_oracle(300)


@pytest.mark.parametrize("size", [160, 301])
def test_fp32_chain_matches_oracle_v2_at_other_sizes(size):
    """160: a 5 x 5 second level, the smallest network tests/test_gpu_launch_parity.py runs; 301: an odd input, 151 -> 76 -> 38 -> 19"""
    _v2_chain_against_the_oracle(size)


# ---- sensitivity: emulated kernels through the same comparator -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def v3():
    """the V3 graph, its synthetic weights, and device-like inputs for every tensor: the fp16 emulation of the chain on two images"""
    g = spec.GRAPHS[V3](num_classes=91)
    sd = synth.state_dict(g, 0)
    imgs = torch.from_numpy(synth.images(21, 2, 320, 320))
    with torch.no_grad():
        _, _, val = op_ref.chain(g, sd, imgs, round_w=True, round_se=True, store=lambda nd, y: op_ref.h16(y))
    return g, sd, val, op_ref.OpRef(g, sd)


def _node(g, pred):
    return next(i for i, nd in enumerate(g.nodes) if pred(nd))


def _worst(got, y, e, fp16=True):
    return op_ref.ratio(got, y, e, fp16).max().item()


def _dw_taps(x, w, b, nd, acc16=False, order=1, pad_fill=None):
    """a depthwise kernel on the CPU: one multiply-add per tap in fp32 (acc16: rounded to fp16 after every tap), taps in order or reversed,
    bias first; pad_fill(xp) may overwrite the padding of the padded input"""
    n, c, h, wd = x.shape
    k, s, p = nd.k, nd.stride, nd.pad
    xp = F.pad(x, (p, p, p, p))
    if pad_fill is not None:
        pad_fill(xp, p)
    ho, wo = (h + 2 * p - k) // s + 1, (wd + 2 * p - k) // s + 1
    acc = b.view(1, -1, 1, 1).expand(n, c, ho, wo).clone()
    taps = [(ky, kx) for ky in range(k) for kx in range(k)][::order]
    for ky, kx in taps:
        acc = acc + w[:, 0, ky, kx].view(1, -1, 1, 1) * xp[:, :, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s]
        if acc16:
            acc = op_ref.h16(acc)
    return acc


def _gemm_kblocked(x, w, kb=16, skip_last_group=False):
    """a 1x1 kernel on the CPU: fp32 partial sums per block of kb input channels, blocks added last to first"""
    cin = x.shape[1]
    stop = cin - 8 if skip_last_group else cin
    out = 0
    for k0 in reversed(range(0, stop, kb)):
        k1 = min(k0 + kb, stop)
        out = out + torch.einsum("nchw,oc->nohw", x[:, k0:k1], w[:, k0:k1, 0, 0])
    return out


def test_depthwise_5x5_stride2(v3):
    g, sd, val, ref = v3
    i = _node(g, lambda nd: nd.op == "dw" and nd.k == 5 and nd.stride == 2)
    nd = g.nodes[i]
    x = val[nd.inp]
    y, e = ref.op(nd, val)
    w, b = op_ref.folded(nd, sd)
    act = op_ref.ACT[nd.act]
    # passes: fp32 accumulation in the reversed tap order
    assert _worst(op_ref.h16(act(_dw_taps(x, w, b, nd, order=-1))), y, e) <= 1.0
    # mutant that must fail: fp16 accumulation (a rounding after every tap)
    assert _worst(op_ref.h16(act(_dw_taps(x, w, b, nd, acc16=True))), y, e) > 1.0


def test_depthwise_3x3_ragged_padding(v3):
    g, sd, val, ref = v3
    i = _node(g, lambda nd: nd.op == "dw" and nd.k == 3 and nd.stride == 1 and g.t(nd.inp).h == 5)
    nd = g.nodes[i]
    x = val[nd.inp]
    y, e = ref.op(nd, val)
    w, b = op_ref.folded(nd, sd)
    act = op_ref.ACT[nd.act]
    assert _worst(op_ref.h16(act(_dw_taps(x, w, b, nd))), y, e) <= 1.0

    def next_image_rows(xp, p):
        # bottom / right padding taps read what follows in NHWC memory: the next image's first row, the next row's first pixel
        nxt = torch.roll(xp[:, :, p:-p, p:-p], -1, 0)
        xp[:, :, -p:, p:-p] = nxt[:, :, :p, :]
        xp[:, :, p:-p, -p:] = torch.cat([xp[:, :, p + 1:-p, p:p + 1], nxt[:, :, :1, :1]], 2)
    # mutant that must fail: bottom / right padding taps that read the next image's first row instead of zero
    assert _worst(op_ref.h16(act(_dw_taps(x, w, b, nd, pad_fill=next_image_rows))), y, e) > 1.0


def _se_projection(v3):
    g, sd, val, ref = v3
    i = _node(g, lambda nd: nd.op == "pw" and nd.se >= 0 and nd.residual >= 0 and nd.cin == 672 and nd.cout == 112)
    nd = g.nodes[i]
    si = _node(g, lambda q: q.op == "se" and q.out == nd.se)
    s, es = ref.op(g.nodes[si], val)            # the SE scale from the pooled sums, and its bound
    vv, ee = dict(val), {nd.se: es}
    vv[nd.se] = s
    y, e = ref.op(nd, vv, ee)
    w, b = op_ref.folded(nd, sd)
    return nd, val[nd.inp], s, val[nd.residual], w, b, y, e


def test_se_projection_with_residual(v3):
    nd, x, s, res, w, b, y, e = _se_projection(v3)
    xs = op_ref.h16(x * s[:, :, None, None])
    good = op_ref.h16(_gemm_kblocked(xs, w) + b.view(1, -1, 1, 1) + res)
    # passes: K-blocked fp32 accumulation in another order
    assert _worst(good, y, e) <= 1.0
    # mutant: the SE scale of the neighbouring image
    xs_n = op_ref.h16(x * torch.roll(s, 1, 0)[:, :, None, None])
    assert _worst(op_ref.h16(_gemm_kblocked(xs_n, w) + b.view(1, -1, 1, 1) + res), y, e) > 1.0
    # mutant: the residual missing on the last, ragged pixel tile (64-pixel tiles over the 20 x 20 map: pixels 384 .. 399)
    r = res.clone().reshape(res.shape[0], res.shape[1], -1)
    r[:, :, 384:] = 0
    assert _worst(op_ref.h16(_gemm_kblocked(xs, w) + b.view(1, -1, 1, 1) + r.view_as(res)), y, e) > 1.0


def test_fused_expand_depthwise_project(v3):
    """expand 1x1 -> depthwise 3x3 -> project 1x1 (+ residual) as one launch: only the projection's output is stored, the two
    intermediates enter their consumers through op_ref.entered()"""
    g, sd, val, ref = v3
    ip = _node(g, lambda nd: nd.op == "pw" and nd.residual >= 0 and nd.se < 0 and g.t(nd.out).h == 20 and nd.cout == 80)
    proj = g.nodes[ip]
    dw, exp = g.nodes[ip - 1], g.nodes[ip - 2]
    assert dw.op == "dw" and exp.op == "pw" and dw.inp == exp.out and proj.inp == dw.out
    x, res = val[exp.inp], val[proj.residual]
    vv, ee = {exp.inp: x, proj.residual: res}, {}
    for nd in (exp, dw):
        yv, ev = ref.op(nd, vv, ee)
        vv[nd.out], ee[nd.out] = op_ref.entered(yv, ev)
    y, e = ref.op(proj, vv, ee)
    (we, be), (wd, bd), (wp, bp) = (op_ref.folded(nd, sd) for nd in (exp, dw, proj))

    def kernel(inter=op_ref.h16, hswish=F.hardswish, bias_after_act=False):
        t = inter(hswish(_gemm_kblocked(x, we) + be.view(1, -1, 1, 1)))
        if bias_after_act:
            t2 = hswish(_dw_taps(t, wd, torch.zeros_like(bd), dw)) + bd.view(1, -1, 1, 1)
        else:
            t2 = hswish(_dw_taps(t, wd, bd, dw))
        return op_ref.h16(_gemm_kblocked(inter(t2), wp) + bp.view(1, -1, 1, 1) + res)

    assert exp.act == dw.act == spec.ACT_HSWISH
    assert _worst(kernel(), y, e) <= 1.0
    # passes: fused intermediates kept in fp32 instead of rounded
    assert _worst(kernel(inter=lambda t: t), y, e) <= 1.0
    # passes: hardswish in another algebraic form
    assert _worst(kernel(hswish=lambda v: v * torch.clamp(v / 6.0 + 0.5, 0.0, 1.0)), y, e) <= 1.0
    # mutant: the depthwise bias added after the activation
    assert _worst(kernel(bias_after_act=True), y, e) > 1.0


def test_class_head_1x1_fp32_output(v3):
    g, sd, val, ref = v3
    i = _node(g, lambda nd: nd.op == "pw" and nd.head == 1 and nd.level == 1)
    nd = g.nodes[i]
    di = _node(g, lambda q: q.out == nd.inp)
    yd, ed = ref.op(g.nodes[di], val)               # the head depthwise stays inside the fused head launch
    vv, ee = {}, {}
    vv[nd.inp], ee[nd.inp] = op_ref.entered(yd, ed)
    y, e = ref.op(nd, vv, ee)
    w, b = op_ref.folded(nd, sd)
    x = op_ref.h16(yd)
    rows = lambda t: op_ref.head_rows(g, nd, t)
    # passes: K-blocked fp32 accumulation, fp32 output (no store rounding in the bound)
    assert _worst(rows(_gemm_kblocked(x, w) + b.view(1, -1, 1, 1)), rows(y), rows(e), fp16=False) <= 1.0
    # mutant: a 1x1 that skips the last 8-channel K group
    assert _worst(rows(_gemm_kblocked(x, w, skip_last_group=True) + b.view(1, -1, 1, 1)), rows(y), rows(e), fp16=False) > 1.0


def test_ulp16():
    v = torch.tensor([1.0, 1.5, 2.0, 65504.0, 2.0 ** -14, 2.0 ** -20, 0.0])
    assert op_ref.ulp16(v).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 32.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24]
