"""fp32 reference of the op IR (demonet_amd/spec.py) with a per-element bound on what the device may differ from it.

One evaluator serves three users:
  - the fp32 chain (round_w=False, round_se=False, bound=False): the op IR in fp32 from weights folded here, pinned to the reference's
    head outputs by tests/test_op_ref.py;
  - the fp16 emulation of tools/emulate_fp16.py: the same chain with the device's rounding points (fp16 weights, fp16 SE product);
  - the per-launch parity test (tests/test_gpu_launch_parity.py): every op evaluated from the device's own inputs, with the bound E.

Weights are folded here in float64 from the state_dict and rounded the way demonet_amd/plan.py documents it: fp16 weights, fp32 biases,
fp32 stem weights, fp16 SE FC weights. plan.py's fold is deliberately not called: a folding bug there must not be invisible here.

The bound (one rule, no per-layer or per-kernel constants):
    E(y) = L_act * (eps * (conv(|w|, |x|) + |b|) + conv(|w|, E(x))) + E(residual)
    + 0.5 ulp16(|got|) where the tensor is stored as fp16 (added by the comparator: ratio())
  eps = 2^-18 for every op: an fp32 fma chain stays within 3.5e-7 * sum|a b| at K = 4096, whatever the accumulation order.
  L_act is the activation's Lipschitz constant: 1 for none / ReLU / ReLU6 / max-pool, 1.5 for hardswish, 1/6 for hardsigmoid.
  A value that stays inside a fused launch enters its consumer as rn16(v) with bound E(v) + ulp16(v) (the device may round either way).
  SE: pooled in fp32 from the unrounded depthwise output; the scaled input is rn16(x s) with bound ulp16(x s) + |x| E(s) + |s| E(x).
Nothing in demonet_amd/ imports this module.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 2.0 ** -18
ACT = {0: lambda v: v, 1: F.relu, 2: F.relu6, 3: F.hardswish}
L_ACT = {0: 1.0, 1: 1.0, 2: 1.0, 3: 1.5}
L_HSIGMOID = 1.0 / 6.0


def h16(t):
    """round to the nearest fp16 (rn16) and back to fp32"""
    return t.half().float()


def ulp16(a):
    """fp16 ulp of |values| a >= 0: 2^(floor(log2 a) - 10), 2^-24 in the subnormal range"""
    return torch.exp2(torch.floor(torch.log2(a.clamp_min(2.0 ** -14))) - 10.0)


def _t64(sd, key):
    v = sd[key]
    v = v.detach().cpu() if hasattr(v, "detach") else torch.from_numpy(v.copy() if hasattr(v, "copy") else v)
    return v.double()


def folded(nd, sd, round_w=True):
    """(w, b) fp32 of a stem / pw / dw / conv node: conv (+ bias) -> BN folded in float64; w rounded to fp16 unless round_w is False or
    the node is a stem (the stem runs on fp32 weights)"""
    w = _t64(sd, nd.conv_key + ".weight")
    b = _t64(sd, nd.conv_key + ".bias") if nd.has_bias else torch.zeros(w.shape[0], dtype=torch.float64)
    if nd.bn_key:
        s = _t64(sd, nd.bn_key + ".weight") / torch.sqrt(_t64(sd, nd.bn_key + ".running_var") + nd.bn_eps)
        w = w * s.view(-1, 1, 1, 1)
        b = (b - _t64(sd, nd.bn_key + ".running_mean")) * s + _t64(sd, nd.bn_key + ".bias")
    if round_w and nd.op != "stem":          # float64 -> fp16 in one rounding, as plan.py's numpy cast does (via fp32 would round twice)
        return torch.from_numpy(w.numpy().astype(np.float16)).float(), b.float()
    return w.float(), b.float()


def se_folded(nd, sd, round_w=True):
    """(w1 [squeeze, c], b1, w2 [c, squeeze], b2) of an SE node: FC weights fp16 (rounded unless round_w is False), biases fp32"""
    w1 = _t64(sd, nd.fc1_key + ".weight").float().reshape(nd.squeeze, nd.cin)
    w2 = _t64(sd, nd.fc2_key + ".weight").float().reshape(nd.cin, nd.squeeze)
    if round_w:
        w1, w2 = h16(w1), h16(w2)
    return w1, _t64(sd, nd.fc1_key + ".bias").float(), w2, _t64(sd, nd.fc2_key + ".bias").float()


def stem_input(g, images):
    """the stem's operand: (pixel - mean) * (1 / std) in fp32, the normalisation as the stem kernels apply it (inv_std = 1.0f / std on
    the host: plan.hip, depthwise.hip stem_split_kernel); zero padding is applied to the normalised image"""
    mean = torch.tensor(g.image_mean, dtype=torch.float32).view(1, 3, 1, 1)
    inv = (1.0 / torch.tensor(g.image_std, dtype=torch.float32)).view(1, 3, 1, 1)
    return (images.float() - mean) * inv


def head_rows(g, nd, y):
    """[N, A*cols, H, W] -> [N, H*W*A, cols] (generalized_ssd.py:66-71)"""
    cols = g.num_classes if nd.head == 1 else 4
    n, _, h, w = y.shape
    return y.reshape(n, -1, cols, h, w).permute(0, 3, 4, 1, 2).reshape(n, -1, cols)


def pool_sum(y, e=None):
    """per (image, channel) fp32 sum of a depthwise output (what the pooled partial sums add up to) and its bound sum E + eps sum |y|"""
    s = y.sum(dim=(2, 3))
    return s, (None if e is None else e.sum(dim=(2, 3)) + EPS * y.abs().sum(dim=(2, 3)))


def ratio(got, y, e, fp16):
    """the comparator: |got - y| / bound per element, the bound E plus 0.5 ulp16(|got|) where got is stored as fp16 (<= 1 passes; NaN fails)"""
    return (got - y).abs() / (e + 0.5 * ulp16(got.abs()) if fp16 else e)


def entered(y, e):
    """a value that stays inside a fused launch, as its consumer reads it: rn16(v), bound E(v) + ulp16(v)"""
    return h16(y), e + ulp16(y.abs() + e)


class OpRef:
    """Evaluates one node of the graph from the values of its inputs.

    val: tensor id -> value (act: NCHW fp32; the image: stem_input(); vec: [N, C] SE scale; pool: [N, C] pooled sums)
    err: tensor id -> bound on |device - value| (missing or None: exact, e.g. the device's own stored values)
    op() returns (y, E): y the fp32 value before the output rounding, E its bound without the store term (None if bound=False)."""

    def __init__(self, g, sd, round_w=True, round_se=True, bound=True):
        self.g, self.bound, self.round_se = g, bound, round_se
        self.w, self.se = {}, {}
        for i, nd in enumerate(g.nodes):
            if nd.op in ("stem", "pw", "dw", "conv"):
                w, b = folded(nd, sd, round_w)
                self.w[i] = (w, b, w.abs(), b.abs())
            elif nd.op == "se":
                w1, b1, w2, b2 = se_folded(nd, sd, round_w)
                self.se[i] = (w1, b1, w2, b2)
            elif nd.op == "l2norm":
                self.w[i] = (_t64(sd, nd.scale_key).float(),)
        self.index = {id(nd): i for i, nd in enumerate(g.nodes)}

    def _conv(self, nd, x, w):
        return F.conv2d(x, w, None, nd.stride, nd.pad, nd.dil, nd.cin if nd.op == "dw" else 1)

    def op(self, nd, val, err=None):
        err = err or {}
        i = self.index[id(nd)]
        x = val[nd.inp]
        ex = err.get(nd.inp)
        if nd.op in ("stem", "pw", "dw", "conv"):
            w, b, aw, ab = self.w[i]
            if nd.op == "pw" and nd.se >= 0:
                s = val[nd.se][:, :, None, None]
                es = err.get(nd.se)
                xs = x * s
                if self.bound:
                    e = (ulp16(xs.abs()) if self.round_se else 0.0) + (0.0 if es is None else x.abs() * es[:, :, None, None])
                    ex = e if ex is None else e + s.abs() * ex
                x = h16(xs) if self.round_se else xs
            z = self._conv(nd, x, w) + b.view(1, -1, 1, 1)
            y = ACT[nd.act](z)
            e = None
            if self.bound:
                t = EPS * x.abs() if ex is None else EPS * x.abs() + ex
                e = L_ACT[nd.act] * (self._conv(nd, t, aw) + EPS * ab.view(1, -1, 1, 1))
            if nd.op == "pw" and nd.residual >= 0:
                y = y + val[nd.residual]
                er = err.get(nd.residual)
                if e is not None and er is not None:
                    e = e + er
            return y, e
        if nd.op == "se":
            w1, b1, w2, b2 = self.se[i]
            m = x * (1.0 / nd.stride)                   # pooled sums -> mean (stride holds the pooled pixel count)
            z = F.relu(m @ w1.t() + b1)
            s = F.hardsigmoid(z @ w2.t() + b2)
            if not self.bound:
                return s, None
            em = EPS * m.abs() if ex is None else ex * (1.0 / nd.stride) + EPS * m.abs()
            ez = EPS * (m.abs() @ w1.abs().t() + b1.abs()) + em @ w1.abs().t()
            es = L_HSIGMOID * (EPS * (z @ w2.abs().t() + b2.abs()) + ez @ w2.abs().t())
            return s, es
        if nd.op == "maxpool":
            y = F.max_pool2d(x, nd.k, nd.stride, nd.pad, ceil_mode=nd.ceil_mode)
            if not self.bound:
                return y, None
            e = torch.zeros_like(y) if ex is None else F.max_pool2d(ex, nd.k, nd.stride, nd.pad, ceil_mode=nd.ceil_mode)
            return y, e
        if nd.op == "l2norm":
            scale = self.w[i][0].view(1, -1, 1, 1)
            nrm = x.norm(dim=1, keepdim=True).clamp_min(1e-12)
            y = scale * (x / nrm)
            if not self.bound:
                return y, None
            # products: |scale| |x| / |x|_2 (sum of squares in fp32: relative eps / 2 on the norm); input error through d(x / |x|)
            e = EPS * y.abs()
            if ex is not None:
                e = e + scale.abs() * (ex + x.abs() * ex.norm(dim=1, keepdim=True) / nrm) / nrm
            return y, e
        raise ValueError(nd.op)


def chain(g, sd, images, round_w=False, round_se=False, store=None):
    """The whole op IR on [N, 3, H, W] images in [0, 1]: (cls_logits [N, A, K], bbox_regression [N, A, 4], val) where val holds every
    non-head tensor. Defaults: the fp32 chain. `store(nd, y)` rounds a stored activation (default: keep fp32)."""
    ref = OpRef(g, sd, round_w=round_w, round_se=round_se, bound=False)
    val = {g.nodes[0].inp: stem_input(g, images)}
    lg, rg = {}, {}
    for nd in g.nodes:
        y, _ = ref.op(nd, val)
        if nd.head and nd.op in ("pw", "conv"):
            (lg if nd.head == 1 else rg)[nd.level] = head_rows(g, nd, y)
            continue
        if nd.op == "dw" and nd.pool >= 0:
            val[nd.pool] = pool_sum(y)[0]           # pooled in fp32 from the unrounded outputs, as the kernels do
        val[nd.out] = store(nd, y) if store is not None and nd.op != "se" else y
    return torch.cat([lg[k] for k in sorted(lg)], 1), torch.cat([rg[k] for k in sorted(rg)], 1), val
