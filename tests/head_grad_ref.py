"""Float64 reference and per-element error bound for the backward through the SSDLite heads (csrc/headgrad.hip, demonet_amd/headgrad.py).

Reference: float64 autograd through plain torch ops -- for a whole model through oracle/ssd_oracle.py's `ssdlite_head` /
`multibox_lite_head` (BN with training=False) with the fp16 features cast up exactly, every head parameter a float64 leaf and dy the
upstream gradient; for one level and one head (the op-level entry point dn_lite_head_backward, which takes folded weights) through
`level_forward` below, which tests/test_head_grad_ref.py pins to `ssdlite_head`.

The bound, in the manner of oracle/op_ref.py: derived from the roundings the implementation applies, nothing fitted.
u = 2^-11 (one fp16 rounding of a factor: u |product|), e = 2^-18 (op_ref's fp32 accumulation term: e sum|products|), and
2^-25 absolute where an fp16 value may be subnormal. The roundings, one line each:
  folded wd'  fp16 (module level only: the op-level call is GIVEN fp16 weights, they are exact there)    u |wd' x|    in z
  folded W1'  fp16 (module level only)                                                                  u |dy W1'|   in dh
  bd'         fp32                                                                                      covered by e |bd'|
  z           fp32 fma chain over nine taps                                                             e (conv(|wd'|, |x|) + |bd'|)
  h           stored as fp16(min(max(z, 0), 6)), the 1x1's operand                                      E(z) + u |h| + 2^-25
  dy          fp16(dy 2^k) 2^-k, k from max|dy| over the call's rows (dy_scale)                         u |dy| + 2^-25 2^-k
  g_b1        fp32 sum of the unrounded dy                                                              e sum|dy|
  g_W1, dh    fp16 x fp16 products exact in the matrix cores, fp32 accumulation                         e sum|products|
  g_bd, g_wd  fp32 sums of dz, dz x (x is fp16 data: exact)                                             e sum|products|
Errors of dh reach g_wd through the tap reduction as conv(|x|, E(dz)) (`tap_sums`), and the fold's chain rule is propagated term by term
(`model_reference`). Mask ambiguity: where |z| < E(z) or |z - 6| < E(z) the implementation may take either mask value, and the element's
whole term (|dh| + E(dh)) enters E(dz). `level_bound` reports the share of such elements; the tests cap it at 0.5 %.
"""
import math

import torch
import torch.nn.functional as F

import ssd_oracle as so

U16 = 2.0 ** -11
EPS = 2.0 ** -18
SUB16 = 2.0 ** -25
AMBIGUOUS_CAP = 0.005
V3 = "ssdlite320_mobilenet_v3_large"
V2 = "ssd_lite_mobilenet_v2"


def dy_scale(dy):
    """2^k of csrc/headgrad.hip (hg_scale): max|dy| 2^k in [2^13, 2^14), k clamped to [-100, 120]; 1 for an all-zero dy"""
    a = dy.abs()
    a = a[torch.isfinite(a)]
    m = float(a.max()) if a.numel() else 0.0
    if m <= 0.0:
        return 1.0
    return 2.0 ** min(120, max(-100, 14 - math.frexp(m)[1]))


def rows(t):
    """[n, ch, h, w] -> [n h w, ch]: the row form of a level (pixel-major, as the head arrays store it)"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def tap_sums(x, g):
    """[9, c]: sum over images and pixels of g[p] x[p + t] for the nine taps t = ky 3 + kx of a 3x3, pad 1 correlation -- the depthwise
    weight gradient, and with (|x|, E) the way an error of dz reaches it"""
    n, c, h, w = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    return torch.stack([(g * xp[:, :, ky:ky + h, kx:kx + w]).sum(dim=(0, 2, 3)) for ky in range(3) for kx in range(3)])


def level_forward(x, wd, bd, w1, b1):
    """one SSDLite head of one level on folded weights: x [n, c, h, w], wd [c, 1, 3, 3] or None (bare 1x1), w1 [cout, c] -> [n, cout, h, w]"""
    hcur = x if wd is None else F.relu6(F.conv2d(x, wd, bd, 1, 1, 1, x.shape[1]))
    return F.conv2d(hcur, w1.reshape(w1.shape[0], -1, 1, 1), b1)


def level_grads(x, wd, bd, w1, dy):
    """float64 autograd through level_forward: dict g_wd [9, c], g_bd [c], g_w1 [cout, c], g_b1 [cout] (the first two None without a depthwise stage)"""
    leaf = lambda t: None if t is None else t.detach().double().clone().requires_grad_(True)
    wd_, bd_, w1_ = leaf(wd), leaf(bd), leaf(w1)
    b1_ = torch.zeros(w1.shape[0], dtype=torch.float64, requires_grad=True)
    level_forward(x.double(), wd_, bd_, w1_, b1_).backward(dy.double())
    return {"g_wd": None if wd is None else wd_.grad.reshape(-1, 9).t().contiguous(), "g_bd": None if wd is None else bd_.grad,
            "g_w1": w1_.grad, "g_b1": b1_.grad}


def level_bound(x, wd, bd, w1, dy, round_w):
    """bounds on the four outputs (same shapes as level_grads) for float64 x, folded float64 wd / bd / w1 and dy [n, cout, h, w];
    round_w: the implementation rounds wd and w1 to fp16 (module level). Also 'ambiguous' (share of mask-ambiguous elements)."""
    x, w1, dy = x.double(), w1.double(), dy.double()
    rw = U16 if round_w else 0.0
    c = x.shape[1]
    edy = U16 * dy.abs() + SUB16 / dy_scale(dy)
    dyr, edyr = rows(dy), rows(edy)
    if wd is None:
        hr, ehr = rows(x.abs()), None
    else:
        wd, bd = wd.double(), bd.double()
        z = F.conv2d(x, wd, bd, 1, 1, 1, c)
        ez = (rw + EPS) * (F.conv2d(x.abs(), wd.abs(), bd.abs(), 1, 1, 1, c))
        hcur = z.clamp(0, 6)
        hr, ehr = rows(hcur), rows(ez + U16 * hcur + SUB16)
    out = {"g_b1": EPS * dyr.abs().sum(0), "ambiguous": 0.0, "g_wd": None, "g_bd": None}
    out["g_w1"] = edyr.t() @ (hr if ehr is None else hr + ehr) + EPS * (dyr.abs().t() @ hr)
    if ehr is not None:
        out["g_w1"] = out["g_w1"] + dyr.abs().t() @ ehr
    if wd is None:
        return out
    aw1 = w1.abs()
    n, _, h, w = x.shape
    unrow = lambda r: r.reshape(n, h, w, c).permute(0, 3, 1, 2)
    dh = unrow(dyr @ w1)
    edh = unrow((1.0 + rw) * (edyr @ aw1) + (rw + EPS) * (dyr.abs() @ aw1))
    mask = (z > 0) & (z < 6)
    amb = (z.abs() < ez) | ((z - 6).abs() < ez)
    edz = torch.where(amb, dh.abs() + edh, mask.double() * edh)
    adz = torch.where(amb | mask, dh.abs(), torch.zeros_like(dh))
    out["ambiguous"] = float(amb.double().mean())
    out["g_bd"] = (edz + EPS * adz).sum(dim=(0, 2, 3))
    out["g_wd"] = tap_sums(x.abs(), edz + EPS * adz)
    return out


def emulate_level(x, wd, bd, w1, dy, round_w, defect=None):
    """what a correct implementation computes, in float64 with the roundings of the module docstring inserted (and, with `defect`, one
    deliberate mistake: 'no_mask', 'mask_on_h', 'no_b1', 'tap_shift')"""
    q16 = lambda t: t.double().half().double()
    x, dy = x.double(), dy.double()
    w1q = q16(w1) if round_w else w1.double()
    S = dy_scale(dy)
    dyq = rows(q16(dy * S) / S)
    out = {"g_b1": rows(dy).sum(0), "g_wd": None, "g_bd": None}
    if defect == "no_b1":
        out["g_b1"] = torch.zeros_like(out["g_b1"])
    if wd is None:
        out["g_w1"] = dyq.t() @ rows(x)
        return out
    c = x.shape[1]
    wdq = q16(wd) if round_w else wd.double()
    z = F.conv2d(x, wdq, bd.float().double(), 1, 1, 1, c)
    hq = q16(z.clamp(0, 6))
    out["g_w1"] = dyq.t() @ rows(hq)
    n, _, h, w = x.shape
    dh = (dyq @ w1q).reshape(n, h, w, c).permute(0, 3, 1, 2)
    mask = (z > 0) & (z < 6)
    if defect == "no_mask":
        mask = torch.ones_like(mask)
    elif defect == "mask_on_h":
        mask = (z > 0) & (hq <= 6)
    dz = dh * mask.double()
    out["g_bd"] = dz.sum(dim=(0, 2, 3))
    out["g_wd"] = tap_sums(x, dz)
    if defect == "tap_shift":            # tap (1, 2) read where tap (1, 1) lies
        out["g_wd"][5] = out["g_wd"][4]
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# whole models: the reference's parameter names
def head_layout(kind, n_levels):
    """per (head, level): the state-dict keys of the reference's head. kind: V3 (ssd_mobilenetv3.py:27-36,65-95) or V2 (box_head.py:24-56)"""
    out = []
    for cols_of, v3name, v2name in (("reg", "regression_head", "bbox_pred"), ("cls", "classification_head", "cls_logits")):
        for lvl in range(n_levels):
            if kind == V3:
                p = "head.%s.module_list.%d" % (v3name, lvl)
                out.append(dict(head=cols_of, level=lvl, dw_w=p + ".0.0.weight", dw_b=None, bn=p + ".0.1", pw_w=p + ".1.weight", pw_b=p + ".1.bias", eps=1e-3))
            else:
                p = "head.%s.%d" % (v2name, lvl)
                if lvl < n_levels - 1:
                    out.append(dict(head=cols_of, level=lvl, dw_w=p + ".0.weight", dw_b=p + ".0.bias", bn=p + ".1", pw_w=p + ".3.weight", pw_b=p + ".3.bias", eps=1e-5))
                else:
                    out.append(dict(head=cols_of, level=lvl, dw_w=None, dw_b=None, bn=None, pw_w=p + ".weight", pw_b=p + ".bias", eps=1e-5))
    return out


def head_param_keys(kind, n_levels):
    keys = []
    for e in head_layout(kind, n_levels):
        keys += [k for k in (e["dw_w"], e["dw_b"], e["bn"] and e["bn"] + ".weight", e["bn"] and e["bn"] + ".bias", e["pw_w"], e["pw_b"]) if k]
    return keys


def fold(sd, e):
    """(wd' [c,1,3,3], bd' [c], s [c], inv [c]) in float64: s = gamma / sqrt(var + eps), inv = 1 / sqrt(var + eps)"""
    w = sd[e["dw_w"]].double()
    inv = 1.0 / torch.sqrt(sd[e["bn"] + ".running_var"].double() + e["eps"])
    s = sd[e["bn"] + ".weight"].double() * inv
    b = sd[e["dw_b"]].double() if e["dw_b"] else torch.zeros_like(s)
    return w * s.view(-1, 1, 1, 1), (b - sd[e["bn"] + ".running_mean"].double()) * s + sd[e["bn"] + ".bias"].double(), s, inv


def level_dy(d, feats, aloc, lvl, shift=0, transposed=False):
    """the rows of level `lvl` in a head array d [n, A, cols] as [n, aloc cols, h, w] (generalized_ssd.py:66-74 undone).
    Defects for the emulation: shift = -1 takes the previous level's anchor offset, transposed reads k A + a for a K + k."""
    off = [0]
    for f, a in zip(feats, aloc):
        off.append(off[-1] + f.shape[2] * f.shape[3] * a)
    n, _, h, w = feats[lvl].shape
    a0 = off[max(0, lvl + shift)]
    r = d[:, a0:a0 + h * w * aloc[lvl], :].reshape(n, h * w, aloc[lvl], d.shape[2])
    if transposed:
        r = r.transpose(2, 3)
    return r.reshape(n, h, w, -1).permute(0, 3, 1, 2).double()


def model_reference(kind, sd, feats, aloc, num_classes, d_cls, d_reg, levels=None):
    """{key: (gradient, bound)} float64 for every head parameter, and the largest ambiguous share over the levels.
    sd: state dict (any float dtype), feats: the level feature maps [n, c, h, w] (fp16 values), d_cls [n, A, K] / d_reg [n, A, 4]: the
    upstream gradients of the head outputs. levels: restrict the result to the parameters of these levels (the bound is the costly part)."""
    feats = [f.double() for f in feats]
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    keys = head_param_keys(kind, len(feats))
    leaves = {k: sd64[k].clone().requires_grad_(True) for k in keys}
    sd_ref = dict(sd64)
    sd_ref.update(leaves)
    out = (so.ssdlite_head if kind == V3 else so.multibox_lite_head)(sd_ref, feats, num_classes)
    ((out["cls_logits"] * d_cls.double()).sum() + (out["bbox_regression"] * d_reg.double()).sum()).backward()
    res, worst_amb = {}, 0.0
    for e in head_layout(kind, len(feats)):
        if levels is not None and e["level"] not in levels:
            continue
        x = feats[e["level"]]
        dy = level_dy(d_cls if e["head"] == "cls" else d_reg, feats, aloc, e["level"])
        w1 = sd64[e["pw_w"]].reshape(sd64[e["pw_w"]].shape[0], -1)
        if e["dw_w"] is None:
            b = level_bound(x, None, None, w1, dy, True)
        else:
            wd, bd, s, inv = fold(sd64, e)
            b = level_bound(x, wd, bd, w1, dy, True)
            worst_amb = max(worst_amb, b["ambiguous"])
            c = x.shape[1]
            e_wd = b["g_wd"].t().reshape(c, 1, 3, 3)
            w = sd64[e["dw_w"]]
            shift = (sd64[e["dw_b"]] if e["dw_b"] else 0.0) - sd64[e["bn"] + ".running_mean"]
            res[e["dw_w"]] = e_wd * s.abs().view(-1, 1, 1, 1)
            res[e["bn"] + ".weight"] = ((e_wd * w.abs()).sum(dim=(1, 2, 3)) + b["g_bd"] * shift.abs()) * inv
            res[e["bn"] + ".bias"] = b["g_bd"]
            if e["dw_b"]:
                res[e["dw_b"]] = b["g_bd"] * s.abs()
        res[e["pw_w"]] = b["g_w1"].reshape(sd64[e["pw_w"]].shape)
        res[e["pw_b"]] = b["g_b1"]
    # the chain rule itself runs in float64 on fp32 inputs and is stored as fp32: e |value| covers it
    return {k: (leaves[k].grad, res[k] + EPS * leaves[k].grad.abs()) for k in keys if k in res}, worst_amb


def emulate_model(kind, sd, feats, aloc, num_classes, d_cls, d_reg, defect=None):
    """{key: gradient}: emulate_level per level and head, then the fold's chain rule as demonet_amd/headgrad.py applies it. Defects
    beyond emulate_level's: 'transposed' (channel order), 'level_shift' (anchor offset of the previous level), 'gamma_no_mu', 'no_rsqrt'."""
    feats = [f.double() for f in feats]
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    res = {}
    for e in head_layout(kind, len(feats)):
        x = feats[e["level"]]
        dy = level_dy(d_cls if e["head"] == "cls" else d_reg, feats, aloc, e["level"], shift=-1 if defect == "level_shift" else 0,
                      transposed=defect == "transposed")
        w1 = sd64[e["pw_w"]].reshape(sd64[e["pw_w"]].shape[0], -1)
        if e["dw_w"] is None:
            g = emulate_level(x, None, None, w1, dy, True, defect)
        else:
            wd, bd, s, inv = fold(sd64, e)
            g = emulate_level(x, wd, bd, w1, dy, True, defect)
            c = x.shape[1]
            g_wd = g["g_wd"].t().reshape(c, 1, 3, 3)
            w = sd64[e["dw_w"]]
            shift = (sd64[e["dw_b"]] if e["dw_b"] else 0.0) - sd64[e["bn"] + ".running_mean"]
            if defect == "no_rsqrt":
                s, inv = sd64[e["bn"] + ".weight"], torch.ones_like(inv)
            res[e["dw_w"]] = g_wd * s.view(-1, 1, 1, 1)
            res[e["bn"] + ".weight"] = ((g_wd * w).sum(dim=(1, 2, 3)) + (0.0 if defect == "gamma_no_mu" else g["g_bd"] * shift)) * inv
            res[e["bn"] + ".bias"] = g["g_bd"]
            if e["dw_b"]:
                res[e["dw_b"]] = g["g_bd"] * s
        res[e["pw_w"]] = g["g_w1"].reshape(sd64[e["pw_w"]].shape)
        res[e["pw_b"]] = g["g_b1"]
    return res


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound (NaN counts as inf; 0 / 0 = 0)"""
    d = (got.double() - ref.double()).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / bound.double())
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------------------------------
# inputs of the tests
# (n, h = w, c, cout, depthwise stage) of the op-level cases
OP_CASES = [(2, 20, 672, 546, True), (3, 10, 480, 126, True), (1, 3, 256, 24, True), (2, 1, 128, 546, True), (2, 5, 512, 7224, True),
            (2, 19, 96, 126, True), (2, 2, 64, 24, False)]


def op_case(i, regime):
    """x [n, c, h, w] fp16 ~ clipped normal, wd [c, 1, 3, 3] fp16 of std 0.3, bd fp32, w1 [cout, c] fp16, dy [n, cout, h, w] fp32 dense:
    regime 'small' = magnitudes spread over 1e-6 .. 1e-3, 'unit' = O(1)"""
    n, hw, c, cout, dw = OP_CASES[i]
    g = torch.Generator().manual_seed(100 + i)
    x = (torch.randn(n, c, hw, hw, generator=g) * 2).clamp(0, 6).half()
    wd = (torch.randn(c, 1, 3, 3, generator=g) * 0.3).half() if dw else None
    bd = (torch.randn(c, generator=g) * 0.5) if dw else None
    w1 = (torch.randn(cout, c, generator=g) * 0.1).half()
    dy = torch.randn(n, cout, hw, hw, generator=g)
    if regime == "small":
        dy = dy * torch.pow(10.0, -6 + 3 * torch.rand(n, cout, hw, hw, generator=g))
    return x, wd, bd, w1, dy.float()


def mini_model(kind, seed=0, num_classes=5):
    """a small head in the reference's key names for the CPU tests: (sd, feats fp16 [n, c, h, w], anchors per location)"""
    g = torch.Generator().manual_seed(seed)
    shapes, aloc = [(16, 5), (24, 3), (8, 2)], [2, 3, 2]
    feats = [(torch.randn(2, c, s, s, generator=g) * 2).clamp(0, 6).half() for c, s in shapes]
    sd = {}
    for e in head_layout(kind, len(shapes)):
        c = shapes[e["level"]][0]
        cout = aloc[e["level"]] * (num_classes if e["head"] == "cls" else 4)
        if e["dw_w"]:
            sd[e["dw_w"]] = torch.randn(c, 1, 3, 3, generator=g) * 0.3
            if e["dw_b"]:
                sd[e["dw_b"]] = torch.randn(c, generator=g) * 0.3
            sd[e["bn"] + ".weight"] = 0.5 + torch.rand(c, generator=g)
            sd[e["bn"] + ".bias"] = torch.randn(c, generator=g) * 0.5
            sd[e["bn"] + ".running_mean"] = torch.randn(c, generator=g) * 0.5
            sd[e["bn"] + ".running_var"] = 0.5 + torch.rand(c, generator=g)
        sd[e["pw_w"]] = torch.randn(cout, c, 1, 1, generator=g) * 0.1
        sd[e["pw_b"]] = torch.randn(cout, generator=g) * 0.1
    return sd, feats, aloc
