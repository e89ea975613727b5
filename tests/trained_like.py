"""Deterministic state dicts that look like a trained checkpoint rather than like demonet_amd/synth.py's unit-variance weights.

A helper module of the tests (no fixture, no conftest; nothing in demonet_amd/ imports it). state_dict(graph, regime, seed) starts from
synth.state_dict(graph, seed) and edits it with synth.uniform / synth.normal streams under keys of its own ("<param key>#tl.<what>"), so
every machine gets the same bits.

Regime "spread"
  BatchNorm models, every BN (backbone, extras, head depthwise):
    |gamma|       2^e, e evenly spaced over [-2.5, 4] (a BN followed by an activation) or [-0.5, 6] (a linear projection), in an order drawn
                  from a stream: the spread within a layer is 2^6.5 whatever the channel count
    sign(gamma)   negative on a quarter of the channels (at least one)
    running_var   evenly spaced in log10 over [1e-3, 20], in a drawn order; the conv row, its bias and running_mean are scaled by
                  sqrt(running_var), as the statistics of a trained layer follow its weights
    beta          5 x the synthetic draw: N(0, 0.5)
    dead          BNs of >= 64 channels: max(2, 2 ceil(0.015 c)) channels with running_var 1e-12, running_mean 0, conv bias 0, a conv row
                  scaled to max |w| = 1e-6, beta = -(0.5 + u) on one half and +(0.5 + u) on the other
  SE: fc2.bias -6 on 30 % of the channels and +6 on another 30 %; fc1.bias -1 on a quarter of the hidden units
  VGG (no BN): per-output-channel gain 2^e, e evenly spaced over [-2.5, 2.5]; conv biases evenly spaced over [-8, 8] (the heads keep
  theirs); the L2Norm scale evenly spaced over [2, 40]
  One multiplier per conv (tests/golden/trained_like_calib.json, made by tests/golden/make_trained_like_calib.py with oracle/op_ref.py on
  synth.images(11, 1, H, W)) keeps the chain in range, as synth_calib.json does for the synthetic weights.

Regime "hot_heads": "spread", then weight and bias of the last convolution of every class head x HOT_CLS and of every box head x HOT_REG.

measure(graph, sd) returns the figures tests/test_lowering_trained_like.py asserts on the fp32 chain of oracle/op_ref.py.
"""
import json
import math
import os

import numpy as np

from demonet_amd import synth

REGIMES = ("spread", "hot_heads")
CALIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trained_like_calib.json")
HOT_CLS, HOT_REG = 24.0, 12.0
BBOX_XFORM_CLIP = math.log(1000.0 / 16.0)
_calib_cache = None
_loaded = {}


def calibration(name):
    global _calib_cache
    if _calib_cache is None:
        with open(CALIB_PATH) as f:
            _calib_cache = json.load(f)
    return _calib_cache[name]


def _grid(seed, key, n, lo, hi):
    """n values evenly spaced over [lo, hi] (both ends present from n = 2), in an order drawn from the stream `key`"""
    order = np.argsort(synth.uniform(seed, key, n), kind="stable")
    v = np.empty(n, dtype=np.float64)
    v[order] = np.linspace(lo, hi, n) if n > 1 else np.array([hi])
    return v


def _lowest(seed, key, n, k):
    """mask of the k channels with the smallest draws of the stream `key`"""
    m = np.zeros(n, dtype=bool)
    m[np.argsort(synth.uniform(seed, key, n), kind="stable")[:k]] = True
    return m


def n_dead(c):
    return 0 if c < 64 else max(2, 2 * int(math.ceil(0.015 * c)))


def _edit_bn(sd, nd, seed):
    bn, ck = nd.bn_key, nd.conv_key
    w = sd[ck + ".weight"].astype(np.float64)
    c = w.shape[0]
    lo, hi = (-0.5, 6.0) if nd.act == 0 else (-2.5, 4.0)
    gamma = np.exp2(_grid(seed, bn + "#tl.gamma", c, lo, hi))
    gamma[_lowest(seed, bn + "#tl.sign", c, max(1, (c + 3) // 4))] *= -1.0
    var = 10.0 ** _grid(seed, bn + "#tl.var", c, -3.0, math.log10(20.0))
    sv = np.sqrt(var)
    w = w * sv.reshape(-1, 1, 1, 1)
    mean = sd[bn + ".running_mean"].astype(np.float64) * sv
    beta = sd[bn + ".bias"].astype(np.float64) * 5.0
    bias = sd[ck + ".bias"].astype(np.float64) * sv if nd.has_bias else None
    k = n_dead(c)
    if k:
        dead = np.argsort(synth.uniform(seed, bn + "#tl.dead", c), kind="stable")[:k]
        u = synth.uniform(seed, bn + "#tl.deadbeta", k).astype(np.float64) + 0.5
        u[:k // 2] *= -1.0
        var[dead], mean[dead], beta[dead] = 1e-12, 0.0, u
        top = np.abs(w[dead]).reshape(k, -1).max(axis=1)
        w[dead] *= (1e-6 / np.maximum(top, 1e-30)).reshape(-1, 1, 1, 1)
        if bias is not None:
            bias[dead] = 0.0
    sd[ck + ".weight"] = w.astype(np.float32)
    sd[bn + ".weight"], sd[bn + ".bias"] = gamma.astype(np.float32), beta.astype(np.float32)
    sd[bn + ".running_mean"], sd[bn + ".running_var"] = mean.astype(np.float32), var.astype(np.float32)
    if bias is not None:
        sd[ck + ".bias"] = bias.astype(np.float32)


def _edit_se(sd, nd, seed):
    b2 = sd[nd.fc2_key + ".bias"].astype(np.float64)
    u = synth.uniform(seed, nd.fc2_key + ".bias#tl.shift", b2.size)
    b2 = b2 + np.where(u < 0.3, -6.0, np.where(u >= 0.7, 6.0, 0.0))
    sd[nd.fc2_key + ".bias"] = b2.astype(np.float32)
    b1 = sd[nd.fc1_key + ".bias"].astype(np.float64)
    b1[_lowest(seed, nd.fc1_key + ".bias#tl.shift", b1.size, b1.size // 4)] -= 1.0
    sd[nd.fc1_key + ".bias"] = b1.astype(np.float32)


def _edit_plain(sd, nd, seed):
    """a convolution without BN of the VGG models"""
    ck = nd.conv_key
    w = sd[ck + ".weight"].astype(np.float64)
    c = w.shape[0]
    sd[ck + ".weight"] = (w * np.exp2(_grid(seed, ck + "#tl.gain", c, -2.5, 2.5)).reshape(-1, 1, 1, 1)).astype(np.float32)
    if not nd.head:
        sd[ck + ".bias"] = _grid(seed, ck + "#tl.bias", c, -8.0, 8.0).astype(np.float32)


def state_dict(graph, regime, seed=0, calib=None):
    """numpy state dict keyed like the reference. calib: the per-conv multipliers (default: the committed table, made for seed 0)"""
    if regime not in REGIMES:
        raise ValueError(regime)
    if calib is None:
        if seed != 0:
            raise ValueError("tests/golden/trained_like_calib.json holds multipliers for weight seed 0 only")
        calib = calibration(graph.name)
    sd = {k: np.array(v) for k, v in synth.state_dict(graph, seed).items()}
    has_bn = any(nd.bn_key for nd in graph.nodes)
    for nd in graph.nodes:
        if nd.op in ("stem", "pw", "dw", "conv"):
            m = calib.get(nd.conv_key, 1.0)                  # (before the edits: a dead row keeps its 1e-6)
            if nd.head and nd.op != "dw" and regime == "hot_heads":
                hot = HOT_CLS if nd.head == 1 else HOT_REG
                m *= hot
                sd[nd.conv_key + ".bias"] = (sd[nd.conv_key + ".bias"].astype(np.float64) * hot).astype(np.float32)
            sd[nd.conv_key + ".weight"] = (sd[nd.conv_key + ".weight"].astype(np.float64) * m).astype(np.float32)
            if nd.bn_key:
                _edit_bn(sd, nd, seed)
            elif not has_bn:
                _edit_plain(sd, nd, seed)
        elif nd.op == "se":
            _edit_se(sd, nd, seed)
        elif nd.op == "l2norm":
            sd[nd.scale_key] = _grid(seed, nd.scale_key + "#tl.scale", sd[nd.scale_key].size, 2.0, 40.0).astype(np.float32)
    return sd


def load(model, regime, seed=0):
    """the regime's weights into an SSD module, as models.load_synthetic does for the synthetic ones"""
    import torch
    g = model.graph
    key = (g.name, tuple(g.size), g.num_classes, regime, seed)
    if key not in _loaded:
        _loaded.clear()                              # (one at a time: the VGG dicts are 100 MB each)
        _loaded[key] = {k: torch.from_numpy(v) for k, v in state_dict(g, regime, seed).items()}
    model.load_state_dict(_loaded[key], strict=True)          # (copies into the module's own parameters)
    return model


def measure(graph, sd):
    """The figures of the regime conditions on the fp32 chain of oracle/op_ref.py (fp16-rounded weights, one image: synth.images(11, 1, H, W))."""
    import torch
    import op_ref
    g = graph
    W, H = g.size
    with torch.no_grad():
        logits, reg, val = op_ref.chain(g, sd, torch.from_numpy(synth.images(11, 1, H, W)), round_w=True)
    out = {"finite": bool(torch.isfinite(logits).all() and torch.isfinite(reg).all()), "max_abs": 0.0, "max_act": 0.0}
    out["max_abs"] = max(float(logits.abs().max()), float(reg.abs().max()))
    r6 = [0, 0]
    hs = [0, 0, 0]
    se = [0, 0, 0]
    const = {}
    sub_layers, sub = 0, {}
    for i, nd in enumerate(g.nodes):
        if nd.op in ("pw", "dw", "conv"):
            w = op_ref.folded(nd, sd)[0]
            nz = w != 0
            share = float(((w.abs() < 2.0 ** -14) & nz).sum()) / max(1, int(nz.sum()))
            sub[nd.conv_key] = share
            sub_layers += share >= 0.01
        if nd.head and nd.op in ("pw", "conv"):
            continue
        y = val[nd.out]
        out["finite"] = out["finite"] and bool(torch.isfinite(y).all())
        if nd.op == "se":
            se[0] += int((y == 0).sum())
            se[1] += int((y == 1).sum())
            se[2] += y.numel()
            continue
        out["max_abs"] = max(out["max_abs"], float(y.abs().max()))
        out["max_act"] = max(out["max_act"], float(y.abs().max()))
        if nd.act == 2:
            r6[0] += int((y == 6).sum())
            r6[1] += y.numel()
        if nd.act == 3:                      # hardswish(z) is 0 exactly for z <= -3 and z itself for z >= 3
            hs[0] += int((y == 0).sum())
            hs[1] += int((y >= 3).sum())
            hs[2] += y.numel()
        if y.shape[2] * y.shape[3] > 1:
            flat = y.reshape(y.shape[0], y.shape[1], -1)
            const[f"op {i} {nd.op} {nd.conv_key or nd.scale_key}"] = float((flat.amax(2) == flat.amin(2)).float().mean())
    for k, v in val.items():
        out["finite"] = out["finite"] and bool(torch.isfinite(v).all())
    out["relu6_at_6"] = r6[0] / r6[1] if r6[1] else None
    out["hswish_low"], out["hswish_high"] = (hs[0] / hs[2], hs[1] / hs[2]) if hs[2] else (None, None)
    out["se_zero"], out["se_one"] = (se[0] / se[2], se[1] / se[2]) if se[2] else (None, None)
    out["subnormal_layers"] = int(sub_layers) if any(nd.bn_key for nd in g.nodes) else None
    out["subnormal"] = sub
    out["max_const"] = max(const.values())
    out["const"] = const
    rows = logits[0]
    out["logit_rows_pm60"] = float(((rows.amax(1) >= 60) & (rows.amin(1) <= -60)).float().mean())
    out["reg_rows_past_clip"] = float(((reg[0][:, 2] / 5 > BBOX_XFORM_CLIP) | (reg[0][:, 3] / 5 > BBOX_XFORM_CLIP)).float().mean())
    return out


def conditions(m, hot):
    """name -> bool for every condition that applies to the model (figures from measure()); hot: the two head conditions too"""
    c = {"finite and max |value| <= 16384": m["finite"] and m["max_abs"] <= 16384.0,
         "a stored activation with max |value| >= 256": m["max_act"] >= 256.0,
         "no layer with more than 60 % of its elements constant across pixels": m["max_const"] <= 0.6}
    if m["relu6_at_6"] is not None:
        c["ReLU6 outputs at 6 >= 3 %"] = m["relu6_at_6"] >= 0.03
    if m["hswish_low"] is not None:
        c["hardswish pre-activations <= -3 and >= 3, each >= 5 %"] = m["hswish_low"] >= 0.05 and m["hswish_high"] >= 0.05
    if m["se_zero"] is not None:
        c["SE scales exactly 0 and exactly 1, each >= 10 %"] = m["se_zero"] >= 0.10 and m["se_one"] >= 0.10
    if m["subnormal_layers"] is not None:
        c[">= 1 % subnormal fp16 weights in >= 5 layers"] = m["subnormal_layers"] >= 5
    if hot:
        c["logit rows spanning +-60"] = m["logit_rows_pm60"] > 0.0
        c[">= 1 % of the regression rows past the clip"] = m["reg_rows_past_clip"] >= 0.01
    return c
