"""CPU tests of the trained-like weight regimes (tests/trained_like.py) and of what demonet_amd/plan.py makes of them.

  conditions   the regimes reach, on the fp32 chain of oracle/op_ref.py alone, the value ranges the synthetic weights never do -- and the
               synthetic weights miss those conditions, so the conditions discriminate;
  fold parity  every weight / bias image of LoweredModel.blob equals, bit for bit, what op_ref.folded / op_ref.se_folded give (folded
               there independently, in float64), put into the layouts include/demonet_hip.h documents and restated here;
  guard        LoweredModel refuses a non-finite parameter and a folded value its storage format cannot hold, with a ValueError that names
               the state_dict key, and lets no numpy RuntimeWarning out.
"""
import warnings

import numpy as np
import pytest
import torch

import op_ref
import trained_like
from demonet_amd import spec, synth
from demonet_amd.plan import LoweredModel

V3, V2 = "ssdlite320_mobilenet_v3_large", "ssd_lite_mobilenet_v2"
MODELS = [(V3, 91, {}), (V2, 21, {}), ("ssd300_vgg16", 91, {}), ("ssd512_vgg16", 91, {})]
MODEL_IDS = [m[0] for m in MODELS]
_MEASURED, _SD = {}, {}


def _graph(name, ncls, kw):
    return spec.GRAPHS[name](num_classes=ncls, **kw)


def _sd(name, ncls, kw, regime):
    """(graph, state dict), made once and shared: nothing below writes into the arrays"""
    key = (name, tuple(kw.items()), regime)
    if key not in _SD:
        g = _graph(name, ncls, kw)
        _SD[key] = (g, synth.state_dict(g, 0) if regime == "synthetic" else trained_like.state_dict(g, regime))
    return _SD[key]


def _measured(name, ncls, kw, regime):
    key = (name, tuple(kw.items()), regime)
    if key not in _MEASURED:
        g, sd = _sd(name, ncls, kw, regime)
        torch.set_num_threads(min(16, torch.get_num_threads()))
        _MEASURED[key] = trained_like.measure(g, sd)
    return _MEASURED[key]


def _figures(m):
    return {k: v for k, v in m.items() if k not in ("subnormal", "const")}


# ------------------------------------------------------------------------------------------------ the edits themselves
@pytest.mark.parametrize("name,ncls,kw", MODELS[:3], ids=MODEL_IDS[:3])
def test_spread_edits_are_what_the_module_says(name, ncls, kw):
    g, sd = _sd(name, ncls, kw, "spread")
    plain = _sd(name, ncls, kw, "synthetic")[1]
    assert set(sd) == set(plain)
    if name == V3:
        again = trained_like.state_dict(g, "spread")
        assert all(np.array_equal(sd[k], again[k]) for k in sd)
    bns = [nd for nd in g.nodes if nd.bn_key]
    for nd in bns:
        gam, var = sd[nd.bn_key + ".weight"].astype(np.float64), sd[nd.bn_key + ".running_var"].astype(np.float64)
        mean, beta = sd[nd.bn_key + ".running_mean"], sd[nd.bn_key + ".bias"]
        c = gam.size
        assert (gam < 0).sum() >= 0.1 * c, nd.bn_key
        assert np.abs(gam).max() / np.abs(gam).min() >= 2.0 ** 6, nd.bn_key
        dead = var <= 1e-10
        assert var[~dead].min() >= 1e-3 * (1 - 1e-6) and var[~dead].max() <= 20.0 * (1 + 1e-6) and var[~dead].max() / var[~dead].min() > 1e4
        if c >= 64:
            assert dead.sum() >= 0.02 * c and dead.sum() % 2 == 0, nd.bn_key
            rows = np.abs(sd[nd.conv_key + ".weight"][dead]).reshape(int(dead.sum()), -1).max(axis=1)
            assert (mean[dead] == 0).all() and (rows <= 1e-6).all() and (rows > 0).all()
            assert (beta[dead] < 0).sum() == (beta[dead] > 0).sum() == dead.sum() // 2
        else:
            assert not dead.any()
    if not bns:
        for nd in g.nodes:
            if nd.op in ("stem", "conv"):
                r = np.abs(sd[nd.conv_key + ".weight"] / plain[nd.conv_key + ".weight"]).reshape(nd.cout, -1)[:, 0]
                assert r.max() / r.min() >= 2.0 ** 5 * (1 - 1e-5), nd.conv_key
                if not nd.head:
                    assert np.abs(sd[nd.conv_key + ".bias"]).max() == 8.0
        s = sd["backbone.scale_weight"]
        assert s.min() == 2.0 and s.max() == 40.0
    hot = _sd(name, ncls, kw, "hot_heads")[1]
    changed = sorted(k for k in sd if not np.array_equal(sd[k], hot[k]))
    heads = sorted(nd.conv_key + s for nd in g.nodes if nd.head and nd.op in ("pw", "conv") for s in (".weight", ".bias"))
    assert changed == heads


# ------------------------------------------------------------------------------------------------ the conditions
@pytest.mark.parametrize("regime", trained_like.REGIMES)
@pytest.mark.parametrize("name,ncls,kw", MODELS + [(V2, 21, {"image_size": 160})], ids=MODEL_IDS + [V2 + "-size160"])
def test_regime_conditions_hold_on_the_reference_chain(name, ncls, kw, regime):
    """On the fp32 chain with fp16-rounded weights, one image. The figures are printed; every condition that applies to the model holds."""
    m = _measured(name, ncls, kw, regime)
    print("\n", name, kw, regime, _figures(m))
    cond = trained_like.conditions(m, regime == "hot_heads")
    assert all(cond.values()), [k for k, v in cond.items() if not v]
    assert m["max_abs"] <= 16384.0 and m["max_act"] >= 256.0


@pytest.mark.parametrize("name,ncls,kw", MODELS[:3], ids=MODEL_IDS[:3])
def test_synthetic_weights_miss_the_conditions(name, ncls, kw):
    """The conditions discriminate: the synthetic weights miss at least four of those that apply to a BatchNorm model, and every one but
    the two keep-alive conditions (finite, not constant) of those that apply to the VGG model (it has no ReLU6, hardswish, SE or BN)."""
    m = _measured(name, ncls, kw, "synthetic")
    print("\n", name, "synthetic", _figures(m))
    cond = trained_like.conditions(m, True)
    missed = [k for k, v in cond.items() if not v]
    assert cond["finite and max |value| <= 16384"] and cond["no layer with more than 60 % of its elements constant across pixels"]
    assert len(missed) >= (4 if any(nd.bn_key for nd in _graph(name, ncls, kw).nodes) else 3), missed
    assert m["max_act"] < 64.0


# ------------------------------------------------------------------------------------------------ fold parity
def _fragment_major(w16):
    """[cout][cin] fp16 -> [ceil(cout / 32)][ceil(cin / 16)][2][32][8] (include/demonet_hip.h, dn_op_desc.w2_off of a PW op), zero beyond
    cout / cin; written element by element from the definition: out[t][s][h][r][j] = w[32 t + r][16 s + 8 h + j]"""
    cout, cin = w16.shape
    nt, ks = (cout + 31) // 32, (cin + 15) // 16
    t, s, h, r, j = np.meshgrid(np.arange(nt), np.arange(ks), np.arange(2), np.arange(32), np.arange(8), indexing="ij")
    row, col = 32 * t + r, 16 * s + 8 * h + j
    ok = (row < cout) & (col < cin)
    out = np.zeros((nt, ks, 2, 32, 8), dtype=np.float16)
    out[ok] = w16[row[ok], col[ok]]
    return out


def _f16(t):
    return t.numpy().astype(np.float16)           # (exact: the values are fp16 already)


def _expected_images(g, sd):
    """op index -> {field: bytes} of what the blob must hold, from op_ref's own fold"""
    head_inputs = {nd.inp for nd in g.nodes if nd.head}
    exp = {}
    for i, nd in enumerate(g.nodes):
        e = {}
        if nd.op in ("stem", "pw", "dw", "conv"):
            w, b = op_ref.folded(nd, sd)
            e["b_off"] = b.numpy().astype(np.float32).tobytes()
            if nd.op == "stem":
                e["w_off"] = np.ascontiguousarray(w.numpy().astype(np.float32).transpose(1, 2, 3, 0)).tobytes()      # [cin][ky][kx][cout] fp32
            elif nd.op == "pw":
                w16 = _f16(w).reshape(nd.cout, nd.cin)
                e["w_off"] = w16.tobytes()
                if nd.cin % 8 == 0:
                    e["w2_off"] = _fragment_major(w16).tobytes()
            elif nd.op == "dw":
                w16 = _f16(w).reshape(nd.cin, nd.k * nd.k)
                e["w_off"] = np.ascontiguousarray(w16.T).tobytes()                                                   # [tap][c]
                if nd.out in head_inputs and nd.k == 3 and nd.cin % 8 == 0:
                    e["w2_off"] = np.ascontiguousarray(w16.reshape(nd.cin // 8, 8, 9).transpose(0, 2, 1)).tobytes()   # [c / 8][tap][8]
            else:
                e["w_off"] = np.ascontiguousarray(_f16(w).transpose(0, 2, 3, 1)).tobytes()                           # [cout][ky][kx][cin]
        elif nd.op == "se":
            w1, b1, w2, b2 = op_ref.se_folded(nd, sd)
            e["w_off"] = np.ascontiguousarray(_f16(w1).T).tobytes()                                                  # [c][squeeze]
            e["b_off"] = b1.numpy().tobytes()
            e["w2_off"] = np.ascontiguousarray(_f16(w2).T).tobytes()                                                 # [squeeze][c]
            e["b2_off"] = b2.numpy().tobytes()
        elif nd.op == "l2norm":
            e["w_off"] = np.asarray(sd[nd.scale_key], dtype=np.float32).tobytes()
        exp[i] = e
    # the 1 KB slots of the fused head launch, b2_off of the class head's depthwise: per 32-channel chunk the box head's depthwise weights
    # [4 groups][9 taps][8] fp16, its bias [32] fp32, the class head's depthwise bias [32] fp32, zeros up to 1024 bytes
    producer = {nd.out: i for i, nd in enumerate(g.nodes)}
    per_level = {}
    for nd in g.nodes:
        if nd.op == "pw" and nd.head and nd.inp in producer and g.nodes[producer[nd.inp]].op == "dw":
            per_level.setdefault(nd.level, {})[nd.head] = producer[nd.inp]
    for lvl, hd in per_level.items():
        ic, ir = hd[1], hd[2]
        c = g.nodes[ic].cin
        if c % 32:
            continue
        slots = b""
        for ch in range(c // 32):
            slots += exp[ir]["w2_off"][ch * 576:(ch + 1) * 576] + exp[ir]["b_off"][ch * 128:(ch + 1) * 128] \
                + exp[ic]["b_off"][ch * 128:(ch + 1) * 128] + b"\0" * (1024 - 832)
        exp[ic]["b2_off"] = slots
    return exp


@pytest.mark.parametrize("regime", trained_like.REGIMES)
@pytest.mark.parametrize("name,ncls,kw", MODELS, ids=MODEL_IDS)
def test_fold_parity_bit_for_bit(name, ncls, kw, regime):
    g, sd = _sd(name, ncls, kw, regime)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        lm = LoweredModel(g, sd)
    exp = _expected_images(g, sd)
    checked = 0
    for i, (nd, o) in enumerate(zip(g.nodes, lm.ops)):
        for field in ("w_off", "b_off", "w2_off", "b2_off"):
            off, want = getattr(o, field), exp[i].get(field)
            if want is None:
                assert off == -1, f"op {i} {nd.op} {nd.conv_key}: {field} = {off}, no image expected"
                continue
            assert off >= 0 and off % 256 == 0, f"op {i} {nd.op} {nd.conv_key}: {field} missing"
            got = lm.blob[off:off + len(want)]
            if got != want:
                a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
                diff = np.flatnonzero(a != b) if a.size == b.size else np.array([min(a.size, b.size)])
                raise AssertionError(f"op {i} {nd.op} {nd.conv_key or nd.fc1_key or nd.scale_key}: {field} differs from op_ref's fold in "
                                     f"{diff.size} of {len(want)} bytes, first at byte {int(diff[0])}")
            checked += 1
    assert checked >= sum(len(e) for e in exp.values()) > 0
    # the regime reaches the fold's edges: folded fp16 weights that are subnormal or flushed to zero are stored, not refused
    if any(nd.bn_key for nd in g.nodes):
        sub = 0
        for i, nd in enumerate(g.nodes):
            if nd.op in ("pw", "dw"):
                w = np.frombuffer(exp[i]["w_off"], dtype=np.float16)
                sub += int(((np.abs(w) < 2.0 ** -14) & (w != 0)).sum())
        assert sub > 1000


# ------------------------------------------------------------------------------------------------ the guard
def _v2_160():
    g = spec.GRAPHS[V2](num_classes=21, image_size=160)
    return g, synth.state_dict(g, 0)


def _set(sd, key, index, value, dtype=None):
    a = np.array(sd[key], dtype=dtype or sd[key].dtype)
    a[index] = value
    sd[key] = a


def _nan_weight(sd):
    _set(sd, "backbone.body.3.conv.0.0.weight", (5, 3, 0, 0), np.nan)


def _gamma_over_zero_var(bn):
    def edit(sd):
        _set(sd, bn + ".running_var", 7, 0.0)
        _set(sd, bn + ".weight", 7, 3000.0)
    return edit


def _bn_of(g, op, **kw):
    return next(nd for nd in g.nodes if nd.op == op and nd.bn_key and all(getattr(nd, k) == v for k, v in kw.items()))


def _guard_cases():
    g2 = spec.GRAPHS[V2](num_classes=21, image_size=160)
    g3 = spec.GRAPHS[V3](num_classes=91)
    stem, dw = _bn_of(g2, "stem"), _bn_of(g2, "dw")
    se = next(nd for nd in g3.nodes if nd.op == "se")
    pw_head = next(nd for nd in g2.nodes if nd.op == "pw" and nd.head == 1)
    big_mean = lambda sd: (_gamma_over_zero_var(dw.bn_key)(sd), _set(sd, dw.bn_key + ".weight", 7, 1.0), _set(sd, dw.bn_key + ".running_mean", 7, -3e37))
    return [
        # (id, model, edit, case, keys the message must name, output channel)
        ("pw-nan-weight", V2, _nan_weight, "non-finite parameter", ["backbone.body.3.conv.0.0.weight"], 5),
        ("pw-gamma-3000-over-var-0", V2, _gamma_over_zero_var("backbone.body.3.conv.0.1"), "folded value out of range",
         ["backbone.body.3.conv.0.0.weight", "backbone.body.3.conv.0.1"], 7),
        ("pw-inf-bias", V2, lambda sd: _set(sd, pw_head.conv_key + ".bias", 11, np.inf), "non-finite parameter", [pw_head.conv_key + ".bias"], 11),
        ("stem-fp32-overflow", V2, lambda sd: (_set(sd, stem.bn_key + ".running_var", 7, 0.0), _set(sd, stem.bn_key + ".weight", 7, 3e38)),
         "folded value out of range", [stem.conv_key + ".weight", stem.bn_key], 7),
        ("dw-gamma-3000-over-var-0", V2, lambda sd: (_gamma_over_zero_var(dw.bn_key)(sd), _set(sd, dw.conv_key + ".weight", 7, 1.0)),
         "folded value out of range", [dw.conv_key + ".weight", dw.bn_key], 7),
        ("dw-folded-bias-fp32-overflow", V2, big_mean, "folded value out of range", [dw.bn_key + ".bias"], 7),
        ("bn-nan-running-mean", V2, lambda sd: _set(sd, dw.bn_key + ".running_mean", 2, np.nan), "non-finite parameter", [dw.bn_key + ".running_mean"], 2),
        ("bn-negative-var", V2, lambda sd: _set(sd, dw.bn_key + ".running_var", 3, -1.0), "folded value out of range", [dw.conv_key + ".weight", dw.bn_key], 3),
        ("conv-fp16-overflow", "ssd300_vgg16", lambda sd: _set(sd, "backbone.features.2.weight", (9, 1, 1, 1), 1e5), "folded value out of range",
         ["backbone.features.2.weight"], 9),
        ("conv-neg-inf-weight", "ssd300_vgg16", lambda sd: _set(sd, "backbone.extra.1.0.weight", (4, 0, 0, 0), -np.inf), "non-finite parameter",
         ["backbone.extra.1.0.weight"], 4),
        ("l2norm-nan-scale", "ssd300_vgg16", lambda sd: _set(sd, "backbone.scale_weight", 100, np.nan), "non-finite parameter", ["backbone.scale_weight"], 100),
        ("l2norm-scale-beyond-fp32", "ssd300_vgg16", lambda sd: _set(sd, "backbone.scale_weight", 100, 1e39, np.float64), "folded value out of range",
         ["backbone.scale_weight"], 100),
        ("se-fc1-weight-fp16-overflow", V3, lambda sd: _set(sd, se.fc1_key + ".weight", (3, 2, 0, 0), 7e4), "folded value out of range", [se.fc1_key + ".weight"], 3),
        ("se-fc2-weight-nan", V3, lambda sd: _set(sd, se.fc2_key + ".weight", (6, 1, 0, 0), np.nan), "non-finite parameter", [se.fc2_key + ".weight"], 6),
        ("se-fc1-bias-inf", V3, lambda sd: _set(sd, se.fc1_key + ".bias", 1, np.inf), "non-finite parameter", [se.fc1_key + ".bias"], 1),
        ("se-fc2-bias-beyond-fp32", V3, lambda sd: _set(sd, se.fc2_key + ".bias", 4, -1e39, np.float64), "folded value out of range", [se.fc2_key + ".bias"], 4),
    ]


_GUARD = _guard_cases()
_BASE = {}


def _base(name):
    if name not in _BASE:
        _BASE[name] = _sd(name, 21, {"image_size": 160}, "synthetic") if name == V2 else _sd(name, 91, {}, "synthetic")   # the synthetic weights, on which the unguarded lowering was seen to emit inf
    g, sd = _BASE[name]
    return g, dict(sd)


@pytest.mark.parametrize("case", _GUARD, ids=[c[0] for c in _GUARD])
def test_lowering_refuses_what_it_cannot_represent(case):
    _, name, edit, which, keys, channel = case
    g, sd = _base(name)
    edit(sd)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # a numpy RuntimeWarning (overflow / invalid value in cast) would surface as an error
        with pytest.raises(ValueError) as ei:
            LoweredModel(g, sd)
    msg = str(ei.value)
    print("\n", msg)
    assert msg.startswith(which), msg
    other = "folded value out of range" if which == "non-finite parameter" else "non-finite parameter"
    assert other not in msg
    for k in keys:
        assert k in msg, (k, msg)
    assert f"output channel {channel} " in msg, msg


def test_the_three_edits_together_are_refused_not_lowered():
    """What a diverged checkpoint looks like (one NaN weight, gamma = 3000 over running_var = 0, an inf bias): refused at the first of them
    in op order, before any blob exists."""
    g, sd = _v2_160()
    _nan_weight(sd)
    _gamma_over_zero_var("backbone.body.3.conv.0.1")(sd)
    _set(sd, "head.cls_logits.0.3.bias", 11, np.inf)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(ValueError, match="non-finite parameter: state_dict\\['backbone.body.3.conv.0.0.weight'\\] is nan at output channel 5 "):
            LoweredModel(g, sd)


def test_torch_state_dicts_are_guarded_too():
    """the form SSD._plan hands over: float32 torch tensors, integer buffers left as they are"""
    g, sd = _v2_160()
    _set(sd, "backbone.body.3.conv.0.1.bias", 0, np.inf)
    tsd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    with pytest.raises(ValueError, match="non-finite parameter: state_dict\\['backbone.body.3.conv.0.1.bias'\\]"):
        LoweredModel(g, tsd)
    g, sd = _v2_160()
    assert len(LoweredModel(g, {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}).blob) > 0
