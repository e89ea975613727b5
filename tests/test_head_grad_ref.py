"""CPU tests (-m "not gpu") of tests/head_grad_ref.py, the float64 reference and error bound the head backward is held to
(tests/test_head_grad.py): the one-level reference equals autograd through the oracle's heads, an honest emulation of the
implementation (float64 with its roundings inserted) lies inside the bound, and each of the defects a head backward risks lies outside it
on at least one case -- the bound is tight enough to matter."""
import pytest
import torch

import head_grad_ref as hr
import ssd_oracle as so

KINDS = [hr.V3, hr.V2]
DEFECTS = ["no_mask", "mask_on_h", "no_b1", "transposed", "level_shift", "tap_shift", "gamma_no_mu", "no_rsqrt"]


def _upstream(feats, aloc, K, seed, scale):
    g = torch.Generator().manual_seed(seed)
    A = sum(f.shape[2] * f.shape[3] * a for f, a in zip(feats, aloc))
    n = feats[0].shape[0]
    return (torch.randn(n, A, K, generator=g) * scale).float(), (torch.randn(n, A, 4, generator=g) * scale).float()


def test_level_reference_is_the_oracle_head():
    """level_grads on folded weights == autograd through ssd_oracle.ssdlite_head on the unfolded ones, level by level (float64: 1e-12)"""
    sd, feats, aloc = hr.mini_model(hr.V3)
    d_cls, d_reg = _upstream(feats, aloc, 5, 1, 1.0)
    ref, _ = hr.model_reference(hr.V3, sd, feats, aloc, 5, d_cls, d_reg)
    sd64 = {k: v.double() for k, v in sd.items()}
    for e in hr.head_layout(hr.V3, len(feats)):
        wd, bd, s, inv = hr.fold(sd64, e)
        dy = hr.level_dy(d_cls if e["head"] == "cls" else d_reg, feats, aloc, e["level"])
        g = hr.level_grads(feats[e["level"]], wd, bd, sd64[e["pw_w"]].reshape(dy.shape[1], -1), dy)
        torch.testing.assert_close(g["g_w1"].reshape(ref[e["pw_w"]][0].shape), ref[e["pw_w"]][0], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(g["g_b1"], ref[e["pw_b"]][0], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(g["g_bd"], ref[e["bn"] + ".bias"][0], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(g["g_wd"].t().reshape(-1, 1, 3, 3) * s.view(-1, 1, 1, 1), ref[e["dw_w"]][0], rtol=1e-12, atol=1e-12)


def test_every_head_parameter_gets_a_reference_gradient():
    for kind in KINDS:
        sd, feats, aloc = hr.mini_model(kind)
        d_cls, d_reg = _upstream(feats, aloc, 5, 2, 1.0)
        ref, _ = hr.model_reference(kind, sd, feats, aloc, 5, d_cls, d_reg)
        assert set(ref) == set(sd) - {k for k in sd if "running_" in k}
        assert all(g is not None and bool((b >= 0).all()) and bool(torch.isfinite(b).all()) for g, b in ref.values())


@pytest.mark.parametrize("i", range(len(hr.OP_CASES)))
@pytest.mark.parametrize("regime", ["small", "unit"])
def test_op_cases_condition_and_emulation(i, regime):
    """the input condition (ambiguous mask elements <= 0.5 %) and the honest emulation inside the bound, for every op-level case"""
    x, wd, bd, w1, dy = hr.op_case(i, regime)
    b = hr.level_bound(x, wd, bd, w1, dy, False)
    assert b["ambiguous"] <= hr.AMBIGUOUS_CAP
    ref = hr.level_grads(x, wd, bd, w1, dy)
    emu = hr.emulate_level(x, wd, bd, w1, dy, False)
    for k in ("g_wd", "g_bd", "g_w1", "g_b1"):
        if ref[k] is not None:
            assert hr.worst_ratio(emu[k], ref[k], b[k]) <= 1.0, k


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("scale", [1.0, 1e-5])
def test_honest_emulation_inside_the_bound(kind, scale):
    for seed in range(3):
        sd, feats, aloc = hr.mini_model(kind, seed)
        d_cls, d_reg = _upstream(feats, aloc, 5, seed, scale)
        ref, amb = hr.model_reference(kind, sd, feats, aloc, 5, d_cls, d_reg)
        assert amb <= hr.AMBIGUOUS_CAP
        emu = hr.emulate_model(kind, sd, feats, aloc, 5, d_cls, d_reg)
        for k, (g, b) in ref.items():
            assert hr.worst_ratio(emu[k], g, b) <= 1.0, k


@pytest.mark.parametrize("defect", DEFECTS)
def test_defect_outside_the_bound(defect):
    worst = 0.0
    for kind in KINDS:
        for seed in range(3):
            sd, feats, aloc = hr.mini_model(kind, seed)
            d_cls, d_reg = _upstream(feats, aloc, 5, seed, 1e-4)
            ref, _ = hr.model_reference(kind, sd, feats, aloc, 5, d_cls, d_reg)
            emu = hr.emulate_model(kind, sd, feats, aloc, 5, d_cls, d_reg, defect)
            worst = max(worst, max(hr.worst_ratio(emu[k], g, b) for k, (g, b) in ref.items()))
    assert worst > 1.0, "the bound does not see '%s' (worst ratio %.3g)" % (defect, worst)
