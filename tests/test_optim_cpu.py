"""CPU part of the optimizer tests: tests/sgd_ref.py's float32 restatement of dn_sgd_step against torch.optim.SGD, the state_dict
interchange of demonet_amd.optim.SGD, the ABI of the three new entry points, the warm-up factors of engine.train_one_epoch. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import sgd_ref
from demonet_amd import _lib, engine, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dn_sgd_workspace_bytes", "dn_grad_norm", "dn_sgd_step")


def _torch_kw(cfg):
    return {k: v for k, v in cfg.items()}


@pytest.mark.parametrize("name", list(sgd_ref.CONFIGS))
def test_float32_restatement_against_torch_sgd(name):
    """three steps; per element |ref - torch| <= 8 * 2^-24 * M (torch's CPU kernels may fuse a multiply-add: a bound, not equality). The
    first step pins b = d without dampening: with dampening 0.1 the buffer after step one must be the gradient itself, not 0.9 of it."""
    cfg = sgd_ref.CONFIGS[name]
    rng = np.random.RandomState(17)
    p0 = rng.standard_normal(1000).astype(np.float32)
    grads = [(rng.standard_normal(1000) * s).astype(np.float32) for s in (1.0, 0.3, 2.0)]
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.SGD([tp], **_torch_kw(cfg))
    p, b = p0.copy(), None
    for i, g in enumerate(grads):
        tol_p = sgd_ref.bound(p, g, b, cfg)
        tol_b = tol_p / cfg["lr"]               # (M - |p|) / lr <= M / lr: the buffer's own roundings
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, b = sgd_ref.step_f32(p, g, b, cfg, first=(i == 0))
        assert p.dtype == np.float32
        err = np.abs(p.astype(np.float64) - tp.detach().numpy().astype(np.float64))
        assert np.all(err <= tol_p), (name, i, float((err / tol_p).max()))
        if cfg.get("momentum", 0.0):
            tb = opt.state[tp]["momentum_buffer"].numpy()
            if i == 0:
                want = g if not cfg.get("weight_decay") else None
                if want is not None:
                    assert np.array_equal(b, want) and np.array_equal(tb, want), "first step: b = d, no dampening"
            errb = np.abs(b.astype(np.float64) - tb.astype(np.float64))
            assert np.all(errb <= tol_b), (name, i, float((errb / tol_b).max()))
        else:
            assert b is None and "momentum_buffer" not in opt.state[tp]


def test_float64_restatement_agrees_with_float32():
    rng = np.random.RandomState(3)
    p, g, b = (rng.standard_normal(500).astype(np.float32) for _ in range(3))
    for name, cfg in sgd_ref.CONFIGS.items():
        for first in (True, False):
            for max_norm in (None, 0.5):
                norm = np.float32(sgd_ref.norm_f64([g]))
                a32, b32 = sgd_ref.step_f32(p, g, b, cfg, first, norm, max_norm)
                a64, b64 = sgd_ref.step_f64(p, g, b, cfg, first, norm, max_norm)
                assert np.all(np.abs(a32 - a64) <= sgd_ref.bound(p, g, None if first else b, cfg)), (name, first, max_norm)
                assert (b32 is None) == (b64 is None)


def test_state_dict_and_param_groups_interchange_with_torch_sgd():
    mk = lambda: [torch.nn.Parameter(torch.arange(6, dtype=torch.float32).reshape(2, 3)), torch.nn.Parameter(torch.ones(4))]
    kw = dict(lr=0.1, momentum=0.9, dampening=0.1, weight_decay=1e-4)
    ours, theirs = optim.SGD(mk(), **kw), torch.optim.SGD(mk(), **kw)
    assert set(ours.param_groups[0]) == set(theirs.param_groups[0])
    assert {k: v for k, v in ours.param_groups[0].items() if k != "params"} == {k: v for k, v in theirs.param_groups[0].items() if k != "params"}
    assert set(ours.state_dict()) == set(theirs.state_dict()) == {"state", "param_groups"}
    # torch -> ours: a stepped torch optimizer's state
    for p in theirs.param_groups[0]["params"]:
        p.grad = torch.full_like(p, 0.5)
    theirs.step()
    sd = theirs.state_dict()
    assert all(set(v) == {"momentum_buffer"} for v in sd["state"].values())
    ours.load_state_dict(sd)
    got = ours.state_dict()
    assert got["param_groups"] == sd["param_groups"]
    assert set(got["state"]) == set(sd["state"])
    for k in sd["state"]:
        assert set(got["state"][k]) == {"momentum_buffer"} and torch.equal(got["state"][k]["momentum_buffer"], sd["state"][k]["momentum_buffer"])
    # ours -> torch
    back = torch.optim.SGD(mk(), lr=1.0)
    back.load_state_dict(got)
    assert back.param_groups[0]["lr"] == 0.1 and back.param_groups[0]["dampening"] == 0.1
    for p in back.param_groups[0]["params"]:
        assert torch.equal(back.state[p]["momentum_buffer"], torch.full_like(p, 0.5) + 1e-4 * p.detach())
        p.grad = torch.zeros_like(p)
    back.step()                              # and it steps on that state
    # schedulers drive it unchanged
    sched = torch.optim.lr_scheduler.MultiStepLR(ours, milestones=[1], gamma=0.1)
    assert isinstance(ours, torch.optim.Optimizer) and sched.get_last_lr() == [0.1]


def test_constructor_refuses_what_torch_sgd_refuses():
    p = [torch.nn.Parameter(torch.zeros(2))]
    for kw in (dict(lr=-1.0), dict(momentum=-0.1), dict(weight_decay=-1.0), dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1),
               dict(max_norm=0.0)):
        with pytest.raises(ValueError):
            optim.SGD(p, **kw)


def test_step_on_cpu_parameters_raises():
    p = torch.nn.Parameter(torch.zeros(8))
    p.grad = torch.ones(8)
    opt = optim.SGD([p], lr=0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert torch.equal(p.detach(), torch.zeros(8))
    assert opt.status() == (False, -1)


def test_symbols_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "demonet_hip.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for sym in NEW_SYMBOLS:
        assert sym in _lib.EXPORTS, sym
        assert re.search(r"DN_API\s+\w+\s+%s\(" % sym, header), sym
        assert hasattr(lib, sym), sym
    assert _lib.DN_ABI_VERSION == 1 and "#define DN_ABI_VERSION 1" in header
    assert "#define DN_SGD_CHUNK %d\n" % _lib.DN_SGD_CHUNK in header and "#define DN_SGD_MAX_GATE %d\n" % _lib.DN_SGD_MAX_GATE in header
    assert C.sizeof(_lib.SgdTensor) == 32 and C.sizeof(_lib.SgdHyper) == 32
    # host-side refusals need no device: they come before anything is enqueued
    L = _lib.lib()
    h = _lib.SgdHyper(lr=0.1)
    one = C.c_void_p(4096)
    assert L.dn_sgd_workspace_bytes(3, 10) == 80 and L.dn_sgd_workspace_bytes(0, 10) == 0 and L.dn_sgd_workspace_bytes(3, -1) == 0
    assert L.dn_grad_norm(None, 1, 1, one, 16, one, None) == -1
    assert L.dn_grad_norm(one, 0, 1, one, 16, one, None) == -1
    assert L.dn_grad_norm(one, 1, -1, one, 16, one, None) == -1
    assert L.dn_grad_norm(one, 1, 4, one, 16, one, None) == -3          # DN_E_WORKSPACE
    assert L.dn_grad_norm(one, 70000, 70000, one, 1 << 20, one, None) == -4
    assert L.dn_sgd_step(None, 1, 1, h, None, 0, None, 0.0, one, None) == -1
    assert L.dn_sgd_step(one, 1, 1, h, None, 0, None, 0.0, None, None) == -1
    assert L.dn_sgd_step(one, 1, 1, h, None, 2, None, 0.0, one, None) == -1        # gate values announced, none given
    assert L.dn_sgd_step(one, 1, 1, h, one, 9, None, 0.0, one, None) == -1
    assert L.dn_sgd_step(one, 1, 1, h, None, 0, None, 1.0, one, None) == -1        # clipping without the norm
    assert L.dn_sgd_step(one, 1, 1, h, None, 0, None, -1.0, one, None) == -1
    assert L.dn_sgd_step(one, 1, 1, _lib.SgdHyper(lr=-0.1), None, 0, None, 0.0, one, None) == -1
    assert L.dn_sgd_step(one, 1, 1, _lib.SgdHyper(lr=0.1, nesterov=1), None, 0, None, 0.0, one, None) == -1
    assert L.dn_sgd_step(one, 1, 1, _lib.SgdHyper(lr=0.1, step=-1), None, 0, None, 0.0, one, None) == -1


def test_warmup_factors_of_a_six_batch_loader():
    """engine.train_one_epoch on epoch 0: LambdaLR, factor 1/1000, min(1000, len - 1) = 5 iterations: 1e-3 (1 - x/5) + x/5, then 1"""
    p = torch.nn.Parameter(torch.zeros(2))
    opt = optim.SGD([p], lr=0.02)
    sched = engine._warmup(opt, 6)
    assert isinstance(sched, torch.optim.lr_scheduler.LambdaLR)
    got = []
    for x in range(8):
        got.append(opt.param_groups[0]["lr"])
        sched.step()
    want = [0.02 * (1e-3 * (1 - x / 5) + x / 5) if x < 5 else 0.02 for x in range(8)]
    assert got == pytest.approx(want, rel=1e-12)
    assert got[0] == pytest.approx(2e-5) and got[5] == 0.02


def test_train_log():
    log = engine.TrainLog()
    log.update(loss=1.0, lr=0.1)
    log.update(loss=3.0, lr=0.1)
    assert log.meters["loss"] == [1.0, 3.0] and log.global_avg == {"loss": 2.0, "lr": 0.1}
    assert "loss" in str(log)
