"""demonet_amd.optim.SGD and engine.train_one_epoch on the GPU: dn_sgd_step bit for bit against tests/sgd_ref.py's float32
restatement and within its bound of the float64 one, dn_grad_norm against the float64 norm, the gate, the state interchange with
torch.optim.SGD, a model's heads, the epoch loop."""
import copy

import numpy as np
import pytest
import torch

import sgd_ref
from demonet_amd import engine, optim

pytestmark = pytest.mark.gpu
CHUNK = optim.CHUNK
NUMELS = [1, 3, 4, 5, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
OFFSET_NUMEL = 1031          # the parameter at a storage offset of one element, its gradient too: 4-byte paths, several sweeps, a ragged end
GRAD_OFFSET_NUMEL = 2051     # an aligned parameter whose GRADIENT alone sits at a storage offset of one element (two chunks)
assert sum(NUMELS) + OFFSET_NUMEL + GRAD_OFFSET_NUMEL + 7 < 10 ** 5


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class _Case:
    """the table of the kernel tests: NUMELS, one parameter viewed at a storage offset of 1 element, one parameter whose .grad stays None"""

    def __init__(self, seed=0):
        rng = np.random.RandomState(seed)
        self.host = [rng.standard_normal(n).astype(np.float32) for n in NUMELS + [GRAD_OFFSET_NUMEL, OFFSET_NUMEL]]
        self.params = [torch.nn.Parameter(torch.from_numpy(h.copy()).cuda()) for h in self.host[:-1]]
        base = torch.zeros(OFFSET_NUMEL + 1, dtype=torch.float32, device="cuda")
        base[1:] = torch.from_numpy(self.host[-1])
        self.params.append(torch.nn.Parameter(base[1:]))
        assert self.params[-1].data_ptr() % 16 == 4 and self.params[-2].data_ptr() % 16 == 0
        self.idle_host = rng.standard_normal(7).astype(np.float32)
        self.idle = torch.nn.Parameter(torch.from_numpy(self.idle_host.copy()).cuda())
        self.rng = rng

    def all(self):
        return self.params[:5] + [self.idle] + self.params[5:]

    def grads(self, scale=1.0):
        """fresh gradients, set as .grad; those of the last two parameters are views at a storage offset of one element (the 4-byte path of the
        norm launch, and of the update through g alone and through p and g). Returns the host copies."""
        out = []
        for k, p in enumerate(self.params):
            g = (self.rng.standard_normal(p.numel()) * scale).astype(np.float32)
            out.append(g)
            if k >= len(self.params) - 2:
                base = torch.zeros(p.numel() + 1, dtype=torch.float32, device="cuda")
                base[1:] = torch.from_numpy(g)
                p.grad = base[1:]
                assert p.grad.data_ptr() % 16 == 4
            else:
                p.grad = torch.from_numpy(g).cuda()
        self.idle.grad = None
        return out


def _run(cfg, max_norm, seed=0, steps=3):
    """three steps; every step is checked against both restatements from the device's own state before it; returns the bits after each step"""
    case = _Case(seed)
    opt = optim.SGD(case.all(), max_norm=max_norm, **cfg)
    p = [h.copy() for h in case.host]
    b = [None] * len(p)
    mu = cfg.get("momentum", 0.0)
    history = []
    for i in range(steps):
        g = case.grads(scale=(1.0, 0.25, 3.0)[i % 3])
        opt.step()
        norm = None
        if max_norm is not None:
            norm = opt.grad_norm.cpu().numpy()[0]
            want = sgd_ref.norm_f64(g)
            assert abs(float(norm) - want) <= 2.0 ** -23 * want, (i, float(norm), want)
            assert (float(norm) > max_norm) == (max_norm == 2.5)     # 2.5 clips in every step, 1e4 in none (coef = 1)
        snap = []
        for k, prm in enumerate(case.params):
            p32, b32 = sgd_ref.step_f32(p[k], g[k], b[k], cfg, i == 0, norm, max_norm)
            p64, b64 = sgd_ref.step_f64(p[k], g[k], b[k], cfg, i == 0, norm, max_norm)
            tol = sgd_ref.bound(p[k], g[k], b[k], cfg)
            got_p = prm.detach().cpu().numpy()
            assert np.array_equal(got_p.view(np.int32), p32.view(np.int32)), ("p", i, k, prm.numel())
            assert np.all(np.abs(got_p - p64) <= tol), ("p64", i, k)
            snap.append(_bits(prm))
            if mu:
                got_b = opt.state[prm]["momentum_buffer"].cpu().numpy()
                assert np.array_equal(got_b.view(np.int32), b32.view(np.int32)), ("buf", i, k)
                assert np.all(np.abs(got_b - b64) <= tol / cfg["lr"]), ("buf64", i, k)
                snap.append(_bits(opt.state[prm]["momentum_buffer"]))
            else:
                assert "momentum_buffer" not in opt.state[prm]
            p[k], b[k] = p32, b32
        assert np.array_equal(case.idle.detach().cpu().numpy().view(np.int32), case.idle_host.view(np.int32)), "the parameter without .grad changed"
        assert case.idle not in opt.state or "momentum_buffer" not in opt.state[case.idle]
        if norm is not None:
            snap.append(_bits(opt.grad_norm))
        history.append(snap)
    assert opt.status() == (False, steps - 1)
    return history


@pytest.mark.parametrize("max_norm", [None, 2.5, 1e4])
@pytest.mark.parametrize("name", list(sgd_ref.CONFIGS))
def test_step_bit_exact_and_within_bound(name, max_norm):
    first = _run(sgd_ref.CONFIGS[name], max_norm)
    again = _run(sgd_ref.CONFIGS[name], max_norm)
    for a, b in zip(first, again):
        assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)), "two runs differ"


def test_grad_is_not_modified_by_clipping():
    case = _Case(1)
    opt = optim.SGD(case.all(), lr=0.1, max_norm=0.5)
    g = case.grads()
    opt.step()
    for prm, h in zip(case.params, g):
        assert np.array_equal(prm.grad.cpu().numpy().view(np.int32), h.view(np.int32))


def _state(case, opt):
    out = [_bits(p) for p in case.all()]
    out += [_bits(opt.state[p]["momentum_buffer"]) for p in case.params if "momentum_buffer" in opt.state.get(p, {})]
    return out


@pytest.mark.parametrize("how", ["gate_nan", "grad_inf"])
def test_gate(how):
    case = _Case(2)
    opt = optim.SGD(case.all(), lr=0.05, momentum=0.9, gate_on_norm=(how == "grad_inf"))
    good = torch.tensor([0.5, 1.5], device="cuda")
    case.grads()
    opt.step(gate=good)                                    # step 0 applies
    assert opt.status() == (False, 0)
    before = _state(case, opt)
    assert not torch.equal(before[0], _bits(torch.from_numpy(case.host[0])))
    case.grads()
    if how == "gate_nan":
        opt.step(gate=[good[0], torch.tensor(float("nan"), device="cuda")])
    else:
        case.params[7].grad[CHUNK - 2] = float("inf")
        opt.step(gate=good)
        assert not np.isfinite(float(opt.grad_norm.item()))
    assert opt.status() == (True, 1)
    assert all(torch.equal(a, b) for a, b in zip(before, _state(case, opt))), "a gated step wrote"
    case.grads()
    opt.step(gate=good)                                    # finite inputs, but the gate is sticky
    assert opt.status() == (True, 1)
    assert all(torch.equal(a, b) for a, b in zip(before, _state(case, opt))), "the step after a tripped gate wrote"
    opt.reset_gate()
    assert opt.status()[0] is False
    g = case.grads()
    p_before = [p.detach().cpu().numpy().copy() for p in case.params]
    b_before = [opt.state[p]["momentum_buffer"].cpu().numpy().copy() for p in case.params]
    opt.step(gate=good)
    assert opt.status() == (False, 3)
    norm = opt.grad_norm.cpu().numpy()[0] if how == "grad_inf" else None
    for k, prm in enumerate(case.params):
        p32, b32 = sgd_ref.step_f32(p_before[k], g[k], b_before[k], dict(lr=0.05, momentum=0.9), False)
        assert np.array_equal(prm.detach().cpu().numpy().view(np.int32), p32.view(np.int32)), k
        assert np.array_equal(opt.state[prm]["momentum_buffer"].cpu().numpy().view(np.int32), b32.view(np.int32)), k
    assert norm is None or np.isfinite(norm)


def test_gate_on_the_first_step_keeps_the_first_step_rule():
    """a skipped FIRST step leaves the buffers uninitialised: after reset_gate the next step is the first (b = d, no dampening)"""
    case = _Case(3)
    cfg = dict(lr=0.05, momentum=0.9, dampening=0.1)
    opt = optim.SGD(case.all(), **cfg)
    case.grads()
    opt.step(gate=torch.tensor([float("inf")], device="cuda"))
    assert opt.status() == (True, 0)
    assert all("momentum_buffer" in opt.state[p] for p in case.params)          # created by the step the device then skipped: zeros
    opt.reset_gate()
    assert not any("momentum_buffer" in opt.state[p] for p in case.params), "reset_gate keeps buffers that no step has written"
    assert opt.state_dict()["state"] == {} or all("momentum_buffer" not in v for v in opt.state_dict()["state"].values())
    g = case.grads()
    opt.step(gate=torch.tensor([1.0], device="cuda"))
    for k, prm in enumerate(case.params):
        p32, b32 = sgd_ref.step_f32(case.host[k], g[k], None, cfg, True)
        assert np.array_equal(prm.detach().cpu().numpy().view(np.int32), p32.view(np.int32)), k
        assert np.array_equal(opt.state[prm]["momentum_buffer"].cpu().numpy().view(np.int32), g[k].view(np.int32)), k


def test_norm_out_without_gate_values_receives_the_norm():
    case = _Case(6)
    opt = optim.SGD(case.all(), lr=0.05, max_norm=2.5)
    slot = torch.zeros(3, device="cuda")
    g = case.grads()
    opt.step(norm_out=slot[1:2])
    want = sgd_ref.norm_f64(g)
    assert abs(float(slot[1]) - want) <= 2.0 ** -23 * want and float(slot[0]) == 0.0 and float(slot[2]) == 0.0
    assert opt.grad_norm.data_ptr() == slot[1:2].data_ptr() and opt.status() == (False, 0)
    with pytest.raises(ValueError, match="norm_out"):
        opt.step(gate=torch.ones(2, device="cuda"), norm_out=slot[2:3])             # not in front of the gate values
    with pytest.raises(ValueError, match="norm_out"):
        opt.step(norm_out=slot[0:2])


def test_interchange_with_torch_sgd():
    cfg = dict(lr=0.05, momentum=0.9, dampening=0.1, weight_decay=1e-4)
    case = _Case(4)
    ours = optim.SGD(case.params, **cfg)
    for _ in range(2):
        case.grads()
        ours.step()
    clones = [torch.nn.Parameter(p.detach().clone()) for p in case.params]
    theirs = torch.optim.SGD(clones, lr=1.0)
    theirs.load_state_dict(copy.deepcopy(ours.state_dict()))      # (load_state_dict keeps a tensor of the right dtype and device as it is: without the copy both would step ONE buffer)
    assert theirs.param_groups[0]["lr"] == 0.05
    g = case.grads()
    before = [(p.detach().cpu().numpy().copy(), ours.state[p]["momentum_buffer"].cpu().numpy().copy()) for p in case.params]
    for c, p in zip(clones, case.params):
        c.grad = p.grad.clone()
    ours.step()
    theirs.step()
    for k, (c, p) in enumerate(zip(clones, case.params)):
        tol = sgd_ref.bound(before[k][0], g[k], before[k][1], cfg)
        assert np.all(np.abs(c.detach().cpu().numpy().astype(np.float64) - p.detach().cpu().numpy()) <= tol), k
        errb = np.abs(theirs.state[c]["momentum_buffer"].cpu().numpy().astype(np.float64) - ours.state[p]["momentum_buffer"].cpu().numpy())
        assert np.all(errb <= tol / cfg["lr"]), k
    # and back: torch's state continues in ours
    back = optim.SGD(case.params, lr=1.0)
    back.load_state_dict(copy.deepcopy(theirs.state_dict()))
    case.grads()
    back.step()
    assert back.status() == (False, 0)


def test_two_param_groups_and_a_scheduler():
    case = _Case(5)
    cfg_a, cfg_b = dict(lr=0.05, momentum=0.9), dict(lr=0.01, momentum=0.9, weight_decay=1e-3)
    opt = optim.SGD([dict(params=case.params[:6], **{k: v for k, v in cfg_a.items() if k != "momentum"}),
                     dict(params=case.params[6:] + [case.idle], lr=0.01, weight_decay=1e-3)], lr=1.0, momentum=0.9, max_norm=1.0)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1], gamma=0.5)
    p = [h.copy() for h in case.host]
    b = [None] * len(p)
    for i in range(2):
        g = case.grads()
        opt.step()
        norm = opt.grad_norm.cpu().numpy()[0]
        want = sgd_ref.norm_f64(g)
        assert abs(float(norm) - want) <= 2.0 ** -23 * want
        for k, prm in enumerate(case.params):
            cfg = dict(cfg_a if k < 6 else cfg_b)
            cfg["lr"] = cfg["lr"] * (0.5 if i >= 1 else 1.0)
            p[k], b[k] = sgd_ref.step_f32(p[k], g[k], b[k], cfg, i == 0, norm, 1.0)
            assert np.array_equal(prm.detach().cpu().numpy().view(np.int32), p[k].view(np.int32)), (i, k)
        sched.step()
    assert opt.param_groups[0]["lr"] == 0.025 and opt.status() == (False, 1)


# ------------------------------------------------------------------------------------------------------------------------------------
# whole models
def _model(K, seed=0):
    from demonet_amd import models
    return models.load_synthetic(models.ssdlite320_mobilenet_v3_large(num_classes=K), seed)


def _targets(boxes_per_image, K, seed=3):
    rng = np.random.RandomState(seed)
    targets = []
    for gcount in boxes_per_image:
        xy = rng.uniform(0, 220, (gcount, 2)).astype(np.float32)
        targets.append({"boxes": torch.from_numpy(np.concatenate([xy, xy + rng.uniform(20, 90, (gcount, 2)).astype(np.float32)], 1)).reshape(-1, 4),
                        "labels": torch.from_numpy(rng.randint(1, K, (gcount,)).astype(np.int64))})
    return targets


def _images(n, size, seed):
    from demonet_amd import synth
    return torch.from_numpy(synth.images(seed, n, size, size)).cuda()


def test_model_one_step_against_torch_sgd_and_twenty_steps():
    K = 21
    cfg = dict(lr=0.02, momentum=0.9)
    imgs, targets = _images(4, 320, 13), _targets((3, 1, 6, 2), K, seed=9)
    a, b = _model(K).cuda().train_heads().train(), _model(K).cuda().train_heads().train()
    ours, theirs = optim.SGD(a.head_parameters().values(), **cfg), torch.optim.SGD(b.head_parameters().values(), **cfg)
    start = {k: v.detach().cpu().numpy().copy() for k, v in a.head_parameters().items()}
    for m, opt in ((a, ours), (b, theirs)):
        losses = m(list(imgs), targets)
        opt.zero_grad()
        (losses["bbox_regression"] + losses["classification"]).backward()
        if opt is ours:
            opt.step(gate=list(losses.values()))
        else:
            opt.step()
    pb = b.head_parameters()
    for k, p in a.head_parameters().items():
        assert torch.equal(p.grad, pb[k].grad), k                      # the same start, the same launches: the same gradients
        tol = sgd_ref.bound(start[k], p.grad.cpu().numpy(), None, cfg)
        err = np.abs(p.detach().cpu().numpy().astype(np.float64) - pb[k].detach().cpu().numpy())
        assert np.all(err <= tol), (k, float((err / np.maximum(tol, 1e-300)).max()))
        assert not np.array_equal(p.detach().cpu().numpy(), start[k]) or not p.grad.abs().sum().item(), k
    gen = a._plan_gen
    history = [{k: v.item() for k, v in losses.items()}]
    for _ in range(19):
        losses = a(list(imgs), targets)
        ours.zero_grad()
        (losses["bbox_regression"] + losses["classification"]).backward()
        ours.step(gate=list(losses.values()))
        history.append({k: v.item() for k, v in losses.items()})
    print("optim.SGD on the heads, 20 steps:", history[0], "->", history[-1])
    for k in ("bbox_regression", "classification"):
        assert history[-1][k] < history[0][k], (k, history[0][k], history[-1][k])
    assert ours.status() == (False, 19)
    assert a._plan_gen == gen, "an optimizer step on the heads rebuilt the plan"


class _Loader:
    """a list-backed loader with a hook in front of a batch"""

    def __init__(self, batches, before=None):
        self.batches, self.before = batches, before or {}

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for i, b in enumerate(self.batches):
            if i in self.before:
                self.before[i]()
            yield b


def _batches(n_batches, K, seed=21):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n_batches):
        images, targets = [], []
        for _ in range(2):
            h, w = int(rng.randint(90, 200)), int(rng.randint(90, 200))
            images.append(torch.from_numpy(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)))
            gcount = int(rng.randint(1, 4))
            x0, y0 = rng.uniform(0, w * 0.5, gcount), rng.uniform(0, h * 0.5, gcount)
            bw, bh = rng.uniform(w * 0.2, w * 0.45, gcount), rng.uniform(h * 0.2, h * 0.45, gcount)
            targets.append({"boxes": torch.from_numpy(np.stack([x0, y0, x0 + bw, y0 + bh], 1).astype(np.float32)),
                            "labels": torch.from_numpy(rng.randint(1, K, (gcount,)).astype(np.int64))})
        out.append((images, targets))
    return out


class _SixLong(_Loader):
    """the first batches of a six-batch epoch: the warm-up schedule of the whole epoch"""

    def __len__(self):
        return 6


def _poisoned_names(m):
    """the biases of the class head's 1x1 convs, one per pyramid level. A single bias reaches the anchors of one level only, and a NaN cross
    entropy at a BACKGROUND anchor never reaches the loss (the mining ranks max(ce, 0)); +inf in all of them makes every logit row +inf, so the
    cross entropy of every foreground anchor, which the loss sums unconditionally, is NaN whatever level the boxes of a batch are matched on."""
    from demonet_amd import headgrad
    return [e.pw_b for e in headgrad.entries(m.graph) if "classification_head" in e.pw_b]


def _poison(m):
    with torch.no_grad():
        for k in _poisoned_names(m):
            m.head_parameters()[k].fill_(float("inf"))


def _epoch(m, loader, base_lr=0.02):
    opt = optim.SGD(m.head_parameters().values(), lr=base_lr, momentum=0.9, gate_on_norm=True)
    run = lambda: engine.train_one_epoch(m, opt, loader, "cuda:0", 0, 2, preset=m.train_preset(), generator=torch.Generator().manual_seed(5))
    return opt, run


def test_train_one_epoch():
    K, base_lr = 21, 0.02
    m = _model(K).cuda().train_heads()
    opt, run = _epoch(m, _Loader(_batches(6, K)), base_lr)
    start = {k: v.detach().clone() for k, v in m.head_parameters().items()}
    log = run()
    assert set(log.meters) == {"loss", "bbox_regression", "classification", "lr", "grad_norm"}
    for k, v in log.meters.items():
        assert len(v) == 6 and all(np.isfinite(x) for x in v), (k, v)
    assert log.meters["lr"] == pytest.approx([base_lr * (1e-3 * (1 - x / 5) + x / 5) for x in range(5)] + [base_lr], rel=1e-12)
    assert log.meters["loss"] == pytest.approx([a + b for a, b in zip(log.meters["bbox_regression"], log.meters["classification"])], rel=1e-6)
    assert set(log.global_avg) == set(log.meters)
    assert opt.status() == (False, 5) and m.training
    assert all(not torch.equal(start[k], p.detach()) for k, p in m.head_parameters().items())


def test_train_one_epoch_stops_at_a_non_finite_loss():
    K = 21
    batches = _batches(6, K)
    twin = _model(K).cuda().train_heads()                  # two good steps: the state the poisoned run must be left in
    topt, run = _epoch(twin, _SixLong(batches[:2]))
    assert len(run().meters["loss"]) == 2
    m = _model(K).cuda().train_heads()
    names = _poisoned_names(m)
    assert len(names) == 6
    opt, run = _epoch(m, _Loader(batches, before={2: lambda: _poison(m)}))
    with pytest.raises(FloatingPointError, match=r"step 2\b.*classification"):
        run()
    assert opt.status() == (True, 2)
    tp = twin.head_parameters()
    for k, p in m.head_parameters().items():
        if k in names:
            assert bool(torch.isinf(p).all())
        else:
            assert torch.equal(p.detach(), tp[k].detach()), k
        assert torch.equal(opt.state[p]["momentum_buffer"], topt.state[tp[k]]["momentum_buffer"]), k


def test_train_one_epoch_with_another_optimizer_checks_on_the_host():
    K = 21
    batches = _batches(3, K, seed=4)
    m = _model(K).cuda().train_heads()
    opt = torch.optim.SGD(m.head_parameters().values(), lr=0.01)
    log = engine.train_one_epoch(m, opt, _Loader(batches), "cuda:0", 1, 2, preset=m.train_preset(), generator=torch.Generator().manual_seed(1))
    assert len(log.meters["loss"]) == 3 and log.meters["lr"] == [0.01] * 3 and "grad_norm" not in log.meters
    _poison(m)
    with pytest.raises(FloatingPointError, match=r"step 0\b"):
        engine.train_one_epoch(m, opt, _Loader(batches), "cuda:0", 1, 2, preset=m.train_preset(), generator=torch.Generator().manual_seed(1))
