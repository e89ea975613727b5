"""numpy restatement of dn_sgd_step (include/demonet_hip.h; csrc/optim.hip), torch.optim.SGD's update with clip_grad_norm_'s coefficient:

    d = g * coef                        clipping on: coef = min(1, max_norm / (norm + 1e-6))
    d = d + wd * p                      wd != 0
    b = first ? d : mu * b + (1 - dampening) * d        mu != 0
    d = nesterov ? d + mu * b : b                       mu != 0
    p = p - lr * d

`step_f32`: every operation one rounded float32 numpy operation in that order, the hyper-parameters rounded to float32 first -- what the device
computes bit for bit. `step_f64`: the same in float64 from the float32 inputs (hyper-parameters as Python floats). `bound`: the per-element
tolerance 8 * 2^-24 * M, M = |p| + lr (|g| + wd |p| + mu |b|) (1 + mu), between any two ways of rounding the at most six operations.
"""
import numpy as np

CONFIGS = {
    "plain": dict(lr=0.05),
    "momentum": dict(lr=0.05, momentum=0.9),
    "dampening": dict(lr=0.05, momentum=0.9, dampening=0.1),
    "nesterov": dict(lr=0.05, momentum=0.9, nesterov=True),
    "weight_decay": dict(lr=0.05, weight_decay=1e-4),
}


def _hyper(cfg):
    return (cfg["lr"], cfg.get("momentum", 0.0), cfg.get("dampening", 0.0), cfg.get("weight_decay", 0.0), bool(cfg.get("nesterov", False)))


def norm_f64(grads):
    return float(np.sqrt(sum(float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for g in grads)))


def step_f32(p, g, b, cfg, first, norm=None, max_norm=None):
    """p, g, b: float32 arrays (b ignored when first or momentum == 0); norm: the float32 norm the device computed. Returns (p', b')."""
    f = np.float32
    lr, mu, damp, wd, nesterov = _hyper(cfg)
    lr, mu, damp, wd = f(lr), f(mu), f(damp), f(wd)
    p = np.asarray(p, dtype=f)
    d = np.asarray(g, dtype=f)
    if max_norm is not None:
        coef = np.minimum(f(1.0), f(max_norm) / (f(norm) + f(1e-6))).astype(f)
        d = (d * coef).astype(f)
    if wd != 0:
        d = (d + (wd * p).astype(f)).astype(f)
    if mu != 0:
        if first:
            b = d.copy()
        else:
            b = ((mu * np.asarray(b, dtype=f)).astype(f) + ((f(1.0) - damp).astype(f) * d).astype(f)).astype(f)
        d = (d + (mu * b).astype(f)).astype(f) if nesterov else b
    else:
        b = None
    return (p - (lr * d).astype(f)).astype(f), b


def step_f64(p, g, b, cfg, first, norm=None, max_norm=None):
    lr, mu, damp, wd, nesterov = _hyper(cfg)
    p = np.asarray(p, dtype=np.float64)
    d = np.asarray(g, dtype=np.float64)
    if max_norm is not None:
        d = d * min(1.0, max_norm / (float(norm) + 1e-6))
    if wd != 0:
        d = d + wd * p
    if mu != 0:
        b = d.copy() if first else mu * np.asarray(b, dtype=np.float64) + (1.0 - damp) * d
        d = d + mu * b if nesterov else b
    else:
        b = None
    return p - lr * d, b


def bound(p, g, b, cfg):
    """8 * 2^-24 * M per element, from the values BEFORE the step (b: None = zeros)"""
    lr, mu, damp, wd, nesterov = _hyper(cfg)
    p = np.abs(np.asarray(p, dtype=np.float64))
    g = np.abs(np.asarray(g, dtype=np.float64))
    b = np.zeros_like(p) if b is None else np.abs(np.asarray(b, dtype=np.float64))
    return 8.0 * 2.0 ** -24 * (p + lr * (g + wd * p + mu * b) * (1.0 + mu))
