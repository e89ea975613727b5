"""torch.optim.SGD on the device in one launch per param group (csrc/optim.hip), with the training loop's finiteness check inside it.

    opt = demonet_amd.optim.SGD(model.head_parameters().values(), lr=0.02, momentum=0.9, weight_decay=1e-4, max_norm=10.0)
    losses = model(images, targets)
    opt.zero_grad()
    (losses["bbox_regression"] + losses["classification"]).backward()
    opt.step(gate=list(losses.values()))        # nothing is written when a loss term (or the gradient norm) is not finite
    ...
    tripped, step = opt.status()                # the ONE host synchronisation, whenever the caller wants to know

Arguments, `param_groups` keys and the per-parameter state {"momentum_buffer"} are torch.optim.SGD's, so state_dict() loads into torch.optim.SGD and
the other way round, and torch's LR schedulers drive it unchanged. What is computed per element is stated in include/demonet_hip.h (dn_sgd_step)
and restated in numpy by tests/sgd_ref.py. Differences from torch.optim.SGD + clip_grad_norm_:
  * max_norm clips by the global L2 norm of ALL gradients of the optimizer (clip_grad_norm_ over every param group), applied on the way: .grad is
    not modified;
  * the gate: once a gate value is not finite, that step and every later one writes nothing until reset_gate();
  * fp32 parameters on the GPU only; no maximize, foreach, differentiable or fused switches; no closure.
"""
import ctypes as C
from typing import Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib

CHUNK = _lib.DN_SGD_CHUNK
MAX_GATE = _lib.DN_SGD_MAX_GATE


class _Table:
    """One device table (include/demonet_hip.h, dn_sgd_tensor): T records and first[T + 1] behind them, in one int64 tensor"""

    def __init__(self, entries, device):
        # entries: (p_ptr, g_ptr, buf_ptr, numel)
        self.T = len(entries)
        first = np.zeros(self.T + 1, dtype=np.int32)
        rec = np.zeros((self.T, 4), dtype=np.int64)
        for t, (p, g, b, n) in enumerate(entries):
            rec[t] = (p, g, b, n)
            first[t + 1] = first[t] + (n + CHUNK - 1) // CHUNK
        self.chunks = int(first[-1])
        words = np.concatenate([rec.reshape(-1).view(np.int32), first, np.zeros((self.T + 1) % 2, dtype=np.int32)]).view(np.int64)
        # .grad tensors may move every step, so a table may be built every step: the upload goes from pinned memory on the current stream and the
        # host does not wait for it (the allocator keeps the pinned block until the copy has run)
        self.dev = torch.empty(words.shape, dtype=torch.int64, device=device)
        self.dev.copy_(torch.from_numpy(words).pin_memory(), non_blocking=True)


class SGD(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False,
                 *, max_norm: Optional[float] = None, gate_on_norm: bool = False):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if max_norm is not None and not max_norm > 0.0:
            raise ValueError(f"Invalid max_norm: {max_norm}")
        # (the last four keys are torch.optim.SGD's implementation switches: carried so that a state_dict moves both ways, refused when set)
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      maximize=False, foreach=None, differentiable=False, fused=None))
        self.max_norm = None if max_norm is None else float(max_norm)
        self.gate_on_norm = bool(gate_on_norm)
        self._steps = 0                 # step() calls so far = the counter of the next step
        self._born = {}                 # parameter -> the step that initialises its momentum buffer (reset_gate deletes the buffers a skipped step left unwritten)
        self._last_norm = None
        self._device = None
        self._status = None             # int32 [2] on the device: (tripped, step)
        self._gatebuf = None            # fp32 [1 + MAX_GATE]: the norm, then the gate values of a step that did not bring contiguous ones
        self._norm = None
        self._sig = None
        self._tables = None
        self._norm_table = None
        self._ws = None
        self.table_builds = 0           # device tables built so far: one per change of any pointer (a small asynchronous upload each)

    # ------------------------------------------------------------------------------------------------------
    def _devices(self, device):
        if self._device is None:
            self._device = device
            self._status = torch.zeros(2, dtype=torch.int32, device=device)
            self._gatebuf = torch.zeros(1 + MAX_GATE, dtype=torch.float32, device=device)
            self._norm = self._gatebuf[0:1]
        elif device != self._device:
            raise RuntimeError(f"optim.SGD: parameters on {device} and {self._device}; one device per optimizer")

    def _collect(self):
        """per group, (fresh, non-fresh) lists of (p, buf): the tensors of this step; creates missing momentum buffers"""
        out = []
        for group in self.param_groups:
            fresh, old = [], []
            if group.get("maximize") or group.get("differentiable"):
                raise NotImplementedError("optim.SGD: maximize and differentiable are not supported")
            for p in group["params"]:
                if p.device.type != "cuda":
                    raise RuntimeError("optim.SGD: a parameter is on {}; demonet_amd has no CPU fallback".format(p.device))
                if p.grad is None:
                    continue
                g = p.grad
                if p.dtype != torch.float32 or g.dtype != torch.float32 or g.is_sparse or not p.is_contiguous() or not g.is_contiguous() or g.shape != p.shape:
                    raise RuntimeError("optim.SGD: parameters and gradients must be dense contiguous float32 tensors of one shape, got {} {} / {} {}".format(
                        tuple(p.shape), p.dtype, tuple(g.shape), g.dtype))
                self._devices(p.device)
                if p.numel() == 0:
                    continue
                buf = None
                is_fresh = False
                if group["momentum"] != 0:
                    st = self.state[p]
                    buf = st.get("momentum_buffer")
                    if buf is None:
                        buf = st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                        self._born[p] = self._steps
                    elif buf.device != p.device or buf.dtype != torch.float32 or not buf.is_contiguous() or buf.shape != p.shape:
                        raise RuntimeError("optim.SGD: momentum_buffer of {} {} on {} for a parameter of {}".format(tuple(buf.shape), buf.dtype, buf.device, tuple(p.shape)))
                    is_fresh = self._born.get(p) == self._steps
                (fresh if is_fresh else old).append((p, buf))
            out.append((fresh, old))
        return out

    def _build(self, parts):
        sig = tuple(tuple((p.data_ptr(), p.grad.data_ptr(), 0 if b is None else b.data_ptr(), p.numel()) for p, b in part) for pair in parts for part in pair)
        if sig == self._sig:
            return
        dev = self._device
        self.table_builds += 1
        self._tables = [_Table(list(part), dev) if part else None for part in sig]
        used = [t for t in self._tables if t is not None]
        if len(used) == 1:
            self._norm_table = used[0]
        elif used:
            self._norm_table = _Table([e for part in sig for e in part], dev)
        else:
            self._norm_table = None
        if used:
            L = _lib.lib()
            need = max(L.dn_sgd_workspace_bytes(t.T, t.chunks) for t in used + [self._norm_table])
            if self._ws is None or self._ws.numel() * 8 < need:
                self._ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)
        self._sig = sig

    def _gate(self, gate, with_norm: bool, slot: Optional[Tensor]):
        """(pointer, count, norm tensor): the gate values contiguous on the device, the norm (when computed) the first of them. slot: step's norm_out"""
        if gate is None:
            vals, k = None, 0
        elif isinstance(gate, Tensor):
            vals = gate.detach().reshape(-1)
            k = vals.numel()
            if vals.device != self._device or vals.dtype != torch.float32:
                raise ValueError("optim.SGD.step: the gate must hold float32 values on {}".format(self._device))
        else:
            vals = [v.detach().reshape(()) for v in gate]
            k = len(vals)
        if k + int(with_norm) > MAX_GATE:
            raise ValueError("optim.SGD.step: {} gate values{}; at most {}".format(k, " and the norm" if with_norm else "", MAX_GATE))
        if slot is not None:
            if not (slot.numel() == 1 and slot.dtype == torch.float32 and slot.device == self._device):
                raise ValueError("optim.SGD.step: norm_out must be one float32 element on {}".format(self._device))
            if k and not (isinstance(vals, Tensor) and vals.is_contiguous() and slot.data_ptr() + 4 == vals.data_ptr()):
                raise ValueError("optim.SGD.step: norm_out must be the float32 element directly in front of a contiguous gate tensor")
            if with_norm:
                return slot.data_ptr(), k + 1, slot
            return (vals.data_ptr() if k else None), k, slot
        if k == 0:
            return (self._norm.data_ptr(), 1, self._norm) if with_norm else (None, 0, self._norm)
        dst = self._gatebuf[1:1 + k]
        if isinstance(vals, Tensor):
            dst.copy_(vals)
        else:
            torch.stack(vals, out=dst)
        return (self._norm.data_ptr(), k + 1, self._norm) if with_norm else (dst.data_ptr(), k, self._norm)

    # ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, gate: Union[None, Tensor, Sequence[Tensor]] = None, norm_out: Optional[Tensor] = None):
        """One optimizer step on the current stream. gate: up to 8 float32 device scalars (a tensor or a list of 0-d tensors, typically the loss
        terms; 7 when the norm is computed, which then joins them): if any is not finite, or the gate has tripped before, nothing is written.
        norm_out: one float32 device element that receives the norm (when one is computed) instead of the optimizer's own buffer; with gate values
        it must lie DIRECTLY IN FRONT of a contiguous `gate` tensor in the same storage, and the gate is then read in place. Without it the gate
        values are copied into the optimizer's own buffer (one small launch)."""
        parts = self._collect()
        step = self._steps
        self._steps += 1
        if self._device is None:
            return None
        self._build(parts)
        if self._norm_table is None:
            return None
        with_norm = self.max_norm is not None or self.gate_on_norm
        gate_ptr, gate_count, norm = self._gate(gate, with_norm, norm_out)
        L = _lib.lib()
        with torch.cuda.device(self._device):
            stream = C.c_void_p(torch.cuda.current_stream(self._device).cuda_stream)
            if with_norm:
                t = self._norm_table
                _lib.check(L.dn_grad_norm(C.c_void_p(t.dev.data_ptr()), t.T, t.chunks, C.c_void_p(self._ws.data_ptr()), self._ws.numel() * 8,
                                          C.c_void_p(norm.data_ptr()), stream), "dn_grad_norm")
                self._last_norm = norm
            for gi, group in enumerate(self.param_groups):
                for fi in (0, 1):
                    t = self._tables[2 * gi + fi]
                    if t is None:
                        continue
                    hyper = _lib.SgdHyper(lr=float(group["lr"]), momentum=float(group["momentum"]), dampening=float(group["dampening"]),
                                          weight_decay=float(group["weight_decay"]), nesterov=int(bool(group["nesterov"])), first_step=int(fi == 0 and group["momentum"] != 0),
                                          step=step, reserved=0)
                    _lib.check(L.dn_sgd_step(C.c_void_p(t.dev.data_ptr()), t.T, t.chunks, hyper, C.c_void_p(gate_ptr) if gate_count else None, gate_count,
                                             C.c_void_p(norm.data_ptr()) if with_norm else None, self.max_norm if self.max_norm is not None else 0.0,
                                             C.c_void_p(self._status.data_ptr()), stream), "dn_sgd_step")
        return None

    @property
    def grad_norm(self) -> Optional[Tensor]:
        """The global gradient norm of the last step that computed one (max_norm or gate_on_norm): a 1-element float32 device tensor, overwritten by
        the next step; None before the first."""
        return self._last_norm

    @property
    def steps(self) -> int:
        """step() calls so far: the counter the next step reports through status()"""
        return self._steps

    def status(self):
        """(tripped, step) by one small device-to-host copy: whether the gate has tripped and, if so, the counter (0-based count of step() calls) of the
        step that tripped it; otherwise the counter of the last step that ran (-1 before any)."""
        if self._status is None:
            return False, -1
        tripped, step = self._status.tolist()
        return bool(tripped), (int(step) if (tripped or self._steps > 0) else -1)

    def reset_gate(self):
        """Clears the gate (waits for the device once). A momentum buffer is created by the step that first needs it, before the device decides
        whether that step runs; the buffers of steps the gate skipped were never written, and this call deletes them from the state, so that
        the next step is again their first (b = d, no dampening). Until then such a buffer is in the state as zeros: a state_dict() taken while
        the gate is tripped carries it, and whoever loads that (torch.optim.SGD, or this class) takes it for an initialised buffer -- call
        reset_gate() before state_dict() after a trip."""
        if self._status is None:
            return
        tripped, at = self.status()
        if tripped:
            for p, born in list(self._born.items()):
                if born >= at:
                    self.state[p].pop("momentum_buffer", None)
                    del self._born[p]
            self._sig = None
            self._status.zero_()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._born = {}                 # loaded buffers are initialised ones
        self._sig = None
