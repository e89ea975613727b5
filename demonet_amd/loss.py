"""SSD training loss -- the mirror of `SSD.compute_loss` plus the anchor matching that precedes it in `SSD.forward` (reference:
demonet/models/generalized_ssd.py:210-269, 316-330; _utils.py:100-133, 264-294, 348-362), computed by `dn_ssd_loss` (csrc/loss.hip;
SURVEY section 8(f) row 4), and differentiable with respect to both head outputs.

    losses, matched = ssd_loss(head_outputs, anchors, targets)         # {'bbox_regression', 'classification'}, [N, A] int64
    (losses['bbox_regression'] + losses['classification']).backward()  # when cls_logits / bbox_regression require grad

When grad mode is on and `cls_logits` or `bbox_regression` requires grad, the value comes from `dn_ssd_loss_train` (the same launches,
the same bits) and the returned losses carry a grad_fn whose backward is one HIP launch (`dn_ssd_loss_backward`); only the gradients
that are needed are computed, and they arrive in the caller's dtype and layout. Otherwise the call is `dn_ssd_loss` as before.
`anchors` and `targets` are not differentiable; neither is the backward itself (once_differentiable). These gradients stop
at the head outputs; `SSD.loss` continues them to the parameters of the model's own SSDLite heads (demonet_amd/headgrad.py). There is no
backward through the backbone.

`head_outputs` = {'cls_logits': [N, A, K], 'bbox_regression': [N, A, 4]} fp32 CUDA tensors (e.g. `SSD.forward_heads`), `anchors`
= [A, 4] (or the reference's list of N identical [A, 4] tensors), `targets` = list of {'boxes': [G, 4], 'labels': [G] int64}.
Same error behaviour as the reference where it has one: degenerate boxes raise ValueError (generalized_ssd.py:300-308).
Tie order: the reference ranks the negatives with two (unstable) sorts; only the SUM of the selected losses enters the result, which
does not depend on the order of equal values -- except in the corner where more negatives are wanted than exist (the -inf entries of
the foreground anchors enter the ranking): there csrc/loss.hip follows the stable-sort order, as torch's CPU sort happens to. The
gradient depends on WHICH negatives are mined: ties at the cut are taken in anchor order, the stable-sort order again."""
import ctypes as C
from typing import Dict, List, Tuple

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _lib

_P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None


class _SSDLossFunction(torch.autograd.Function):
    """logits [N, A, K] / reg [N, A, 4] fp32 contiguous -> (losses [2], matched [N, A]); everything else is not differentiable."""

    @staticmethod
    def forward(ctx, lg, rg, an, gb, gl, gc, gmax, iou_thresh, neg_to_pos_ratio):
        n, A, K = lg.shape
        dev = lg.device
        L = _lib.lib()
        ws = torch.empty(int(L.dn_ssd_loss_workspace_bytes(n, A)), dtype=torch.uint8, device=dev)
        state = torch.empty(int(L.dn_ssd_loss_state_bytes(n, A)), dtype=torch.uint8, device=dev)
        matched = torch.empty((n, A), dtype=torch.int64, device=dev)
        losses = torch.empty(2, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.dn_ssd_loss_train(_P(lg), _P(rg), _P(an), _P(gb), _P(gl), _P(gc), n, A, K, gmax, iou_thresh, neg_to_pos_ratio, _P(matched),
                                           _P(losses), _P(ws), ws.numel(), _P(state), state.numel(),
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "dn_ssd_loss_train")
        ctx.save_for_backward(lg, rg, an, gb, gl, state)
        ctx.gmax = gmax
        ctx.mark_non_differentiable(matched)
        return losses, matched

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_losses, _grad_matched):
        lg, rg, an, gb, gl, state = ctx.saved_tensors
        n, A, K = lg.shape
        dev = lg.device
        g = grad_losses.to(torch.float32).contiguous()
        glg = torch.empty_like(lg) if ctx.needs_input_grad[0] else None
        grg = torch.empty_like(rg) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().dn_ssd_loss_backward(_P(lg), _P(rg), _P(an), _P(gb), _P(gl), _P(state), state.numel(), _P(g), n, A, K, ctx.gmax,
                                                       _P(glg), _P(grg), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                       "dn_ssd_loss_backward")
        return glg, grg, None, None, None, None, None, None, None


def ssd_loss(head_outputs: Dict[str, Tensor], anchors, targets: List[Dict[str, Tensor]], iou_thresh: float = 0.5,
             neg_to_pos_ratio: float = 3.0) -> Tuple[Dict[str, Tensor], Tensor]:
    logits, reg = head_outputs["cls_logits"], head_outputs["bbox_regression"]
    if not logits.is_cuda:
        raise RuntimeError("ssd_loss needs CUDA tensors: there is no CPU fallback path")
    if isinstance(anchors, (list, tuple)):
        anchors = anchors[0]
    n, A, K = logits.shape
    if n == 0:
        raise ValueError("ssd_loss: empty batch")
    if reg.shape != (n, A, 4) or anchors.shape != (A, 4) or len(targets) != n:
        raise ValueError("ssd_loss: inconsistent shapes")
    GMAX = 256                                  # csrc/loss.hip: ground-truth boxes per image the matcher keeps in LDS
    for ti, t in enumerate(targets):
        if int(t["boxes"].shape[0]) > GMAX:
            raise ValueError("ssd_loss: {} ground-truth boxes for target at index {}; the matcher kernel holds at most {} per image".format(
                int(t["boxes"].shape[0]), ti, GMAX))
    for ti, t in enumerate(targets):
        b = t["boxes"]
        if b.numel():
            bad = b[:, 2:] <= b[:, :2]
            if bool(bad.any()):
                bb = b[torch.where(bad.any(dim=1))[0][0]].tolist()
                raise ValueError("All bounding boxes should have positive height and width."
                                 " Found invalid box {} for target at index {}.".format(bb, ti))
    dev = logits.device
    gmax = max(1, max(int(t["boxes"].shape[0]) for t in targets))
    gb = torch.zeros((n, gmax, 4), dtype=torch.float32, device=dev)
    gl = torch.zeros((n, gmax), dtype=torch.int64, device=dev)
    gc = torch.zeros((n,), dtype=torch.int32, device=dev)
    for i, t in enumerate(targets):
        g = int(t["boxes"].shape[0])
        if g:
            gb[i, :g] = t["boxes"].to(dev, torch.float32)
            gl[i, :g] = t["labels"].to(dev, torch.int64)
        gc[i] = g
    lg, rg, an = logits.contiguous().float(), reg.contiguous().float(), anchors.to(dev, torch.float32).contiguous()
    if torch.is_grad_enabled() and (lg.requires_grad or rg.requires_grad):
        losses, matched = _SSDLossFunction.apply(lg, rg, an, gb, gl, gc, gmax, float(iou_thresh), float(neg_to_pos_ratio))
        return {"bbox_regression": losses[0], "classification": losses[1]}, matched
    L = _lib.lib()
    ws = torch.empty(int(L.dn_ssd_loss_workspace_bytes(n, A)), dtype=torch.uint8, device=dev)
    matched = torch.empty((n, A), dtype=torch.int64, device=dev)
    losses = torch.empty(2, dtype=torch.float32, device=dev)
    P = _P
    with torch.cuda.device(dev):
        _lib.check(L.dn_ssd_loss(P(lg), P(rg), P(an), P(gb), P(gl), P(gc), n, A, K, gmax, float(iou_thresh), float(neg_to_pos_ratio),
                                 P(matched), P(losses), P(ws), ws.numel(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "dn_ssd_loss")
    return {"bbox_regression": losses[0], "classification": losses[1]}, matched
