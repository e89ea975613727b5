"""Training the SSDLite heads on the frozen backbone: the head forward from the module's current fp32 parameters and its backward to
every head parameter (csrc/headgrad.hip).

    model.train_heads(True)
    losses = model.loss(images, targets)                 # or: model.train(); model(images, targets)
    (losses["bbox_regression"] + losses["classification"]).backward()      # .grad of every head parameter that requires it

Scope: depthwise 3x3 + BN + ReLU6 -> 1x1 conv with bias per level, class and box head (reference: ssd_mobilenetv3.py:27-36; the V2 hub
model's MultiBoxLiteHead, box_head.py:24-56, whose depthwise conv has a bias and whose last level is a bare 1x1). The dense 3x3 heads of
the VGG models need a convolution weight gradient and are not covered: `entries` raises NotImplementedError for them.

One step: the features come from the plan (dn_forward_features: frozen fp16 backbone, BN folded; the plan is not rebuilt while only head
parameters change), one piece per sub-batch chain (dn_level_features). The head is folded on the device from the fp32 master
parameters in float64 exactly as plan.py folds it -- s = gamma / sqrt(var + eps), wd' = fp16(w s), bd' = fp32((b - mean) s + beta),
W1' = fp16(W1): the same bits as the plan's weight blob -- and run with the launch-per-layer kernels (dn_depthwise_conv,
dn_pointwise_conv(out_fp32 = 1) at the level's anchor offset). The backward calls dn_lite_head_backward per level, head and piece
(pieces are added in chain order: deterministic) and applies the fold's chain rule in float64, straight through the fp16 rounding:
    dw = g_wd s,  dgamma = (sum_t g_wd w + g_bd (b - mean)) / sqrt(var + eps),  dbeta = g_bd,  db = g_bd s,  dW1 = g_W1,  db1 = g_b1.

Deviation from the reference, stated: head BN uses its running statistics (frozen, as FrozenBatchNorm2d fine-tuning does), where the
reference's train mode would use batch statistics: the gradients are those of the reference model with its head BN modules in eval()."""
import ctypes as C
from typing import List

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _lib

_P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
DN_ACT_NONE, DN_ACT_RELU6 = 0, 2


class Entry:
    """one head of one level: its parameter keys and geometry"""

    def __init__(self, graph, pw, dw, aoff):
        t = graph.t(graph.features[pw.level])
        self.kind, self.level = pw.head, pw.level                 # 1 class logits, 2 box regression
        self.c, self.h, self.w, self.cout = t.c, t.h, t.w, pw.cout
        self.cols = graph.num_classes if pw.head == 1 else 4
        self.aoff = aoff                                          # first anchor of the level
        self.pw_w, self.pw_b = pw.conv_key + ".weight", pw.conv_key + ".bias"
        self.dw_w = dw.conv_key + ".weight" if dw is not None else None
        self.dw_b = dw.conv_key + ".bias" if dw is not None and dw.has_bias else None
        self.bn = dw.bn_key if dw is not None else None
        self.eps = dw.bn_eps if dw is not None else 0.0

    def keys(self) -> List[str]:
        """parameter keys in the module's registration order"""
        k = []
        if self.dw_w:
            k.append(self.dw_w)
            if self.dw_b:
                k.append(self.dw_b)
            k += [self.bn + ".weight", self.bn + ".bias"]
        return k + [self.pw_w, self.pw_b]


def entries(graph) -> List[Entry]:
    """the SSDLite heads of a graph, level by level; NotImplementedError for any other head form"""
    by_out = {nd.out: nd for nd in graph.nodes}
    aoff, off = [], 0
    for a, f in zip(graph.anchors_per_loc, graph.features):
        aoff.append(off)
        off += a * graph.t(f).h * graph.t(f).w
    res = []
    for nd in graph.nodes:
        if not nd.head or nd.op == "dw":
            continue
        feat = graph.features[nd.level]
        dw = None
        ok = nd.op == "pw" and nd.has_bias and nd.bn_key is None
        if ok and nd.inp != feat:
            dw = by_out.get(nd.inp)
            ok = (dw is not None and dw.op == "dw" and dw.inp == feat and dw.k == 3 and dw.stride == 1 and dw.pad == 1 and dw.dil == 1
                  and dw.act == DN_ACT_RELU6 and dw.bn_key is not None)
        if not ok:
            raise NotImplementedError("the head backward covers the SSDLite heads (depthwise 3x3 + BN + ReLU6 -> 1x1) only; '{}' has a {} head "
                                      "at level {} (the dense 3x3 heads of the VGG models need a convolution weight gradient)".format(
                                          graph.name, nd.op, nd.level))
        res.append(Entry(graph, nd, dw, aoff[nd.level]))
    return res


def parameter_names(graph) -> List[str]:
    return [k for e in entries(graph) for k in e.keys()]


def to_half_once(d: Tensor) -> Tensor:
    """float64 -> fp16 with ONE rounding, as numpy's astype(float16) in plan.py: a device cast goes through fp32 and rounds twice, so
    the fp32 intermediate is made by round-to-odd (truncate towards zero, then set the last bit if anything was lost), after which the
    nearest-even rounding of the 13 bits below fp16's precision is the correct one"""
    a = d.abs()
    f = a.float()
    back = f.double()
    bits = f.view(torch.int32)
    bits = torch.where(back > a, bits - 1, bits)
    bits = torch.where(back != a, bits | 1, bits)
    return torch.copysign(bits.view(torch.float32), d.float()).half()


def fold(e: Entry, P: dict, B: dict):
    """(wd' [9][c] fp16, bd' [c] fp32, W1' [cout][c] fp16, b1 [cout] fp32, s, inv) on the parameters' device; the first two and the last
    two None without a depthwise stage. Float64 throughout, in plan.py's order of operations."""
    w1 = P[e.pw_w].detach().reshape(e.cout, e.c).double()
    w1h = to_half_once(w1).contiguous()
    b1 = P[e.pw_b].detach().double().float().contiguous()
    if e.dw_w is None:
        return None, None, w1h, b1, None, None
    g, beta = P[e.bn + ".weight"].detach().double(), P[e.bn + ".bias"].detach().double()
    mu, var = B[e.bn + ".running_mean"].double(), B[e.bn + ".running_var"].double()
    inv = 1.0 / torch.sqrt(var + e.eps)
    s = g / torch.sqrt(var + e.eps)
    b = P[e.dw_b].detach().double() if e.dw_b else torch.zeros_like(s)
    wd = P[e.dw_w].detach().reshape(e.c, 9).double() * s[:, None]
    return to_half_once(wd).t().contiguous(), ((b - mu) * s + beta).float().contiguous(), w1h, b1, s, inv


class _Step:
    """what one training forward leaves for its backward: the feature pieces inside the model's workspace and the folded weights"""

    def __init__(self, model, n, ents, pieces, gen):
        self.model, self.n, self.ents, self.pieces, self.gen = model, n, ents, pieces, gen
        self.folded = []


class _LiteHeads(torch.autograd.Function):
    """(step, *head parameters in parameter_names order) -> (cls_logits [n, A, K], bbox_regression [n, A, 4]) fp32"""

    @staticmethod
    def forward(ctx, step, *params):
        model, n, ents = step.model, step.n, step.ents
        g = model.graph
        names = parameter_names(g)
        P = dict(zip(names, params))
        B = dict(model.named_buffers())
        dev = params[0].device
        A, K = g.num_anchors(), g.num_classes
        logits = torch.empty((n, A, K), dtype=torch.float32, device=dev)
        reg = torch.empty((n, A, 4), dtype=torch.float32, device=dev)
        L = _lib.lib()
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        hmax = max(im * e.h * e.w * e.c for e in ents for _, _, im in step.pieces[e.level])
        hbuf = torch.empty(hmax, dtype=torch.float16, device=dev)
        with torch.cuda.device(dev):
            for e in ents:
                wd, bd, w1, b1, s, inv = fold(e, P, B)
                step.folded.append((wd, bd, w1, b1, s, inv))
                out = logits if e.kind == 1 else reg
                for x, first, im in step.pieces[e.level]:
                    src = x
                    if wd is not None:
                        _lib.check(L.dn_depthwise_conv(_P(x), _P(wd), _P(bd), _P(hbuf), im, e.h, e.w, e.c, 3, 1, 1, DN_ACT_RELU6, stream), "dn_depthwise_conv")
                        src = hbuf
                    dst = C.c_void_p(out.data_ptr() + 4 * (first * A * e.cols + e.aoff * e.cols))
                    _lib.check(L.dn_pointwise_conv(_P(src), _P(w1), None, _P(b1), None, None, dst, im * e.h * e.w, e.c, e.cout, e.h * e.w,
                                                   DN_ACT_NONE, 1, A * e.cols, stream), "dn_pointwise_conv")
        ctx.step = step
        ctx.save_for_backward(*params)
        return logits, reg

    @staticmethod
    @once_differentiable
    def backward(ctx, g_logits, g_reg):
        step = ctx.step
        model, ents = step.model, step.ents
        if model._feat_gen != step.gen:
            raise RuntimeError("SSD.loss backward: the model ran another forward since this loss was computed; its features are gone "
                               "(call backward() before the next forward of the model)")
        g = model.graph
        names = parameter_names(g)
        P = dict(zip(names, ctx.saved_tensors))
        need = dict(zip(names, ctx.needs_input_grad[1:]))
        B = dict(model.named_buffers())
        dev = ctx.saved_tensors[0].device
        A = g.num_anchors()
        L = _lib.lib()
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        ws_bytes = max(int(L.dn_lite_head_backward_workspace_bytes(im, e.h, e.w, e.c, e.cout, int(e.dw_w is not None)))
                       for e in ents for _, _, im in step.pieces[e.level])
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        grads = {}
        f32 = dict(dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            for e, (wd, bd, w1, b1, s, inv) in zip(ents, step.folded):
                if not any(need[k] for k in e.keys()):
                    continue
                dy = g_logits if e.kind == 1 else g_reg
                if dy is None:
                    continue
                dy = dy.contiguous().float()
                total = None
                for x, first, im in step.pieces[e.level]:
                    out = [torch.empty((9, e.c), **f32) if wd is not None else None, torch.empty((e.c,), **f32) if wd is not None else None,
                           torch.empty((e.cout, e.c), **f32), torch.empty((e.cout,), **f32)]
                    dyp = C.c_void_p(dy.data_ptr() + 4 * (first * A * e.cols + e.aoff * e.cols))
                    _lib.check(L.dn_lite_head_backward(_P(x), _P(wd), _P(bd), _P(w1), dyp, A * e.cols, im, e.h, e.w, e.c, e.cout, _P(out[0]), _P(out[1]),
                                                       _P(out[2]), _P(out[3]), _P(ws), ws.numel(), stream), "dn_lite_head_backward")
                    total = out if total is None else [a + b if a is not None else None for a, b in zip(total, out)]     # chain order
                g_wd, g_bd, g_w1, g_b1 = total
                grads[e.pw_w] = g_w1.reshape(P[e.pw_w].shape)
                grads[e.pw_b] = g_b1
                if wd is None:
                    continue
                gw = g_wd.double().t().reshape(e.c, 1, 3, 3)
                gb = g_bd.double()
                w = P[e.dw_w].detach().double()
                shift = (P[e.dw_b].detach().double() if e.dw_b else 0.0) - B[e.bn + ".running_mean"].double()
                grads[e.dw_w] = gw * s.view(-1, 1, 1, 1)
                grads[e.bn + ".weight"] = ((gw * w).sum(dim=(1, 2, 3)) + gb * shift) * inv
                grads[e.bn + ".bias"] = gb
                if e.dw_b:
                    grads[e.dw_b] = gb * s
        res = []
        for k in names:
            gk = grads.get(k) if need[k] else None
            res.append(gk.to(P[k].dtype) if gk is not None else None)
        return (None, *res)


def head_outputs(model, images: Tensor):
    """the training forward: {'cls_logits', 'bbox_regression'} with a grad_fn that reaches the head parameters of `model`"""
    g = model.graph
    ents = entries(g)
    dev = images.device
    handle = model._plan(dev, heads_may_differ=True)
    n, _, h, w = images.shape
    b = model._buffers_for(n, h, w, dev)
    b["images"].copy_(images)
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ws = b["ws"]
    with torch.cuda.device(dev):
        _lib.check(L.dn_forward_features(C.c_void_p(handle), _P(b["images"]), n, h, w, _P(ws), ws.numel(), C.c_void_p(stream)), "dn_forward_features")
    model._feat_gen += 1
    chains = model.batch_split(n)
    pieces = []
    for lvl, f in enumerate(g.features):
        t = g.t(f)
        lv = []
        for k in range(chains):
            p, first, im = C.c_void_p(), C.c_int(), C.c_int()
            _lib.check(L.dn_level_features(C.c_void_p(handle), _P(ws), n, lvl, k, C.byref(p), C.byref(first), C.byref(im)), "dn_level_features")
            off = p.value - ws.data_ptr()
            lv.append((ws[off:off + im.value * t.h * t.w * t.c * 2].view(torch.float16).view(im.value, t.h, t.w, t.c), first.value, im.value))
        pieces.append(lv)
    named = dict(model.named_parameters())
    params = [named[k] for k in parameter_names(g)]
    logits, reg = _LiteHeads.apply(_Step(model, n, ents, pieces, model._feat_gen), *params)
    return {"cls_logits": logits, "bbox_regression": reg}
