"""Weighted boxes fusion on the device: horizontal-flip test-time augmentation and ensembles of models.

`sliced.merge_detections` reduces several sources of one image with one more hard NMS: right for tiles, which see different parts of the image.
When the sources are different opinions about the same objects -- the plain and the mirrored pass, several checkpoints -- the standard reducer is
weighted boxes fusion (Solovyev, Wang, Gabruseva 2019; ensemble_boxes.weighted_boxes_fusion with conf_type 'avg'): overlapping boxes of one label
are averaged with their scores as weights, and a cluster that only some of the sources saw is marked down.

`fuse_detections` is dn_fuse_detections on tensors (include/demonet_hip.h has the semantics); `detect_tta` and `ensemble_detect` run the forwards,
stage their outputs so that the sources of an image are adjacent, and fuse them on the device: between the images and the result there is one
device-to-host copy, the fused counts.
"""
import ctypes as C
import math
from typing import List, Sequence

import torch
from torch import Tensor

from . import _lib
from .sliced import _check_groups, _check_images, _check_tensors, _padded_outputs, _stream, merge_detections

MAX_D = 512                 # rows per source, and rows per fused image
MAX_SLOTS = 8192            # sources * rows per output image (the merge takes 65 536: the fusion walk is quadratic in the worst case)
FUSE_MODES = ("wbf", "nms")


def check_fuse_limits(sources: int, d: int, what: str = "fuse"):
    if d > MAX_D:
        raise ValueError("{}: {} rows per source, the fusion takes at most {}".format(what, d, MAX_D))
    if sources * d > MAX_SLOTS:
        raise ValueError("{}: {} sources x {} rows = {} slots for one image, the fusion takes at most {}".format(what, sources, d, sources * d, MAX_SLOTS))


def _check_thresholds(what: str, thresh: float, skip_thresh: float):
    for name, v in (("thresh", thresh), ("skip_thresh", skip_thresh)):
        if not (v >= 0.0):      # (a NaN compares false)
            raise ValueError("{}: {} must be a number >= 0, got {!r}".format(what, name, v))


def fuse_detections(boxes: Tensor, scores: Tensor, labels: Tensor, counts: Tensor, offsets: Tensor, group_begin: Sequence[int], weights: Tensor = None,
                    thresh: float = 0.55, skip_thresh: float = 0.0, d_out: int = None, return_members: bool = False):
    """dn_fuse_detections on tensors: boxes [S, d, 4] fp32, scores [S, d] fp32, labels [S, d] int64, counts [S] int32 (what forward_batch returns,
    for S sources), offsets [S, 2] fp32 (ox, oy), group_begin: groups + 1 ascending source indices (a host sequence), weights: [S] fp32 on the
    device, one per source (None: all 1). Returns padded device tensors (boxes [G, d_out, 4], scores [G, d_out], labels [G, d_out], counts [G]
    int32[, members [G, d_out] int32 = the number of boxes fused into each row]); semantics: include/demonet_hip.h."""
    if scores.dim() != 2:
        raise ValueError("fuse_detections: scores must be [S, d], got {}".format(tuple(scores.shape)))
    S, d = scores.shape
    d_out = d if d_out is None else int(d_out)
    thresh, skip_thresh = float(thresh), float(skip_thresh)
    _check_thresholds("fuse_detections", thresh, skip_thresh)
    dev = scores.device
    want = [(boxes, (S, d, 4), torch.float32), (scores, (S, d), torch.float32), (labels, (S, d), torch.int64), (counts, (S,), torch.int32),
            (offsets, (S, 2), torch.float32)]
    if weights is not None:
        want.append((weights, (S,), torch.float32))
    _check_tensors("fuse_detections", want, dev)
    gb, largest = _check_groups("fuse_detections", group_begin, S, d_out)
    G = len(gb) - 1
    check_fuse_limits(largest, max(d, d_out), "fuse_detections")
    L = _lib.lib()
    gb_c = (C.c_int32 * (G + 1))(*gb)
    ws = torch.empty(L.dn_fuse_detections_workspace_bytes(S, d, gb_c, G), dtype=torch.uint8, device=dev)
    ob, os_, ol, oc, om = _padded_outputs(G, d_out, dev, return_members)
    p = C.c_void_p
    with torch.cuda.device(dev):
        _lib.check(L.dn_fuse_detections(p(boxes.data_ptr()), p(scores.data_ptr()), p(labels.data_ptr()), p(counts.data_ptr()), p(offsets.data_ptr()),
                                        p(weights.data_ptr()) if weights is not None else None, S, d, gb_c, G, thresh, skip_thresh, d_out,
                                        p(ob.data_ptr()), p(os_.data_ptr()), p(ol.data_ptr()), p(oc.data_ptr()),
                                        p(om.data_ptr()) if return_members else None, p(ws.data_ptr()), ws.numel(), _stream(dev)), "dn_fuse_detections")
    return (ob, os_, ol, oc, om) if return_members else (ob, os_, ol, oc)


def _image_list(what: str, images) -> List[Tensor]:
    if isinstance(images, Tensor):
        if images.dim() != 4:
            raise ValueError("{}: a tensor of images must be [N, 3, H, W], got {}".format(what, tuple(images.shape)))
        imgs = list(images.unbind(0))
    else:
        imgs = list(images)
    _check_images(what, imgs)
    return imgs


def _detect(what: str, model_list, weights, images, hflip: bool, fuse: str, thresh, skip_thresh):
    """The common body of detect_tta and ensemble_detect: sources per image = (plain[, flipped]) per model, in that order."""
    if fuse not in FUSE_MODES:
        raise ValueError("{}: fuse must be one of {}, got {!r}".format(what, FUSE_MODES, fuse))
    for m in model_list:
        if m.training:
            raise ValueError("{}: the models must be in eval mode".format(what))
    P = len(model_list) * (2 if hflip else 1)
    if fuse == "wbf" and P < 2:
        raise ValueError("{}: fuse='wbf' with a single source per image (one model, hflip=False) has nothing to fuse: "
                         "use hflip=True, several models, or fuse='nms'".format(what))
    m0 = model_list[0]
    thresh = float(m0.nms_thresh if thresh is None else thresh)
    skip_thresh = float(m0.score_thresh if skip_thresh is None else skip_thresh)
    _check_thresholds(what, thresh, skip_thresh)
    imgs = _image_list(what, images)
    if not imgs:
        return []
    whole = images if isinstance(images, Tensor) else None      # an [N, 3, H, W] tensor is one size group and needs no stack
    D = m0.detections_per_img
    if fuse == "wbf":
        check_fuse_limits(P, D, what)
    device = imgs[0].device
    for m in model_list:
        m._plan(device)                                  # (raises off the GPU: there is no CPU path)
    G = len(imgs)
    S = G * P
    # staging: the models' output buffers are reused by their next forward; sources g * P .. g * P + P - 1 form group g
    sb = torch.empty((G, P, D, 4), dtype=torch.float32, device=device)
    ss = torch.empty((G, P, D), dtype=torch.float32, device=device)
    sl = torch.empty((G, P, D), dtype=torch.int64, device=device)
    sc = torch.empty((G, P), dtype=torch.int32, device=device)
    by_shape = {}                                        # shape -> indices, in order of first appearance
    for i, img in enumerate(imgs):
        by_shape.setdefault(tuple(img.shape), []).append(i)
    f32 = torch.float32
    for shape, idxs in by_shape.items():
        n, width = len(idxs), float(shape[2])
        nb = 2 * n if hflip else n                       # both passes as one forward of 2 n images
        where = slice(idxs[0], idxs[0] + n) if idxs == list(range(idxs[0], idxs[0] + n)) else torch.tensor(idxs, device=device)
        first = None
        for k, m in enumerate(model_list):
            buf = m._buffers_for(nb, shape[1], shape[2], device)["images"]      # straight into the forward's own input buffer
            if first is None:
                if whole is not None:
                    buf[:n].copy_(whole)
                else:
                    torch.stack([imgs[i] if imgs[i].dtype is f32 else imgs[i].to(f32) for i in idxs], out=buf[:n])
                if hflip:                                # torch.flip(batch, [-1]), written behind the plain images by one gather
                    torch.index_select(buf[:n], 3, torch.arange(shape[2] - 1, -1, -1, device=device), out=buf[n:])
                first = buf
            elif buf is not first:                       # (the same model twice shares its buffer)
                buf.copy_(first)
            ob, os_, ol, oc = m.forward_batch(buf, persistent_input=True)
            p = k * (2 if hflip else 1)
            for dst, src in zip((sb, ss, sl, sc), (ob, os_, ol, oc)):
                dst[where, p] = src[:n]
            if hflip:
                fb = ob[n:]
                sb[where, p + 1] = torch.stack([width - fb[..., 2], fb[..., 1], width - fb[..., 0], fb[..., 3]], -1)      # x1' = W - x2, x2' = W - x1
                for dst, src in zip((ss, sl, sc), (os_, ol, oc)):
                    dst[where, p + 1] = src[n:]
    w_dev = None
    if fuse == "wbf" and weights is not None:
        w_dev = torch.tensor([w for w in weights for _ in range(2 if hflip else 1)] * G, dtype=torch.float32).to(device)
    return _reduce(fuse, sb, ss, sl, sc, G, P, D, w_dev, thresh, skip_thresh, device)


def _reduce(fuse: str, sb, ss, sl, sc, G: int, P: int, D: int, w_dev, thresh: float, skip_thresh: float, device):
    """The staged sources [G, P, ...] of G images (sources g * P .. g * P + P - 1 form group g) -> the fused or merged per-image results"""
    S = G * P
    sb, ss, sl, sc = sb.view(S, D, 4), ss.view(S, D), sl.view(S, D), sc.view(S)
    offsets = torch.zeros((S, 2), dtype=torch.float32, device=device)
    group_begin = list(range(0, S + 1, P))
    if fuse == "wbf":
        boxes, scores, labels, counts = fuse_detections(sb, ss, sl, sc, offsets, group_begin, w_dev, thresh, skip_thresh, D)
    else:
        boxes, scores, labels, counts = merge_detections(sb, ss, sl, sc, offsets, group_begin, thresh, "iou", False, D)
    cnt = counts.tolist()                                # the one device->host copy
    return [{"boxes": boxes[g, :c], "scores": scores[g, :c], "labels": labels[g, :c]} for g, c in enumerate(cnt)]


def detect_tta(model, images, hflip: bool = True, fuse: str = "wbf", thresh: float = None, skip_thresh: float = None):
    """SSD.detect_tta (see there)."""
    return _detect("detect_tta", [model], None, images, bool(hflip), fuse, thresh, skip_thresh)


def detect_tta_frames(model, batch, fuse: str = "wbf", thresh: float = None, skip_thresh: float = None):
    """SSD.detect_tta_frames (see there)."""
    from .frames import FrameBatch, RegionTable, forward_regions
    what = "detect_tta_frames"
    if fuse not in FUSE_MODES:
        raise ValueError("{}: fuse must be one of {}, got {!r}".format(what, FUSE_MODES, fuse))
    if model.training:
        raise ValueError("{}: the models must be in eval mode".format(what))
    if not isinstance(batch, FrameBatch):
        raise ValueError("{}: expected a FrameBatch, got {}".format(what, type(batch).__name__))
    if batch.table is None:
        raise ValueError("{}: the FrameBatch names no frames yet: call set() first".format(what))
    thresh = float(model.nms_thresh if thresh is None else thresh)
    skip_thresh = float(model.score_thresh if skip_thresh is None else skip_thresh)
    _check_thresholds(what, thresh, skip_thresh)
    D, G, device = model.detections_per_img, batch.n, batch.device
    if fuse == "wbf":
        check_fuse_limits(2, D, what)
    # per camera layout: the 2 G regions -- every frame whole, then every frame whole and mirrored -- and the frames' widths for the map-back
    cache = model.__dict__.setdefault("_tta_tables", {})
    key = (tuple(batch.sizes), str(device))
    entry = cache.get(key)
    if entry is None:
        regions = [(g, 0, 0, w, h, flip) for flip in (False, True) for g, (h, w) in enumerate(batch.sizes)]
        if len(cache) >= 4:
            cache.clear()
        entry = cache[key] = (RegionTable(2 * G, device).set(regions, batch.sizes),
                              torch.tensor([float(w) for _, w in batch.sizes], dtype=torch.float32).to(device)[:, None])
    table, width = entry
    ob, os_, ol, oc = forward_regions(model, batch, table)       # both passes as one forward of 2 G images
    sb = torch.empty((G, 2, D, 4), dtype=torch.float32, device=device)
    ss = torch.empty((G, 2, D), dtype=torch.float32, device=device)
    sl = torch.empty((G, 2, D), dtype=torch.int64, device=device)
    sc = torch.empty((G, 2), dtype=torch.int32, device=device)
    for dst, src in zip((sb, ss, sl, sc), (ob, os_, ol, oc)):
        dst[:, 0] = src[:G]
        if dst is not sb:
            dst[:, 1] = src[G:]
    fb = ob[G:]
    sb[:, 1] = torch.stack([width - fb[..., 2], fb[..., 1], width - fb[..., 0], fb[..., 3]], -1)      # x1' = W - x2, x2' = W - x1
    return _reduce(fuse, sb, ss, sl, sc, G, 2, D, None, thresh, skip_thresh, device)


def ensemble_detect(model_list, images, weights: Sequence[float] = None, hflip: bool = False, fuse: str = "wbf", thresh: float = None,
                    skip_thresh: float = None):
    """Detections of several models on the same images, fused per image on the device. models: SSD models in eval mode on one device with the same
    num_classes and detections_per_img (network sizes and architectures may differ). Per image there is one source per model (two with hflip: the
    plain pass and the mirrored one, mapped back), in the order of `models`. weights: one positive number per model (None: all 1), applied to that
    model's sources. fuse="wbf": weighted boxes fusion (dn_fuse_detections; thresh defaults to the first model's nms_thresh, skip_thresh to its
    score_thresh), where the weights scale the scores before the skip test and a cluster seen by sources of total weight below the sum of all
    weights is marked down; fuse="nms": one more hard NMS per class (dn_merge_detections; the weights are not used). Returns one {"boxes",
    "scores", "labels"} per image, in the input order, at most detections_per_img each; one device-to-host copy. ValueError for bad arguments,
    mismatched models, and fuse="wbf" with one model and hflip=False (a single source has nothing to fuse)."""
    model_list = list(model_list)
    if not model_list:
        raise ValueError("ensemble_detect: no model")
    m0 = model_list[0]
    for m in model_list[1:]:
        if m.graph.num_classes != m0.graph.num_classes or m.detections_per_img != m0.detections_per_img:
            raise ValueError("ensemble_detect: the models must share num_classes and detections_per_img, got ({}, {}) and ({}, {})".format(
                m0.graph.num_classes, m0.detections_per_img, m.graph.num_classes, m.detections_per_img))
    if weights is not None:
        weights = [float(w) for w in weights]
        if len(weights) != len(model_list) or not all(math.isfinite(w) and w > 0.0 for w in weights):
            raise ValueError("ensemble_detect: weights must be one positive finite number per model ({}), got {!r}".format(len(model_list), weights))
    return _detect("ensemble_detect", model_list, weights, images, bool(hflip), fuse, thresh, skip_thresh)
