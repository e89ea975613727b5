"""Sliced inference: detection on images much larger than the network size.

Every model here resizes its input to a small fixed size first, so a small object of a full-HD frame reaches the network below the smallest default
box. `detect_sliced` runs the detector on overlapping tiles at native resolution (and, optionally, on the whole image as well), shifts the per-tile
detections into image coordinates and merges them with one more hard NMS. The tiles are cut by one gather launch (dn_crop_tiles) straight into the
model's input buffer, a batch of tiles is one forward, and the merge (dn_merge_detections) runs on the device on the arrays the forwards wrote:
between the image and the result there is one device-to-host copy, the merged counts.

`merge_detections` is the general piece: an NMS over detections that already exist, per class or class-agnostic, for any set of sources with one
offset each (tiles, flipped passes, several models).

`FrameSlicer` is the same on video surfaces: the tiles and the whole-frame passes are regions of a frames.FrameBatch, read by the
forward's first kernel, the regions of all frames share forwards, and the merged detections stay padded on the device (no host copy at all),
ready for ByteTracker.update.
"""
import ctypes as C
from typing import List, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib

MAX_D = 512                 # rows per source, and rows per merged image
MAX_SOURCES = 1024          # sources per output image
MAX_SLOTS = 65536           # sources * rows per output image


def _axis(extent: int, tile: int, overlap: float) -> List[int]:
    stride = max(1, tile - int(round(overlap * tile)))
    out, x = [], 0
    while x + tile < extent:
        out.append(x)
        x += stride
    out.append(extent - tile)      # the last origin is clamped: every tile has the same size and lies inside the image
    return out


def tile_grid(H: int, W: int, th: int, tw: int, overlap: float = 0.25) -> Tuple[List[Tuple[int, int]], int, int]:
    """The tiles of an H x W image: (origins [(x0, y0), ...] in row-major order, th', tw') with th' = min(th, H), tw' = min(tw, W). Per axis the
    stride is tile - round(overlap * tile) (Python's round: halves go to the even integer), at least 1; origins are 0, stride, 2 stride, ... and
    the last one is clamped to extent - tile. 500 x 700, tile 320, overlap 0.25: xs [0, 240, 380], ys [0, 180], 6 tiles."""
    H, W, th, tw = int(H), int(W), int(th), int(tw)
    if H < 1 or W < 1 or th < 1 or tw < 1:
        raise ValueError("tile_grid: sizes must be positive, got H={} W={} th={} tw={}".format(H, W, th, tw))
    if not (0.0 <= overlap < 1.0):
        raise ValueError("tile_grid: overlap must be in [0, 1), got {!r}".format(overlap))
    th, tw = min(th, H), min(tw, W)
    xs, ys = _axis(W, tw, overlap), _axis(H, th, overlap)
    return [(x, y) for y in ys for x in xs], th, tw


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def crop_tiles(image: Tensor, origins: Tensor, th: int, tw: int, out: Tensor = None) -> Tensor:
    """image [3, H, W] fp32 contiguous on the GPU, origins [t, 2] int32 (x0, y0) on the same device -> [t, 3, th, tw] (dn_crop_tiles, one launch;
    `out` receives it when given). The call validates the origins on the host: it waits for the current stream."""
    if image.dim() != 3 or image.shape[0] != 3 or image.dtype != torch.float32 or not image.is_contiguous() or image.device.type != "cuda":
        raise ValueError("crop_tiles: image must be a contiguous [3, H, W] float32 tensor on the GPU, got {} {} on {}".format(
            tuple(image.shape), image.dtype, image.device))
    if origins.dim() != 2 or origins.shape[1] != 2 or origins.dtype != torch.int32 or not origins.is_contiguous() or origins.device != image.device:
        raise ValueError("crop_tiles: origins must be a contiguous [t, 2] int32 tensor on {}".format(image.device))
    t = origins.shape[0]
    if out is None:
        out = torch.empty((t, 3, th, tw), dtype=torch.float32, device=image.device)
    elif tuple(out.shape) != (t, 3, th, tw) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != image.device:
        raise ValueError("crop_tiles: out must be a contiguous float32 tensor of shape {} on {}".format((t, 3, th, tw), image.device))
    with torch.cuda.device(image.device):
        _lib.check(_lib.lib().dn_crop_tiles(C.c_void_p(image.data_ptr()), image.shape[1], image.shape[2], C.c_void_p(origins.data_ptr()), t, th, tw,
                                            C.c_void_p(out.data_ptr()), _stream(image.device)), "dn_crop_tiles")
    return out


def check_merge_limits(sources: int, d: int, what: str = "merge"):
    if d > MAX_D:
        raise ValueError("{}: {} rows per source, the merge takes at most {}".format(what, d, MAX_D))
    if sources > MAX_SOURCES:
        raise ValueError("{}: {} sources for one image, the merge takes at most {}".format(what, sources, MAX_SOURCES))
    if sources * d > MAX_SLOTS:
        raise ValueError("{}: {} sources x {} rows = {} slots for one image, the merge takes at most {}".format(what, sources, d, sources * d, MAX_SLOTS))


# What merge_detections and fusion.fuse_detections check and allocate alike: S sources of d rows, grouped per output image by group_begin.
def _check_tensors(what: str, want, dev):
    """want: (tensor, shape, dtype) triples; every tensor contiguous, of that shape and dtype, on the GPU `dev`."""
    for t, shape, dtype in want:
        if not isinstance(t, Tensor) or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev or dev.type != "cuda":
            raise ValueError("{}: expected a contiguous {} tensor of shape {} on the GPU, got {}".format(
                what, dtype, shape, "{} {} on {}".format(t.dtype, tuple(t.shape), t.device) if isinstance(t, Tensor) else type(t)))


def _check_groups(what: str, group_begin: Sequence[int], S: int, d_out: int) -> Tuple[List[int], int]:
    """-> (group_begin as ints, the sources of the largest group)"""
    gb = [int(x) for x in group_begin]
    if len(gb) < 2 or d_out < 1 or gb[0] < 0 or gb[-1] > S or any(a > b for a, b in zip(gb, gb[1:])):
        raise ValueError("{}: group_begin must hold groups + 1 ascending source indices in 0 .. {}, d_out >= 1".format(what, S))
    return gb, max(b - a for a, b in zip(gb, gb[1:]))


def _padded_outputs(G: int, d_out: int, dev, extra: bool):
    """-> boxes [G, d_out, 4], scores [G, d_out], labels [G, d_out], counts [G], and an int32 [G, d_out] (src, members) or None"""
    return (torch.empty((G, d_out, 4), dtype=torch.float32, device=dev), torch.empty((G, d_out), dtype=torch.float32, device=dev),
            torch.empty((G, d_out), dtype=torch.int64, device=dev), torch.empty((G,), dtype=torch.int32, device=dev),
            torch.empty((G, d_out), dtype=torch.int32, device=dev) if extra else None)


def _check_images(what: str, imgs):
    for img in imgs:
        if not isinstance(img, Tensor) or img.dim() != 3 or img.shape[0] != 3 or not img.is_floating_point():
            raise ValueError("{}: images must be [3, H, W] float tensors, got {}".format(
                what, (tuple(img.shape), img.dtype) if isinstance(img, Tensor) else type(img)))
        if img.device != imgs[0].device:
            raise ValueError("{}: all images must be on one device".format(what))


def merge_detections(boxes: Tensor, scores: Tensor, labels: Tensor, counts: Tensor, offsets: Tensor, group_begin: Sequence[int], thresh: float,
                     metric: str = "iou", class_agnostic: bool = False, d_out: int = None, return_src: bool = False):
    """dn_merge_detections on tensors: boxes [S, d, 4] fp32, scores [S, d] fp32, labels [S, d] int64, counts [S] int32 (what forward_batch returns,
    for S sources), offsets [S, 2] fp32 (ox, oy), group_begin: groups + 1 ascending source indices (a host sequence). Returns padded device tensors
    (boxes [G, d_out, 4], scores [G, d_out], labels [G, d_out], counts [G] int32[, src [G, d_out] int32]); semantics: include/demonet_hip.h."""
    if metric not in _lib.DN_MERGE:
        raise ValueError("merge_detections: metric must be one of {}, got {!r}".format(sorted(_lib.DN_MERGE), metric))
    S, d = scores.shape
    d_out = d if d_out is None else int(d_out)
    dev = scores.device
    _check_tensors("merge_detections", ((boxes, (S, d, 4), torch.float32), (scores, (S, d), torch.float32), (labels, (S, d), torch.int64),
                                        (counts, (S,), torch.int32), (offsets, (S, 2), torch.float32)), dev)
    gb, largest = _check_groups("merge_detections", group_begin, S, d_out)
    G = len(gb) - 1
    check_merge_limits(largest, max(d, d_out), "merge_detections")
    L = _lib.lib()
    ws = torch.empty(L.dn_merge_detections_workspace_bytes(S, d, G), dtype=torch.uint8, device=dev)
    ob, os_, ol, oc, src = _padded_outputs(G, d_out, dev, return_src)
    p = C.c_void_p
    with torch.cuda.device(dev):
        _lib.check(L.dn_merge_detections(p(boxes.data_ptr()), p(scores.data_ptr()), p(labels.data_ptr()), p(counts.data_ptr()), p(offsets.data_ptr()),
                                         S, d, (C.c_int32 * (G + 1))(*gb), G, _lib.DN_MERGE[metric], float(thresh), int(bool(class_agnostic)), d_out,
                                         p(ob.data_ptr()), p(os_.data_ptr()), p(ol.data_ptr()), p(oc.data_ptr()),
                                         p(src.data_ptr()) if return_src else None, p(ws.data_ptr()), ws.numel(), _stream(dev)), "dn_merge_detections")
    return (ob, os_, ol, oc, src) if return_src else (ob, os_, ol, oc)


def _slice_args(what: str, model, tile, merge_thresh, metric, max_tiles_per_forward):
    """-> (th0, tw0, max_tiles_per_forward, merge threshold) of the arguments detect_sliced and FrameSlicer share; ValueError for a bad one"""
    if tile is None:
        tw0, th0 = model.graph.size
    elif isinstance(tile, int):
        th0 = tw0 = tile
    else:
        th0, tw0 = (int(x) for x in tile)
    if th0 < 1 or tw0 < 1:
        raise ValueError("{}: tile must be positive, got {!r}".format(what, tile))
    if metric not in _lib.DN_MERGE:
        raise ValueError("{}: metric must be one of {}, got {!r}".format(what, sorted(_lib.DN_MERGE), metric))
    max_tiles_per_forward = int(max_tiles_per_forward)
    if max_tiles_per_forward < 1:
        raise ValueError("{}: max_tiles_per_forward must be >= 1, got {}".format(what, max_tiles_per_forward))
    thresh = model.nms_thresh if merge_thresh is None else float(merge_thresh)
    if thresh != thresh:
        raise ValueError("{}: merge_thresh is NaN".format(what))
    return th0, tw0, max_tiles_per_forward, thresh


def detect_sliced(model, images, tile=None, overlap: float = 0.25, full_image: bool = True, merge_thresh: float = None, metric: str = "iou",
                  class_agnostic: bool = False, max_tiles_per_forward: int = 64):
    """SSD.detect_sliced (see there)."""
    if model.training:
        raise ValueError("detect_sliced: the model must be in eval mode")
    single = isinstance(images, Tensor)
    imgs = [images] if single else list(images)
    if not imgs:
        return []
    _check_images("detect_sliced", imgs)
    th0, tw0, max_tiles_per_forward, thresh = _slice_args("detect_sliced", model, tile, merge_thresh, metric, max_tiles_per_forward)
    D = model.detections_per_img
    grids = [tile_grid(img.shape[1], img.shape[2], th0, tw0, overlap) for img in imgs]      # (ValueError for a bad overlap)
    extra = 1 if full_image else 0
    for origins, _, _ in grids:
        check_merge_limits(len(origins) + extra, D, "detect_sliced")
    device = imgs[0].device
    model._plan(device)                                  # (raises off the GPU: there is no CPU path)
    group_begin, all_origins, all_offsets = [0], [], []
    for origins, _, _ in grids:
        all_origins += origins
        all_offsets += [(float(x), float(y)) for x, y in origins] + [(0.0, 0.0)] * extra
        group_begin.append(group_begin[-1] + len(origins) + extra)
    S = group_begin[-1]
    origins_dev = torch.tensor(all_origins, dtype=torch.int32).to(device)
    offsets_dev = torch.tensor(all_offsets, dtype=torch.float32).to(device)
    # staging: the model's output buffers are reused by the next forward of the same shape
    sb = torch.empty((S, D, 4), dtype=torch.float32, device=device)
    ss = torch.empty((S, D), dtype=torch.float32, device=device)
    sl = torch.empty((S, D), dtype=torch.int64, device=device)
    sc = torch.empty((S,), dtype=torch.int32, device=device)
    f32 = torch.float32
    s, o = 0, 0
    for img, (origins, th, tw) in zip(imgs, grids):
        img = img if img.dtype is f32 and img.is_contiguous() else img.to(f32).contiguous()
        for a in range(0, len(origins), max_tiles_per_forward):
            nb = min(max_tiles_per_forward, len(origins) - a)
            b = model._buffers_for(nb, th, tw, device)
            crop_tiles(img, origins_dev[o + a:o + a + nb], th, tw, out=b["images"])      # straight into the forward's own input buffer
            outs = model.forward_batch(b["images"], persistent_input=True)
            for dst, src in zip((sb, ss, sl, sc), outs):
                dst[s:s + nb].copy_(src)
            s += nb
        o += len(origins)
        if full_image:
            outs = model.forward_batch(img.unsqueeze(0))      # dn_forward resizes it and maps its boxes back
            for dst, src in zip((sb, ss, sl, sc), outs):
                dst[s:s + 1].copy_(src)
            s += 1
    boxes, scores, labels, counts = merge_detections(sb, ss, sl, sc, offsets_dev, group_begin, thresh, metric, class_agnostic, D)
    cnt = counts.tolist()                                # the one device->host copy
    return [{"boxes": boxes[g, :c], "scores": scores[g, :c], "labels": labels[g, :c]} for g, c in enumerate(cnt)]


class FrameSlicer:
    """Sliced inference straight from video surfaces, built once per camera layout: sizes = FrameBatch.sizes, one (height, width) per
    frame; the other arguments are detect_sliced's. Holds the tile_grid of every frame, the region table (per frame: its tiles in tile_grid's
    order, then with full_image one whole-frame region), the offsets, group_begin, the staging arrays and the merge workspace.

    slicer(batch) runs ceil(S / max_tiles_per_forward) forwards over ALL S regions of ALL frames (a forward may span frames), merges with one
    dn_merge_detections and returns padded device tensors (boxes [G, D, 4], scores [G, D], labels [G, D] int64, counts [G] int32), G = frames,
    in each frame's pixel coordinates: the slicer's own tensors, overwritten by its next call. No device-to-host copy, no host wait.

    Every forward reads its records from ONE slot table of max_tiles_per_forward records, filled by a device-to-device copy on the stream, and
    writes the model's (n, 0, 0) output buffers, which are then copied into the staging arrays: the plan sees at most two graph keys (the full
    sub-batch and the remainder), however many sub-batches a step has."""

    def __init__(self, model, sizes, tile=None, overlap: float = 0.25, full_image: bool = True, merge_thresh: float = None, metric: str = "iou",
                 class_agnostic: bool = False, max_tiles_per_forward: int = 64):
        what = "FrameSlicer"
        th0, tw0, self.max_tiles_per_forward, self.thresh = _slice_args(what, model, tile, merge_thresh, metric, max_tiles_per_forward)
        self.model, self.metric, self.class_agnostic, self.full_image = model, metric, bool(class_agnostic), bool(full_image)
        self.sizes = [(int(h), int(w)) for h, w in sizes]
        if not self.sizes:
            raise ValueError("FrameSlicer: no frame sizes")
        self.D = D = model.detections_per_img
        self.grids = [tile_grid(h, w, th0, tw0, overlap) for h, w in self.sizes]        # (ValueError for a bad size or overlap)
        extra = 1 if self.full_image else 0
        self.regions, self.offsets, self.group_begin = [], [], [0]
        for f, ((h, w), (origins, th, tw)) in enumerate(zip(self.sizes, self.grids)):
            check_merge_limits(len(origins) + extra, D, what)
            self.regions += [(f, x, y, tw, th, False) for x, y in origins] + [(f, 0, 0, w, h, False)] * extra
            self.offsets += [(float(x), float(y)) for x, y in origins] + [(0.0, 0.0)] * extra
            self.group_begin.append(len(self.regions))
        self.S, self.G = len(self.regions), len(self.sizes)
        from .frames import region_records
        region_records(self.regions, self.sizes, self.S)      # (every region lies inside its frame by construction: checked all the same)
        self.table = None           # the device side: made by the first call

    def _materialise(self, device):
        from .frames import RegionTable
        S, G, D, M = self.S, self.G, self.D, min(self.max_tiles_per_forward, self.S)
        self.table = RegionTable(S, device).set(self.regions, self.sizes)
        self.slot = torch.zeros(M * C.sizeof(_lib.Region), dtype=torch.uint8, device=device)
        self.offsets_dev = torch.tensor(self.offsets, dtype=torch.float32).to(device)
        self.staging = (torch.empty((S, D, 4), dtype=torch.float32, device=device), torch.empty((S, D), dtype=torch.float32, device=device),
                        torch.empty((S, D), dtype=torch.int64, device=device), torch.empty((S,), dtype=torch.int32, device=device))
        self.ws = torch.empty(_lib.lib().dn_merge_detections_workspace_bytes(S, D, G), dtype=torch.uint8, device=device)
        self.outs = _padded_outputs(G, D, device, False)[:4]
        self._gb = (C.c_int32 * (G + 1))(*self.group_begin)

    def __call__(self, batch):
        from .frames import FrameBatch, check_regions, run_regions
        m = self.model
        if m.training:
            raise ValueError("FrameSlicer: the model must be in eval mode")
        if m.detections_per_img != self.D:
            raise ValueError("FrameSlicer: built for detections_per_img = {}, the model now has {}".format(self.D, m.detections_per_img))
        if not isinstance(batch, FrameBatch):
            raise ValueError("FrameSlicer: expected a FrameBatch, got {}".format(type(batch).__name__))
        if batch.table is None:
            raise ValueError("FrameSlicer: the FrameBatch names no frames yet: call set() first")
        if list(batch.sizes) != self.sizes:
            raise ValueError("FrameSlicer: stale sizes: built for frames of {} (height, width), the batch holds {}".format(self.sizes, list(batch.sizes)))
        mdev = next(m.parameters()).device
        if mdev != batch.device:
            raise ValueError("FrameSlicer: the FrameBatch is on {}, the model on {}".format(batch.device, mdev))
        if self.table is None:
            self._materialise(batch.device)
        check_regions("FrameSlicer", m, batch, self.table)
        dev, rb, M = batch.device, C.sizeof(_lib.Region), self.max_tiles_per_forward
        for a in range(0, self.S, M):
            nb = min(M, self.S - a)
            self.slot[:nb * rb].copy_(self.table.table[a * rb:(a + nb) * rb])
            outs = run_regions(m, batch, self.slot.data_ptr(), nb)
            for dst, src in zip(self.staging, outs):
                dst[a:a + nb].copy_(src)
        sb, ss, sl, sc = self.staging
        ob, os_, ol, oc = self.outs
        p = C.c_void_p
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().dn_merge_detections(p(sb.data_ptr()), p(ss.data_ptr()), p(sl.data_ptr()), p(sc.data_ptr()), p(self.offsets_dev.data_ptr()),
                                                      self.S, self.D, self._gb, self.G, _lib.DN_MERGE[self.metric], float(self.thresh),
                                                      int(self.class_agnostic), self.D, p(ob.data_ptr()), p(os_.data_ptr()), p(ol.data_ptr()),
                                                      p(oc.data_ptr()), None, p(self.ws.data_ptr()), self.ws.numel(), _stream(dev)), "dn_merge_detections")
        return self.outs


def detect_sliced_frames(model, batch, tile=None, overlap: float = 0.25, full_image: bool = True, merge_thresh: float = None, metric: str = "iou",
                         class_agnostic: bool = False, max_tiles_per_forward: int = 64):
    """SSD.detect_sliced_frames (see there)."""
    from .frames import FrameBatch
    if not isinstance(batch, FrameBatch):
        raise ValueError("detect_sliced_frames: expected a FrameBatch, got {}".format(type(batch).__name__))
    if batch.table is None:
        raise ValueError("detect_sliced_frames: the FrameBatch names no frames yet: call set() first")
    key = (tuple(batch.sizes), str(batch.device), tile if tile is None or isinstance(tile, int) else tuple(tile), overlap, bool(full_image), merge_thresh,
           metric, bool(class_agnostic), int(max_tiles_per_forward), model.detections_per_img, model.nms_thresh)
    cache = model.__dict__.setdefault("_frame_slicers", {})
    slicer = cache.get(key)
    if slicer is None:
        slicer = FrameSlicer(model, batch.sizes, tile, overlap, full_image, merge_thresh, metric, class_agnostic, max_tiles_per_forward)
        if len(cache) >= 4:
            cache.clear()
        cache[key] = slicer
    boxes, scores, labels, counts = (t.clone() for t in slicer(batch))      # (the slicer's tensors are overwritten by its next call)
    cnt = counts.tolist()                                # the one device->host copy
    return [{"boxes": boxes[g, :c], "scores": scores[g, :c], "labels": labels[g, :c]} for g, c in enumerate(cnt)]


def track_sliced_frames(model, batch, tracker, slicer: FrameSlicer, analytics=None, motion=None, osd=None, compose=None, wall=None, warp=None, source=None,
                        jpeg=None):
    """SSD.track_sliced_frames (see there)."""
    from .warp import check_warping, warped
    from .track import ByteTracker, MAX_D as TRACK_MAX_D, with_analytics
    from .osd import check_overlay, painted
    from .compose import check_composition, composed
    from .jpeg import check_jpeg, encoded
    if not isinstance(tracker, ByteTracker):
        raise ValueError("track_sliced_frames: tracker must be a ByteTracker, got {}".format(type(tracker)))
    if not isinstance(slicer, FrameSlicer) or slicer.model is not model:
        raise ValueError("track_sliced_frames: slicer must be a FrameSlicer of this model")
    if slicer.D > TRACK_MAX_D:
        raise ValueError("track_sliced_frames: detections_per_img = {} rows per frame, the tracker takes at most {}".format(slicer.D, TRACK_MAX_D))
    if analytics is not None:
        from .zones import check_analytics
        check_analytics(analytics, tracker, "track_sliced_frames")
    check_overlay(osd, tracker, "track_sliced_frames")
    check_composition(compose, wall, batch, "track_sliced_frames")
    check_warping(warp, source, batch, "track_sliced_frames")
    check_jpeg(jpeg, wall, batch, "track_sliced_frames")
    if motion is None:
        warped(warp, source, batch)
        return encoded(composed(painted(with_analytics(tracker.update(*slicer(batch)), analytics), osd, batch, analytics), compose, batch, wall),
                       jpeg, wall, batch)
    from .motion import check_motion, compensated
    check_motion(motion, tracker, batch, "track_sliced_frames")
    warped(warp, source, batch)
    boxes, scores, labels, counts = slicer(batch)
    compensated(motion, tracker, batch, boxes, scores, counts)
    return encoded(composed(painted(with_analytics(tracker.update(boxes, scores, labels, counts), analytics), osd, batch, analytics), compose, batch, wall),
                   jpeg, wall, batch)
