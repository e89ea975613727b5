"""Object crops from video surfaces on the device, behind the tracker.

An `ObjectCropper` cuts the boxes of every stream out of the frames of a `FrameBatch` at native resolution and hands them on as fixed-size
normalised patches -- the input of a second model: a re-identification embedder, an attribute or plate classifier, a face model. The boxes
never visit the host and no frame is converted: two small launches (include/demonet_hip.h, dn_crop_objects, has the rules) turn boxes into
rectangles clamped to the frame, compact the valid ones into patch slots, and gather the patches from the surfaces with the arithmetic of
`SSD.forward_regions`, followed by torchvision `Normalize`'s `(v - mean) / std`.

    cropper = ObjectCropper(streams, "cuda:0", size=(128, 64))
    boxes, scores, labels, ids, det, counts, det_ids = model.track_sliced_frames(batch, tracker, slicer)
    patches, index, totals = cropper(batch, boxes, counts)       # [capacity, 3, 128, 64] fp16, [capacity, 8] int32, [4] int32
    patch_ids = cropper.gather(ids)                              # the track id of every patch slot

`totals` is (kept, dropped, 0, 0); index row s < kept is (stream, row, x0, y0, width, height, 0, 0), the rows beyond are (-1, 0, ...). Patches
beyond `kept` are NOT written and hold stale data. Everything stays on the device: a captured step replays, and the host reads `totals` when it
wants to, or never. There is no CPU fallback.
"""
import ctypes as C
import math
from typing import Optional

import torch
from torch import Tensor

from . import _lib
from .frames import FrameBatch

MAX_STREAMS, MAX_D, MAX_SIZE, MAX_CAPACITY = 1024, 512, 1024, 8192
DTYPES = (torch.float16, torch.float32)


def _int(v, what, lo, hi):
    if not isinstance(v, int) or isinstance(v, bool):
        raise ValueError("ObjectCropper: {} must be an int, got {!r}".format(what, v))
    if v < lo or v > hi:
        raise ValueError("ObjectCropper: {} = {}, it takes {} .. {}".format(what, v, lo, hi))
    return v


def _pair(v, what, lo, hi):
    if not isinstance(v, (tuple, list)) or len(v) != 2:
        raise ValueError("ObjectCropper: {} must be a pair, got {!r}".format(what, v))
    return _int(v[0], what + "[0]", lo, hi), _int(v[1], what + "[1]", lo, hi)


def _triple(v, what):
    if not isinstance(v, (tuple, list)) or len(v) != 3:
        raise ValueError("ObjectCropper: {} must hold three numbers (R, G, B), got {!r}".format(what, v))
    out = []
    for x in v:
        try:
            x = float(x)
        except (TypeError, ValueError):
            raise ValueError("ObjectCropper: {} must hold three numbers (R, G, B), got {!r}".format(what, v))
        if not math.isfinite(x) or not math.isfinite(C.c_float(x).value):
            raise ValueError("ObjectCropper: {} must be finite in fp32, got {!r}".format(what, v))
        out.append(x)
    return tuple(out)


def crop_params(size=(128, 64), capacity=1024, dtype=torch.float16, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), margin=0.0,
                square=False, min_size=(1, 1)) -> "_lib.CropParams":
    """The validated dn_crop_params of an ObjectCropper's arguments; ValueError otherwise. Host work only."""
    h, w = _pair(size, "size (height, width)", 1, MAX_SIZE)
    capacity = _int(capacity, "capacity", 1, MAX_CAPACITY)
    if dtype not in DTYPES:
        raise ValueError("ObjectCropper: dtype must be torch.float16 or torch.float32, got {!r}".format(dtype))
    mean, std = _triple(mean, "mean"), _triple(std, "std")
    if any(C.c_float(s).value <= 0.0 for s in std):
        raise ValueError("ObjectCropper: std must be positive in fp32, got {!r}".format(std))
    try:
        margin = float(margin)
    except (TypeError, ValueError):
        raise ValueError("ObjectCropper: margin must be a number, got {!r}".format(margin))
    if not math.isfinite(margin) or margin < 0.0 or not math.isfinite(C.c_float(margin).value):
        raise ValueError("ObjectCropper: margin must be finite and >= 0, got {!r}".format(margin))
    if not isinstance(square, bool):
        raise ValueError("ObjectCropper: square must be a bool, got {!r}".format(square))
    min_h, min_w = _pair(min_size, "min_size (height, width)", 1, 2 ** 31 - 1)
    p = _lib.CropParams()
    p.margin, p.square, p.min_width, p.min_height = margin, int(square), min_w, min_h
    for c in range(3):
        p.mean[c], p.std[c] = mean[c], std[c]
    p.out_h, p.out_w, p.out_fp16, p.capacity = h, w, int(dtype == torch.float16), capacity
    return p


def check_step(streams: int, device, batch, boxes, counts, select=None) -> int:
    """What a step of a cropper of `streams` streams on `device` checks before anything reaches the device (host work only); returns d. ValueError
    otherwise."""
    if not isinstance(batch, FrameBatch):
        raise ValueError("ObjectCropper: expected a FrameBatch, got {}".format(type(batch).__name__))
    if batch.n != streams:
        raise ValueError("ObjectCropper: a FrameBatch of {} frames, the cropper has {} streams".format(batch.n, streams))
    if batch.device != device:
        raise ValueError("ObjectCropper: the FrameBatch is on {}, the cropper on {}".format(batch.device, device))
    if batch.table is None:
        raise ValueError("ObjectCropper: the FrameBatch names no frames yet: call set() first")
    if not isinstance(boxes, Tensor) or boxes.dim() != 3 or boxes.shape[2] != 4:
        raise ValueError("ObjectCropper: boxes must be [B, d, 4], got {}".format(tuple(boxes.shape) if isinstance(boxes, Tensor) else type(boxes)))
    B, d = int(boxes.shape[0]), int(boxes.shape[1])
    if B != streams:
        raise ValueError("ObjectCropper: {} streams of boxes, the cropper has {}".format(B, streams))
    if d < 1 or d > MAX_D:
        raise ValueError("ObjectCropper: {} rows per stream, the cropper takes 1 .. {}".format(d, MAX_D))
    dev = device
    for t, shape, dtypes in ((boxes, (B, d, 4), (torch.float32,)), (counts, (B,), (torch.int32,))) + (
            ((select, (B, d), (torch.uint8, torch.bool)),) if select is not None else ()):
        if not isinstance(t, Tensor) or tuple(t.shape) != shape or t.dtype not in dtypes or not t.is_contiguous() or t.device != dev:
            raise ValueError("ObjectCropper: expected a contiguous {} tensor of shape {} on {}, got {}".format(
                " or ".join(str(x) for x in dtypes), shape, dev, "{} {} on {}".format(t.dtype, tuple(t.shape), t.device) if isinstance(t, Tensor) else type(t)))
    return d


class ObjectCropper:
    """Patches of the objects of `streams` video streams; owns the patch, index, totals and workspace tensors on `device`. Their addresses are fixed
    for the life of the object, so a captured step replays.

    size: (height, width) of a patch, 1 .. 1024 each. capacity: patch slots, 1 .. 8192; what survives beyond them is counted in totals[1].
    dtype: torch.float16 (round to nearest even of the fp32 value) or torch.float32. mean, std: per channel R, G, B; the stored value is
    (v - mean) / std of the resized 0 .. 1 pixel. margin: the box grows by margin * its width (height) on each side. square: afterwards the shorter
    side grows to the longer one about the centre. min_size: (height, width); rectangles smaller than this after clamping to the frame are skipped."""

    def __init__(self, streams: int, device, size=(128, 64), capacity: int = 1024, dtype=torch.float16, mean=(0.485, 0.456, 0.406),
                 std=(0.229, 0.224, 0.225), margin: float = 0.0, square: bool = False, min_size=(1, 1)):
        self.streams = _int(streams, "streams", 1, MAX_STREAMS)
        self.params = crop_params(size, capacity, dtype, mean, std, margin, square, min_size)
        self.size, self.capacity, self.dtype = (self.params.out_h, self.params.out_w), self.params.capacity, dtype
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("demonet_amd runs on an MI355X only (the cropper must be on a cuda device); there is no CPU fallback path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        dev = self.device
        self.patches = torch.empty((self.capacity, 3) + self.size, dtype=dtype, device=dev)
        self.index = torch.empty((self.capacity, 8), dtype=torch.int32, device=dev)
        self.totals = torch.zeros((4,), dtype=torch.int32, device=dev)
        self.index.zero_()
        self.index[:, 0] = -1                # (no step yet: no slot is kept)
        self._ws = {}                        # rows per stream -> the workspace of that d

    def _stream(self, stream):
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        return C.c_void_p(s.cuda_stream if hasattr(s, "cuda_stream") else int(s))

    def __call__(self, batch: FrameBatch, boxes: Tensor, counts: Tensor, select: Optional[Tensor] = None, stream=None):
        """One step: frame b of the batch is the current frame of stream b; boxes [B, d, 4] contiguous fp32 in frame pixels (the tracker's boxes, or a
        forward's), counts [B] int32, select [B, d] uint8 or bool or None (rows whose byte is 0 are skipped), all on the cropper's device, B = streams
        = batch.n. Enqueued on `stream` (default: the current stream); no device-to-host copy. Returns (patches [capacity, 3, h, w], index
        [capacity, 8] int32, totals [4] int32): the cropper's own tensors, overwritten by the next step. Patches at or beyond totals[0] are not
        written."""
        d = check_step(self.streams, self.device, batch, boxes, counts, select)
        L = _lib.lib()
        ws = self._ws.get(d)
        if ws is None:
            ws = self._ws[d] = torch.empty(L.dn_crop_workspace_bytes(self.streams, d), dtype=torch.uint8, device=self.device)
        p = C.c_void_p
        with torch.cuda.device(self.device):
            _lib.check(L.dn_crop_objects(p(batch.table.data_ptr()), batch.format_code, batch.color_code, p(boxes.data_ptr()), p(counts.data_ptr()),
                                         p(select.data_ptr()) if select is not None else None, self.streams, d, C.byref(self.params),
                                         p(self.patches.data_ptr()), p(self.index.data_ptr()), p(self.totals.data_ptr()), p(ws.data_ptr()),
                                         ws.numel(), self._stream(stream)), "dn_crop_objects")
        return self.patches, self.index, self.totals

    def gather(self, t: Tensor) -> Tensor:
        """The values of a [B, d, ...] device tensor (the tracker's ids, labels or scores) for every patch slot, by the index table of the last
        step: [capacity, ...], built with indexing on the device, without synchronising. ROWS AT OR BEYOND totals[0] TAKE ROW (0, 0)'S VALUE AND
        ARE MEANINGLESS."""
        if not isinstance(t, Tensor) or t.dim() < 2 or t.shape[0] != self.streams or t.device != self.device:
            raise ValueError("ObjectCropper.gather: expected a [{}, d, ...] tensor on {}, got {}".format(
                self.streams, self.device, "{} on {}".format(tuple(t.shape), t.device) if isinstance(t, Tensor) else type(t)))
        b = self.index[:, 0].clamp(min=0).long()
        j = self.index[:, 1].clamp(min=0, max=t.shape[1] - 1).long()
        return t[b, j]


def crop_objects(model, batch, cropper, boxes, counts, select=None):
    """SSD.crop_objects (see there)."""
    if not isinstance(cropper, ObjectCropper):
        raise ValueError("crop_objects: cropper must be an ObjectCropper, got {}".format(type(cropper)))
    mdev = next(model.parameters()).device
    if mdev != cropper.device:
        raise ValueError("crop_objects: the cropper is on {}, the model on {}".format(cropper.device, mdev))
    return cropper(batch, boxes, counts, select)
