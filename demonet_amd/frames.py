"""Video frames as the detector's input: NV12 / I420 / pitched RGB or BGR surfaces, one allocation and one size per frame.

Decoders do not produce the packed [n][h][w][3] block of `SSD.forward_uint8`: a hardware decoder returns one NV12 surface per frame with a
row pitch wider than the width, a software decoder I420 planes, OpenCV pitched BGR. A `FrameBatch` describes n such surfaces in a table of
48-byte records in device memory (include/demonet_hip.h, dn_frame); `SSD.forward_frames` runs the forward on them: the first kernel reads
the records, converts each bilinear tap of the resize to 8-bit RGB in the integer arithmetic the header fixes, and writes the network
input -- no converted frame, no stacked block, and frames of different sizes in one batch.

    batch = FrameBatch(4, "cuda:0", format="nv12", matrix="bt709")
    batch.set(surfaces)                       # per frame: one [h*3/2, w] tensor, or a tuple of plane tensors (row-strided views are fine)
    boxes, scores, labels, counts = model.forward_frames(batch)

The library trusts the records (it cannot inspect a device table), so `set` validates every plane on the host first: dtype, device, the
shapes against the frame's width and height, pitch >= payload, and that the plane's last byte lies inside the tensor's storage.

A `RegionTable` names rectangles of those frames, optionally mirrored, as the network's images (dn_region): `SSD.forward_regions`
runs the forward on them -- the tiles of sliced inference and the passes of flip TTA without a converted frame (sliced.FrameSlicer,
SSD.detect_sliced_frames, SSD.detect_tta_frames). Every region is validated against its frame's size before its record goes up, and a
forward refuses a table whose frames have changed size since.

    table = RegionTable(3, "cuda:0").set([(0, 0, 0, 320, 320), (0, 240, 0, 320, 320), (1, 0, 0, 1920, 1080, True)], batch.sizes)
    boxes, scores, labels, counts = model.forward_regions(batch, table)        # boxes in each region's own coordinates
"""
import ctypes as C
from typing import List, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib

FORMATS = tuple(_lib.DN_FRAME)
MATRICES = tuple(_lib.DN_COLOR)
_PLANE_NAMES = {"nv12": ("Y", "UV"), "i420": ("Y", "U", "V"), "rgb24": ("RGB",), "bgr24": ("BGR",)}
_INT32_MAX = 2 ** 31 - 1


def codes(format: str, matrix: str, full_range: bool) -> Tuple[int, int]:
    """(DN_FRAME_*, DN_COLOR_* | DN_COLOR_FULL_RANGE) of the names; ValueError for an unknown one."""
    if not isinstance(format, str) or format not in _lib.DN_FRAME:
        raise ValueError("format must be one of {}, got {!r}".format(FORMATS, format))
    if not isinstance(matrix, str) or matrix not in _lib.DN_COLOR:
        raise ValueError("matrix must be one of {}, got {!r}".format(MATRICES, matrix))
    return _lib.DN_FRAME[format], _lib.DN_COLOR[matrix] | (_lib.DN_COLOR_FULL_RANGE if full_range else 0)


def _plane(t, i: int, name: str, device, rows: int, payload: int, inner=None):
    """(address, pitch) of one plane: `rows` rows of `payload` bytes. t: [rows, payload] uint8, or [rows, payload / inner, inner] with the two
    last dimensions dense; stride(0) is the pitch."""
    where = "frame {}, plane {}".format(i, name)
    if not isinstance(t, Tensor):
        raise ValueError("{}: expected a tensor, got {}".format(where, type(t).__name__))
    if t.dtype != torch.uint8:
        raise ValueError("{}: expected uint8, got {}".format(where, t.dtype))
    if t.device != device:
        raise ValueError("{}: the plane is on {}, the batch on {}".format(where, t.device, device))
    shapes = [(rows, payload)] + ([(rows, payload // inner, inner)] if inner else [])
    if tuple(t.shape) not in shapes:
        raise ValueError("{}: shape {} does not fit the frame, expected {}".format(where, tuple(t.shape), " or ".join(str(s) for s in shapes)))
    if t.stride(-1) != 1 or (t.dim() == 3 and t.stride(1) != inner):
        raise ValueError("{}: the bytes of a row must be contiguous, got strides {}".format(where, tuple(t.stride())))
    pitch = t.stride(0) if rows > 1 else payload        # (the stride of a single row is never used)
    if pitch < payload:
        raise ValueError("{}: pitch {} is smaller than the row's {} bytes".format(where, pitch, payload))
    if pitch > _INT32_MAX:
        raise ValueError("{}: pitch {} does not fit the record's int32".format(where, pitch))
    end = t.storage_offset() + (rows - 1) * pitch + payload
    have = t.untyped_storage().nbytes()
    if end > have:
        raise ValueError("{}: the plane ends at byte {} of a storage of {} bytes".format(where, end, have))
    return t.data_ptr(), pitch


def frame_records(frames: Sequence, format: str, device, n: int):
    """The validated dn_frame records of `frames` as a ctypes array of n _lib.Frame; ValueError naming the frame and the plane otherwise.
    Host work only: nothing here touches the device."""
    if format not in _lib.DN_FRAME:
        raise ValueError("format must be one of {}, got {!r}".format(FORMATS, format))
    device = torch.device(device)
    if isinstance(frames, Tensor) or not isinstance(frames, (list, tuple)):
        raise ValueError("expected a list of {} frames, got {}".format(n, type(frames).__name__))
    if len(frames) != n:
        raise ValueError("expected {} frames, got {}".format(n, len(frames)))
    names = _PLANE_NAMES[format]
    rec = (_lib.Frame * n)()
    for i, fr in enumerate(frames):
        yuv = format in ("nv12", "i420")
        if isinstance(fr, Tensor) and yuv:
            # the contiguous form: [h * 3 / 2, w], the planes one behind the other
            where = "frame {}".format(i)
            if fr.dim() != 2 or not fr.is_contiguous():
                raise ValueError("{}: the single-tensor form is a contiguous [h * 3 / 2, w] tensor, got shape {} strides {}; pass a tuple of planes "
                                 "for anything else".format(where, tuple(fr.shape), tuple(fr.stride())))
            rows, w = fr.shape
            if rows % 3 != 0 or rows == 0 or w == 0 or w % 2 != 0:      # (h = 2 * rows / 3: rows % 3 == 0 is "h is even")
                raise ValueError("{}: a [h * 3 / 2, w] tensor needs even h and w, got shape {}".format(where, tuple(fr.shape)))
            h = rows // 3 * 2
            flat = fr.reshape(-1)
            y = flat[:h * w].view(h, w)
            if format == "nv12":
                planes = (y, flat[h * w:].view(h // 2, w))
            else:
                q = (h // 2) * (w // 2)
                planes = (y, flat[h * w:h * w + q].view(h // 2, w // 2), flat[h * w + q:].view(h // 2, w // 2))
        elif isinstance(fr, Tensor):
            planes = (fr,)
        elif isinstance(fr, (list, tuple)):
            planes = tuple(fr)
        else:
            raise ValueError("frame {}: expected a tensor or a tuple of plane tensors, got {}".format(i, type(fr).__name__))
        if len(planes) != len(names):
            raise ValueError("frame {}: {} has {} plane(s) ({}), got {}".format(i, format, len(names), ", ".join(names), len(planes)))
        p0 = planes[0]
        if not isinstance(p0, Tensor) or p0.dim() != (2 if yuv else 3):
            raise ValueError("frame {}, plane {}: expected a {} tensor, got {}".format(
                i, names[0], "[h, w]" if yuv else "[h, w, 3]", tuple(p0.shape) if isinstance(p0, Tensor) else type(p0).__name__))
        h, w = int(p0.shape[0]), int(p0.shape[1])
        if h < 1 or w < 1 or h > _INT32_MAX or w > _INT32_MAX // 3:
            raise ValueError("frame {}, plane {}: bad size {} x {}".format(i, names[0], h, w))
        ch, cw = (h + 1) // 2, (w + 1) // 2
        if format == "nv12":
            spec = ((h, w, None), (ch, 2 * cw, 2))
        elif format == "i420":
            spec = ((h, w, None), (ch, cw, None), (ch, cw, None))
        else:
            spec = ((h, 3 * w, 3),)
        r = rec[i]
        for j, (t, (rows, payload, inner)) in enumerate(zip(planes, spec)):
            r.plane[j], r.pitch[j] = _plane(t, i, names[j], device, rows, payload, inner)
        r.width, r.height = w, h
    return rec


class FrameBatch:
    """n video surfaces as one forward's input; owns the table of n dn_frame records in device memory.

    format: "nv12" (Y plane + interleaved UV), "i420" (Y, U, V planes), "rgb24" / "bgr24" (packed pixels). matrix / full_range: how YUV
    becomes RGB ("bt601" | "bt709"; limited range 16..235 / 16..240 unless full_range) -- ignored by the RGB formats.
    The table keeps its address for the life of the batch, so the forward's captured graph replays on whatever `set` put there last."""

    def __init__(self, n: int, device, format: str = "nv12", matrix: str = "bt709", full_range: bool = False):
        if not isinstance(n, int) or n < 1:
            raise ValueError("n must be a positive int, got {!r}".format(n))
        self.format_code, self.color_code = codes(format, matrix, full_range)
        self.n, self.format, self.matrix, self.full_range = n, format, matrix, bool(full_range)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.table = None           # [n * 48] uint8 on the device: allocated by the first set()
        self.frames = None          # the surfaces the table names: kept alive until the next set()
        self.planes: List[Tensor] = []              # every tensor of them
        self.sizes: List[Tuple[int, int]] = []      # (height, width) per frame
        self._host = None           # the records of the last set() in pinned memory (a ForwardPipeline uploads them into its slot's table)

    def set(self, frames: Sequence):
        """Name the batch's n surfaces. Per frame: a contiguous [h * 3 / 2, w] uint8 tensor (NV12 / I420, even h and w); or a tuple of plane
        tensors -- NV12: (Y [h, w], UV [ceil(h/2), 2 ceil(w/2)] or [ceil(h/2), ceil(w/2), 2]), I420: (Y, U, V), row-strided views allowed, the
        pitch is .stride(0); or for rgb24 / bgr24 an [h, w, 3] tensor, possibly row-strided. ValueError for anything malformed, naming the frame
        and the plane, before anything is changed. The records go up from pinned memory on the current stream; the host does not wait. The
        surfaces must be complete on that stream before the forward runs, and the batch keeps them alive until the next set()."""
        rec = frame_records(frames, self.format, self.device, self.n)
        if self.device.type != "cuda":
            raise RuntimeError("demonet_amd runs on an MI355X only (frames must be on a cuda device); there is no CPU fallback path")
        host = torch.frombuffer(rec, dtype=torch.uint8).pin_memory()       # (a copy: the allocator keeps the pinned block until the upload has run)
        if self.table is None:
            self.table = torch.empty(self.n * C.sizeof(_lib.Frame), dtype=torch.uint8, device=self.device)
        self.table.copy_(host, non_blocking=True)
        self._host = host
        self.frames = list(frames)
        self.planes = [t for fr in self.frames for t in ((fr,) if isinstance(fr, Tensor) else fr)]
        self.sizes = [(int(r.height), int(r.width)) for r in rec]
        return self


def forward_frames(model, batch: FrameBatch, packed=None):
    """SSD.forward_frames (see there)."""
    if not isinstance(batch, FrameBatch):
        raise ValueError("forward_frames: expected a FrameBatch, got {}".format(type(batch).__name__))
    dev = batch.device
    mdev = next(model.parameters()).device
    if mdev != dev:
        raise ValueError("forward_frames: the FrameBatch is on {}, the model on {}".format(dev, mdev))
    if batch.table is None:
        raise ValueError("forward_frames: the FrameBatch names no frames yet: call set() first")
    handle = model._plan(dev)
    n = batch.n
    model._check_packed(packed, n, dev)
    b = model._buffers_for(n, 0, 0, dev)        # (h = w = 0: the float staging image of this key is empty -- at 1080p it would be the call's largest allocation)
    stream = torch.cuda.current_stream(dev).cuda_stream
    model._set_packed(packed)
    model._feat_gen += 1
    from .ssd import forward_args
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dn_forward_frames(*forward_args(handle, batch.table.data_ptr(), n, batch.format_code, batch.color_code, b["outs"], b["ws"], stream)),
                   "dn_forward_frames")
    return b["outs"]


def track_frames(model, batch: FrameBatch, tracker, analytics=None, motion=None, osd=None, compose=None, wall=None, warp=None, source=None, jpeg=None):
    """SSD.track_frames (see there)."""
    from .track import ByteTracker, with_analytics
    from .osd import check_overlay, painted
    from .compose import check_composition, composed
    from .warp import check_warping, warped
    from .jpeg import check_jpeg, encoded
    if model.training:
        raise ValueError("track_frames: the model must be in eval mode")
    if not isinstance(tracker, ByteTracker):
        raise ValueError("track_frames: tracker must be a ByteTracker, got {}".format(type(tracker)))
    if analytics is not None:
        from .zones import check_analytics
        check_analytics(analytics, tracker, "track_frames")
    if motion is not None:
        from .motion import check_motion, compensated
        check_motion(motion, tracker, batch, "track_frames")
    check_overlay(osd, tracker, "track_frames")
    check_composition(compose, wall, batch, "track_frames")
    check_warping(warp, source, batch, "track_frames")
    check_jpeg(jpeg, wall, batch, "track_frames")
    warped(warp, source, batch)
    boxes, scores, labels, counts = forward_frames(model, batch)
    if motion is not None:
        compensated(motion, tracker, batch, boxes, scores, counts)
    return encoded(composed(painted(with_analytics(tracker.update(boxes, scores, labels, counts), analytics), osd, batch, analytics), compose, batch, wall),
                   jpeg, wall, batch)


def track_frames_appearance(model, batch: FrameBatch, tracker, cropper, embedder, analytics=None, motion=None, osd=None, compose=None, wall=None, warp=None,
                            source=None, jpeg=None):
    """SSD.track_frames_appearance (see there)."""
    from .crops import ObjectCropper
    from .warp import check_warping, warped
    from .osd import check_overlay, painted
    from .compose import check_composition, composed
    from .track import AppearanceTracker, with_analytics
    from .jpeg import check_jpeg, encoded
    if model.training:
        raise ValueError("track_frames_appearance: the model must be in eval mode")
    if not isinstance(tracker, AppearanceTracker):
        raise ValueError("track_frames_appearance: tracker must be an AppearanceTracker, got {}".format(type(tracker)))
    if not isinstance(cropper, ObjectCropper):
        raise ValueError("track_frames_appearance: cropper must be an ObjectCropper, got {}".format(type(cropper)))
    if not callable(embedder):
        raise ValueError("track_frames_appearance: embedder must be callable, got {}".format(type(embedder)))
    if analytics is not None:
        from .zones import check_analytics
        check_analytics(analytics, tracker, "track_frames_appearance")
    if motion is not None:
        from .motion import check_motion, compensated
        check_motion(motion, tracker, batch, "track_frames_appearance")
    check_overlay(osd, tracker, "track_frames_appearance")
    check_composition(compose, wall, batch, "track_frames_appearance")
    check_warping(warp, source, batch, "track_frames_appearance")
    check_jpeg(jpeg, wall, batch, "track_frames_appearance")
    warped(warp, source, batch)
    boxes, scores, labels, counts = forward_frames(model, batch)
    if motion is not None:
        compensated(motion, tracker, batch, boxes, scores, counts)
    select = scores >= tracker.params.track_thresh          # the HIGH rows: the ones whose appearance the step uses (a device op, no wait)
    patches, index, _ = cropper(batch, boxes, counts, select)
    emb = embedder(patches)
    if not isinstance(emb, Tensor) or tuple(emb.shape) != (cropper.capacity, tracker.dim):
        raise ValueError("track_frames_appearance: the embedder must return [{}, {}], got {}".format(
            cropper.capacity, tracker.dim, tuple(emb.shape) if isinstance(emb, Tensor) else type(emb)))
    return encoded(composed(painted(with_analytics(tracker.update(boxes, scores, labels, counts, emb.contiguous(), index), analytics), osd, batch, analytics),
                            compose, batch, wall), jpeg, wall, batch)


# ---------------------------------------------------------------------------------------------------------------- regions
def region_records(regions: Sequence, sizes: Sequence[Tuple[int, int]], n: int):
    """The validated dn_region records of `regions` -- (frame, x0, y0, w, h[, hflip]) tuples -- against sizes[frame] = (height, width), as
    (a ctypes array of n _lib.Region, the normalised tuples); ValueError naming the region otherwise. Host work only."""
    if isinstance(regions, Tensor) or not isinstance(regions, (list, tuple)):
        raise ValueError("expected a list of {} regions, got {}".format(n, type(regions).__name__))
    if len(regions) != n:
        raise ValueError("expected {} regions, got {}".format(n, len(regions)))
    sizes = [(int(h), int(w)) for h, w in sizes]
    rec = (_lib.Region * n)()
    norm = []
    for i, rg in enumerate(regions):
        if not isinstance(rg, (list, tuple)) or len(rg) not in (5, 6):
            raise ValueError("region {}: expected (frame, x0, y0, w, h[, hflip]), got {!r}".format(i, rg))
        vals = rg[:5]
        if not all(isinstance(v, int) and not isinstance(v, bool) for v in vals):
            raise ValueError("region {}: frame, x0, y0, w, h must be ints, got {!r}".format(i, tuple(rg)))
        f, x0, y0, w, h = vals
        flip = bool(rg[5]) if len(rg) == 6 else False
        if any(abs(v) > _INT32_MAX for v in vals) or x0 + w > _INT32_MAX or y0 + h > _INT32_MAX:
            raise ValueError("region {}: {!r} does not fit the record's int32".format(i, tuple(rg)))
        if f < 0 or f >= len(sizes):
            raise ValueError("region {}: frame index {} out of range ({} frames)".format(i, f, len(sizes)))
        H, W = sizes[f]
        if w < 1 or h < 1:
            raise ValueError("region {}: bad size {} x {} (width, height >= 1)".format(i, w, h))
        if x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
            raise ValueError("region {}: the rectangle x {} .. {}, y {} .. {} leaves frame {} of {} x {} (width x height)".format(
                i, x0, x0 + w, y0, y0 + h, f, W, H))
        r = rec[i]
        r.frame, r.x0, r.y0, r.width, r.height, r.flags = f, x0, y0, w, h, _lib.DN_REGION_HFLIP if flip else 0
        norm.append((f, x0, y0, w, h, flip))
    return rec, norm


class RegionTable:
    """n regions of the frames of a FrameBatch as one forward's input (SSD.forward_regions); owns the table of n dn_region records in device
    memory. The table keeps its address for the life of the object, so the forward's captured graph replays on whatever `set` put there last."""

    def __init__(self, n: int, device):
        if not isinstance(n, int) or n < 1:
            raise ValueError("n must be a positive int, got {!r}".format(n))
        self.n = n
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.table = None           # [n * 32] uint8 on the device: allocated by the first set()
        self.regions: List[Tuple] = []      # (frame, x0, y0, w, h, hflip) per network image
        self.frame_sizes = {}       # frame index -> the (height, width) its regions were validated against
        self._host = None

    def set(self, regions: Sequence, sizes: Sequence[Tuple[int, int]]):
        """Name the table's n regions: (frame, x0, y0, w, h[, hflip]) tuples of ints, validated against sizes[frame] = (height, width) -- pass
        FrameBatch.sizes. Frame index in range, w, h >= 1, x0, y0 >= 0, x0 + w <= W, y0 + h <= H, everything within int32; ValueError naming the
        region before anything is changed. The records go up from pinned memory on the current stream; the host does not wait."""
        rec, norm = region_records(regions, sizes, self.n)
        if self.device.type != "cuda":
            raise RuntimeError("demonet_amd runs on an MI355X only (regions must be on a cuda device); there is no CPU fallback path")
        host = torch.frombuffer(rec, dtype=torch.uint8).pin_memory()
        if self.table is None:
            self.table = torch.empty(self.n * C.sizeof(_lib.Region), dtype=torch.uint8, device=self.device)
        self.table.copy_(host, non_blocking=True)
        self._host = host
        self.regions = norm
        self.frame_sizes = {f: (int(sizes[f][0]), int(sizes[f][1])) for f in sorted({r[0] for r in norm})}
        return self


def check_regions(what: str, model, batch, table):
    """What every forward over regions checks before a record reaches the device: the objects, one device, both set, and that every frame the
    regions name has, in the batch AS IT IS NOW, the size the regions were validated against."""
    if not isinstance(batch, FrameBatch):
        raise ValueError("{}: expected a FrameBatch, got {}".format(what, type(batch).__name__))
    if not isinstance(table, RegionTable):
        raise ValueError("{}: expected a RegionTable, got {}".format(what, type(table).__name__))
    dev = batch.device
    mdev = next(model.parameters()).device
    if mdev != dev:
        raise ValueError("{}: the FrameBatch is on {}, the model on {}".format(what, dev, mdev))
    if table.device != dev:
        raise ValueError("{}: the RegionTable is on {}, the FrameBatch on {}".format(what, table.device, dev))
    if batch.table is None:
        raise ValueError("{}: the FrameBatch names no frames yet: call set() first".format(what))
    if table.table is None:
        raise ValueError("{}: the RegionTable names no regions yet: call set() first".format(what))
    for f, size in table.frame_sizes.items():
        have = batch.sizes[f] if f < len(batch.sizes) else None
        if have != size:
            raise ValueError("{}: stale sizes: the regions of frame {} were validated against {} (height, width), the batch now holds {}; "
                             "set() the table again".format(what, f, size, have if have is not None else "{} frames".format(len(batch.sizes))))


def run_regions(model, batch: FrameBatch, regions_ptr: int, n: int, packed=None):
    """dn_forward_regions on n records at regions_ptr (checked by the caller) -> the model's (n, 0, 0) output tensors"""
    dev = batch.device
    handle = model._plan(dev)
    model._check_packed(packed, n, dev)
    b = model._buffers_for(n, 0, 0, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    model._set_packed(packed)
    model._feat_gen += 1
    p = C.c_void_p
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dn_forward_regions(p(handle), p(batch.table.data_ptr()), p(regions_ptr), n, batch.format_code, batch.color_code,
                                                 *(p(t.data_ptr()) for t in b["outs"]), p(b["ws"].data_ptr()), b["ws"].numel(), p(stream)),
                   "dn_forward_regions")
    return b["outs"]


def forward_regions(model, batch: FrameBatch, table: RegionTable, packed=None):
    """SSD.forward_regions (see there)."""
    check_regions("forward_regions", model, batch, table)
    return run_regions(model, batch, table.table.data_ptr(), table.n, packed)
