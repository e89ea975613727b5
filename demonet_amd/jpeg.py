"""Baseline JPEG encoding on the device: rectangles of the surfaces of a `FrameBatch` become complete .jpg files in one device byte
arena -- the snapshot that goes with a CROSS / ENTER event, the thumbnail of a tracked object, a redacted evidence frame, a low-rate preview of the
wall -- without a copy of the pixels to the host and without a host wait.

A `JpegEncoder` codes every item as a baseline sequential JFIF 1.01 file, 4:2:0, with the Annex K tables at a quality per item and one restart
interval per MCU row (include/demonet_hip.h, dn_jpeg_encode, fixes the stream; tests/jpeg_ref.py restates it). Three launches, nothing visits the
host, and a captured graph follows new surfaces, new items and new counts.

    enc = JpegEncoder(64, "cuda:0", arena_bytes=64 << 20, quality=85).set([Item(i) for i in range(batch.n)], batch)      # whole frames
    arena, results, totals = enc.encode(batch)                      # device tensors at fixed addresses; results rows (offset, length, status, 0)
    files = enc.files()                                             # one synchronising copy: a list of bytes, None for a slot that was not written
    enc.encode_objects(batch, cropper)                              # ... or one file per patch slot of an ObjectCropper's last step
    outs = model.track_frames(batch, tracker, osd=overlay, compose=comp, wall=wall, jpeg=enc)     # ... or as the step's last act, on the wall

A thumbnail at another size is a `Compositor` item into a small batch first: the encoder does not scale. The library trusts the item table as it
trusts a compose table, so `set` validates every item on the host first and remembers the batch's sizes; a call refuses a batch whose sizes, format
or colour code have changed since. `encode_objects` lets the device write the table from index rows it does not trust. There is no CPU fallback.
"""
import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from .frames import FrameBatch

MAX_ITEMS = _lib.DN_JPEG_MAX_ITEMS
MAX_SIDE = 32768
HEADER_BYTES = _lib.DN_JPEG_HEADER_BYTES
STATUS = ("written", "empty", "refused", "no space")
_YUV = ("nv12", "i420")
_INT32_MAX = 2 ** 31 - 1


@dataclass(frozen=True)
class Item:
    """One file: the rectangle rect = (x0, y0, w, h) of frame `frame` of the batch (None: the whole frame) at `quality` 1 .. 100 (None: the
    encoder's default)."""
    frame: int
    rect: Optional[Tuple[int, int, int, int]] = None
    quality: Optional[int] = None


def _int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _quality(q, what):
    if not _int(q) or q < 1 or q > 100:
        raise ValueError("{}: quality takes an int in 1 .. 100, got {!r}".format(what, q))
    return q


def item_records(items: Sequence, sizes, yuv: bool, capacity: int, quality: int, max_segments: int):
    """The validated table of `items` -- Item objects, (frame[, rect[, quality]]) tuples or plain frame indices -- against sizes[frame] = (height,
    width): (the bytes of the dn_jpeg_header and `capacity` dn_jpeg_item records, the normalised (frame, rect, quality) list, the MCU-row count).
    ValueError naming the item otherwise. Host work only."""
    if isinstance(items, torch.Tensor) or not isinstance(items, (list, tuple)):
        raise ValueError("JpegEncoder: expected a list of items, got {}".format(type(items).__name__))
    if len(items) > capacity:
        raise ValueError("JpegEncoder: {} items, the capacity is {}".format(len(items), capacity))
    sizes = [(int(h), int(w)) for h, w in sizes]
    head = _lib.JpegHeader()
    rec = (_lib.JpegItem * capacity)()
    norm, seg = [], 0
    for i, it in enumerate(items):
        if _int(it):
            it = Item(it)
        elif isinstance(it, (tuple, list)) and 1 <= len(it) <= 3:
            it = Item(*it)
        if not isinstance(it, Item):
            raise ValueError("item {}: expected an Item, a frame index or (frame[, rect[, quality]]), got {!r}".format(i, it))
        if not _int(it.frame):
            raise ValueError("item {}: frame must be an int, got {!r}".format(i, it.frame))
        if it.frame < 0 or it.frame >= len(sizes):
            raise ValueError("item {}: frame index {} out of range ({} frames)".format(i, it.frame, len(sizes)))
        H, W = sizes[it.frame]
        rect = (0, 0, W, H) if it.rect is None else it.rect
        if not (isinstance(rect, (tuple, list)) and len(rect) == 4 and all(_int(v) for v in rect)):
            raise ValueError("item {}: the rectangle must be four ints (x0, y0, w, h), got {!r}".format(i, rect))
        x0, y0, w, h = rect
        if w < 1 or h < 1 or w > MAX_SIDE or h > MAX_SIDE:
            raise ValueError("item {}: the rectangle is {} x {}, a side takes 1 .. {}".format(i, w, h, MAX_SIDE))
        if x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
            raise ValueError("item {}: the rectangle x {} .. {}, y {} .. {} lies outside its frame of {} x {} (width x height)".format(
                i, x0, x0 + w, y0, y0 + h, W, H))
        if yuv and (x0 % 2 or y0 % 2):
            raise ValueError("item {}: odd origin ({}, {}): a 4:2:0 surface takes even x0 and y0".format(i, x0, y0))
        q = _quality(quality if it.quality is None else it.quality, "item {}".format(i))
        r = rec[i]
        r.frame, r.x0, r.y0, r.width, r.height, r.quality, r.seg0 = it.frame, x0, y0, w, h, q, seg
        seg += (h + 15) // 16
        if seg > max_segments:
            raise ValueError("item {}: the items have {} or more MCU rows, max_segments is {}".format(i, seg, max_segments))
        norm.append((it.frame, (x0, y0, w, h), q))
    for i in range(len(norm), capacity):
        rec[i].frame, rec[i].seg0 = -1, seg
    head.n_items, head.n_segments = len(norm), seg
    return bytes(head) + bytes(rec), norm, seg


class JpegEncoder:
    """At most `items` files per call on `device` into an arena of `arena_bytes` bytes; owns the item table, the arena, the result and total
    tensors and the workspace. Their addresses are fixed for the life of the object, so a captured call replays on whatever set() put into the
    table last -- other items, another item count. quality: the default of an item that names none. max_segments: the MCU rows (of 16 pixel rows)
    of all items of a call together; the default holds `items` full-HD frames."""

    def __init__(self, items: int, device, arena_bytes: int, quality: int = 85, max_segments: Optional[int] = None):
        if not _int(items) or items < 1 or items > MAX_ITEMS:
            raise ValueError("JpegEncoder: items takes an int in 1 .. {}, got {!r}".format(MAX_ITEMS, items))
        if not _int(arena_bytes) or arena_bytes < 1 or arena_bytes > _INT32_MAX:
            raise ValueError("JpegEncoder: arena_bytes takes an int in 1 .. 2^31 - 1, got {!r}".format(arena_bytes))
        if max_segments is None:
            max_segments = items * 68
        if not _int(max_segments) or max_segments < 1 or max_segments > _INT32_MAX:
            raise ValueError("JpegEncoder: max_segments takes an int in 1 .. 2^31 - 1, got {!r}".format(max_segments))
        self.capacity, self.arena_bytes, self.max_segments = items, arena_bytes, max_segments
        self.quality = _quality(quality, "JpegEncoder")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.table = None            # [16 + capacity * 32] uint8 on the device: allocated with the other tensors by the first use
        self.arena = self.results = self.totals = self.workspace = None
        self.items: List[Tuple] = []        # (frame, rect, quality) per item of the last set()
        self.segments = 0
        self.sizes = None            # the (height, width) list the items were validated against
        self.space = None            # (format code, colour code) of that batch
        self._host = self._keep = None

    def _allocate(self):
        if self.device.type != "cuda":
            raise RuntimeError("demonet_amd runs on an MI355X only (the encoder must be on a cuda device); there is no CPU fallback path")
        if self.table is None:
            dev = self.device
            self.table = torch.zeros(C.sizeof(_lib.JpegHeader) + self.capacity * C.sizeof(_lib.JpegItem), dtype=torch.uint8, device=dev)
            self.arena = torch.zeros(self.arena_bytes, dtype=torch.uint8, device=dev)
            self.results = torch.zeros((self.capacity, 4), dtype=torch.int32, device=dev)
            self.results[:, 2] = 1            # (no call yet: every slot is empty)
            self.totals = torch.zeros(4, dtype=torch.int32, device=dev)
            ws = int(_lib.lib().dn_jpeg_workspace_bytes(self.capacity, self.max_segments))
            if ws <= 0:
                raise RuntimeError("dn_jpeg_workspace_bytes({}, {}) refused the sizes".format(self.capacity, self.max_segments))
            self.workspace = torch.empty(ws, dtype=torch.uint8, device=dev)

    def _check_batch(self, what, batch):
        if not isinstance(batch, FrameBatch):
            raise ValueError("{}: expected a FrameBatch, got {}".format(what, type(batch).__name__))
        if batch.device != self.device:
            raise ValueError("{}: the FrameBatch is on {}, the encoder on {}".format(what, batch.device, self.device))
        if not batch.sizes or batch.table is None:
            raise ValueError("{}: the FrameBatch names no frames yet: call set() first".format(what))

    def set(self, items: Sequence, batch: FrameBatch):
        """Name the items: Item objects, (frame[, rect[, quality]]) tuples or frame indices, rectangles (x0, y0, w, h) in frame pixels, None
        meaning the whole frame. Validated against the batch as it is now: frame indices in range; rectangles inside their frames, sides
        1 .. 32768; even origins on NV12 / I420; quality 1 .. 100; at most `items` items and max_segments MCU rows. ValueError naming the item,
        before anything is changed. The table goes up from pinned memory on the current stream; the host does not wait."""
        self._check_batch("JpegEncoder", batch)
        raw, norm, seg = item_records(items, batch.sizes, batch.format in _YUV, self.capacity, self.quality, self.max_segments)
        self._allocate()
        host = torch.frombuffer(bytearray(raw), dtype=torch.uint8).pin_memory()
        self.table.copy_(host, non_blocking=True)
        self._host = host
        self.items, self.segments = norm, seg
        self.sizes, self.space = list(batch.sizes), (batch.format_code, batch.color_code)
        return self

    def _run(self, batch, stream):
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        if not hasattr(s, "cuda_stream"):
            s = torch.cuda.ExternalStream(int(s), device=self.device)
        p = C.c_void_p
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().dn_jpeg_encode(p(batch.table.data_ptr()), batch.format_code, batch.color_code, p(self.table.data_ptr()), self.capacity,
                                                 p(self.arena.data_ptr()), self.arena_bytes, p(self.results.data_ptr()), p(self.totals.data_ptr()),
                                                 p(self.workspace.data_ptr()), self.workspace.numel(), p(s.cuda_stream)), "dn_jpeg_encode")
        return self.arena, self.results, self.totals

    def encode(self, batch: FrameBatch, stream=None):
        """Code the items of the last set() from the batch's surfaces as they are when the kernels run. Enqueued on `stream` (default: the current
        stream); no host wait. Returns (arena [arena_bytes] uint8, results [items, 4] int32 rows (offset, length, status, 0), totals [4] int32
        (written, refused, bytes_used, 0)): the encoder's own tensors, overwritten by the next call. Status 0 written, 1 empty slot, 2 rectangle
        refused, 3 no space; the bytes between the files and beyond totals[2] keep their contents. ValueError for an unset or foreign batch and
        for sizes, a format or a colour code that changed since set()."""
        check_encoder("JpegEncoder.encode", self, batch)
        return self._run(batch, stream)

    def encode_objects(self, batch: FrameBatch, cropper_or_index, select=None, quality: Optional[int] = None, stream=None):
        """One file per patch slot of an ObjectCropper's last step (or of an index tensor [rows <= items, 8] int32 with its rows (stream, row, x0,
        y0, width, height, 0, 0), stream -1 an unused slot): the device writes the item table from the rows, which it does not trust -- a row
        that names no frame of the batch or a rectangle not inside it has status 2, an unused or deselected slot status 1, a slot beyond
        max_segments MCU rows status 3. On NV12 / I420 an odd origin moves down to the even pixel and the side grows by one. select: None or a
        bool / uint8 device tensor [rows], False deselects the slot. File s is patch slot s, so cropper.gather(ids) names the track of every
        file. Replaces the items of set(). Returns encode()'s tensors; no host wait."""
        self._check_batch("JpegEncoder.encode_objects", batch)
        index = cropper_or_index if isinstance(cropper_or_index, torch.Tensor) else getattr(cropper_or_index, "index", None)
        if not isinstance(index, torch.Tensor) or index.dtype != torch.int32 or index.dim() != 2 or index.shape[1] != 8 or not index.is_contiguous():
            raise ValueError("JpegEncoder.encode_objects: expected an ObjectCropper or a contiguous [rows, 8] int32 index tensor, got {}".format(
                type(cropper_or_index).__name__ if not isinstance(index, torch.Tensor) else (tuple(index.shape), index.dtype)))
        rows = int(index.shape[0])
        if rows < 1 or rows > self.capacity:
            raise ValueError("JpegEncoder.encode_objects: {} index rows, the encoder holds 1 .. {} items".format(rows, self.capacity))
        if index.device != self.device:
            raise ValueError("JpegEncoder.encode_objects: the index is on {}, the encoder on {}".format(index.device, self.device))
        if select is not None:
            if not isinstance(select, torch.Tensor) or select.dtype not in (torch.bool, torch.uint8) or tuple(select.shape) != (rows,) \
                    or select.device != self.device or not select.is_contiguous():
                raise ValueError("JpegEncoder.encode_objects: select must be a contiguous bool or uint8 tensor [{}] on {}".format(rows, self.device))
            if select.dtype == torch.bool:
                select = select.view(torch.uint8)
        q = _quality(self.quality if quality is None else quality, "JpegEncoder.encode_objects")
        self._allocate()
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        if not hasattr(s, "cuda_stream"):
            s = torch.cuda.ExternalStream(int(s), device=self.device)
        p = C.c_void_p
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().dn_jpeg_items_from_index(p(batch.table.data_ptr()), batch.n, batch.format_code, p(index.data_ptr()), rows,
                                                           p(select.data_ptr()) if select is not None else None, q, self.max_segments,
                                                           p(self.table.data_ptr()), p(s.cuda_stream)), "dn_jpeg_items_from_index")
        self._keep = (index, select)            # alive until the next call: the launch reads them
        self.items, self.segments = [], 0          # the table is the device's now
        self.sizes, self.space = list(batch.sizes), (batch.format_code, batch.color_code)
        return self._run(batch, s)

    def files(self) -> List[Optional[bytes]]:
        """The files of the last call as a list of bytes, one entry per slot, None for a slot that was not written. One synchronising copy of the
        results and of the used part of the arena."""
        if self.results is None:
            raise ValueError("JpegEncoder.files: nothing was encoded yet")
        res = self.results.cpu()
        used = int(self.totals.cpu()[2])
        data = self.arena[:used].cpu().numpy().tobytes()
        return [data[int(o):int(o) + int(n)] if int(st) == 0 else None for o, n, st, _ in res.tolist()]


def check_encoder(what: str, enc, batch):
    """What every encode checks before the library is touched: the objects, one device, everything set, and that the batch has, AS IT IS NOW, the
    sizes, format and colour code the items were validated against."""
    if not isinstance(enc, JpegEncoder):
        raise ValueError("{}: expected a JpegEncoder, got {}".format(what, type(enc).__name__))
    enc._check_batch(what, batch)
    if enc.table is None or enc.sizes is None:
        raise ValueError("{}: the encoder holds no items yet: call set() first".format(what))
    if list(batch.sizes) != enc.sizes:
        raise ValueError("{}: stale sizes: the items were validated against frames of {} (height, width), the batch now holds {}; set() the encoder "
                         "again".format(what, enc.sizes, list(batch.sizes)))
    if (batch.format_code, batch.color_code) != enc.space:
        raise ValueError("{}: the items were validated for a batch of format / colour code {}, this one has {}; set() the encoder again".format(
            what, enc.space, (batch.format_code, batch.color_code)))


def check_jpeg(jpeg, wall, batch, who: str):
    """The `jpeg=` argument of SSD.track_frames / track_frames_appearance / track_sliced_frames: None, or a JpegEncoder that was set() for the wall
    when the step has one, for the batch otherwise. Checked before the step starts."""
    if jpeg is not None:
        check_encoder(who, jpeg, batch if wall is None else wall)


def encoded(outs, jpeg, wall, batch):
    """A tracking step's outputs, unchanged; with a JpegEncoder its items are coded first -- behind the paint and the composition -- from the wall's
    surfaces when the step has a wall, from the batch's otherwise."""
    if jpeg is not None:
        jpeg.encode(batch if wall is None else wall)
    return outs
