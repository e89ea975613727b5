"""Surface composition on the device: scale, convert and tile video surfaces -- the step behind the on-screen display.

A `Compositor` copies rectangles of the surfaces of one `FrameBatch` into rectangles of the surfaces of another, through an exact integer area
filter and, where the two batches differ in format or colour space, the integer colour arithmetic the header fixes (include/demonet_hip.h,
dn_compose): 64 painted streams into one wall surface for a single encoder session, a preview per camera, NV12 to RGB for a snapshot, pitched BGR
to NV12 for an encoder. One launch, no float copy of a frame, nothing visits the host, and a captured graph follows new surfaces and new items.

    wall = FrameBatch(1, "cuda:0", format="nv12").set([wall_surface])
    comp = Compositor(64, "cuda:0").set(grid(batch.sizes, wall.sizes[0], 8, 8), batch, wall)
    comp(batch, wall, clear=(0, 0, 0))                                         # black, then the 64 cells
    outs = model.track_frames(batch, tracker, osd=overlay, compose=comp, wall=wall)     # ... or as the step's last act, behind the paint

The library trusts the item table as it trusts a region table, so `set` validates every item on the host first and remembers both batches' sizes;
a call refuses batches whose sizes, formats or colour codes have changed since. There is no CPU fallback.
"""
import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from .frames import FrameBatch
from .osd import to_surface

MAX_ITEMS = 65536
MAX_SIDE = 32768             # of a rectangle: (j * sw) stays inside 32 bits
MAX_AREA = 1 << 24           # sw * sh of an item: 255 * sw * sh stays inside an unsigned 32-bit sum
TILE = 32
BUCKET = 256             # pixels: the side of the buckets the overlap check sorts destination rectangles into
_YUV = ("nv12", "i420")


@dataclass(frozen=True)
class Item:
    """One copy: the rectangle src_rect = (x0, y0, w, h) of frame `src` of the source batch (None: the whole frame) to the rectangle
    dst_rect = (x0, y0, w, h) of frame `dst` of the destination batch."""
    src: int
    dst: int
    dst_rect: Tuple[int, int, int, int]
    src_rect: Optional[Tuple[int, int, int, int]] = None


def _ints(v, n):
    return isinstance(v, (tuple, list)) and len(v) == n and all(isinstance(x, int) and not isinstance(x, bool) for x in v)


def _overlap(a, b):
    return a[0] < b[0] + b[2] and b[0] < a[0] + a[2] and a[1] < b[1] + b[3] and b[1] < a[1] + a[3]


def _chroma(r):
    return r[0] // 2, r[1] // 2, (r[2] + 1) // 2, (r[3] + 1) // 2


def item_records(items: Sequence, src_sizes, dst_sizes, src_yuv: bool, dst_yuv: bool, capacity: int):
    """The validated table of `items` -- Item objects or (src, dst, dst_rect[, src_rect]) tuples -- against src_sizes[src] and dst_sizes[dst] =
    (height, width): (the bytes of the dn_compose_header and `capacity` dn_compose_item records, the normalised (src, src_rect, dst, dst_rect)
    list, the tile count). ValueError naming the item otherwise. Host work only."""
    if isinstance(items, torch.Tensor) or not isinstance(items, (list, tuple)):
        raise ValueError("Compositor: expected a list of items, got {}".format(type(items).__name__))
    if len(items) > capacity:
        raise ValueError("Compositor: {} items, the capacity is {}".format(len(items), capacity))
    src_sizes = [(int(h), int(w)) for h, w in src_sizes]
    dst_sizes = [(int(h), int(w)) for h, w in dst_sizes]
    head = _lib.ComposeHeader()
    rec = (_lib.ComposeItem * capacity)()
    norm, tiles = [], 0
    buckets = {}
    for i, it in enumerate(items):
        if isinstance(it, (tuple, list)) and len(it) in (3, 4):
            it = Item(*it)
        if not isinstance(it, Item):
            raise ValueError("item {}: expected an Item or (src, dst, dst_rect[, src_rect]), got {!r}".format(i, it))
        if not _ints((it.src, it.dst), 2):
            raise ValueError("item {}: src and dst must be ints, got {!r}, {!r}".format(i, it.src, it.dst))
        if it.src < 0 or it.src >= len(src_sizes):
            raise ValueError("item {}: source index {} out of range ({} frames)".format(i, it.src, len(src_sizes)))
        if it.dst < 0 or it.dst >= len(dst_sizes):
            raise ValueError("item {}: destination index {} out of range ({} frames)".format(i, it.dst, len(dst_sizes)))
        SH, SW = src_sizes[it.src]
        DH, DW = dst_sizes[it.dst]
        srect = (0, 0, SW, SH) if it.src_rect is None else it.src_rect
        for what, r, (H, W), yuv in (("source", srect, (SH, SW), src_yuv), ("destination", it.dst_rect, (DH, DW), dst_yuv)):
            if not _ints(r, 4):
                raise ValueError("item {}: the {} rectangle must be four ints (x0, y0, w, h), got {!r}".format(i, what, r))
            x0, y0, w, h = r
            if w < 1 or h < 1 or w > MAX_SIDE or h > MAX_SIDE:
                raise ValueError("item {}: the {} rectangle is {} x {}, a side takes 1 .. {}".format(i, what, w, h, MAX_SIDE))
            if x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
                raise ValueError("item {}: the {} rectangle x {} .. {}, y {} .. {} lies outside its frame of {} x {} (width x height)".format(
                    i, what, x0, x0 + w, y0, y0 + h, W, H))
            if yuv and (x0 % 2 or y0 % 2):
                raise ValueError("item {}: odd origin ({}, {}) of the {} rectangle: a 4:2:0 surface takes even x0 and y0".format(i, x0, y0, what))
        srect, drect = tuple(srect), tuple(it.dst_rect)
        if srect[2] * srect[3] > MAX_AREA:
            raise ValueError("item {}: the source rectangle has {} x {} = {} pixels, sw * sh takes at most 2^24".format(
                i, srect[2], srect[3], srect[2] * srect[3]))
        # the earlier items of this destination that can touch this one: those that share a bucket of BUCKET x BUCKET pixels (the chroma footprint of
        # a rectangle lies inside the buckets of its luma rectangle grown by one pixel)
        cells = [(it.dst, bx, by) for bx in range(drect[0] // BUCKET, (drect[0] + drect[2]) // BUCKET + 1)
                 for by in range(drect[1] // BUCKET, (drect[1] + drect[3]) // BUCKET + 1)]
        for k, other in sorted({e for cell in cells for e in buckets.get(cell, ())}):
            if _overlap(drect, other) or (dst_yuv and _overlap(_chroma(drect), _chroma(other))):
                raise ValueError("item {}: its destination rectangle {} overlaps item {}'s {} in destination {}{}".format(
                    i, drect, k, other, it.dst, "" if _overlap(drect, other) else " (their chroma samples do)"))
        for cell in cells:
            buckets.setdefault(cell, []).append((i, drect))
        r = rec[i]
        r.src, r.sx0, r.sy0, r.sw, r.sh = (it.src,) + srect
        r.dst, r.dx0, r.dy0, r.dw, r.dh = (it.dst,) + drect
        r.tile0 = tiles
        tiles += ((drect[2] + TILE - 1) // TILE) * ((drect[3] + TILE - 1) // TILE)
        if tiles >= 2 ** 31:
            raise ValueError("item {}: the items have 2^31 or more tiles of {} x {} pixels".format(i, TILE, TILE))
        norm.append((it.src, srect, it.dst, drect))
    head.n_items, head.n_tiles = len(norm), tiles
    return bytes(head) + bytes(rec), norm, tiles


def grid(src_sizes, dst_size, rows: int, cols: int, fit: str = "contain", margin: int = 0, yuv: bool = True, dst: int = 0) -> List[Item]:
    """The items of a wall: source i of src_sizes = [(height, width), ...] goes, whole, into cell (i // cols, i % cols) of a rows x cols grid over a
    destination surface of dst_size = (height, width), index `dst`. fit="contain": the largest rectangle of the source's aspect inside the cell less
    `margin` pixels on every side, centred; "stretch": that whole area. With yuv every origin is even, and no chroma sample is shared between
    cells. Host geometry only; ValueError for more sources than cells or a cell that is left without a pixel."""
    if fit not in ("contain", "stretch"):
        raise ValueError("grid: fit must be 'contain' or 'stretch', got {!r}".format(fit))
    if not _ints((rows, cols, margin), 3) or rows < 1 or cols < 1 or margin < 0:
        raise ValueError("grid: rows, cols >= 1 and margin >= 0 must be ints, got {!r}, {!r}, {!r}".format(rows, cols, margin))
    src_sizes = [(int(h), int(w)) for h, w in src_sizes]
    if len(src_sizes) > rows * cols:
        raise ValueError("grid: {} sources, {} x {} cells".format(len(src_sizes), rows, cols))
    H, W = int(dst_size[0]), int(dst_size[1])
    up = (lambda v: v + (v & 1)) if yuv else (lambda v: v)
    items = []
    for i, (h, w) in enumerate(src_sizes):
        r, c = divmod(i, cols)
        x0, x1 = up(c * W // cols + margin), (c + 1) * W // cols - margin
        y0, y1 = up(r * H // rows + margin), (r + 1) * H // rows - margin
        cw, ch = x1 - x0, y1 - y0
        if cw < 1 or ch < 1 or h < 1 or w < 1:
            raise ValueError("grid: cell {} of a {} x {} surface is left without a pixel".format(i, W, H))
        if fit == "stretch":
            dw, dh, dx, dy = cw, ch, x0, y0
        else:
            if cw * h <= ch * w:
                dw, dh = cw, max(1, h * cw // w)
            else:
                dw, dh = max(1, w * ch // h), ch
            dx, dy = x0 + (cw - dw) // 2, y0 + (ch - dh) // 2
            if yuv:
                dx, dy = dx & ~1, dy & ~1           # (x0, y0 are even: still inside the cell)
        items.append(Item(i, dst, (dx, dy, dw, dh)))
    return items


def check_compose(what: str, comp, src_batch, dst_batch):
    """What every composition checks before the library is touched: the objects, one device, everything set, and that both batches have, AS THEY
    ARE NOW, the sizes, formats and colour codes the items were validated against."""
    if not isinstance(comp, Compositor):
        raise ValueError("{}: expected a Compositor, got {}".format(what, type(comp).__name__))
    for name, b in (("source", src_batch), ("destination", dst_batch)):
        if not isinstance(b, FrameBatch):
            raise ValueError("{}: the {} must be a FrameBatch, got {}".format(what, name, type(b).__name__))
        if b.device != comp.device:
            raise ValueError("{}: the {} FrameBatch is on {}, the compositor on {}".format(what, name, b.device, comp.device))
        if b.table is None:
            raise ValueError("{}: the {} FrameBatch names no frames yet: call set() first".format(what, name))
    if src_batch is dst_batch:
        raise ValueError("{}: source and destination must be two batches (and must not share memory)".format(what))
    if comp.table is None:
        raise ValueError("{}: the compositor holds no items yet: call set() first".format(what))
    for name, b, sizes, space in (("source", src_batch, comp.src_sizes, comp.src_space), ("destination", dst_batch, comp.dst_sizes, comp.dst_space)):
        if list(b.sizes) != sizes:
            raise ValueError("{}: stale sizes: the items were validated against {} frames of {} (height, width), the batch now holds {}; "
                             "set() the compositor again".format(what, name, sizes, list(b.sizes)))
        if (b.format_code, b.color_code) != space:
            raise ValueError("{}: the items were validated for a {} batch of format / colour code {}, this one has {}; set() the compositor "
                             "again".format(what, name, space, (b.format_code, b.color_code)))


def _rgb(v):
    if not isinstance(v, (tuple, list)) or len(v) != 3 or not all(isinstance(x, int) and not isinstance(x, bool) and 0 <= x <= 255 for x in v):
        raise ValueError("Compositor: clear must be three ints (R, G, B) in 0 .. 255 or None, got {!r}".format(v))
    return tuple(v)


class Compositor:
    """A table of at most `capacity` items on `device`; owns the dn_compose_header + dn_compose_item table in device memory. The table keeps its
    address for the life of the object, so a captured call replays on whatever set() put there last -- other items, another item count."""

    def __init__(self, capacity: int, device):
        if not isinstance(capacity, int) or isinstance(capacity, bool) or capacity < 1 or capacity > MAX_ITEMS:
            raise ValueError("Compositor: capacity takes an int in 1 .. {}, got {!r}".format(MAX_ITEMS, capacity))
        self.capacity = capacity
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.table = None            # [16 + capacity * 48] uint8 on the device: allocated by the first set()
        self.items: List[Tuple] = []        # (src, src_rect, dst, dst_rect) per item
        self.tiles = 0
        self.src_sizes = self.dst_sizes = None      # the (height, width) lists the items were validated against
        self.src_space = self.dst_space = None      # (format code, colour code) of the two batches
        self._host = None

    def set(self, items: Sequence, src_batch: FrameBatch, dst_batch: FrameBatch):
        """Name the items: Item objects or (src, dst, dst_rect[, src_rect]) tuples, rectangles (x0, y0, w, h) in frame pixels, a source rectangle
        left out meaning the whole frame. Validated against both batches as they are now: indices in range; rectangles inside their frames, sides
        1 .. 32768; sw * sh <= 2^24; even origins on a 4:2:0 side; the destination rectangles of one surface disjoint, on a 4:2:0 destination
        their chroma samples too. ValueError naming the item, before anything is changed. The table goes up from pinned memory on the current
        stream; the host does not wait."""
        for name, b in (("source", src_batch), ("destination", dst_batch)):
            if not isinstance(b, FrameBatch):
                raise ValueError("Compositor: the {} must be a FrameBatch, got {}".format(name, type(b).__name__))
            if b.device != self.device:
                raise ValueError("Compositor: the {} FrameBatch is on {}, the compositor on {}".format(name, b.device, self.device))
            if not b.sizes:
                raise ValueError("Compositor: the {} FrameBatch names no frames yet: call set() first".format(name))
        raw, norm, tiles = item_records(items, src_batch.sizes, dst_batch.sizes, src_batch.format in _YUV, dst_batch.format in _YUV, self.capacity)
        if self.device.type != "cuda":
            raise RuntimeError("demonet_amd runs on an MI355X only (the compositor must be on a cuda device); there is no CPU fallback path")
        host = torch.frombuffer(bytearray(raw), dtype=torch.uint8).pin_memory()
        if self.table is None:
            self.table = torch.empty(len(raw), dtype=torch.uint8, device=self.device)
        self.table.copy_(host, non_blocking=True)
        self._host = host
        self.items, self.tiles = norm, tiles
        self.src_sizes, self.dst_sizes = list(src_batch.sizes), list(dst_batch.sizes)
        self.src_space, self.dst_space = (src_batch.format_code, src_batch.color_code), (dst_batch.format_code, dst_batch.color_code)
        return self

    def __call__(self, src_batch: FrameBatch, dst_batch: FrameBatch, clear=None, stream=None):
        """Run the items: the source batch's surfaces into the destination batch's, which are written in place. clear: an (R, G, B) colour every
        destination surface's payload is filled with first (converted to the destination's colour space as the overlay converts its palette), or
        None: bytes no item covers keep their value. Enqueued on `stream` (default: the current stream); no host wait. Returns dst_batch.
        ValueError for unset or foreign batches and for sizes, formats or colour codes that changed since set()."""
        check_compose("Compositor", self, src_batch, dst_batch)
        fill = None if clear is None else to_surface(_rgb(clear), dst_batch.format, dst_batch.matrix, dst_batch.full_range)
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        if not hasattr(s, "cuda_stream"):
            s = torch.cuda.ExternalStream(int(s), device=self.device)
        p = C.c_void_p
        with torch.cuda.device(self.device):
            if fill is not None:
                _lib.check(_lib.lib().dn_surface_fill(p(dst_batch.table.data_ptr()), dst_batch.n, dst_batch.format_code, fill[0], fill[1], fill[2],
                                                      p(s.cuda_stream)), "dn_surface_fill")
            _lib.check(_lib.lib().dn_compose(p(src_batch.table.data_ptr()), src_batch.format_code, src_batch.color_code, p(dst_batch.table.data_ptr()),
                                             dst_batch.format_code, dst_batch.color_code, p(self.table.data_ptr()), self.capacity, p(s.cuda_stream)),
                       "dn_compose")
        return dst_batch


def check_composition(compose, wall, batch, who: str):
    """The `compose=` / `wall=` arguments of SSD.track_frames / track_frames_appearance / track_sliced_frames: both None, or a Compositor that was
    set() for (batch, wall) and the destination FrameBatch. Checked before the step starts."""
    if compose is None and wall is None:
        return
    if compose is None or wall is None:
        raise ValueError("{}: compose= (a Compositor) and wall= (its destination FrameBatch) go together".format(who))
    check_compose(who, compose, batch, wall)


def composed(outs, compose, batch, wall):
    """A tracking step's outputs, unchanged; with a Compositor the batch's frames -- painted, when the step has an overlay -- are composed into
    the wall's surfaces first."""
    if compose is not None:
        compose(batch, wall)
    return outs

