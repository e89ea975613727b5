"""On-screen display on the device: boxes, labels, counting lines, zone edges and redaction painted into the frames.

An `Overlay` paints a tracking step's outputs (or raw detections) IN PLACE into the surfaces a `FrameBatch` names, in their own colour space:
outlines, translucent fills, class / id / score labels in a built-in 5 x 7 font, the lines and zones of a `ZoneAnalytics`, and redaction by
pixelation or opaque fill. Nothing visits the host: boxes, ids and the zone geometry are read where they lie, the label text is formatted on
the device, and the call is two launches (include/demonet_hip.h, dn_osd_paint, has the rules) that a captured graph replays.

    overlay = Overlay(streams, "cuda:0", names=["person", "car"], scale=2)
    overlay.redact([0])                                   # persons are pixelated instead of outlined
    outs = model.track_frames(batch, tracker, analytics=za, osd=overlay)      # ... and painted as the step's last act
    overlay.paint(batch, boxes, scores, labels, counts, ids=ids, zones=za)    # or by hand

Traffic is proportional to the 32 x 32 tiles the primitives touch, not to the frames. PAINT LAST: whatever reads the frames afterwards (a motion
estimate, crops, a second forward) sees the painted pixels. There is no CPU fallback.
"""
import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib, osd_font
from .frames import FrameBatch

MAX_STREAMS, MAX_D, MAX_COLORS, MAX_LABELS = 65535, 512, 256, 65536
BLOCKS = (0, 4, 8, 16, 32)
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
SHIFT = 14
# the default palette, RGB: 32 hues that stay apart on video
PALETTE = [(230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240), (240, 50, 230),
           (210, 245, 60), (250, 190, 212), (0, 128, 128), (220, 190, 255), (170, 110, 40), (255, 250, 200), (128, 0, 0), (170, 255, 195),
           (128, 128, 0), (255, 215, 180), (0, 0, 128), (128, 128, 128), (255, 99, 71), (0, 191, 255), (154, 205, 50), (255, 20, 147),
           (72, 61, 139), (255, 165, 0), (32, 178, 170), (186, 85, 211), (205, 92, 92), (46, 139, 87), (100, 149, 237), (218, 165, 32)]


def forward_coeffs(matrix: str, full_range: bool):
    """((yr, yg, yb), (ur, ug, ub), (vr, vg, vb), yo): round(c * 2^14) of the RGB -> YUV matrix of Kr, Kb, derived in float64."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    sy, sc, yo = (1.0, 1.0, 0) if full_range else (219.0 / 255.0, 224.0 / 255.0, 16)
    rows = ((kr * sy, kg * sy, kb * sy),
            (-kr / (2 * (1 - kb)) * sc, -kg / (2 * (1 - kb)) * sc, 0.5 * sc),
            (0.5 * sc, -kg / (2 * (1 - kr)) * sc, -kb / (2 * (1 - kr)) * sc))
    q = tuple(tuple(int(np.floor(c * (1 << SHIFT) + 0.5)) for c in row) for row in rows)
    return q[0], q[1], q[2], yo


def to_surface(rgb: Sequence[int], format: str, matrix: str, full_range: bool):
    """The three bytes of an RGB colour in the space of a surface, logical order: (Y, U, V) for nv12 / i420 by the integer formulas of
    include/demonet_hip.h, (R, G, B) unchanged for rgb24 / bgr24 (the kernel swaps R and B for bgr24)."""
    r, g, b = (int(v) for v in rgb)
    if format in ("rgb24", "bgr24"):
        return r, g, b
    cy, cu, cv, yo = forward_coeffs(matrix, full_range)
    half = 1 << (SHIFT - 1)
    out = []
    for (cr, cg, cb), off in ((cy, yo), (cu, 128), (cv, 128)):
        out.append(min(max(((cr * r + cg * g + cb * b + half) >> SHIFT) + off, 0), 255))      # (>> of a Python int: arithmetic)
    return tuple(out)


def _rgb(v, what):
    if not isinstance(v, (tuple, list)) or len(v) != 3 or not all(isinstance(x, int) and not isinstance(x, bool) and 0 <= x <= 255 for x in v):
        raise ValueError("Overlay: {} must be three ints (R, G, B) in 0 .. 255, got {!r}".format(what, v))
    return tuple(v)


def _int(v, what, lo, hi):
    if not isinstance(v, int) or isinstance(v, bool) or v < lo or v > hi:
        raise ValueError("Overlay: {} takes an int in {} .. {}, got {!r}".format(what, lo, hi, v))
    return v


def _bool(v, what):
    if not isinstance(v, bool):
        raise ValueError("Overlay: {} must be a bool, got {!r}".format(what, v))
    return v


def make_style(thickness=2, fill_alpha=0, pixelate=0, label=True, score=True, hide=False) -> "_lib.OsdStyle":
    """The validated dn_osd_style; ValueError otherwise. Host work only."""
    s = _lib.OsdStyle()
    s.thickness = _int(thickness, "thickness", 0, 16)
    s.fill_alpha = _int(fill_alpha, "fill_alpha", 0, 255)
    if pixelate not in BLOCKS or isinstance(pixelate, bool):
        raise ValueError("Overlay: pixelate takes a block of {}, got {!r}".format(BLOCKS, pixelate))
    s.pixelate = pixelate
    s.flags = (_lib.DN_OSD_LABEL if _bool(label, "label") else 0) | (_lib.DN_OSD_SCORE if _bool(score, "score") else 0) | (
        _lib.DN_OSD_HIDE if _bool(hide, "hide") else 0)
    return s


def check_names(names) -> list:
    """names -> the list of 16-byte NUL-padded records; ValueError naming the label for a name that is not ASCII or longer than 15 characters."""
    if not isinstance(names, (list, tuple)) or not names or len(names) > MAX_LABELS:
        raise ValueError("Overlay: names must be a list of 1 .. {} strings, got {!r}".format(MAX_LABELS, type(names).__name__))
    out = []
    for i, nm in enumerate(names):
        if not isinstance(nm, str):
            raise ValueError("Overlay: the name of label {} must be a str, got {!r}".format(i, nm))
        try:
            raw = nm.encode("ascii")
        except UnicodeEncodeError:
            raise ValueError("Overlay: the name of label {} is not ASCII: {!r}".format(i, nm))
        if len(raw) > 15 or b"\0" in raw:
            raise ValueError("Overlay: the name of label {} has {} characters, a name takes at most 15 and no NUL: {!r}".format(i, len(raw), nm))
        out.append(raw.ljust(16, b"\0"))
    return out


def check_paint(streams: int, device, batch, boxes, scores, labels, counts, ids=None) -> int:
    """What a paint of an overlay of `streams` streams on `device` checks before anything reaches the device (host work only); returns d."""
    if not isinstance(batch, FrameBatch):
        raise ValueError("Overlay: expected a FrameBatch, got {}".format(type(batch).__name__))
    if batch.n != streams:
        raise ValueError("Overlay: a FrameBatch of {} frames, the overlay has {} streams".format(batch.n, streams))
    if batch.device != device:
        raise ValueError("Overlay: the FrameBatch is on {}, the overlay on {}".format(batch.device, device))
    if batch.table is None:
        raise ValueError("Overlay: the FrameBatch names no frames yet: call set() first")
    if not isinstance(boxes, Tensor) or boxes.dim() != 3 or boxes.shape[2] != 4:
        raise ValueError("Overlay: boxes must be [B, d, 4], got {}".format(tuple(boxes.shape) if isinstance(boxes, Tensor) else type(boxes)))
    B, d = int(boxes.shape[0]), int(boxes.shape[1])
    if B != streams:
        raise ValueError("Overlay: {} streams of boxes, the overlay has {}".format(B, streams))
    if d < 1 or d > MAX_D:
        raise ValueError("Overlay: {} rows per stream, the overlay takes 1 .. {}".format(d, MAX_D))
    for t, shape, dtype in ((boxes, (B, d, 4), torch.float32), (scores, (B, d), torch.float32), (labels, (B, d), torch.int64),
                            (counts, (B,), torch.int32)) + (((ids, (B, d), torch.int64),) if ids is not None else ()):
        if not isinstance(t, Tensor) or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != device:
            raise ValueError("Overlay: expected a contiguous {} tensor of shape {} on {}, got {}".format(
                dtype, shape, device, "{} {} on {}".format(t.dtype, tuple(t.shape), t.device) if isinstance(t, Tensor) else type(t)))
    return d


class Overlay:
    """The painter of `streams` video streams; owns the style, name, palette and font tables, the statistics and the workspace on `device`.

    names: one string per label (ASCII, at most 15 characters), or None: 2048 labels named by their number. palette: RGB triples, 1 .. 256 (the
    default: 32 fixed colours); the text on a colour is black or white by its luma. It is converted to the FrameBatch's colour space at the
    first paint, and again when format, matrix or range change. colour_by: "id" (the track id when ids are given, else the label) or "label".
    scale: 1 .. 4, a character cell is 8 scale x 8 scale pixels. thickness, fill_alpha, label, score: the style every label starts with (set_style
    and redact change one label's). label_alpha: the label's opacity. line_colour, zone_colour, zone_alpha, line_thickness: how the lines and
    zones of a ZoneAnalytics are drawn."""

    def __init__(self, streams: int, device, names=None, palette=None, colour_by: str = "id", scale: int = 1, thickness: int = 2,
                 fill_alpha: int = 0, label: bool = True, score: bool = True, label_alpha: int = 255, line_colour=(255, 255, 0),
                 zone_colour=(0, 255, 255), zone_alpha: int = 255, line_thickness: int = 2):
        self.streams = _int(streams, "streams", 1, MAX_STREAMS)
        records = check_names([str(i) for i in range(2048)] if names is None else names)
        self.n_labels = len(records)
        pal = PALETTE if palette is None else palette
        if not isinstance(pal, (list, tuple)) or not 1 <= len(pal) <= MAX_COLORS:
            raise ValueError("Overlay: palette must be a list of 1 .. {} RGB triples".format(MAX_COLORS))
        self.palette = [_rgb(c, "palette entry {}".format(i)) for i, c in enumerate(pal)]
        if colour_by not in ("id", "label"):
            raise ValueError("Overlay: colour_by must be 'id' or 'label', got {!r}".format(colour_by))
        self.colour_by = colour_by
        self.line_colour, self.zone_colour = _rgb(line_colour, "line_colour"), _rgb(zone_colour, "zone_colour")
        default = make_style(thickness, fill_alpha, 0, label, score, False)
        p = _lib.OsdParams()
        p.default_style = default
        p.n_colors, p.color_by_id = len(self.palette), int(colour_by == "id")
        p.scale = _int(scale, "scale", 1, 4)
        p.label_alpha = _int(label_alpha, "label_alpha", 0, 255)
        p.line_thickness = p.zone_thickness = _int(line_thickness, "line_thickness", 1, 64)
        p.zone_alpha = _int(zone_alpha, "zone_alpha", 0, 255)
        self.params = p
        self.styles = [_lib.OsdStyle.from_buffer_copy(default) for _ in range(self.n_labels)]      # host mirror of the device table
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("demonet_amd runs on an MI355X only (the overlay must be on a cuda device); there is no CPU fallback path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        dev = self.device
        self._names = torch.frombuffer(bytearray(b"".join(records)), dtype=torch.uint8).to(dev)
        self._font = torch.from_numpy(osd_font.table().reshape(-1).copy()).to(dev)
        self._styles = torch.zeros(self.n_labels * 8, dtype=torch.uint8, device=dev)
        self._palette = torch.zeros(len(self.palette) * 8, dtype=torch.uint8, device=dev)
        self.stats = torch.zeros((self.streams, 4), dtype=torch.int32, device=dev)
        self._space = None                   # (format, matrix, full_range) the palette on the device is in
        self._ws = {}                        # rows per stream -> (tile capacity, workspace)
        self._upload_styles()

    # ------------------------------------------------------------------------------------------------------
    def _upload(self, dst: Tensor, raw: bytes):
        host = torch.frombuffer(bytearray(raw), dtype=torch.uint8).pin_memory()      # (a copy: the allocator keeps the pinned block until the upload has run)
        dst.copy_(host, non_blocking=True)

    def _upload_styles(self):
        self._upload(self._styles, b"".join(bytes(s) for s in self.styles))

    def _set_space(self, batch: FrameBatch):
        space = (batch.format, batch.matrix, batch.full_range)
        if space == self._space:
            return
        raw = []
        for r, g, b in self.palette:
            text = (0, 0, 0) if (299 * r + 587 * g + 114 * b) >= 128000 else (255, 255, 255)
            raw.append(bytes(to_surface((r, g, b), *space)) + bytes(to_surface(text, *space)) + b"\0\0")
        self._upload(self._palette, b"".join(raw))
        for c in range(3):
            self.params.line_color[c] = to_surface(self.line_colour, *space)[c]
            self.params.zone_color[c] = to_surface(self.zone_colour, *space)[c]
        self._space = space

    def set_style(self, index: int, thickness: Optional[int] = None, fill_alpha: Optional[int] = None, pixelate: Optional[int] = None,
                  label: Optional[bool] = None, score: Optional[bool] = None, hide: Optional[bool] = None):
        """Change how the rows of the label `index` are painted; an argument left out keeps its value. thickness 0 .. 16 (0: no outline), fill_alpha
        0 .. 255, pixelate a block of 0 (off), 4, 8, 16 or 32, label= / score= whether the text and its score part are drawn, hide= whether the
        rows are skipped altogether. Validated on the host before anything changes; the table goes up without a blocking wait."""
        _int(index, "index (the label)", 0, self.n_labels - 1)
        old = self.styles[index]
        pick = lambda new, cur: cur if new is None else new
        self.styles[index] = make_style(pick(thickness, old.thickness), pick(fill_alpha, old.fill_alpha), pick(pixelate, old.pixelate),
                                        pick(label, bool(old.flags & _lib.DN_OSD_LABEL)), pick(score, bool(old.flags & _lib.DN_OSD_SCORE)),
                                        pick(hide, bool(old.flags & _lib.DN_OSD_HIDE)))
        self._upload_styles()
        return self

    def redact(self, labels: Sequence[int], block: int = 16):
        """The rows of these labels are pixelated with this block and get neither outline nor text: faces, plates, persons made unrecognisable."""
        labels = list(labels)
        for lb in labels:
            _int(lb, "label", 0, self.n_labels - 1)
        if block not in BLOCKS[1:] or isinstance(block, bool):
            raise ValueError("Overlay: redact takes a block of {}, got {!r}".format(BLOCKS[1:], block))
        for lb in labels:
            self.styles[lb] = make_style(0, 0, block, False, False, False)
        self._upload_styles()
        return self

    # ------------------------------------------------------------------------------------------------------
    @staticmethod
    def tiles(sizes) -> int:
        """The 32 x 32 tiles of frames of these (height, width): what a paint can touch at most."""
        return sum(((h + 31) // 32) * ((w + 31) // 32) for h, w in sizes)

    def _workspace(self, d: int, capacity: int) -> Tensor:
        have = self._ws.get(d)
        if have is None or have[0] < capacity:
            nbytes = _lib.lib().dn_osd_workspace_bytes(self.streams, d, capacity)
            if nbytes == 0:
                raise ValueError("Overlay: {} streams x {} rows is outside the limits".format(self.streams, d))
            have = self._ws[d] = (capacity, torch.zeros(nbytes, dtype=torch.uint8, device=self.device))
        return have[1]

    def paint(self, batch: FrameBatch, boxes: Tensor, scores: Tensor, labels: Tensor, counts: Tensor, ids: Optional[Tensor] = None, zones=None,
              stream=None) -> Tensor:
        """Paint one step into the frames of the batch, in place: frame b is stream b's. boxes [B, d, 4] fp32 in frame pixels, scores [B, d] fp32,
        labels [B, d] int64, counts [B] int32, ids [B, d] int64 or None -- a tracker's outputs or a forward's --, contiguous, on the overlay's
        device. zones: a zones.ZoneAnalytics of the same streams, whose lines and zone edges are drawn under the boxes, or None. Enqueued on
        `stream` (default: the current stream); no device-to-host copy. Returns stats [B, 4] int32 (rows painted, rows skipped, tiles touched,
        tiles dropped), the overlay's own tensor. The workspace is sized from batch.sizes and grows when a set() changed them; a new one is
        zeroed on `stream`. A CAPTURED GRAPH KEEPS THE WORKSPACE AND THE TILE CAPACITY IT WAS CAPTURED WITH: paint once outside the capture first
        (the fill of a new workspace would otherwise become a node of the graph), and capture again after a set() that made the frames larger --
        a replay on larger frames cannot grow the list, drops the tiles beyond it and says so only in stats[:, 3]."""
        d = check_paint(self.streams, self.device, batch, boxes, scores, labels, counts, ids)
        cfg = None
        if zones is not None:
            from .zones import ZoneAnalytics
            if not isinstance(zones, ZoneAnalytics):
                raise ValueError("Overlay: zones must be a ZoneAnalytics or None, got {}".format(type(zones)))
            if zones.streams != self.streams or zones.device != self.device:
                raise ValueError("Overlay: the analytics has {} streams on {}, the overlay {} on {}".format(
                    zones.streams, zones.device, self.streams, self.device))
            cfg = zones.config
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        if not hasattr(s, "cuda_stream"):
            s = torch.cuda.ExternalStream(int(s), device=self.device)
        p = C.c_void_p
        # everything the call depends on -- the palette's upload, the zeros of a new workspace -- is enqueued on the call's own stream
        with torch.cuda.device(self.device), torch.cuda.stream(s):
            self._set_space(batch)
            ws = self._workspace(d, max(self.tiles(batch.sizes), 1))
            rc = _lib.lib().dn_osd_paint(p(batch.table.data_ptr()), self.streams, batch.format_code, p(boxes.data_ptr()), p(scores.data_ptr()),
                                               p(labels.data_ptr()), p(ids.data_ptr()) if ids is not None else None, p(counts.data_ptr()), d,
                                               p(self._styles.data_ptr()), self.n_labels, p(self._names.data_ptr()), p(self._palette.data_ptr()),
                                               p(self._font.data_ptr()), p(cfg.data_ptr()) if cfg is not None else None, C.byref(self.params),
                                               p(ws.data_ptr()), ws.numel(), p(self.stats.data_ptr()), p(s.cuda_stream))
            if rc == -2:                      # DN_E_HIP: a launch may be missing; the header's recovery is to zero the counters again
                ws[:16].zero_()
            _lib.check(rc, "dn_osd_paint")
        return self.stats


def check_overlay(osd, tracker, who):
    """The `osd=` argument of SSD.track_frames / track_frames_appearance / track_sliced_frames: None or an Overlay of the tracker's streams."""
    if osd is None:
        return
    if not isinstance(osd, Overlay):
        raise ValueError("{}: osd must be an Overlay or None, got {}".format(who, type(osd)))
    if osd.streams != tracker.streams or osd.device != tracker.device:
        raise ValueError("{}: the overlay has {} streams on {}, the tracker {} on {}".format(who, osd.streams, osd.device, tracker.streams, tracker.device))


def painted(outs, osd, batch, analytics):
    """A tracking step's outputs, unchanged; with an Overlay they are painted into the batch's frames first -- the step's last act, behind
    everything that reads the frames."""
    if osd is not None:
        boxes, scores, labels, ids, _, counts = outs[:6]
        osd.paint(batch, boxes, scores, labels, counts, ids=ids, zones=analytics)
    return outs


def paint_frames(model, batch, overlay, boxes, scores, labels, counts, ids=None, zones=None):
    """SSD.paint_frames (see there)."""
    if not isinstance(overlay, Overlay):
        raise ValueError("paint_frames: overlay must be an Overlay, got {}".format(type(overlay)))
    mdev = next(model.parameters()).device
    if mdev != overlay.device:
        raise ValueError("paint_frames: the overlay is on {}, the model on {}".format(overlay.device, mdev))
    return overlay.paint(batch, boxes, scores, labels, counts, ids, zones)
