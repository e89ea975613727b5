"""Line-crossing and zone analytics on the device, behind the tracker.

`ZoneAnalytics` binds to a `ByteTracker` and keeps, per stream, up to 16 directed lines and 16 polygon zones with their counters on the device:
crossings per line, direction and class bin; entries, exits, vanishings, occupancy and dwell per zone and class bin; and the events of the last
step. `update()` is ONE small launch behind the tracker's (include/demonet_hip.h, dn_zone_update, has the rules). It reads the tracker's state where
it lies and never writes it. Lines, zones and the class map live in device memory, so a captured step follows edits; the host reads the counters
every N frames, or never.
"""
import ctypes as C
import math
from typing import Dict, Optional, Sequence

import torch
from torch import Tensor

from . import _lib
from .track import ByteTracker, padded_tracks

MAX_LINES, MAX_ZONES, MAX_VERTS, BINS = 16, 16, 16, 8
MAX_EVENTS = 1024
IGNORE = 255                                # a class-bin value: tracks of this label are ignored
ANCHORS = {"center": 0, "bottom": 1}


def state_fields(max_tracks: int) -> Dict[str, tuple]:
    """name -> (byte offset inside a stream's block, torch dtype, shape per stream): the zone state's layout of include/demonet_hip.h."""
    tp = padded_tracks(max_tracks)
    i32, i64, f32 = torch.int32, torch.int64, torch.float32
    c = 16 + 88 * tp
    return {"header": (0, i32, (4,)), "id": (16, i32, (tp,)), "bin": (16 + 4 * tp, i32, (tp,)), "has_prev": (16 + 8 * tp, i32, (tp,)),
            "px": (16 + 12 * tp, f32, (tp,)), "py": (16 + 16 * tp, f32, (tp,)), "inside": (16 + 20 * tp, i32, (tp,)),
            "enter_frame": (16 + 24 * tp, i32, (16, tp)), "line_count": (c, i32, (16, 2, 8)), "entries": (c + 1024, i32, (16, 8)),
            "exits": (c + 1536, i32, (16, 8)), "vanished": (c + 2048, i32, (16, 8)), "occupancy": (c + 2560, i32, (16, 8)),
            "dwell_max": (c + 3072, i32, (16, 8)), "dwell_sum": (c + 3584, i64, (16, 8))}


def _number(v, what):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError("{}: expected a number, got {!r}".format(what, v))
    if not math.isfinite(v):
        raise ValueError("{}: coordinates must be finite, got {!r}".format(what, v))
    return v


def config_record(lines: Sequence = (), zones: Sequence = ()) -> "_lib.ZoneConfig":
    """The validated dn_zone_config of one stream: lines = [(ax, ay, bx, by)], zones = [[(x, y), ...]] in frame pixels. Host work only.
    ValueError for more than 16 of either, a number that is not finite, a line whose ends coincide, a polygon of fewer than 3 or more than 16
    vertices."""
    lines, zones = list(lines), list(zones)
    if len(lines) > MAX_LINES:
        raise ValueError("{} lines, a stream takes at most {}".format(len(lines), MAX_LINES))
    if len(zones) > MAX_ZONES:
        raise ValueError("{} zones, a stream takes at most {}".format(len(zones), MAX_ZONES))
    rec = _lib.ZoneConfig()
    rec.n_lines, rec.n_zones = len(lines), len(zones)
    for i, ln in enumerate(lines):
        ln = tuple(ln)
        if len(ln) != 4:
            raise ValueError("line {}: expected (ax, ay, bx, by), got {!r}".format(i, ln))
        v = [_number(x, "line {}".format(i)) for x in ln]
        f = [C.c_float(x).value for x in v]
        if f[0] == f[2] and f[1] == f[3]:
            raise ValueError("line {}: its two ends coincide at ({}, {})".format(i, f[0], f[1]))
        for k in range(4):
            rec.lines[i][k] = v[k]
    for z, poly in enumerate(zones):
        poly = [tuple(p) for p in poly]
        if len(poly) < 3 or len(poly) > MAX_VERTS:
            raise ValueError("zone {}: {} vertices, a polygon takes 3 .. {}".format(z, len(poly), MAX_VERTS))
        rec.nv[z] = len(poly)
        for e, p in enumerate(poly):
            if len(p) != 2:
                raise ValueError("zone {}, vertex {}: expected (x, y), got {!r}".format(z, e, p))
            rec.verts[z][e][0], rec.verts[z][e][1] = (_number(x, "zone {}, vertex {}".format(z, e)) for x in p)
    return rec


class ZoneAnalytics:
    """Counters and events for the tracks of a ByteTracker: its streams, its max_tracks, its device.

    anchor: the point of a track's box that is tested, "bottom" (the bottom centre: where an upright object stands) or "center".
    class_bins: None (every label counts in bin 0) or a sequence, label l -> bin 0 .. 7 or IGNORE (255); labels beyond it are ignored.
    max_events: rows of the per-step event list, 1 .. 1024; what a step emits beyond them is counted in events_dropped."""

    def __init__(self, tracker: ByteTracker, anchor: str = "bottom", class_bins: Optional[Sequence[int]] = None, max_events: int = 256):
        if not isinstance(tracker, ByteTracker):
            raise ValueError("ZoneAnalytics: tracker must be a ByteTracker, got {}".format(type(tracker)))
        if anchor not in ANCHORS:
            raise ValueError("ZoneAnalytics: anchor must be one of {}, got {!r}".format(sorted(ANCHORS), anchor))
        max_events = int(max_events)
        if max_events < 1 or max_events > MAX_EVENTS:
            raise ValueError("ZoneAnalytics: max_events = {}, the event list takes 1 .. {} rows".format(max_events, MAX_EVENTS))
        self.tracker, self.anchor, self.max_events = tracker, anchor, max_events
        self.streams, self.max_tracks, self.device = tracker.streams, tracker.max_tracks, tracker.device
        dev = self.device
        self.class_bins = None
        self._bins = None
        if class_bins is not None:
            bins = [int(v) for v in class_bins]
            if not bins:
                raise ValueError("ZoneAnalytics: class_bins is empty")
            if any((v < 0 or v >= BINS) and v != IGNORE for v in bins):
                raise ValueError("ZoneAnalytics: class bins are 0 .. {} or {} (ignored), got {}".format(BINS - 1, IGNORE, bins))
            self.class_bins = tuple(bins)
            self._bins = torch.tensor(bins, dtype=torch.uint8).to(dev)
        nbytes = _lib.lib().dn_zone_state_bytes(self.streams, self.max_tracks)
        if nbytes == 0:
            raise ValueError("ZoneAnalytics: {} streams x {} slots is outside the limits".format(self.streams, self.max_tracks))
        self.state = torch.empty((self.streams, nbytes // self.streams), dtype=torch.uint8, device=dev)
        self._rec = C.sizeof(_lib.ZoneConfig)
        self.config = torch.zeros((self.streams, self._rec), dtype=torch.uint8, device=dev)     # (all zero: no lines, no zones)
        self.events = torch.zeros((self.streams, max_events, 8), dtype=torch.int32, device=dev)
        self.event_counts = torch.zeros((self.streams,), dtype=torch.int32, device=dev)
        self._records = [config_record() for _ in range(self.streams)]      # host mirrors of the device records
        self._which = None
        self.reset()

    # ------------------------------------------------------------------------------------------------------
    def _stream(self, stream):
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        return C.c_void_p(s.cuda_stream if hasattr(s, "cuda_stream") else int(s))

    def _check_stream(self, stream):
        if not isinstance(stream, int) or isinstance(stream, bool) or stream < 0 or stream >= self.streams:
            raise ValueError("ZoneAnalytics: stream must be an index in 0 .. {}, got {!r}".format(self.streams - 1, stream))

    def _upload(self, first, records):
        """records -> the device records first .. first + len(records) - 1, from pinned memory on the current stream; the host does not wait."""
        raw = b"".join(bytes(r) for r in records)
        host = torch.frombuffer(bytearray(raw), dtype=torch.uint8).pin_memory()      # (a copy: the allocator keeps the pinned block until the upload has run)
        self.config[first:first + len(records)].view(-1).copy_(host, non_blocking=True)
        for i, r in enumerate(records):
            self._records[first + i] = r

    def _edited(self, stream, lines=None, zones=None):
        old = self._records[stream]
        rec = config_record(() if lines is None else lines, () if zones is None else zones)
        if lines is None:
            rec.n_lines = old.n_lines
            C.memmove(rec.lines, old.lines, C.sizeof(old.lines))
        if zones is None:
            rec.n_zones = old.n_zones
            C.memmove(rec.nv, old.nv, C.sizeof(old.nv))
            C.memmove(rec.verts, old.verts, C.sizeof(old.verts))
        return rec

    def set_lines(self, stream: int, lines: Sequence):
        """The lines of one stream, [(ax, ay, bx, by)] in frame pixels, at most 16; its zones stay. A crossing is counted in direction 0 when the
        anchor ends on the side where (bx - ax) * (py - ay) - (by - ay) * (px - ax) >= 0, else in direction 1: in image coordinates (y down), for a
        line drawn left to right direction 0 is downwards. Validated on the host before anything changes; one record goes up without a blocking wait."""
        self._check_stream(stream)
        self._upload(stream, [self._edited(stream, lines=lines)])
        return self

    def set_zones(self, stream: int, polygons: Sequence):
        """The zones of one stream, [[(x, y), ...]] of 3 .. 16 vertices each, at most 16 (even-odd rule; concave polygons are fine); its lines stay."""
        self._check_stream(stream)
        self._upload(stream, [self._edited(stream, zones=polygons)])
        return self

    def set_all(self, lines: Sequence, zones: Sequence):
        """The same lines and zones for every stream: one upload."""
        rec = config_record(lines, zones)
        self._upload(0, [_lib.ZoneConfig.from_buffer_copy(rec) for _ in range(self.streams)])
        return self

    # ------------------------------------------------------------------------------------------------------
    def reset(self, streams: Optional[Sequence[int]] = None, stream=None):
        """Clear every stream (None) or the listed ones, ByteTracker.reset's selection: counters, events_dropped and the per-slot memory become
        zero; lines and zones stay. One launch, no synchronisation."""
        which = None
        if streams is not None:
            idx = [int(i) for i in streams]
            if any(i < 0 or i >= self.streams for i in idx):
                raise ValueError("ZoneAnalytics.reset: stream indices must be in 0 .. {}, got {}".format(self.streams - 1, idx))
            host = torch.zeros(self.streams, dtype=torch.uint8)
            host[idx] = 1
            which = host.to(self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().dn_zone_reset(C.c_void_p(self.state.data_ptr()), self.streams, self.max_tracks,
                                                C.c_void_p(which.data_ptr()) if which is not None else None, self._stream(stream)), "dn_zone_reset")
        self._which = which

    def update(self, stream=None):
        """One analytics step for every stream, from the tracker's state as its last update left it: call it after ByteTracker.update on the same
        stream. Enqueued on `stream` (default: the current stream); no device-to-host copy. Returns views (events [B, max_events, 8] int32 --
        rows (kind, index, id, label, bin, frame, dwell, direction), zero at and beyond the count -- and event_counts [B] int32): the analytics'
        own tensors, overwritten by the next update."""
        t = self.tracker
        if t.streams != self.streams or t.max_tracks != self.max_tracks or t.device != self.device:
            raise ValueError("ZoneAnalytics.update: the tracker has {} streams x {} slots on {}, the analytics {} x {} on {}".format(
                t.streams, t.max_tracks, t.device, self.streams, self.max_tracks, self.device))
        p = C.c_void_p
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().dn_zone_update(p(t.state.data_ptr()), t.state.numel(), self.streams, self.max_tracks, p(self.config.data_ptr()),
                                                 p(self._bins.data_ptr()) if self._bins is not None else None,
                                                 len(self.class_bins) if self.class_bins is not None else 0, ANCHORS[self.anchor],
                                                 p(self.state.data_ptr()), self.state.numel(), p(self.events.data_ptr()),
                                                 p(self.event_counts.data_ptr()), self.max_events, self._stream(stream)), "dn_zone_update")
        return self.events, self.event_counts

    # ------------------------------------------------------------------------------------------------------
    def table(self) -> Dict[str, Tensor]:
        """Views (no copies) of every field of the device state: events_dropped [B]; the per-slot fields id, bin, has_prev, px, py, inside [B, T],
        enter_frame [B, 16, T], the padding slots cut off; and the counters of `counters`."""
        out = {}
        T = self.max_tracks
        for name, (off, dtype, shape) in state_fields(self.max_tracks).items():
            n = 1
            for s in shape:
                n *= s
            v = self.state[:, off:off + n * torch.empty((), dtype=dtype).element_size()].view(dtype).view((self.streams,) + shape)
            if name == "header":
                out["events_dropped"] = v[:, 0]
            elif name in ("id", "bin", "has_prev", "px", "py", "inside", "enter_frame"):
                out[name] = v[..., :T]
            else:
                out[name] = v
        return out

    def counters(self) -> Dict[str, Tensor]:
        """Views (no copies) into the device state: line_count [B, 16, 2, 8] (line, direction, bin); entries, exits, vanished, occupancy, dwell_max
        [B, 16, 8] (zone, bin) int32; dwell_sum [B, 16, 8] int64, in frames; events_dropped [B]. Reading them on the host waits for the device."""
        t = self.table()
        return {k: t[k] for k in ("line_count", "entries", "exits", "vanished", "occupancy", "dwell_sum", "dwell_max", "events_dropped")}

    def state_dict(self) -> dict:
        """The state and configuration bytes (host copies: this call waits for the device) and the settings: load_state_dict resumes bit for bit."""
        return {"state": self.state.cpu(), "config": self.config.cpu(), "streams": self.streams, "max_tracks": self.max_tracks, "anchor": self.anchor,
                "class_bins": self.class_bins, "max_events": self.max_events}

    def load_state_dict(self, sd: dict):
        if int(sd["streams"]) != self.streams or int(sd["max_tracks"]) != self.max_tracks:
            raise ValueError("ZoneAnalytics.load_state_dict: the state is for {} streams x {} slots, this instance has {} x {}".format(
                sd["streams"], sd["max_tracks"], self.streams, self.max_tracks))
        if sd["anchor"] != self.anchor or (None if sd["class_bins"] is None else tuple(sd["class_bins"])) != self.class_bins:
            raise ValueError("ZoneAnalytics.load_state_dict: the state was kept with anchor {!r} and class bins {}, this instance has {!r} and {}".format(
                sd["anchor"], sd["class_bins"], self.anchor, self.class_bins))
        for name, mine in (("state", self.state), ("config", self.config)):
            t = sd[name]
            if not isinstance(t, Tensor) or t.dtype != torch.uint8 or tuple(t.shape) != tuple(mine.shape):
                raise ValueError("ZoneAnalytics.load_state_dict: expected a uint8 {} of shape {}".format(name, tuple(mine.shape)))
        host = sd["config"].contiguous()
        self.state.copy_(sd["state"])
        self.config.copy_(host)
        raw = bytes(host.numpy().tobytes())
        self._records = [_lib.ZoneConfig.from_buffer_copy(raw[i * self._rec:(i + 1) * self._rec]) for i in range(self.streams)]


def check_analytics(analytics, tracker, who):
    """The `analytics=` argument of SSD.track / track_frames / track_sliced_frames: None or a ZoneAnalytics bound to this tracker."""
    if analytics is None:
        return
    if not isinstance(analytics, ZoneAnalytics):
        raise ValueError("{}: analytics must be a ZoneAnalytics or None, got {}".format(who, type(analytics)))
    if analytics.tracker is not tracker:
        raise ValueError("{}: the analytics is bound to another tracker".format(who))
