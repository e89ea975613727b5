"""Multi-object tracking on the device: ByteTrack over batched streams.

A detector that serves 64 camera streams with one frame each per forward needs identities that persist from frame to frame. `ByteTracker` keeps
the tracker state of `streams` independent streams on the device and advances all of them by one frame in ONE launch (include/demonet_hip.h,
dn_track_update, has the semantics: ByteTrack's three association stages and its constant-velocity Kalman filter, greedy association, per-stream
id counters). Nothing is copied to the host and nothing waits: the frame counter and the id counters are part of the device state, so every step is
the same call and can be captured in a graph.
"""
import ctypes as C
from typing import Dict, Optional, Sequence

import torch
from torch import Tensor

from . import _lib

MAX_D = 512                 # detection rows per stream and frame
MAX_TRACKS = 256            # track slots per stream
STATES = ("free", "tentative", "tracked", "lost")
_THRESHOLDS = ("track_thresh", "low_thresh", "new_thresh", "match_thresh", "second_thresh", "unconfirmed_thresh")


def padded_tracks(max_tracks: int) -> int:
    return (max_tracks + 3) & ~3


def state_fields(max_tracks: int) -> Dict[str, tuple]:
    """name -> (byte offset inside a stream's block, torch dtype, shape per stream): the layout include/demonet_hip.h documents."""
    tp = padded_tracks(max_tracks)
    i32, i64, f32 = torch.int32, torch.int64, torch.float32
    return {"header": (0, i32, (4,)), "state": (16, i32, (tp,)), "id": (16 + 4 * tp, i32, (tp,)), "label": (16 + 8 * tp, i64, (tp,)),
            "score": (16 + 16 * tp, f32, (tp,)), "filter": (16 + 20 * tp, f32, (20, tp)), "start_frame": (16 + 100 * tp, i32, (tp,)),
            "last_frame": (16 + 104 * tp, i32, (tp,)), "det": (16 + 108 * tp, i32, (tp,))}


class ByteTracker:
    """ByteTrack for `streams` independent streams on one GPU. update() takes the padded detections of one frame per stream (what forward_batch
    returns) and returns the tracks seen in that frame; all state stays on the device."""

    def __init__(self, streams: int, device, max_tracks: int = 256, track_thresh: float = 0.5, low_thresh: float = 0.1, new_thresh: float = None,
                 match_thresh: float = 0.8, second_thresh: float = 0.5, unconfirmed_thresh: float = 0.7, track_buffer: int = 30,
                 class_agnostic: bool = False):
        streams, max_tracks, track_buffer = int(streams), int(max_tracks), int(track_buffer)
        if streams < 1:
            raise ValueError("ByteTracker: streams must be >= 1, got {}".format(streams))
        if max_tracks < 1 or max_tracks > MAX_TRACKS:
            raise ValueError("ByteTracker: {} track slots per stream, the tracker takes 1 .. {}".format(max_tracks, MAX_TRACKS))
        if track_buffer < 0:
            raise ValueError("ByteTracker: track_buffer must be >= 0, got {}".format(track_buffer))
        track_thresh = float(track_thresh)
        new_thresh = track_thresh + 0.1 if new_thresh is None else float(new_thresh)
        values = dict(track_thresh=track_thresh, low_thresh=float(low_thresh), new_thresh=new_thresh, match_thresh=float(match_thresh),
                      second_thresh=float(second_thresh), unconfirmed_thresh=float(unconfirmed_thresh))
        for name in _THRESHOLDS:
            if not (values[name] >= 0.0):      # (a NaN compares false)
                raise ValueError("ByteTracker: {} must be a number >= 0, got {!r}".format(name, values[name]))
        for name in ("match_thresh", "second_thresh", "unconfirmed_thresh"):
            if values[name] > 1.0:
                raise ValueError("ByteTracker: {} is a cost 1 - IoU, at most 1, got {!r}".format(name, values[name]))
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("ByteTracker needs a GPU device, got {}: there is no CPU path".format(device))
        if device.index is None:                # ("cuda" -> "cuda:0": tensors report their device with the index)
            device = torch.device("cuda", torch.cuda.current_device())
        self.streams, self.max_tracks, self.device = streams, max_tracks, device
        self.params = _lib.TrackParams(track_buffer=track_buffer, class_agnostic=int(bool(class_agnostic)), max_tracks=max_tracks, reserved=0, **values)
        L = _lib.lib()
        nbytes = L.dn_track_state_bytes(streams, max_tracks)
        self._stride = nbytes // streams
        self.state = torch.empty((streams, self._stride), dtype=torch.uint8, device=device)
        self._outs = {}                         # d -> the output tensors of update for that row count
        self._which = None                      # the selection of the last partial reset: kept alive until the next one
        self.reset()

    # ------------------------------------------------------------------------------------------------------
    def _stream(self, stream):
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        return C.c_void_p(s.cuda_stream if hasattr(s, "cuda_stream") else int(s))

    def reset(self, streams: Optional[Sequence[int]] = None, stream=None):
        """Restart every stream (None) or the listed ones: frame 0, ids from 1, an empty table. One launch, no synchronisation."""
        which = None
        if streams is not None:
            idx = [int(i) for i in streams]
            if any(i < 0 or i >= self.streams for i in idx):
                raise ValueError("ByteTracker.reset: stream indices must be in 0 .. {}, got {}".format(self.streams - 1, idx))
            host = torch.zeros(self.streams, dtype=torch.uint8)
            host[idx] = 1
            which = host.to(self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().dn_track_reset(C.c_void_p(self.state.data_ptr()), self.streams, self.max_tracks,
                                                 C.c_void_p(which.data_ptr()) if which is not None else None, self._stream(stream)), "dn_track_reset")
        self._which = which

    def update(self, boxes: Tensor, scores: Tensor, labels: Tensor, counts: Tensor, stream=None):
        """One frame step for every stream. boxes [B, d, 4] fp32, scores [B, d] fp32, labels [B, d] int64, counts [B] int32 on the tracker's device
        (forward_batch's outputs, or ForwardPipeline.outputs(ticket) with stream=pipe.stream_of(ticket)), B = streams. Enqueued on `stream`
        (default: the current stream); no device-to-host copy. Returns padded device tensors (boxes [B, T, 4], scores [B, T], labels [B, T] int64,
        ids [B, T] int64, det [B, T] int32, counts [B] int32, det_ids [B, d] int64), T = max_tracks: the confirmed tracks updated in this frame in
        slot order, and for every detection row the id of the track it updated or -1. The tensors are the tracker's own and are overwritten by
        the next update with the same d."""
        if not isinstance(scores, Tensor) or scores.dim() != 2:
            raise ValueError("ByteTracker.update: scores must be [B, d], got {}".format(tuple(scores.shape) if isinstance(scores, Tensor) else type(scores)))
        B, d = scores.shape
        if B != self.streams:
            raise ValueError("ByteTracker.update: {} streams of detections, the tracker has {}".format(B, self.streams))
        if d < 1 or d > MAX_D:
            raise ValueError("ByteTracker.update: {} rows per stream, the tracker takes 1 .. {}".format(d, MAX_D))
        dev = self.device
        for t, shape, dtype in ((boxes, (B, d, 4), torch.float32), (scores, (B, d), torch.float32), (labels, (B, d), torch.int64),
                                (counts, (B,), torch.int32)):
            if not isinstance(t, Tensor) or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev:
                raise ValueError("ByteTracker.update: expected a contiguous {} tensor of shape {} on {}, got {}".format(
                    dtype, shape, dev, "{} {} on {}".format(t.dtype, tuple(t.shape), t.device) if isinstance(t, Tensor) else type(t)))
        outs = self._outs.get(d)
        if outs is None:
            T = self.max_tracks
            outs = self._outs[d] = (torch.empty((B, T, 4), dtype=torch.float32, device=dev), torch.empty((B, T), dtype=torch.float32, device=dev),
                                    torch.empty((B, T), dtype=torch.int64, device=dev), torch.empty((B, T), dtype=torch.int64, device=dev),
                                    torch.empty((B, T), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev),
                                    torch.empty((B, d), dtype=torch.int64, device=dev))
        p = C.c_void_p
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().dn_track_update(p(boxes.data_ptr()), p(scores.data_ptr()), p(labels.data_ptr()), p(counts.data_ptr()), B, d,
                                                  C.byref(self.params), p(self.state.data_ptr()), self.state.numel(),
                                                  *[p(o.data_ptr()) for o in outs], self._stream(stream)), "dn_track_update")
        return outs

    # ------------------------------------------------------------------------------------------------------
    def table(self) -> Dict[str, Tensor]:
        """Views (no copies) of the device state: frame, next_id, dropped [B] int32 and the per-slot fields state, id, label, score,
        filter [B, 20, T], start_frame, last_frame, det [B, T], the padding slots cut off."""
        out = {}
        T = self.max_tracks
        for name, (off, dtype, shape) in state_fields(self.max_tracks).items():
            n = 1
            for s in shape:
                n *= s
            v = self.state[:, off:off + n * torch.empty((), dtype=dtype).element_size()].view(dtype).view((self.streams,) + shape)
            if name == "header":
                out["frame"], out["next_id"], out["dropped"] = v[:, 0], v[:, 1], v[:, 2]
            else:
                out[name] = v[..., :T]
        return out

    def state_dict(self) -> dict:
        """The state bytes (a host copy: this call waits for the device) and the parameters: load_state_dict resumes the run bit for bit."""
        params = {name: getattr(self.params, name) for name, _ in _lib.TrackParams._fields_ if name != "reserved"}
        return {"state": self.state.cpu(), "streams": self.streams, "params": params}

    def load_state_dict(self, sd: dict):
        if int(sd["streams"]) != self.streams or int(sd["params"]["max_tracks"]) != self.max_tracks:
            raise ValueError("ByteTracker.load_state_dict: the state is for {} streams x {} slots, this tracker has {} x {}".format(
                sd["streams"], sd["params"]["max_tracks"], self.streams, self.max_tracks))
        st = sd["state"]
        if not isinstance(st, Tensor) or st.dtype != torch.uint8 or tuple(st.shape) != tuple(self.state.shape):
            raise ValueError("ByteTracker.load_state_dict: expected a uint8 state of shape {}".format(tuple(self.state.shape)))
        for name, value in sd["params"].items():
            setattr(self.params, name, value)
        self.state.copy_(st)


def with_analytics(outs, analytics):
    """The tracker step's outputs, or -- with a zones.ZoneAnalytics -- those followed by the analytics step's (events, event_counts): the step is
    enqueued behind the tracker's on the same (the current) stream."""
    if analytics is None:
        return outs
    return tuple(outs) + (analytics.update(),)


def track(model, images: Tensor, tracker: ByteTracker, analytics=None):
    """SSD.track (see there)."""
    if model.training:
        raise ValueError("track: the model must be in eval mode")
    if not isinstance(tracker, ByteTracker):
        raise ValueError("track: tracker must be a ByteTracker, got {}".format(type(tracker)))
    if analytics is not None:
        from .zones import check_analytics
        check_analytics(analytics, tracker, "track")
    boxes, scores, labels, counts = model.forward_batch(images)
    return with_analytics(tracker.update(boxes, scores, labels, counts), analytics)
