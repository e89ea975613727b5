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
        B, d, outs = self._check_step(boxes, scores, labels, counts)
        p = C.c_void_p
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().dn_track_update(p(boxes.data_ptr()), p(scores.data_ptr()), p(labels.data_ptr()), p(counts.data_ptr()), B, d,
                                                  C.byref(self.params), p(self.state.data_ptr()), self.state.numel(),
                                                  *[p(o.data_ptr()) for o in outs], self._stream(stream)), "dn_track_update")
        return outs

    def compensate(self, motion: Tensor, stream=None):
        """Camera-motion compensation: warp the state of every stream b with motion[b] = (s, tx, ty, ok), ok != 0, by x' = s x + tx,
        y' = s y + ty -- the centres, the heights, their velocities and covariances (include/demonet_hip.h, dn_track_compensate). motion:
        [B, 4] fp32 on the tracker's device, what motion.MotionCompensator.estimate returns for the frame whose update comes next; a stream
        whose ok is 0 is not written. One launch, no device-to-host copy."""
        if not isinstance(motion, Tensor) or tuple(motion.shape) != (self.streams, 4) or motion.dtype != torch.float32 or not motion.is_contiguous() \
                or motion.device != self.device:
            raise ValueError("ByteTracker.compensate: motion must be a contiguous fp32 [{}, 4] tensor on {}, got {}".format(
                self.streams, self.device, "{} {} on {}".format(motion.dtype, tuple(motion.shape), motion.device) if isinstance(motion, Tensor)
                else type(motion)))
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().dn_track_compensate(C.c_void_p(self.state.data_ptr()), self.state.numel(), self.streams, self.max_tracks,
                                                      C.c_void_p(motion.data_ptr()), self._stream(stream)), "dn_track_compensate")

    def _check_step(self, boxes, scores, labels, counts):
        """What update checks before anything reaches the device -> (B, d, the output tensors of that d)."""
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
        return B, d, outs

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


MAX_E = 8192                # embedding slots per step (the cropper's capacity)
MAX_DIM = 512               # embedding dimension: a multiple of 32 in 32 .. 512
EMB_DTYPES = (torch.float16, torch.float32)


def _up16(v: int) -> int:
    return (v + 15) & ~15


def workspace_fields(streams: int, max_tracks: int, d: int, E: int, dim: int) -> Dict[str, tuple]:
    """name -> (byte offset, torch dtype, shape) of the appearance step's workspace: the layout include/demonet_hip.h documents."""
    tp = padded_tracks(max_tracks)
    present = _up16(E * dim * 2)
    rowmap = present + _up16(E * 4)
    S = rowmap + _up16(streams * d * 4)
    return {"en": (0, torch.float16, (E, dim)), "present": (present, torch.int32, (E,)), "map": (rowmap, torch.int32, (streams, d)),
            "S": (S, torch.float32, (streams, tp, d)), "total": (S + streams * tp * d * 4, torch.uint8, ())}


def appearance_params(dim, alpha=0.9, appearance_thresh=0.25, proximity_thresh=0.5) -> "_lib.TrackAppearanceParams":
    """The validated dn_track_appearance_params of an AppearanceTracker's arguments (emb_fp16 is set per step); ValueError otherwise. Host work
    only."""
    if not isinstance(dim, int) or isinstance(dim, bool) or dim < 32 or dim > MAX_DIM or dim % 32:
        raise ValueError("AppearanceTracker: dim must be a multiple of 32 in 32 .. {}, got {!r}".format(MAX_DIM, dim))
    alpha, appearance_thresh, proximity_thresh = float(alpha), float(appearance_thresh), float(proximity_thresh)
    if not (0.0 <= alpha <= 1.0):               # (a NaN compares false)
        raise ValueError("AppearanceTracker: alpha must be a number in 0 .. 1, got {!r}".format(alpha))
    for name, v in (("appearance_thresh", appearance_thresh), ("proximity_thresh", proximity_thresh)):
        if not (v >= 0.0):
            raise ValueError("AppearanceTracker: {} must be a number >= 0, got {!r}".format(name, v))
    return _lib.TrackAppearanceParams(dim=dim, alpha=alpha, appearance_thresh=appearance_thresh, proximity_thresh=proximity_thresh, emb_fp16=0)


class AppearanceTracker(ByteTracker):
    """ByteTrack with BoT-SORT's appearance term (Aharon et al. 2022): update() also takes the re-identification embeddings of the
    frame's detection rows, as a second model computed them from an ObjectCropper's patches, and fuses appearance with IoU in stages 1 and 3
    (include/demonet_hip.h, dn_track_update_appearance, has the rules). Every track keeps an exponentially smoothed unit-norm feature on the
    device. Everything a ByteTracker is bound to -- ZoneAnalytics, ObjectCropper.gather, SSD.track* -- works with it unchanged.

    dim: the embedding dimension. alpha: the feature's smoothing. appearance_thresh: the largest (1 - cosine) / 2 at which appearance counts.
    proximity_thresh: the largest 1 - IoU at which it counts; 1 lets a lost track be found again without overlap. The others: ByteTracker's."""

    def __init__(self, streams: int, device, dim: int, alpha: float = 0.9, appearance_thresh: float = 0.25, proximity_thresh: float = 0.5, **kwargs):
        self.app = appearance_params(dim, alpha, appearance_thresh, proximity_thresh)
        self.dim = dim
        self.features_buf = None                # (ByteTracker's constructor resets: nothing to clear yet)
        super().__init__(streams, device, **kwargs)
        nbytes = _lib.lib().dn_track_feature_bytes(self.streams, self.max_tracks, dim)
        self.features_buf = torch.empty((self.streams, nbytes // self.streams), dtype=torch.uint8, device=self.device)
        self._ws = {}                           # (d, E) -> the workspace of a step with E embedding slots
        self._last = None                       # the (d, E) of the last step that had embeddings
        self._reset_features(None, None)

    def _reset_features(self, which, stream):
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().dn_track_feature_reset(C.c_void_p(self.features_buf.data_ptr()), self.streams, self.max_tracks, self.dim,
                                                         C.c_void_p(which.data_ptr()) if which is not None else None, self._stream(stream)),
                       "dn_track_feature_reset")

    def reset(self, streams: Optional[Sequence[int]] = None, stream=None):
        """ByteTracker.reset, and the features of the same streams are cleared: one more launch."""
        super().reset(streams, stream)
        if self.features_buf is not None:
            self._reset_features(self._which, stream)

    def update(self, boxes: Tensor, scores: Tensor, labels: Tensor, counts: Tensor, embeddings: Optional[Tensor] = None,
               index: Optional[Tensor] = None, stream=None):
        """ByteTracker.update with appearance. embeddings [E, dim] fp16 or fp32 and index [E, 8] int32 (an ObjectCropper's index table as it lies:
        word 0 the stream or -1, word 1 the row), contiguous, on the tracker's device, E = 1 .. 8192. Neither is trusted: rows the index does not
        name validly, and embeddings that hold a non-finite element or have norm 0, are as if absent. With embeddings=None the step is
        ByteTracker's (the same outputs and state, bit for bit; the features of freed slots are still cleared). Four graph nodes with embeddings,
        one without; no device-to-host copy. Returns what ByteTracker.update returns."""
        B, d, outs = self._check_step(boxes, scores, labels, counts)
        p = C.c_void_p
        if embeddings is None:
            if index is not None:
                raise ValueError("AppearanceTracker.update: an index table without embeddings")
            E, emb, idx, ws, wsn = 0, None, None, None, 0
            self.app.emb_fp16 = 0
        else:
            if not isinstance(embeddings, Tensor) or embeddings.dim() != 2 or embeddings.shape[1] != self.dim or embeddings.dtype not in EMB_DTYPES \
                    or not embeddings.is_contiguous() or embeddings.device != self.device:
                raise ValueError("AppearanceTracker.update: embeddings must be a contiguous fp16 or fp32 [E, {}] tensor on {}, got {}".format(
                    self.dim, self.device, "{} {} on {}".format(embeddings.dtype, tuple(embeddings.shape), embeddings.device)
                    if isinstance(embeddings, Tensor) else type(embeddings)))
            E = int(embeddings.shape[0])
            if E < 1 or E > MAX_E:
                raise ValueError("AppearanceTracker.update: {} embedding slots, the tracker takes 1 .. {}".format(E, MAX_E))
            if not isinstance(index, Tensor) or tuple(index.shape) != (E, 8) or index.dtype != torch.int32 or not index.is_contiguous() \
                    or index.device != self.device:
                raise ValueError("AppearanceTracker.update: index must be a contiguous int32 [{}, 8] tensor on {}, got {}".format(
                    E, self.device, "{} {} on {}".format(index.dtype, tuple(index.shape), index.device) if isinstance(index, Tensor) else type(index)))
            if embeddings.data_ptr() % 16 or index.data_ptr() % 16:
                raise ValueError("AppearanceTracker.update: embeddings and index must be 16-byte aligned")
            buf = self._ws.get((d, E))
            if buf is None:
                n = _lib.lib().dn_track_appearance_workspace_bytes(B, self.max_tracks, d, E, self.dim)
                buf = self._ws[(d, E)] = torch.empty(n, dtype=torch.uint8, device=self.device)
            self._last = (d, E)
            self.app.emb_fp16 = int(embeddings.dtype == torch.float16)
            emb, idx, ws, wsn = p(embeddings.data_ptr()), p(index.data_ptr()), p(buf.data_ptr()), buf.numel()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().dn_track_update_appearance(
                p(boxes.data_ptr()), p(scores.data_ptr()), p(labels.data_ptr()), p(counts.data_ptr()), B, d, C.byref(self.params), C.byref(self.app),
                emb, idx, E, p(self.state.data_ptr()), self.state.numel(), p(self.features_buf.data_ptr()), self.features_buf.numel(), ws, wsn,
                *[p(o.data_ptr()) for o in outs], self._stream(stream)), "dn_track_update_appearance")
        return outs

    # ------------------------------------------------------------------------------------------------------
    def features(self):
        """Views (no copies) of the device features: (valid [B, T] int32, feature [B, T, dim] fp32). The values of a slot whose flag is 0 mean
        nothing."""
        tp, T = padded_tracks(self.max_tracks), self.max_tracks
        valid = self.features_buf[:, :4 * tp].view(torch.int32)[:, :T]
        feat = self.features_buf[:, 4 * tp:].view(torch.float32).view(self.streams, tp, self.dim)[:, :T]
        return valid, feat

    def _ws_view(self, name):
        if self._last is None:
            raise RuntimeError("AppearanceTracker: no step with embeddings yet")
        d, E = self._last
        off, dtype, shape = workspace_fields(self.streams, self.max_tracks, d, E, self.dim)[name]
        n = 1
        for s in shape:
            n *= s
        return self._ws[(d, E)][off:off + n * torch.empty((), dtype=dtype).element_size()].view(dtype).view(shape)

    def similarity(self) -> Tensor:
        """A view of the last step's S [B, T, d] fp32: fp16(feature) . en with fp32 accumulation, 0 where the slot or the row has no feature."""
        return self._ws_view("S")[:, :self.max_tracks]

    def normalised(self) -> Tensor:
        """A view of the last step's normalised embedding rows en [E, dim] fp16 (absent embeddings: 0)."""
        return self._ws_view("en")

    def state_dict(self) -> dict:
        """ByteTracker.state_dict with the features and the appearance parameters: load_state_dict resumes the run bit for bit."""
        sd = super().state_dict()
        sd["features"] = self.features_buf.cpu()
        sd["appearance"] = {k: getattr(self.app, k) for k in ("dim", "alpha", "appearance_thresh", "proximity_thresh")}
        return sd

    def load_state_dict(self, sd: dict):
        ft = sd.get("features")
        if "appearance" not in sd or int(sd["appearance"]["dim"]) != self.dim:
            raise ValueError("AppearanceTracker.load_state_dict: the state has no features of dimension {}".format(self.dim))
        if not isinstance(ft, Tensor) or ft.dtype != torch.uint8 or tuple(ft.shape) != tuple(self.features_buf.shape):
            raise ValueError("AppearanceTracker.load_state_dict: expected uint8 features of shape {}".format(tuple(self.features_buf.shape)))
        super().load_state_dict(sd)
        for name, value in sd["appearance"].items():
            setattr(self.app, name, value)
        self.features_buf.copy_(ft)


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
