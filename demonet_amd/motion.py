"""Camera-motion compensation for the trackers on the device: the third part of BoT-SORT.

The trackers' filter is constant-velocity in image coordinates, which is right for a fixed camera only: on a PTZ, handheld, vehicle or drone
camera a pan of a few dozen pixels per frame moves every predicted box off its object. A `MotionCompensator` measures, per stream and frame
step, the global motion of the image (translation + isotropic scale, previous frame -> current frame) from the luma of the surfaces of a
`FrameBatch`, and `ByteTracker.compensate` applies it to the tracker's state in front of that frame's `update` (include/demonet_hip.h,
dn_motion_estimate and dn_track_compensate, has the semantics). Nothing is copied to the host and nothing waits: the previous frame's thumbnail
and the parity word that selects it are part of the device state, so every step is the same call and can be captured in a graph.

    mc = MotionCompensator(streams, "cuda:0")
    boxes, scores, labels, counts = model.forward_frames(batch)
    motion, stats = mc.estimate(batch, boxes, scores, counts)     # the frame's detections mask the moving objects out of the estimate
    tracker.compensate(motion)
    tracks = tracker.update(boxes, scores, labels, counts)
    # or: model.track_frames(batch, tracker, motion=mc)
"""
import ctypes as C
from typing import Optional, Sequence

import torch
from torch import Tensor

from . import _lib

MAX_SIDE = 512              # thumbnail capacity per side
MAX_RADIUS = 16
MAX_K = 4096                # the box filter's side: k * k * 255 stays below 2^32
MAX_D = 512                 # masking rows per stream
MAX_STREAMS = 65535
BLOCKS = (8, 16)


def box_side(H: int, W: int, TH: int, TW: int) -> int:
    """k: the smallest integer >= 1 with floor(W / k) <= TW and floor(H / k) <= TH."""
    return max(W // (TW + 1), H // (TH + 1)) + 1


def motion_params(max_size=(144, 256), block=16, radius=16, min_texture=None, min_blocks=8, mask_thresh=0.5) -> "_lib.MotionParams":
    """The validated dn_motion_params of a MotionCompensator's arguments; ValueError otherwise. Host work only."""
    if not isinstance(block, int) or isinstance(block, bool) or block not in BLOCKS:
        raise ValueError("MotionCompensator: block must be 8 or 16, got {!r}".format(block))
    if not isinstance(radius, int) or isinstance(radius, bool) or radius < 1 or radius > MAX_RADIUS:
        raise ValueError("MotionCompensator: radius must be an int in 1 .. {}, got {!r}".format(MAX_RADIUS, radius))
    if not isinstance(max_size, (tuple, list)) or len(max_size) != 2 or not all(isinstance(v, int) and not isinstance(v, bool) for v in max_size):
        raise ValueError("MotionCompensator: max_size must be (height, width) ints, got {!r}".format(max_size))
    need = block + 2 * radius
    if any(v < need or v > MAX_SIDE for v in max_size):
        raise ValueError("MotionCompensator: max_size {} x {}, each side must be block + 2 radius = {} .. {}".format(max_size[0], max_size[1], need, MAX_SIDE))
    min_texture = 2 * block * block if min_texture is None else min_texture
    for name, v, low in (("min_texture", min_texture, 0), ("min_blocks", min_blocks, 1)):
        if not isinstance(v, int) or isinstance(v, bool) or v < low or v > 2 ** 31 - 1:
            raise ValueError("MotionCompensator: {} must be an int >= {}, got {!r}".format(name, low, v))
    mask_thresh = float(mask_thresh)
    if mask_thresh != mask_thresh:
        raise ValueError("MotionCompensator: mask_thresh must be a number, got {!r}".format(mask_thresh))
    return _lib.MotionParams(max_h=max_size[0], max_w=max_size[1], block=block, radius=radius, min_texture=min_texture, min_blocks=min_blocks,
                             mask_thresh=mask_thresh, reserved=0)


def max_blocks(p) -> int:
    return ((p.max_w - 2 * p.radius) // p.block) * ((p.max_h - 2 * p.radius) // p.block)


def state_fields(p) -> dict:
    """name -> (byte offset inside a stream's block, torch dtype, shape per stream), and "stride": the layout include/demonet_hip.h documents."""
    twp = (p.max_w + 15) & ~15
    nb = max_blocks(p)
    return {"header": (0, torch.int32, (4,)), "vectors": (16, torch.int32, (nb, 4)), "thumbs": (16 + 16 * nb, torch.uint8, (2, p.max_h, twp)),
            "stride": 16 + 16 * nb + 2 * p.max_h * twp}


def check_sizes(sizes: Sequence, p) -> list:
    """Per frame (height, width) -> its k; ValueError for a frame whose thumbnail is smaller than block + 2 radius on a side, or whose box filter
    would overflow (k above 4096: k * k * 255 must stay below 2^32). Host work only."""
    need = p.block + 2 * p.radius
    ks = []
    for i, (H, W) in enumerate(sizes):
        k = box_side(H, W, p.max_h, p.max_w)
        if k > MAX_K:
            raise ValueError("MotionCompensator.estimate: frame {} of {} x {} (height x width) needs a {} x {} box filter, at most {}".format(i, H, W, k, k, MAX_K))
        if H // k < need or W // k < need:
            raise ValueError("MotionCompensator.estimate: frame {} of {} x {} (height x width) gives a {} x {} thumbnail, smaller than one block and "
                             "its search range ({})".format(i, H, W, H // k, W // k, need))
        ks.append(k)
    return ks


class MotionCompensator:
    """Global motion of `streams` independent video streams on one GPU. estimate() takes the FrameBatch of the current frames (frame b is the
    current frame of stream b) and returns the motion previous frame -> current frame of every stream; all state stays on the device.

    max_size: the thumbnail capacity (height, width); a frame is box-filtered by the smallest integer factor that fits it. block: 8 or 16
    thumbnail pixels; radius: the search range, 1 .. 16 thumbnail pixels (times the factor in frame pixels: 128 at full HD with the defaults).
    min_texture: the smallest sum |p - mean| of a block that is searched (default 2 block^2); min_blocks: the fewest valid blocks of an
    estimate; mask_thresh: detections with at least this score mask the blocks whose centre they cover."""

    def __init__(self, streams: int, device, max_size=(144, 256), block: int = 16, radius: int = 16, min_texture: Optional[int] = None,
                 min_blocks: int = 8, mask_thresh: float = 0.5):
        if not isinstance(streams, int) or isinstance(streams, bool) or streams < 1 or streams > MAX_STREAMS:
            raise ValueError("MotionCompensator: streams must be an int in 1 .. {}, got {!r}".format(MAX_STREAMS, streams))
        self.params = motion_params(max_size, block, radius, min_texture, min_blocks, mask_thresh)
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("MotionCompensator needs a GPU device, got {}: there is no CPU path".format(device))
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.streams, self.device = streams, device
        self.max_blocks = max_blocks(self.params)
        self._fields = state_fields(self.params)
        nbytes = _lib.lib().dn_motion_state_bytes(streams, C.byref(self.params))
        if nbytes != streams * self._fields["stride"]:
            raise RuntimeError("MotionCompensator: the library's state size {} is not the documented layout's {}".format(nbytes, streams * self._fields["stride"]))
        self.state = torch.empty((streams, self._fields["stride"]), dtype=torch.uint8, device=device)
        self.motion = torch.empty((streams, 4), dtype=torch.float32, device=device)
        self.stats = torch.empty((streams, 4), dtype=torch.int32, device=device)
        self._vectors = torch.empty((streams, self.max_blocks, 4), dtype=torch.int32, device=device)
        self._which = None
        self.reset()

    def _stream(self, stream):
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        return C.c_void_p(s.cuda_stream if hasattr(s, "cuda_stream") else int(s))

    def reset(self, streams: Optional[Sequence[int]] = None, stream=None):
        """Forget the previous frame of every stream (None) or of the listed ones: their next step re-seeds. One launch, no synchronisation."""
        which = None
        if streams is not None:
            idx = [int(i) for i in streams]
            if any(i < 0 or i >= self.streams for i in idx):
                raise ValueError("MotionCompensator.reset: stream indices must be in 0 .. {}, got {}".format(self.streams - 1, idx))
            host = torch.zeros(self.streams, dtype=torch.uint8)
            host[idx] = 1
            which = host.to(self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().dn_motion_reset(C.c_void_p(self.state.data_ptr()), self.state.numel(), self.streams, C.byref(self.params),
                                                  C.c_void_p(which.data_ptr()) if which is not None else None, self._stream(stream)), "dn_motion_reset")
        self._which = which

    def _check(self, batch, boxes, scores, counts):
        """What estimate checks before anything reaches the library -> d."""
        from .frames import FrameBatch
        if not isinstance(batch, FrameBatch):
            raise ValueError("MotionCompensator.estimate: expected a FrameBatch, got {}".format(type(batch).__name__))
        if batch.device != self.device:
            raise ValueError("MotionCompensator.estimate: the FrameBatch is on {}, the compensator on {}".format(batch.device, self.device))
        if batch.n != self.streams:
            raise ValueError("MotionCompensator.estimate: {} frames, the compensator has {} streams".format(batch.n, self.streams))
        if batch.table is None:
            raise ValueError("MotionCompensator.estimate: the FrameBatch names no frames yet: call set() first")
        check_sizes(batch.sizes, self.params)
        given = [t is not None for t in (boxes, scores, counts)]
        if not any(given):
            return 0
        if not all(given):
            raise ValueError("MotionCompensator.estimate: boxes, scores and counts come together or not at all")
        if not isinstance(scores, Tensor) or scores.dim() != 2:
            raise ValueError("MotionCompensator.estimate: scores must be [B, d], got {}".format(tuple(scores.shape) if isinstance(scores, Tensor) else type(scores)))
        B, d = scores.shape
        if B != self.streams:
            raise ValueError("MotionCompensator.estimate: {} streams of detections, the compensator has {}".format(B, self.streams))
        if d < 1 or d > MAX_D:
            raise ValueError("MotionCompensator.estimate: {} rows per stream, the compensator takes 1 .. {}".format(d, MAX_D))
        for t, shape, dtype in ((boxes, (B, d, 4), torch.float32), (scores, (B, d), torch.float32), (counts, (B,), torch.int32)):
            if not isinstance(t, Tensor) or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != self.device:
                raise ValueError("MotionCompensator.estimate: expected a contiguous {} tensor of shape {} on {}, got {}".format(
                    dtype, shape, self.device, "{} {} on {}".format(t.dtype, tuple(t.shape), t.device) if isinstance(t, Tensor) else type(t)))
        return d

    def estimate(self, batch, boxes: Optional[Tensor] = None, scores: Optional[Tensor] = None, counts: Optional[Tensor] = None, stream=None):
        """One step for every stream: the motion from the stream's previous frame to frame b of the FrameBatch. boxes [B, d, 4] fp32, scores
        [B, d] fp32, counts [B] int32 (that frame's detections: a forward's outputs) mask the blocks that lie on objects; all three or none.
        Every frame's size is validated on the host first (ValueError for a frame too small for one block). Enqueued on `stream` (default: the
        current stream); three launches, no device-to-host copy. Returns (motion [B, 4] fp32 = (s, tx, ty, ok), stats [B, 4] int32 = (blocks,
        valid, inliers, k)): the compensator's own tensors, overwritten by the next step. A stream whose step is not ok (its first frame, a
        changed size, too few textured blocks, no consensus, a scale outside 0.8 .. 1.25) has the identity (1, 0, 0, 0)."""
        d = self._check(batch, boxes, scores, counts)
        p = C.c_void_p
        ptr = lambda t: p(t.data_ptr()) if t is not None else None
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().dn_motion_estimate(p(batch.table.data_ptr()), self.streams, batch.format_code, C.byref(self.params), ptr(boxes),
                                                     ptr(scores), ptr(counts), d, p(self.state.data_ptr()), self.state.numel(),
                                                     p(self.motion.data_ptr()), p(self.stats.data_ptr()), p(self._vectors.data_ptr()),
                                                     self._stream(stream)), "dn_motion_estimate")
        return self.motion, self.stats

    # ------------------------------------------------------------------------------------------------------
    def vectors(self) -> Tensor:
        """A view of the last step's block vectors [B, max_blocks, 4] int32 = (dx, dy, sad, valid); the rows at or beyond stats[:, 0] are 0."""
        return self._vectors

    def _field(self, name):
        off, dtype, shape = self._fields[name]
        n = 1
        for s in shape:
            n *= s
        return self.state[:, off:off + n * torch.empty((), dtype=dtype).element_size()].view(dtype).view((self.streams,) + shape)

    def thumbnails(self):
        """Views (no copies) of the device thumbnails: (both [B, 2, TH, TW] uint8, parity [B] int32). both[b, parity[b]] is the stored thumbnail
        of stream b -- after a step, that step's. Only its floor(H / k) x floor(W / k) corner means anything."""
        return self._field("thumbs")[..., :self.params.max_w], self._field("header")[:, 0]

    def state_dict(self) -> dict:
        """The state bytes (a host copy: this call waits for the device) and the parameters: load_state_dict resumes the run bit for bit."""
        params = {name: getattr(self.params, name) for name, _ in _lib.MotionParams._fields_ if name != "reserved"}
        return {"state": self.state.cpu(), "streams": self.streams, "params": params}

    def load_state_dict(self, sd: dict):
        mine = {name: getattr(self.params, name) for name, _ in _lib.MotionParams._fields_}
        layout = ("max_h", "max_w", "block", "radius")
        if int(sd["streams"]) != self.streams or any(sd["params"][k] != mine[k] for k in layout):
            raise ValueError("MotionCompensator.load_state_dict: the state is for {} streams with {}, this compensator has {} with {}".format(
                sd["streams"], {k: sd["params"][k] for k in layout}, self.streams, {k: mine[k] for k in layout}))
        st = sd["state"]
        if not isinstance(st, Tensor) or st.dtype != torch.uint8 or tuple(st.shape) != tuple(self.state.shape):
            raise ValueError("MotionCompensator.load_state_dict: expected a uint8 state of shape {}".format(tuple(self.state.shape)))
        for name, value in sd["params"].items():
            setattr(self.params, name, value)
        self.state.copy_(st)


def check_motion(motion, tracker, batch, who: str):
    """What the SSD.track_* calls check of their motion= argument before the forward runs."""
    if not isinstance(motion, MotionCompensator):
        raise ValueError("{}: motion must be a MotionCompensator, got {}".format(who, type(motion)))
    if motion.device != tracker.device or motion.streams != tracker.streams:
        raise ValueError("{}: the compensator has {} streams on {}, the tracker {} on {}".format(who, motion.streams, motion.device, tracker.streams,
                                                                                               tracker.device))
    if batch.n != motion.streams:
        raise ValueError("{}: {} frames, the compensator has {} streams".format(who, batch.n, motion.streams))
    check_sizes(batch.sizes, motion.params)


def compensated(motion, tracker, batch, boxes, scores, counts):
    """estimate with the frame's detections, then compensate: what the SSD.track_* calls run between the forward and the update."""
    m, _ = motion.estimate(batch, boxes, scores, counts)
    tracker.compensate(m)
