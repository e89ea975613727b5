"""Host-side mirror of the reference's detector module for the inference path.

`SSD` keeps the reference's contract (demonet/models/generalized_ssd.py:95-349): an nn.Module built by a factory,
`forward(images: List[Tensor[3,H,W]], targets=None) -> List[Dict[boxes, scores, labels]]` in eval mode, a
state_dict with the reference's key names, the same exceptions for malformed input -- but its body is one call
into the HIP library through the C ABI (include/demonet_hip.h). There is no PyTorch/CPU fallback: without the
library or without a GPU the forward raises.
"""
import ctypes as C
import math
from collections import OrderedDict
from typing import Dict, List, Optional

import torch
from torch import nn, Tensor

from . import _lib
from .plan import LoweredModel
from .spec import Graph


# Structure epoch: bumped whenever a module OF THIS PACKAGE (an SSD or one of its name containers) registers a parameter, a buffer or a
# sub-module, i.e. whenever the set of tensor OBJECTS behind a model can have changed (swapped Parameters, load_state_dict(assign=True),
# add_module ...). SSD caches its tensor list per epoch, so the per-forward "did the weights change" test walks a flat list (data_ptr +
# _version of ~480 tensors: tens of microseconds) instead of the module tree (~0.4 ms per call -- a third of a synchronous 64-image
# forward). The hooks live on these two classes only: unrelated modules in the process neither pay for them nor invalidate the cache.
_STRUCT_EPOCH = [0]


class _Tracked(nn.Module):
    def register_parameter(self, name, param):
        _STRUCT_EPOCH[0] += 1
        return super().register_parameter(name, param)

    def register_buffer(self, name, tensor, persistent=True):
        _STRUCT_EPOCH[0] += 1
        return super().register_buffer(name, tensor, persistent)

    def add_module(self, name, module):
        _STRUCT_EPOCH[0] += 1
        return super().add_module(name, module)

    def register_module(self, name, module):
        _STRUCT_EPOCH[0] += 1
        return super().register_module(name, module)

    def __setattr__(self, name, value):
        # nn.Module.__setattr__ stores sub-modules and re-assigned buffers without going through the register_* methods
        if isinstance(value, (Tensor, nn.Module)) or name in self.__dict__.get("_parameters", ()) or name in self.__dict__.get("_buffers", ()) \
                or name in self.__dict__.get("_modules", ()):
            _STRUCT_EPOCH[0] += 1
        return super().__setattr__(name, value)

    def __delattr__(self, name):
        _STRUCT_EPOCH[0] += 1
        return super().__delattr__(name)


class _Node(_Tracked):
    """Container that only exists to reproduce the reference's dotted parameter names."""


def _attach(root: nn.Module, key: str, value: Tensor, buffer: bool):
    parts = key.split(".")
    m = root
    for p in parts[:-1]:
        if p not in m._modules:
            m.add_module(p, _Node())
        m = m._modules[p]
    if buffer:
        m.register_buffer(parts[-1], value)
    else:
        m.register_parameter(parts[-1], nn.Parameter(value, requires_grad=False))


def _require_floating(t: Tensor):
    if not t.is_floating_point():
        raise TypeError(f"Expected input images to be of floating type (in range [0, 1]), but found type {t.dtype} instead")  # transform.py:130-134


def _require_float_batch(images: Tensor):
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError("expected a [N,3,H,W] batch, got {}".format(tuple(images.shape)))
    _require_floating(images)


def forward_args(handle, src_ptr, n, h, w, outs, ws, stream):
    """The ctypes argument tuple of dn_forward / dn_forward_u8 (include/demonet_hip.h); outs: (boxes, scores, labels, counts), stream: a raw hipStream_t."""
    p = C.c_void_p
    return (p(handle), p(src_ptr), n, h, w, *(p(t.data_ptr()) for t in outs), p(ws.data_ptr()), ws.numel(), p(stream))


class SSD(_Tracked):
    def __init__(self, graph: Graph, init: str = "normal"):
        super().__init__()
        self.graph = graph
        gen = torch.Generator().manual_seed(0)
        for p in graph.params:
            if p.kind == "conv_w":
                if init == "xavier":                                   # generalized_ssd.py:17-22
                    fan_in = p.shape[1] * p.shape[2] * p.shape[3]
                    fan_out = p.shape[0] * p.shape[2] * p.shape[3]
                    a = (6.0 / (fan_in + fan_out)) ** 0.5
                    v = (torch.rand(p.shape, generator=gen) * 2 - 1) * a
                else:                                                  # ssd_mobilenetv3.py:57-62 (std 0.03)
                    v = torch.randn(p.shape, generator=gen) * 0.03
                _attach(self, p.key, v, False)
            elif p.kind == "bias":
                _attach(self, p.key, torch.zeros(p.shape), False)
            elif p.kind in ("bn_gamma",):
                _attach(self, p.key, torch.ones(p.shape), False)
            elif p.kind == "bn_beta":
                _attach(self, p.key, torch.zeros(p.shape), False)
            elif p.kind == "bn_mean":
                _attach(self, p.key, torch.zeros(p.shape), True)
            elif p.kind == "bn_var":
                _attach(self, p.key, torch.ones(p.shape), True)
            elif p.kind == "bn_nbt":
                _attach(self, p.key, torch.zeros((), dtype=torch.long), True)
            elif p.kind == "scale20":
                _attach(self, p.key, torch.ones(p.shape) * 20, False)  # ssd_vgg16.py:40
            else:
                raise ValueError(p.kind)
        self.score_thresh = graph.post["score_thresh"]
        self.nms_thresh = graph.post["nms_thresh"]
        self.detections_per_img = graph.post["detections_per_img"]
        self.topk_candidates = graph.post["topk_candidates"]
        self._handle = None
        self._sig = None
        self._lowered = None
        self._bufs = {}
        self._call = None
        self._packed_set = -1         # address the plan's dn_set_packed_output setting holds (-1: unknown): _set_packed
        self._fast_sig = None         # _remember_weights
        self._graph_mode = None       # set_graph_mode; None: never asked, the library's default (DN_GRAPH) holds
        self.nms_method, self.nms_sigma = "hard", 0.5      # set_nms
        self._plan_gen = 0            # counts the plans built (a new plan may reuse the old one's address: pipelines compare this)
        self._pipe_refs, self._pipe_chains = 0, None      # open ForwardPipelines of the current plan, and the `chains` they share
        self._feat_gen = 0            # counts the forwards that wrote this model's workspaces (a head backward checks its features are still there)
        self.eval()

    # ------------------------------------------------------------------------------------------------------
    def _weights_signature(self):
        """What the folded fp16 weight blob of the plan was built from: every tensor's identity, storage address and in-place
        version counter (optimizer steps, load_state_dict, .to(), load_state_dict(assign=True) and swapped Parameters all change
        one of them). Writes that bypass the version counter (`p.data.copy_()`, `p.data.mul_()`) do not: call invalidate()."""
        dev = None
        sig = []
        for t in list(self.parameters()) + list(self.buffers()):
            sig.append((id(t), t.data_ptr(), t._version))
            dev = t.device
        return (hash(tuple(sig)), str(dev), self.score_thresh, self.nms_thresh, self.detections_per_img, self.topk_candidates)

    def _weights_unchanged(self, device, heads_may_differ: bool = False) -> bool:
        """The per-call form of the test above: True when the plan in hand is still what the current weights lower to. Same criteria
        (tensor identities through the structure epoch, storage addresses, in-place version counters, the post-process settings), walked
        over a cached flat list. heads_may_differ: only the backbone part of the list is compared -- the training forward takes the
        features from the plan and computes the heads from the current parameters itself (headgrad.py), so optimizer steps on the heads
        do not rebuild the plan; the remembered state is left as it is, and the next eval forward sees the change and rebuilds once."""
        c = self._fast_sig
        if c is None or c[0] != _STRUCT_EPOCH[0]:
            return False
        _, dev, hyper, tensors, ptrs, vers, n_backbone = c
        if dev != device or hyper != (self.score_thresh, self.nms_thresh, self.detections_per_img, self.topk_candidates):
            return False
        if heads_may_differ:
            tensors, ptrs, vers = tensors[:n_backbone], ptrs[:n_backbone], vers[:n_backbone]
        return [t._version for t in tensors] == vers and [t.data_ptr() for t in tensors] == ptrs

    def _remember_weights(self, device):
        named = list(self.named_parameters()) + list(self.named_buffers())
        tensors = [t for k, t in named if not k.startswith("head.")]      # the backbone part first, then the head's
        n_backbone = len(tensors)
        tensors += [t for k, t in named if k.startswith("head.")]
        self._fast_sig = (_STRUCT_EPOCH[0], device, (self.score_thresh, self.nms_thresh, self.detections_per_img, self.topk_candidates),
                          tensors, [t.data_ptr() for t in tensors], [t._version for t in tensors], n_backbone)

    def invalidate(self):
        """Drop the device plan; the next forward lowers the current parameters again. Needed only after weight edits that bypass
        autograd's version counter (`.data` writes)."""
        self.release()
        self._sig = None
        self._fast_sig = None

    def _load_from_state_dict(self, *args, **kwargs):
        self.invalidate()
        return super()._load_from_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self.invalidate()
        return super()._apply(fn, *args, **kwargs)

    def _plan(self, device, heads_may_differ: bool = False):
        if device.type != "cuda":
            raise RuntimeError("demonet_amd runs on an MI355X only (images must be on a cuda device); "
                               "there is no CPU fallback path")
        if self._handle is not None and self._weights_unchanged(device, heads_may_differ):
            return self._handle
        sig = (self._weights_signature(), str(device))
        if self._handle is not None and sig == self._sig:
            self._remember_weights(device)
            return self._handle
        self.release()
        self.graph.post.update(score_thresh=self.score_thresh, nms_thresh=self.nms_thresh,
                               detections_per_img=self.detections_per_img, topk_candidates=self.topk_candidates)
        sd = {k: v.detach().float().cpu() if v.is_floating_point() else v.detach().cpu() for k, v in self.state_dict().items()}
        with torch.cuda.device(device):
            self._lowered = LoweredModel(self.graph, sd)
            self._handle = self._lowered.create()
        if self.nms_method != "hard":
            self._apply_nms(self.nms_method, self.nms_sigma)
        self._sig = sig
        self._remember_weights(device)
        self._bufs = {}
        self._plan_gen += 1
        self._pipe_refs = 0
        return self._handle

    def release(self):
        if getattr(self, "_handle", None) is not None:
            _lib.lib().dn_destroy(C.c_void_p(self._handle))
            self._handle = None
            self._bufs = {}
            self._call = None
            self._packed_set = -1

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def set_graph_mode(self, enabled: bool):
        self._graph_mode = bool(enabled)
        if self._handle is not None:
            _lib.check(_lib.lib().dn_set_graph_mode(C.c_void_p(self._handle), int(enabled)))

    def set_nms(self, method: str = "hard", sigma: float = 0.5):
        """The per-class reduce of the post-process: "hard" (the reference's NMS, the default), or soft-NMS (Bodla et al., 2017) with
        "linear" (a box overlapping an emitted one by IoU u > nms_thresh keeps 1 - u of its score) or "gaussian" (exp(-u^2 / sigma) of it)
        decay; the scores returned are the decayed ones (include/demonet_hip.h, dn_set_nms). Plan state: every forward of this model
        (forward, forward_batch, forward_uint8, the packed output, a ForwardPipeline) follows it from the next call on, the plan is not
        rebuilt, and a rebuilt plan inherits it. Call it with no forward in flight. Returns self.
        ValueError for an unknown method or a sigma that is not a finite number > 0 -- for every method, stricter than the C ABI, which
        reads sigma in Gaussian mode only: the attribute always holds a value that a later switch to "gaussian" can use. A call that
        fails, here or in the library, leaves the model's setting as it was."""
        if not isinstance(method, str) or method not in _lib.DN_NMS:
            raise ValueError("set_nms: method must be one of {}, got {!r}".format(sorted(_lib.DN_NMS), method))
        try:
            sigma = float(sigma)
        except (TypeError, ValueError):
            raise ValueError("set_nms: sigma must be a number, got {!r}".format(sigma)) from None
        if not (math.isfinite(sigma) and sigma > 0.0):
            raise ValueError("set_nms: sigma must be finite and > 0, got {!r}".format(sigma))
        if self._handle is not None:
            self._apply_nms(method, sigma)      # (raises when the library refuses: the attributes then still describe the plan)
        self.nms_method, self.nms_sigma = method, sigma
        return self

    def _apply_nms(self, method, sigma):
        _lib.check(_lib.lib().dn_set_nms(C.c_void_p(self._handle), _lib.DN_NMS[method], sigma), "dn_set_nms")

    def _buffers_for(self, n, h, w, device):
        key = (n, h, w, str(device))
        b = self._bufs.get(key)
        if b is None:
            L = _lib.lib()
            ws = L.dn_workspace_bytes(C.c_void_p(self._handle), n)
            # the four outputs are typed views of ONE allocation, so that the list API takes its private copy of a call's results
            # with one device copy (forward())
            out = torch.empty(self._out_bytes(n), dtype=torch.uint8, device=device)
            b = dict(
                images=torch.empty((n, 3, h, w), dtype=torch.float32, device=device),
                ws=torch.empty(ws, dtype=torch.uint8, device=device),
                out=out, outs=self._out_views(out, n),       # outs: (boxes, scores, labels, counts)
            )
            if len(self._bufs) >= 4:
                self._bufs.clear()
            self._call = None
            self._bufs[key] = b
            if self._graph_mode is not None:
                _lib.check(L.dn_set_graph_mode(C.c_void_p(self._handle), int(self._graph_mode)))
        return b

    def _out_bytes(self, n):
        D = self.detections_per_img
        return n * D * 16 + n * D * 8 + n * D * 4 + n * 4       # boxes fp32 x 4 | labels int64 | scores fp32 | counts int32 (every offset 8-byte aligned)

    def _out_views(self, out: Tensor, n: int):
        D = self.detections_per_img
        o1, o2, o3 = n * D * 16, n * D * 24, n * D * 28
        return (out[:o1].view(torch.float32).view(n, D, 4), out[o2:o3].view(torch.float32).view(n, D),
                out[o1:o2].view(torch.int64).view(n, D), out[o3:o3 + 4 * n].view(torch.int32))

    # ------------------------------------------------------------------------------------------------------
    def forward_batch(self, images: Tensor, persistent_input: bool = False, packed: Optional[Tensor] = None):
        """images: [N,3,H,W] fp32 on the GPU. Returns padded device tensors (boxes [N,D,4], scores [N,D],
        labels [N,D] int64, counts [N] int32) that stay valid until the next call with the same shape.
        persistent_input=True promises that `images` keeps its address between calls (lets the hipGraph replay).
        packed: optional [N, D+1, 6] fp32 device tensor that additionally receives the gather payload (dist.py)."""
        _require_float_batch(images)
        handle = self._plan(images.device)
        n, _, h, w = images.shape
        self._check_packed(packed, n, images.device)
        b = self._buffers_for(n, h, w, images.device)
        if persistent_input and images.dtype == torch.float32 and images.is_contiguous():
            src = images
        else:
            b["images"].copy_(images)
            src = b["images"]
        dev = images.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        self._set_packed(packed)
        self._feat_gen += 1
        # one C call per forward: the argument tuple of (plan, buffers, input address, stream) is built once and reused while none
        # of them changes -- a synchronous caller pays for every microsecond of Python in front of the graph launch
        key = (handle, b["ws"].data_ptr(), src.data_ptr(), stream)
        call = self._call
        if call is None or call[0] != key:
            call = self._call = (key, _lib.lib().dn_forward, forward_args(handle, src.data_ptr(), n, h, w, b["outs"], b["ws"], stream), b["outs"])
        if torch.cuda.current_device() == dev.index:
            rc = call[1](*call[2])
        else:
            with torch.cuda.device(dev):
                rc = call[1](*call[2])
        if rc < 0:
            _lib.check(rc, "dn_forward")
        return call[3]

    def _check_packed(self, packed, n, device):
        """The merge kernel writes [n][D+1][6] fp32 rows through this pointer: anything else would be an out-of-bounds device write."""
        if packed is None:
            return
        want = (n, self.detections_per_img + 1, 6)
        if tuple(packed.shape) != want or packed.dtype != torch.float32 or not packed.is_contiguous() or packed.device != device:
            raise ValueError("packed must be a contiguous float32 tensor of shape {} on {}, got {} {} on {}".format(
                want, device, tuple(packed.shape), packed.dtype, packed.device))

    def _set_packed(self, packed: Optional[Tensor]):
        """Make `packed` (None: nothing) the extra output of the plan's next forwards: plan-global state of the library, changed only here."""
        pk = packed.data_ptr() if packed is not None else 0
        if self._packed_set != pk:
            _lib.check(_lib.lib().dn_set_packed_output(C.c_void_p(self._handle), C.c_void_p(pk) if pk else None))
            self._packed_set = pk

    def forward_uint8(self, images: Tensor, packed: Optional[Tensor] = None):
        """images: [N,H,W,3] uint8 on the GPU -- a decoder's output (HWC, RGB). ToTensor (/255), the bilinear resize to the network
        size and the HWC -> planar conversion run on the device ahead of the stem (transform.py:27-53,129-138); results equal
        forward_batch(images.permute(0,3,1,2).float() / 255). `images` must keep its address between calls for the graph replay.
        Returns the padded device tensors of forward_batch."""
        if images.dim() != 4 or images.shape[3] != 3 or images.dtype != torch.uint8:
            raise ValueError("expected a [N,H,W,3] uint8 batch, got {} {}".format(tuple(images.shape), images.dtype))
        if not images.is_contiguous():
            raise ValueError("forward_uint8 needs a contiguous [N,H,W,3] tensor")
        handle = self._plan(images.device)
        n, h, w, _ = images.shape
        self._check_packed(packed, n, images.device)
        b = self._buffers_for(n, h, w, images.device)
        stream = torch.cuda.current_stream(images.device).cuda_stream
        self._set_packed(packed)
        self._feat_gen += 1
        with torch.cuda.device(images.device):
            _lib.check(_lib.lib().dn_forward_u8(*forward_args(handle, images.data_ptr(), n, h, w, b["outs"], b["ws"], stream)), "dn_forward_u8")
        return b["outs"]

    def detect_sliced(self, images, tile=None, overlap: float = 0.25, full_image: bool = True, merge_thresh: Optional[float] = None,
                      metric: str = "iou", class_agnostic: bool = False, max_tiles_per_forward: int = 64) -> List[Dict[str, Tensor]]:
        """Sliced inference for images much larger than the network size (demonet_amd/sliced.py): the detector runs on overlapping
        tiles at native resolution -- and, with full_image, on the whole image as well, which keeps the objects larger than a tile -- and the
        per-tile detections, shifted into image coordinates, are merged by one more hard NMS on the device (include/demonet_hip.h,
        dn_merge_detections: IoU or "ios" = intersection over the smaller box, threshold merge_thresh, per class or class_agnostic).
        images: one [3, H, W] float tensor in [0, 1] on the GPU or a list of them (sizes may differ). tile: an int or (th, tw); default: the
        network size, so tiles are not resized at all (tile_grid: stride tile - round(overlap * tile), the last tile of a row / column clamped
        into the image). merge_thresh defaults to nms_thresh. The tiles of an image go through forward_batch in sub-batches of at most
        max_tiles_per_forward; the NMS mode of set_nms applies inside each tile. Eval mode only.
        Returns one {"boxes", "scores", "labels"} per image like forward, in image coordinates, at most detections_per_img each.
        ValueError for bad arguments and for an image with more tiles than the merge takes (1 024 sources, 65 536 sources x detections_per_img)."""
        from .sliced import detect_sliced
        return detect_sliced(self, images, tile, overlap, full_image, merge_thresh, metric, class_agnostic, max_tiles_per_forward)

    def detect_tta(self, images, hflip: bool = True, fuse: str = "wbf", thresh: Optional[float] = None,
                   skip_thresh: Optional[float] = None) -> List[Dict[str, Tensor]]:
        """Horizontal-flip test-time augmentation (demonet_amd/fusion.py): every image is detected twice, as it is and mirrored
        (torch.flip along the width; the mirrored pass's boxes are mapped back by x1' = W - x2, x2' = W - x1), both passes in one forward_batch,
        and the two sets of detections are reduced per image on the device. fuse="wbf": weighted boxes fusion (include/demonet_hip.h,
        dn_fuse_detections): boxes of one label with IoU > thresh are averaged with their scores as weights, and a detection that only one of the
        passes made keeps half its score; detections below skip_thresh do not take part. fuse="nms": one more hard NMS per class instead
        (dn_merge_detections). images: an [N, 3, H, W] float tensor in [0, 1] on the GPU or a list of [3, H, W] tensors (sizes may differ: one
        pass pair per distinct size). thresh defaults to nms_thresh, skip_thresh to score_thresh. Eval mode only.
        Returns one {"boxes", "scores", "labels"} per image like forward, in the input order, at most detections_per_img each; one device-to-host
        copy (the counts). ValueError for bad arguments and for hflip=False with fuse="wbf": a single source has nothing to fuse."""
        from .fusion import detect_tta
        return detect_tta(self, images, hflip, fuse, thresh, skip_thresh)

    def track(self, images: Tensor, tracker, analytics=None):
        """Detect and track one frame of every stream (demonet_amd/track.py): forward_batch on images [B, 3, H, W], image b being the
        current frame of stream b, then tracker.update (a ByteTracker with B streams on the same device) on the detections where they lie: one
        more launch behind the forward, no device-to-host copy. Returns what ByteTracker.update returns: padded device tensors (boxes [B, T, 4],
        scores, labels, ids, det [B, T], counts [B], det_ids [B, D]) of the confirmed tracks seen in this frame. Eval mode only.
        analytics: None, or a zones.ZoneAnalytics bound to this tracker: its step -- line crossings, zone entries, exits and dwell,
        accumulated on the device -- follows the tracker's on the same stream, and the return value gains the pair (events [B, max_events, 8],
        event_counts [B]) as its last element. With None the call, its launches and its results are exactly those without the argument."""
        from .track import track
        return track(self, images, tracker, analytics)

    def forward_frames(self, batch, packed: Optional[Tensor] = None):
        """The forward on video surfaces (demonet_amd/frames.py): batch is a FrameBatch naming n NV12 / I420 / RGB24 / BGR24 frames, each
        its own allocation with its own pitches and its own SIZE. The colour conversion (integer arithmetic fixed in include/demonet_hip.h,
        dn_forward_frames), /255, the bilinear resize and the planar layout run as one pass ahead of the stem, reading four taps per network
        pixel; no converted frame and no float staging image exist. Results equal forward_uint8 of the frames converted by those formulas, bit
        for bit; boxes are in each frame's own pixel coordinates. The graph replays on whatever frames batch.set() named last.
        Returns the padded device tensors of forward_batch. ValueError for a batch without frames or on another device than the model."""
        from .frames import forward_frames
        return forward_frames(self, batch, packed)

    def track_frames(self, batch, tracker, analytics=None, motion=None, osd=None, compose=None, wall=None, warp=None, source=None, jpeg=None):
        """`track` on top of forward_frames: frame b of the FrameBatch is the current frame of stream b. Returns what ByteTracker.update returns;
        analytics as in `track`. motion: a motion.MotionCompensator for a moving camera: forward -> motion.estimate(batch, that
        frame's detections) -> tracker.compensate -> update; None (the default): exactly the calls above. osd: an osd.Overlay: the
        tracker's outputs -- and the analytics' lines and zones -- are painted INTO THE FRAMES as the step's last act, after the motion estimate
        (and the crops) have read them; the return value does not change. THE PAINT MUST COME LAST: whatever reads the frames after it sees
        painted pixels. None (the default): exactly the calls above. compose, wall: a compose.Compositor that was set() for (batch, wall) and its
        destination FrameBatch: behind the paint -- the paint must precede the copy -- the frames are composed into the wall's
        surfaces, compose(batch, wall); both or neither; None (the default): exactly the calls above. warp, source: a warp.Warper that was set()
        for (source, batch) and its source FrameBatch: as the step's FIRST act, in front of the forward, the batch's frames are filled
        from the source's surfaces -- views of a fisheye, an undistorted or a turned camera --, warp(source, batch); both or neither; None (the
        default): exactly the calls above. jpeg: a jpeg.JpegEncoder that was set() for the wall when the step has one, for the batch
        otherwise: behind the paint and the composition its items are coded into its arena, jpeg.encode(wall or batch); None (the default):
        exactly the calls above."""
        from .frames import track_frames
        return track_frames(self, batch, tracker, analytics, motion, osd, compose, wall, warp, source, jpeg)

    def track_frames_appearance(self, batch, tracker, cropper, embedder, analytics=None, motion=None, osd=None, compose=None, wall=None, warp=None,
                                source=None, jpeg=None):
        """`track_frames` with appearance, nothing leaving the device: forward_frames; cropper(batch, boxes, counts, select) with
        select = scores >= the tracker's track_thresh, built on the device; embedder(patches), any callable that returns a [capacity, dim] fp16
        or fp32 device tensor (the re-identification model: not part of this package); tracker.update(..., embeddings, cropper.index) for a
        track.AppearanceTracker; then the analytics as in `track`. Returns what ByteTracker.update returns. motion: as in `track_frames`
        (estimate and compensate run behind the forward, in front of the crops). osd: as in `track_frames` (the paint follows the crops). compose, wall:
        as in `track_frames` (the composition follows the paint). warp, source: as in `track_frames` (the warp precedes the forward). jpeg: as in
        `track_frames` (the encoder runs last)."""
        from .frames import track_frames_appearance
        return track_frames_appearance(self, batch, tracker, cropper, embedder, analytics, motion, osd, compose, wall, warp, source, jpeg)

    def forward_regions(self, batch, table, packed: Optional[Tensor] = None):
        """The forward on REGIONS of video surfaces (demonet_amd/frames.py): table is a frames.RegionTable of n (frame, x0, y0, w, h[,
        hflip]) rectangles of the FrameBatch's frames; network image i is rectangle i, mirrored left-right when flagged, resized to the network
        size by forward_frames' pass in region coordinates (include/demonet_hip.h, dn_forward_regions): bit for bit what forward_uint8 computes
        from the rectangle cut out of the converted frame. Boxes are in each region's own coordinates (a mirrored region's are the mirrored ones).
        Returns the padded device tensors of forward_batch. ValueError for an unset batch or table, another device, and STALE SIZES: a frame
        the regions name whose size in the batch is no longer the one the regions were validated against (set() the table again)."""
        from .frames import forward_regions
        return forward_regions(self, batch, table, packed)

    def detect_sliced_frames(self, batch, tile=None, overlap: float = 0.25, full_image: bool = True, merge_thresh: Optional[float] = None,
                             metric: str = "iou", class_agnostic: bool = False, max_tiles_per_forward: int = 64) -> List[Dict[str, Tensor]]:
        """detect_sliced on the frames of a FrameBatch, with the same arguments and the same results: the tiles and the whole-frame passes are
        regions of the surfaces (sliced.FrameSlicer) -- no converted frame, no float image, and the regions of ALL frames share
        forwards of at most max_tiles_per_forward images. One device-to-host copy, the merged counts. The slicer is cached on (batch.sizes,
        arguments). Returns one {"boxes", "scores", "labels"} per frame, in frame coordinates."""
        from .sliced import detect_sliced_frames
        return detect_sliced_frames(self, batch, tile, overlap, full_image, merge_thresh, metric, class_agnostic, max_tiles_per_forward)

    def detect_tta_frames(self, batch, fuse: str = "wbf", thresh: Optional[float] = None, skip_thresh: Optional[float] = None) -> List[Dict[str, Tensor]]:
        """detect_tta (hflip=True) on the frames of a FrameBatch: every frame is one plain and one mirrored whole-frame region, all of them in one
        forward, mapped back and fused or merged as detect_tta does. Returns one {"boxes", "scores", "labels"} per frame."""
        from .fusion import detect_tta_frames
        return detect_tta_frames(self, batch, fuse, thresh, skip_thresh)

    def track_sliced_frames(self, batch, tracker, slicer, analytics=None, motion=None, osd=None, compose=None, wall=None, warp=None, source=None,
                            jpeg=None):
        """Video -> tiles -> merge -> ByteTrack without a host wait per frame step: tracker.update(*slicer(batch)) for a sliced.FrameSlicer of
        this model (frame g of the batch is the current frame of stream g). Returns what ByteTracker.update returns; analytics as in `track`.
        ValueError when detections_per_img exceeds the tracker's 512 rows. motion: as in `track_frames`, with the merged detections. osd, compose and
        wall: as in `track_frames`; warp and source too (the warp precedes the tiles); jpeg too (the encoder runs last)."""
        from .sliced import track_sliced_frames
        return track_sliced_frames(self, batch, tracker, slicer, analytics, motion, osd, compose, wall, warp, source, jpeg)

    def paint_frames(self, batch, overlay, boxes, scores, labels, counts, ids=None, zones=None):
        """On-screen display (demonet_amd/osd.py): overlay.paint(batch, boxes, scores, labels, counts, ids, zones) for an osd.Overlay on
        this model's device -- boxes, labels, lines, zones and redaction painted in place into the frames, in their own colour space, without a
        device-to-host copy. Returns the overlay's stats [B, 4] int32. Paint last: later readers of the frames see the painted pixels."""
        from .osd import paint_frames
        return paint_frames(self, batch, overlay, boxes, scores, labels, counts, ids, zones)

    def crop_objects(self, batch, cropper, boxes, counts, select=None):
        """The objects of the frames as fixed-size normalised patches for a second model, on the device (demonet_amd/crops.py):
        cropper(batch, boxes, counts, select) for a crops.ObjectCropper on this model's device. boxes and counts are a tracking step's or a
        forward's, in frame pixels:
            boxes, scores, labels, ids, det, counts, det_ids = model.track_sliced_frames(batch, tracker, slicer)
            patches, index, totals = model.crop_objects(batch, cropper, boxes, counts)
        Returns what the cropper returns; no device-to-host copy."""
        from .crops import crop_objects
        return crop_objects(self, batch, cropper, boxes, counts, select)

    def batch_split(self, n: int) -> int:
        """Number of parallel sub-batch launch chains a forward of n images is issued as (1 = a single chain)."""
        if self._handle is None:
            raise RuntimeError("batch_split: the plan is built on the first forward / .cuda()")
        return _lib.check(_lib.lib().dn_batch_split(C.c_void_p(self._handle), int(n)))

    def forward_heads(self, images: Tensor):
        """Backbone + heads only: returns (cls_logits [N,A,K], bbox_regression [N,A,4]) fp32 device tensors (copies)."""
        _require_float_batch(images)
        handle = self._plan(images.device)
        n, _, h, w = images.shape
        b = self._buffers_for(n, h, w, images.device)
        b["images"].copy_(images)
        L = _lib.lib()
        stream = torch.cuda.current_stream(images.device).cuda_stream
        self._feat_gen += 1
        with torch.cuda.device(images.device):
            _lib.check(L.dn_forward_heads(C.c_void_p(handle), C.c_void_p(b["images"].data_ptr()), n, h, w,
                                          C.c_void_p(b["ws"].data_ptr()), b["ws"].numel(), C.c_void_p(stream)), "dn_forward_heads")
        pl, pr = C.c_void_p(), C.c_void_p()
        _lib.check(L.dn_head_outputs(C.c_void_p(handle), C.c_void_p(b["ws"].data_ptr()), n, C.byref(pl), C.byref(pr)))
        A, K = self.graph.num_anchors(), self.graph.num_classes
        base = b["ws"].data_ptr()
        lo = (pl.value - base)
        ro = (pr.value - base)
        logits = b["ws"][lo:lo + n * A * K * 4].view(torch.float32).view(n, A, K).clone()
        reg = b["ws"][ro:ro + n * A * 16].view(torch.float32).view(n, A, 4).clone()
        return logits, reg

    def tensor(self, images_shape, tensor_id: int) -> Tensor:
        """NHWC fp16 view (copy) of an intermediate activation of the LAST forward with this batch shape."""
        n, _, h, w = images_shape
        key = next(k for k in self._bufs if k[:3] == (n, h, w))
        b = self._bufs[key]
        p, sz = C.c_void_p(), C.c_size_t()
        _lib.check(_lib.lib().dn_tensor_ptr(C.c_void_p(self._handle), C.c_void_p(b["ws"].data_ptr()), n, tensor_id,
                                            C.byref(p), C.byref(sz)))
        t = self.graph.t(tensor_id)
        off = p.value - b["ws"].data_ptr()
        return b["ws"][off:off + sz.value].view(torch.float16).view(n, t.h, t.w, t.c).clone()

    def compute_loss(self, targets: List[Dict[str, Tensor]], head_outputs: Dict[str, Tensor], anchors=None, matched_idxs=None,
                     iou_thresh: float = 0.5, positive_fraction: float = 0.25) -> Dict[str, Tensor]:
        """The training loss (generalized_ssd.py:210-269 on the matching of :316-330), computed on the GPU by dn_ssd_loss
        (demonet_amd/loss.py). When head_outputs['cls_logits'] or ['bbox_regression'] requires grad, the returned losses are
        differentiable with respect to them (dn_ssd_loss_train / dn_ssd_loss_backward), so any PyTorch head can be trained against
        this loss -- and this model's own SSDLite heads through SSD.loss, which continues the gradient to their parameters
        (headgrad.py); the backward through the fp16 backbone stays out of scope. `anchors` defaults to the model's own
        default boxes; `matched_idxs`, which the reference's forward computes and passes in, is recomputed here and, when given,
        checked against."""
        from .loss import ssd_loss
        dev = head_outputs["cls_logits"].device
        if anchors is None:
            self._plan(dev, heads_may_differ=True)      # (the default boxes do not depend on the weights: no rebuild between optimizer steps on the heads)
            anchors = torch.from_numpy(self._lowered.anchors).to(dev)
        losses, matched = ssd_loss(head_outputs, anchors, targets, iou_thresh, (1.0 - positive_fraction) / positive_fraction)
        if matched_idxs is not None:
            given = torch.stack(list(matched_idxs)).to(matched.device)
            if not torch.equal(given, matched):
                raise ValueError("compute_loss: matched_idxs differ from the SSDMatcher result for these targets and anchors")
        return losses

    def head_parameters(self) -> "OrderedDict[str, nn.Parameter]":
        """The parameters of the SSDLite heads (conv weights and biases, BN weight and bias) by the reference's names -- what
        train_heads() switches and SSD.loss(...).backward() fills. NotImplementedError for the dense 3x3 heads of the VGG models."""
        from .headgrad import parameter_names
        named = dict(self.named_parameters())
        return OrderedDict((k, named[k]) for k in parameter_names(self.graph))

    def train_heads(self, mode: bool = True):
        """requires_grad of every head parameter (and of nothing else): fine-tuning the heads on the frozen backbone. Default: False
        for every parameter of the model."""
        for p in self.head_parameters().values():
            p.requires_grad_(bool(mode))
        return self

    def _heads_trainable(self) -> bool:
        if not any(p.requires_grad for k, p in self.named_parameters() if k.startswith("head.")):
            return False
        return any(p.requires_grad for p in self.head_parameters().values())

    def loss(self, images: Tensor, targets: List[Dict[str, Tensor]]) -> Dict[str, Tensor]:
        """Backbone + heads (forward_heads) -> compute_loss: the loss values a reference model in train mode would return for this
        batch with the same (eval-mode, BN folded) weights. images: [N,3,H,W] AT THE NETWORK SIZE: the reference's transform also resizes
        the target boxes with the images (transform.py:93-108), which this entry point does not do -- other sizes raise.
        When grad mode is on and a head parameter requires grad (train_heads), the returned losses are differentiable with respect to
        the head parameters: backward() fills .grad of every head parameter that requires it and of nothing else (headgrad.py: features
        from the plan, the heads from the current fp32 parameters, head BN on its running statistics). Otherwise the call is the plain
        one: the same launches, the same bits."""
        W, H = self.graph.size
        if tuple(images.shape[-2:]) != (H, W):
            raise ValueError("SSD.loss: images of {}x{} but the network size is {}x{}; resize the images AND the target boxes first "
                             "(the reference's transform does both, transform.py:93-108)".format(images.shape[-2], images.shape[-1], H, W))
        if torch.is_grad_enabled() and self._heads_trainable():
            from .headgrad import head_outputs
            _require_float_batch(images)
            return self.compute_loss(targets, head_outputs(self, images))
        logits, reg = self.forward_heads(images)
        return self.compute_loss(targets, {"cls_logits": logits, "bbox_regression": reg})

    def train_preset(self, data_augmentation: str = "ssd", **kw):
        """The reference's DetectionPresetTrain (presets.py:4-23) bound to this model's network size, on the device (demonet_amd/augment.py,
        DESIGN 4l): preset(images, targets, generator=None) takes a list of decoded [h, w, 3] uint8 device tensors of any sizes with their
        targets and returns (batch, targets) as SSD.loss takes them -- model.loss(*model.train_preset()(images, targets)) is the whole input
        side of a fine-tuning step. kw: hflip_prob, mean and the other constructor arguments of augment.AugmentSampler."""
        from .augment import DetectionPresetTrain
        W, H = self.graph.size
        return DetectionPresetTrain(data_augmentation, size=(H, W), **kw)

    def forward(self, images, targets: Optional[List[Dict[str, Tensor]]] = None):
        if self.training:
            if targets is None:
                raise ValueError("In training mode, targets should be passed")     # generalized_ssd.py:273-274
            if self._heads_trainable():                                             # generalized_ssd.py:271-349, training branch
                if not isinstance(images, Tensor):
                    images = torch.stack(list(images))
                return self.loss(images, targets)
            raise NotImplementedError("demonet_amd trains the SSDLite heads on the frozen backbone only, and no head parameter of this model requires "
                                      "grad: call train_heads() first (VGG models: not covered). The loss VALUE of a batch is available through "
                                      "SSD.loss(images, targets) / compute_loss (differentiable w.r.t. the head outputs it is given)")
        legacy = isinstance(images, Tensor) and images.dim() == 4                   # hub call form model(x[1,3,S,S], shapes)
        if legacy:
            images = list(images.unbind(0))
        groups: Dict = {}                                                           # shape -> indices, in order of first appearance
        for i, img in enumerate(images):
            if img.dim() != 3:
                raise ValueError("images is expected to be a list of 3d tensors "
                                 "of shape [C, H, W], got {}".format(img.shape))    # transform.py:110-112
            _require_floating(img)
            g = groups.get(img.shape)
            if g is None:
                groups[img.shape] = [i]
            else:
                g.append(i)
        out: List[Optional[Dict[str, Tensor]]] = [None] * len(images)
        f32 = torch.float32
        for shape, idxs in groups.items():
            device = images[idxs[0]].device
            self._plan(device)
            b = self._buffers_for(len(idxs), shape[1], shape[2], device)
            torch.stack([images[i] if images[i].dtype is f32 else images[i].to(f32) for i in idxs], out=b["images"])
            self.forward_batch(b["images"], persistent_input=True)
            # The padded outputs live in buffers that the next call overwrites: ONE private copy per call (a single device copy of the
            # allocation that holds all four), and the per-image results are views into it. They therefore SHARE storage: keeping one
            # image's result alive keeps the whole batch copy (n x D x 28 bytes) alive, and an in-place edit of a full-length result
            # edits that copy -- the reference returns independent tensors per image; clone() a result to detach it.
            boxes, scores, labels, counts = self._out_views(b["out"].clone(), len(idxs))
            # The full-length views are made BEFORE the host waits for the counts: 192 tensor objects cost ~0.13 ms of host time, which
            # this way runs under the forward on the device instead of behind it. Only images with fewer than D detections need a slice
            # afterwards (2 us each).
            D = boxes.shape[1]
            ub, us, ul = boxes.unbind(0), scores.unbind(0), labels.unbind(0)
            cnt = counts.tolist()                                                   # the one device->host sync
            for j, i in enumerate(idxs):
                c = cnt[j]
                d = {"boxes": ub[j], "scores": us[j], "labels": ul[j]} if c == D else {"boxes": ub[j][:c], "scores": us[j][:c], "labels": ul[j][:c]}
                if legacy:
                    d = OrderedDict((k, d[k]) for k in ("scores", "labels", "boxes"))   # box_head.py:379 order
                out[i] = d
        return out
