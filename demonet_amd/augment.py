"""SSD training augmentation on the device: the reference's DetectionPresetTrain (data/presets.py, data/transforms.py) and the resize of
its model transform (transform.py:27-53, 150-173, 278-292) as ONE call per batch, from decoded uint8 images to the input of SSD.loss.

    preset = model.train_preset()                       # DetectionPresetTrain('ssd', size = the network size)
    losses = model.loss(*preset(images, targets))       # images: a list of [h, w, 3] uint8 device tensors of any sizes

Two halves:
  * AugmentSampler.sample -- host, pure torch on the CPU: draws one parameter record (Params) per image from the reference's distributions and
    transforms the boxes, which depend on the parameters only, with the reference's own float32 statements.
  * augment_batch -- the launch (dn_augment_batch, csrc/augment.hip): applies the records to the pixels. Photometric distortion, zoom-out canvas,
    crop, flip, ToTensor and the bilinear resize collapse into one gather-and-blend launch behind two small reduction launches (the contrast means).

What is computed per image is stated in include/demonet_hip.h (dn_augment_batch) and restated in float64 by tests/augment_ref.py.

The sampler's draw order is its own (torchvision's RNG stream differs between versions and is not matched). Per image, policy 'ssd':
  1. torch.rand(7): the gates r[0..6] of RandomPhotometricDistort.forward (brightness, contrast_before = r[1] < 0.5, contrast if before,
     saturation, hue, contrast if after, channel permutation), each step on when its r < p;
  2. torch.rand(4): the factors lo + (hi - lo) u of brightness, contrast, saturation, hue (always drawn; float32 arithmetic);
  3. torch.randperm(3) (always drawn; used when r[6] < p);
  4. torch.rand(4): zoom-out: u[0] < p keeps the image as it is (transforms.py:157-158); else ratio = lo + u[1] (hi - lo),
     canvas = int(size * ratio), left = int((Wc - w) u[2]), top = int((Hc - h) u[3]) (transforms.py:162-168, float32 tensors, int() truncation);
  5. the RandomIoUCrop loop (transforms.py:81-129) unless the image has no boxes: torch.randint over the options; an option >= 1 leaves the canvas
     as it is; else up to `trials` times torch.rand(2) for the scales and, when the aspect ratio passes, torch.rand(2) for the position; a trial is
     rejected when left == right or top == bottom, no box centre lies strictly inside, or the largest IoU is below the option; after `trials`
     rejections the option is drawn again;
  6. torch.rand(1): the flip, on when below hflip_prob.
Policy 'hflip' draws step 6 only. An image without boxes takes the as-is crop and draws nothing in step 5 (the reference leaves its loop for such an
image only through the as-is option).
"""
import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib

# record layout of include/demonet_hip.h (DN_AUG_*)
WORDS = 20
FLAGS, BRIGHTNESS, CONTRAST, SATURATION, HUE, PERM, CANVAS_H, CANVAS_W, LEFT, TOP, FILL, CROP_L, CROP_T, CROP_W, CROP_H = 0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 15, 16, 17, 18
F_BRIGHTNESS, F_CONTRAST, F_SATURATION, F_HUE, F_CONTRAST_BEFORE, F_FLIP, F_ALL = 1, 2, 4, 8, 16, 32, 63


def _f32(v) -> float:
    return float(np.float32(v))


@dataclass
class Params:
    """One image's parameter record. A photometric factor of None = that step is off; the others are stored rounded to float32, as the device reads
    them. `option` is the sampler's IoU-crop option (>= 1: the as-is crop, whose boxes are neither filtered nor clamped); it does not reach the device, but the boxes depend on it: a hand-made record
    with a real crop sets option < 1 (tests/augment_ref.boxes_ref refuses one that does not)."""
    canvas_h: int
    canvas_w: int
    left: int = 0
    top: int = 0
    crop_l: int = 0
    crop_t: int = 0
    crop_w: int = 0
    crop_h: int = 0
    flip: bool = False
    brightness: Optional[float] = None
    contrast: Optional[float] = None
    saturation: Optional[float] = None
    hue: Optional[float] = None
    contrast_before: bool = False
    perm: Tuple[int, int, int] = (0, 1, 2)
    fill: Tuple[float, float, float] = (_f32(123.0 / 255.0), _f32(117.0 / 255.0), _f32(104.0 / 255.0))
    option: float = 1.0

    def __post_init__(self):
        for k in ("brightness", "contrast", "saturation", "hue"):
            v = getattr(self, k)
            if v is not None:
                setattr(self, k, _f32(v))
        self.fill = tuple(_f32(v) for v in self.fill)
        self.perm = tuple(int(v) for v in self.perm)

    @classmethod
    def identity(cls, h: int, w: int, **kw) -> "Params":
        """The record that changes nothing: canvas = image, crop = canvas."""
        kw.setdefault("crop_w", kw.get("canvas_w", w))
        kw.setdefault("crop_h", kw.get("canvas_h", h))
        kw.setdefault("canvas_h", h)
        kw.setdefault("canvas_w", w)
        return cls(**kw)

    def flags(self) -> int:
        return ((F_BRIGHTNESS if self.brightness is not None else 0) | (F_CONTRAST if self.contrast is not None else 0)
                | (F_SATURATION if self.saturation is not None else 0) | (F_HUE if self.hue is not None else 0)
                | (F_CONTRAST_BEFORE if self.contrast_before else 0) | (F_FLIP if self.flip else 0))


def pack(params: Sequence[Params]) -> np.ndarray:
    """[n][WORDS] int32: the records as dn_augment_batch reads them (float words hold the fp32 bits)"""
    rec = np.zeros((len(params), WORDS), dtype=np.int32)
    fl = rec.view(np.float32)
    for i, p in enumerate(params):
        rec[i, FLAGS] = p.flags()
        fl[i, BRIGHTNESS] = 1.0 if p.brightness is None else p.brightness
        fl[i, CONTRAST] = 1.0 if p.contrast is None else p.contrast
        fl[i, SATURATION] = 1.0 if p.saturation is None else p.saturation
        fl[i, HUE] = 0.0 if p.hue is None else p.hue
        rec[i, PERM:PERM + 3] = p.perm
        rec[i, CANVAS_H], rec[i, CANVAS_W], rec[i, LEFT], rec[i, TOP] = p.canvas_h, p.canvas_w, p.left, p.top
        fl[i, FILL:FILL + 3] = p.fill
        rec[i, CROP_L], rec[i, CROP_T], rec[i, CROP_W], rec[i, CROP_H] = p.crop_l, p.crop_t, p.crop_w, p.crop_h
    return rec


def _box_iou(boxes: Tensor, crop: Tensor) -> Tensor:
    """torchvision.ops.boxes.box_iou of [G, 4] against one box [1, 4], float32"""
    area1 = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    area2 = (crop[:, 2] - crop[:, 0]) * (crop[:, 3] - crop[:, 1])
    lt = torch.max(boxes[:, None, :2], crop[:, :2])
    rb = torch.min(boxes[:, None, 2:], crop[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (area1[:, None] + area2 - inter)


class AugmentSampler:
    """The random half of DetectionPresetTrain: one Params per image and the transformed targets. Every default is the reference's
    (transforms.py:55-66 RandomIoUCrop, :133-141 RandomZoomOut, :191-198 RandomPhotometricDistort, presets.py:5)."""

    def __init__(self, data_augmentation: str = "ssd", hflip_prob: float = 0.5, mean=(123.0, 117.0, 104.0), size: Tuple[int, int] = (320, 320),
                 p: float = 0.5, brightness=(0.875, 1.125), contrast=(0.5, 1.5), saturation=(0.5, 1.5), hue=(-0.05, 0.05),
                 side_range=(1.0, 4.0), zoom_p: float = 0.5, min_scale: float = 0.3, max_scale: float = 1.0, min_aspect_ratio: float = 0.5,
                 max_aspect_ratio: float = 2.0, sampler_options: Optional[Sequence[float]] = None, trials: int = 40):
        if data_augmentation not in ("hflip", "ssd"):
            raise ValueError(f'Unknown data augmentation policy "{data_augmentation}"')         # presets.py:20
        if side_range[0] < 1.0 or side_range[0] > side_range[1]:
            raise ValueError("Invalid canvas side range provided {}.".format(side_range))           # transforms.py:139-140
        self.policy = data_augmentation
        self.hflip_prob = hflip_prob
        self.fill = tuple(float(m) / 255.0 for m in mean)       # ToTensor comes last in the reference: its uint8 fill, in [0, 1] units
        self.size = (int(size[0]), int(size[1]))                # (S_h, S_w)
        self.p = p
        self.ranges = (tuple(brightness), tuple(contrast), tuple(saturation), tuple(hue))
        self.side_range = tuple(side_range)
        self.zoom_p = zoom_p
        self.min_scale, self.max_scale = min_scale, max_scale
        self.min_aspect_ratio, self.max_aspect_ratio = min_aspect_ratio, max_aspect_ratio
        self.options = list(sampler_options) if sampler_options is not None else [0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0]
        self.trials = trials

    def _iou_crop(self, par: Params, boxes: Tensor, g):
        """transforms.py:81-129 on the canvas; returns the mask of the boxes kept (None: as is)"""
        orig_w, orig_h = par.canvas_w, par.canvas_h
        while True:
            idx = int(torch.randint(low=0, high=len(self.options), size=(1,), generator=g))
            par.option = float(self.options[idx])
            if par.option >= 1.0:
                return None
            for _ in range(self.trials):
                r = self.min_scale + (self.max_scale - self.min_scale) * torch.rand(2, generator=g)
                new_w = int(orig_w * r[0])
                new_h = int(orig_h * r[1])
                if new_h == 0:          # (the reference divides by it: ZeroDivisionError; a zero-area crop is rejected below anyway)
                    continue
                aspect_ratio = new_w / new_h
                if not (self.min_aspect_ratio <= aspect_ratio <= self.max_aspect_ratio):
                    continue
                r = torch.rand(2, generator=g)
                left = int((orig_w - new_w) * r[0])
                top = int((orig_h - new_h) * r[1])
                right = left + new_w
                bottom = top + new_h
                if left == right or top == bottom:
                    continue
                cx = 0.5 * (boxes[:, 0] + boxes[:, 2])
                cy = 0.5 * (boxes[:, 1] + boxes[:, 3])
                within = (left < cx) & (cx < right) & (top < cy) & (cy < bottom)
                if not within.any():
                    continue
                ious = _box_iou(boxes[within], torch.tensor([[left, top, right, bottom]], dtype=boxes.dtype))
                if ious.max() < par.option:
                    continue
                par.crop_l, par.crop_t, par.crop_w, par.crop_h = left, top, new_w, new_h
                return within

    def sample(self, sizes: Sequence[Tuple[int, int]], targets: Sequence[Dict[str, Tensor]], generator: Optional[torch.Generator] = None):
        """sizes: (h, w) per image; targets: {"boxes" [G, 4] float32 xyxy pixels, "labels" [G] int64} per image (CPU tensors; not modified).
        Returns (list of Params, list of {"boxes", "labels"} CPU tensors in the coordinates of the size[0] x size[1] output)."""
        if len(sizes) != len(targets):
            raise ValueError("sample: {} sizes but {} targets".format(len(sizes), len(targets)))
        g = generator
        out_p, out_t = [], []
        for (h, w), tgt in zip(sizes, targets):
            h, w = int(h), int(w)
            boxes = tgt["boxes"].detach().to("cpu", torch.float32).reshape(-1, 4).clone()
            labels = tgt["labels"].detach().to("cpu").clone()
            par = Params.identity(h, w, fill=self.fill)
            if self.policy == "ssd":
                r = torch.rand(7, generator=g)
                u = torch.rand(4, generator=g)
                fac = [float(lo + (hi - lo) * u[k]) for k, (lo, hi) in enumerate(self.ranges)]
                perm = torch.randperm(3, generator=g)
                par.contrast_before = bool(r[1] < 0.5)
                if r[0] < self.p:
                    par.brightness = _f32(fac[0])
                if (r[2] if par.contrast_before else r[5]) < self.p:
                    par.contrast = _f32(fac[1])
                if r[3] < self.p:
                    par.saturation = _f32(fac[2])
                if r[4] < self.p:
                    par.hue = _f32(fac[3])
                if r[6] < self.p:
                    par.perm = tuple(int(v) for v in perm)
                z = torch.rand(4, generator=g)
                if not (z[0] < self.zoom_p):
                    ratio = self.side_range[0] + z[1:2] * (self.side_range[1] - self.side_range[0])
                    par.canvas_w = int(w * ratio)
                    par.canvas_h = int(h * ratio)
                    par.left = int((par.canvas_w - w) * z[2])
                    par.top = int((par.canvas_h - h) * z[3])
                    boxes[:, 0::2] += par.left                                                     # transforms.py:184-185
                    boxes[:, 1::2] += par.top
                par.crop_w, par.crop_h = par.canvas_w, par.canvas_h
                within = self._iou_crop(par, boxes, g) if boxes.shape[0] > 0 else None
                if within is not None:                                                             # transforms.py:121-126
                    boxes = boxes[within]
                    labels = labels[within]
                    boxes[:, 0::2] -= par.crop_l
                    boxes[:, 1::2] -= par.crop_t
                    boxes[:, 0::2].clamp_(min=0, max=par.crop_w)
                    boxes[:, 1::2].clamp_(min=0, max=par.crop_h)
            if torch.rand(1, generator=g) < self.hflip_prob:
                par.flip = True
                boxes[:, [0, 2]] = par.crop_w - boxes[:, [2, 0]]                                   # transforms.py:37
            # transform.py:278-292 (resize_boxes), the ratios as float32 tensors
            ratio_h = torch.tensor(self.size[0], dtype=torch.float32) / torch.tensor(par.crop_h, dtype=torch.float32)
            ratio_w = torch.tensor(self.size[1], dtype=torch.float32) / torch.tensor(par.crop_w, dtype=torch.float32)
            xmin, ymin, xmax, ymax = boxes.unbind(1)
            boxes = torch.stack((xmin * ratio_w, ymin * ratio_h, xmax * ratio_w, ymax * ratio_h), dim=1)
            out_p.append(par)
            out_t.append({"boxes": boxes, "labels": labels})
        return out_p, out_t


def _check_images(images, what: str):
    if not isinstance(images, (list, tuple)) or len(images) == 0:
        raise ValueError("{}: images must be a non-empty list of [h, w, 3] uint8 tensors".format(what))
    dev = images[0].device if isinstance(images[0], Tensor) else None
    for i, im in enumerate(images):
        if (not isinstance(im, Tensor) or im.dim() != 3 or im.shape[2] != 3 or im.dtype != torch.uint8 or not im.is_contiguous() or im.device != dev
                or im.shape[0] < 1 or im.shape[1] < 1):
            raise ValueError("{}: image {} must be a contiguous [h, w, 3] uint8 tensor on {}, got {}".format(
                what, i, dev, "{} {} on {}".format(tuple(im.shape), im.dtype, im.device) if isinstance(im, Tensor) else type(im).__name__))
    return dev


def augment_batch(images: Sequence[Tensor], params: Sequence[Params], size: Tuple[int, int], out: Optional[Tensor] = None) -> Tensor:
    """The launch: images (a list of contiguous [h_i, w_i, 3] uint8 tensors on one GPU) and one Params each -> [n, 3, size[0], size[1]] float32 in
    [0, 1], not normalised (dn_augment_batch; `out` receives it when given). The library validates every record on the host before anything is launched (RuntimeError), and the call waits
    until the parameter table, host memory of the call, has been copied to the device; the launches run on behind it on the current stream."""
    dev = _check_images(images, "augment_batch")
    n = len(images)
    if len(params) != n:
        raise ValueError("augment_batch: {} images but {} parameter records".format(n, len(params)))
    if dev.type != "cuda":
        raise RuntimeError("augment_batch: the images must be on the GPU (demonet_amd has no CPU fallback)")
    sh, sw = int(size[0]), int(size[1])
    if out is None:
        out = torch.empty((n, 3, sh, sw), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (n, 3, sh, sw) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError("augment_batch: out must be a contiguous float32 tensor of shape {} on {}".format((n, 3, sh, sw), dev))
    L = _lib.lib()
    ptrs = (C.c_void_p * n)(*[im.data_ptr() for im in images])
    sizes = np.ascontiguousarray([[im.shape[0], im.shape[1]] for im in images], dtype=np.int32)
    rec = pack(params)
    ws_bytes = L.dn_augment_workspace_bytes(n)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.dn_augment_batch(ptrs, sizes.ctypes.data_as(C.POINTER(C.c_int32)), rec.ctypes.data_as(C.POINTER(C.c_int32)), n, sh, sw,
                                      C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                                      C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "dn_augment_batch")
    return out


class DetectionPresetTrain:
    """The reference's DetectionPresetTrain (presets.py:4-23) for a whole batch on the device, resize to `size` = (S_h, S_w) included.
    preset(images, targets, generator=None) -> (batch [n, 3, S_h, S_w] float32 in [0, 1], targets): what SSD.loss takes. Further keyword
    arguments are AugmentSampler's (the reference's constructor defaults)."""

    def __init__(self, data_augmentation, hflip_prob=0.5, mean=(123.0, 117.0, 104.0), size=(320, 320), **sampler_kw):
        self.sampler = AugmentSampler(data_augmentation, hflip_prob=hflip_prob, mean=mean, size=size, **sampler_kw)
        self.size = self.sampler.size

    def __call__(self, images: Sequence[Tensor], targets: Sequence[Dict[str, Tensor]], generator: Optional[torch.Generator] = None):
        dev = _check_images(images, "DetectionPresetTrain")
        if not isinstance(targets, (list, tuple)) or len(targets) != len(images):
            raise ValueError("DetectionPresetTrain: {} images but {} targets".format(
                len(images), len(targets) if isinstance(targets, (list, tuple)) else type(targets).__name__))
        params, tg = self.sampler.sample([(im.shape[0], im.shape[1]) for im in images], targets, generator)
        batch = augment_batch(images, params, self.size)
        return batch, [{"boxes": t["boxes"].to(dev), "labels": t["labels"].to(dev)} for t in tg]
