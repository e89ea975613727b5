"""dev tool: what the training augmentation costs per batch, and what the hand-written launches replace.
    python tools/time_augment.py [--out profiles/augment_timing.json] [--rounds 5] [--reps 20]
64 decoded images of 375 x 500 (uint8 HWC noise, five boxes each) through DetectionPresetTrain('ssd') to 320 x 320, one fixed set of sampled
records. Device events around `reps` calls of each variant, the variants alternated over `rounds` rounds, medians reported (ms per batch):
  launch        augment_batch alone on the fixed records: the table upload and the three launches (dn_augment_batch)
  preset        the whole preset call: host sampler (fresh draws from a seeded generator), launch, targets to the device -- host clock
  sampler       the host sampler alone -- host clock
  torch         the SAME fixed records applied per image with torch ops on the same device (torchvision's tensor formulas restated: blend, gray,
                _rgb2hsv / _hsv2rgb, pad, slice, flip, F.interpolate), stacked into the batch
Before anything is timed the two results are compared (largest absolute difference). One JSON document on stdout and in --out. The figures are
one box's."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from demonet_amd import augment  # noqa: E402

N, H, W, S = 64, 375, 500, (320, 320)


def _gray(x):
    return (0.2989 * x[0] + 0.587 * x[1] + 0.114 * x[2]).unsqueeze(0)


def _blend(a, b, f):
    return (f * a + (1.0 - f) * b).clamp(0, 1)


def _rgb2hsv(img):
    r, g, b = img.unbind(0)
    maxc, minc = img.max(0).values, img.min(0).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    div = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    return torch.stack((h, s, maxc))


def _hsv2rgb(img):
    h, s, v = img.unbind(0)
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.to(torch.int32) % 6
    p = (v * (1.0 - s)).clamp(0, 1)
    q = (v * (1.0 - s * f)).clamp(0, 1)
    t = (v * (1.0 - s * (1.0 - f))).clamp(0, 1)
    mask = i.unsqueeze(0) == torch.arange(6, device=img.device).view(-1, 1, 1)
    a4 = torch.stack((torch.stack((v, q, p, p, t, v)), torch.stack((t, v, v, q, p, p)), torch.stack((p, p, t, v, v, q))))
    return torch.einsum("ijk, xijk -> xjk", mask.to(img.dtype), a4)


def torch_apply(u8, p, size):
    """one record with torch ops on the image's device -> [3, S_h, S_w]"""
    x = u8.permute(2, 0, 1).float() / 255
    if p.brightness is not None:
        x = _blend(x, torch.zeros_like(x), p.brightness)
    if p.contrast is not None and p.contrast_before:
        x = _blend(x, _gray(x).mean(), p.contrast)
    if p.saturation is not None:
        x = _blend(x, _gray(x), p.saturation)
    if p.hue is not None:
        hsv = _rgb2hsv(x)
        x = _hsv2rgb(torch.stack(((hsv[0] + p.hue) % 1.0, hsv[1], hsv[2])))
    if p.contrast is not None and not p.contrast_before:
        x = _blend(x, _gray(x).mean(), p.contrast)
    x = x[list(p.perm)]
    h, w = x.shape[1:]
    canvas = torch.tensor(p.fill, dtype=torch.float32, device=x.device).view(3, 1, 1).expand(3, p.canvas_h, p.canvas_w).clone()
    canvas[:, p.top:p.top + h, p.left:p.left + w] = x
    crop = canvas[:, p.crop_t:p.crop_t + p.crop_h, p.crop_l:p.crop_l + p.crop_w]
    if p.flip:
        crop = crop.flip(-1)
    return F.interpolate(crop[None], size=size, mode="bilinear", align_corners=False)[0]


def _events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def _host_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_timing.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    rng = np.random.default_rng(0)
    images = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda() for _ in range(N)]
    targets = []
    for _ in range(N):
        xy = rng.uniform(0, 0.5, (5, 2)).astype(np.float32) * np.array([W, H], np.float32)
        wh = rng.uniform(0.1, 0.5, (5, 2)).astype(np.float32) * np.array([W, H], np.float32)
        targets.append({"boxes": torch.from_numpy(np.concatenate([xy, xy + wh], 1)), "labels": torch.from_numpy(rng.integers(1, 91, 5))})
    preset = augment.DetectionPresetTrain("ssd", size=S)
    sizes = [(H, W)] * N
    params, _ = preset.sampler.sample(sizes, targets, torch.Generator().manual_seed(0))
    out = torch.empty((N, 3) + S, device="cuda")
    gen = torch.Generator().manual_seed(1)

    launch = lambda: augment.augment_batch(images, params, S, out=out)
    torch_path = lambda: torch.stack([torch_apply(im, p, S) for im, p in zip(images, params)])
    diff = float((launch() - torch_path()).abs().max())
    variants = dict(launch=(launch, _events_ms), preset=(lambda: preset(images, targets, gen), _host_ms),
                    sampler=(lambda: preset.sampler.sample(sizes, targets, gen), _host_ms), torch=(torch_path, _events_ms))
    for fn, _ in variants.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for name, (fn, timer) in variants.items():
            times[name].append(timer(fn, a.reps))
    flags = [p.flags() for p in params]
    doc = dict(images=N, image_size=[H, W], out_size=list(S), policy="ssd", rounds=a.rounds, reps=a.reps, device=torch.cuda.get_device_name(0),
               records=dict(brightness=sum(f & 1 > 0 for f in flags), contrast=sum(f & 2 > 0 for f in flags), saturation=sum(f & 4 > 0 for f in flags),
                            hue=sum(f & 8 > 0 for f in flags), flip=sum(f & 32 > 0 for f in flags), zoomed=sum(p.canvas_h != H for p in params),
                            cropped=sum(p.option < 1.0 for p in params)),
               max_abs_diff_launch_vs_torch=diff,
               median_ms={k: round(statistics.median(v), 4) for k, v in times.items()},
               min_ms={k: round(min(v), 4) for k, v in times.items()}, max_ms={k: round(max(v), 4) for k, v in times.items()})
    med = doc["median_ms"]
    doc["launch_images_per_s"] = round(N / med["launch"] * 1e3)
    doc["torch_over_launch"] = round(med["torch"] / med["launch"], 2)
    doc["torch_over_preset"] = round(med["torch"] / med["preset"], 2)
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
