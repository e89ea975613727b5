"""Reference of dn_crop_objects (include/demonet_hip.h): steps 1-8 in float32 numpy, one rounding per operation. `rect` is one row's way from box
to integer rectangle, `rects` numbers the survivors and builds the index table, `patches` cuts every kept rectangle out of the CONVERTED frame and
resizes it with regions_ref.resize_u8 (the uint8 path's resize), then normalises; `patches_sampled` does the same tap by tap from the planes with
regions_ref.sample -- tests/test_crops.py shows the two agree bit for bit. The deliberate mistakes (MISTAKES) are what the tests use to show that
the box and frame set of the GPU tests can tell right from wrong. Nothing here is fitted to device output."""
from collections import namedtuple

import numpy as np

import regions_ref as rr

F = np.float32
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

Params = namedtuple("Params", "margin square min_w min_h mean std out_h out_w fp16 capacity")


def params(size=(16, 8), capacity=64, fp16=False, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), margin=0.0, square=False, min_size=(1, 1)):
    """size and min_size are (height, width), as ObjectCropper's"""
    return Params(float(margin), bool(square), int(min_size[1]), int(min_size[0]), tuple(mean), tuple(std), int(size[0]), int(size[1]), bool(fp16),
                  int(capacity))


# "round": floor(x + 0.5) for both edges instead of floor / ceil; "clamp_first": the box clamped to the frame BEFORE the margin is applied;
# "no_intersection": step 4's test that the rectangle meets the frame left out; "reciprocal": (v - mean) * (1 / std) instead of the division
MISTAKES = ("round", "clamp_first", "no_intersection", "reciprocal")


def rect(box, W, H, p, mistake=None):
    """steps 1 (without select) to 5 of one row: (X0, Y0, width, height) or None"""
    with np.errstate(all="ignore"):
        x1, y1, x2, y2 = (F(v) for v in box)
        if not all(np.isfinite(v) for v in (x1, y1, x2, y2)):
            return None
        if mistake == "clamp_first":
            x1, y1, x2, y2 = np.maximum(x1, F(0)), np.maximum(y1, F(0)), np.minimum(x2, F(W)), np.minimum(y2, F(H))
        w, h = x2 - x1, y2 - y1
        if not (w > 0 and h > 0):
            return None
        m = F(p.margin)
        mx, my = w * m, h * m
        xa, xb, ya, yb = x1 - mx, x2 + mx, y1 - my, y2 + my
        if p.square:
            cw, ch = xb - xa, yb - ya
            s = np.maximum(cw, ch)
            hs = s * F(0.5)
            cx, cy = (xa + xb) * F(0.5), (ya + yb) * F(0.5)
            xa, xb, ya, yb = cx - hs, cx + hs, cy - hs, cy + hs
        assert all(v.dtype == F for v in (xa, xb, ya, yb))
        if not all(np.isfinite(v) for v in (xa, xb, ya, yb)):
            return None
        if mistake != "no_intersection" and not (xb > 0 and xa < F(W) and yb > 0 and ya < F(H)):
            return None
        lo, hi = (lambda v: np.floor(v + F(0.5)), lambda v: np.floor(v + F(0.5))) if mistake == "round" else (np.floor, np.ceil)
        X0 = int(np.minimum(np.maximum(lo(xa), F(0)), F(W - 1)))
        X1 = int(np.minimum(np.maximum(hi(xb), F(X0 + 1)), F(W)))
        Y0 = int(np.minimum(np.maximum(lo(ya), F(0)), F(H - 1)))
        Y1 = int(np.minimum(np.maximum(hi(yb), F(Y0 + 1)), F(H)))
    width, height = X1 - X0, Y1 - Y0
    if width < p.min_w or height < p.min_h:
        return None
    return X0, Y0, width, height


def rects(boxes, counts, sizes, select, p, mistake=None):
    """boxes [B, d, 4] fp32, counts [B], sizes [(H, W)] per stream, select [B, d] or None -> (index [capacity, 8] int32, kept, dropped)"""
    boxes = np.asarray(boxes, dtype=F)
    B, d = boxes.shape[:2]
    rows = []
    for b in range(B):
        H, W = sizes[b]
        for j in range(min(max(int(counts[b]), 0), d)):
            if select is not None and not select[b][j]:
                continue
            r = rect(boxes[b, j], W, H, p, mistake)
            if r is not None:
                rows.append((b, j) + r + (0, 0))
    kept = min(len(rows), p.capacity)
    index = np.zeros((p.capacity, 8), dtype=np.int32)
    index[:, 0] = -1
    if kept:
        index[:kept] = np.asarray(rows[:kept], dtype=np.int32)
    return index, kept, len(rows) - kept


def normalise(v, p, mistake=None):
    """[3, oh, ow] fp32 -> the stored patch: (v - mean) / std per channel in fp32, then the fp16 conversion (numpy's rounds to nearest even)"""
    mean, std = np.asarray(p.mean, dtype=F)[:, None, None], np.asarray(p.std, dtype=F)[:, None, None]
    o = (v - mean) * (F(1) / std) if mistake == "reciprocal" else (v - mean) / std
    assert o.dtype == F
    return o.astype(np.float16) if p.fp16 else o


def patches(rgbs, index, kept, p, mistake=None):
    """rgbs: the converted frames [H, W, 3] uint8 per stream -> [kept, 3, out_h, out_w] in the output type"""
    out = np.zeros((kept, 3, p.out_h, p.out_w), dtype=np.float16 if p.fp16 else F)
    for s in range(kept):
        b, _, x0, y0, w, h = (int(v) for v in index[s, :6])
        out[s] = normalise(rr.resize_u8(rr.crop(rgbs[b], (b, x0, y0, w, h, 0)), p.out_h, p.out_w), p, mistake)
    return out


def patches_sampled(planes, matrix, full, index, kept, p):
    """the same from the (Y, U, V) planes of every stream, tap by tap (regions_ref.sample)"""
    out = np.zeros((kept, 3, p.out_h, p.out_w), dtype=np.float16 if p.fp16 else F)
    for s in range(kept):
        b, _, x0, y0, w, h = (int(v) for v in index[s, :6])
        Y, U, V = planes[b]
        out[s] = normalise(rr.sample(Y, U, V, matrix, full, (b, x0, y0, w, h, 0), p.out_h, p.out_w), p)
    return out


def step(rgbs, boxes, counts, sizes, select, p, mistake=None):
    """(patches [kept, ...], index, totals [4] int32)"""
    index, kept, dropped = rects(boxes, counts, sizes, select, p, None if mistake == "reciprocal" else mistake)
    return patches(rgbs, index, kept, p, mistake), index, np.asarray([kept, dropped, 0, 0], dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------- the set the GPU tests run
# two frames of regions_ref.SIZES, (height, width) = (200, 260) and (97, 131); D rows per stream, the rows behind COUNTS are garbage
D = 24
NAN, INF = float("nan"), float("inf")
BOXES = [
    [(10.2, 20.7, 30.1, 40.0),            # the header's worked example
     (-5.5, 50.0, 20.5, 90.0), (240.0, 10.0, 275.0, 60.0), (100.0, -8.0, 140.0, 12.5), (100.0, 180.0, 150.0, 215.0),      # over each edge
     (-30.0, 10.0, -2.0, 40.0), (262.0, 10.0, 290.0, 40.0), (10.0, -40.0, 40.0, -1.0), (10.0, 201.0, 40.0, 230.0),        # outside on each side
     (NAN, 10.0, 50.0, 60.0), (10.0, 10.0, INF, 60.0), (-INF, 10.0, 50.0, 60.0), (40.0, 40.0, 40.0, 80.0), (60.0, 40.0, 50.0, 80.0),
     (-3e38, 10.0, 3e38, 60.0), (3e38, 3e38, 3.2e38, 3.2e38),
     (50.5, 60.5, 70.5, 100.5),           # halves: where rounding and floor / ceil part
     (40.0, 30.0, 48.0, 46.0),            # 8 x 16: exactly the (16, 8) patch
     (100.2, 100.3, 100.6, 100.8),        # a 1 x 1 rectangle
     (0.0, 0.0, 260.0, 200.0),            # the whole frame
     (1e9, 1e9, 2e9, 2e9), (7.0, 7.0, 9.0, 8.0), (5.0, 5.0, 6.0, 6.0), (1.0, 2.0, 3.0, 4.0)],
    [(125.5, 90.2, 140.0, 100.0),         # over the bottom-right corner of the odd frame
     (130.1, 96.2, 130.9, 96.8),          # its last row and column
     (20.3, 10.1, 60.7, 80.9), (0.0, 0.0, 131.0, 97.0), (64.5, 3.5, 99.5, 91.5), (-2.0, -2.0, 1.5, 1.5), (90.0, 60.0, 98.0, 76.0),
     (30.0, 30.0, 31.0, 31.0), (131.0, 10.0, 140.0, 20.0), (10.0, 97.0, 20.0, 110.0), (-9.0, 5.0, 0.0, 50.0), (5.0, -9.0, 50.0, 0.0),
     (0.0, 96.1, 131.0, 96.9), (130.2, 0.0, 130.7, 97.0)] +     # the whole last row, the whole last column
    [(10.0, 10.0, 20.0, 20.0)] * 2 + [(NAN,) * 4] * 8,
]
COUNTS = [21, 14]
assert all(len(b) == D for b in BOXES)
# the parameter sets the GPU tests run on BOXES (name -> Params): every mistake changes the result of at least one of them (tests/test_crops.py)
CONFIGS = {
    "f32-16x8": params((16, 8)),
    "f32-12x20": params((12, 20)),
    "f32-7x5": params((7, 5)),
    "f16-6x9": params((6, 9), fp16=True),
    "f16-16x8": params((16, 8), fp16=True),
    "f32-1x1": params((1, 1)),
    "imagenet-f32": params((16, 8), mean=IMAGENET_MEAN, std=IMAGENET_STD),
    "imagenet-f16": params((16, 8), fp16=True, mean=IMAGENET_MEAN, std=IMAGENET_STD),
    "margin": params((16, 8), margin=0.1),
    "square": params((12, 12), square=True, margin=0.25, fp16=True),
    "min-size": params((16, 8), min_size=(3, 2)),
    "overflow": params((4, 4), capacity=5),
}


def boxes_array():
    return np.asarray(BOXES, dtype=F), np.asarray(COUNTS, dtype=np.int32)


def random_boxes(seed, sizes, d, keep=0.6):
    """seeded boxes around each frame, a fifth of them hanging over an edge or outside, and a random select: (boxes [B, d, 4], counts [B], select [B, d])"""
    rng = np.random.default_rng(seed)
    B = len(sizes)
    boxes = np.zeros((B, d, 4), dtype=F)
    for b, (H, W) in enumerate(sizes):
        cx, cy = rng.uniform(-0.1 * W, 1.1 * W, d), rng.uniform(-0.1 * H, 1.1 * H, d)
        w, h = rng.uniform(0.5, 0.3 * W, d), rng.uniform(0.5, 0.5 * H, d)
        boxes[b] = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1).astype(F)
    counts = np.asarray([d if b % 2 == 0 else d - 7 for b in range(B)], dtype=np.int32)
    select = (rng.uniform(0, 1, (B, d)) < keep).astype(np.uint8)
    return boxes, counts, select
