"""TEST INFRASTRUCTURE: the reference of camera-motion compensation (demonet_amd/motion.py, csrc/motion.hip).

`RefCompensator` restates the text of include/demonet_hip.h (dn_motion_estimate) in integer and float64 numpy: the luma thumbnail, the block
vectors by exhaustive search under the total order (SAD, dx^2 + dy^2, dy, dx), the lower medians, the exact integer sums (Python ints) and the
closed-form fit. `compensate` restates dn_track_compensate on a track_ref.RefTracker in float32, one operation per line. A correct device
implementation must agree with both bit for bit. `textured` / `pan_scene` are the seeded image generators of the tests and of
tools/time_motion.py.
"""
import numpy as np

f32 = np.float32
MAX_K = 4096


def luma(frame, format):
    """The 8-bit luma [H, W] of a frame: the Y plane as it lies, or (77 R + 150 G + 29 B + 128) >> 8 of an [H, W, 3] RGB / BGR image."""
    frame = np.asarray(frame)
    if format in ("nv12", "i420"):
        assert frame.ndim == 2 and frame.dtype == np.uint8
        return frame
    assert frame.ndim == 3 and frame.shape[2] == 3 and frame.dtype == np.uint8
    p = frame.astype(np.int64)
    r, g, b = (p[..., 0], p[..., 1], p[..., 2]) if format == "rgb24" else (p[..., 2], p[..., 1], p[..., 0])
    return ((77 * r + 150 * g + 29 * b + 128) >> 8).astype(np.uint8)


def box_side(H, W, TH, TW):
    """k: the smallest integer >= 1 with floor(W / k) <= TW and floor(H / k) <= TH."""
    k = 1
    while W // k > TW or H // k > TH:
        k += 1
    return k


def thumbnail(y, TH, TW):
    """(the thumbnail [th, tw] uint8, k) of the luma image y [H, W]."""
    H, W = y.shape
    k = box_side(H, W, TH, TW)
    assert k <= MAX_K
    th, tw = H // k, W // k
    s = y[:th * k, :tw * k].astype(np.int64).reshape(th, k, tw, k).sum(axis=(1, 3))
    return ((s + (k * k) // 2) // (k * k)).astype(np.uint8), k


def grid(th, tw, block, radius):
    """(nbx, nby) of a thumbnail."""
    need = block + 2 * radius
    if tw < need or th < need:
        return 0, 0
    return (tw - 2 * radius) // block, (th - 2 * radius) // block


def block_vector(cur, prev, bx, by, block, radius):
    """(dx, dy, sad) of the block at (bx, by) of cur searched in prev: the minimum of the total order (SAD, dx^2 + dy^2, dy, dx)."""
    blk = cur[by:by + block, bx:bx + block].astype(np.int32)
    win = prev[by - radius:by + radius + block, bx - radius:bx + radius + block].astype(np.int32)
    cand = np.lib.stride_tricks.sliding_window_view(win, (block, block))            # [dy + radius, dx + radius, block, block]
    sad = np.abs(cand - blk).sum(axis=(2, 3)).reshape(-1)
    dy, dx = [v.reshape(-1) for v in np.mgrid[-radius:radius + 1, -radius:radius + 1]]
    i = np.lexsort((dx, dy, dx * dx + dy * dy, sad))[0]                             # (the last key is the primary one)
    return int(dx[i]), int(dy[i]), int(sad[i])


def texture(cur, bx, by, block):
    p = cur[by:by + block, bx:bx + block].astype(np.int64)
    m = (int(p.sum()) + block * block // 2) // (block * block)
    return int(np.abs(p - m).sum())


def masked(k, bx, by, block, boxes, scores, count, mask_thresh):
    """Does the block's centre lie inside a masking row (boxes [d, 4] f32, scores [d] f32, the rows below count)."""
    if boxes is None:
        return False
    cx = f32(k * (bx + block // 2)) - f32(0.5)
    cy = f32(k * (by + block // 2)) - f32(0.5)
    n = min(max(int(count), 0), len(scores))
    for j in range(n):
        s, b = f32(scores[j]), np.asarray(boxes[j], f32)
        if np.isnan(s) or not s >= f32(mask_thresh) or not np.all(np.isfinite(b)):
            continue
        if b[0] <= cx and cx < b[2] and b[1] <= cy and cy < b[3]:
            return True
    return False


def lower_median(v):
    return sorted(v)[(len(v) - 1) // 2]


def fit(vectors, nbx, block, radius, k, min_blocks):
    """The robust fit over the rows (dx, dy, sad, valid) of a frame's blocks -> (s, tx, ty, ok) float32 [4], valid, inliers."""
    ident = np.array([1, 0, 0, 0], f32)
    val = [(i, int(v[0]), int(v[1])) for i, v in enumerate(vectors) if v[3]]
    if not val:
        return ident, 0, 0
    mdx, mdy = lower_median([v[1] for v in val]), lower_median([v[2] for v in val])
    n = sx = sy = sxp = syp = sqq = sxx = 0            # Python ints: exact
    for i, dx, dy in val:
        if max(abs(dx - mdx), abs(dy - mdy)) > 2:
            continue
        xp, yp = radius + (i % nbx) * block + block // 2, radius + (i // nbx) * block + block // 2
        x, y = xp + dx, yp + dy
        n, sx, sy, sxp, syp = n + 1, sx + x, sy + y, sxp + xp, syp + yp
        sqq += x * x + y * y
        sxx += x * xp + y * yp
    num, den = n * sxx - sx * sxp - sy * syp, n * sqq - sx * sx - sy * sy
    if len(val) < min_blocks or 2 * n < len(val) or den == 0:
        return ident, len(val), n
    f64 = np.float64
    s = f64(num) / f64(den)
    if not (s >= 0.8 and s <= 1.25):
        return ident, len(val), n
    tu = (f64(sxp) - s * f64(sx)) / f64(n)
    tv = (f64(syp) - s * f64(sy)) / f64(n)
    c = ((f64(1) - s) * f64(k - 1)) / f64(2)
    return np.array([f32(s), f32(f64(k) * tu + c), f32(f64(k) * tv + c), 1], f32), len(val), n


class RefCompensator:
    def __init__(self, streams, max_size=(144, 256), block=16, radius=16, min_texture=None, min_blocks=8, mask_thresh=0.5):
        self.B, (self.TH, self.TW), self.block, self.radius = streams, max_size, block, radius
        self.min_texture = 2 * block * block if min_texture is None else min_texture
        self.min_blocks, self.mask_thresh = min_blocks, mask_thresh
        self.max_blocks = ((self.TW - 2 * radius) // block) * ((self.TH - 2 * radius) // block)
        self.reset()

    def reset(self, streams=None):
        if streams is None:
            self.stored = [None] * self.B            # per stream: (thumbnail, (H, W)) of the previous frame
        else:
            for b in streams:
                self.stored[b] = None

    def estimate(self, lumas, boxes=None, scores=None, counts=None):
        """One step. lumas: per stream the luma image [H, W] uint8 -> motion [B, 4] f32, stats [B, 4] i32, vectors [B, max_blocks, 4] i32; the
        step's thumbnails are in self.thumbs."""
        B = self.B
        assert len(lumas) == B
        motion, stats = np.zeros((B, 4), f32), np.zeros((B, 4), np.int32)
        vectors = np.zeros((B, self.max_blocks, 4), np.int32)
        self.thumbs = []
        for b in range(B):
            cur, k = thumbnail(np.asarray(lumas[b]), self.TH, self.TW)
            self.thumbs.append(cur)
            th, tw = cur.shape
            nbx, nby = grid(th, tw, self.block, self.radius)
            st = self.stored[b]
            seeded = st is not None and st[1] == tuple(lumas[b].shape)
            if seeded:
                for n in range(nbx * nby):
                    bx, by = self.radius + (n % nbx) * self.block, self.radius + (n // nbx) * self.block
                    dx, dy, sad = block_vector(cur, st[0], bx, by, self.block, self.radius)
                    ok = texture(cur, bx, by, self.block) >= self.min_texture and not masked(
                        k, bx, by, self.block, None if boxes is None else boxes[b], None if boxes is None else scores[b],
                        None if boxes is None else counts[b], self.mask_thresh)
                    vectors[b, n] = (dx, dy, sad, int(ok))
                motion[b], valid, inl = fit(vectors[b, :nbx * nby], nbx, self.block, self.radius, k, self.min_blocks)
            else:
                motion[b], valid, inl = np.array([1, 0, 0, 0], f32), 0, 0
            stats[b] = (nbx * nby, valid, inl, k)
            self.stored[b] = (cur, tuple(lumas[b].shape))
        return motion, stats, vectors


def compensate(tracker, motion):
    """dn_track_compensate on a track_ref.RefTracker: float32, one operation per line."""
    motion = np.asarray(motion, f32)
    for b in range(tracker.B):
        s, tx, ty, ok = motion[b]
        if not ok != 0:
            continue
        s2 = s * s
        for slot in range(tracker.T):
            if tracker.state[b, slot] == 0:
                continue
            f = tracker.filter[b, :, slot]
            for k, t in ((0, tx), (1, ty), (3, None)):
                x = s * f[5 * k]
                f[5 * k] = x + t if t is not None else x
                f[5 * k + 1] = s * f[5 * k + 1]
                f[5 * k + 2] = f[5 * k + 2] * s2
                f[5 * k + 3] = f[5 * k + 3] * s2
                f[5 * k + 4] = f[5 * k + 4] * s2
            assert f.dtype == np.float32


# ---------------------------------------------------------------------------------------------------------- images
def textured(seed, H, W, cell=4):
    """A random image with structure at the scale of `cell` pixels (so that a box-filtered thumbnail keeps texture): uint8 [H, W]."""
    rng = np.random.RandomState(seed)
    small = rng.randint(0, 256, ((H + cell - 1) // cell, (W + cell - 1) // cell)).astype(np.uint8)
    return np.repeat(np.repeat(small, cell, axis=0), cell, axis=1)[:H, :W].copy()


def window(canvas, x, y, H, W):
    """The [H, W] view of a canvas with its corner at (x, y): a camera at that position. The content at frame pixel (i, j) is canvas[y + j, x + i]:
    a camera that moves by (+px, +py) moves the image content by (-px, -py)."""
    assert 0 <= x and 0 <= y and y + H <= canvas.shape[0] and x + W <= canvas.shape[1]
    return np.ascontiguousarray(canvas[y:y + H, x:x + W])
