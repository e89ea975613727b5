"""Reference of the on-screen display (include/demonet_hip.h, dn_osd_paint) in numpy: planes in, planes out, the text builder, and the
colour conversion derived from Kr, Kb in float64. Nothing here is fitted to device output. Every float operation of the segment test is one
numpy float32 operation (one rounding each, no contraction); everything else is integer arithmetic.

A frame is three channel arrays in LOGICAL order with a subsampling factor each: (Y, U, V) with (1, 2, 2) for nv12 / i420, (R, G, B) with
(1, 1, 1) for rgb24 / bgr24 (`split` / `join` go from and to the payload planes of tests/test_gpu_regions.py's `_source`).

`paint(..., variant=)` also states six WRONG painters -- the classic mistakes -- so that tests/test_osd.py can show that the scenes of the GPU
tests tell each of them from the right one."""
import numpy as np

import frames_ref as fr

LABEL, SCORE, HIDE = 1, 2, 4
VARIANTS = ("reverse_boxes", "chroma_bottom_right", "blend_truncates", "pixelate_painted", "label_inside", "outline_unclamped")
f32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- colours
def forward_coeffs(matrix, full):
    """((yr, yg, yb), (ur, ug, ub), (vr, vg, vb), yo): round(c 2^14) of the forward matrix, read off frames_ref.rgb_to_yuv_real (Kr, Kb in float64)"""
    zero = np.array(fr.rgb_to_yuv_real(np.zeros(3), matrix, full), np.float64)
    cols = [(np.array(fr.rgb_to_yuv_real(255.0 * np.eye(3)[i], matrix, full), np.float64) - zero) / 255.0 for i in range(3)]
    m = np.stack(cols, 1)                                    # [component][R, G, B]
    q = np.floor(m * (1 << 14) + 0.5).astype(np.int64)
    return tuple(int(v) for v in q[0]), tuple(int(v) for v in q[1]), tuple(int(v) for v in q[2]), 0 if full else 16


def to_surface(rgb, fmt, matrix, full):
    if fmt in ("rgb24", "bgr24"):
        return tuple(int(v) for v in rgb)
    cy, cu, cv, yo = forward_coeffs(matrix, full)
    out = []
    for c, off in ((cy, yo), (cu, 128), (cv, 128)):
        s = int(c[0]) * int(rgb[0]) + int(c[1]) * int(rgb[1]) + int(c[2]) * int(rgb[2]) + (1 << 13)
        out.append(int(np.clip((s >> 14) + off, 0, 255)))
    return tuple(out)


def text_colour(rgb):
    return (0, 0, 0) if 299 * rgb[0] + 587 * rgb[1] + 114 * rgb[2] >= 128000 else (255, 255, 255)


def palette_records(palette_rgb, fmt, matrix, full):
    """[(colour, text colour)] in surface space"""
    return [(to_surface(c, fmt, matrix, full), to_surface(text_colour(c), fmt, matrix, full)) for c in palette_rgb]


# ---------------------------------------------------------------------------------------------------------------- planes
def split(fmt, planes):
    """payload planes -> ([three channel arrays, logical order], subs)"""
    if fmt == "nv12":
        return [planes[0].copy(), planes[1][:, 0::2].copy(), planes[1][:, 1::2].copy()], (1, 2, 2)
    if fmt == "i420":
        return [p.copy() for p in planes], (1, 2, 2)
    h = planes[0].shape[0]
    px = planes[0].reshape(h, -1, 3)
    order = (0, 1, 2) if fmt == "rgb24" else (2, 1, 0)
    return [px[..., i].copy() for i in order], (1, 1, 1)


def join(fmt, chans):
    if fmt == "nv12":
        return [chans[0], fr.interleave(chans[1], chans[2])]
    if fmt == "i420":
        return list(chans)
    order = (0, 1, 2) if fmt == "rgb24" else (2, 1, 0)
    h = chans[0].shape[0]
    return [np.stack([chans[i] for i in order], -1).reshape(h, -1)]


# ---------------------------------------------------------------------------------------------------------------- text
def build_text(name, ident, with_score, score):
    """name: bytes (16, NUL-padded) or None; ident: int or None (no ids); returns the label's bytes"""
    out = b""
    if name is not None:
        out += bytes(name[:15]).split(b"\0")[0]
    if ident is not None:
        out += b" #" + (str(int(ident)).encode() if 0 <= int(ident) <= 999999999 else b"?")
    if with_score:
        s = f32(score)
        if not np.isfinite(s):
            out += b" ?%"
        else:
            with np.errstate(all="ignore"):
                v = s * f32(100.0) + f32(0.5)
            p = 0 if v < 0 else (100 if v > 100 else int(v))
            out += b" " + str(p).encode() + b"%"
    return out


def glyph(byte):
    if 97 <= byte <= 122:
        byte -= 32
    return (byte if 32 <= byte <= 95 else 63) - 32


# ---------------------------------------------------------------------------------------------------------------- the painter
def _clampi(v, lo, hi):
    return int(min(max(v, f32(lo)), f32(hi)))


def row_rect(box, W, H):
    """(ix0, iy0, ix1, iy1) or None for a box that is not finite or whose rectangle is empty"""
    b = np.asarray(box, f32)
    if not np.all(np.isfinite(b)):
        return None
    r = (_clampi(np.floor(b[0]), 0, W), _clampi(np.floor(b[1]), 0, H), _clampi(np.ceil(b[2]), 0, W), _clampi(np.ceil(b[3]), 0, H))
    return None if r[0] >= r[2] or r[1] >= r[3] else r


def segments(cfg):
    """[(ax, ay, bx, by, is_line)] of a zone config dict (n_lines, lines [16][4], n_zones, nv [16], verts [16][16][2]) in paint order, clamped"""
    if cfg is None:
        return []
    out = []
    for i in range(int(np.clip(cfg["n_lines"], 0, 16))):
        out.append(tuple(f32(v) for v in cfg["lines"][i]) + (True,))
    for z in range(int(np.clip(cfg["n_zones"], 0, 16))):
        nv = int(np.clip(cfg["nv"][z], 3, 16))
        for e in range(nv):
            a, b = cfg["verts"][z][e], cfg["verts"][z][(e + 1) % nv]
            out.append((f32(a[0]), f32(a[1]), f32(b[0]), f32(b[1]), False))
    return out


def segment_mask(seg, r, W, H):
    ax, ay, bx, by = seg[:4]
    with np.errstate(all="ignore"):
        dx, dy = bx - ax, by - ay
        L = dx * dx + dy * dy
        if not np.isfinite(L) or L == 0:
            return None
        px = (np.arange(W).astype(f32) + f32(0.5))[None, :]
        py = (np.arange(H).astype(f32) + f32(0.5))[:, None]
        t = ((px - ax) * dx + (py - ay) * dy) / L
        t = np.fmin(np.fmax(t, f32(0)), f32(1))
        qx, qy = ax + t * dx, ay + t * dy
        ex, ey = px - qx, py - qy
        rr = f32(r) * f32(r)
        return ex * ex + ey * ey <= rr


def block_mean(arr, s):
    h, w = arr.shape
    out = np.empty((h, w), np.int64)
    for y in range(0, h, s):
        for x in range(0, w, s):
            blk = arr[y:y + s, x:x + s].astype(np.int64)
            out[y:y + s, x:x + s] = (blk.sum() + blk.size // 2) // blk.size
    return out


def paint(chans, subs, rows, styles, default_style, n_labels, names, palette, font, cfg, params, variant=None):
    """chans: three uint8 arrays (logical order), subs their subsampling. rows: dict(boxes [d][4], scores [d], labels [d], ids [d] or None, count).
    styles: [n_labels] of (thickness, fill_alpha, pixelate, flags) or None; names: [n_labels] 16-byte records or None; palette: [(colour,
    text colour)] in surface space; font [64][8]; cfg: a zone config dict or None; params: dict(colour_by_id, scale, label_alpha, line_thickness,
    zone_thickness, zone_alpha, line_colour, zone_colour). Returns (the painted channels, (rows painted, rows skipped))."""
    H, W = chans[0].shape
    orig = [c.astype(np.int64) for c in chans]
    out = [c.astype(np.int64) for c in chans]
    off = 1 if variant == "chroma_bottom_right" else 0

    def governed(mask, i):
        if subs[i] == 1:
            return mask
        ch, cw = out[i].shape
        ys, xs = np.minimum(2 * np.arange(ch) + off, H - 1), np.minimum(2 * np.arange(cw) + off, W - 1)
        return mask[np.ix_(ys, xs)]

    def blend(mask, alpha, colour):
        for i in range(3):
            m = governed(mask, i)
            num = alpha * int(colour[i]) + (255 - alpha) * out[i][m] + (0 if variant == "blend_truncates" else 127)
            out[i][m] = num // 255

    def rect_mask(x0, y0, x1, y1):
        m = np.zeros((H, W), bool)
        m[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = True
        return m

    # 1. lines and zone edges
    for seg in segments(cfg):
        m = segment_mask(seg, f32(params["line_thickness"] if seg[4] else params["zone_thickness"]) * f32(0.5), W, H)
        if m is not None:
            blend(m, params["zone_alpha"], params["line_colour"] if seg[4] else params["zone_colour"])

    # 2. boxes
    d = len(rows["boxes"])
    n = min(max(int(rows["count"]), 0), d)
    used = []
    for j in range(n):
        label = int(rows["labels"][j])
        rect = row_rect(rows["boxes"][j], W, H)
        if rect is None or label < 0 or label >= n_labels:
            continue
        st = styles[label] if styles is not None else default_style
        if st[3] & HIDE:
            continue
        ident = int(rows["ids"][j]) if rows["ids"] is not None else None
        key = (ident if (ident is not None and params["colour_by_id"]) else label) & 0xFFFFFFFF
        used.append((j, rect, st, palette[key % len(palette)], label, ident))
    means = {}
    for j, rect, st, (colour, _), label, ident in (used[::-1] if variant == "reverse_boxes" else used):
        x0, y0, x1, y1 = rect
        thick = min(st[0], 16)
        block = st[2] if st[2] in (4, 8, 16, 32) else 0
        full = rect_mask(x0, y0, x1, y1)
        if block:
            for i in range(3):
                s = block // subs[i]
                if variant == "pixelate_painted":
                    mean = block_mean(out[i], s)
                else:
                    if (i, s) not in means:
                        means[(i, s)] = block_mean(orig[i], s)
                    mean = means[(i, s)]
                m = governed(full, i)
                out[i][m] = mean[m]
        if st[1]:
            blend(full, st[1], colour)
        if thick:
            if variant == "outline_unclamped":
                b = np.asarray(rows["boxes"][j], f32)
                ux0, uy0, ux1, uy1 = int(np.floor(b[0])), int(np.floor(b[1])), int(np.ceil(b[2])), int(np.ceil(b[3]))
            else:
                ux0, uy0, ux1, uy1 = x0, y0, x1, y1
            sx0, sy0, sx1, sy1 = ux0 + thick, uy0 + thick, ux1 - thick, uy1 - thick
            m = full.copy()
            if sx0 < sx1 and sy0 < sy1:
                m &= ~rect_mask(sx0, sy0, sx1, sy1)
            blend(m, 255, colour)

    # 3. labels
    k = params["scale"]
    for j, rect, st, (colour, tcolour), label, ident in used:
        if not st[3] & LABEL:
            continue
        text = build_text(names[label] if names is not None else None, ident, bool(st[3] & SCORE), rows["scores"][j])
        x0, y0 = rect[0], rect[1]
        top = y0 - 8 * k if (y0 >= 8 * k and variant != "label_inside") else y0
        right, bottom = min(x0 + 8 * k * len(text), W), min(top + 8 * k, H)
        if len(text) == 0 or x0 >= right or top >= bottom:
            continue
        cols = (np.arange(x0, right) - x0) // k
        rws = (np.arange(top, bottom) - top) // k
        g = np.array([glyph(c) for c in text], np.int64)[cols >> 3]
        on = ((font[g[None, :], rws[:, None]].astype(np.int64) >> (7 - (cols & 7))[None, :]) & 1).astype(bool)
        m_on = np.zeros((H, W), bool)
        m_off = np.zeros((H, W), bool)
        m_on[top:bottom, x0:right] = on
        m_off[top:bottom, x0:right] = ~on
        # a pixel takes one of the two colours; the two masks are disjoint, so the two blends are one per pixel
        blend(m_on, params["label_alpha"], tcolour)
        blend(m_off, params["label_alpha"], colour)
    return [c.astype(np.uint8) for c in out], (len(used), n - len(used))


# ---------------------------------------------------------------------------------------------------------------- the scenes the tests share
NAMES = ["person", "car", "Bus_01", "truck", "hidden", "abcdefghijklmno"]
PALETTE_RGB = [(230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48)]


def name_records(names=NAMES):
    return [n.encode("ascii").ljust(16, b"\0") for n in names]


def default_params(**kw):
    p = dict(colour_by_id=1, scale=1, label_alpha=255, line_thickness=2, zone_thickness=2, zone_alpha=255, line_colour=(255, 255, 0),
             zone_colour=(0, 255, 255))
    p.update(kw)
    return p


def make_rows(boxes, scores=None, labels=None, ids=None, count=None, d=None):
    n = len(boxes)
    d = n if d is None else d
    out = dict(boxes=np.zeros((d, 4), f32), scores=np.zeros(d, f32), labels=np.zeros(d, np.int64), ids=None, count=n if count is None else count)
    out["boxes"][:n] = np.asarray(boxes, f32).reshape(n, 4)
    out["scores"][:n] = np.asarray(scores if scores is not None else [0.5] * n, f32)
    out["labels"][:n] = np.asarray(labels if labels is not None else [0] * n, np.int64)
    if ids is not None:
        out["ids"] = np.zeros(d, np.int64)
        out["ids"][:n] = np.asarray(ids, np.int64)
    return out


# per label: (thickness, fill_alpha, pixelate, flags)
MIXED_STYLES = [(2, 0, 0, LABEL | SCORE), (1, 128, 0, LABEL), (3, 0, 0, 0), (0, 0, 8, 0), (2, 0, 0, HIDE), (5, 64, 4, LABEL | SCORE)]


def mixed_scene(W, H, shift=0):
    """One mixed scene for a frame of at least 131 x 97: outline + label, fill, an outline cut by the left edge, a pixelate row over the earlier
    fill, a box leaving the frame at the right and the bottom, a NaN row, a label out of range, a hidden row; two lines and one concave zone.
    Frames of 260 x 200 get the same set once more, moved into their other tiles. Returns (rows, zone config dict)."""
    base = [(10.3, 30.2, 60.7, 70.9), (40.5, 50.5, 90.2, 90.1), (-5.5, 20.0, 25.0, 45.0), (70.0, 10.0, 120.0, 60.0), (100.2, 70.3, 140.0, 99.0),
            (np.nan, 1.0, 5.0, 9.0), (1.0, 1.0, 30.0, 30.0), (3.0, 3.0, 40.0, 40.0), (33.0, 1.0, 47.5, 12.0)]
    labels = [0, 1, 2, 3, 0, 0, 99, 4, 5]
    ids = [7 + shift, 123456789, 3, 4, 10 ** 9, 5, 6, 8, 31]
    scores = [0.9, 0.5, 0.25, 0.75, 0.994, 0.1, 0.2, 0.3, 1.0]
    boxes = list(base)
    if W >= 260 and H >= 200:
        boxes += [(b[0] + 120.0, b[1] + 95.0, b[2] + 120.0, b[3] + 95.0) for b in base[:5]]
        labels += labels[:5]
        ids += [i + 100 for i in ids[:5]]
        scores += scores[:5]
    rows = make_rows(boxes, scores, labels, ids, d=len(boxes) + 3)
    cfg = dict(n_lines=2, lines=np.zeros((16, 4), f32), n_zones=1, nv=np.zeros(16, np.int32), verts=np.zeros((16, 16, 2), f32))
    cfg["lines"][0] = (5.0, 5.0, W - 6.0, H - 7.0)
    cfg["lines"][1] = (0.5, H - 16.5, W + 10.0, H - 16.5)
    poly = [(20.0, 15.0), (110.0, 20.0), (60.0, 45.0), (100.0, 85.0), (15.0, 75.0)]
    cfg["nv"][0] = len(poly)
    cfg["verts"][0, :len(poly)] = np.asarray(poly, f32)
    return rows, cfg
