"""Reference of the surface dewarping (include/demonet_hip.h, dn_warp) in numpy, in exact integers: the bilinear interpolation of the
mesh, the 1/32 positions, the four tested taps and the blend, per plane on the stored bytes, for all four formats (surfaces as the payload planes of
tests/compose_ref.py; the pitch is the caller's) and both border modes. Nothing here is fitted to device output. The keyword `mistake` makes the
classic wrong resamplers (tests only):

    nearest         the sample nearest to the position, no blend
    float           the position and the blend in float64, rounded half up at the end (grid_sample and a final rounding)
    no_round        q = P >> 7 and qc = (P2 >> 10) - 8: the positions truncated instead of rounded
    cosited         chroma sited on the even luma pixel (2 cxs, 2 cys) instead of the centre of its 2 x 2 block
    chroma_luma     chroma taps at the luma coordinates of the sample's first pixel, not halved
    swap_uv         U and V exchanged on the way out
    swap_border     constant and replicate border exchanged
"""
import numpy as np

import compose_ref as cr

MISTAKES = ("nearest", "float", "no_round", "cosited", "chroma_luma", "swap_uv", "swap_border")
YUV = cr.YUV
CELL = 8


def corner_points(mesh, x, y):
    """A, B, C, D [h, w, 2] int64 of the pixels (x [w], y [h]) of the rectangle"""
    m = np.asarray(mesh, np.int64)
    cx, cy = (x >> 3)[None, :], (y >> 3)[:, None]
    return m[cy, cx], m[cy, cx + 1], m[cy + 1, cx], m[cy + 1, cx + 1]


def luma_positions(mesh, dw, dh, mistake=None):
    """(q [dh, dw, 2] in 1/32 pixel, P in 1/4096)"""
    x, y = np.arange(dw, dtype=np.int64), np.arange(dh, dtype=np.int64)
    A, B, C, D = corner_points(mesh, x, y)
    i, j = (x & 7)[None, :, None], (y & 7)[:, None, None]
    P = (8 - j) * ((8 - i) * A + i * B) + j * ((8 - i) * C + i * D)
    assert np.abs(P).max() < 1 << 27
    return ((P >> 7) if mistake == "no_round" else ((P + 64) >> 7)), P


def chroma_positions(mesh, dw, dh, mistake=None):
    """(qc [ceil(dh / 2), ceil(dw / 2), 2] in 1/32 chroma sample, the position in chroma samples as float64)"""
    x, y = 2 * np.arange((dw + 1) // 2, dtype=np.int64), 2 * np.arange((dh + 1) // 2, dtype=np.int64)
    A, B, C, D = corner_points(mesh, x, y)
    one = 0 if mistake == "cosited" else 1
    i, j = (2 * (x & 7) + one)[None, :, None], (2 * (y & 7) + one)[:, None, None]
    P = (16 - j) * ((16 - i) * A + i * B) + j * ((16 - i) * C + i * D)
    assert np.abs(P).max() < 1 << 29
    if mistake == "chroma_luma":
        return (P + 256) >> 9, P / 16384.0                    # the luma position of the sample, in 1/32, used as a chroma coordinate
    shift = 0 if mistake == "cosited" else 8                 # co-sited: chroma = luma / 2 without the quarter sample
    q = ((P >> 10) if mistake == "no_round" else ((P + 512) >> 10)) - shift
    return q, P / 32768.0 - shift / 32.0


def tap(p, x, y, replicate, border):
    """plane samples at integer coordinates with the border rule, int64"""
    H, W = p.shape
    xc, yc = np.clip(x, 0, W - 1), np.clip(y, 0, H - 1)
    v = p[yc, xc]
    return v if replicate else np.where((x == xc) & (y == yc), v, border)


def sample(p, q, replicate, border, mistake=None, real=None):
    """one plane [H, W] through positions q [h, w, 2] in 1/32 sample: int64 [h, w]"""
    p = np.asarray(p, np.int64)
    if mistake == "swap_border":
        replicate = not replicate
    if mistake == "nearest":
        r = (q + 16) >> 5
        return tap(p, r[..., 0], r[..., 1], replicate, border)
    if mistake == "float":
        x0, y0 = np.floor(real[..., 0]).astype(np.int64), np.floor(real[..., 1]).astype(np.int64)
        fx, fy = real[..., 0] - x0, real[..., 1] - y0
        t = [tap(p, x0 + a, y0 + b, replicate, border).astype(np.float64) for b in (0, 1) for a in (0, 1)]
        return np.floor((1 - fy) * ((1 - fx) * t[0] + fx * t[1]) + fy * ((1 - fx) * t[2] + fx * t[3]) + 0.5).astype(np.int64)
    x0, fx, y0, fy = q[..., 0] >> 5, q[..., 0] & 31, q[..., 1] >> 5, q[..., 1] & 31
    t = [tap(p, x0 + a, y0 + b, replicate, border) for b in (0, 1) for a in (0, 1)]
    return ((32 - fx) * (32 - fy) * t[0] + fx * (32 - fy) * t[1] + (32 - fx) * fy * t[2] + fx * fy * t[3] + 512) >> 10


def warp(src_planes, dst_planes, items, fmt, mistake=None):
    """The destinations after dn_warp. src_planes / dst_planes: per surface the list of payload planes of format fmt; items: (src, dst, mesh, (x0, y0),
    border) with mesh an int [mh, mw, 2] array for a rectangle of (8 (mw - 1), 8 (mh - 1)) or fewer pixels -- or (src, dst, mesh, (x0, y0), border,
    (dw, dh)) --, border "replicate" or three bytes in the surface's logical order, (Y, U, V) or (R, G, B). Returns new payload planes per
    destination surface."""
    sc = [cr.channels(fmt, p) for p in src_planes]
    out = [[np.array(c, np.int64) for c in cr.channels(fmt, p)] for p in dst_planes]
    for it in items:
        s, d, mesh, (x0, y0), border = it[:5]
        mesh = np.asarray(mesh)
        dw, dh = it[5] if len(it) > 5 else (None, None)
        assert dw is not None, "pass the rectangle's size"
        assert mesh.shape == ((dh + 7) // 8 + 1, (dw + 7) // 8 + 1, 2) and np.abs(mesh.astype(np.int64)).max() <= (1 << 21) - 1
        rep = border == "replicate"
        b = (0, 0, 0) if rep else border
        q, P = luma_positions(mesh, dw, dh, mistake)
        if fmt in YUV:
            out[d][0][y0:y0 + dh, x0:x0 + dw] = sample(sc[s][0], q, rep, b[0], mistake, P / 4096.0)
            qc, real = chroma_positions(mesh, dw, dh, mistake)
            ey, ex, eh, ew = y0 // 2, x0 // 2, (dh + 1) // 2, (dw + 1) // 2
            for k in (1, 2):
                out[d][3 - k if mistake == "swap_uv" else k][ey:ey + eh, ex:ex + ew] = sample(sc[s][k], qc, rep, b[k], mistake, real)
        else:
            for k in range(3):
                out[d][k][y0:y0 + dh, x0:x0 + dw] = sample(sc[s][k], q, rep, b[k], mistake, P / 4096.0)
    return [cr.planes_of(fmt, c) for c in out]


def applies(mistake, fmt):
    """whether a mistake can show on this format: the chroma mistakes need chroma planes"""
    return fmt in YUV or mistake not in ("cosited", "chroma_luma", "swap_uv")


def ref_items(items, fmt="nv12", matrix="bt709", full=False):
    """warp.Item objects -> the tuples warp() takes: the border colour converted as the Warper converts it"""
    from demonet_amd.osd import to_surface
    out = []
    for it in items:
        border = it.border if it.border == "replicate" else to_surface(tuple(it.border), fmt, matrix, full)
        out.append((it.src, it.dst, it.mesh.points, tuple(it.dst_origin), border, (it.mesh.size[1], it.mesh.size[0])))
    return out


noise_planes = cr.noise_planes


# ---------------------------------------------------------------------------------------------------------------- scenes
SRC_SIZES = [(80, 96), (45, 67)]             # (height, width): one even, one odd
DST_SIZES = [(200, 240), (57, 73)]           # one even, one odd


def _crop(x0, y0, scale=1.0):
    """the map of a (magnified) crop at (x0, y0): half-pixel centres"""
    return lambda x, y: (x0 + (x + 0.5) / scale - 0.5, y0 + (y + 0.5) / scale - 0.5)


def mixed_items():
    """The mixed scene over sources of SRC_SIZES and destinations of DST_SIZES, legal for every format (even origins), as warp.Item objects.
    Destination 0: an identity copy of the odd source; a half-pixel shift of 33 x 17 that ends at the odd column 101 beside a neighbour at 102; a
    quarter turn; a 3 x magnification (a tile's footprint is 12 x 12 samples: staged in LDS); a 120 degree fisheye view whose corners leave the image circle and
    the frame, once with a constant border and once -- the SAME mesh -- with replicate; a 6:1 minification of a whole frame and a view across the
    rim (a tile's footprint touches the frame's edge or leaves it: gathered); a 1 x 1 rectangle; a mesh at +-(2^21 - 1): all border; uncovered payload remains.
    The odd destination 1 holds four items: a bilinear downscale that ends at the odd column 35 beside a neighbour at 36, a crop that ends at the
    frame's odd last column, a mirrored half turn that ends at its odd last row, an undistortion with a replicate border."""
    from demonet_amd import warp as W
    s0, s1 = SRC_SIZES
    big = (1 << 21) - 1
    half = W.Mesh((np.stack(np.meshgrid(np.arange(6) * 512 + 32 + 64 * 20, np.arange(4) * 512 + 32 + 64 * 11), -1)).astype(np.int32), (17, 33))
    view = W.fisheye_view(s0, (56, 72), fov=120, pan=30, tilt=35)
    far = W.Mesh(np.broadcast_to(np.array([big, -big], np.int32), (3, 4, 2)).copy(), (12, 20))
    K = np.array([[60.0, 0, 33.0], [0, 60.0, 22.0], [0, 0, 1]])
    newK = np.array([[34.0, 0, 18.0], [0, 34.0, 14.0], [0, 0, 1]])
    return [
        W.Item(1, 0, W.identity(s1), (0, 0)),
        W.Item(0, 0, half, (68, 0), (1, 2, 3)),
        W.Item(1, 0, W.rotate(s1, 1), (102, 0)),
        W.Item(0, 0, W.mesh_from_function((54, 72), _crop(20, 30, 3.0)), (148, 0)),
        W.Item(0, 0, view, (0, 68), (200, 30, 90)),
        W.Item(0, 0, view, (74, 68), "replicate"),
        W.Item(0, 0, W.resize(s0, (13, 16)), (148, 68)),
        W.Item(0, 0, W.fisheye_view(s0, (24, 40), fov=100, pan=200, tilt=80), (166, 68), (10, 250, 40)),
        W.Item(1, 0, W.mesh_from_function((1, 1), _crop(40, 20)), (210, 68), "replicate"),
        W.Item(0, 0, far, (148, 100), (9, 200, 77)),
        W.Item(0, 1, W.resize(s0, (27, 35)), (0, 0)),
        W.Item(1, 1, W.mesh_from_function((27, 37), _crop(12, 10)), (36, 0)),
        W.Item(0, 1, W.mesh_from_function((29, 35), lambda x, y: W.rotate_map((29, 35), 2, True)(x, y)), (0, 28)),
        W.Item(1, 1, W.undistort(K, (-0.35, 0.12, 0.01, -0.02, 0.0), (29, 37), newK), (36, 28), "replicate"),
    ]


def second_items():
    """other items, other meshes and fewer of them: what the captured call is replayed on"""
    from demonet_amd import warp as W
    s0, s1 = SRC_SIZES
    return [
        W.Item(0, 0, W.fisheye_panorama(s0, (40, 200), inner=15), (2, 4), (90, 90, 90)),
        W.Item(1, 0, W.rotate(s1, 3, True), (10, 50), "replicate"),
        W.Item(1, 1, W.resize(s1, (51, 70)), (2, 6)),
        W.Item(0, 0, W.fisheye_view(s0, (61, 83), fov=70, pan=-60, tilt=50, roll=20, lens="equisolid"), (60, 50), (0, 0, 255)),
        W.Item(0, 0, W.homography([[0.9, 0.2, 3.0], [-0.1, 1.1, 5.0], [0.001, 0.002, 1.0]], (33, 47)), (150, 120), (255, 255, 255)),
    ]


def many_items(side=48, cell=34):
    """side x side items of 33 x 33 destination pixels (four tiles each, three of them ragged) on a grid of `cell` pixels in ONE destination of
    (side cell) x (side cell), through six shared meshes, sources alternating, borders alternating. With side = 48 these are 2304 items and 9216
    tiles: more than two tiles per workgroup of the kernel's grid, and runs of tiles that cross item boundaries."""
    from demonet_amd import warp as W
    size = (33, 33)
    meshes = [W.mesh_from_function(size, _crop(6, 4)), W.mesh_from_function(size, _crop(10.5, 3.25)), W.mesh_from_function(size, _crop(20, 9, 2.0)),
              W.mesh_from_function(size, lambda x, y: W.rotate_map((33, 33), 1)(x, y)), W.resize((45, 67), size),
              W.fisheye_view((45, 67), size, fov=110, pan=45, tilt=40)]
    return [W.Item(n & 1, 0, meshes[n % 6], ((n % side) * cell, (n // side) * cell), "replicate" if n % 3 == 0 else (n % 256, 7, 200)) for n in range(side * side)]


STAGE_LIMIT = 112            # csrc/warp.hip, WP_ST_W = WP_ST_H: the widest and the tallest source footprint of a tile that is staged in LDS
LIMIT_SRC = (130, 160)


def limit_items():
    """One-tile items over a source of LIMIT_SRC whose footprints are exactly STAGE_LIMIT samples wide (3 .. 114) or tall (5 .. 116), and one sample
    more: the last tiles the kernel stages and the first it gathers, in both directions; destination: one surface of 72 x 72."""
    from demonet_amd import warp as W
    n = STAGE_LIMIT - 2         # the span of the control points: the box adds the right tap and the rounding's half step
    return [W.Item(0, 0, W.mesh_from_function((32, 32), lambda x, y: (3 + x * (n / 32), 9 + y)), (0, 0), (7, 7, 7)),
            W.Item(0, 0, W.mesh_from_function((32, 32), lambda x, y: (3 + x * ((n + 1) / 32), 9 + y)), (34, 0), (7, 7, 7)),
            W.Item(0, 0, W.mesh_from_function((32, 32), lambda x, y: (11 + x * 1.5, 5 + y * (n / 32))), (0, 34), "replicate"),
            W.Item(0, 0, W.mesh_from_function((32, 32), lambda x, y: (11 + x * 1.5, 5 + y * ((n + 1) / 32))), (34, 34), "replicate")]
