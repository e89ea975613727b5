"""Surface dewarping on the device: fisheye views and panoramas, lens undistortion, homographies, quarter turns, mirrors and bilinear
scaling -- the first stage of the video path for cameras that are not rectilinear and upright.

A `Warper` fills rectangles of the surfaces of one `FrameBatch` from the surfaces of another through coordinate meshes: a `Mesh` holds, for every
eighth pixel of a destination rectangle, the source position in 1/64 pixel; the kernel interpolates the positions between the points and blends the
four source samples around each, all in the integer arithmetic the header fixes (include/demonet_hip.h, dn_warp). Both batches have the same format
and colour space: the remap works on the stored bytes, colour conversion is the Compositor's job. One launch, no float copy of a frame, no workspace,
nothing visits the host, and a captured graph follows new surfaces, new items, new meshes and a new item count.

    fisheye = FrameBatch(16, "cuda:0", format="nv12").set(decoder_surfaces)                    # 2880 x 2880 each
    views = FrameBatch(64, "cuda:0", format="nv12").set(view_surfaces)                         # 960 x 720 each
    meshes = [fisheye_view((2880, 2880), (720, 960), fov=90, pan=90 * k, tilt=50) for k in range(4)]
    warp = Warper(64, "cuda:0").set([Item(i // 4, i, meshes[i % 4]) for i in range(64)], fisheye, views)
    warp(fisheye, views)
    outs = model.track_frames(views, tracker, warp=warp, source=fisheye)                       # ... or as the step's first act
    centre_in_fisheye = meshes[0].source_points(box_centres_in_view)                           # host: a view position back into the fisheye

The meshes are built on the host in float64 (`mesh_from_function` and the named builders below); `mesh_error` measures what the 8-pixel cell costs
against the exact function. The library trusts the item table as it trusts a region table, so `set` validates every item on the host first and
remembers both batches' sizes; a call refuses batches whose sizes, formats or colour codes have changed since. There is no CPU fallback.
"""
import ctypes as C
import math
from dataclasses import dataclass
from typing import Callable, List, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .compose import BUCKET, MAX_ITEMS, MAX_SIDE, TILE, _chroma, _ints, _overlap
from .frames import FrameBatch
from .osd import to_surface

CELL = _lib.DN_WARP_CELL
COORD_MAX = (1 << 21) - 1        # of a mesh value, in 1/64 pixel
LENSES = ("equidistant", "equisolid", "stereographic", "orthographic")
_YUV = ("nv12", "i420")


def mesh_shape(height: int, width: int) -> Tuple[int, int]:
    """(mh, mw): the control points of a destination rectangle of width x height pixels"""
    return (height + CELL - 1) // CELL + 1, (width + CELL - 1) // CELL + 1


class Mesh:
    """The coordinate mesh of one destination rectangle. points: int32 [mh, mw, 2], point (cy, cx) = (X, Y): the source position of rectangle pixel
    (8 cx, 8 cy) in 1/64 source pixel (pixel indices: an integer is a pixel centre), |X|, |Y| <= 2^21 - 1; size: the rectangle's (height, width).
    Immutable once built: a Warper de-duplicates meshes by identity."""

    def __init__(self, points, size):
        if not _ints(tuple(size), 2) or size[0] < 1 or size[1] < 1 or size[0] > MAX_SIDE or size[1] > MAX_SIDE:
            raise ValueError("Mesh: size must be (height, width) ints in 1 .. {}, got {!r}".format(MAX_SIDE, size))
        self.size = (int(size[0]), int(size[1]))
        p = np.asarray(points)
        want = mesh_shape(*self.size) + (2,)
        if p.dtype != np.int32 or p.shape != want:
            raise ValueError("Mesh: a destination of {} x {} (width x height) takes int32 points of shape {}, got {} {}".format(
                self.size[1], self.size[0], want, p.dtype, p.shape))
        if p.size and int(np.abs(p.astype(np.int64)).max()) > COORD_MAX:
            raise ValueError("Mesh: a point lies outside +-(2^21 - 1) units of 1/64 pixel (largest magnitude {})".format(int(np.abs(p.astype(np.int64)).max())))
        self.points = np.ascontiguousarray(p)
        self.points.setflags(write=False)

    def positions(self, xy) -> np.ndarray:
        """The mesh-interpolated source positions, float64 [..., 2], of the INTEGER destination pixels xy [..., 2]: exactly the header's P / 4096."""
        xy = np.asarray(xy)
        x, y = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
        m = self.points.astype(np.int64)
        cx, i, cy, j = x >> 3, x & 7, y >> 3, y & 7
        A, B, Cc, D = m[cy, cx], m[cy, cx + 1], m[cy + 1, cx], m[cy + 1, cx + 1]
        i, j = i[..., None], j[..., None]
        P = (8 - j) * ((8 - i) * A + i * B) + j * ((8 - i) * Cc + i * D)
        return P / 4096.0

    def source_points(self, xy) -> np.ndarray:
        """Destination positions xy [..., 2] (float, pixel indices, anywhere inside the rectangle) -> source positions, float64 [..., 2], through the
        mesh as the kernel interpolates it. Host work: carries a box centre from a view back into the fisheye."""
        xy = np.asarray(xy, np.float64)
        mh, mw = self.points.shape[:2]
        u, v = xy[..., 0] / CELL, xy[..., 1] / CELL
        cx = np.clip(np.floor(u), 0, mw - 2).astype(np.int64)
        cy = np.clip(np.floor(v), 0, mh - 2).astype(np.int64)
        s, t = (u - cx)[..., None], (v - cy)[..., None]
        m = self.points.astype(np.float64)
        return ((1 - t) * ((1 - s) * m[cy, cx] + s * m[cy, cx + 1]) + t * ((1 - s) * m[cy + 1, cx] + s * m[cy + 1, cx + 1])) / 64.0


def mesh_from_function(dst_size, fn: Callable) -> Mesh:
    """The mesh of fn over a destination of dst_size = (height, width): fn(x, y) takes float64 arrays of destination pixel positions and returns the
    source positions (sx, sy); it is evaluated at the control points (8 cx, 8 cy), those past the rectangle's end included, and rounded by
    floor(64 v + 0.5). Values that are not finite or leave +-(2^21 - 1) / 64 pixels are clamped there (far outside every frame: border)."""
    h, w = int(dst_size[0]), int(dst_size[1])
    mh, mw = mesh_shape(h, w)
    x, y = np.meshgrid(np.arange(mw, dtype=np.float64) * CELL, np.arange(mh, dtype=np.float64) * CELL)
    sx, sy = fn(x, y)
    pts = np.stack([np.broadcast_to(np.asarray(sx, np.float64), x.shape), np.broadcast_to(np.asarray(sy, np.float64), x.shape)], -1)
    pts = np.floor(64.0 * np.nan_to_num(pts, nan=float(COORD_MAX), posinf=float(COORD_MAX), neginf=-float(COORD_MAX)) + 0.5)
    return Mesh(np.clip(pts, -COORD_MAX, COORD_MAX).astype(np.int32), (h, w))


def mesh_error(mesh: Mesh, fn: Callable) -> float:
    """The largest distance, in source pixels, between the mesh-interpolated luma position and fn over all destination pixels: what the 8-pixel
    cell and the 1/64 rounding of the points cost against the exact map."""
    h, w = mesh.size
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    got = mesh.positions(np.stack([x, y], -1))
    sx, sy = fn(x.astype(np.float64), y.astype(np.float64))
    return float(np.hypot(got[..., 0] - sx, got[..., 1] - sy).max())


# ---------------------------------------------------------------------------------------------------------------- the maps (float64, host)
def identity_map():
    return lambda x, y: (x, y)


def resize_map(src_size, dst_size):
    """bilinear scale with half-pixel centres: sx = (x + 0.5) SW / DW - 0.5"""
    (sh, sw), (dh, dw) = src_size, dst_size
    return lambda x, y: ((x + 0.5) * (sw / dw) - 0.5, (y + 0.5) * (sh / dh) - 0.5)


def rotate_map(src_size, quarter_turns: int, mirror: bool = False):
    """out = np.rot90(np.fliplr(src) if mirror else src, quarter_turns): counter-clockwise quarter turns of the (mirrored) source"""
    sh, sw = src_size
    k = quarter_turns % 4

    def fn(x, y):
        if k == 0:
            sx, sy = x, y
        elif k == 1:
            sx, sy = (sw - 1) - y, x
        elif k == 2:
            sx, sy = (sw - 1) - x, (sh - 1) - y
        else:
            sx, sy = y, (sh - 1) - x
        return ((sw - 1) - sx if mirror else sx), sy
    return fn


def homography_map(H):
    """(sx, sy, s) = H (x, y, 1): H maps DESTINATION pixel positions to source positions (the inverse-map convention)"""
    H = np.asarray(H, np.float64)
    if H.shape != (3, 3):
        raise ValueError("homography: H must be 3 x 3, got {}".format(H.shape))

    def fn(x, y):
        s = H[2, 0] * x + H[2, 1] * y + H[2, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            return (H[0, 0] * x + H[0, 1] * y + H[0, 2]) / s, (H[1, 0] * x + H[1, 1] * y + H[1, 2]) / s
    return fn


def undistort_map(K, dist, new_K=None):
    """Brown-Conrady with dist = (k1, k2, p1, p2, k3), the formulas of initUndistortRectifyMap without a rectification: destination pixel (u, v)
    of a pinhole camera new_K (default K) -> the pixel of the distorted camera K."""
    K = np.asarray(K, np.float64)
    N = K if new_K is None else np.asarray(new_K, np.float64)
    if K.shape != (3, 3) or N.shape != (3, 3):
        raise ValueError("undistort: K and new_K must be 3 x 3")
    d = [float(v) for v in dist] + [0.0] * (5 - len(dist))
    if len(d) != 5:
        raise ValueError("undistort: dist takes up to five coefficients (k1, k2, p1, p2, k3), got {}".format(len(dist)))
    k1, k2, p1, p2, k3 = d

    def fn(u, v):
        x, y = (u - N[0, 2]) / N[0, 0], (v - N[1, 2]) / N[1, 1]
        r2 = x * x + y * y
        radial = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        return K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]
    return fn


def _lens_radius(theta, lens: str, lens_fov: float, radius: float):
    """the image radius of a ray at angle theta from the optical axis; the rim of the image circle (theta = lens_fov / 2) lies at `radius`"""
    if lens not in LENSES:
        raise ValueError("lens must be one of {}, got {!r}".format(LENSES, lens))
    half = math.radians(lens_fov) / 2
    if lens == "equidistant":
        return radius * theta / half
    if lens == "equisolid":
        return radius * np.sin(theta / 2) / math.sin(half / 2)
    if lens == "stereographic":
        with np.errstate(divide="ignore", invalid="ignore"):
            return radius * np.tan(np.minimum(theta, math.pi) / 2) / math.tan(half / 2)
    return np.where(theta <= math.pi / 2, radius * np.sin(theta) / math.sin(min(half, math.pi / 2)), np.inf)     # orthographic: nothing behind 90 degrees


def _circle(src_size, center, radius):
    sh, sw = src_size
    cx, cy = ((sw - 1) / 2.0, (sh - 1) / 2.0) if center is None else (float(center[0]), float(center[1]))
    return cx, cy, (min(sw, sh) / 2.0 if radius is None else float(radius))


def fisheye_view_map(src_size, dst_size, fov, pan, tilt, roll=0.0, lens="equidistant", lens_fov=180.0, center=None, radius=None):
    """A virtual pan-tilt-zoom camera inside a fisheye image (angles in degrees). The view is a pinhole camera of dst_size with a horizontal field of
    view `fov`; its axis leaves the lens axis by `tilt` towards the image azimuth `pan` (measured from +x towards +y), its up direction points away
    from the lens axis -- the horizon is up for a ceiling mount -- and `roll` turns it about its own axis. The image circle has `center` (x, y;
    default: the frame's centre) and `radius` (default: half the shorter side) at lens_fov / 2."""
    dh, dw = dst_size
    cx, cy, R = _circle(src_size, center, radius)
    if not 0 < fov < 180:
        raise ValueError("fisheye_view: fov takes 0 < fov < 180 degrees, got {!r}".format(fov))
    f = (dw / 2.0) / math.tan(math.radians(fov) / 2)
    p, t, r = math.radians(pan), math.radians(tilt), math.radians(roll)
    axis = np.array([math.sin(t) * math.cos(p), math.sin(t) * math.sin(p), math.cos(t)])
    right = np.array([-math.sin(p), math.cos(p), 0.0])
    down = -np.array([math.cos(t) * math.cos(p), math.cos(t) * math.sin(p), -math.sin(t)])

    def fn(x, y):
        u0, v0 = x - (dw - 1) / 2.0, y - (dh - 1) / 2.0
        u, v = math.cos(r) * u0 - math.sin(r) * v0, math.sin(r) * u0 + math.cos(r) * v0
        wx, wy, wz = (u * right[k] + v * down[k] + f * axis[k] for k in range(3))
        rho = np.hypot(wx, wy)
        rad = _lens_radius(np.arctan2(rho, wz), lens, lens_fov, R)
        with np.errstate(divide="ignore", invalid="ignore"):
            ux, uy = np.where(rho > 0, wx / rho, 0.0), np.where(rho > 0, wy / rho, 0.0)
        return cx + np.where(rho > 0, rad * ux, 0.0), cy + np.where(rho > 0, rad * uy, 0.0)
    return fn


def fisheye_panorama_map(src_size, dst_size, lens="equidistant", lens_fov=180.0, center=None, radius=None, inner=20.0, outer=None, pan=0.0):
    """The cylindrical unroll of a ceiling-mounted fisheye (angles in degrees): column x is the azimuth pan + 360 (x + 0.5) / width, row y the
    angle from the lens axis, from `outer` (default lens_fov / 2: the rim, the horizon) at the top to `inner` at the bottom, equally spaced."""
    dh, dw = dst_size
    cx, cy, R = _circle(src_size, center, radius)
    outer = lens_fov / 2.0 if outer is None else outer

    def fn(x, y):
        phi = math.radians(pan) + 2 * math.pi * (x + 0.5) / dw
        theta = np.radians(outer + (inner - outer) * (y + 0.5) / dh)
        rad = _lens_radius(theta, lens, lens_fov, R)
        return cx + rad * np.cos(phi), cy + rad * np.sin(phi)
    return fn


# ---------------------------------------------------------------------------------------------------------------- the builders
def identity(size) -> Mesh:
    """a byte copy of every plane"""
    return mesh_from_function(size, identity_map())


def resize(src_size, dst_size) -> Mesh:
    """bilinear scale of a whole frame of src_size to dst_size, half-pixel centres (minify strongly with the Compositor's area filter instead)"""
    return mesh_from_function(dst_size, resize_map(src_size, dst_size))


def rotate(src_size, quarter_turns: int, mirror: bool = False) -> Mesh:
    """np.rot90(np.fliplr(src) if mirror else src, quarter_turns); the destination has the source's size, sides swapped for an odd turn count"""
    sh, sw = int(src_size[0]), int(src_size[1])
    return mesh_from_function((sw, sh) if quarter_turns % 2 else (sh, sw), rotate_map((sh, sw), quarter_turns, mirror))


def homography(H, dst_size) -> Mesh:
    """a projective map (bird's-eye views): H takes destination pixel positions to source positions"""
    return mesh_from_function(dst_size, homography_map(H))


def undistort(K, dist, dst_size, new_K=None) -> Mesh:
    return mesh_from_function(dst_size, undistort_map(K, dist, new_K))


def fisheye_view(src_size, dst_size, fov, pan, tilt, roll=0.0, lens="equidistant", lens_fov=180.0, center=None, radius=None) -> Mesh:
    return mesh_from_function(dst_size, fisheye_view_map(src_size, dst_size, fov, pan, tilt, roll, lens, lens_fov, center, radius))


def fisheye_panorama(src_size, dst_size, lens="equidistant", lens_fov=180.0, center=None, radius=None, inner=20.0, outer=None, pan=0.0) -> Mesh:
    return mesh_from_function(dst_size, fisheye_panorama_map(src_size, dst_size, lens, lens_fov, center, radius, inner, outer, pan))


for _b, _m in ((undistort, undistort_map), (fisheye_view, fisheye_view_map), (fisheye_panorama, fisheye_panorama_map)):
    _b.__doc__ = "The Mesh of " + _m.__name__ + " over a destination of dst_size = (height, width). " + _m.__doc__


# ---------------------------------------------------------------------------------------------------------------- items and the table
@dataclass(frozen=True)
class Item:
    """One remap: the rectangle of mesh.size at dst_origin = (x0, y0) of frame `dst` of the destination batch, from frame `src` of the source batch
    through `mesh`. border: (R, G, B), the colour of taps outside the source (converted to the surfaces' space), or "replicate": clamp them."""
    src: int
    dst: int
    mesh: Mesh
    dst_origin: Tuple[int, int] = (0, 0)
    border: Union[Tuple[int, int, int], str] = (0, 0, 0)


def item_records(items: Sequence, src_sizes, dst_sizes, format: str, matrix: str, full_range: bool, capacity: int):
    """The validated table of `items` -- Item objects or (src, dst, mesh[, dst_origin[, border]]) tuples -- against src_sizes[src] and
    dst_sizes[dst] = (height, width): (the bytes of the dn_warp_header and `capacity` dn_warp_item records, all meshes as one int32 [M, 2] array
    with shared meshes stored once, the normalised (src, dst, dst_rect, mesh0, border) list, the tile count). ValueError naming the item otherwise.
    Host work only."""
    if isinstance(items, torch.Tensor) or not isinstance(items, (list, tuple)):
        raise ValueError("Warper: expected a list of items, got {}".format(type(items).__name__))
    if len(items) > capacity:
        raise ValueError("Warper: {} items, the capacity is {}".format(len(items), capacity))
    src_sizes = [(int(h), int(w)) for h, w in src_sizes]
    dst_sizes = [(int(h), int(w)) for h, w in dst_sizes]
    yuv = format in _YUV
    head = _lib.WarpHeader()
    rec = (_lib.WarpItem * capacity)()
    norm, tiles, points = [], 0, 0
    buckets, first, meshes = {}, {}, []
    for i, it in enumerate(items):
        if isinstance(it, (tuple, list)) and 3 <= len(it) <= 5:
            it = Item(*it)
        if not isinstance(it, Item):
            raise ValueError("item {}: expected an Item or (src, dst, mesh[, dst_origin[, border]]), got {!r}".format(i, it))
        if not _ints((it.src, it.dst), 2):
            raise ValueError("item {}: src and dst must be ints, got {!r}, {!r}".format(i, it.src, it.dst))
        if it.src < 0 or it.src >= len(src_sizes):
            raise ValueError("item {}: source index {} out of range ({} frames)".format(i, it.src, len(src_sizes)))
        if it.dst < 0 or it.dst >= len(dst_sizes):
            raise ValueError("item {}: destination index {} out of range ({} frames)".format(i, it.dst, len(dst_sizes)))
        if not isinstance(it.mesh, Mesh):
            raise ValueError("item {}: mesh must be a Mesh, got {}".format(i, type(it.mesh).__name__))
        if not _ints(it.dst_origin, 2):
            raise ValueError("item {}: dst_origin must be two ints (x0, y0), got {!r}".format(i, it.dst_origin))
        dh, dw = it.mesh.size
        x0, y0 = it.dst_origin
        m = it.mesh.points
        if m.dtype != np.int32 or m.shape != mesh_shape(dh, dw) + (2,):
            raise ValueError("item {}: the mesh of a {} x {} rectangle takes int32 points of shape {}, got {} {}".format(
                i, dw, dh, mesh_shape(dh, dw) + (2,), m.dtype, m.shape))
        if id(it.mesh) not in first and int(np.abs(m.astype(np.int64)).max()) > COORD_MAX:
            raise ValueError("item {}: a mesh value lies outside +-(2^21 - 1)".format(i))
        DH, DW = dst_sizes[it.dst]
        if dw < 1 or dh < 1 or dw > MAX_SIDE or dh > MAX_SIDE:
            raise ValueError("item {}: the destination rectangle is {} x {}, a side takes 1 .. {}".format(i, dw, dh, MAX_SIDE))
        if x0 < 0 or y0 < 0 or x0 + dw > DW or y0 + dh > DH:
            raise ValueError("item {}: the destination rectangle x {} .. {}, y {} .. {} lies outside its frame of {} x {} (width x height)".format(
                i, x0, x0 + dw, y0, y0 + dh, DW, DH))
        if yuv and (x0 % 2 or y0 % 2):
            raise ValueError("item {}: odd origin ({}, {}) of the destination rectangle: a 4:2:0 surface takes even x0 and y0".format(i, x0, y0))
        if it.border == "replicate":
            flags, border = _lib.DN_WARP_BORDER["replicate"], (0, 0, 0)
        else:
            b = it.border
            if not isinstance(b, (tuple, list)) or len(b) != 3 or not all(isinstance(v, int) and not isinstance(v, bool) and 0 <= v <= 255 for v in b):
                raise ValueError("item {}: border must be three ints (R, G, B) in 0 .. 255 or \"replicate\", got {!r}".format(i, b))
            flags, border = _lib.DN_WARP_BORDER["constant"], to_surface(tuple(b), format, matrix, full_range)
            if format == "bgr24":
                border = border[::-1]                  # the record holds a packed pixel's bytes in memory order
        drect = (x0, y0, dw, dh)
        cells = [(it.dst, bx, by) for bx in range(x0 // BUCKET, (x0 + dw) // BUCKET + 1) for by in range(y0 // BUCKET, (y0 + dh) // BUCKET + 1)]
        for k, other in sorted({e for cell in cells for e in buckets.get(cell, ())}):
            if _overlap(drect, other) or (yuv and _overlap(_chroma(drect), _chroma(other))):
                raise ValueError("item {}: its destination rectangle {} overlaps item {}'s {} in destination {}{}".format(
                    i, drect, k, other, it.dst, "" if _overlap(drect, other) else " (their chroma samples do)"))
        for cell in cells:
            buckets.setdefault(cell, []).append((i, drect))
        if id(it.mesh) not in first:
            first[id(it.mesh)] = points
            meshes.append(m.reshape(-1, 2))
            points += m.shape[0] * m.shape[1]
            if points >= 2 ** 31:
                raise ValueError("item {}: the meshes have 2^31 or more points".format(i))
        r = rec[i]
        r.src, r.dst, r.dx0, r.dy0, r.dw, r.dh = it.src, it.dst, x0, y0, dw, dh
        r.mesh0, r.mesh_w, r.flags = first[id(it.mesh)], m.shape[1], flags
        r.border = border[0] | border[1] << 8 | border[2] << 16
        r.tile0 = tiles
        tiles += ((dw + TILE - 1) // TILE) * ((dh + TILE - 1) // TILE)
        if tiles >= 2 ** 31:
            raise ValueError("item {}: the items have 2^31 or more tiles of {} x {} pixels".format(i, TILE, TILE))
        norm.append((it.src, it.dst, drect, first[id(it.mesh)], "replicate" if flags else tuple(border)))
    head.n_items, head.n_tiles, head.n_points = len(norm), tiles, points
    mesh = np.concatenate(meshes) if meshes else np.zeros((0, 2), np.int32)
    return bytes(head) + bytes(rec), np.ascontiguousarray(mesh, np.int32), norm, tiles


def _spans(batch):
    """the [first byte, last byte + 1) address ranges of a batch's planes"""
    out = []
    for t in batch.planes:
        rows = t.shape[0]
        row_bytes = int(np.prod(t.shape[1:]))
        out.append((t.data_ptr(), t.data_ptr() + (rows - 1) * (t.stride(0) if rows > 1 else 0) + row_bytes))
    return out


def _shared(src_batch, dst_batch):
    """whether a plane of one batch overlaps a plane of the other in memory"""
    ev = sorted([(a, 0, b) for a, b in _spans(src_batch)] + [(a, 1, b) for a, b in _spans(dst_batch)])
    end = [0, 0]
    for a, which, b in ev:
        if a < end[1 - which]:
            return True
        end[which] = max(end[which], b)
    return False


def check_warp(what: str, warp, src_batch, dst_batch):
    """What every warp checks before the library is touched: the objects, one device, everything set, and that both batches have, AS THEY ARE NOW,
    the sizes, formats and colour codes the items were validated against."""
    if not isinstance(warp, Warper):
        raise ValueError("{}: expected a Warper, got {}".format(what, type(warp).__name__))
    for name, b in (("source", src_batch), ("destination", dst_batch)):
        if not isinstance(b, FrameBatch):
            raise ValueError("{}: the {} must be a FrameBatch, got {}".format(what, name, type(b).__name__))
        if b.device != warp.device:
            raise ValueError("{}: the {} FrameBatch is on {}, the warper on {}".format(what, name, b.device, warp.device))
        if b.table is None:
            raise ValueError("{}: the {} FrameBatch names no frames yet: call set() first".format(what, name))
    if src_batch is dst_batch:
        raise ValueError("{}: source and destination must be two batches (and must not share memory)".format(what))
    if warp.table is None:
        raise ValueError("{}: the warper holds no items yet: call set() first".format(what))
    for name, b, sizes in (("source", src_batch, warp.src_sizes), ("destination", dst_batch, warp.dst_sizes)):
        if list(b.sizes) != sizes:
            raise ValueError("{}: stale sizes: the items were validated against {} frames of {} (height, width), the batch now holds {}; "
                             "set() the warper again".format(what, name, sizes, list(b.sizes)))
        if (b.format_code, b.color_code) != warp.space:
            raise ValueError("{}: the items were validated for batches of format / colour code {}, the {} has {}; set() the warper "
                             "again".format(what, warp.space, name, (b.format_code, b.color_code)))


class Warper:
    """A table of at most `capacity` items on `device`; owns the dn_warp_header + dn_warp_item table and the mesh tensor in device memory. The table
    keeps its address for the life of the object; the mesh tensor holds `mesh_points` points (default: what the first set() needs) and keeps its
    address until a set() needs more, which allocates a larger one -- give mesh_points when a captured call must follow larger meshes later. A
    captured call replays on whatever set() put there last: other items, other meshes, another item count."""

    def __init__(self, capacity: int, device, mesh_points: int = None):
        if not isinstance(capacity, int) or isinstance(capacity, bool) or capacity < 1 or capacity > MAX_ITEMS:
            raise ValueError("Warper: capacity takes an int in 1 .. {}, got {!r}".format(MAX_ITEMS, capacity))
        if mesh_points is not None and (not isinstance(mesh_points, int) or isinstance(mesh_points, bool) or mesh_points < 1 or mesh_points >= 2 ** 31):
            raise ValueError("Warper: mesh_points takes a positive int below 2^31 or None, got {!r}".format(mesh_points))
        self.capacity = capacity
        self.mesh_points = mesh_points
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.table = None            # [16 + capacity * 48] uint8 on the device: allocated by the first set()
        self.mesh = None             # [mesh_points, 2] int32 on the device
        self.items: List[Tuple] = []        # (src, dst, dst_rect, mesh0, border) per item
        self.tiles = 0
        self.points = 0              # mesh points in use
        self.src_sizes = self.dst_sizes = None      # the (height, width) lists the items were validated against
        self.space = None            # (format code, colour code) of both batches
        self._host = None

    def set(self, items: Sequence, src_batch: FrameBatch, dst_batch: FrameBatch):
        """Name the items: Item objects or (src, dst, mesh[, dst_origin[, border]]) tuples. Validated against both batches as they are now: one
        format and one colour code (colour conversion is the Compositor's job: warp first, compose behind it); no memory shared between the
        batches; indices in range; every mesh of its rectangle's shape with values inside +-(2^21 - 1); rectangles inside their frames, sides
        1 .. 32768; even origins on a 4:2:0 surface; the rectangles of one destination surface disjoint, on 4:2:0 their chroma samples too.
        ValueError naming the item, before anything is changed. Table and meshes go up from pinned memory on the current stream; the host does not
        wait."""
        for name, b in (("source", src_batch), ("destination", dst_batch)):
            if not isinstance(b, FrameBatch):
                raise ValueError("Warper: the {} must be a FrameBatch, got {}".format(name, type(b).__name__))
            if b.device != self.device:
                raise ValueError("Warper: the {} FrameBatch is on {}, the warper on {}".format(name, b.device, self.device))
            if not b.sizes:
                raise ValueError("Warper: the {} FrameBatch names no frames yet: call set() first".format(name))
        if src_batch is dst_batch:
            raise ValueError("Warper: source and destination must be two batches (and must not share memory)")
        if (src_batch.format_code, src_batch.color_code) != (dst_batch.format_code, dst_batch.color_code):
            raise ValueError("Warper: the source is {} with colour code {}, the destination {} with {}: a warp keeps format and colour space -- "
                             "colour conversion is the Compositor's job (compose.Compositor), warp into a batch of the source's format first".format(
                                 src_batch.format, src_batch.color_code, dst_batch.format, dst_batch.color_code))
        if _shared(src_batch, dst_batch):
            raise ValueError("Warper: a destination surface shares memory with a source surface")
        raw, mesh, norm, tiles = item_records(items, src_batch.sizes, dst_batch.sizes, src_batch.format, src_batch.matrix, src_batch.full_range,
                                              self.capacity)
        if self.mesh_points is not None and len(mesh) > self.mesh_points:
            raise ValueError("Warper: the meshes have {} points, mesh_points is {}".format(len(mesh), self.mesh_points))
        if self.device.type != "cuda":
            raise RuntimeError("demonet_amd runs on an MI355X only (the warper must be on a cuda device); there is no CPU fallback path")
        host = torch.frombuffer(bytearray(raw), dtype=torch.uint8).pin_memory()
        if self.table is None:
            self.table = torch.empty(len(raw), dtype=torch.uint8, device=self.device)
        self.table.copy_(host, non_blocking=True)
        if self.mesh is None or len(mesh) > self.mesh.shape[0]:
            self.mesh = torch.zeros((max(self.mesh_points or 0, len(mesh), 1), 2), dtype=torch.int32, device=self.device)
        mesh_host = torch.from_numpy(mesh).pin_memory()
        if len(mesh):
            self.mesh[:len(mesh)].copy_(mesh_host, non_blocking=True)
        self._host = (host, mesh_host)
        self.items, self.tiles, self.points = norm, tiles, len(mesh)
        self.src_sizes, self.dst_sizes = list(src_batch.sizes), list(dst_batch.sizes)
        self.space = (src_batch.format_code, src_batch.color_code)
        return self

    def __call__(self, src_batch: FrameBatch, dst_batch: FrameBatch, stream=None):
        """Run the items: the source batch's surfaces into the destination batch's, which are written in place; bytes no item covers keep their
        value. One dn_warp call, enqueued on `stream` (default: the current stream); no host wait. Returns dst_batch. ValueError for unset or
        foreign batches and for sizes, formats or colour codes that changed since set()."""
        check_warp("Warper", self, src_batch, dst_batch)
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        if not hasattr(s, "cuda_stream"):
            s = torch.cuda.ExternalStream(int(s), device=self.device)
        p = C.c_void_p
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().dn_warp(p(src_batch.table.data_ptr()), p(dst_batch.table.data_ptr()), dst_batch.format_code, p(self.table.data_ptr()),
                                          self.capacity, p(self.mesh.data_ptr()), p(s.cuda_stream)), "dn_warp")
        return dst_batch


def check_warping(warp, source, batch, who: str):
    """The `warp=` / `source=` arguments of SSD.track_frames / track_frames_appearance / track_sliced_frames: both None, or a Warper that was set()
    for (source, batch) and the source FrameBatch. Checked before the step starts."""
    if warp is None and source is None:
        return
    if warp is None or source is None:
        raise ValueError("{}: warp= (a Warper) and source= (its source FrameBatch) go together".format(who))
    check_warp(who, warp, source, batch)


def warped(warp, source, batch):
    """The first act of a tracking step with a Warper: the step's frames are filled from the source's surfaces, in front of the forward."""
    if warp is not None:
        warp(source, batch)
