"""Surface dewarping without a GPU: the arithmetic of include/demonet_hip.h as tests/warp_ref.py restates it, against hand-worked cases
and seven wrong resamplers; the host-side mesh builders of demonet_amd/warp.py against direct evaluation; every refusal of Warper.set; the records
against the header."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import warp_ref as ref
from demonet_amd import _lib, warp
from demonet_amd.frames import FrameBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ["nv12", "i420", "rgb24", "bgr24"]


def _item(src, dst, mesh, origin=(0, 0), border=(0, 0, 0)):
    return (src, dst, mesh.points, origin, border, (mesh.size[1], mesh.size[0]))


def _one(fmt, src, mesh, border="replicate", mistake=None, seed=5):
    """one whole-destination item: the destination's payload planes"""
    h, w = mesh.size
    dst = ref.noise_planes(fmt, seed, h, w)
    return ref.warp([src], [dst], [_item(0, 0, mesh, (0, 0), border)], fmt, mistake)[0]


# ---------------------------------------------------------------------------------------------------------------- reference arithmetic
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("size", [(80, 96), (45, 67)])
def test_identity_is_a_byte_copy_of_every_plane(fmt, size):
    src = ref.noise_planes(fmt, 1, *size)
    got = _one(fmt, src, warp.identity(size), border=(9, 9, 9))
    assert all(np.array_equal(a, b) for a, b in zip(got, src))


def test_half_pixel_shift_by_hand():
    """X = 64 x + 32: every output is (a + b + 1) >> 1 of its two horizontal neighbours; the last column's right tap is outside"""
    img = np.array([[10, 20, 31, 255], [0, 1, 2, 3]], np.uint8)
    rgb = np.repeat(img, 3, axis=1)
    mesh = warp.mesh_from_function((2, 4), lambda x, y: (x + 0.5, y))
    assert mesh.points[0, :, 0].tolist() == [32, 544] and mesh.points[:, 0, 1].tolist() == [0, 512]
    want = lambda b: np.array([[15, 26, 143, (255 + b + 1) >> 1], [1, 2, 3, (3 + b + 1) >> 1]])      # noqa: E731
    got = _one("rgb24", [rgb], mesh, border=(77, 77, 77))[0]
    assert np.array_equal(got[:, 0::3], want(77)) and np.array_equal(got[:, 1::3], want(77))
    assert np.array_equal(_one("rgb24", [rgb], mesh, border="replicate")[0][:, 2::3], np.array([[15, 26, 143, 255], [1, 2, 3, 3]]))


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("turns", [0, 1, 2, 3])
def test_quarter_turns_and_mirrors_are_exact_permutations(turns, mirror):
    def turned(p):
        return np.rot90(np.fliplr(p) if mirror else p, turns)
    for fmt, size in (("nv12", (46, 68)), ("i420", (46, 68)), ("rgb24", (45, 67))):
        src = ref.noise_planes(fmt, 2, *size)
        got = _one(fmt, src, warp.rotate(size, turns, mirror), border=(1, 2, 3))
        sc = ref.cr.channels(fmt, src)
        want = ref.cr.planes_of(fmt, [turned(c) for c in sc])
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), (fmt, turns, mirror)


def test_resize_by_two_is_the_hand_written_bilinear():
    src = ref.noise_planes("i420", 3, 20, 30)[0].astype(np.int64)
    got = _one("i420", ref.noise_planes("i420", 3, 20, 30), warp.resize((20, 30), (40, 60)))[0]
    pad = np.pad(src, 1, mode="edge")
    want = np.zeros((40, 60), np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            # output (2 r + dy, 2 c + dx) sits a quarter sample from src (r, c) towards its neighbour on side (dy, dx)
            near = pad[1:-1, 1:-1]
            nx = pad[1:-1, 2 * dx:2 * dx + 30]
            ny = pad[2 * dy:2 * dy + 20, 1:-1]
            nxy = pad[2 * dy:2 * dy + 20, 2 * dx:2 * dx + 30]
            want[dy::2, dx::2] = (9 * near + 3 * nx + 3 * ny + nxy + 8) >> 4
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------- wrong resamplers
def _fisheye_scene():
    return (96, 96), warp.fisheye_view((96, 96), (24, 40), fov=110, pan=40, tilt=55), (200, 30, 90)


def _undistort_scene():
    K = np.array([[70.0, 0, 47.5], [0, 70.0, 39.5], [0, 0, 1]])
    newK = np.array([[30.0, 0, 27.5], [0, 30.0, 21.5], [0, 0, 1]])
    return (80, 96), warp.undistort(K, (-0.3, 0.1, 0.01, -0.02, 0.0), (44, 56), newK), (10, 250, 40)


@pytest.mark.parametrize("scene", [_fisheye_scene, _undistort_scene], ids=["fisheye", "undistort"])
@pytest.mark.parametrize("mistake", ref.MISTAKES)
def test_the_scenes_tell_every_wrong_resampler_from_the_right_one(scene, mistake):
    size, mesh, border = scene()
    from demonet_amd.osd import to_surface
    for fmt in ("nv12", "i420", "rgb24"):
        if not ref.applies(mistake, fmt):
            continue
        src = ref.noise_planes(fmt, 4, *size)
        b = to_surface(border, fmt, "bt709", False)
        right, wrong = _one(fmt, src, mesh, b), _one(fmt, src, mesh, b, mistake)
        assert any(not np.array_equal(a, c) for a, c in zip(right, wrong)), (fmt, mistake)
        if mistake == "swap_border":
            assert any(not np.array_equal(a, c) for a, c in zip(right, _one(fmt, src, mesh, "replicate"))), "the scene has no tap outside"


# ---------------------------------------------------------------------------------------------------------------- builders
def _points(mesh):
    mh, mw = mesh.points.shape[:2]
    return np.meshgrid(np.arange(mw) * 8.0, np.arange(mh) * 8.0)


def test_homography_and_undistort_against_direct_evaluation():
    H = np.array([[0.9, 0.2, 3.0], [-0.1, 1.1, 5.0], [0.001, 0.002, 1.0]])
    m = warp.homography(H, (33, 47))
    x, y = _points(m)
    v = np.einsum("ij,jhw->ihw", H, np.stack([x, y, np.ones_like(x)]))
    assert np.array_equal(m.points, np.floor(64 * np.stack([v[0] / v[2], v[1] / v[2]], -1) + 0.5).astype(np.int32))
    K = np.array([[60.0, 0, 33.0], [0, 50.0, 22.0], [0, 0, 1]])
    N = np.array([[40.0, 0, 20.0], [0, 45.0, 12.0], [0, 0, 1]])
    z = warp.undistort(K, (0, 0, 0, 0, 0), (29, 37), N)
    x, y = _points(z)
    want = np.stack([60.0 * (x - 20.0) / 40.0 + 33.0, 50.0 * (y - 12.0) / 45.0 + 22.0], -1)
    assert np.array_equal(z.points, np.floor(64 * want + 0.5).astype(np.int32))
    assert np.array_equal(warp.undistort(K, (0, 0, 0, 0, 0), (29, 37)).points, warp.identity((29, 37)).points)
    # one point with every coefficient, by hand: initUndistortRectifyMap's formulas
    k1, k2, p1, p2, k3 = d = (-0.3, 0.1, 0.01, -0.02, 0.05)
    sx, sy = warp.undistort_map(K, d, N)(np.array([30.0]), np.array([25.0]))
    xn, yn = (30.0 - 20.0) / 40.0, (25.0 - 12.0) / 45.0
    r2 = xn * xn + yn * yn
    rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    assert abs(sx[0] - (60.0 * (xn * rad + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn)) + 33.0)) < 1e-9
    assert abs(sy[0] - (50.0 * (yn * rad + p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn) + 22.0)) < 1e-9


def test_the_equidistant_model():
    """the lens axis maps to the image centre, and the view axis at angle theta from it lands at radius R theta / (lens_fov / 2), azimuth pan"""
    src, dst = (1000, 1200), (481, 641)
    centre = np.array([320.0]), np.array([240.0])
    sx, sy = warp.fisheye_view_map(src, dst, 90, 77, 0)(*centre)
    assert abs(sx[0] - 599.5) < 1e-9 and abs(sy[0] - 499.5) < 1e-9
    for lens_fov, theta, pan in ((180, 30, 0), (180, 60, 120), (220, 90, -45)):
        sx, sy = warp.fisheye_view_map(src, dst, 90, pan, theta, roll=13, lens_fov=lens_fov)(*centre)
        r = 500.0 * theta / (lens_fov / 2)
        assert abs(sx[0] - (599.5 + r * math.cos(math.radians(pan)))) < 1e-9 and abs(sy[0] - (499.5 + r * math.sin(math.radians(pan)))) < 1e-9
    # the other models at the rim and on the axis; a panorama's top row runs along the rim
    for lens in warp.LENSES:
        sx, sy = warp.fisheye_view_map(src, dst, 60, 0, 90, lens=lens)(*centre)
        assert abs(sx[0] - 1099.5) < 1e-6 and abs(sy[0] - 499.5) < 1e-6, lens
    sx, sy = warp.fisheye_panorama_map(src, (100, 720), inner=10)(np.arange(720.0), np.full(720, -0.5))
    assert np.allclose(np.hypot(sx - 599.5, sy - 499.5), 500.0)
    with pytest.raises(ValueError):
        warp.fisheye_view(src, dst, 90, 0, 0, lens="pinhole")


def test_source_points_against_the_function():
    fn = warp.homography_map([[0.9, 0.2, 3.0], [-0.1, 1.1, 5.0], [0.0, 0.0, 1.0]])      # affine: the mesh interpolates it exactly
    m = warp.mesh_from_function((33, 47), fn)
    xy = np.array([[0.0, 0.0], [46.0, 32.0], [10.25, 7.5], [39.9, 0.1]])
    got = m.source_points(xy)
    want = np.stack(fn(xy[:, 0], xy[:, 1]), -1)
    assert np.abs(got - want).max() <= 1 / 64
    v = warp.fisheye_view((1024, 1024), (480, 640), 90, 30, 40)
    px = np.array([[100, 50], [639, 479], [320, 240]])
    assert np.allclose(v.source_points(px.astype(np.float64)), v.positions(px), atol=1e-9)


@pytest.mark.parametrize("dst,pan,tilt,src,fov", [((480, 640), 30, 40, 1024, 90), ((720, 960), 120, 60, 2048, 110), ((720, 1280), 0, 0, 2880, 60),
                                               ((480, 640), 200, 80, 2880, 60)])
def test_mesh_error_of_the_equidistant_views(dst, pan, tilt, src, fov):
    """What the 8-pixel cell and the 1/64 rounding cost against the exact map, in source pixels, for views of 90, 110, 60 and 60 degrees (horizontal):
    measured 0.042, 0.090, 0.013 and 0.062. The error grows with the square of the source pixels a cell spans: the last view, 10 degrees from the
    rim of a 2880 x 2880 fisheye, measures 0.188 at 90 and 0.380 at 110 degrees -- give such a view more destination pixels or a narrower field."""
    fn = warp.fisheye_view_map((src, src), dst, fov, pan, tilt)
    err = warp.mesh_error(warp.mesh_from_function(dst, fn), fn)
    print("mesh_error", dst, pan, tilt, src, fov, err)
    assert err < 0.1


def test_mesh_refuses_wrong_shapes_and_values():
    with pytest.raises(ValueError, match="shape"):
        warp.Mesh(np.zeros((3, 3, 2), np.int32), (16, 17))
    with pytest.raises(ValueError, match="shape"):
        warp.Mesh(np.zeros((3, 4, 2), np.int64), (16, 17))
    with pytest.raises(ValueError, match="2\\^21"):
        warp.Mesh(np.full((3, 4, 2), 1 << 21, np.int32), (16, 17))
    far = warp.mesh_from_function((16, 17), lambda x, y: (x * np.inf, y * 0 + np.nan))
    assert np.abs(far.points).max() == (1 << 21) - 1


# ---------------------------------------------------------------------------------------------------------------- set
class _Batch(FrameBatch):
    """a FrameBatch whose surfaces were never uploaded: what set() validates against, without a device"""

    def __init__(self, sizes, fmt="nv12", matrix="bt709", full=False):
        super().__init__(len(sizes), "cpu", format=fmt, matrix=matrix, full_range=full)
        self.sizes = list(sizes)


def _records(items, fmt="nv12", capacity=8, src=ref.SRC_SIZES, dst=ref.DST_SIZES):
    return warp.item_records(items, src, dst, fmt, "bt709", False, capacity)


def test_every_refusal_of_set_names_the_item():
    ident = warp.identity((16, 20))
    ok = warp.Item(0, 0, ident, (0, 0))
    raw, mesh, norm, tiles = _records([ok, warp.Item(1, 1, ident, (2, 2), "replicate"), (0, 0, ident, (40, 40), (255, 0, 0))])
    assert tiles == 3 and len(mesh) == 3 * 4 and [n[3] for n in norm] == [0, 0, 0] and len(raw) == 16 + 8 * 48
    for bad, match in (
            (warp.Item(2, 0, ident), "item 1: source index 2"), (warp.Item(0, -1, ident), "item 1: destination index -1"),
            (warp.Item(0, 0, ident, (230, 100)), "item 1: the destination rectangle x 230 .. 250"),
            (warp.Item(0, 0, ident, (30, 190)), "item 1: .* lies outside"), (warp.Item(0, 0, ident, (-2, 0)), "item 1: .* lies outside"),
            (warp.Item(0, 0, ident, (31, 40)), "item 1: odd origin"), (warp.Item(0, 0, ident, (40, 41)), "item 1: odd origin"),
            (warp.Item(0, 0, ident, (18, 14)), "item 1: .* overlaps item 0"),
            (warp.Item(0, 0, ident, (0, 0), (0, 0, 256)), "item 1: border"), (warp.Item(0, 0, ident, (0, 0), "clamp"), "item 1: border"),
            (warp.Item(0, 0, ident.points, (40, 40)), "item 1: mesh must be a Mesh"), (warp.Item(0.0, 0, ident, (40, 40)), "item 1: src and dst"),
            ("nonsense", "item 1: expected an Item")):
        with pytest.raises(ValueError, match=match):
            _records([ok, bad])
    # A rectangle that ends at an odd column or row owns the chroma sample of the pixel behind its end. The only rectangle that overlaps it in chroma
    # but not in luma starts on that odd pixel, and set refuses it by its origin; the next even pixel is free. The chroma clause itself:
    odd = warp.identity((15, 19))
    a, b = (0, 0, 19, 15), (19, 0, 4, 4)
    assert not warp._overlap(a, b) and warp._overlap(warp._chroma(a), warp._chroma(b)) and not warp._overlap(warp._chroma(a), warp._chroma((20, 16, 4, 4)))
    with pytest.raises(ValueError, match="item 1: odd origin"):
        _records([warp.Item(0, 0, odd, (0, 0)), warp.Item(0, 0, ident, (19, 0))])
    with pytest.raises(ValueError, match="item 1: odd origin"):
        _records([warp.Item(0, 0, odd, (0, 0)), warp.Item(0, 0, ident, (0, 15))])
    _records([warp.Item(0, 0, odd, (0, 0)), warp.Item(0, 0, odd, (20, 0)), warp.Item(0, 0, odd, (0, 16))])
    _records([warp.Item(0, 0, odd, (0, 0)), warp.Item(0, 0, ident, (19, 0)), warp.Item(0, 0, ident, (31, 41))], fmt="rgb24")      # packed pixels: any origin, no chroma
    # mesh shape and mesh values: a Mesh whose points were swapped behind its back
    for pts, match in ((np.zeros((3, 3, 2), np.int32), "item 1: the mesh of a 20 x 16"), (np.full((3, 4, 2), -(1 << 21), np.int32), "item 1: a mesh value")):
        m = warp.identity((16, 20))
        m.points = pts
        with pytest.raises(ValueError, match=match):
            _records([ok, warp.Item(0, 0, m, (40, 40))])
    with pytest.raises(ValueError, match="3 items, the capacity is 2"):
        _records([ok, ok, ok], capacity=2)
    with pytest.raises(ValueError, match="expected a list"):
        _records(torch.zeros(3))


def test_set_refuses_batches_that_differ_and_a_call_refuses_stale_sizes():
    ident = warp.identity((16, 20))
    w = warp.Warper(4, "cpu")
    src = _Batch(ref.SRC_SIZES)
    with pytest.raises(ValueError, match="the Compositor's job"):
        w.set([warp.Item(0, 0, ident)], src, _Batch(ref.DST_SIZES, "i420"))
    with pytest.raises(ValueError, match="the Compositor's job"):
        w.set([warp.Item(0, 0, ident)], src, _Batch(ref.DST_SIZES, "nv12", "bt601"))
    with pytest.raises(ValueError, match="the Compositor's job"):
        w.set([warp.Item(0, 0, ident)], src, _Batch(ref.DST_SIZES, "nv12", "bt709", True))
    with pytest.raises(ValueError, match="two batches"):
        w.set([warp.Item(0, 0, ident)], src, src)
    with pytest.raises(ValueError, match="must be a FrameBatch"):
        w.set([warp.Item(0, 0, ident)], src, None)
    with pytest.raises(ValueError, match="item 0: source index 5"):
        w.set([warp.Item(5, 0, ident)], src, _Batch(ref.DST_SIZES))
    assert w.table is None and w.items == [] and w.src_sizes is None                       # nothing changed
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        w.set([warp.Item(0, 0, ident)], src, _Batch(ref.DST_SIZES))
    for bad in (0, 65537, True, 2.0):
        with pytest.raises(ValueError, match="capacity"):
            warp.Warper(bad, "cpu")
    with pytest.raises(ValueError, match="mesh_points"):
        warp.Warper(4, "cpu", mesh_points=0)
    # a call: what set() remembered against the batches as they are now (the state of a set() written by hand: there is no device here)
    dst = _Batch(ref.DST_SIZES)
    src.table = dst.table = w.table = torch.zeros(1)
    w.src_sizes, w.dst_sizes, w.space = list(ref.SRC_SIZES), list(ref.DST_SIZES), (src.format_code, src.color_code)
    warp.check_warp("Warper", w, src, dst)
    src.sizes = [(80, 96), (46, 67)]
    with pytest.raises(ValueError, match="stale sizes: .* source"):
        w(src, dst)
    src.sizes = list(ref.SRC_SIZES)
    dst.sizes = dst.sizes[:1]
    with pytest.raises(ValueError, match="stale sizes: .* destination"):
        w(src, dst)
    dst.sizes = list(ref.DST_SIZES)
    other = _Batch(ref.DST_SIZES, "i420")
    other.table = torch.zeros(1)
    with pytest.raises(ValueError, match="format / colour code"):
        w(src, other)
    with pytest.raises(ValueError, match="go together"):
        warp.check_warping(w, None, dst, "track_frames")
    with pytest.raises(ValueError, match="expected a Warper"):
        warp.check_warping(object(), src, dst, "track_frames")
    warp.check_warping(None, None, dst, "track_frames")


def test_the_records_match_the_header(tmp_path):
    fields = ["src", "dst", "dx0", "dy0", "dw", "dh", "mesh0", "mesh_w", "flags", "border", "tile0", "reserved"]
    head = ["n_items", "n_tiles", "n_points", "reserved"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "demonet_hip.h"\nint main(){printf("%zu %zu %d %d %d", sizeof(dn_warp_item), sizeof(dn_warp_header), '
            'DN_WARP_CELL, DN_WARP_BORDER_CONSTANT, DN_WARP_BORDER_REPLICATE);\n'
            + "".join('printf(" %zu", offsetof(dn_warp_item, {}));\n'.format(f) for f in fields)
            + "".join('printf(" %zu", offsetof(dn_warp_header, {}));\n'.format(f) for f in head) + "return 0;}\n")
    (tmp_path / "w.c").write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "w.c"), "-o", str(tmp_path / "w")])
    a = [int(v) for v in subprocess.check_output([str(tmp_path / "w")]).split()]
    assert a[:5] == [C.sizeof(_lib.WarpItem), C.sizeof(_lib.WarpHeader), _lib.DN_WARP_CELL, _lib.DN_WARP_BORDER["constant"], _lib.DN_WARP_BORDER["replicate"]]
    assert a[:2] == [48, 16]
    assert a[5:17] == [getattr(_lib.WarpItem, f).offset for f in fields] and a[17:] == [getattr(_lib.WarpHeader, f).offset for f in head]
    assert [f for f, _ in _lib.WarpItem._fields_] == fields and "dn_warp" in _lib.EXPORTS
    # the table set() writes: tile0 is the running tile count, shared meshes are stored once, a bgr24 border is in memory order
    m = warp.identity((40, 70))
    raw, mesh, norm, tiles = warp.item_records([warp.Item(0, 0, m, (0, 0), (1, 2, 3)), warp.Item(1, 0, m, (0, 40), "replicate"), warp.Item(0, 1, warp.identity((3, 5)))],
                                               ref.SRC_SIZES, ref.DST_SIZES, "bgr24", "bt709", False, 4)
    h = _lib.WarpHeader.from_buffer_copy(raw[:16])
    it = [_lib.WarpItem.from_buffer_copy(raw[16 + 48 * i:64 + 48 * i]) for i in range(4)]
    assert (h.n_items, h.n_tiles, h.n_points) == (3, 13, 6 * 10 + 2 * 2) == (3, tiles, len(mesh))
    assert [(r.mesh0, r.mesh_w, r.tile0, r.flags, r.border) for r in it[:3]] == [(0, 10, 0, 0, 3 | 2 << 8 | 1 << 16), (0, 10, 6, 1, 0), (60, 2, 12, 0, 0)]
    assert bytes(it[3]) == bytes(48)
