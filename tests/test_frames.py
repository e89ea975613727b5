"""Video frames as input, CPU side (-m "not gpu"): the integer colour conversion of dn_forward_frames against the real-valued formula it rounds
(tests/frames_ref.py), the classic mistakes that must leave the bound, known colours, the ABI of dn_frame / dn_forward_frames, and the host-side
validation of FrameBatch.set, which runs before any device use."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import frames_ref as fr
from demonet_amd import _lib
from demonet_amd.frames import FrameBatch, frame_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "demonet_hip.h")

# |integer result before clamping - real-valued formula| <= 0.5 (the rounding of >> 14 after + 2^13) + 511 * 2^-15: |y| <= 255, |u|, |v| <= 128,
# and every coefficient is off by at most half a unit of 2^-14
BOUND = 0.5 + 511 * 2.0 ** -15
TABLE = {("bt601", False): (19077, 26149, 33050, 6419, 13320, 16), ("bt601", True): (16384, 22970, 29032, 5638, 11700, 0),
         ("bt709", False): (19077, 29372, 34610, 3494, 8731, 16), ("bt709", True): (16384, 25802, 30402, 3069, 7670, 0)}
_U, _V = np.meshgrid(np.arange(256, dtype=np.int32), np.arange(256, dtype=np.int32), indexing="ij")


def _worst(matrix, full, ref=None, slabs=range(0, 256, 32), **mutant):
    """max over all 256^3 triples (or the slabs of 32 luma codes named) and the three channels of |integer (unclamped) - real|; ref: the (matrix, full) of
    the real-valued side when it differs"""
    worst, differs = 0.0, False
    rm, rf = ref or (matrix, full)
    for y0 in slabs:
        Y = np.arange(y0, y0 + 32, dtype=np.int32)[:, None, None]
        Yb, Ub, Vb = np.broadcast_arrays(Y, _U[None], _V[None])
        got = fr.yuv_to_rgb_int(Yb, Ub, Vb, matrix, full, clamp=False, **mutant)
        want = fr.yuv_to_rgb_real(Yb, Ub, Vb, rm, rf)
        worst = max(worst, float(np.abs(got - want).max()))
        if mutant:
            differs = differs or bool((got != fr.yuv_to_rgb_int(Yb, Ub, Vb, rm, rf, clamp=False)).any())
    return worst, differs


def test_integer_coefficients_are_the_rounded_real_ones():
    for key, want in TABLE.items():
        assert fr.int_coeffs(*key) == want, key
        # all sums fit in int32
        cy, crv, cbu, cgu, cgv, yo = want
        assert cy * 255 + max(crv, cbu, cgu + cgv) * 128 + (1 << 13) < 2 ** 31


@pytest.mark.parametrize("matrix,full", fr.VARIANTS, ids=["601-limited", "601-full", "709-limited", "709-full"])
def test_integer_conversion_is_within_the_bound_of_the_real_formula(matrix, full):
    worst, _ = _worst(matrix, full)
    print("\n{} {}: max |integer - real| = {:.4f} (bound {:.4f})".format(matrix, "full" if full else "limited", worst, BOUND))
    assert worst <= BOUND


MUTANTS = [("U-and-V-swapped", ("bt709", False), ("bt709", False), dict(swap_uv=True)),
           ("limited-treated-as-full", ("bt709", True), ("bt709", False), {}),
           ("601-treated-as-709", ("bt709", False), ("bt601", False), {}),
           ("minus-128-dropped", ("bt601", False), ("bt601", False), dict(offset=0))]


@pytest.mark.parametrize("what,used,meant,kw", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_the_bound_catches_a_wrong_conversion(what, used, meant, kw):
    worst, _ = _worst(*used, ref=meant, slabs=(0, 224), **kw)         # (some triple: the darkest and the brightest luma codes are enough)
    assert worst > BOUND + 10.0, (what, worst)


def test_truncation_toward_zero_differs_from_the_arithmetic_shift():
    _, differs = _worst("bt601", False, slabs=(0,), truncate=True)
    assert differs


def test_known_colours():
    for matrix in ("bt601", "bt709"):
        assert fr.yuv_to_rgb_int(16, 128, 128, matrix, False).tolist() == [0, 0, 0]
        assert fr.yuv_to_rgb_int(235, 128, 128, matrix, False).tolist() == [255, 255, 255]
        g = np.arange(256)
        assert np.array_equal(fr.yuv_to_rgb_int(g, 128, 128, matrix, True), np.stack([g, g, g], -1))
    assert [int(np.floor(x + 0.5)) for x in fr.rgb_to_yuv_real([255, 0, 0], "bt601", False)] == [81, 90, 240]
    assert [int(np.floor(x + 0.5)) for x in fr.rgb_to_yuv_real([0, 255, 0], "bt709", False)] == [173, 42, 26]
    for matrix, full in fr.VARIANTS:
        for rgb in ([255, 0, 0], [0, 255, 0], [0, 0, 255]):
            yuv = [int(np.floor(x + 0.5)) for x in fr.rgb_to_yuv_real(rgb, matrix, full)]
            back = fr.yuv_to_rgb_int(*yuv, matrix, full)
            assert np.abs(back - np.array(rgb)).max() <= 2, (matrix, full, rgb, yuv, back)


def test_planes_to_rgb_replicates_chroma_over_2x2():
    Y, U, V = fr.noise_yuv(3, 5, 7)
    rgb = fr.planes_to_rgb(Y, U, V, "bt601", False)
    assert rgb.shape == (5, 7, 3) and rgb.dtype == np.uint8
    for (y, x) in ((0, 0), (1, 1), (4, 6), (3, 2), (2, 5)):
        assert rgb[y, x].tolist() == fr.yuv_to_rgb_int(Y[y, x], U[y >> 1, x >> 1], V[y >> 1, x >> 1], "bt601", False).tolist()


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_forward_frames_is_declared_exported_and_bound():
    txt = open(HEADER).read()
    assert re.search(r"DN_API\s+int\s+dn_forward_frames\s*\(", txt)
    assert re.search(r"^#define DN_ABI_VERSION 1$", txt, re.M)
    assert "dn_forward_frames" in _lib.EXPORTS
    if not os.path.exists(_lib.LIB_PATH):
        from demonet_amd import build
        build.build(verbose=False)
    assert hasattr(C.CDLL(_lib.LIB_PATH), "dn_forward_frames")
    assert _lib.DN_FRAME == dict(nv12=0, i420=1, rgb24=2, bgr24=3) and _lib.DN_COLOR == dict(bt601=0, bt709=1) and _lib.DN_COLOR_FULL_RANGE == 0x10


def test_frame_record_layout_matches_c(tmp_path):
    src = tmp_path / "fr.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "demonet_hip.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d\\n", sizeof(dn_frame), offsetof(dn_frame, plane), offsetof(dn_frame, pitch), '
                   'offsetof(dn_frame, width), offsetof(dn_frame, height), offsetof(dn_frame, reserved), DN_FRAME_NV12, DN_FRAME_I420, DN_FRAME_RGB24, '
                   'DN_FRAME_BGR24, DN_COLOR_BT601, DN_COLOR_BT709, DN_COLOR_FULL_RANGE);return 0;}\n')
    exe = tmp_path / "fr"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    F = _lib.Frame
    assert a[0] == 48 == C.sizeof(F)
    assert a[1:6] == [F.plane.offset, F.pitch.offset, F.width.offset, F.height.offset, F.reserved.offset]
    assert a[6:] == [0, 1, 2, 3, 0, 1, 0x10]


# ---------------------------------------------------------------------------------------------------------------- FrameBatch.set validation
def _u8(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


def test_records_of_valid_frames():
    h, w = 6, 10
    flat = _u8(h * 3 // 2, w)
    big = _u8(h, 32)
    uv = _u8(3, 16)
    rec = frame_records([flat, (big[:, 3:3 + w], uv[:, :w])], "nv12", "cpu", 2)
    assert (rec[0].width, rec[0].height, rec[0].plane[0], rec[0].plane[1], list(rec[0].pitch)[:2]) == (w, h, flat.data_ptr(), flat.data_ptr() + h * w, [w, w])
    assert (rec[1].width, rec[1].height, rec[1].plane[0], rec[1].plane[1], list(rec[1].pitch)[:2]) == (w, h, big.data_ptr() + 3, uv.data_ptr(), [32, 16])
    rec = frame_records([flat], "i420", "cpu", 1)
    assert [rec[0].plane[j] - flat.data_ptr() for j in range(3)] == [0, h * w, h * w + (h // 2) * (w // 2)] and list(rec[0].pitch) == [w, w // 2, w // 2]
    # odd sizes through the plane form: chroma is ceil(h/2) x ceil(w/2); NV12's UV plane also as [ch, cw, 2]
    rec = frame_records([(_u8(5, 7), _u8(3, 4, 2))], "nv12", "cpu", 1)
    assert (rec[0].width, rec[0].height, list(rec[0].pitch)[:2]) == (7, 5, [7, 8])
    rec = frame_records([(_u8(5, 7), _u8(3, 4), _u8(3, 4))], "i420", "cpu", 1)
    assert list(rec[0].pitch) == [7, 4, 4]
    img = _u8(4, 20, 3)
    rec = frame_records([img[:, 2:7]], "bgr24", "cpu", 1)
    assert (rec[0].width, rec[0].height, rec[0].pitch[0], rec[0].plane[0]) == (5, 4, 60, img.data_ptr() + 6)
    # ... and a valid set() on a CPU batch ends where the device would begin: there is no CPU path
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FrameBatch(1, "cpu", "nv12").set([flat])


def _shrunk():
    t = _u8(6, 8)
    t.untyped_storage().resize_(40)         # the view now ends 8 bytes past its storage
    return t


BAD = [("wrong-dtype", "nv12", lambda: [torch.zeros((9, 8), dtype=torch.int8), _u8(9, 8)], r"frame 0, plane Y.*uint8"),
       ("float-plane", "i420", lambda: [_u8(9, 8), (_u8(6, 8), _u8(3, 4), torch.zeros(3, 4))], r"frame 1, plane V.*uint8"),
       ("odd-h-contiguous", "nv12", lambda: [_u8(9, 8), _u8(10, 8)], r"frame 1.*even h and w"),
       ("odd-w-contiguous", "i420", lambda: [_u8(9, 7), _u8(9, 8)], r"frame 0.*even h and w"),
       ("pitch-smaller-than-width", "nv12", lambda: [_u8(9, 8), (_u8(6, 8).as_strided((6, 8), (4, 1)), _u8(3, 8))], r"frame 1, plane Y.*pitch 4"),
       ("rows-overlap-rgb", "rgb24", lambda: [_u8(4, 5, 3), _u8(4, 15).as_strided((4, 5, 3), (12, 3, 1))], r"frame 1, plane RGB.*pitch 12"),
       ("past-its-storage", "nv12", lambda: [_u8(9, 8), (_shrunk(), _u8(3, 8))], r"frame 1, plane Y.*storage of 40 bytes"),
       ("chroma-shape", "nv12", lambda: [_u8(9, 8), (_u8(6, 8), _u8(3, 6))], r"frame 1, plane UV.*shape"),
       ("chroma-shape-i420", "i420", lambda: [(_u8(5, 7), _u8(3, 4), _u8(2, 4)), _u8(9, 8)], r"frame 0, plane V.*shape"),
       ("column-strided", "i420", lambda: [_u8(9, 8), (_u8(6, 8), _u8(3, 8)[:, ::2], _u8(3, 4))], r"frame 1, plane U.*contiguous"),
       ("plane-count", "i420", lambda: [_u8(9, 8), (_u8(6, 8), _u8(3, 8))], r"frame 1.*3 plane"),
       ("wrong-count", "nv12", lambda: [_u8(9, 8)], r"expected 2 frames, got 1"),
       ("a-tensor-not-a-list", "nv12", lambda: _u8(2, 9, 8), r"expected a list"),
       ("rgb-not-3d", "rgb24", lambda: [_u8(4, 15), _u8(4, 5, 3)], r"frame 0, plane RGB")]


@pytest.mark.parametrize("what,fmt,make,msg", BAD, ids=[b[0] for b in BAD])
def test_set_refuses_malformed_frames(what, fmt, make, msg):
    batch = FrameBatch(2, "cpu", fmt)
    with pytest.raises(ValueError, match=msg):
        batch.set(make())
    assert batch.table is None and batch.frames is None


def test_set_refuses_a_plane_on_another_device():
    with pytest.raises(ValueError, match=r"frame 0, plane Y.*is on cpu"):
        frame_records([_u8(9, 8)], "nv12", "meta", 1)


def test_constructor_refuses_unknown_names():
    for kw in (dict(format="nv21"), dict(matrix="bt2020"), dict(format=0)):
        with pytest.raises(ValueError):
            FrameBatch(1, "cpu", **kw)
    with pytest.raises(ValueError):
        FrameBatch(0, "cpu")
