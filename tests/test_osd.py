"""CPU tests of the on-screen display: tests/osd_ref.py against closed forms written out by hand, the colour conversion, the font,
the text builder, the host-side validation of demonet_amd/osd.py and the ABI of its records -- and that the scenes of tests/test_gpu_osd.py tell
the reference from six wrong painters, so that a device painter that made one of those mistakes could not pass there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import frames_ref as fr
import osd_ref as ref
import regions_ref as rr
from demonet_amd import _lib, osd, osd_font
from demonet_amd.frames import FrameBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FONT = osd_font.table()
FORMATS = ("nv12", "i420", "rgb24", "bgr24")


def _paint(chans, subs, rows, style, palette, cfg=None, params=None, **kw):
    return ref.paint(chans, subs, rows, None, style, 6, ref.name_records(), palette, FONT, cfg, params or ref.default_params(), **kw)[0]


# ---------------------------------------------------------------------------------------------------------------- 1. closed forms
def test_a_fill_of_alpha_128_on_a_constant_nv12_frame_by_hand():
    chans = [np.full((6, 6), 100, np.uint8), np.full((3, 3), 100, np.uint8), np.full((3, 3), 100, np.uint8)]
    out = _paint(chans, (1, 2, 2), ref.make_rows([(1.0, 1.0, 4.0, 4.0)]), (0, 128, 0, 0), [((200, 50, 220), (0, 0, 0))])
    # (128 * 200 + 127 * 100 + 127) / 255 = 38427 / 255 = 150; U: 19227 / 255 = 75; V: 40987 / 255 = 160
    Y = np.full((6, 6), 100, np.uint8)
    Y[1:4, 1:4] = 150
    U = np.full((3, 3), 100, np.uint8)
    V = np.full((3, 3), 100, np.uint8)
    U[1, 1], V[1, 1] = 75, 160                    # the only chroma sample whose governing pixel (2, 2) lies in 1 .. 3
    assert np.array_equal(out[0], Y) and np.array_equal(out[1], U) and np.array_equal(out[2], V)


def test_an_outline_of_thickness_1_by_hand():
    chans = [np.full((6, 6), 9, np.uint8), np.full((3, 3), 9, np.uint8), np.full((3, 3), 9, np.uint8)]
    out = _paint(chans, (1, 2, 2), ref.make_rows([(1.0, 1.0, 5.0, 5.0)]), (1, 0, 0, 0), [((200, 50, 220), (0, 0, 0))])
    Y = np.full((6, 6), 9, np.uint8)
    Y[1:5, 1:5] = 200
    Y[2:4, 2:4] = 9
    U = np.full((3, 3), 9, np.uint8)
    U[1, 2] = U[2, 1] = U[2, 2] = 50              # pixels (4, 2), (2, 4), (4, 4) are on the ring, (2, 2) is inside it, (0, .) outside
    V = np.where(U == 50, 220, 9).astype(np.uint8)
    assert np.array_equal(out[0], Y) and np.array_equal(out[1], U) and np.array_equal(out[2], V)


def test_a_pixelate_of_block_4_on_a_ramp_by_hand():
    ramp = (np.arange(6)[None, :] + 10 * np.arange(6)[:, None]).astype(np.uint8)
    out = _paint([ramp, ramp.copy(), ramp.copy()], (1, 1, 1), ref.make_rows([(0.0, 0.0, 6.0, 6.0)]), (0, 0, 4, 0), [((1, 2, 3), (0, 0, 0))])
    want = np.empty((6, 6), np.uint8)
    want[:4, :4] = 17                             # mean 16.5 of 16: (264 + 8) / 16
    want[:4, 4:] = 20                             # 19.5 of 8: (156 + 4) / 8
    want[4:, :4] = 47                             # 46.5 of 8: (372 + 4) / 8
    want[4:, 4:] = 50                             # 49.5 of 4: (198 + 2) / 4
    for c in out:
        assert np.array_equal(c, want)


# ---------------------------------------------------------------------------------------------------------------- 2. colours
@pytest.mark.parametrize("matrix,full", fr.VARIANTS)
def test_palette_to_surface_and_back_stays_within_the_derived_bound(matrix, full):
    """Forward: each of Y, U, V is off by at most 0.5 (its final rounding) + 3 * 255 * 0.5 / 2^14 (the rounded coefficients). The inverse multiplies
    those errors by the magnitudes of its row's coefficients, adds its own coefficients' rounding, at most (255 + 2 * 128) * 0.5 / 2^14 per term, and
    rounds once more (0.5). Clamping moves a value towards the range the true colour lies in. The bound is stated, not tuned."""
    assert osd.forward_coeffs(matrix, full) == ref.forward_coeffs(matrix, full)
    cy, crv, cbu, cgu, cgv, _ = fr.real_coeffs(matrix, full)
    e = 0.5 + 3 * 255 * 0.5 / 2 ** 14
    own = 0.5 + 3 * 255 * 0.5 / 2 ** 14
    bound = np.array([(cy + crv) * e + own, (cy + cgu + cgv) * e + own, (cy + cbu) * e + own])
    levels = np.linspace(0, 255, 6).round().astype(int)
    worst = np.zeros(3)
    for r in levels:
        for g in levels:
            for b in levels:
                yuv = osd.to_surface((int(r), int(g), int(b)), "nv12", matrix, full)
                assert yuv == ref.to_surface((r, g, b), "nv12", matrix, full)
                back = fr.planes_to_rgb(np.array([[yuv[0]]], np.uint8), np.array([[yuv[1]]], np.uint8), np.array([[yuv[2]]], np.uint8), matrix, full)
                worst = np.maximum(worst, np.abs(back[0, 0].astype(int) - np.array([r, g, b])))
    print("round trip", matrix, full, "worst", worst, "bound", bound)
    assert np.all(worst <= bound), (worst, bound)
    assert osd.to_surface((1, 2, 3), "bgr24", matrix, full) == (1, 2, 3)


# ---------------------------------------------------------------------------------------------------------------- 3. font
def test_the_font_has_64_distinct_glyphs_inside_5_by_7():
    assert FONT.shape == (64, 8) and FONT.dtype == np.uint8
    bits = np.unpackbits(FONT[:, :, None], axis=2)             # [glyph][row][column], column 0 = bit 7
    assert not bits[0].any()
    assert all(bits[g].any() for g in range(1, 64))
    assert len({FONT[g].tobytes() for g in range(64)}) == 64
    for g in range(1, 64):
        ys, xs = np.nonzero(bits[g])
        assert ys.max() - ys.min() < 7 and xs.max() - xs.min() < 5
    assert not bits[:, 7].any() and not bits[:, :, 0].any() and not bits[:, :, 6:].any()       # the gap between characters and between lines
    assert osd_font.glyph_index(ord("q")) == osd_font.glyph_index(ord("Q")) == ref.glyph(ord("q")) == ord("Q") - 32
    assert osd_font.glyph_index(200) == ref.glyph(200) == ord("?") - 32
    assert all(osd_font.glyph_index(b) == ref.glyph(b) for b in range(256))


# ---------------------------------------------------------------------------------------------------------------- 4. text
def test_the_text_builder():
    name = b"car".ljust(16, b"\0")
    t = lambda i, s=None: ref.build_text(name, i, s is not None, 0.0 if s is None else s)
    assert t(0) == b"car #0" and t(7) == b"car #7" and t(999999999) == b"car #999999999"
    assert t(10 ** 9) == b"car #?" and t(-1) == b"car #?" and t(None) == b"car"
    assert t(None, 0.0) == b"car 0%" and t(None, 0.994) == b"car 99%" and t(None, 0.995) == b"car 100%" and t(None, 1.0) == b"car 100%"
    assert t(None, 2.0) == b"car 100%" and t(None, -1.0) == b"car 0%" and t(None, float("nan")) == b"car ?%" and t(None, float("inf")) == b"car ?%"
    longest = ref.build_text(b"abcdefghijklmno\0", 999999999, True, 1.0)
    assert longest == b"abcdefghijklmno #999999999 100%" and len(longest) == 31
    assert ref.build_text(None, 5, False, 0.0) == b" #5"


# ---------------------------------------------------------------------------------------------------------------- 5. discrimination
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("size", rr.SIZES)
def test_the_gpu_scenes_tell_the_reference_from_six_wrong_painters(fmt, size):
    """(the chroma mistake cannot show where there is no chroma plane: it is asked of the 4:2:0 formats)"""
    h, w = size
    if fmt in ("nv12", "i420"):
        Y, U, V = fr.noise_yuv(77, h, w)
        chans, subs = [Y, U, V], (1, 2, 2)
    else:
        rgb = fr.noise_rgb(77, h, w)
        chans, subs = [rgb[..., 0], rgb[..., 1], rgb[..., 2]], (1, 1, 1)
    rows, cfg = ref.mixed_scene(w, h)
    pal = ref.palette_records(ref.PALETTE_RGB, fmt, "bt709", False)
    args = (chans, subs, rows, ref.MIXED_STYLES, ref.MIXED_STYLES[0], len(ref.MIXED_STYLES), ref.name_records(), pal, FONT, cfg, ref.default_params())
    right, (painted, skipped) = ref.paint(*args)
    assert painted >= 6 and skipped == 3
    assert any(not np.array_equal(a, b) for a, b in zip(right, chans))
    for variant in ref.VARIANTS:
        if variant == "chroma_bottom_right" and subs == (1, 1, 1):
            continue
        wrong = ref.paint(*args, variant=variant)[0]
        assert any(not np.array_equal(a, b) for a, b in zip(right, wrong)), variant


# ---------------------------------------------------------------------------------------------------------------- 6. validation
def test_the_overlay_refuses_bad_arguments_on_the_host():
    for kw in (dict(names=["ok", "x" * 16]), dict(names=["café"]), dict(names=[]), dict(names=[3]), dict(palette=[(1, 2)]), dict(palette=[(1, 2, 256)]),
               dict(palette=[]), dict(palette=[(0, 0, 0)] * 257), dict(scale=0), dict(scale=5), dict(thickness=17), dict(thickness=-1),
               dict(fill_alpha=256), dict(label_alpha=-1), dict(colour_by="track"), dict(label=1), dict(score="yes"), dict(line_thickness=0),
               dict(zone_alpha=300), dict(line_colour=(1, 2))):
        with pytest.raises(ValueError):
            osd.Overlay(2, "cpu", **kw)
    with pytest.raises(ValueError, match="label 1"):
        osd.Overlay(2, "cpu", names=["ok", "much too long a name"])
    with pytest.raises(ValueError):
        osd.Overlay(0, "cpu")
    with pytest.raises(RuntimeError):
        osd.Overlay(2, "cpu")                       # everything valid: there is no CPU path
    for kw in (dict(pixelate=5), dict(pixelate=64), dict(pixelate=True), dict(thickness=17), dict(fill_alpha=-1), dict(hide=2)):
        with pytest.raises(ValueError):
            osd.make_style(**kw)
    s = osd.make_style(3, 10, 16, True, False, True)
    assert (s.thickness, s.fill_alpha, s.pixelate, s.flags) == (3, 10, 16, _lib.DN_OSD_LABEL | _lib.DN_OSD_HIDE)


def test_paint_refuses_wrong_tensors_before_the_library_is_touched(monkeypatch):
    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    dev = torch.device("cpu")
    batch = FrameBatch(2, "cpu")
    good = dict(boxes=torch.zeros(2, 5, 4), scores=torch.zeros(2, 5), labels=torch.zeros(2, 5, dtype=torch.int64), counts=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="names no frames"):
        osd.check_paint(2, dev, batch, **good)
    batch.table = torch.zeros(96, dtype=torch.uint8)
    assert osd.check_paint(2, dev, batch, **good) == 5
    assert osd.check_paint(2, dev, batch, ids=torch.zeros(2, 5, dtype=torch.int64), **good) == 5
    bad = [dict(boxes=torch.zeros(2, 5, 3)), dict(boxes=torch.zeros(3, 5, 4)), dict(boxes=torch.zeros(2, 5, 4, dtype=torch.float64)),
           dict(boxes=torch.zeros(2, 10, 4)[:, ::2]), dict(scores=torch.zeros(2, 4)), dict(scores=torch.zeros(2, 5, dtype=torch.float16)),
           dict(labels=torch.zeros(2, 5, dtype=torch.int32)), dict(counts=torch.zeros(2, dtype=torch.int64)), dict(counts=torch.zeros(3, dtype=torch.int32)),
           dict(ids=torch.zeros(2, 5, dtype=torch.int32)), dict(ids=torch.zeros(2, 4, dtype=torch.int64)), dict(boxes=np.zeros((2, 5, 4), np.float32)),
           dict(scores=torch.zeros(2, 5, device="meta")), dict(boxes=torch.zeros(2, 513, 4))]
    for change in bad:
        with pytest.raises(ValueError):
            osd.check_paint(2, dev, batch, **dict(good, **change))
    with pytest.raises(ValueError):
        osd.check_paint(3, dev, batch, **good)
    with pytest.raises(ValueError):
        osd.check_paint(2, torch.device("meta"), batch, **good)
    with pytest.raises(ValueError):
        osd.check_paint(2, dev, "frames", **good)


def test_workspace_tiles_are_counted_from_the_sizes():
    assert osd.Overlay.tiles([(200, 260), (97, 131)]) == 7 * 9 + 4 * 5
    assert osd.Overlay.tiles([(1080, 1920)]) == 34 * 60


# ---------------------------------------------------------------------------------------------------------------- 7. ABI
def test_the_records_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    fields = ["n_colors", "color_by_id", "scale", "label_alpha", "line_thickness", "zone_thickness", "zone_alpha", "line_color", "zone_color", "reserved"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "demonet_hip.h"\nint main(){printf("%zu %zu %zu", sizeof(dn_osd_params), '
                   'sizeof(dn_osd_style), sizeof(dn_osd_color));\n'
                   + "".join('printf(" %zu", offsetof(dn_osd_params, {}));\n'.format(f) for f in fields)
                   + 'printf(" %zu %zu %zu %zu", offsetof(dn_osd_style, fill_alpha), offsetof(dn_osd_style, pixelate), offsetof(dn_osd_style, flags), '
                   'offsetof(dn_osd_color, text));\nprintf(" %d %d %d\\n", DN_OSD_LABEL, DN_OSD_SCORE, DN_OSD_HIDE);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert a[:3] == [C.sizeof(_lib.OsdParams), C.sizeof(_lib.OsdStyle), C.sizeof(_lib.OsdColor)] == [64, 8, 8]
    assert a[3:13] == [getattr(_lib.OsdParams, f).offset for f in fields]
    assert a[13:17] == [_lib.OsdStyle.fill_alpha.offset, _lib.OsdStyle.pixelate.offset, _lib.OsdStyle.flags.offset, _lib.OsdColor.text.offset]
    assert a[17:] == [_lib.DN_OSD_LABEL, _lib.DN_OSD_SCORE, _lib.DN_OSD_HIDE] == [ref.LABEL, ref.SCORE, ref.HIDE]
