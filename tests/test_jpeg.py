"""The baseline JPEG encoder's statement (tests/jpeg_ref.py; include/demonet_hip.h, dn_jpeg_encode) held from outside, on the CPU: its own
decoder returns the coefficients it coded, an independent decoder (Pillow's libjpeg) opens every file and finds the luma as close to the source as
its own encoder gets, the tables are the ones that encoder writes, the scenes tell eight wrong encoders from the right one and contain every case
the entropy coder has, and JpegEncoder refuses on the host what the device would have to trust. No device work here."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

import compose_ref as cr
import jpeg_ref as ref
import regions_ref as rr
from demonet_amd import _lib, jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ref.plane_scenes()
_FILES = {}


def _encode(name, q, mistake=None):
    """(file, counters) of a plane-wise scene, computed once"""
    key = (name, q, mistake)
    if key not in _FILES:
        fmt, planes, rect = SCENES[name]
        _FILES[key] = ref.encode_item(fmt, "bt601", True, planes, rect, q, mistake)
    return _FILES[key]


def _all():
    return [(name, q) for name in SCENES for q in ref.QUALITIES]


def test_the_transform_constants_are_the_closed_forms_and_the_output_is_eight_times_the_dct():
    assert ref.DCT_CONSTANTS == (2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172)
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.integers(-128, 128, (500, 8, 8)), np.full((1, 8, 8), -128), np.full((1, 8, 8), 127),
                        (((np.indices((8, 8)).sum(0) & 1) * 255) - 128)[None]])
    got = ref.fdct(x)
    assert np.abs(got - ref.DCT_SCALE * ref.dct_float(x)).max() < 2.0          # 13-bit constants, two roundings: below two units of 1/8
    assert np.abs(got).max() < 1 << 15 and got[-3, 0, 0] == -8 * 1024


def test_round_trip_through_the_reference_decoder():
    for name, q in _all():
        data, stats = _encode(name, q)
        dec = ref.decode(data)
        fmt, planes, rect = SCENES[name]
        assert (dec["width"], dec["height"]) == (rect[2], rect[3])
        ql, qc = ref.quant_tables(q)
        assert np.array_equal(dec["q"][0], ql) and np.array_equal(dec["q"][1], qc)
        for got, want in zip(dec["coefficients"], stats["coefficients"]):
            assert np.array_equal(got, want), (name, q)


def test_the_tables_are_the_ones_an_independent_encoder_writes():
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.fromarray(cr.fr.noise_rgb(1, 32, 32)).save(buf, format="JPEG", quality=50, subsampling=2)
    d = buf.getvalue()
    at, huff, quant = 2, {}, {}
    while d[at + 1] != 0xDA:
        n = (d[at + 2] << 8) | d[at + 3]
        seg = d[at + 4:at + 2 + n]
        if d[at + 1] == 0xC4:
            while seg:
                cnt = sum(seg[1:17])
                huff[seg[0]] = (list(seg[1:17]), list(seg[17:17 + cnt]))
                seg = seg[17 + cnt:]
        if d[at + 1] == 0xDB:
            while seg:
                quant[seg[0] & 15] = list(seg[1:65])
                seg = seg[65:]
        at += 2 + n
    for table, key in zip(ref.HUFF, (0x00, 0x10, 0x01, 0x11)):
        assert (list(table[0]), list(table[1])) == huff[key]
    ql, qc = ref.quant_tables(50)
    assert ql[ref.ZIGZAG].tolist() == quant[0] and qc[ref.ZIGZAG].tolist() == quant[1]
    for q in (1, 5, 30, 49, 50, 85, 100):
        buf = io.BytesIO()
        Image.fromarray(cr.fr.noise_rgb(1, 32, 32)).save(buf, format="JPEG", quality=q, subsampling=2)
        theirs = Image.open(buf).quantization
        for mine, k in zip(ref.quant_tables(q), (0, 1)):
            assert sorted(mine.tolist()) == sorted(theirs[k]), q


def _pillow_luma_error(Y, q):
    """the mean absolute error of Pillow's own encoder on the plane saved as mode L at quality q"""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(Y, "L").save(buf, format="JPEG", quality=q)
    back = np.asarray(Image.open(buf).convert("L"), np.int64)
    return np.abs(back - Y.astype(np.int64)).mean()


@pytest.mark.parametrize("q", [30, 85, 100])
def test_pillow_opens_every_file_and_finds_the_luma(q):
    """Every reference file opens in Pillow 12 (libjpeg-turbo) with the right size and mode; the decoded luma's mean absolute error against the
    source Y plane is at most 1.05 times the error of Pillow's own encoder on the same plane at the same quality. Measured ratios (ours / theirs,
    over the scenes with a non-zero error of theirs): 1.000 .. 1.000 at each of the three qualities -- libjpeg-turbo's default forward transform is
    the same Loeffler-Ligtenberg-Moschytz form, so both encoders quantise the same integers (the test prints every figure; DESIGN 4y quotes them)."""
    Image = pytest.importorskip("PIL.Image")
    ratios = []
    for name in SCENES:
        data, _ = _encode(name, q)
        im = Image.open(io.BytesIO(data))
        fmt, planes, rect = SCENES[name]
        assert im.format == "JPEG" and im.size == (rect[2], rect[3]) and im.mode == "RGB"
        im.draft("YCbCr", im.size)
        got = np.asarray(im.convert("YCbCr"), np.int64)[..., 0]
        Y = ref.item_planes(fmt, "bt601", True, planes, rect)[0]
        ours, theirs = np.abs(got - Y.astype(np.int64)).mean(), _pillow_luma_error(Y, q)
        print("quality {} {}: ours {:.4f} theirs {:.4f}".format(q, name, ours, theirs))
        assert ours <= 1.05 * theirs + 1e-12, (name, q, ours, theirs)
        if theirs > 0:
            ratios.append(ours / theirs)
    print("quality {}: ratios {:.3f} .. {:.3f}".format(q, min(ratios), max(ratios)))


def test_an_rgb_path_file_opens_too():
    """a limited-range BT.709 NV12 frame and a BGR frame go through RGB8: the files open, and the decoded picture is close to the frame's RGB"""
    Image = pytest.importorskip("PIL.Image")
    h, w = rr.SIZES[1]
    for fmt, space in (("nv12", ("bt709", False)), ("bgr24", ("bt601", True))):
        planes = cr.noise_planes(fmt, 7, h, w)
        smooth = [np.sort(p, axis=1) for p in planes]          # (noise is no picture: sorted rows are one)
        data, _ = ref.encode_item(fmt, space[0], space[1], smooth, (0, 0, w, h), 95)
        im = Image.open(io.BytesIO(data))
        assert im.size == (w, h)
        rgb = cr.rgb_of(fmt, space[0], space[1], cr.channels(fmt, smooth))
        assert np.abs(np.asarray(im.convert("RGB"), np.int64) - rgb).mean() < 6.0


def test_the_scenes_tell_the_mistakes_apart():
    for mistake in ref.MISTAKES:
        differs = [name for name, q in _all() if _encode(name, q, mistake)[0] != _encode(name, q)[0]]
        assert differs, mistake


def test_the_scenes_contain_every_case_of_the_coder():
    stats = [_encode(name, q)[1] for name, q in _all()]
    assert any(s["stuffed"] > 0 for s in stats)
    assert any(s["zrl"] > 0 for s in stats)
    assert any(s["eob_only"] > 0 for s in stats)
    board = _encode("checkerboard", 100)[1]
    assert board["dc_cat"] == 11 and board["ac_cat"] == 10
    assert any(s["mcu_rows"] > 8 for s in stats)
    assert any(s["mcus_per_row"] > 64 for s in stats)
    assert {(s["mcu_rows"], s["mcus_per_row"]) for s in stats} >= {(1, 1), (1, 2), (3, 3), (2, 66), (13, 17)}


def test_placement_is_a_prefix_sum():
    res, totals = ref.place([700, -1, 1000, -2, 33, -3], 1760)
    assert res.tolist() == [[0, 700, 0, 0], [0, 0, 1, 0], [704, 1000, 0, 0], [0, 0, 2, 0], [1712, 33, 0, 0], [0, 0, 3, 0]]
    assert totals.tolist() == [3, 2, 1745, 0]
    res, totals = ref.place([700, 1000, 33], 1703)            # one byte short of the second: the third is judged by the rule, and does not fit either
    assert res[:, 2].tolist() == [0, 3, 3] and res[:, 0].tolist() == [0, 704, 1712] and totals.tolist() == [1, 2, 700, 0]


def test_the_index_statement():
    index = [[0, 3, 11, 21, 30, 40, 0, 0], [-1, 0, 0, 0, 0, 0, 0, 0], [2, 0, 0, 0, 8, 8, 0, 0], [1, 1, 100, 90, 40, 8, 0, 0], [1, 2, 0, 0, 16, 16, 0, 0],
             [0, 0, 0, 0, 16, 17, 0, 0]]
    got = ref.items_from_index(index, rr.SIZES, True, [1, 1, 1, 1, 0, 1], 4)
    assert got == [(0, (0, 10, 20, 31, 41)), (1, None), (2, None), (2, None), (1, None), (3, None)]
    assert ref.items_from_index(index, rr.SIZES, False, None, 6)[0] == (0, (0, 11, 21, 30, 40))


# ---------------------------------------------------------------------------------------------------------------- host validation
def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "demonet_hip.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %d %d\\n", sizeof(dn_jpeg_item), sizeof(dn_jpeg_header), offsetof(dn_jpeg_item, quality), '
                   'offsetof(dn_jpeg_item, seg0), DN_JPEG_MAX_ITEMS, DN_JPEG_HEADER_BYTES);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert a == [32, 16, _lib.JpegItem.quality.offset, _lib.JpegItem.seg0.offset, jpeg.MAX_ITEMS, jpeg.HEADER_BYTES]
    assert C.sizeof(_lib.JpegItem) == 32 and C.sizeof(_lib.JpegHeader) == 16 and ref.HEADER_BYTES == jpeg.HEADER_BYTES == 613


def test_the_constructor_refuses():
    for kw in (dict(items=0), dict(items=8193), dict(items=True), dict(items="4"), dict(arena_bytes=0), dict(arena_bytes=2 ** 31), dict(arena_bytes=1.5),
               dict(quality=0), dict(quality=101), dict(quality=85.0), dict(max_segments=0), dict(max_segments=2 ** 31)):
        a = dict(items=4, device="cpu", arena_bytes=1 << 20)
        a.update(kw)
        with pytest.raises(ValueError):
            jpeg.JpegEncoder(**a)
    enc = jpeg.JpegEncoder(4, "cpu", 1 << 20)
    assert (enc.capacity, enc.quality, enc.max_segments) == (4, 85, 4 * 68)


def test_set_refuses_on_the_host():
    sizes = rr.SIZES

    def records(items, yuv=True, capacity=4, quality=85, max_segments=64):
        return jpeg.item_records(items, sizes, yuv, capacity, quality, max_segments)
    raw, norm, seg = records([jpeg.Item(0), (1, (2, 4, 33, 47), 30), 1])
    assert norm == [(0, (0, 0, 260, 200), 85), (1, (2, 4, 33, 47), 30), (1, (0, 0, 131, 97), 85)] and seg == 13 + 3 + 7
    head = _lib.JpegHeader.from_buffer_copy(raw[:16])
    items = (_lib.JpegItem * 4).from_buffer_copy(raw[16:])
    assert (head.n_items, head.n_segments) == (3, 23) and len(raw) == 16 + 4 * 32
    assert [(i.frame, i.x0, i.y0, i.width, i.height, i.quality, i.seg0) for i in items] == [
        (0, 0, 0, 260, 200, 85, 0), (1, 2, 4, 33, 47, 30, 13), (1, 0, 0, 131, 97, 85, 16), (-1, 0, 0, 0, 0, 0, 23)]
    bad = [("a list", 5), ("capacity", [0] * 5), ("expected an Item", [(0, None, 85, 1)]), ("expected an Item", ["0"]), ("must be an int", [jpeg.Item(0.0)]),
           ("out of range", [2]), ("out of range", [-1]), ("four ints", [(0, (0, 0, 8))]), ("four ints", [(0, (0, 0, 8.0, 8))]), ("a side takes", [(0, (0, 0, 0, 8))]),
           ("a side takes", [(0, (0, 0, 8, 32769))]), ("outside its frame", [(0, (254, 0, 8, 8))]), ("outside its frame", [(1, (0, 90, 8, 8))]),
           ("outside its frame", [(0, (-2, 0, 8, 8))]), ("odd origin", [(0, (1, 0, 8, 8))]), ("odd origin", [(0, (0, 3, 8, 8))]),
           ("quality", [(0, None, 0)]), ("quality", [(0, None, 101)]), ("quality", [(0, None, 50.0)])]
    for match, items in bad:
        with pytest.raises(ValueError, match=match):
            records(items)
    records([(0, (1, 3, 8, 8))], yuv=False)                       # packed RGB takes odd origins
    with pytest.raises(ValueError, match="max_segments"):
        records([0, 0, 0, 0], max_segments=51)
    assert records([0, 0, 0, 0], max_segments=52)[2] == 52
    big = jpeg.item_records([(0, (0, 0, 32768, 32768))], [(40000, 40000)], True, 1, 85, 2048)
    assert big[2] == 2048
    enc = jpeg.JpegEncoder(4, "cpu", 1 << 20)
    with pytest.raises(ValueError, match="expected a FrameBatch"):
        enc.set([0], object())
    with pytest.raises(ValueError, match="expected a FrameBatch"):
        enc.encode(object())
    with pytest.raises(ValueError, match="nothing was encoded"):
        enc.files()
