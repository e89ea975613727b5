"""Regions of video surfaces as input, CPU side (-m "not gpu"): the ABI of dn_region / dn_forward_regions, the records of RegionTable field by field,
every refusal by name with nothing launched, FrameSlicer's table against tile_grid, and the proof that the region set of the GPU tests tells the
right sampler from three wrong ones (tests/regions_ref.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import frames_ref as fr
import regions_ref as rr
from demonet_amd import _lib, models
from demonet_amd.frames import FrameBatch, RegionTable, check_regions, forward_regions, region_records
from demonet_amd.sliced import FrameSlicer, tile_grid, track_sliced_frames
from demonet_amd.track import ByteTracker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "demonet_hip.h")
SIZE = 160


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_forward_regions_is_declared_exported_and_bound():
    txt = open(HEADER).read()
    assert re.search(r"DN_API\s+int\s+dn_forward_regions\s*\(", txt)
    assert re.search(r"^#define DN_ABI_VERSION 1$", txt, re.M)
    assert "TRUST BOUNDARY: AS FOR dn_frame" in txt
    assert "dn_forward_regions" in _lib.EXPORTS
    if not os.path.exists(_lib.LIB_PATH):
        from demonet_amd import build
        build.build(verbose=False)
    assert hasattr(C.CDLL(_lib.LIB_PATH), "dn_forward_regions")
    assert _lib.DN_REGION_HFLIP == 1 and _lib.DN_ABI_VERSION == 1


def test_region_record_layout_matches_c(tmp_path):
    src = tmp_path / "rg.c"
    fields = ("frame", "x0", "y0", "width", "height", "flags", "reserved")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "demonet_hip.h"\n'
                   'int main(){printf("%zu ' + "%zu " * len(fields) + '%d\\n", sizeof(dn_region), '
                   + ", ".join("offsetof(dn_region, {})".format(f) for f in fields) + ', DN_REGION_HFLIP);return 0;}\n')
    exe = tmp_path / "rg"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    R = _lib.Region
    assert a[0] == 32 == C.sizeof(R)
    assert a[1:8] == [getattr(R, f).offset for f in fields] == [0, 4, 8, 12, 16, 20, 24]
    assert a[8] == 1


# ---------------------------------------------------------------------------------------------------------------- records and refusals
def test_records_of_valid_regions():
    rec, norm = region_records(rr.REGIONS, rr.SIZES, len(rr.REGIONS))
    for r, (f, x0, y0, w, h, flip) in zip(rec, rr.REGIONS):
        assert (r.frame, r.x0, r.y0, r.width, r.height, r.flags, list(r.reserved)) == (f, x0, y0, w, h, flip, [0, 0])
    assert norm == [(f, x0, y0, w, h, bool(flip)) for f, x0, y0, w, h, flip in rr.REGIONS]
    rec, norm = region_records([(1, 2, 3, 4, 5)], rr.SIZES, 1)          # the five-tuple form: not mirrored
    assert (rec[0].frame, rec[0].x0, rec[0].y0, rec[0].width, rec[0].height, rec[0].flags) == (1, 2, 3, 4, 5, 0) and norm == [(1, 2, 3, 4, 5, False)]
    raw = bytes(region_records([(1, 2, 3, 4, 5, True)], rr.SIZES, 1)[0])
    assert np.frombuffer(raw, dtype=np.int32).tolist() == [1, 2, 3, 4, 5, 1, 0, 0]
    # ... and a valid set() on a CPU table ends where the device would begin: there is no CPU path
    t = RegionTable(1, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.set([(0, 0, 0, 260, 200)], rr.SIZES)
    assert t.table is None and t.regions == [] and t.frame_sizes == {}


BAD = [("frame-out-of-range", [(0, 0, 0, 4, 4), (2, 0, 0, 4, 4)], r"region 1: frame index 2 out of range \(2 frames\)"),
       ("negative-frame", [(-1, 0, 0, 4, 4), (0, 0, 0, 4, 4)], r"region 0: frame index -1"),
       ("zero-width", [(0, 0, 0, 4, 4), (0, 5, 5, 0, 4)], r"region 1: bad size 0 x 4"),
       ("negative-height", [(0, 5, 5, 3, -2), (0, 0, 0, 4, 4)], r"region 0: bad size 3 x -2"),
       ("negative-x0", [(0, 0, 0, 4, 4), (0, -1, 0, 4, 4)], r"region 1: the rectangle x -1 \.\. 3.*leaves frame 0 of 260 x 200"),
       ("negative-y0", [(1, 0, -7, 4, 4), (0, 0, 0, 4, 4)], r"region 0: the rectangle.*y -7 \.\. -3.*leaves frame 1 of 131 x 97"),
       ("one-column-too-wide", [(0, 0, 0, 4, 4), (0, 100, 0, 161, 4)], r"region 1: the rectangle x 100 \.\. 261.*leaves frame 0"),
       ("one-row-too-tall", [(0, 0, 0, 4, 4), (1, 0, 90, 4, 8)], r"region 1: the rectangle.*y 90 \.\. 98.*leaves frame 1"),
       ("width-and-height-swapped", [(1, 0, 0, 97, 131), (0, 0, 0, 4, 4)], r"region 0: .*leaves frame 1"),
       ("beyond-int32", [(0, 0, 0, 4, 4), (0, 2 ** 31, 0, 4, 4)], r"region 1: .*int32"),
       ("sum-beyond-int32", [(0, 2 ** 31 - 2, 0, 4, 4), (0, 0, 0, 4, 4)], r"region 0: .*int32"),
       ("float-coordinate", [(0, 0.0, 0, 4, 4), (0, 0, 0, 4, 4)], r"region 0: .*must be ints"),
       ("four-fields", [(0, 0, 0, 4, 4), (0, 0, 4, 4)], r"region 1: expected \(frame, x0, y0, w, h"),
       ("wrong-count", [(0, 0, 0, 4, 4)], r"expected 2 regions, got 1"),
       ("a-tensor-not-a-list", torch.zeros((2, 6), dtype=torch.int32), r"expected a list")]


@pytest.mark.parametrize("what,regions,msg", BAD, ids=[b[0] for b in BAD])
def test_set_refuses_bad_regions(what, regions, msg):
    t = RegionTable(2, "cpu")
    with pytest.raises(ValueError, match=msg):
        t.set(regions, rr.SIZES)
    assert t.table is None and t.regions == [] and t.frame_sizes == {} and t._host is None


def test_constructor_refuses_a_bad_count():
    for n in (0, -1, 2.0):
        with pytest.raises(ValueError):
            RegionTable(n, "cpu")


@pytest.fixture(scope="module")
def cpu_model():
    return models.ssd_lite_mobilenet_v2(image_size=SIZE, num_classes=3).eval()


def _fake_set_batch(sizes, device="cpu"):
    """a FrameBatch that looks set without a device: check_regions reads the table's presence and the sizes only"""
    b = FrameBatch(len(sizes), device)
    b.table, b.sizes = torch.zeros(len(sizes) * 48, dtype=torch.uint8), list(sizes)
    return b


def _fake_set_table(regions, sizes, device="cpu"):
    t = RegionTable(len(regions), device)
    _, t.regions = region_records(regions, sizes, len(regions))
    t.table = torch.zeros(len(regions) * 32, dtype=torch.uint8)
    t.frame_sizes = {f: tuple(sizes[f]) for f in {r[0] for r in t.regions}}
    return t


def test_forward_regions_refuses_by_name_before_any_launch(cpu_model):
    m = cpu_model
    batch = _fake_set_batch(rr.SIZES)
    table = _fake_set_table(rr.REGIONS, rr.SIZES)
    with pytest.raises(ValueError, match="expected a FrameBatch"):
        forward_regions(m, torch.zeros(3), table)
    with pytest.raises(ValueError, match="expected a RegionTable"):
        forward_regions(m, batch, [(0, 0, 0, 4, 4)])
    with pytest.raises(ValueError, match="FrameBatch names no frames yet"):
        forward_regions(m, FrameBatch(2, "cpu"), table)
    with pytest.raises(ValueError, match="RegionTable names no regions yet"):
        forward_regions(m, batch, RegionTable(3, "cpu"))
    with pytest.raises(ValueError, match="the RegionTable is on meta, the FrameBatch on cpu"):
        forward_regions(m, batch, _fake_set_table(rr.REGIONS, rr.SIZES, "meta"))
    with pytest.raises(ValueError, match="the FrameBatch is on meta, the model on cpu"):
        forward_regions(m, _fake_set_batch(rr.SIZES, "meta"), table)
    # stale sizes: the batch now names a smaller frame 1 -- a region validated against the old size must not reach the device
    with pytest.raises(ValueError, match=r"stale sizes: the regions of frame 1 were validated against \(97, 131\).*now holds \(96, 131\)"):
        forward_regions(m, _fake_set_batch([rr.SIZES[0], (96, 131)]), table)
    with pytest.raises(ValueError, match=r"stale sizes: the regions of frame 1.*1 frames"):
        forward_regions(m, _fake_set_batch(rr.SIZES[:1]), table)
    # only the frames the regions name are compared: a table over frame 0 alone does not care what frame 1 became
    only0 = _fake_set_table([r for r in rr.REGIONS if r[0] == 0], rr.SIZES)
    check_regions("x", m, _fake_set_batch([rr.SIZES[0], (10, 10)]), only0)
    # everything in order: the call ends where the device would begin
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        forward_regions(m, batch, table)


# ---------------------------------------------------------------------------------------------------------------- FrameSlicer
def test_slicer_table_is_the_tile_grid_plus_the_whole_frame(cpu_model):
    m = cpu_model
    sizes = [(200, 260), (97, 131)]           # the second one is smaller than the tile in both directions
    for full in (True, False):
        for tile in (None, (120, 140)):
            s = FrameSlicer(m, sizes, tile=tile, full_image=full)
            th0, tw0 = (SIZE, SIZE) if tile is None else tile
            want, offsets, gb = [], [], [0]
            for f, (h, w) in enumerate(sizes):
                origins, th, tw = tile_grid(h, w, th0, tw0, 0.25)
                assert (th, tw) == (min(th0, h), min(tw0, w))
                want += [(f, x, y, tw, th, False) for x, y in origins]
                offsets += [(float(x), float(y)) for x, y in origins]
                if full:
                    want.append((f, 0, 0, w, h, False))
                    offsets.append((0.0, 0.0))
                gb.append(len(want))
            assert s.regions == want and s.offsets == offsets and s.group_begin == gb
            assert (s.S, s.G, s.D) == (len(want), 2, m.detections_per_img) and s.table is None
    s = FrameSlicer(m, sizes)
    assert s.group_begin == [0, 5, 7]        # 260 x 200 at tile 160, overlap 0.25: xs [0, 100], ys [0, 40] + the frame; the small frame: itself twice
    assert s.regions[5:] == [(1, 0, 0, 131, 97, False)] * 2
    region_records(s.regions, sizes, s.S)


def test_slicer_refusals(cpu_model):
    m = cpu_model
    with pytest.raises(ValueError, match="FrameSlicer: tile must be positive"):
        FrameSlicer(m, rr.SIZES, tile=0)
    with pytest.raises(ValueError, match="FrameSlicer: metric"):
        FrameSlicer(m, rr.SIZES, metric="giou")
    with pytest.raises(ValueError, match="FrameSlicer: max_tiles_per_forward"):
        FrameSlicer(m, rr.SIZES, max_tiles_per_forward=0)
    with pytest.raises(ValueError, match="overlap"):
        FrameSlicer(m, rr.SIZES, overlap=1.0)
    with pytest.raises(ValueError, match="no frame sizes"):
        FrameSlicer(m, [])
    with pytest.raises(ValueError, match=r"FrameSlicer: 1025 sources"):      # the existing merge limits: 1 024 tiles + the frame
        FrameSlicer(m, [(1, 1024)], tile=1, overlap=0.0)
    s = FrameSlicer(m, rr.SIZES)
    with pytest.raises(ValueError, match="expected a FrameBatch"):
        s(torch.zeros(3))
    with pytest.raises(ValueError, match="names no frames yet"):
        s(FrameBatch(2, "cpu"))
    with pytest.raises(ValueError, match="stale sizes"):
        s(_fake_set_batch([rr.SIZES[0], (96, 131)]))
    with pytest.raises(ValueError, match="the FrameBatch is on meta, the model on cpu"):
        s(_fake_set_batch(rr.SIZES, "meta"))
    assert s.table is None                    # nothing was allocated
    tracker = ByteTracker.__new__(ByteTracker)
    with pytest.raises(ValueError, match="tracker must be a ByteTracker"):
        track_sliced_frames(m, _fake_set_batch(rr.SIZES), object(), s)
    with pytest.raises(ValueError, match="slicer must be a FrameSlicer of this model"):
        track_sliced_frames(m, _fake_set_batch(rr.SIZES), tracker, object())
    s.D = 513
    with pytest.raises(ValueError, match=r"track_sliced_frames: detections_per_img = 513 rows per frame, the tracker takes at most 512"):
        track_sliced_frames(m, _fake_set_batch(rr.SIZES), tracker, s)


# ---------------------------------------------------------------------------------------------------------------- the region set discriminates
@pytest.fixture(scope="module")
def planes():
    return [fr.noise_yuv(900 + f, h, w) for f, (h, w) in enumerate(rr.SIZES)]


def test_the_tap_by_tap_sampler_equals_resize_of_the_crop(planes):
    """the header's consequence, in numpy: sampling the region tap by tap from the planes = converting the frame, cutting, mirroring, resizing"""
    for matrix, full in (("bt709", False), ("bt601", True)):
        rgb = [fr.planes_to_rgb(Y, U, V, matrix, full) for Y, U, V in planes]
        for reg in rr.REGIONS:
            Y, U, V = planes[reg[0]]
            got = rr.sample(Y, U, V, matrix, full, reg, SIZE, SIZE)
            want = rr.resize_u8(rr.crop(rgb[reg[0]], reg), SIZE, SIZE)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32)), reg


def test_identity_size_regions_are_a_plain_conversion(planes):
    rgb = fr.planes_to_rgb(*planes[0], "bt709", False)
    for reg in rr.REGIONS:
        if reg[3:5] == (SIZE, SIZE):
            want = rr.crop(rgb, reg).astype(np.float32).transpose(2, 0, 1) / np.float32(255)
            assert np.array_equal(rr.resize_u8(rr.crop(rgb, reg), SIZE, SIZE).view(np.int32), want.view(np.int32))


def test_the_region_set_tells_the_wrong_samplers_from_the_right_one(planes):
    worst = {}
    for mistake in rr.MISTAKES:
        fractions = []
        for reg in rr.REGIONS:
            Y, U, V = planes[reg[0]]
            right = rr.sample(Y, U, V, "bt709", False, reg, SIZE, SIZE)
            wrong = rr.sample(Y, U, V, "bt709", False, reg, SIZE, SIZE, **{mistake: True})
            fractions.append(float((right.view(np.int32) != wrong.view(np.int32)).mean()))
        worst[mistake] = max(fractions)
        print("\n{}: fraction of differing elements per region: {}".format(mistake, " ".join("{:.3f}".format(x) for x in fractions)))
    assert all(v > 0.01 for v in worst.values()), worst
