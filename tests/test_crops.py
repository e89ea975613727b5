"""CPU tests (-m "not gpu") of the object crops (dn_crop_objects, demonet_amd/crops.py): the reference tests/crops_ref.py against rectangles computed
by hand from the header's rules, the numbering and the capacity, the power of the box set the GPU tests run (every deliberate mistake changes its
result), the two reference samplers against each other, the C struct against its ctypes mirror, and every ValueError that needs no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import crops_ref as cr
import frames_ref as fr
import regions_ref as rr
from demonet_amd import _lib, crops
from demonet_amd.frames import FrameBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 260, 200
NAN, INF = float("nan"), float("inf")
EXAMPLE = (10.2, 20.7, 30.1, 40.0)


# ---------------------------------------------------------------------------------------------------------------- rectangles by hand
@pytest.mark.parametrize("box,kw,want", [
    (EXAMPLE, {}, (10, 20, 21, 20)),                                        # the header's worked example
    (EXAMPLE, dict(margin=0.1), (8, 18, 25, 24)),                           # 8.21 .. 32.09, 18.77 .. 41.93
    (EXAMPLE, dict(square=True), (10, 20, 21, 21)),                         # side 19.9 about (20.15, 30.35): y 20.4 .. 40.3
    (EXAMPLE, dict(margin=0.1, square=True), (8, 18, 25, 25)),              # side 23.88: y 18.41 .. 42.29
    ((-5.5, 50.0, 20.5, 90.0), {}, (0, 50, 21, 40)),                        # over the left edge
    ((240.0, 10.0, 275.0, 60.0), {}, (240, 10, 20, 50)),                    # right
    ((100.0, -8.0, 140.0, 12.5), {}, (100, 0, 40, 13)),                     # top
    ((100.0, 180.0, 150.0, 215.0), {}, (100, 180, 50, 20)),                 # bottom
    ((-30.0, 10.0, -2.0, 40.0), {}, None), ((262.0, 10.0, 290.0, 40.0), {}, None),      # wholly outside, each side
    ((10.0, -40.0, 40.0, -1.0), {}, None), ((10.0, 201.0, 40.0, 230.0), {}, None),
    ((-9.0, 5.0, 0.0, 50.0), {}, None), ((260.0, 5.0, 270.0, 50.0), {}, None),          # touching from outside: xb > 0 and xa < W are strict
    ((5.0, -9.0, 50.0, 0.0), {}, None), ((5.0, 200.0, 50.0, 210.0), {}, None),
    ((259.5, 199.5, 300.0, 300.0), {}, (259, 199, 1, 1)),                   # the last pixel
    ((NAN, 10.0, 50.0, 60.0), {}, None), ((10.0, NAN, 50.0, 60.0), {}, None), ((10.0, 10.0, INF, 60.0), {}, None),
    ((-INF, 10.0, 50.0, 60.0), {}, None), ((10.0, 10.0, 50.0, -INF), {}, None),
    ((40.0, 40.0, 40.0, 80.0), {}, None), ((40.0, 40.0, 80.0, 40.0), {}, None),         # zero extent
    ((60.0, 40.0, 50.0, 80.0), {}, None), ((40.0, 80.0, 50.0, 70.0), {}, None),         # negative extent
    ((-3e38, 10.0, 3e38, 60.0), {}, None),                                  # w overflows: inf * 0 is NaN
    ((-3e38, 10.0, 3e38, 60.0), dict(margin=0.5), None),                    # ... and the margin makes the edges infinite
    ((-2e38, 10.0, 1e38, 60.0), {}, (0, 10, 260, 50)),                      # finite and huge: clamped
    ((-2e38, 10.0, 1e38, 60.0), dict(margin=1.0), None),                    # the same box overflows under the margin (-2e38 - 3e38)
    ((-2e38, 10.0, 1e38, 60.0), dict(square=True), (0, 0, 260, 200)),       # side 3e38 about (-5e37, 35): y -1.5e38 .. 1.5e38, finite: all of the frame
    (EXAMPLE, dict(min_size=(20, 21)), (10, 20, 21, 20)),                   # min_size is (height, width): exactly met
    (EXAMPLE, dict(min_size=(21, 21)), None), (EXAMPLE, dict(min_size=(20, 22)), None),
    (EXAMPLE, dict(min_size=(1, 1)), (10, 20, 21, 20)),
])
def test_rectangles_by_hand(box, kw, want):
    assert cr.rect(box, W, H, cr.params(**kw)) == want


def test_the_first_edge_is_clamped_into_the_frame_and_the_second_behind_it():
    p = cr.params()
    assert cr.rect((259.2, 10.0, 259.6, 20.0), W, H, p) == (259, 10, 1, 10)
    assert cr.rect((-0.5, -0.5, 0.25, 0.25), W, H, p) == (0, 0, 1, 1)
    assert cr.rect((12.0, 13.0, 14.0, 15.0), W, H, p) == (12, 13, 2, 2)      # integers: floor and ceil change nothing
    assert cr.rect((100.2, 100.3, 100.6, 100.8), W, H, p) == (100, 100, 1, 1)
    assert cr.rect((130.1, 96.2, 130.9, 96.8), 131, 97, p) == (130, 96, 1, 1)
    assert cr.rect((125.5, 90.2, 140.0, 100.0), 131, 97, p) == (125, 90, 6, 7)


# ---------------------------------------------------------------------------------------------------------------- numbering, capacity, counts, select
def _rows(index, kept):
    return [tuple(int(v) for v in r) for r in index[:kept]]


def test_order_capacity_and_the_rows_behind_kept():
    boxes, counts = cr.boxes_array()
    sizes = rr.SIZES
    index, kept, dropped = cr.rects(boxes, counts, sizes, None, cr.params(capacity=64))
    rows = _rows(index, kept)
    assert dropped == 0 and kept == len(rows) and kept >= 16
    assert rows == sorted(rows, key=lambda r: (r[0], r[1]))                  # stream ascending, row ascending
    assert {r[0] for r in rows} == {0, 1}
    assert all(r[6:] == (0, 0) for r in rows)
    assert rows[0] == (0, 0, 10, 20, 21, 20, 0, 0)
    assert all(r[1] < counts[r[0]] for r in rows)                           # nothing from behind the counts
    assert (index[kept:] == np.asarray([-1, 0, 0, 0, 0, 0, 0, 0])).all()
    small, k5, d5 = cr.rects(boxes, counts, sizes, None, cr.params(capacity=5))
    assert k5 == 5 and d5 == kept - 5 and small.shape == (5, 8) and _rows(small, 5) == rows[:5]
    one, k1, d1 = cr.rects(boxes, counts, sizes, None, cr.params(capacity=kept))
    assert k1 == kept and d1 == 0 and (one[:, 0] >= 0).all()


def test_counts_negative_and_above_d():
    boxes, _ = cr.boxes_array()
    sizes = rr.SIZES
    p = cr.params(capacity=64)
    none = cr.rects(boxes, [-3, 0], sizes, None, p)
    assert none[1:] == (0, 0) and (none[0][:, 0] == -1).all()
    full = cr.rects(boxes, [cr.D, cr.D], sizes, None, p)
    above = cr.rects(boxes, [cr.D + 100, 2 ** 31 - 1], sizes, None, p)
    assert above[1:] == full[1:] and np.array_equal(above[0], full[0])
    usual = cr.rects(boxes, cr.COUNTS, sizes, None, p)
    assert full[1] > usual[1]                                               # the rows behind COUNTS hold boxes that would be kept


def test_select_skips_rows():
    boxes, counts = cr.boxes_array()
    p = cr.params(capacity=64)
    index, kept, _ = cr.rects(boxes, counts, rr.SIZES, None, p)
    rows = _rows(index, kept)
    select = np.ones((2, cr.D), dtype=np.uint8)
    select[0, 0] = 0
    select[1, 2] = 0
    got, k, _ = cr.rects(boxes, counts, rr.SIZES, select, p)
    assert _rows(got, k) == [r for r in rows if (r[0], r[1]) not in ((0, 0), (1, 2))]
    select[:] = 0
    select[1, 2] = 7                                                        # any non-zero byte selects
    got, k, _ = cr.rects(boxes, counts, rr.SIZES, select, p)
    assert _rows(got, k) == [r for r in rows if (r[0], r[1]) == (1, 2)]


# ---------------------------------------------------------------------------------------------------------------- the GPU tests' set has power
@pytest.fixture(scope="module")
def frames():
    planes = [fr.noise_yuv(3 + i, h, w) for i, (h, w) in enumerate(rr.SIZES)]
    return planes, [fr.planes_to_rgb(Y, U, V, "bt709", False) for Y, U, V in planes]


def _differs(a, b):
    return any(x.shape != y.shape or x.tobytes() != y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("mistake", cr.MISTAKES)
def test_every_mistake_changes_the_result_of_the_gpu_tests_set(mistake, frames):
    _, rgbs = frames
    boxes, counts = cr.boxes_array()
    changed = [name for name, p in cr.CONFIGS.items()
               if _differs(cr.step(rgbs, boxes, counts, rr.SIZES, None, p), cr.step(rgbs, boxes, counts, rr.SIZES, None, p, mistake))]
    assert changed, mistake
    if mistake == "reciprocal":
        assert "imagenet-f32" in changed                                    # fp32 output is where a reciprocal shows
        assert not any(np.asarray(cr.CONFIGS[n].std).tolist() == [1.0] * 3 for n in changed)
    if mistake == "clamp_first":
        assert "margin" in changed


def test_the_set_holds_what_the_gpu_tests_promise():
    boxes, counts = cr.boxes_array()
    index, kept, dropped = cr.rects(boxes, counts, rr.SIZES, None, cr.CONFIGS["f32-16x8"])
    rows = _rows(index, kept)
    sizes = {r[4:6] for r in rows}
    assert (8, 16) in sizes                                                 # exactly the patch: the one-tap path
    assert (1, 1) in sizes                                                  # a single pixel, upscaled
    assert (1, 0, 96, 131, 1, 0, 0) in [r[:1] + r[2:] for r in rows]        # the odd frame's whole last row
    assert (1, 130, 0, 1, 97, 0, 0) in [r[:1] + r[2:] for r in rows]        # ... and last column
    assert (1, 130, 96, 1, 1, 0, 0) in [r[:1] + r[2:] for r in rows]
    assert dropped == 0
    _, k, d = cr.rects(boxes, counts, rr.SIZES, None, cr.CONFIGS["overflow"])
    assert k == 5 and d > 0
    _, kmin, _ = cr.rects(boxes, counts, rr.SIZES, None, cr.CONFIGS["min-size"])
    assert 0 < kmin < kept


def test_both_reference_samplers_agree(frames):
    planes, rgbs = frames
    boxes, counts = cr.boxes_array()
    for name in ("f32-16x8", "imagenet-f16", "f32-7x5"):
        p = cr.CONFIGS[name]
        index, kept, _ = cr.rects(boxes, counts, rr.SIZES, None, p)
        a, b = cr.patches(rgbs, index, kept, p), cr.patches_sampled(planes, "bt709", False, index, kept, p)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name


def test_identity_normalisation_is_the_region_input(frames):
    _, rgbs = frames
    p = cr.CONFIGS["f32-16x8"]
    got = cr.normalise(rr.resize_u8(rr.crop(rgbs[0], (0, 40, 30, 8, 16, 0)), 16, 8), p)
    want = rgbs[0][30:46, 40:48].transpose(2, 0, 1).astype(np.float32) / np.float32(255)      # the patch-size rectangle: a plain conversion
    assert got.tobytes() == np.ascontiguousarray(want).tobytes()


def test_random_boxes_number_across_waves_and_streams():
    sizes = rr.SIZES + [rr.SIZES[0]]
    boxes, counts, select = cr.random_boxes(11, sizes, 512)
    index, kept, dropped = cr.rects(boxes, counts, sizes, select, cr.params((4, 4), capacity=2048))
    per_stream = [int((index[:kept, 0] == b).sum()) for b in range(3)]
    assert all(n > 64 for n in per_stream) and dropped == 0, per_stream
    assert (select == 0).sum() > 100


# ---------------------------------------------------------------------------------------------------------------- the C struct
def test_crop_params_layout_matches_c(tmp_path):
    fields = [n for n, _ in _lib.CropParams._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "demonet_hip.h"\nint main(){printf("%zu", sizeof(dn_crop_params));\n'
                   + "".join('printf(" %zu", offsetof(dn_crop_params, {}));\n'.format(f) for f in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert a[0] == C.sizeof(_lib.CropParams) == 64
    assert a[1:] == [getattr(_lib.CropParams, f).offset for f in fields]
    assert {"dn_crop_workspace_bytes", "dn_crop_objects"} <= set(_lib.EXPORTS)


# ---------------------------------------------------------------------------------------------------------------- validation without a device
@pytest.mark.parametrize("kw,match", [
    (dict(size=(0, 8)), r"size \(height, width\)\[0\] = 0"), (dict(size=(8, 1025)), r"\[1\] = 1025"), (dict(size=8), "must be a pair"),
    (dict(size=(8.0, 8)), "must be an int"), (dict(size=(8, 8, 8)), "must be a pair"),
    (dict(capacity=0), "capacity = 0"), (dict(capacity=8193), "capacity = 8193"), (dict(capacity=True), "capacity must be an int"),
    (dict(dtype=torch.bfloat16), "dtype must be"), (dict(dtype="half"), "dtype must be"),
    (dict(mean=(0.5, 0.5)), "mean must hold three"), (dict(mean=(0.5, NAN, 0.5)), "mean must be finite"), (dict(mean=(0.5, "x", 0.5)), "three numbers"),
    (dict(std=(1.0, 0.0, 1.0)), "std must be positive"), (dict(std=(1.0, -1.0, 1.0)), "std must be positive"), (dict(std=(1.0, INF, 1.0)), "std must be finite"),
    (dict(std=(1.0, 1e-60, 1.0)), "std must be positive in fp32"), (dict(mean=(1e39, 0.0, 0.0)), "finite in fp32"),
    (dict(margin=-0.1), "margin must be finite and >= 0"), (dict(margin=NAN), "margin must be finite"), (dict(margin=INF), "margin must be finite"),
    (dict(margin="wide"), "margin must be a number"),
    (dict(square=1), "square must be a bool"),
    (dict(min_size=(0, 1)), r"min_size \(height, width\)\[0\] = 0"), (dict(min_size=(1, 0)), r"\[1\] = 0"), (dict(min_size=3), "must be a pair"),
])
def test_cropper_arguments_are_refused_before_any_device_work(kw, match):
    with pytest.raises(ValueError, match=match):
        crops.crop_params(**kw)
    with pytest.raises(ValueError, match=match):
        crops.ObjectCropper(2, "cuda:0", **kw)          # (the arguments are checked before the device is touched: this machine has none)


def test_cropper_streams_and_device():
    for bad in (0, -1, 1025, 2.0, True):
        with pytest.raises(ValueError, match="streams"):
            crops.ObjectCropper(bad, "cuda:0")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crops.ObjectCropper(2, "cpu")


def test_crop_params_mirror_the_arguments():
    p = crops.crop_params(size=(128, 64), capacity=77, dtype=torch.float32, mean=(0.1, 0.2, 0.3), std=(0.5, 0.6, 0.7), margin=0.25, square=True,
                          min_size=(9, 5))
    assert (p.out_h, p.out_w, p.capacity, p.out_fp16, p.square, p.min_height, p.min_width) == (128, 64, 77, 0, 1, 9, 5)
    assert [np.float32(v) for v in p.mean] == [np.float32(v) for v in (0.1, 0.2, 0.3)] and np.float32(p.margin) == np.float32(0.25)
    assert list(p.reserved) == [0, 0] and crops.crop_params().out_fp16 == 1


def test_step_arguments_are_refused_on_the_host():
    cpu = torch.device("cpu")
    batch = FrameBatch(2, "cpu")
    boxes, counts = torch.zeros((2, 8, 4)), torch.zeros((2,), dtype=torch.int32)
    with pytest.raises(ValueError, match="names no frames yet"):
        crops.check_step(2, cpu, batch, boxes, counts)
    batch.table = torch.zeros(96, dtype=torch.uint8)       # (stands in for a table that was set: nothing here reaches a device)
    assert crops.check_step(2, cpu, batch, boxes, counts) == 8
    assert crops.check_step(2, cpu, batch, boxes, counts, torch.ones((2, 8), dtype=torch.uint8)) == 8
    assert crops.check_step(2, cpu, batch, boxes, counts, torch.ones((2, 8), dtype=torch.bool)) == 8
    with pytest.raises(ValueError, match="expected a FrameBatch"):
        crops.check_step(2, cpu, [batch], boxes, counts)
    with pytest.raises(ValueError, match="a FrameBatch of 2 frames, the cropper has 3"):
        crops.check_step(3, cpu, batch, boxes, counts)
    with pytest.raises(ValueError, match="the FrameBatch is on cpu, the cropper on cuda:0"):
        crops.check_step(2, torch.device("cuda:0"), batch, boxes, counts)
    with pytest.raises(ValueError, match=r"boxes must be \[B, d, 4\]"):
        crops.check_step(2, cpu, batch, boxes[..., :3], counts)
    with pytest.raises(ValueError, match=r"boxes must be \[B, d, 4\]"):
        crops.check_step(2, cpu, batch, None, counts)
    with pytest.raises(ValueError, match="3 streams of boxes"):
        crops.check_step(2, cpu, batch, torch.zeros((3, 8, 4)), counts)
    with pytest.raises(ValueError, match="513 rows per stream"):
        crops.check_step(2, cpu, batch, torch.zeros((2, 513, 4)), counts)
    with pytest.raises(ValueError, match="0 rows per stream"):
        crops.check_step(2, cpu, batch, torch.zeros((2, 0, 4)), counts)
    for bad_boxes in (boxes.double(), torch.zeros((2, 4, 8)).transpose(1, 2)):
        with pytest.raises(ValueError, match="contiguous torch.float32"):
            crops.check_step(2, cpu, batch, bad_boxes, counts)
    for bad_counts in (counts.long(), torch.zeros((3,), dtype=torch.int32), [0, 0]):
        with pytest.raises(ValueError, match="contiguous torch.int32"):
            crops.check_step(2, cpu, batch, boxes, bad_counts)
    for bad_select in (torch.ones((2, 8)), torch.ones((2, 7), dtype=torch.uint8), torch.ones((8, 2), dtype=torch.uint8).t()):
        with pytest.raises(ValueError, match="torch.uint8 or torch.bool"):
            crops.check_step(2, cpu, batch, boxes, counts, bad_select)
    with pytest.raises(ValueError, match="cropper must be an ObjectCropper"):
        crops.crop_objects(None, batch, object(), boxes, counts)
