"""Camera-motion compensation without a GPU: the C ABI of csrc/motion.hip against the header and gcc, the state-size arithmetic, every
refusal before a launch, and the reference itself -- tests/motion_ref.py pinned by closed forms, so that the bit-for-bit GPU tests of
tests/test_gpu_motion.py compare against something whose meaning is known."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import motion_ref as mr
import track_ref as tr
from demonet_amd import _lib
from demonet_amd import motion as dmotion
from demonet_amd.frames import FrameBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ("dn_motion_state_bytes", "dn_motion_reset", "dn_motion_estimate", "dn_track_compensate")
DN_E_INVALID, DN_E_UNSUPPORTED, DN_E_WORKSPACE = -1, -4, -3


def _library():
    if not os.path.exists(_lib.LIB_PATH):
        from demonet_amd import build
        build.build(verbose=False)
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------------- the boundary
def test_the_symbols_are_exported_declared_and_bound_and_the_struct_mirror_matches_gcc(tmp_path):
    L = _library()
    header = open(os.path.join(ROOT, "include", "demonet_hip.h")).read()
    declared = set(re.findall(r"DN_API\s+[\w\s\*]+?\b(dn_\w+)\s*\(", header))
    assert set(NAMES) <= set(_lib.EXPORTS)
    for n in NAMES:
        assert hasattr(L, n) and n in declared, n
    names = [n for n, _ in _lib.MotionParams._fields_]
    src = tmp_path / "mp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "demonet_hip.h"\nint main(){printf("%zu %zu", sizeof(dn_motion_params), '
                   'sizeof(dn_frame));' + "".join('printf(" %zu", offsetof(dn_motion_params, {}));'.format(n) for n in names) + "return 0;}\n")
    exe = tmp_path / "mp"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert a[0] == C.sizeof(_lib.MotionParams) == 32 and a[1] == C.sizeof(_lib.Frame) == 48
    assert a[2:] == [getattr(_lib.MotionParams, n).offset for n in names]
    assert "static_assert(sizeof(dn_motion_params) == 32" in header
    assert "only a transform that does not mix cx with cy" in header               # why rotation is left out is said where the semantics are


def test_state_size_is_host_arithmetic_and_matches_the_python_layout():
    L = _library()
    sb = lambda streams, **kw: L.dn_motion_state_bytes(streams, C.byref(dmotion.motion_params(**kw)))
    assert sb(1) == 16 + 16 * 98 + 2 * 144 * 256                                     # 14 x 7 blocks of 16 at radius 16 in 256 x 144
    assert sb(64) == 64 * sb(1)
    assert sb(3, max_size=(64, 96), block=8, radius=7) == 3 * (16 + 16 * (10 * 6) + 2 * 64 * 96)
    assert sb(2, max_size=(50, 100), block=8, radius=1) == 2 * (16 + 16 * (12 * 6) + 2 * 50 * 112)          # rows of 100 bytes lie 112 apart
    for kw in (dict(), dict(max_size=(64, 96), block=8, radius=7), dict(max_size=(50, 100), block=8, radius=1)):
        p = dmotion.motion_params(**kw)
        f = dmotion.state_fields(p)
        assert f["stride"] * 5 == L.dn_motion_state_bytes(5, C.byref(p)) and f["stride"] % 16 == 0
        assert f["vectors"][2][0] == dmotion.max_blocks(p) and f["thumbs"][0] == 16 + 16 * dmotion.max_blocks(p)
    assert sb(0) == 0 and sb(65536) == 0
    bad = dmotion.motion_params()
    bad.max_w = 513
    assert L.dn_motion_state_bytes(1, C.byref(bad)) == 0
    assert dmotion.box_side(1080, 1920, 144, 256) == 8 and [dmotion.box_side(h, w, 96, 128) for h, w in ((96, 128), (135, 241), (270, 480))] == [1, 2, 4]
    for H, W, TH, TW in ((1080, 1920, 144, 256), (135, 241, 64, 96), (97, 128, 96, 128), (96, 129, 96, 128), (7, 5000, 144, 256)):
        assert dmotion.box_side(H, W, TH, TW) == mr.box_side(H, W, TH, TW)


def _estimate_args(**over):
    p = dmotion.motion_params()
    a = dict(frames=0x10000, n=2, format=0, params=p, boxes=0x20000, scores=0x30000, counts=0x40000, d=8, state=0x50000, state_bytes=1 << 30,
             motion=0x60000, stats=0x70000, vectors=0x80000)
    a.update(over)
    return a


@pytest.mark.parametrize("what,over,pover,code", [
    ("null frames", dict(frames=0), None, DN_E_INVALID),
    ("null state", dict(state=0), None, DN_E_INVALID),
    ("null motion", dict(motion=0), None, DN_E_INVALID),
    ("null stats", dict(stats=0), None, DN_E_INVALID),
    ("n 0", dict(n=0), None, DN_E_INVALID),
    ("boxes without scores", dict(scores=0), None, DN_E_INVALID),
    ("counts alone", dict(boxes=0, scores=0), None, DN_E_INVALID),
    ("d 0 with masking", dict(d=0), None, DN_E_INVALID),
    ("misaligned state", dict(state=0x50008), None, DN_E_INVALID),
    ("misaligned vectors", dict(vectors=0x80004), None, DN_E_INVALID),
    ("misaligned scores", dict(scores=0x30002), None, DN_E_INVALID),
    ("block 12", {}, dict(block=12), DN_E_INVALID),
    ("radius 0", {}, dict(radius=0), DN_E_INVALID),
    ("radius 17", {}, dict(radius=17), DN_E_INVALID),
    ("min_blocks 0", {}, dict(min_blocks=0), DN_E_INVALID),
    ("negative min_texture", {}, dict(min_texture=-1), DN_E_INVALID),
    ("NaN mask_thresh", {}, dict(mask_thresh=float("nan")), DN_E_INVALID),
    ("reserved", {}, dict(reserved=1), DN_E_INVALID),
    ("capacity too wide", {}, dict(max_w=528), DN_E_UNSUPPORTED),
    ("capacity below one block", {}, dict(max_h=47), DN_E_UNSUPPORTED),
    ("format 4", dict(format=4), None, DN_E_UNSUPPORTED),
    ("d 513", dict(d=513), None, DN_E_UNSUPPORTED),
    ("n 65536", dict(n=65536), None, DN_E_UNSUPPORTED),
    ("small state", dict(state_bytes=2 * (16 + 16 * 98 + 2 * 144 * 256) - 1), None, DN_E_WORKSPACE),
])
def test_estimate_refuses_before_anything_is_enqueued(what, over, pover, code):
    """Every refusal comes back with its code and a dn_last_error text that names the entry point; the addresses are made up, so a call that got
    as far as a launch would not come back like this."""
    L = _library()
    a = _estimate_args(**over)
    for k, v in (pover or {}).items():
        setattr(a["params"], k, v)
    v = lambda x: C.c_void_p(x) if x else None
    rc = L.dn_motion_estimate(v(a["frames"]), a["n"], a["format"], C.byref(a["params"]), v(a["boxes"]), v(a["scores"]), v(a["counts"]), a["d"],
                              v(a["state"]), a["state_bytes"], v(a["motion"]), v(a["stats"]), v(a["vectors"]), None)
    assert rc == code, (what, rc, L.dn_last_error())
    assert b"dn_motion_estimate" in L.dn_last_error(), what


def test_the_other_entry_points_refuse_before_anything_is_enqueued():
    L = _library()
    v = C.c_void_p
    p = dmotion.motion_params()
    need = L.dn_motion_state_bytes(2, C.byref(p))
    assert L.dn_motion_reset(None, need, 2, C.byref(p), None, None) == DN_E_INVALID
    assert L.dn_motion_reset(v(0x1008), need, 2, C.byref(p), None, None) == DN_E_INVALID
    assert L.dn_motion_reset(v(0x1000), need, 0, C.byref(p), None, None) == DN_E_INVALID
    assert L.dn_motion_reset(v(0x1000), need, 2, None, None, None) == DN_E_INVALID
    assert L.dn_motion_reset(v(0x1000), need - 1, 2, C.byref(p), None, None) == DN_E_WORKSPACE and b"dn_motion_reset" in L.dn_last_error()
    tb = L.dn_track_state_bytes(2, 63)
    assert L.dn_track_compensate(None, tb, 2, 63, v(0x2000), None) == DN_E_INVALID
    assert L.dn_track_compensate(v(0x1000), tb, 2, 63, None, None) == DN_E_INVALID
    assert L.dn_track_compensate(v(0x1000), tb, 2, 63, v(0x2004), None) == DN_E_INVALID
    assert L.dn_track_compensate(v(0x1000), tb, 0, 63, v(0x2000), None) == DN_E_INVALID
    assert L.dn_track_compensate(v(0x1000), tb, 2, 257, v(0x2000), None) == DN_E_UNSUPPORTED
    assert L.dn_track_compensate(v(0x1000), tb - 1, 2, 63, v(0x2000), None) == DN_E_WORKSPACE and b"dn_track_compensate" in L.dn_last_error()


def test_the_python_layer_refuses_on_the_host(monkeypatch):
    """Nothing reaches the library for any of these: its loader is replaced by one that fails the test."""
    def no_library():
        raise AssertionError("the library was reached")
    for kw in (dict(block=12), dict(block=True), dict(radius=0), dict(radius=17), dict(radius=1.5), dict(max_size=(47, 256)), dict(max_size=(144, 513)),
               dict(max_size=144), dict(min_blocks=0), dict(min_texture=-1), dict(mask_thresh=float("nan"))):
        with pytest.raises(ValueError, match="MotionCompensator"):
            dmotion.motion_params(**kw)
    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(ValueError, match="block must be 8 or 16"):
        dmotion.MotionCompensator(2, "cuda:0", block=4)
    with pytest.raises(ValueError, match="streams"):
        dmotion.MotionCompensator(0, "cuda:0")
    with pytest.raises(RuntimeError, match="needs a GPU device"):
        dmotion.MotionCompensator(2, "cpu")
    # a compensator without a device behind it: what estimate checks is host work
    mc = object.__new__(dmotion.MotionCompensator)
    mc.params, mc.streams, mc.device = dmotion.motion_params(), 2, torch.device("cuda:0")
    batch = FrameBatch(2, "cuda:0")
    with pytest.raises(ValueError, match="call set"):
        mc.estimate(batch)
    batch.table = object()
    batch.sizes = [(1080, 1920), (47, 1920)]                                        # k = 8: a 5 x 240 thumbnail
    with pytest.raises(ValueError, match="frame 1 .* smaller than one block"):
        mc.estimate(batch)
    batch.sizes = [(1080, 1920), (384, 8 * 47)]                                     # k = 3: 128 x 125 -- fine; k = 8 on 47 columns is not reached
    assert dmotion.check_sizes(batch.sizes, mc.params) == [8, 3]
    batch.sizes = [(1080, 1920), (48, 4097 * 257)]                                  # k = 4098: the box sum would pass 2^32
    with pytest.raises(ValueError, match="box filter"):
        mc.estimate(batch)
    batch.sizes = [(1080, 1920), (720, 1280)]
    with pytest.raises(ValueError, match="expected a FrameBatch"):
        mc.estimate(object())
    with pytest.raises(ValueError, match="3 frames"):
        other = FrameBatch(3, "cuda:0")
        other.table = object()
        mc.estimate(other)
    with pytest.raises(ValueError, match="the FrameBatch is on"):
        mc.estimate(FrameBatch(2, "cpu"))
    d = 4
    boxes, scores, counts = torch.zeros(2, d, 4), torch.zeros(2, d), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="together"):
        mc.estimate(batch, boxes, scores)
    with pytest.raises(ValueError, match="expected a contiguous"):                   # (CPU tensors: the wrong device)
        mc.estimate(batch, boxes, scores, counts)
    with pytest.raises(ValueError, match="scores must be"):
        mc.estimate(batch, boxes, scores[0], counts)
    with pytest.raises(ValueError, match="3 streams"):
        mc.estimate(batch, torch.zeros(3, d, 4), torch.zeros(3, d), counts)
    with pytest.raises(ValueError, match="rows per stream"):
        mc.estimate(batch, torch.zeros(2, 513, 4), torch.zeros(2, 513), counts)


# ---------------------------------------------------------------------------------------------------------------- the reference, pinned
def _steps(ref, images, **kw):
    return [ref.estimate([im], **kw) for im in images]


@pytest.mark.parametrize("k,size,cap,a,b", [(1, (96, 128), (96, 128), 5, -3), (3, (288, 385), (96, 128), -7, 11), (1, (96, 128), (144, 256), 16, 16)])
def test_a_shift_by_whole_thumbnail_pixels_is_found_exactly(k, size, cap, a, b):
    """A random textured image and its copy shifted by (k a, k b): exactly s = 1, tx = k a, ty = k b. k = 3 on 385 columns has a remainder column."""
    H, W = size
    assert mr.box_side(H, W, *cap) == k and (k == 1 or W % k)
    canvas = mr.textured(1, H + 40 * k, W + 40 * k, cell=2 * k)
    x0 = y0 = 20 * k
    first, second = mr.window(canvas, x0, y0, H, W), mr.window(canvas, x0 - k * a, y0 - k * b, H, W)      # the content moves by (+k a, +k b)
    ref = mr.RefCompensator(1, cap)
    (m0, s0, _), (m1, s1, v1) = _steps(ref, [first, second])
    assert m0[0].tolist() == [1, 0, 0, 0] and s0[0].tolist()[1:] == [0, 0, k]
    assert m1[0].tolist() == [1.0, float(k * a), float(k * b), 1.0], m1
    n = int(s1[0, 0])
    assert n >= 8 and s1[0].tolist() == [n, n, n, k]
    assert (v1[0, :n, :2] == (-a, -b)).all() and (v1[0, :n, 2] == 0).all() and not v1[0, n:].any()


def test_flat_images_masked_majorities_and_minorities():
    H, W = 96, 128
    flat = np.full((H, W), 117, np.uint8)
    ref = mr.RefCompensator(1, (96, 128))
    (_, _, _), (m, s, v) = _steps(ref, [flat, flat])
    assert m[0].tolist() == [1, 0, 0, 0] and s[0].tolist() == [24, 0, 0, 1] and not v[0, :, 3].any()         # no texture: nothing is valid
    # a masked-out majority: 18 of 24 blocks (three of the four rows) lie under one detection
    canvas = mr.textured(2, H + 20, W + 20)
    views = [mr.window(canvas, 10, 10, H, W), mr.window(canvas, 7, 12, H, W)]
    boxes, scores = np.array([[[0, 0, 128, 64], [0, 0, 128, 96]]], f32), np.array([[0.9, 0.3]], f32)
    ref = mr.RefCompensator(1, (96, 128))
    ref.estimate([views[0]])
    m, s, v = ref.estimate([views[1]], boxes, scores, np.array([2], np.int32))
    assert s[0].tolist() == [24, 6, 6, 1] and m[0].tolist() == [1, 0, 0, 0]                                  # fewer than min_blocks = 8
    m, s, v = mr.RefCompensator(1, (96, 128), min_blocks=6).estimate([views[1]])                              # (a first frame)
    ref = mr.RefCompensator(1, (96, 128), min_blocks=6)
    ref.estimate([views[0]])
    m, s, v = ref.estimate([views[1]], boxes, scores, np.array([2], np.int32))
    assert m[0].tolist() == [1.0, 3.0, -2.0, 1.0]
    # a 25 % minority that moves differently (one row of six blocks of the four rows) leaves the estimate unchanged
    second = views[1].copy()
    second[:32] = mr.window(canvas, 10 + 9, 10 - 6, H, W)[:32]
    ref = mr.RefCompensator(1, (96, 128))
    ref.estimate([views[0]])
    m, s, v = ref.estimate([second])
    assert s[0].tolist() == [24, 24, 18, 1] and m[0].tolist() == [1.0, 3.0, -2.0, 1.0]
    assert {tuple(r) for r in v[0, :6, :2].tolist()} == {(9, -6)} and {tuple(r) for r in v[0, 6:, :2].tolist()} == {(-3, 2)}
    # ... and with 50 % + of outliers around the median there is no consensus
    vec = np.zeros((24, 4), np.int32)
    vec[:, 3] = 1
    vec[:14, 0] = [-3, -5, -7, -9, -11, -13, -15, 3, 5, 7, 9, 11, 13, 15]                                    # the median is 0; ten blocks agree with it
    m, valid, inl = mr.fit(vec, 6, 16, 16, 1, 8)
    assert (valid, inl) == (24, 10) and m.tolist() == [1, 0, 0, 0]
    vec[0, 0] = vec[1, 0] = 1
    m, valid, inl = mr.fit(vec, 6, 16, 16, 1, 8)
    assert (valid, inl) == (24, 12) and m[3] == 1                                                            # 2 inliers >= valid: just enough


def _zoom_vectors(block, radius, nbx, nby, div):
    """The vectors of a zoom about the thumbnail's origin: a block centre u of the current frame was at u (1 - 1 / div) in the previous one."""
    vec = np.zeros((nbx * nby, 4), np.int32)
    for i in range(nbx * nby):
        cx, cy = radius + (i % nbx) * block + block // 2, radius + (i // nbx) * block + block // 2
        assert cx % div == 0 and cy % div == 0
        vec[i] = (-(cx // div), -(cy // div), 0, 1)
    return vec


def test_an_exact_zoom_gives_the_closed_form_scale():
    """A zoom by 2 pixels per 16: d = -u / 8 exactly on block centres 16, 32, 48, 64 (block 16, radius 8). The inliers are the blocks within 2
    of the medians (-4, -4): three columns, three rows. Over them x = 7 x' / 8, so num / den = 8 / 7 in exact integers, and tu = tv = 0 up to
    the rounding of s Sx."""
    vec = _zoom_vectors(16, 8, 4, 3, 8)
    assert sorted(set(vec[:, 0].tolist())) == [-8, -6, -4, -2] and sorted(set(vec[:, 1].tolist())) == [-6, -4, -2]
    m, valid, inl = mr.fit(vec, 4, 16, 8, 1, 8)
    assert (valid, inl) == (12, 9)
    assert m[3] == 1 and m[0] == f32(8.0 / 7.0) and abs(m[1]) < 1e-12 and abs(m[2]) < 1e-12, m
    # the same in frame coordinates with k = 4: tx = k tu + (1 - s) (k - 1) / 2 with tu = 0
    m4, _, _ = mr.fit(vec, 4, 16, 8, 4, 8)
    want = (1.0 - 8.0 / 7.0) * 3 / 2
    assert m4[0] == f32(8.0 / 7.0) and abs(m4[1] - want) < 1e-6 and abs(m4[2] - want) < 1e-6
    # twice the zoom (block 8, radius 4: centres 8, 16, 24, 32, d = -u / 4): s = 4 / 3 is outside 0.8 .. 1.25 and the step is not ok
    m, valid, inl = mr.fit(_zoom_vectors(8, 4, 4, 3, 4), 4, 8, 4, 1, 8)
    assert (valid, inl) == (12, 9) and m.tolist() == [1, 0, 0, 0]
    # one inlier: the denominator is 0
    one = np.zeros((9, 4), np.int32)
    one[0] = (1, 1, 0, 1)
    m, valid, inl = mr.fit(one, 3, 16, 16, 1, 1)
    assert (valid, inl) == (1, 1) and m.tolist() == [1, 0, 0, 0]


def test_the_first_frame_and_a_size_change_reseed():
    canvas = mr.textured(4, 200, 300)
    ref = mr.RefCompensator(2, (96, 128))
    a = [mr.window(canvas, 10 + i, 10, 96, 128) for i in range(4)]
    c = [mr.window(canvas, 10 + i, 10, 96, 112) for i in range(4)]
    oks = []
    for step, frames in enumerate([(a[0], a[0]), (a[1], a[1]), (c[2], a[2]), (c[3], a[3])]):
        if step == 3:
            ref.reset([1])
        m, s, v = ref.estimate(list(frames))
        oks.append(m[:, 3].tolist())
        if step == 2:
            assert s[0].tolist() == [20, 0, 0, 1] and not v[0].any()                                          # 96 x 112: 4 x 5 blocks, none searched
    assert oks == [[0, 0], [1, 1], [0, 1], [1, 0]]


def test_luma_and_the_thumbnail():
    rgb = np.array([[[255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30]]], np.uint8)
    assert mr.luma(rgb, "rgb24")[0].tolist() == [255, 77, 149, 29, (770 + 3000 + 870 + 128) >> 8]
    assert mr.luma(rgb[..., ::-1], "bgr24")[0].tolist() == mr.luma(rgb, "rgb24")[0].tolist()
    y = np.arange(7 * 10, dtype=np.uint8).reshape(7, 10) * 3
    t, k = mr.thumbnail(y, 2, 3)                                                      # k = 3 (10 // 3 = 3 <= 3, 7 // 3 = 2 <= 2): the 10th column, the 7th row ignored
    assert k == 3 and t.shape == (2, 3)
    assert t[1, 2] == (int(y[3:6, 6:9].sum()) + 4) // 9 and t[0, 0] == (int(y[:3, :3].sum()) + 4) // 9
    assert mr.thumbnail(np.array([[1, 2], [2, 2]], np.uint8), 1, 1)[0][0, 0] == 2     # (7 + 2) / 4: the mean rounds half up


# ---------------------------------------------------------------------------------------------------------------- compensate
def _populated(seed=3):
    frames, _ = tr.scene(seed, 10, 2, 32, objects=8, max_dropout=4)
    t = tr.RefTracker(2, 16, track_buffer=4)
    for fr in frames:
        t.update(*fr)
    return t


def test_compensate_against_float64_with_a_bound_counted_from_its_operations():
    t = _populated()
    assert set(np.unique(t.state).tolist()) >= {tr.FREE, tr.TRACKED, tr.LOST}
    before = {k: v.copy() for k, v in t.table().items()}
    mo = np.array([[1.0625, 17.3, -9.1, 1], [0.93, 4.0, 4.0, 0]], f32)
    mr.compensate(t, mo)
    for k in tr.RefTracker.FIELDS:
        if k != "filter":
            assert np.array_equal(getattr(t, k), before[k]), k                          # nothing but the filter is touched
    assert np.array_equal(t.filter[1], before["filter"][1])                            # not ok: not written
    s, tx, ty = [np.float64(v) for v in mo[0, :3]]
    eps = 2.0 ** -24
    f0, f1 = before["filter"][0].astype(np.float64), t.filter[0].astype(np.float64)
    live = before["state"][0] != tr.FREE
    assert live.any() and not live.all()
    assert np.array_equal(t.filter[0][:, ~live], before["filter"][0][:, ~live])       # free slots are not touched
    assert np.array_equal(t.filter[0][10:15], before["filter"][0][10:15])             # a = w / h is not touched
    for kc, tr_ in ((0, tx), (1, ty), (3, 0.0)):
        x, v, P = f0[5 * kc][live], f0[5 * kc + 1][live], f0[5 * kc + 2:5 * kc + 5][:, live]
        # x: the product rounds once, the sum once (for h there is no sum): each error at most eps times the rounded value's size
        bound = eps * np.abs(s * x) * (1 + eps) + (eps * np.abs(s * x + tr_) * (1 + eps) if kc != 3 else 0)
        assert (np.abs(f1[5 * kc][live] - (s * x + tr_)) <= bound).all(), kc
        assert (np.abs(f1[5 * kc + 1][live] - s * v) <= eps * np.abs(s * v)).all(), kc
        # P: s2 = s * s rounds once, the product once: a relative error of at most 2 eps + eps^2
        assert (np.abs(f1[5 * kc + 2:5 * kc + 5][:, live] - s * s * P) <= (2 * eps + eps * eps) * np.abs(s * s * P)).all(), kc
        assert (f1[5 * kc + 2:5 * kc + 5][:, live] != P).any()


def test_warp_then_predict_equals_predict_then_warp_in_float64():
    """F commutes with the transform, and Q scales with it (its entries are squares of multiples of h, the ones of a = w / h constants that the
    transform leaves alone): BoT-SORT's predict-then-warp and this package's warp-then-predict are the same map in exact arithmetic."""
    t = _populated(5)
    s, tx, ty = 1.07, -13.5, 6.25
    W = np.diag([s, s, 1, s, s, s, 1, s])
    shift = np.array([tx, ty, 0, 0, 0, 0, 0, 0])
    n = 0
    for slot in range(16):
        if t.state[0, slot] == tr.FREE:
            continue
        mean, cov = tr.to64(t.filter[0, :, slot])
        m1, c1 = tr.predict64(W @ mean + shift, W @ cov @ W.T)
        m2, c2 = tr.predict64(mean, cov)
        m2, c2 = W @ m2 + shift, W @ c2 @ W.T
        assert np.allclose(m1, m2, rtol=1e-13, atol=1e-11) and np.allclose(c1, c2, rtol=1e-12, atol=0), slot
        n += 1
    assert n >= 3
