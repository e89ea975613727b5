"""Surface dewarping on the device (dn_warp, warp.Warper, SSD.track_frames(..., warp=, source=)) against tests/warp_ref.py, bit for bit
on every plane's payload; the gap bytes of the pitched destinations, filled with 0xA5, and every payload byte no item covers must stay. Sources are
noise surfaces of warp_ref.SRC_SIZES (80 x 96 and the odd 45 x 67), destinations noise surfaces of warp_ref.DST_SIZES (200 x 240 and the odd
57 x 73), built with the helpers of tests/test_gpu_regions.py and tests/test_gpu_compose.py. tests/test_warp.py shows that scenes of this kind tell
seven wrong resamplers from the right one."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_compose as tgc
import test_gpu_regions as tgr
import warp_ref as ref
from demonet_amd import _lib, models, warp
from demonet_amd.frames import FrameBatch
from demonet_amd.track import ByteTracker

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GAP = tgc.GAP
FORMATS = ["nv12", "i420", "rgb24", "bgr24"]
SPACE = ("bt709", False)
_WANT = {}


def _planes(fmt, sizes, seed):
    return [ref.noise_planes(fmt, seed + i, h, w) for i, (h, w) in enumerate(sizes)]


def _batch(fmt, planes, pitch, space=SPACE):
    return tgc._batch(fmt, space, planes, pitch)


def _want(fmt, scene, sp, dp, items):
    """the reference of a scene, computed once per format"""
    if (fmt, scene) not in _WANT:
        _WANT[(fmt, scene)] = ref.warp(sp, dp, ref.ref_items(items, fmt, *SPACE), fmt)
    return _WANT[(fmt, scene)]


def _run(fmt, items, scene, src_pitch="w+1", dst_pitch="256", capacity=16):
    sp, dp = _planes(fmt, ref.SRC_SIZES, 940), _planes(fmt, ref.DST_SIZES, 950)
    sb, _ = _batch(fmt, sp, src_pitch)
    db, dsurf = _batch(fmt, dp, dst_pitch)
    w = warp.Warper(capacity, DEV).set(items, sb, db)
    assert w(sb, db) is db
    torch.cuda.synchronize()
    want = _want(fmt, scene, sp, dp, items)
    tgc._same(dsurf, dp, want, "{} {}".format(scene, fmt))
    assert any(not np.array_equal(a, b) for x, d in zip(want, dp) for a, b in zip(x, d))
    return w, [p.copy() for s, planes in zip(dsurf, dp) for p in tgc._payloads(s, planes)]


# ---------------------------------------------------------------------------------------------------------------- 1. formats and pitches
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_on_the_mixed_scene_at_two_pitches(fmt):
    items = ref.mixed_items()
    w, first = _run(fmt, items, "mixed")
    assert _lib.debug_last_kernel() == "warp_kernel<{}>".format({"nv12": 0, "i420": 1}.get(fmt, 2))
    assert len(w.items) == 14 and w.items[4][3] == w.items[5][3] and w.points < sum(i.mesh.points.shape[0] * i.mesh.points.shape[1] for i in items)    # one mesh, two items
    _, again = _run(fmt, items, "mixed", src_pitch="w", dst_pitch="w+1")
    assert all(np.array_equal(a, b) for a, b in zip(first, again))          # two runs, other pitches: equal bytes
    # the rectangle of the mesh at +-(2^21 - 1) holds nothing but its border colour
    far = ref.ref_items(items, fmt, *SPACE)[9]
    (x0, y0), border, (dw, dh) = far[3], far[4], far[5]
    chans = ref.cr.channels(fmt, [first[0]] if fmt in ("rgb24", "bgr24") else first[:{"nv12": 2, "i420": 3}[fmt]])
    assert (chans[0][y0:y0 + dh, x0:x0 + dw] == border[0]).all()
    if fmt in ref.YUV:
        assert (chans[1][y0 // 2:(y0 + dh) // 2, x0 // 2:(x0 + dw) // 2] == border[1]).all() and (chans[2][y0 // 2:(y0 + dh) // 2, x0 // 2:(x0 + dw) // 2] == border[2]).all()
    else:
        assert (chans[1][y0:y0 + dh, x0:x0 + dw] == border[1]).all() and (chans[2][y0:y0 + dh, x0:x0 + dw] == border[2]).all()


@pytest.mark.parametrize("fmt", ["nv12", "i420", "rgb24"])
def test_the_gather_path_alone_gives_the_same_bits(fmt, monkeypatch):
    """DN_WARP_STAGE=0 (read by every dn_warp call) sends the tiles that would be staged -- the identity, the half-pixel shift, the quarter turn, the
    magnification, the tile at the staging limit -- through the gather path: the same bytes"""
    monkeypatch.setenv("DN_WARP_STAGE", "0")
    _run(fmt, ref.mixed_items(), "mixed", src_pitch="w", dst_pitch="w+1")


@pytest.mark.parametrize("fmt", ["nv12", "i420", "rgb24"])
def test_tiles_at_the_staging_limit_and_one_sample_over_it(fmt):
    """footprints of exactly 112 samples, the widest and tallest the kernel stages, and of 113, which it gathers: the same arithmetic on both sides"""
    items = ref.limit_items()
    sp, dp = [ref.noise_planes(fmt, 970, *ref.LIMIT_SRC)], [ref.noise_planes(fmt, 971, 72, 72)]
    for pitch in ("w+1", "256"):
        sb, _ = _batch(fmt, sp, pitch)
        db, dsurf = _batch(fmt, dp, "w+1")
        warp.Warper(4, DEV).set(items, sb, db)(sb, db)
        torch.cuda.synchronize()
        tgc._same(dsurf, dp, ref.warp(sp, dp, ref.ref_items(items, fmt, *SPACE), fmt), "staging limit {} {}".format(fmt, pitch))


def test_a_full_range_bt601_batch_converts_its_border_colour():
    items = ref.mixed_items()
    space = ("bt601", True)
    sp, dp = _planes("nv12", ref.SRC_SIZES, 940), _planes("nv12", ref.DST_SIZES, 950)
    sb, _ = _batch("nv12", sp, "w+1", space)
    db, dsurf = _batch("nv12", dp, "w+1", space)
    warp.Warper(16, DEV).set(items, sb, db)(sb, db)
    torch.cuda.synchronize()
    tgc._same(dsurf, dp, ref.warp(sp, dp, ref.ref_items(items, "nv12", *space), "nv12"), "bt601 full range")


# ---------------------------------------------------------------------------------------------------------------- 2. the persistent walk
@pytest.mark.parametrize("fmt", ["nv12", "i420", "bgr24"])
def test_more_tiles_than_workgroups_and_runs_that_cross_items(fmt):
    """The scenes above have fewer tiles than the kernel has workgroups, so each workgroup there handles one tile. Here 2304 items of four tiles each
    make 9216 tiles: every workgroup that works walks a run of three, which crosses an item boundary for most of them."""
    items = ref.many_items()
    side = 48 * 34
    sp, dp = _planes(fmt, ref.SRC_SIZES, 940), [ref.noise_planes(fmt, 950, side, side)]
    sb, _ = _batch(fmt, sp, "w+1")
    db, dsurf = _batch(fmt, dp, "w+1")
    w = warp.Warper(4096, DEV).set(items, sb, db)
    assert w.tiles == 9216 > 2 * 4096 and len(w.items) == 2304 and w.points == 6 * 36
    w(sb, db)
    torch.cuda.synchronize()
    tgc._same(dsurf, dp, ref.warp(sp, dp, ref.ref_items(items, fmt, *SPACE), fmt), "9216 tiles, {}".format(fmt))


# ---------------------------------------------------------------------------------------------------------------- 3. a captured call
def test_a_captured_call_follows_surfaces_items_meshes_and_the_item_count():
    fmt = "nv12"
    sp = [_planes(fmt, ref.SRC_SIZES, 940), _planes(fmt, ref.SRC_SIZES, 960)]
    dp = _planes(fmt, ref.DST_SIZES, 950)
    sb, _ = _batch(fmt, sp[0], "w+1")
    db, _ = _batch(fmt, dp, "256")
    mixed, second = ref.mixed_items(), ref.second_items()
    w = warp.Warper(16, DEV, mesh_points=600).set(mixed, sb, db)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        w(sb, db)                                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        w(sb, db)
    tables = (sb.table.data_ptr(), db.table.data_ptr(), w.table.data_ptr(), w.mesh.data_ptr())
    assert len(second) != len(mixed)
    got = []
    for which, items in ((0, mixed), (1, mixed), (1, second), (1, second[:2]), (1, second[:2])):
        sb.set([tgr._surface(fmt, p, "w+1", GAP) for p in sp[which]])                    # other source surfaces ...
        dsurf = [tgr._surface(fmt, p, "256", GAP) for p in dp]
        db.set(dsurf)                                                                     # ... fresh destinations ...
        w.set(items, sb, db)                                                              # ... other items and meshes, another count
        assert (sb.table.data_ptr(), db.table.data_ptr(), w.table.data_ptr(), w.mesh.data_ptr()) == tables
        graph.replay()
        torch.cuda.synchronize()
        tgc._same(dsurf, dp, ref.warp(sp[which], dp, ref.ref_items(items, fmt, *SPACE), fmt), "replay on {} items".format(len(items)))
        got.append([p.copy() for s, planes in zip(dsurf, dp) for p in tgc._payloads(s, planes)])
    assert all(np.array_equal(a, b) for a, b in zip(got[3], got[4]))          # two replays on equal inputs: equal bits
    w.set([], sb, db)                                                          # no item: nothing is written
    dsurf = [tgr._surface(fmt, p, "256", GAP) for p in dp]
    db.set(dsurf)
    graph.replay()
    torch.cuda.synchronize()
    tgc._same(dsurf, dp, dp, "replay on no items")
    with pytest.raises(ValueError, match="mesh_points is 600"):
        w.set([warp.Item(0, 0, warp.identity((200, 240)))] + second[2:3], sb, db)
    with pytest.raises(ValueError, match="shares memory"):
        w.set(second, sb, FrameBatch(2, DEV, format=fmt).set([sb.frames[0], dsurf[1]]))


# ---------------------------------------------------------------------------------------------------------------- 4. in front of the tracker
def test_warp_in_front_of_a_tracking_step():
    """track_frames(views, tracker, warp=w, source=fisheye) equals the explicit w(fisheye, views) followed by track_frames(views, tracker), output
    for output and byte for byte of the views; the sliced and the appearance steps take the same pair."""
    from demonet_amd.sliced import FrameSlicer
    m = models.load_synthetic(models.ssd_lite_mobilenet_v2(image_size=160, num_classes=3), 0).to(DEV)
    try:
        fmt = "nv12"
        fish = [tgr._source(fmt, "bt709", False, 930, 200, 260)[0]]
        view_sizes = [(120, 160), (97, 131)]
        vp = _planes(fmt, view_sizes, 950)
        items = [warp.Item(0, 0, warp.fisheye_view((200, 260), view_sizes[0], fov=90, pan=20, tilt=40), (0, 0), (16, 128, 128)),
                 warp.Item(0, 1, warp.fisheye_view((200, 260), view_sizes[1], fov=70, pan=190, tilt=30), (0, 0), "replicate")]
        kw = dict(max_tracks=64, track_thresh=0.05, low_thresh=0.01, new_thresh=0.05)
        ta, tb, sa, sb_ = ByteTracker(2, DEV, **kw), ByteTracker(2, DEV, **kw), ByteTracker(2, DEV, **kw), ByteTracker(2, DEV, **kw)
        slicer = FrameSlicer(m, view_sizes, max_tiles_per_forward=3)
        want = None
        for step in range(2):
            a_f, _ = _batch(fmt, fish, "256")
            b_f, _ = _batch(fmt, fish, "256")
            a_v, a_vs = _batch(fmt, vp, "w+1")
            b_v, b_vs = _batch(fmt, vp, "w+1")
            wa, wb = warp.Warper(4, DEV).set(items, a_f, a_v), warp.Warper(4, DEV).set(items, b_f, b_v)
            outs_a = [t.clone() for t in m.track_frames(a_v, ta, warp=wa, source=a_f)[:6]]
            wb(b_f, b_v)
            outs_b = [t.clone() for t in m.track_frames(b_v, tb, warp=None, source=None)[:6]]
            torch.cuda.synchronize()
            assert all(torch.equal(x, y) for x, y in zip(outs_a, outs_b)), step
            if want is None:
                want = ref.warp([fish[0]], vp, ref.ref_items(items, fmt, *SPACE), fmt)
            tgc._same(a_vs, vp, want, "views of the step")
            tgc._same(b_vs, vp, want, "views of the explicit call")
            c_v, c_vs = _batch(fmt, vp, "w+1")
            wc = warp.Warper(4, DEV).set(items, a_f, c_v)
            outs_c = [t.clone() for t in m.track_sliced_frames(c_v, sa, slicer, warp=wc, source=a_f)[:6]]
            outs_d = [t.clone() for t in m.track_sliced_frames(b_v, sb_, slicer)[:6]]
            torch.cuda.synchronize()
            assert all(torch.equal(x, y) for x, y in zip(outs_c, outs_d)), step
            tgc._same(c_vs, vp, want, "views of the sliced step")
        with pytest.raises(ValueError, match="go together"):
            m.track_frames(a_v, ta, warp=wa)
        with pytest.raises(ValueError, match="go together"):
            m.track_sliced_frames(a_v, sa, slicer, source=a_f)
        with pytest.raises(ValueError, match="expected a Warper"):
            m.track_frames(a_v, ta, warp=slicer, source=a_f)
        with pytest.raises(ValueError, match="stale sizes"):
            m.track_frames(b_f, ta, warp=wa, source=a_f)
    finally:
        m.release()


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def test_every_error_code_of_the_entry_point():
    DN_E_INVALID, DN_E_UNSUPPORTED = -1, -4
    sp, dp = _planes("nv12", ref.SRC_SIZES, 940), _planes("nv12", ref.DST_SIZES, 950)
    sb, _ = _batch("nv12", sp, "w+1")
    db, dsurf = _batch("nv12", dp, "w+1")
    w = warp.Warper(16, DEV).set(ref.mixed_items(), sb, db)
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda v: C.c_void_p(v) if v else None      # noqa: E731

    def call(**kw):
        a = dict(src=sb.table.data_ptr(), dst=db.table.data_ptr(), fmt=0, table=w.table.data_ptr(), capacity=16, mesh=w.mesh.data_ptr())
        a.update(kw)
        return L.dn_warp(p(a["src"]), p(a["dst"]), a["fmt"], p(a["table"]), a["capacity"], p(a["mesh"]), stream)
    for kw in (dict(src=0), dict(dst=0), dict(table=0), dict(mesh=0), dict(src=sb.table.data_ptr() + 4), dict(dst=db.table.data_ptr() + 2),
               dict(table=w.table.data_ptr() + 8), dict(mesh=w.mesh.data_ptr() + 4), dict(capacity=0), dict(capacity=-3)):
        assert call(**kw) == DN_E_INVALID, kw
        assert L.dn_last_error()
    for kw in (dict(fmt=4), dict(fmt=-1), dict(capacity=65537)):
        assert call(**kw) == DN_E_UNSUPPORTED, kw
    torch.cuda.synchronize()
    tgc._same(dsurf, dp, dp, "every error is raised before anything is enqueued")
    assert call() == 0
    torch.cuda.synchronize()
    tgc._same(dsurf, dp, _want("nv12", "mixed", sp, dp, ref.mixed_items()), "the plain call")
