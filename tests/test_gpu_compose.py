"""Surface composition on the device (dn_compose, dn_surface_fill, compose.Compositor, SSD.track_frames(..., compose=, wall=)) against
tests/compose_ref.py, bit for bit on every plane's payload; the gap bytes of the pitched destinations, filled with 0xA5, and every payload byte no
item covers must stay. Sources are the noise surfaces of tests/regions_ref.SIZES (200 x 260 and 97 x 131), destinations noise surfaces of
compose_ref.DST_SIZES (128 x 160 and the odd 67 x 91), built with the helpers of tests/test_gpu_regions.py. tests/test_compose.py shows that the
scenes used here tell six wrong resamplers from the right one."""
import ctypes as C

import numpy as np
import pytest
import torch

import compose_ref as ref
import regions_ref as rr
import test_gpu_regions as tgr
from demonet_amd import _lib, compose, models, osd
from demonet_amd.frames import FrameBatch
from demonet_amd.track import ByteTracker

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GAP = 0xA5
FORMATS = ["nv12", "i420", "rgb24", "bgr24"]
SPACE = ("bt709", False)


# ---------------------------------------------------------------------------------------------------------------- helpers
def _root(t):
    while t._base is not None:
        t = t._base
    return t


def _payloads(surface, planes):
    """the payload planes of a surface as numpy, after checking that its gap bytes are still GAP"""
    out = []
    views = surface if isinstance(surface, tuple) else (surface,)
    for view, p in zip(views, planes):
        full = _root(view).cpu().numpy()
        payload = p.shape[1]
        assert full.shape[0] == p.shape[0] and (full[:, payload:] == GAP).all(), "a gap byte changed"
        out.append(full[:, :payload])
    return out


def _planes(fmt, sizes, seed):
    return [ref.noise_planes(fmt, seed + i, h, w) for i, (h, w) in enumerate(sizes)]


def _batch(fmt, space, planes, pitch):
    surfaces = [tgr._surface(fmt, p, pitch, GAP) for p in planes]
    return FrameBatch(len(planes), DEV, format=fmt, matrix=space[0], full_range=space[1]).set(surfaces), surfaces


def _same(surfaces, planes, want, what):
    for b, (surface, p, w) in enumerate(zip(surfaces, planes, want)):
        for i, (g, x) in enumerate(zip(_payloads(surface, p), w)):
            bad = np.argwhere(g != x)
            assert bad.size == 0, "{}: surface {} plane {}: {} bytes differ, first at {} (got {}, want {})".format(
                what, b, i, len(bad), tuple(bad[0]), g[tuple(bad[0])], x[tuple(bad[0])])


def _run(src, dst, items, src_pitch="w+1", dst_pitch="256", clear=None, capacity=16, what=""):
    """one composition of noise sources into noise destinations, compared with the reference; returns the destination payloads"""
    sp, dp = _planes(src[0], rr.SIZES, 940), _planes(dst[0], ref.DST_SIZES, 950)
    sb, _ = _batch(src[0], src[1:], sp, src_pitch)
    db, dsurf = _batch(dst[0], dst[1:], dp, dst_pitch)
    comp = compose.Compositor(capacity, DEV).set(ref.api_items(items), sb, db)
    assert comp(sb, db, clear=clear) is db
    torch.cuda.synchronize()
    base = dp
    if clear is not None:
        fill = osd.to_surface(clear, dst[0], dst[1], dst[2])
        base = [ref.planes_of(dst[0], [np.full_like(c, fill[k]) for k, c in enumerate(ref.channels(dst[0], p))]) for p in dp]
    want = ref.compose(sp, base, items, src, dst)
    _same(dsurf, dp, want, what or "{} -> {}".format(src[0], dst[0]))
    assert any(not np.array_equal(a, b) for w, d in zip(want, dp) for a, b in zip(w, d))
    return [p.copy() for s, planes in zip(dsurf, dp) for p in _payloads(s, planes)]


# ---------------------------------------------------------------------------------------------------------------- 1. format pairs
@pytest.mark.parametrize("dfmt", FORMATS)
@pytest.mark.parametrize("sfmt", FORMATS)
def test_every_format_pair_on_the_mixed_scene(sfmt, dfmt):
    items = ref.mixed_items(rr.SIZES)
    first = _run((sfmt,) + SPACE, (dfmt,) + SPACE, items)
    planewise = sfmt in ref.YUV and dfmt in ref.YUV
    code = _lib.DN_FRAME
    assert _lib.debug_last_kernel() == ("compose_planes_kernel" if planewise else "compose_rgb_kernel") + "<{},{}>".format(code[sfmt], code[dfmt])
    again = _run((sfmt,) + SPACE, (dfmt,) + SPACE, items, src_pitch="w", dst_pitch="w+1")
    assert all(np.array_equal(a, b) for a, b in zip(first, again))          # two runs, other pitches: equal bytes


def test_a_yuv_pair_across_matrix_and_range_goes_through_rgb():
    _run(("nv12", "bt601", False), ("i420", "bt709", True), ref.mixed_items(rr.SIZES))
    assert _lib.debug_last_kernel() == "compose_rgb_kernel<0,1>"
    _run(("i420", "bt709", True), ("nv12", "bt601", True), ref.second_items(rr.SIZES))
    assert _lib.debug_last_kernel() == "compose_rgb_kernel<1,0>"


# ---------------------------------------------------------------------------------------------------------------- 1b. the persistent walk
@pytest.mark.parametrize("src,dst", [(("nv12",) + SPACE, ("i420",) + SPACE), (("i420",) + SPACE, ("rgb24",) + SPACE), (("bgr24",) + SPACE, ("nv12",) + SPACE)],
                         ids=["planes", "yuv-rgb", "rgb-yuv"])
def test_more_tiles_than_workgroups_and_runs_that_cross_items(src, dst):
    """The scenes above have fewer tiles than the kernels have workgroups, so each workgroup there handles one tile. Here 2304 items of four tiles
    each make 9216 tiles: every workgroup that works walks a run of three, which crosses an item boundary for most of them, and reuses its edge
    tables and row sums from tile to tile. The same bits as the reference all the same."""
    items = ref.many_items(rr.SIZES)
    side = 48 * 34
    sp, dp = _planes(src[0], rr.SIZES, 940), [ref.noise_planes(dst[0], 950, side, side)]
    sb, _ = _batch(src[0], src[1:], sp, "w+1")
    db, dsurf = _batch(dst[0], dst[1:], dp, "w+1")
    comp = compose.Compositor(4096, DEV).set(ref.api_items(items), sb, db)
    assert comp.tiles == 9216 > 2 * 4096 and len(comp.items) == 2304
    comp(sb, db)
    torch.cuda.synchronize()
    _same(dsurf, dp, ref.compose(sp, dp, items, src, dst), "9216 tiles, {} -> {}".format(src[0], dst[0]))


# ---------------------------------------------------------------------------------------------------------------- 2. rounding
def _edge_plane(ky, kx, rows, cols, rng):
    """[rows ky, cols kx] bytes whose ky x kx blocks sum to k D + ceil(D / 2) - 1 (even block columns: the last sum that rounds down to k) or
    k D + ceil(D / 2) (odd block columns: the first that rounds up to k + 1)"""
    D = ky * kx
    p = np.zeros((rows, ky, cols, kx), np.int64)
    for r in range(rows):
        for c in range(cols):
            k = int(rng.integers(0, 255))
            blk = np.full(D, k)
            blk[:(D + 1) // 2 - 1 + (c & 1)] += 1
            p[r, :, c, :] = rng.permutation(blk).reshape(ky, kx)
    return p.reshape(rows * ky, cols * kx).astype(np.uint8)


def test_sums_on_both_sides_of_the_rounding_edge():
    rng = np.random.default_rng(77)
    items, planes = [], []
    for n, (ky, kx) in enumerate([(2, 2), (3, 3), (4, 2), (5, 7)]):
        Y = _edge_plane(ky, kx, 12, 20, rng)
        U, V = _edge_plane(ky, kx, 6, 10, rng), _edge_plane(ky, kx, 6, 10, rng)
        planes.append([Y, U, V])
        items.append((n, (0, 0, 20 * kx, 12 * ky), 0, (0, 14 * n, 20, 12)))
    dp = [ref.noise_planes("i420", 5, 60, 24)]
    sb, _ = _batch("i420", SPACE, planes, "w+1")
    db, dsurf = _batch("i420", SPACE, dp, "w+1")
    compose.Compositor(4, DEV).set(ref.api_items(items), sb, db)(sb, db)
    torch.cuda.synchronize()
    want = ref.compose(planes, dp, items, ("i420",) + SPACE, ("i420",) + SPACE)
    floor = ref.compose(planes, dp, items, ("i420",) + SPACE, ("i420",) + SPACE, mistake="floor")
    for n in range(4):            # every odd block column rounds up, every even one down, at each of the four ratios
        rows = slice(14 * n, 14 * n + 12)
        assert (want[0][0][rows, 1:20:2] == floor[0][0][rows, 1:20:2] + 1).all() and (want[0][0][rows, 0:20:2] == floor[0][0][rows, 0:20:2]).all()
    _same(dsurf, dp, want, "rounding edges")


def test_the_largest_sum_the_limit_allows():
    """sw sh = 2^24, the limit: a 4096 x 4096 rectangle into one pixel. All 255: the largest sum, 255 * 2^24 + 2^23 with the rounding term, still
    below 2^32. Then 254 with 2^23 - 1 and with 2^23 bytes raised to 255: the sums 254 D + D / 2 - 1 and 254 D + D / 2, out 254 and 255."""
    n = 4096
    D = n * n
    frames = []
    for raised in (None, D // 2 - 1, D // 2):
        Y = np.full(D, 255 if raised is None else 254, np.uint8)
        if raised is not None:
            Y[:raised] = 255
        frames.append([Y.reshape(n, n), np.full((n // 2, n), 128, np.uint8)])
    dp = [ref.noise_planes("nv12", 6, 8, 8)]
    sb = FrameBatch(3, DEV, format="nv12").set([tuple(torch.from_numpy(p).to(DEV) for p in f) for f in frames])
    db, dsurf = _batch("nv12", SPACE, dp, "w+1")
    items = [(i, (0, 0, n, n), 0, (2 * i, 2, 1, 1)) for i in range(3)]
    compose.Compositor(3, DEV).set(ref.api_items(items), sb, db)(sb, db)
    torch.cuda.synchronize()
    want = ref.compose(frames, dp, items, ("nv12",) + SPACE, ("nv12",) + SPACE)
    assert want[0][0][2, [0, 2, 4]].tolist() == [255, 254, 255]
    _same(dsurf, dp, want, "largest sum")


# ---------------------------------------------------------------------------------------------------------------- 3. clear
@pytest.mark.parametrize("dfmt", ["nv12", "i420", "bgr24"])
def test_clear_then_items(dfmt):
    _run(("nv12",) + SPACE, (dfmt, "bt601", False), ref.second_items(rr.SIZES), clear=(200, 30, 90), dst_pitch="w+1", what="clear " + dfmt)
    assert _lib.debug_last_kernel().startswith("compose_")


# ---------------------------------------------------------------------------------------------------------------- 4. a captured call
def test_a_captured_call_follows_surfaces_items_and_the_item_count():
    src, dst = ("nv12",) + SPACE, ("i420",) + SPACE
    sp = [_planes("nv12", rr.SIZES, 940), _planes("nv12", rr.SIZES, 960)]
    dp = _planes("i420", ref.DST_SIZES, 950)
    sb, _ = _batch("nv12", SPACE, sp[0], "w+1")
    db, _ = _batch("i420", SPACE, dp, "256")
    mixed, second = ref.mixed_items(rr.SIZES), ref.second_items(rr.SIZES)
    comp = compose.Compositor(16, DEV).set(ref.api_items(mixed), sb, db)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        comp(sb, db)                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        comp(sb, db)
    tables = (sb.table.data_ptr(), db.table.data_ptr(), comp.table.data_ptr())
    assert len(second) != len(mixed)
    got = []
    for which, items in ((0, mixed), (1, mixed), (1, second), (1, second[:2]), (1, second[:2])):
        sb.set([tgr._surface("nv12", p, "w+1", GAP) for p in sp[which]])                 # other source surfaces ...
        dsurf = [tgr._surface("i420", p, "256", GAP) for p in dp]
        db.set(dsurf)                                                                     # ... fresh destinations ...
        comp.set(ref.api_items(items), sb, db)                                            # ... other items, another count
        assert (sb.table.data_ptr(), db.table.data_ptr(), comp.table.data_ptr()) == tables
        graph.replay()
        torch.cuda.synchronize()
        _same(dsurf, dp, ref.compose(sp[which], dp, items, src, dst), "replay on {} items".format(len(items)))
        got.append([p.copy() for s, planes in zip(dsurf, dp) for p in _payloads(s, planes)])
    assert all(np.array_equal(a, b) for a, b in zip(got[3], got[4]))          # two replays on equal inputs: equal bits
    comp.set([], sb, db)                                                       # no item: nothing is written
    dsurf = [tgr._surface("i420", p, "256", GAP) for p in dp]
    db.set(dsurf)
    graph.replay()
    torch.cuda.synchronize()
    _same(dsurf, dp, dp, "replay on no items")


# ---------------------------------------------------------------------------------------------------------------- 5. behind the tracker
def test_compose_behind_the_paint_of_a_tracking_step():
    m = models.load_synthetic(models.ssd_lite_mobilenet_v2(image_size=160, num_classes=3), 0).to(DEV)
    try:
        fmt = "nv12"
        sp = [tgr._source(fmt, "bt709", False, 930 + i, h, w)[0] for i, (h, w) in enumerate(rr.SIZES)]
        dp = _planes("rgb24", ref.DST_SIZES, 950)
        kw = dict(max_tracks=64, track_thresh=0.05, low_thresh=0.01, new_thresh=0.05)
        trackers = [ByteTracker(2, DEV, **kw) for _ in range(3)]
        ov = osd.Overlay(2, DEV, names=["background", "thing", "other"], scale=1)
        items = ref.mixed_items(rr.SIZES)

        def fresh():
            sb, ssurf = _batch(fmt, SPACE, sp, "256")
            db, dsurf = _batch("rgb24", SPACE, dp, "w+1")
            return sb, ssurf, db, dsurf
        painted = 0
        for step in range(3):
            a_sb, a_ss, a_db, a_ds = fresh()
            b_sb, b_ss, b_db, b_ds = fresh()
            c_sb, c_ss, _, _ = fresh()
            comp_a = compose.Compositor(16, DEV).set(ref.api_items(items), a_sb, a_db)
            comp_b = compose.Compositor(16, DEV).set(ref.api_items(items), b_sb, b_db)
            outs_a = [t.clone() for t in m.track_frames(a_sb, trackers[0], osd=ov, compose=comp_a, wall=a_db)[:6]]
            outs_b = [t.clone() for t in m.track_frames(b_sb, trackers[1], osd=ov)[:6]]
            comp_b(b_sb, b_db)
            outs_c = [t.clone() for t in m.track_frames(c_sb, trackers[2], compose=None, wall=None)[:6]]       # None: today's call
            torch.cuda.synchronize()
            assert all(torch.equal(x, y) for x, y in zip(outs_a, outs_b)) and all(torch.equal(x, y) for x, y in zip(outs_a, outs_c))
            pa = [p for s, planes in zip(a_ss, sp) for p in _payloads(s, planes)]
            pb = [p for s, planes in zip(b_ss, sp) for p in _payloads(s, planes)]
            pc = [p for s, planes in zip(c_ss, sp) for p in _payloads(s, planes)]
            assert all(np.array_equal(x, y) for x, y in zip(pa, pb))                                # the same paint
            assert all(np.array_equal(x, y) for x, planes in zip([pc[:2], pc[2:]], sp) for x, y in zip(x, planes))      # compose=None: frames untouched
            painted += int(any(not np.array_equal(x, y) for x, y in zip(pa, pc)))
            wa = [p for s, planes in zip(a_ds, dp) for p in _payloads(s, planes)]
            wb = [p for s, planes in zip(b_ds, dp) for p in _payloads(s, planes)]
            assert all(np.array_equal(x, y) for x, y in zip(wa, wb))                                # the keyword = the explicit call behind the step
            want = ref.compose([pa[:2], pa[2:]], dp, items, (fmt,) + SPACE, ("rgb24",) + SPACE)     # ... = the reference on the PAINTED frames
            _same(a_ds, dp, want, "behind the paint, step {}".format(step))
        assert painted >= 1
        with pytest.raises(ValueError, match="go together"):
            m.track_frames(a_sb, trackers[0], compose=comp_a)
        with pytest.raises(ValueError, match="expected a Compositor"):
            m.track_frames(a_sb, trackers[0], compose=ov, wall=a_db)
    finally:
        m.release()


def test_compose_behind_the_sliced_and_the_appearance_steps():
    """compose= / wall= of track_sliced_frames (with and without motion=) and track_frames_appearance: the outputs are those of the call without
    them, and the wall equals the explicit composition behind that call -- which the test above holds against the reference."""
    from demonet_amd.crops import ObjectCropper
    from demonet_amd.motion import MotionCompensator
    from demonet_amd.sliced import FrameSlicer
    from demonet_amd.track import AppearanceTracker
    m = models.load_synthetic(models.ssd_lite_mobilenet_v2(image_size=160, num_classes=3), 0).to(DEV)
    try:
        fmt = "nv12"
        sp = [tgr._source(fmt, "bt709", False, 930 + i, h, w)[0] for i, (h, w) in enumerate(rr.SIZES)]
        dp = _planes("i420", ref.DST_SIZES, 950)
        kw = dict(max_tracks=64, track_thresh=0.05, low_thresh=0.01, new_thresh=0.05)
        ov = osd.Overlay(2, DEV, names=["background", "thing", "other"], scale=1)
        items = ref.api_items(ref.second_items(rr.SIZES))
        slicer = FrameSlicer(m, rr.SIZES, max_tiles_per_forward=3)
        dim = 32
        W = torch.from_numpy(np.random.RandomState(9).normal(0, 1, (3 * 16 * 8, dim)).astype(np.float32)).to(DEV)
        embedder = lambda patches: patches.reshape(patches.shape[0], -1).float() @ W      # noqa: E731

        def cropper():
            c = ObjectCropper(2, DEV, size=(16, 8), capacity=128, dtype=torch.float16)
            c.patches.zero_()
            return c

        def sliced(batch, tracker, extra, **kwargs):
            return m.track_sliced_frames(batch, tracker, slicer, osd=ov, **kwargs)

        def sliced_motion(batch, tracker, extra, **kwargs):
            return m.track_sliced_frames(batch, tracker, slicer, motion=extra, osd=ov, **kwargs)

        def appearance(batch, tracker, extra, **kwargs):
            return m.track_frames_appearance(batch, tracker, extra, embedder, osd=ov, **kwargs)
        cases = (("sliced", sliced, lambda: ByteTracker(2, DEV, **kw), lambda: None),
                 ("sliced with motion", sliced_motion, lambda: ByteTracker(2, DEV, **kw), lambda: MotionCompensator(2, DEV, max_size=(120, 160), mask_thresh=2.0)),
                 ("appearance", appearance, lambda: AppearanceTracker(2, DEV, dim, **kw), cropper))
        for name, step, make_tracker, make_extra in cases:
            ta, tb, ea, eb = make_tracker(), make_tracker(), make_extra(), make_extra()
            for n in range(2):
                a_sb, a_ss = _batch(fmt, SPACE, sp, "256")
                b_sb, b_ss = _batch(fmt, SPACE, sp, "256")
                a_db, a_ds = _batch("i420", SPACE, dp, "w+1")
                b_db, b_ds = _batch("i420", SPACE, dp, "w+1")
                comp_a = compose.Compositor(8, DEV).set(items, a_sb, a_db)
                comp_b = compose.Compositor(8, DEV).set(items, b_sb, b_db)
                outs_a = [t.clone() for t in step(a_sb, ta, ea, compose=comp_a, wall=a_db)[:6]]
                outs_b = [t.clone() for t in step(b_sb, tb, eb)[:6]]
                comp_b(b_sb, b_db)
                torch.cuda.synchronize()
                assert all(torch.equal(x, y) for x, y in zip(outs_a, outs_b)), (name, n)
                frames_a = [p for s_, planes in zip(a_ss, sp) for p in _payloads(s_, planes)]
                frames_b = [p for s_, planes in zip(b_ss, sp) for p in _payloads(s_, planes)]
                assert all(np.array_equal(x, y) for x, y in zip(frames_a, frames_b)), (name, n)
                walls_a = [p for s_, planes in zip(a_ds, dp) for p in _payloads(s_, planes)]
                walls_b = [p for s_, planes in zip(b_ds, dp) for p in _payloads(s_, planes)]
                assert all(np.array_equal(x, y) for x, y in zip(walls_a, walls_b)), (name, n)
                _same(a_ds, dp, ref.compose([frames_a[:2], frames_a[2:]], dp, ref.second_items(rr.SIZES), (fmt,) + SPACE, ("i420",) + SPACE), name)
            with pytest.raises(ValueError, match="go together"):
                step(a_sb, ta, ea, wall=a_db)
    finally:
        m.release()


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_every_error_code_of_the_entry_points():
    DN_E_INVALID, DN_E_UNSUPPORTED = -1, -4
    sp, dp = _planes("nv12", rr.SIZES, 940), _planes("nv12", ref.DST_SIZES, 950)
    sb, _ = _batch("nv12", SPACE, sp, "w+1")
    db, dsurf = _batch("nv12", SPACE, dp, "w+1")
    comp = compose.Compositor(16, DEV).set(ref.api_items(ref.mixed_items(rr.SIZES)), sb, db)
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda v: C.c_void_p(v) if v else None      # noqa: E731

    def call(**kw):
        a = dict(src=sb.table.data_ptr(), sf=0, sc=1, dst=db.table.data_ptr(), df=0, dc=1, table=comp.table.data_ptr(), capacity=16)
        a.update(kw)
        return L.dn_compose(p(a["src"]), a["sf"], a["sc"], p(a["dst"]), a["df"], a["dc"], p(a["table"]), a["capacity"], stream)
    for kw in (dict(src=0), dict(dst=0), dict(table=0), dict(src=sb.table.data_ptr() + 4), dict(dst=db.table.data_ptr() + 2), dict(table=comp.table.data_ptr() + 8),
               dict(capacity=0), dict(capacity=-3), dict(sf=4), dict(df=-1), dict(sc=2), dict(dc=0x20), dict(sc=0x13)):
        assert call(**kw) == DN_E_INVALID, kw
        assert L.dn_last_error()
    assert call(capacity=65537) == DN_E_UNSUPPORTED
    fill = lambda **kw: L.dn_surface_fill(p(kw.get("frames", db.table.data_ptr())), kw.get("n", 2), kw.get("fmt", 0), *kw.get("c", (1, 2, 3)), stream)      # noqa: E731
    for kw in (dict(frames=0), dict(frames=db.table.data_ptr() + 4), dict(n=0), dict(fmt=7), dict(c=(256, 0, 0)), dict(c=(0, -1, 0))):
        assert fill(**kw) == DN_E_INVALID, kw
    assert fill(n=65536) == DN_E_UNSUPPORTED
    torch.cuda.synchronize()
    _same(dsurf, dp, dp, "every error is raised before anything is enqueued")
    assert call() == 0 and fill() == 0
    torch.cuda.synchronize()
    got = [p_ for s, planes in zip(dsurf, dp) for p_ in _payloads(s, planes)]
    assert (got[0] == 1).all() and (got[1][:, 0::2] == 2).all() and (got[1][:, 1::2] == 3).all()        # the fill came last: whole payloads, gaps kept
