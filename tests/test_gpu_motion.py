"""Camera-motion compensation on the device (dn_motion_estimate, dn_track_compensate, motion.MotionCompensator, ByteTracker.compensate,
SSD.track_*(motion=...)): thumbnails, every block's (dx, dy, sad, valid), stats and the bits of the motion equal tests/motion_ref.py; the warped
tracker state equals motion_ref.compensate on track_ref.RefTracker bit for bit. The frames are the smallest that still have structure: 96 x 128
(k = 1, 4 x 6 blocks), 135 x 241 (k = 2 or 3, remainders on both axes) and 270 x 480 (k = 4: the wide-load paths)."""
import numpy as np
import pytest
import torch

import motion_ref as mr
import track_ref as tr
from demonet_amd import models
from demonet_amd.frames import FrameBatch
from demonet_amd.motion import MotionCompensator
from demonet_amd.track import AppearanceTracker, ByteTracker

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32
PITCH = {"w": lambda p: p, "w+1": lambda p: p + 1, "w+4": lambda p: p + 4, "256": lambda p: (p + 255) // 256 * 256}
SIZES3 = [(96, 128), (135, 241), (270, 480)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _pitched(plane, pitch):
    """The [rows, payload] plane on the device as a view of an allocation whose rows are `pitch` bytes apart; the gap bytes are 0xA5."""
    rows, payload = plane.shape
    buf = np.full((rows, pitch(payload)), 0xA5, np.uint8)
    buf[:, :payload] = plane
    return _dev(buf)[:, :payload]


def _image(fmt, y, seed):
    """What the reference sees of a frame whose first channel is y: the luma plane itself, or an [H, W, 3] image for the packed formats."""
    if fmt in ("nv12", "i420"):
        return y
    return np.stack([y, 255 - y, y // 2 + (seed & 63)], axis=2)             # three channels that move together and weigh differently


def _surface(fmt, img, pitch="w", seed=0):
    rng = np.random.RandomState(seed)
    if fmt in ("rgb24", "bgr24"):
        H, W, _ = img.shape
        return _pitched(img.reshape(H, 3 * W), PITCH[pitch]).unflatten(1, (-1, 3))
    H, W = img.shape
    ch, cw = (H + 1) // 2, (W + 1) // 2
    if fmt == "nv12":
        return (_pitched(img, PITCH[pitch]), _pitched(rng.randint(0, 256, (ch, 2 * cw)).astype(np.uint8), PITCH[pitch]))
    return (_pitched(img, PITCH[pitch]),) + tuple(_pitched(rng.randint(0, 256, (ch, cw)).astype(np.uint8), PITCH[pitch]) for _ in range(2))


def _check_step(mc, ref, fmt, images, dets=None, where=""):
    """One step of both on the same frames; everything the device produced is compared with the reference. -> (motion, stats) of the reference."""
    lumas = [mr.luma(im, fmt) for im in images]
    if dets is None:
        want_m, want_s, want_v = ref.estimate(lumas)
    else:
        want_m, want_s, want_v = ref.estimate(lumas, dets[0], dets[1], dets[2])
    got_m, got_s = mc.motion.cpu().numpy(), mc.stats.cpu().numpy()
    got_v = mc.vectors().cpu().numpy()
    both, parity = mc.thumbnails()
    both, parity = both.cpu().numpy(), parity.cpu().numpy()
    for b, t in enumerate(ref.thumbs):
        th, tw = t.shape
        assert np.array_equal(both[b, parity[b], :th, :tw], t), (where, b, "thumbnail")
    assert np.array_equal(got_v, want_v), (where, "vectors", np.argwhere(got_v != want_v)[:4].tolist())
    assert np.array_equal(got_s, want_s), (where, got_s.tolist(), want_s.tolist())
    assert np.array_equal(_bits(got_m), _bits(want_m)), (where, got_m.tolist(), want_m.tolist())
    return want_m, want_s


def _camera(seed, H, W, positions, cell=4):
    """The views of one textured canvas from the camera positions (x, y)."""
    mx, my = max(p[0] for p in positions), max(p[1] for p in positions)
    canvas = mr.textured(seed, H + my, W + mx, cell)
    return [mr.window(canvas, x, y, H, W) for x, y in positions]


# ---------------------------------------------------------------------------------------------------------------- 1. estimate
@pytest.mark.parametrize("pitch", list(PITCH))
@pytest.mark.parametrize("fmt", ["nv12", "i420", "rgb24", "bgr24"])
def test_formats_pitches_odd_and_mixed_sizes_in_one_batch(fmt, pitch):
    """Three streams of three sizes (k = 1, 2, 4), planes pitched four ways: rows at the width, one byte more (nothing is aligned: the byte path),
    four bytes more (4-byte loads) and at multiples of 256 (16-byte loads)."""
    mc, ref = MotionCompensator(3, DEV, max_size=(96, 128)), mr.RefCompensator(3, (96, 128))
    batch = FrameBatch(3, DEV, fmt)
    pos = [(20, 12), (27, 9), (21, 17)]
    views = [_camera(10 + b, H, W, pos, cell=4 * (b + 1)) for b, (H, W) in enumerate(SIZES3)]
    oks = []
    for step in range(3):
        images = [_image(fmt, views[b][step], 50 + b) for b in range(3)]
        mc.estimate(batch.set([_surface(fmt, im, pitch, b) for b, im in enumerate(images)]))
        m, s = _check_step(mc, ref, fmt, images, where=step)
        oks.append(m[:, 3].tolist())
        assert s[:, 3].tolist() == [1, 2, 4] and s[:, 0].tolist() == [24, 10, 10]
    assert oks[0] == [0, 0, 0] and oks[1] == [1, 1, 1] and oks[2] == [1, 1, 1]


@pytest.mark.parametrize("block,radius,size,cap", [(8, 1, (135, 241), (64, 96)), (8, 7, (135, 241), (64, 96)), (8, 16, (135, 241), (64, 96)),
                                                   (16, 1, (135, 241), (64, 96)), (16, 7, (135, 241), (64, 96)), (16, 16, (96, 128), (144, 256))])
def test_blocks_and_radii(block, radius, size, cap):
    """One stream (B = 1), k = 3 with remainder rows and columns for five of the six; shifts inside and beyond the radius."""
    H, W = size
    k = mr.box_side(H, W, *cap)
    mc, ref = MotionCompensator(1, DEV, max_size=cap, block=block, radius=radius, min_blocks=4), mr.RefCompensator(1, cap, block, radius, min_blocks=4)
    batch = FrameBatch(1, DEV, "nv12")
    pos = [(60, 60), (60 + k, 60), (60 + k - 3 * k, 60 + 2 * k), (60 - 2 * k - 20 * k, 60 + 2 * k), (1, 59)]
    pos = [(max(x, 0), y) for x, y in pos]
    for step, y in enumerate(_camera(3, H, W, pos, cell=2 * k)):
        mc.estimate(batch.set([_surface("nv12", y)]))
        m, s = _check_step(mc, ref, "nv12", [y], where=step)
        if step == 1:
            assert m[0].tolist() == [1.0, -float(k), 0.0, 1.0]          # the camera went right by one thumbnail pixel: the image goes left


def test_65_streams():
    B = 65
    mc, ref = MotionCompensator(B, DEV, max_size=(48, 64), radius=7, min_blocks=4), mr.RefCompensator(B, (48, 64), 16, 7, min_blocks=4)
    batch = FrameBatch(B, DEV, "i420")
    pos = [(8, 8), (11, 6)]
    views = [_camera(200 + b, 48, 64, [(x + b % 5, y + b % 3) for x, y in pos] if b % 2 else pos, cell=3) for b in range(B)]
    for step in range(2):
        images = [views[b][step] for b in range(B)]
        mc.estimate(batch.set([_surface("i420", im, "w", b) for b, im in enumerate(images)]))
        m, s = _check_step(mc, ref, "i420", images, where=step)
    assert m[:, 3].sum() >= B - 2 and (s[:, 0] == 6).all()


def test_ties_in_sad_go_to_the_stated_order():
    """A texture of period 4 in x and 8 in y: every block has dozens of candidates with SAD 0. The order (SAD, dx^2 + dy^2, dy, dx) decides."""
    H, W = 96, 128
    tile = np.random.RandomState(5).randint(0, 256, (8, 4)).astype(np.uint8)
    canvas = np.tile(tile, (H // 8 + 2, W // 4 + 2))
    mc, ref = MotionCompensator(1, DEV, max_size=(96, 128)), mr.RefCompensator(1, (96, 128))
    batch = FrameBatch(1, DEV, "nv12")
    want = [None, (-2, 0), (-2, 1), (-2, -4)]             # the camera steps (2, 0), (2, 1), (2, 4): the nearest of the equivalent shifts, then dy, dx
    for step, (x, y) in enumerate([(0, 0), (2, 0), (4, 1), (6, 5)]):
        img = mr.window(canvas, x, y, H, W)
        mc.estimate(batch.set([_surface("nv12", img)]))
        _check_step(mc, ref, "nv12", [img], where=step)
        v = mc.vectors().cpu().numpy()[0]
        if want[step] is not None:
            assert (v[:, 2] == 0).all() and {(int(a), int(b)) for a, b in v[:, :2]} == {want[step]}, (step, v[:3])


def test_masking_with_garbage_beyond_the_count_and_nan_scores():
    B, d = 3, 6
    mc, ref = MotionCompensator(B, DEV, max_size=(96, 128), min_blocks=4), mr.RefCompensator(B, (96, 128), min_blocks=4)
    batch = FrameBatch(B, DEV, "nv12")
    views = [_camera(30 + b, 96, 128, [(4, 4), (9, 2)]) for b in range(B)]
    rng = np.random.RandomState(0)
    boxes = rng.uniform(0, 128, (B, d, 4)).astype(f32)
    boxes[:, :, 2:] = boxes[:, :, :2] + 70                                  # garbage that WOULD mask, beyond the counts
    scores = np.full((B, d), 0.9, f32)
    counts = np.array([0, d, 2], np.int32)
    boxes[1, 0] = (16, 16, 64, 64)                                          # masks the nine blocks with centres at 23.5, 39.5, 55.5 ...
    boxes[1, 1], scores[1, 1] = (64, 16, 128, 96), np.nan                   # ... a NaN score masks nothing
    boxes[1, 2], scores[1, 2] = (64, 16, 128, 96), 0.4                      # below mask_thresh
    boxes[1, 3] = (np.inf, 0, 128, 96)
    boxes[1, 4] = (87.5, 23.5, 88.5, 24.5)                                  # the centre (87.5, 23.5) of block 4: x1 <= c < x2
    boxes[1, 5] = (103.0, 0, 103.5, 96)                                     # c = 103.5 is not < x2
    boxes[2, 0] = (0, 0, 128, 96)                                           # everything masked: not ok
    boxes[2, 1] = (0, 0, 1, 1)
    dets = (boxes, scores, counts)
    dd = [_dev(a) for a in dets]
    for step in range(2):
        images = [views[b][step] for b in range(B)]
        mc.estimate(batch.set([_surface("nv12", im) for im in images]), *dd)
        m, s = _check_step(mc, ref, "nv12", images, dets, where=step)
    assert s[:, 1].tolist() == [24, 14, 0] and m[:, 3].tolist() == [1, 1, 0]
    with pytest.raises(ValueError, match="together"):
        mc.estimate(batch, dd[0], dd[1])
    with pytest.raises(ValueError, match="shape"):
        mc.estimate(batch, dd[0][:, :3], dd[1], dd[2])


def _sequence():
    """(images per step, action before the step): stream 1 is reset before step 3, stream 0 changes its size at step 4."""
    a = _camera(40, 96, 128, [(10, 10), (13, 11), (13, 6), (20, 6), (22, 9), (25, 9)])
    b = _camera(41, 135, 241, [(10, 10), (14, 12), (18, 14), (22, 16), (26, 18), (30, 20)], cell=8)
    c = _camera(42, 96, 112, [(0, 0), (3, 1)])
    return [([a[0], b[0]], None), ([a[1], b[1]], None), ([a[2], b[2]], None), ([a[3], b[3]], "reset1"), ([c[0], b[4]], None), ([c[1], b[5]], None)]


def test_reset_size_change_state_dict_and_two_runs_give_the_same_bits():
    seq = _sequence()
    mk = lambda: MotionCompensator(2, DEV, max_size=(96, 128), min_blocks=4)
    first, second, resumed = mk(), mk(), mk()
    ref = mr.RefCompensator(2, (96, 128), min_blocks=4)
    batch = FrameBatch(2, DEV, "nv12")
    oks, keep = [], []
    for step, (images, action) in enumerate(seq):
        if action == "reset1":
            first.reset([1])
            ref.reset([1])
        first.estimate(batch.set([_surface("nv12", im) for im in images]))
        m, s = _check_step(first, ref, "nv12", images, where=step)
        oks.append(m[:, 3].tolist())
        keep.append((first.motion.clone(), first.stats.clone(), first.vectors().clone(), first.state.clone()))
        if step == 2:
            sd = first.state_dict()
            assert sd["state"].device.type == "cpu" and sd["params"]["block"] == 16
    assert oks == [[0, 0], [1, 1], [1, 1], [1, 0], [0, 1], [1, 1]]
    resumed.load_state_dict(sd)
    with pytest.raises(ValueError):
        MotionCompensator(2, DEV, max_size=(96, 128), block=8).load_state_dict(sd)
    for step, (images, action) in enumerate(seq):
        batch.set([_surface("nv12", im) for im in images])
        for mc in (second,) + ((resumed,) if step > 2 else ()):
            if action == "reset1":
                mc.reset([1])
            mc.estimate(batch)
            for got, want in zip((mc.motion, mc.stats, mc.vectors(), mc.state), keep[step]):
                assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), step


def test_graph_replay_of_four_frames_with_set_between_replays():
    seq = _camera(60, 135, 241, [(10, 10), (14, 12), (18, 9), (25, 9), (25, 15), (21, 19)], cell=8)
    eager, captured = MotionCompensator(1, DEV, max_size=(96, 128), min_blocks=4), MotionCompensator(1, DEV, max_size=(96, 128), min_blocks=4)
    be, bc = FrameBatch(1, DEV, "nv12"), FrameBatch(1, DEV, "nv12")
    for img in seq[:2]:
        eager.estimate(be.set([_surface("nv12", img, "256")]))
        captured.estimate(bc.set([_surface("nv12", img, "256")]))
    torch.cuda.synchronize()
    snap = captured.state.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.estimate(bc)
    captured.state.copy_(snap)                           # (the capture enqueued nothing)
    oks = 0
    for i, img in enumerate(seq[2:]):
        bc.set([_surface("nv12", img, "w+4" if i % 2 else "256")])          # new surfaces, another pitch: the table is read when the kernels run
        graph.replay()
        m, _ = eager.estimate(be.set([_surface("nv12", img, "256")]))
        torch.cuda.synchronize()
        assert torch.equal(captured.motion.view(torch.int32), m.view(torch.int32)) and torch.equal(captured.stats, eager.stats), i
        assert torch.equal(captured.vectors(), eager.vectors()) and torch.equal(captured.state, eager.state), i
        oks += int(m[0, 3])
    assert oks == 4


# ---------------------------------------------------------------------------------------------------------------- 2. compensate
@pytest.mark.parametrize("T", [1, 63, 256])
def test_compensate_is_the_reference_on_a_populated_state(T):
    B = 3
    frames, _ = tr.scene(7, 12, B, 32, objects=min(10, max(T, 2)), max_dropout=4)
    dev, ref = ByteTracker(B, DEV, max_tracks=T, track_buffer=4), tr.RefTracker(B, T, track_buffer=4)
    seen = set()
    motions = [np.array([[1.03125, 7.5, -3.25, 1], [0.9, 100.0, 2.0, 0], [0.97, -11.125, 0.3, 1]], f32),
               np.array([[1.0, 0.0, 0.0, 1], [1.1, -4.7, 19.0, 1], [np.nan, np.nan, np.nan, 0]], f32)]
    for i, fr in enumerate(frames):
        if i >= 4:
            mo = motions[i % 2]
            before = dev.state.clone()
            dev.compensate(_dev(mo))
            mr.compensate(ref, mo)
            tab = {k: v.cpu().numpy() for k, v in dev.table().items()}
            for k in tr.RefTracker.FIELDS:
                want = getattr(ref, k)
                assert np.array_equal(tab[k].view(np.uint32) if want.dtype == f32 else tab[k], want.view(np.uint32) if want.dtype == f32 else want), (i, k)
            for b in range(B):
                if mo[b, 3] == 0:
                    assert torch.equal(dev.state[b], before[b]), (i, b)              # a stream that is not ok is not written at all
                elif mo[b, 0] != 1 and ref.state[b].any():
                    assert not torch.equal(dev.state[b], before[b]), (i, b)
            seen |= set(np.unique(ref.state).tolist())
        want = ref.update(*fr)
        got = dev.update(*[_dev(a) for a in fr])
        for w, g in zip(want, got):
            g = g.cpu().numpy()
            assert np.array_equal(g.view(np.uint32) if w.dtype == f32 else g, w.view(np.uint32) if w.dtype == f32 else w), i
    assert seen >= ({tr.FREE, tr.TENTATIVE, tr.TRACKED, tr.LOST} if T > 1 else {tr.TRACKED})
    with pytest.raises(ValueError, match="motion must be"):
        dev.compensate(_dev(motions[0][:2]))


# ---------------------------------------------------------------------------------------------------------------- 3. the point of it
def _pan_scene(frames=20):
    """A textured world seen by a camera that jerks by 24 px per frame, the direction reversing every third frame, and three flat objects
    that drift slowly over the world. -> per frame (image [192, 256], boxes [1, 4, 4], scores, labels, counts, the camera's x)."""
    H, W, step = 192, 256, 24
    world = mr.textured(77, H, W + 160, 6)
    objs = [dict(p=(130.0, 30.0), v=(1.0, 0.5), w=26, h=40, g=20), dict(p=(190.0, 90.0), v=(-1.0, 0.25), w=30, h=44, g=128),
            dict(p=(240.0, 40.0), v=(0.5, 1.0), w=24, h=36, g=235)]
    cam, out = 72, []
    for f in range(frames):
        if f:
            cam += step if (f // 3) % 2 == 0 else -step
        img = mr.window(world, cam, 0, H, W).copy()
        boxes, scores = np.zeros((1, 4, 4), f32), np.zeros((1, 4), f32)
        for j, o in enumerate(objs):
            x, y = int(round(o["p"][0] + f * o["v"][0])) - cam, int(round(o["p"][1] + f * o["v"][1]))       # world position minus the camera's
            boxes[0, j], scores[0, j] = (x, y, x + o["w"], y + o["h"]), 0.9
            img[y:y + o["h"], x:x + o["w"]] = o["g"]
        out.append((img, boxes, scores, np.ones((1, 4), np.int64), np.array([3], np.int32), cam))
    return out


def test_a_jerking_camera_reissues_ids_without_compensation_and_keeps_them_with_it():
    scene = _pan_scene()
    cams = [s[5] for s in scene]
    assert all(abs(a - b) == 24 for a, b in zip(cams[1:], cams[:-1]))
    for s in scene:                                          # every object is wholly inside every frame
        assert (s[1][0, :3, :2] >= 0).all() and (s[1][0, :3, 2] <= 256).all() and (s[1][0, :3, 3] <= 192).all()
    kw = dict(max_tracks=16)
    plain, comp, ref = ByteTracker(1, DEV, **kw), ByteTracker(1, DEV, **kw), tr.RefTracker(1, 16)
    mc, rc = MotionCompensator(1, DEV, max_size=(96, 128)), mr.RefCompensator(1, (96, 128))
    batch = FrameBatch(1, DEV, "nv12")
    ids_plain, ids_comp = [], []
    for f, (img, boxes, scores, labels, counts, _) in enumerate(scene):
        dets = [_dev(a) for a in (boxes, scores, labels, counts)]
        ids_plain.append(plain.update(*dets)[6][0, :3].tolist())
        motion, _ = mc.estimate(batch.set([_surface("nv12", img)]), dets[0], dets[1], dets[3])
        comp.compensate(motion)
        got = [o.cpu().numpy() for o in comp.update(*dets)]
        want_m, _ = _check_step(mc, rc, "nv12", [img], (boxes, scores, counts), where=f)
        if f:
            assert want_m[0, 3] == 1 and abs(want_m[0, 0] - 1) < 0.02 and abs(abs(want_m[0, 1]) - 24) <= 1 and abs(want_m[0, 2]) <= 1, (f, want_m)
        mr.compensate(ref, want_m)
        want = ref.update(boxes, scores, labels, counts)
        for w, g in zip(want, got):
            assert np.array_equal(g.view(np.uint32) if w.dtype == f32 else g, w.view(np.uint32) if w.dtype == f32 else w), f
        tab = {k: v.cpu().numpy() for k, v in comp.table().items()}
        for k in tr.RefTracker.FIELDS:
            w = getattr(ref, k)
            assert np.array_equal(tab[k].view(np.uint32) if w.dtype == f32 else tab[k], w.view(np.uint32) if w.dtype == f32 else w), (f, k)
        ids_comp.append(got[6][0, :3].tolist())
    assert all(row == [1, 2, 3] for row in ids_comp), ids_comp                 # one id per object over the 20 frames
    assert int(plain.table()["next_id"][0]) > 4, ids_plain                     # the scene is hard: ByteTrack alone hands out new ids
    assert sum(i == -1 for row in ids_plain for i in row) >= 30                 # ... while its tracks miss the objects in most frames


# ---------------------------------------------------------------------------------------------------------------- 4. behind the model
def _model_frames(step):
    return [mr.window(mr.textured(90 + b, 260, 380, 6), 8 * step + b, 4 * step, 240, 320) for b in range(2)]


@pytest.fixture(scope="module")
def v3():
    m = models.load_synthetic(models.ssdlite320_mobilenet_v3_large(num_classes=21, score_thresh=0.02), 0).to(DEV).eval()
    yield m
    m.release()


TKW = dict(max_tracks=64, track_thresh=0.05, low_thresh=0.01, new_thresh=0.05)
# synthetic weights put hundreds of boxes everywhere: at the default mask_thresh they would mask every block and every step would be the identity.
# No score reaches 2, so the detections travel the whole way and the motion that is applied is a real one.
MK_M = lambda: MotionCompensator(2, DEV, max_size=(120, 160), mask_thresh=2.0)


def _equal_outs(got, want, where):
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and torch.equal(g.view(torch.uint8), w.view(torch.uint8)), (where, i)


def test_ssd_track_frames_with_motion_is_the_composition_and_without_it_is_todays(v3):
    m = v3
    ta, tb, tc, td = (ByteTracker(2, DEV, **TKW) for _ in range(4))
    ma, mb = MK_M(), MK_M()
    batch = FrameBatch(2, DEV, "nv12")
    rows = oks = 0
    for step in range(3):
        batch.set([_surface("nv12", y, "256", b) for b, y in enumerate(_model_frames(step))])
        got = [o.clone() for o in m.track_frames(batch, ta, motion=ma)]
        boxes, scores, labels, counts = m.forward_frames(batch)
        motion, _ = mb.estimate(batch, boxes, scores, counts)
        tb.compensate(motion)
        _equal_outs(got, tb.update(boxes, scores, labels, counts), step)
        assert torch.equal(ta.state, tb.state) and torch.equal(ma.state, mb.state) and torch.equal(ma.motion.view(torch.int32), mb.motion.view(torch.int32))
        none = [o.clone() for o in m.track_frames(batch, tc, motion=None)]
        _equal_outs(none, td.update(*m.forward_frames(batch)), step)
        assert torch.equal(tc.state, td.state)
        rows += int(got[5].sum())
        oks += int(motion[:, 3].sum())
    assert rows > 0 and oks == 4
    with pytest.raises(ValueError, match="MotionCompensator"):
        m.track_frames(batch, ta, motion=ma.motion)
    with pytest.raises(ValueError, match="streams"):
        m.track_frames(batch, ta, motion=MotionCompensator(3, DEV))


def test_ssd_track_sliced_frames_and_track_frames_appearance_with_motion(v3):
    from demonet_amd.crops import ObjectCropper
    from demonet_amd.sliced import FrameSlicer
    m = v3
    batch = FrameBatch(2, DEV, "nv12")
    mk_m = MK_M
    # sliced
    ta, tb, tc, td, ma, mb = ByteTracker(2, DEV, **TKW), ByteTracker(2, DEV, **TKW), ByteTracker(2, DEV, **TKW), ByteTracker(2, DEV, **TKW), mk_m(), mk_m()
    slicer = FrameSlicer(m, [(240, 320), (240, 320)], tile=(160, 160), max_tiles_per_forward=16)
    for step in range(2):
        batch.set([_surface("nv12", y, "256", b) for b, y in enumerate(_model_frames(step))])
        got = [o.clone() for o in m.track_sliced_frames(batch, ta, slicer, motion=ma)]
        boxes, scores, labels, counts = [t.clone() for t in slicer(batch)]
        motion, _ = mb.estimate(batch, boxes, scores, counts)
        tb.compensate(motion)
        _equal_outs(got, tb.update(boxes, scores, labels, counts), ("sliced", step))
        assert torch.equal(ta.state, tb.state) and torch.equal(ma.state, mb.state)
        none = [o.clone() for o in m.track_sliced_frames(batch, tc, slicer)]
        _equal_outs(none, td.update(*slicer(batch)), ("sliced none", step))
    assert int(motion[:, 3].sum()) == 2
    # appearance
    dim, cap = 32, 128
    mk_t = lambda: AppearanceTracker(2, DEV, dim, **TKW)
    mk_c = lambda: ObjectCropper(2, DEV, size=(16, 8), capacity=cap, dtype=torch.float16)
    ta, tb, tc, td, ca, cb, cc, cd, ma, mb = mk_t(), mk_t(), mk_t(), mk_t(), mk_c(), mk_c(), mk_c(), mk_c(), mk_m(), mk_m()
    for c in (ca, cb, cc, cd):
        c.patches.zero_()
    Wm = torch.from_numpy(np.random.RandomState(9).normal(0, 1, (3 * 16 * 8, dim)).astype(f32)).to(DEV)
    embedder = lambda patches: patches.reshape(patches.shape[0], -1).float() @ Wm
    for step in range(2):
        batch.set([_surface("nv12", y, "256", b) for b, y in enumerate(_model_frames(step))])
        got = [o.clone() for o in m.track_frames_appearance(batch, ta, ca, embedder, motion=ma)]
        boxes, scores, labels, counts = m.forward_frames(batch)
        motion, _ = mb.estimate(batch, boxes, scores, counts)
        tb.compensate(motion)
        patches, index, _ = cb(batch, boxes, counts, scores >= tb.params.track_thresh)
        _equal_outs(got, tb.update(boxes, scores, labels, counts, embedder(patches), index), ("appearance", step))
        assert torch.equal(ta.state, tb.state) and torch.equal(ta.features_buf, tb.features_buf) and torch.equal(ma.state, mb.state)
        none = [o.clone() for o in m.track_frames_appearance(batch, tc, cc, embedder)]
        boxes, scores, labels, counts = m.forward_frames(batch)
        patches, index, _ = cd(batch, boxes, counts, scores >= td.params.track_thresh)
        _equal_outs(none, td.update(boxes, scores, labels, counts, embedder(patches), index), ("appearance none", step))
        assert torch.equal(tc.state, td.state)
    assert int(motion[:, 3].sum()) == 2
