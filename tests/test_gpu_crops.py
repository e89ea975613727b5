"""Object crops from video surfaces on the device (dn_crop_objects, crops.ObjectCropper, SSD.crop_objects): patches, index and totals equal, bit for
bit, the float32 restatement of the header's rules in tests/crops_ref.py -- for every surface format and colour matrix, pitched rows, both output
types, ragged patch widths, the one-tap path, margins, squares, a full patch table, garbage boxes, a captured graph, and behind the tracker.
Noise frames of tests/regions_ref.SIZES with the surfaces of tests/test_gpu_regions.py; tests/test_crops.py shows that the box set used here tells
four wrong croppers from the right one. The frame table is always valid; the boxes are not."""
import ctypes as C

import numpy as np
import pytest
import torch

import crops_ref as cr
import regions_ref as rr
import test_gpu_regions as tgr
from demonet_amd import _lib, models
from demonet_amd.crops import ObjectCropper
from demonet_amd.frames import FrameBatch
from demonet_amd.track import ByteTracker

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEEDS = (2, 3)                                    # frame b is noise of seed SEEDS[b]
_dev = tgr._dev


def _sources(fmt, matrix, full, sizes=rr.SIZES, seeds=SEEDS):
    return [tgr._source(fmt, matrix, full, s, h, w) for s, (h, w) in zip(seeds, sizes)]


def _batch(fmt, matrix, full, src, pitch="w", gap=0):
    return FrameBatch(len(src), DEV, fmt, matrix, full).set([tgr._surface(fmt, planes, pitch, gap) for planes, _ in src])


def _cropper(p, streams=2):
    return ObjectCropper(streams, DEV, size=(p.out_h, p.out_w), capacity=p.capacity, dtype=torch.float16 if p.fp16 else torch.float32, mean=p.mean,
                         std=p.std, margin=p.margin, square=p.square, min_size=(p.min_h, p.min_w))


def _poison(cropper):
    cropper.patches.view(torch.uint8).fill_(255)
    cropper.index.view(torch.uint8).fill_(255)
    cropper.totals.view(torch.uint8).fill_(255)


def _run(cropper, batch, boxes, counts, select=None):
    """poison the outputs, one step, -> (patches, index, totals) as numpy"""
    _poison(cropper)
    out = cropper(batch, _dev(boxes), _dev(counts), None if select is None else _dev(select))
    torch.cuda.synchronize()
    assert out[0] is cropper.patches and out[1] is cropper.index and out[2] is cropper.totals
    return tuple(t.cpu().numpy() for t in out)


def _check(got, want, what=""):
    """totals and the whole index table equal; the kept patches equal bit for bit; the patches behind them still hold the poison"""
    patches, index, totals = got
    wp, wi, wt = want
    kept = int(wt[0])
    assert totals.tolist() == wt.tolist(), "{} totals".format(what)
    assert np.array_equal(index, wi), "{} index".format(what)
    assert patches.dtype == wp.dtype and patches[:kept].shape == wp.shape
    diff = int((patches[:kept].view(np.uint8) != wp.view(np.uint8)).reshape(kept, -1).any(1).sum()) if kept else 0
    assert diff == 0, "{}: {} of {} patches differ".format(what, diff, kept)
    assert (patches[kept:].view(np.uint8) == 255).all(), "{}: a patch behind the kept ones was written".format(what)


_WANT = {}


def _want(key, rgbs, name):
    """the reference's step of CONFIGS[name] on the set's boxes, once per conversion"""
    if (key, name) not in _WANT:
        boxes, counts = cr.boxes_array()
        _WANT[key, name] = cr.step(rgbs, boxes, counts, rr.SIZES, None, cr.CONFIGS[name])
    return _WANT[key, name]


# ---------------------------------------------------------------------------------------------------------------- 1. formats, matrices, pitches
@pytest.mark.parametrize("fmt,matrix,full", tgr.FORMATS, ids=tgr.IDS)
def test_formats_matrices_and_pitches(fmt, matrix, full):
    src = _sources(fmt, matrix, full)
    key = (matrix, full) if fmt in ("nv12", "i420") else "rgb"
    boxes, counts = cr.boxes_array()
    for name in ("f32-16x8", "imagenet-f16"):
        want = _want(key, [rgb for _, rgb in src], name)
        assert want[2][0] >= 16
        cropper = _cropper(cr.CONFIGS[name])
        for pitch, gap in (("w", 0), ("w+1", 0), ("256", 0xA5)):       # the bytes between a row's payload and the next row must not matter
            _check(_run(cropper, _batch(fmt, matrix, full, src, pitch, gap), boxes, counts), want, "{} pitch {}".format(name, pitch))


# ---------------------------------------------------------------------------------------------------------------- 2. patch sizes and parameters
@pytest.mark.parametrize("name", list(cr.CONFIGS))
def test_patch_sizes_and_parameters(name):
    """(16, 8), (12, 20), the ragged (7, 5) and (6, 9), fp16, (1, 1), mean and std in fp32 (where a reciprocal would show), margin, square, min_size
    and a full table; the set holds a rectangle of exactly (16, 8), a 1 x 1 rectangle and the odd frame's last row and column (tests/test_crops.py)"""
    fmt, matrix, full = "nv12", "bt709", False
    src = _sources(fmt, matrix, full)
    want = _want((matrix, full), [rgb for _, rgb in src], name)
    if name == "overflow":
        assert want[2][1] > 0 and want[2][0] == cr.CONFIGS[name].capacity
    else:
        assert 0 < want[2][0] < cr.CONFIGS[name].capacity and want[2][1] == 0
    boxes, counts = cr.boxes_array()
    _check(_run(_cropper(cr.CONFIGS[name]), _batch(fmt, matrix, full, src, "w+1"), boxes, counts), want, name)


def test_the_index_rows_behind_kept_are_minus_one_and_the_patches_untouched():
    fmt, matrix, full = "i420", "bt601", True
    src = _sources(fmt, matrix, full)
    p = cr.CONFIGS["f16-6x9"]
    boxes, counts = cr.boxes_array()
    want = _want((matrix, full), [rgb for _, rgb in src], "f16-6x9")
    kept = int(want[2][0])
    patches, index, totals = _run(_cropper(p), _batch(fmt, matrix, full, src), boxes, counts)
    assert 0 < kept < p.capacity and totals.tolist() == [kept, 0, 0, 0]
    assert (index[kept:] == np.asarray([-1, 0, 0, 0, 0, 0, 0, 0], dtype=np.int32)).all()
    assert (patches[kept:].view(np.uint8) == 255).all() and not (patches[:kept].view(np.uint8) == 255).all()
    none = _run(_cropper(p), _batch(fmt, matrix, full, src), boxes, np.asarray([0, -5], dtype=np.int32))       # nothing kept at all
    assert none[2].tolist() == [0, 0, 0, 0] and (none[1][:, 0] == -1).all() and (none[1][:, 1:] == 0).all() and (none[0].view(np.uint8) == 255).all()


# ---------------------------------------------------------------------------------------------------------------- 3. numbering across waves and streams
def test_numbering_crosses_waves_and_streams_with_select():
    fmt, matrix, full = "nv12", "bt601", False
    sizes, seeds = rr.SIZES + [rr.SIZES[0]], (2, 3, 4)
    src = _sources(fmt, matrix, full, sizes, seeds)
    p = cr.params((4, 4), capacity=2048)
    boxes, counts, select = cr.random_boxes(11, sizes, 512)
    want = cr.step([rgb for _, rgb in src], boxes, counts, sizes, select, p)
    per_stream = [int((want[1][:want[2][0], 0] == b).sum()) for b in range(3)]
    assert all(n > 64 for n in per_stream) and want[2][1] == 0, per_stream
    batch = _batch(fmt, matrix, full, src, "w+1")
    _check(_run(_cropper(p, 3), batch, boxes, counts, select), want, "uint8 select")
    cropper = _cropper(p, 3)
    _poison(cropper)
    cropper(batch, _dev(boxes), _dev(counts), _dev(select).bool())
    torch.cuda.synchronize()
    _check(tuple(t.cpu().numpy() for t in (cropper.patches, cropper.index, cropper.totals)), want, "bool select")
    few = cr.params((4, 4), capacity=400)                                    # the table fills inside the second stream
    want = cr.step([rgb for _, rgb in src], boxes, counts, sizes, select, few)
    assert want[2][0] == 400 and want[2][1] == sum(per_stream) - 400 and per_stream[0] < 400 < per_stream[0] + per_stream[1]
    _check(_run(_cropper(few, 3), batch, boxes, counts, select), want, "capacity 400")


# ---------------------------------------------------------------------------------------------------------------- 4. boxes are not trusted
def test_garbage_boxes_cannot_leave_the_frame():
    """Any bit pattern as a box, counts far above d, garbage behind the counts: the rectangle is clamped against the frame record, so the call
    returns cleanly and equals the reference. The frame table is valid throughout."""
    fmt, matrix, full = "nv12", "bt709", True
    src = _sources(fmt, matrix, full)
    rng = np.random.default_rng(5)
    d = 512
    boxes = rng.integers(0, 2 ** 32, (2, d, 4), dtype=np.uint64).astype(np.uint32).view(np.float32)
    special = np.asarray([np.nan, np.inf, -np.inf, 3e38, -3e38, 1e30, -1e30, 0.0, -0.0, 1e-40, 2.0 ** 31, -2.0 ** 31, 2.0 ** 32, 130.5, 96.5, 259.5],
                         dtype=np.float32)
    boxes[0, :256] = special[rng.integers(0, len(special), (256, 4))]
    boxes[1, :128] = rng.uniform(-400, 400, (128, 4)).astype(np.float32)     # sorted or not, inside or not
    counts = np.asarray([2 ** 31 - 1, d + 1], dtype=np.int32)
    for p in (cr.params((4, 4), capacity=2048), cr.params((3, 5), capacity=2048, margin=0.5, square=True, fp16=True)):
        want = cr.step([rgb for _, rgb in src], boxes, counts, rr.SIZES, None, p)
        assert want[2][0] >= 8
        _check(_run(_cropper(p), _batch(fmt, matrix, full, src, "w+1"), boxes, counts), want, "garbage")


def test_two_runs_give_the_same_bits():
    fmt, matrix, full = "bgr24", "bt709", False
    src = _sources(fmt, matrix, full)
    boxes, counts = cr.boxes_array()
    cropper = _cropper(cr.CONFIGS["imagenet-f32"])
    batch = _batch(fmt, matrix, full, src, "256")
    a = _run(cropper, batch, boxes, counts)
    b = _run(cropper, batch, boxes, counts)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    _check(a, _want("rgb", [rgb for _, rgb in src], "imagenet-f32"), "bgr24")


# ---------------------------------------------------------------------------------------------------------------- 5. a captured step follows its inputs
def test_a_captured_step_follows_boxes_and_surfaces():
    fmt, matrix, full = "nv12", "bt709", False
    p = cr.CONFIGS["imagenet-f16"]
    first, second = _sources(fmt, matrix, full), _sources(fmt, matrix, full, seeds=(12, 13))
    boxes, counts = cr.boxes_array()
    other = boxes[:, ::-1].copy()                                            # the same rows in another order ...
    other[:, :, [0, 2]] += np.float32(3.25)                                  # ... moved
    other_counts = np.asarray([cr.D, 9], dtype=np.int32)
    batch = _batch(fmt, matrix, full, first)
    cropper = _cropper(p)
    static_boxes, static_counts = _dev(boxes), _dev(counts)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cropper(batch, static_boxes, static_counts)                          # warm-up outside the capture: allocates the workspace
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = cropper(batch, static_boxes, static_counts)
    for src, bx, cn in ((first, boxes, counts), (second, other, other_counts), (first, other, counts)):
        table = batch.table.data_ptr()
        batch.set([tgr._surface(fmt, planes, "w+1") for planes, _ in src])
        assert batch.table.data_ptr() == table
        static_boxes.copy_(torch.from_numpy(bx))
        static_counts.copy_(torch.from_numpy(cn))
        _poison(cropper)
        graph.replay()
        torch.cuda.synchronize()
        want = cr.step([rgb for _, rgb in src], bx, cn, rr.SIZES, None, p)
        assert want[2][0] >= 8
        _check(tuple(t.cpu().numpy() for t in out), want, "replay")


# ---------------------------------------------------------------------------------------------------------------- 6. behind the tracker
def test_crops_behind_the_tracker():
    m = models.load_synthetic(models.ssd_lite_mobilenet_v2(image_size=160, num_classes=3), 0).to(DEV)
    try:
        fmt, matrix, full = "nv12", "bt709", False
        src = _sources(fmt, matrix, full, seeds=(930, 931))
        batch = _batch(fmt, matrix, full, src, "256")
        # thresholds far below the model's score threshold: every detection starts a track in the first step and is matched in the second
        tracker = ByteTracker(2, DEV, max_tracks=64, track_thresh=0.05, low_thresh=0.01, new_thresh=0.05)
        p = cr.params((16, 8), capacity=128, fp16=True, mean=cr.IMAGENET_MEAN, std=cr.IMAGENET_STD, margin=0.05)
        cropper = _cropper(p)
        m.track_frames(batch, tracker)
        boxes, scores, labels, ids, det, counts, det_ids = m.track_frames(batch, tracker)
        _poison(cropper)
        out = m.crop_objects(batch, cropper, boxes, counts)
        patch_ids = cropper.gather(ids)
        patch_scores = cropper.gather(scores)
        torch.cuda.synchronize()
        hb, hc, hi, hs = boxes.cpu().numpy(), counts.cpu().numpy(), ids.cpu().numpy(), scores.cpu().numpy()
        want = cr.step([rgb for _, rgb in src], hb, hc, rr.SIZES, None, p)
        kept = int(want[2][0])
        assert all(int((want[1][:kept, 0] == b).sum()) >= 1 for b in range(2)), (hc, want[2])
        _check(tuple(t.cpu().numpy() for t in out), want, "behind the tracker")
        assert patch_ids.shape == (p.capacity,) and patch_ids.dtype == ids.dtype
        assert np.array_equal(patch_ids.cpu().numpy()[:kept], hi[want[1][:kept, 0], want[1][:kept, 1]])
        assert np.array_equal(patch_scores.cpu().numpy()[:kept].view(np.int32), hs[want[1][:kept, 0], want[1][:kept, 1]].view(np.int32))
        assert (patch_ids.cpu().numpy()[kept:] == hi[0, 0]).all()           # rows behind kept: row (0, 0)'s value, meaningless
        with pytest.raises(ValueError, match="cropper must be an ObjectCropper"):
            m.crop_objects(batch, tracker, boxes, counts)
    finally:
        m.release()


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def test_every_error_code_of_the_entry_point():
    DN_E_INVALID, DN_E_WORKSPACE, DN_E_UNSUPPORTED = -1, -3, -4
    fmt, matrix, full = "nv12", "bt709", False
    src = _sources(fmt, matrix, full)
    batch = _batch(fmt, matrix, full, src)
    boxes_np, counts_np = cr.boxes_array()
    boxes, counts = _dev(boxes_np), _dev(counts_np)
    cropper = _cropper(cr.CONFIGS["f32-16x8"])
    cropper(batch, boxes, counts)
    torch.cuda.synchronize()
    last = _lib.debug_last_kernel()
    assert last == "crop_gather_kernel<0,0>"
    L = _lib.lib()
    d = cr.D
    need = L.dn_crop_workspace_bytes(2, d)
    assert need > 0 and need == 256 + 2 * d * 32
    for s, dd in ((0, d), (2, 0), (-1, d), (1025, d), (2, 513)):
        assert L.dn_crop_workspace_bytes(s, dd) == 0
    assert L.dn_crop_workspace_bytes(1024, 512) > 0
    ws = cropper._ws[d]
    before = [t.clone() for t in (cropper.patches, cropper.index, cropper.totals)]
    good = dict(frames=batch.table.data_ptr(), format=batch.format_code, color=batch.color_code, boxes=boxes.data_ptr(), counts=counts.data_ptr(),
                select=0, streams=2, d=d, patches=cropper.patches.data_ptr(), index=cropper.index.data_ptr(), totals=cropper.totals.data_ptr(),
                ws=ws.data_ptr(), ws_bytes=ws.numel())

    def call(params=None, null_params=False, **kw):
        a = dict(good, **kw)
        rec = _lib.CropParams.from_buffer_copy(cropper.params)
        for k, v in (params or {}).items():
            if isinstance(v, tuple):
                k, i = k.split(":")
                getattr(rec, k)[int(i)] = v[0]
            else:
                setattr(rec, k, v)
        p = lambda v: C.c_void_p(v) if v else None      # noqa: E731
        return L.dn_crop_objects(p(a["frames"]), a["format"], a["color"], p(a["boxes"]), p(a["counts"]), p(a["select"]), a["streams"], a["d"],
                                 None if null_params else C.byref(rec), p(a["patches"]), p(a["index"]), p(a["totals"]), p(a["ws"]), a["ws_bytes"],
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))

    nan, inf = float("nan"), float("inf")
    for name in ("frames", "boxes", "counts", "patches", "index", "totals", "ws"):
        assert call(**{name: 0}) == DN_E_INVALID, name
    assert call(null_params=True) == DN_E_INVALID
    for kw in (dict(streams=0), dict(streams=-2), dict(d=0), dict(d=-1)):
        assert call(**kw) == DN_E_INVALID, kw
    for params in (dict(out_h=0), dict(out_w=-1), dict(capacity=0), dict(margin=nan), dict(margin=-0.5), dict(margin=inf), {"std:1": (0.0,)},
                   {"std:2": (-1.0,)}, {"std:0": (inf,)}, {"std:0": (nan,)}, {"mean:2": (inf,)}, {"mean:0": (nan,)}, dict(square=2), dict(square=-1),
                   dict(out_fp16=2), dict(min_width=0), dict(min_height=0), {"reserved:0": (1,)}, {"reserved:1": (-1,)}):
        assert call(params) == DN_E_INVALID, params
    for kw in (dict(boxes=good["boxes"] + 4), dict(patches=good["patches"] + 8), dict(index=good["index"] + 4), dict(totals=good["totals"] + 4),
               dict(ws=good["ws"] + 4), dict(counts=good["counts"] + 2)):
        assert call(**kw) == DN_E_INVALID, kw
        assert b"aligned" in L.dn_last_error()
    for f, c in ((4, 1), (-1, 0), (0, 2), (0, 0x21), (1, -1), (0, 0x100)):
        assert call(format=f, color=c) == DN_E_UNSUPPORTED, (f, c)
        assert b"unknown format" in L.dn_last_error()
    for kw in (dict(streams=1025), dict(d=513)):
        assert call(**kw) == DN_E_UNSUPPORTED, kw
    for params in (dict(capacity=8193), dict(out_h=1025), dict(out_w=1025)):
        assert call(params) == DN_E_UNSUPPORTED, params
    assert call(ws_bytes=need - 1) == DN_E_WORKSPACE
    assert call(ws_bytes=0) == DN_E_WORKSPACE
    assert _lib.debug_last_kernel() == last          # a refused call launches nothing
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, (cropper.patches, cropper.index, cropper.totals)))
    every = _dev(np.ones((2, d), dtype=np.uint8))
    assert call() == 0 and call(ws_bytes=need) == 0 and call(select=every.data_ptr()) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="names no frames yet"):
        cropper(FrameBatch(2, DEV), boxes, counts)
    with pytest.raises(ValueError, match="contiguous torch.float32"):
        cropper(batch, boxes.cpu(), counts)
