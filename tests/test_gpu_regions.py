"""Regions of video surfaces as input on the device (dn_forward_regions, SSD.forward_regions, sliced.FrameSlicer, SSD.detect_sliced_frames,
detect_tta_frames, track_sliced_frames): the network input of a region is, bit for bit, that of forward_uint8 on the rectangle cut out of the
frame converted by tests/frames_ref.py (tests/regions_ref.py: crop, optional mirror), and the sliced / TTA / tracking results equal those of the
float-image entry points. Noise frames, ssd_lite_mobilenet_v2 at network size 160 as in tests/test_gpu_frames.py; tests/test_regions.py shows
that the region set used here tells three wrong samplers from the right one. Every record the device sees has passed the host validation."""
import ctypes as C

import numpy as np
import pytest
import torch

import frames_ref as fr
import regions_ref as rr
from demonet_amd import _lib, models
from demonet_amd.frames import FrameBatch, RegionTable
from demonet_amd.sliced import FrameSlicer
from demonet_amd.track import ByteTracker

pytestmark = pytest.mark.gpu

SIZE = 160
DEV = "cuda:0"
YUV = [(f, m, full) for f in ("nv12", "i420") for m, full in fr.VARIANTS]
FORMATS = YUV + [("rgb24", "bt709", False), ("bgr24", "bt709", False)]
IDS = ["{}-{}-{}".format(f, m, "full" if full else "limited") for f, m, full in YUV] + ["rgb24", "bgr24"]


@pytest.fixture(scope="module")
def v2_160():
    m = models.load_synthetic(models.ssd_lite_mobilenet_v2(image_size=SIZE, num_classes=3), 0).to(DEV)
    yield m
    m.release()


# ---------------------------------------------------------------------------------------------------------------- frames (as in test_gpu_frames.py)
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_SRC = {}


def _source(fmt, matrix, full, seed, h, w):
    """(payload planes [rows, bytes] uint8 of a noise frame, the [h, w, 3] RGB frame frames_ref makes of it); computed once"""
    key = (fmt, matrix, full, seed, h, w)
    if key not in _SRC:
        if fmt in ("nv12", "i420"):
            Y, U, V = fr.noise_yuv(seed, h, w)
            planes = [Y, fr.interleave(U, V)] if fmt == "nv12" else [Y, U, V]
            rgb = fr.planes_to_rgb(Y, U, V, matrix, full)
        else:
            rgb = fr.noise_rgb(seed, h, w)
            planes = [(rgb if fmt == "rgb24" else rgb[..., ::-1]).reshape(h, 3 * w)]
        _SRC[key] = (planes, np.ascontiguousarray(rgb))
    return _SRC[key]


PITCH = {"w": lambda p: p, "w+1": lambda p: p + 1, "256": lambda p: (p + 255) // 256 * 256}


def _surface(fmt, planes, pitch="w", gap=0):
    """the frame on the device in a form FrameBatch.set takes: every plane an allocation of its own, rows `pitch` apart, the gap bytes = gap"""
    views = []
    for p in planes:
        payload = p.shape[1]
        views.append(_dev(fr.pitched(p, PITCH[pitch](payload), gap))[:, :payload])
    if fmt in ("rgb24", "bgr24"):
        return views[0].unflatten(1, (-1, 3))
    return tuple(views)


def _net_input_fn():
    fn = _lib.lib().dn_debug_network_input
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    return fn


def _network_input(m, n, h, w, run):
    """fill the resized and the ratio block of the model's (n, h, w) workspace with 0xFF, run(), return (block [n, 3, H, W] fp32 copy, ratios [n, 2])"""
    dev = torch.device(DEV)
    handle = m._plan(dev)
    ws = m._buffers_for(n, h, w, dev)["ws"]
    base = ws.data_ptr()
    pr, ps = C.c_void_p(), C.c_void_p()
    _lib.check(_net_input_fn()(C.c_void_p(handle), C.c_void_p(base), n, C.byref(pr), C.byref(ps)), "dn_debug_network_input")
    W, H = m.graph.size
    ro, rbytes, so, sbytes = pr.value - base, n * 3 * H * W * 4, ps.value - base, n * 8
    assert 0 <= ro and ro + rbytes <= ws.numel() and 0 <= so and so + sbytes <= ws.numel()
    ws[ro:ro + rbytes].fill_(255)
    ws[so:so + sbytes].fill_(255)
    torch.cuda.synchronize()
    out = run()
    torch.cuda.synchronize()
    assert m._buffers_for(n, h, w, dev)["ws"].data_ptr() == base
    return ws[ro:ro + rbytes].view(torch.float32).view(n, 3, H, W).clone(), ws[so:so + sbytes].view(torch.float32).view(n, 2).cpu().numpy(), out


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _same_detections(got, want, what=""):
    assert torch.equal(got[3], want[3]), what + " counts"
    assert torch.equal(got[2], want[2]), what + " labels"
    assert _same_bits(got[1], want[1]), what + " scores"
    assert _same_bits(got[0], want[0]), what + " boxes"


def _same_lists(got, want, what=""):
    assert len(got) == len(want)
    for g, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a["labels"], b["labels"]), "{} image {} labels".format(what, g)
        assert _same_bits(a["scores"], b["scores"]), "{} image {} scores".format(what, g)
        assert _same_bits(a["boxes"], b["boxes"]), "{} image {} boxes".format(what, g)


def _float_image(rgb):
    """[3, H, W] fp32 on the device, divided on the HOST (true division: torch's GPU kernel multiplies by 1 / 255, which differs in the last ulp)"""
    return _dev(rgb.transpose(2, 0, 1).astype(np.float32) / np.float32(255))


# ---------------------------------------------------------------------------------------------------------------- 1. the network input
_WANT = {}


def _reference_rows(m, key, rgbs, regions):
    """per region: (the resized block [1, 3, H, W], the ratio [1, 2]) of forward_uint8 on the reference crop, n = 1; computed once per conversion
    (NV12 and I420 share their converted frames), in eager mode: every crop size is a signature of its own"""
    if key not in _WANT:
        rows = []
        m.set_graph_mode(False)
        try:
            for reg in regions:
                c = rr.crop(rgbs[reg[0]], reg)
                d = _dev(c[None])
                block, ratio, _ = _network_input(m, 1, c.shape[0], c.shape[1], lambda: m.forward_uint8(d))
                rows.append((block, ratio))
        finally:
            m.set_graph_mode(True)
        _WANT[key] = rows
    return _WANT[key]


@pytest.mark.parametrize("fmt,matrix,full", FORMATS, ids=IDS)
def test_network_input_equals_forward_uint8_of_the_crop(fmt, matrix, full, v2_160):
    m = v2_160
    regions, n = rr.REGIONS, len(rr.REGIONS)
    src = [_source(fmt, matrix, full, 900 + f, h, w) for f, (h, w) in enumerate(rr.SIZES)]
    yuv = fmt in ("nv12", "i420")
    want = _reference_rows(m, (matrix, full) if yuv else "rgb", [rgb for _, rgb in src], regions)
    batch, table = FrameBatch(2, DEV, fmt, matrix, full), RegionTable(n, DEV)
    blocks = []
    for gap, pitches in ((0, ("w", "w+1")), (0xA5, ("256", "w+1"))):      # the bytes between a row's payload and the next row must not matter
        batch.set([_surface(fmt, planes, pitch, gap) for (planes, _), pitch in zip(src, pitches)])
        assert batch.sizes == rr.SIZES
        table.set(regions, batch.sizes)
        got, ratios, _ = _network_input(m, n, 0, 0, lambda: [t.clone() for t in m.forward_regions(batch, table)])
        assert int((got.view(torch.int32) == -1).sum()) == 0, "elements of the resized block not written"
        assert int((torch.from_numpy(ratios.view(np.int32)) == -1).sum()) == 0, "elements of the ratio block not written"
        for i, (reg, (block, ratio)) in enumerate(zip(regions, want)):
            assert int((block.view(torch.int32) == -1).sum()) == 0
            diff = int((got[i:i + 1].view(torch.int32) != block.view(torch.int32)).sum())
            assert diff == 0, "region {} {} gap {:#x}: {} of {} elements differ".format(i, reg, gap, diff, block.numel())
            if reg[3:5] != (SIZE, SIZE):          # (forward_uint8 at the network size writes no ratio: its boxes are not mapped back)
                assert np.array_equal(ratios[i:i + 1].view(np.int32), ratio.view(np.int32)), (reg, ratios[i], ratio)
            w_h = np.array([np.float32(reg[3]) / np.float32(SIZE), np.float32(reg[4]) / np.float32(SIZE)], dtype=np.float32)
            assert np.array_equal(ratios[i].view(np.int32), w_h.view(np.int32)), (reg, ratios[i])
        blocks.append(got)
    assert _same_bits(blocks[0], blocks[1])
    assert not _same_bits(blocks[0][0], blocks[0][1])                     # a region and its mirrored twin


# ---------------------------------------------------------------------------------------------------------------- 2. whole frames
def test_whole_frame_regions_reproduce_forward_frames(v2_160):
    m = v2_160
    fmt, matrix, full = "nv12", "bt601", False
    sizes = [(200, 260), (97, 131), (SIZE, SIZE)]
    src = [_source(fmt, matrix, full, 910 + i, h, w) for i, (h, w) in enumerate(sizes)]
    batch = FrameBatch(3, DEV, fmt, matrix, full).set([_surface(fmt, planes, "w+1") for planes, _ in src])
    table = RegionTable(3, DEV).set([(i, 0, 0, w, h, 0) for i, (h, w) in enumerate(sizes)], batch.sizes)
    want_block, want_ratios, want = _network_input(m, 3, 0, 0, lambda: [t.clone() for t in m.forward_frames(batch)])
    got_block, got_ratios, got = _network_input(m, 3, 0, 0, lambda: [t.clone() for t in m.forward_regions(batch, table)])
    assert int((got_block.view(torch.int32) == -1).sum()) == 0
    assert _same_bits(got_block, want_block)
    assert np.array_equal(got_ratios.view(np.int32), want_ratios.view(np.int32))
    assert int(want[3].sum()) > 0
    _same_detections(got, want)


# ---------------------------------------------------------------------------------------------------------------- 3. two chains
def test_detections_equal_forward_uint8_over_two_chains(v2_160):
    """the smallest n the plan splits into sub-batch chains: every chain starts at its own REGION record and indexes the SAME frame table -- the
    first chain's regions name the last frame, all later ones frame 0, so a frame table advanced per chain would read other frames"""
    m = v2_160
    m._plan(torch.device(DEV))
    n = next(k for k in range(2, 257) if m.batch_split(k) > 1)
    S = m.batch_split(n)
    first = n // S + (1 if n % S else 0)
    fmt, matrix, full = "i420", "bt709", False
    sizes = [(96, 128), (97, 131), (120, 200)]
    src = [_source(fmt, matrix, full, 920 + i, h, w) for i, (h, w) in enumerate(sizes)]
    w, h = 64, 48
    regions = []
    for i in range(n):
        f = 2 if i < first else 0
        H, W = sizes[f]
        regions.append((f, (7 * i + 1) % (W - w + 1), (5 * i + 3) % (H - h + 1), w, h, i % 3 == 1))
    batch = FrameBatch(3, DEV, fmt, matrix, full).set([_surface(fmt, planes, "w+1") for planes, _ in src])
    table = RegionTable(n, DEV).set(regions, batch.sizes)
    got = [t.clone() for t in m.forward_regions(batch, table)]
    want = [t.clone() for t in m.forward_uint8(_dev(np.stack([rr.crop(src[reg[0]][1], reg) for reg in regions])))]
    assert int(want[3].sum()) > 0
    _same_detections(got, want, "n={} as {} chains".format(n, S))


# ---------------------------------------------------------------------------------------------------------------- 4. sliced inference
SLICED_SIZES = [(200, 260), (97, 131)]


def _sliced_inputs(fmt="nv12", matrix="bt709", full=False, seed=930):
    src = [_source(fmt, matrix, full, seed + i, h, w) for i, (h, w) in enumerate(SLICED_SIZES)]
    batch = FrameBatch(2, DEV, fmt, matrix, full).set([_surface(fmt, planes, "256") for planes, _ in src])
    return batch, [_float_image(rgb) for _, rgb in src]


@pytest.mark.parametrize("tile,full_image", [(None, True), (None, False), ((120, 140), True)], ids=["default-tile", "tiles-only", "resized-tiles"])
def test_detect_sliced_frames_equals_detect_sliced(tile, full_image, v2_160):
    m = v2_160
    batch, images = _sliced_inputs()
    kw = dict(tile=tile, full_image=full_image, max_tiles_per_forward=3)      # 3: forwards span the two frames
    want = m.detect_sliced(images, **kw)
    got = m.detect_sliced_frames(batch, **kw)
    assert sum(len(d["scores"]) for d in want) > 0
    _same_lists(got, want, "detect_sliced_frames")
    assert m.detect_sliced_frames(batch, **kw) is not None and len(m._frame_slicers) >= 1      # (the cached slicer serves the second call)
    slicer = FrameSlicer(m, batch.sizes, **kw)
    assert slicer.S > 3
    boxes, scores, labels, counts = slicer(batch)
    assert boxes.shape == (2, m.detections_per_img, 4) and counts.dtype == torch.int32
    cnt = counts.tolist()
    assert cnt == [len(d["scores"]) for d in want]
    _same_lists([{"boxes": boxes[g, :c], "scores": scores[g, :c], "labels": labels[g, :c]} for g, c in enumerate(cnt)], want, "FrameSlicer")


# ---------------------------------------------------------------------------------------------------------------- 5. flip TTA
@pytest.mark.parametrize("fuse", ["wbf", "nms"])
def test_detect_tta_frames_equals_detect_tta(fuse, v2_160):
    m = v2_160
    batch, images = _sliced_inputs("i420", "bt601", True, 940)
    want = m.detect_tta(images, fuse=fuse)
    got = m.detect_tta_frames(batch, fuse=fuse)
    assert sum(len(d["scores"]) for d in want) > 0
    _same_lists(got, want, "detect_tta_frames " + fuse)


# ---------------------------------------------------------------------------------------------------------------- 6. the graph follows both tables
def test_the_graph_follows_both_tables(v2_160):
    m = v2_160
    fmt, matrix, full = "nv12", "bt709", True
    rounds = [([(96, 128), (200, 120)], [(0, 3, 5, 91, 67, 0), (1, 0, 0, 120, 200, 1), (1, 11, 20, 100, 160, 0)]),
              ([(240, 320), (97, 131)], [(1, 1, 1, 130, 96, 1), (0, 80, 40, 160, 160, 0), (0, 0, 0, 320, 240, 0)]),
              ([(SIZE, SIZE), (64, 48)], [(0, 0, 0, 160, 160, 1), (1, 5, 7, 40, 50, 0), (0, 10, 20, 33, 35, 1)])]
    sets = [[_surface(fmt, _source(fmt, matrix, full, 950 + 2 * r + i, h, w)[0], "w+1") for i, (h, w) in enumerate(sizes)] for r, (sizes, _) in enumerate(rounds)]
    batch, table = FrameBatch(2, DEV, fmt, matrix, full), RegionTable(3, DEV)
    addresses = None
    replayed = []
    for s, (_, regions) in zip(sets, rounds):
        batch.set(s)
        table.set(regions, batch.sizes)
        assert addresses in (None, (batch.table.data_ptr(), table.table.data_ptr()))
        addresses = (batch.table.data_ptr(), table.table.data_ptr())
        replayed.append([t.clone() for t in m.forward_regions(batch, table)])
    try:
        m.set_graph_mode(False)
        for r, (s, (_, regions)) in enumerate(zip(sets, rounds)):
            fresh = FrameBatch(2, DEV, fmt, matrix, full).set(s)
            _same_detections(replayed[r], [t.clone() for t in m.forward_regions(fresh, RegionTable(3, DEV).set(regions, fresh.sizes))], "round {}".format(r))
    finally:
        m.set_graph_mode(True)
    assert sum(int(x[3].sum()) for x in replayed) > 0
    assert not _same_bits(replayed[0][0], replayed[1][0])


# ---------------------------------------------------------------------------------------------------------------- 7. tracking
def test_track_sliced_frames_equals_update_on_detect_sliced(v2_160):
    m = v2_160
    fmt, matrix, full = "nv12", "bt709", False
    D = m.detections_per_img
    a, b = ByteTracker(2, DEV), ByteTracker(2, DEV)
    batch = FrameBatch(2, DEV, fmt, matrix, full)
    slicer = FrameSlicer(m, SLICED_SIZES, max_tiles_per_forward=3)
    rows = 0
    for step in range(3):
        src = [_source(fmt, matrix, full, 960 + 2 * step + i, h, w) for i, (h, w) in enumerate(SLICED_SIZES)]
        got = [t.clone() for t in m.track_sliced_frames(batch.set([_surface(fmt, planes) for planes, _ in src]), a, slicer)]
        dets = m.detect_sliced([_float_image(rgb) for _, rgb in src], max_tiles_per_forward=3)
        pb, ps = torch.zeros((2, D, 4), device=DEV), torch.zeros((2, D), device=DEV)
        pl, pc = torch.zeros((2, D), dtype=torch.int64, device=DEV), torch.zeros((2,), dtype=torch.int32, device=DEV)
        for g, d in enumerate(dets):
            c = len(d["scores"])
            pb[g, :c], ps[g, :c], pl[g, :c], pc[g] = d["boxes"], d["scores"], d["labels"], c
        want = b.update(pb, ps, pl, pc)
        for x, y in zip(got, want):
            assert x.dtype == y.dtype and torch.equal(_bits(x), _bits(y)), step
        rows += int(got[5].sum())
    assert torch.equal(a.state, b.state)
    assert rows > 0


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_the_library_refuses_null_tables_unknown_codes_and_empty_calls(v2_160):
    m = v2_160
    dev = torch.device(DEV)
    handle = m._plan(dev)
    n = 2
    planes, _ = _source("nv12", "bt709", False, 970, 48, 64)
    batch = FrameBatch(1, DEV).set([_surface("nv12", planes)])
    table = RegionTable(n, DEV).set([(0, 0, 0, 64, 48, 0), (0, 3, 5, 30, 20, 1)], batch.sizes)
    assert int(m.forward_regions(batch, table)[3].numel()) == n
    torch.cuda.synchronize()
    b = m._buffers_for(n, 0, 0, dev)
    before = [t.clone() for t in b["outs"]]
    last = _lib.debug_last_kernel()
    p = C.c_void_p
    L = _lib.lib()

    def call(frames, regions, n_, fmt, color):
        return L.dn_forward_regions(p(handle), p(frames) if frames else None, p(regions) if regions else None, n_, fmt, color,
                                    *(p(t.data_ptr()) for t in b["outs"]), p(b["ws"].data_ptr()), b["ws"].numel(), p(torch.cuda.current_stream(dev).cuda_stream))
    DN_E_INVALID, DN_E_UNSUPPORTED = -1, -4
    fp, rp = batch.table.data_ptr(), table.table.data_ptr()
    for fmt, color in ((4, 1), (-1, 0), (0, 2), (0, 0x21), (1, -1), (0, 0x100)):
        assert call(fp, rp, n, fmt, color) == DN_E_UNSUPPORTED, (fmt, color)
        assert b"unknown format" in L.dn_last_error()
    assert call(0, rp, n, 0, 1) == DN_E_INVALID
    assert call(fp, 0, n, 0, 1) == DN_E_INVALID
    assert call(fp, rp, 0, 0, 1) == DN_E_INVALID
    assert call(fp, rp, -3, 0, 1) == DN_E_INVALID
    assert _lib.debug_last_kernel() == last          # a refused call launches nothing
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, b["outs"]))


def test_forward_regions_refuses_stale_sizes_other_devices_and_unset_tables(v2_160):
    m = v2_160
    fmt, matrix, full = "nv12", "bt709", False
    big, small = _source(fmt, matrix, full, 980, 120, 200), _source(fmt, matrix, full, 981, 96, 128)
    batch = FrameBatch(2, DEV).set([_surface(fmt, big[0]), _surface(fmt, big[0])])
    table = RegionTable(2, DEV).set([(0, 0, 0, 200, 120, 0), (1, 100, 60, 100, 60, 1)], batch.sizes)
    m.forward_regions(batch, table)
    last = _lib.debug_last_kernel()
    batch.set([_surface(fmt, big[0]), _surface(fmt, small[0])])            # frame 1 is now smaller than its region's rectangle
    with pytest.raises(ValueError, match=r"stale sizes: the regions of frame 1 were validated against \(120, 200\)"):
        m.forward_regions(batch, table)
    with pytest.raises(ValueError, match=r"region 1: the rectangle"):
        table.set(table.regions, batch.sizes)
    table.set([(0, 0, 0, 200, 120, 0), (1, 28, 36, 100, 60, 1)], batch.sizes)      # validated again: accepted
    m.forward_regions(batch, table)
    last = _lib.debug_last_kernel()
    with pytest.raises(ValueError, match="RegionTable names no regions yet"):
        m.forward_regions(batch, RegionTable(2, DEV))
    with pytest.raises(ValueError, match="FrameBatch names no frames yet"):
        m.forward_regions(FrameBatch(2, DEV), table)
    with pytest.raises(ValueError, match="is on cpu"):
        m.forward_regions(batch, RegionTable(2, "cpu"))
    with pytest.raises(ValueError, match="stale sizes"):
        FrameSlicer(m, [(120, 200), (120, 200)])(batch)
    with pytest.raises(ValueError, match="expected a RegionTable"):
        m.forward_regions(batch, [(0, 0, 0, 4, 4)])
    assert _lib.debug_last_kernel() == last
