"""Video frames as input on the device (dn_forward_frames, SSD.forward_frames, ForwardPipeline(frames=...), SSD.track_frames): the network input
and the detections are, bit for bit, those of forward_uint8 on the frames converted by tests/frames_ref.py. Noise frames (a smooth image hides
a half-pixel or chroma-offset slip), ssd_lite_mobilenet_v2 at network size 160 as tests/test_resize.py uses it. Every record the device sees
has passed FrameBatch.set's validation."""
import ctypes as C

import numpy as np
import pytest
import torch

import frames_ref as fr
from demonet_amd import _lib, models
from demonet_amd.frames import FrameBatch
from demonet_amd.pipeline import ForwardPipeline
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


# ---------------------------------------------------------------------------------------------------------------- frames
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


def _surface(fmt, planes, pitch="w", gap=0, flat=False):
    """the frame on the device in a form FrameBatch.set takes: every plane an allocation of its own, rows `pitch` apart, the gap bytes = gap;
    flat: the contiguous [h * 3 / 2, w] form (one allocation)"""
    if flat:
        w = planes[0].shape[1]
        return _dev(np.concatenate([p.reshape(-1) for p in planes]).reshape(-1, w))
    views = []
    for p in planes:
        payload = p.shape[1]
        views.append(_dev(fr.pitched(p, PITCH[pitch](payload), gap))[:, :payload])
    if fmt in ("rgb24", "bgr24"):
        return views[0].unflatten(1, (-1, 3))
    return tuple(views)


# ---------------------------------------------------------------------------------------------------------------- the network input
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


def _frames_input(m, batch):
    return _network_input(m, batch.n, 0, 0, lambda: [t.clone() for t in m.forward_frames(batch)])


def _u8_input(m, rgb):
    """rgb: [n, h, w, 3] uint8 numpy"""
    d = _dev(rgb)
    n, h, w, _ = rgb.shape
    return _network_input(m, n, h, w, lambda: [t.clone() for t in m.forward_uint8(d)])


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ratios(m, sizes):
    W, H = m.graph.size
    return np.array([[np.float32(w) / np.float32(W), np.float32(h) / np.float32(H)] for h, w in sizes], dtype=np.float32)


def _same_detections(got, want, what=""):
    assert torch.equal(got[3], want[3]), what + " counts"
    assert torch.equal(got[2], want[2]), what + " labels"
    assert _same_bits(got[1], want[1]), what + " scores"
    assert _same_bits(got[0], want[0]), what + " boxes"


# (name, h, w, per frame: (pitch rule, flat form))
INPUT_CASES = [("2x-640x480", 480, 640, [("w", True), ("w+1", False), ("256", False)]),
               ("up-97x131", 97, 131, [("w", False), ("w+1", False)]),
               ("network-size", SIZE, SIZE, [("w", True), ("256", False)])]


@pytest.mark.parametrize("fmt,matrix,full", FORMATS, ids=IDS)
def test_network_input_equals_forward_uint8_of_the_converted_frames(fmt, matrix, full, v2_160):
    m = v2_160
    for name, h, w, forms in INPUT_CASES:
        n = len(forms)
        src = [_source(fmt, matrix, full, 100 + i, h, w) for i in range(n)]
        want, _, _ = _u8_input(m, np.stack([rgb for _, rgb in src]))
        assert int((want.view(torch.int32) == -1).sum()) == 0
        batch = FrameBatch(n, DEV, fmt, matrix, full)
        blocks = []
        for gap in (0, 0xA5):      # the bytes between a row's payload and the next row must not matter
            yuv_flat = fmt in ("nv12", "i420")
            batch.set([_surface(fmt, planes, pitch, gap, flat and yuv_flat) for (planes, _), (pitch, flat) in zip(src, forms)])
            assert batch.sizes == [(h, w)] * n
            got, ratios, _ = _frames_input(m, batch)
            assert int((got.view(torch.int32) == -1).sum()) == 0, "{}: elements of the resized block not written".format(name)
            assert _same_bits(got, want), "{} gap {:#x}: {} of {} elements differ".format(name, gap, int((got.view(torch.int32) != want.view(torch.int32)).sum()), got.numel())
            assert np.array_equal(ratios.view(np.int32), _ratios(m, [(h, w)] * n).view(np.int32)), (name, ratios)
            blocks.append(got)
        assert _same_bits(blocks[0], blocks[1])


def _uniform_case(m, fmt, matrix, full, n, h, w, seed):
    src = [_source(fmt, matrix, full, seed + i % 5, h, w) for i in range(n)]       # (five distinct frames: the references are computed once)
    batch = FrameBatch(n, DEV, fmt, matrix, full).set([_surface(fmt, planes, "w+1") for planes, _ in src])
    got = [t.clone() for t in m.forward_frames(batch)]
    want = [t.clone() for t in m.forward_uint8(_dev(np.stack([rgb for _, rgb in src])))]
    assert int(want[3].sum()) > 0
    _same_detections(got, want, "n={}".format(n))
    # no float staging image: the (n, 0, 0) buffers of the call hold an empty one, and no other buffers were made for it
    assert m._buffers_for(n, 0, 0, torch.device(DEV))["images"].numel() == 0


def test_detections_equal_forward_uint8_n3(v2_160):
    _uniform_case(v2_160, "nv12", "bt709", False, 3, 120, 200, 300)


def test_detections_equal_forward_uint8_over_two_chains(v2_160):
    """the smallest n the plan splits into sub-batch chains: chain 1 starts at its own record of the table (Call::chain)"""
    m = v2_160
    m._plan(torch.device(DEV))
    n = next(k for k in range(2, 257) if m.batch_split(k) > 1)
    _uniform_case(m, "i420", "bt601", False, n, 48, 64, 310)


def test_detections_equal_forward_uint8_v3_320():
    m = models.load_synthetic(models.ssdlite320_mobilenet_v3_large(num_classes=21), 0).to(DEV)
    try:
        _uniform_case(m, "nv12", "bt601", True, 4, 180, 250, 320)
    finally:
        m.release()


MIXED = [(480, 640), (97, 131), (SIZE, SIZE), (120, 200)]


def test_mixed_sizes_in_one_batch(v2_160):
    m = v2_160
    fmt, matrix, full = "nv12", "bt709", False
    src = [_source(fmt, matrix, full, 400 + i, h, w) for i, (h, w) in enumerate(MIXED)]
    n = len(MIXED)
    batch = FrameBatch(n, DEV, fmt, matrix, full).set([_surface(fmt, planes, "256" if i % 2 else "w") for i, (planes, _) in enumerate(src)])
    block, ratios, first = _frames_input(m, batch)
    for i, (_, rgb) in enumerate(src):
        want, _, _ = _u8_input(m, rgb[None])
        assert _same_bits(block[i:i + 1], want), "frame {}".format(i)
    want_ratios = _ratios(m, MIXED)
    assert np.array_equal(ratios.view(np.int32), want_ratios.view(np.int32)), ratios
    second = [t.clone() for t in m.forward_batch(block)]
    assert int(first[3].sum()) > 0
    assert torch.equal(first[3], second[3]) and torch.equal(first[2], second[2]) and _same_bits(first[1], second[1])
    r4 = torch.from_numpy(want_ratios[:, [0, 1, 0, 1]]).to(DEV)[:, None, :]
    assert _same_bits(first[0], second[0] * r4), "boxes"


def test_the_graph_follows_the_table(v2_160):
    """three forwards on one FrameBatch, set() naming other surfaces (of other sizes) each time: replays of the graph captured on the first equal
    the eager forward of the same surfaces"""
    m = v2_160
    fmt, matrix, full = "i420", "bt709", True
    rounds = [[(96, 128), (200, 120)], [(240, 320), (97, 131)], [(SIZE, SIZE), (64, 48)]]
    sets = [[_surface(fmt, _source(fmt, matrix, full, 500 + 2 * r + i, h, w)[0], "w+1") for i, (h, w) in enumerate(sizes)] for r, sizes in enumerate(rounds)]
    batch = FrameBatch(2, DEV, fmt, matrix, full)
    table = None
    replayed = []
    for s in sets:
        batch.set(s)
        assert table in (None, batch.table.data_ptr())
        table = batch.table.data_ptr()
        replayed.append([t.clone() for t in m.forward_frames(batch)])
    try:
        m.set_graph_mode(False)
        for r, s in enumerate(sets):
            batch.set(s)
            _same_detections(replayed[r], [t.clone() for t in m.forward_frames(batch)], "round {}".format(r))
    finally:
        m.set_graph_mode(True)
    assert sum(int(x[3].sum()) for x in replayed) > 0
    assert not _same_bits(replayed[0][0], replayed[1][0])


def test_pipeline_of_frame_batches(v2_160):
    m = v2_160
    fmt, matrix, full = "nv12", "bt601", False
    sizes = [(96, 128), (120, 200)]
    sets = [[_surface(fmt, _source(fmt, matrix, full, 600 + 2 * t + i, h, w)[0], "256") for i, (h, w) in enumerate(sizes)] for t in range(5)]
    batch = FrameBatch(2, DEV, fmt, matrix, full)       # ONE batch, set again right behind every submit: the slot has its own copy of the records
    got = {}
    with ForwardPipeline(m, batch=2, depth=2, device=DEV, frames=(fmt, matrix, full)) as pipe:
        with pytest.raises(ValueError):
            pipe.submit(FrameBatch(3, DEV, fmt, matrix, full).set(sets[0] + sets[1][:1]))
        with pytest.raises(ValueError):
            pipe.submit(FrameBatch(2, DEV, "i420", matrix, full))
        with pytest.raises(ValueError):
            pipe.submit(torch.zeros((2, 3, SIZE, SIZE), device=DEV))
        for t, s in enumerate(sets):
            assert pipe.submit(batch.set(s)) == t
            if t >= 1:
                got[t - 1] = [x.clone() for x in pipe.result(t - 1)]
        got[4] = [x.clone() for x in pipe.result(4)]
    for t, s in enumerate(sets):
        _same_detections(got[t], m.forward_frames(batch.set(s)), "ticket {}".format(t))
    assert sum(int(x[3].sum()) for x in got.values()) > 0


def test_track_frames_equals_track_on_the_float_images(v2_160):
    m = v2_160
    fmt, matrix, full = "i420", "bt601", True
    h, w = 120, 200
    a, b = ByteTracker(2, DEV), ByteTracker(2, DEV)
    batch = FrameBatch(2, DEV, fmt, matrix, full)
    rows = 0
    for step in range(4):
        src = [_source(fmt, matrix, full, 700 + 2 * step + i, h, w) for i in range(2)]
        got = [t.clone() for t in m.track_frames(batch.set([_surface(fmt, planes) for planes, _ in src]), a)]
        # what forward_uint8 would have seen; divided on the host (true division: torch's GPU kernel multiplies by 1 / 255, which differs in the last ulp)
        images = _dev(np.stack([rgb for _, rgb in src]).transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255))
        want = m.track(images, b)
        for x, y in zip(got, want):
            assert x.dtype == y.dtype and torch.equal(_bits(x), _bits(y)), step
        rows += int(got[5].sum())
    assert torch.equal(a.state, b.state)
    assert rows > 0


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_the_library_refuses_unknown_codes_and_empty_calls(v2_160):
    m = v2_160
    dev = torch.device(DEV)
    handle = m._plan(dev)
    n = 2
    planes, _ = _source("nv12", "bt709", False, 800, 48, 64)
    batch = FrameBatch(n, DEV).set([_surface("nv12", planes), _surface("nv12", planes)])
    b = m._buffers_for(n, 0, 0, dev)
    before = [t.clone() for t in b["outs"]]
    p = C.c_void_p
    L = _lib.lib()

    def call(table, n_, fmt, color):
        return L.dn_forward_frames(p(handle), p(table) if table else None, n_, fmt, color, *(p(t.data_ptr()) for t in b["outs"]), p(b["ws"].data_ptr()), b["ws"].numel(),
                                   p(torch.cuda.current_stream(dev).cuda_stream))
    DN_E_INVALID, DN_E_UNSUPPORTED = -1, -4
    tp = batch.table.data_ptr()
    for fmt, color in ((4, 1), (-1, 0), (0, 2), (0, 0x21), (1, -1), (0, 0x100)):
        assert call(tp, n, fmt, color) == DN_E_UNSUPPORTED, (fmt, color)
        assert b"unknown format" in L.dn_last_error()
    assert call(0, n, 0, 1) == DN_E_INVALID
    assert call(tp, 0, 0, 1) == DN_E_INVALID
    assert call(tp, -3, 0, 1) == DN_E_INVALID
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, b["outs"]))       # a refused call launches nothing


def test_forward_frames_refuses_other_batches(v2_160):
    m = v2_160
    with pytest.raises(ValueError, match="is on cpu"):
        m.forward_frames(FrameBatch(2, "cpu"))
    with pytest.raises(ValueError, match="set"):
        m.forward_frames(FrameBatch(2, DEV))
    with pytest.raises(ValueError, match="FrameBatch"):
        m.forward_frames(torch.zeros((2, 6, 4), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match=r"frame 1, plane UV.*is on cpu"):
        FrameBatch(2, DEV).set([torch.zeros((6, 4), dtype=torch.uint8, device=DEV), (torch.zeros((4, 4), dtype=torch.uint8, device=DEV), torch.zeros((2, 4), dtype=torch.uint8))])
