"""The input resize (csrc/dense.hip resize_kernel, u8hwc_kernel) against a float64 reference with a derived bound (tests/resize_ref.py).

CPU tests pin the reference and the bound: the restatement equals F.interpolate in float64, two fp32 evaluations stay inside the bound, and
six classic mistakes leave it. GPU tests read what the forwards wrote -- the network-size image and the box ratios -- through
dn_debug_network_input, from a block filled with 0xFF first, on rough images (i.i.d. noise: a smooth image hides a half-pixel shift)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize_ref as rr
from demonet_amd import _lib, models

V2_SIZE = 160
CASES = rr.CASES
IDS = [c[0] for c in CASES]
_REF = {}


def _float_case(case, size):
    """(images [n, 3, h, w] float32, bilinear_ref, E) of a case at a network size; computed once"""
    key = ("f", case[0], size)
    if key not in _REF:
        name, h, w, n = case
        img = rr.noise(1000 + CASES.index(case), n, h, w)
        _REF[key] = (img, rr.bilinear_ref(img, size, size), rr.bound(img, size, size))
    return _REF[key]


def _u8_case(case, size):
    """(images [n, h, w, 3] uint8, bilinear_ref of u8 / 255, E)"""
    key = ("u", case[0], size)
    if key not in _REF:
        name, h, w, n = case
        u8 = rr.noise_u8(2000 + CASES.index(case), n, h, w)
        img = u8.transpose(0, 3, 1, 2).astype(np.float64) / 255.0
        _REF[key] = (u8, rr.bilinear_ref(img, size, size), rr.bound(img, size, size))
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------- CPU: reference and bound
def test_bilinear_ref_is_aten_bilinear_in_float64():
    for case in CASES:
        img, ref, _ = _float_case(case, V2_SIZE)
        want = F.interpolate(torch.from_numpy(img).double(), size=(V2_SIZE, V2_SIZE), mode="bilinear", align_corners=False).numpy()
        assert np.abs(ref - want).max() <= 1e-12, case[0]
    img, ref, _ = _float_case(CASES[4], 320)
    want = F.interpolate(torch.from_numpy(img).double(), size=(320, 320), mode="bilinear", align_corners=False).numpy()
    assert np.abs(ref - want).max() <= 1e-12


def test_fp32_evaluations_stay_inside_the_bound():
    """the numpy-float32 emulation of resize_kernel (float images and uint8 / 255) and F.interpolate in float32"""
    worst = {}
    for case in CASES:
        img, ref, e = _float_case(case, V2_SIZE)
        n = img.shape[0]
        emu = rr.emulate_fp32(img.reshape(n * 3, *img.shape[2:]), V2_SIZE, V2_SIZE).reshape(ref.shape)
        aten = F.interpolate(torch.from_numpy(img), size=(V2_SIZE, V2_SIZE), mode="bilinear", align_corners=False).numpy()
        u8, ref8, e8 = _u8_case(case, V2_SIZE)
        planes = u8.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)          # one rounding, as (float)p / 255.f
        emu8 = rr.emulate_fp32(planes.reshape(n * 3, *planes.shape[2:]), V2_SIZE, V2_SIZE).reshape(ref8.shape)
        for what, got, y, bound in (("emulation", emu, ref, e), ("aten fp32", aten, ref, e), ("emulation of the uint8 path", emu8, ref8, e8)):
            assert (bound > 0).all()
            r = float((np.abs(got.astype(np.float64) - y) / bound).max())
            worst[what] = max(worst.get(what, 0.0), r)
            assert r <= 1.0, (case[0], what, r)
    print("\nmax |fp32 - ref| / E:", {k: round(v, 3) for k, v in worst.items()})


# mutant -> the case that must expose it
MUTANTS = [("no half-pixel terms", dict(half_pixel=False), "375x500"),
           ("align_corners=True", dict(align_corners=True), "427x640"),
           ("rh and rw swapped", dict(swap_ratios=True), "2x-640x480"),
           ("x1 not clamped at w - 1", dict(clamp_x1=False), "up-97x131"),
           ("src not clamped at 0", dict(clamp_src=False), "up-97x131"),
           ("nearest", dict(nearest=True), "2x-320x320")]


@pytest.mark.parametrize("what,kw,case_name", MUTANTS, ids=[m[0].replace(" ", "-") for m in MUTANTS])
def test_the_bound_catches_a_wrong_resize(what, kw, case_name):
    case = CASES[IDS.index(case_name)]
    img, ref, e = _float_case(case, V2_SIZE)
    n = img.shape[0]
    got = rr.emulate_fp32(img.reshape(n * 3, *img.shape[2:]), V2_SIZE, V2_SIZE, **kw).reshape(ref.shape)
    over = np.abs(got.astype(np.float64) - ref) > e
    assert over.any(), f"{what}: inside the bound everywhere on {case_name}"
    # ... and far outside: the mistakes are errors of the size of the image's contrast, the bound is a few ulps
    assert float((np.abs(got - ref) / e).max()) > 100.0


# ---------------------------------------------------------------------------------------------------------------- GPU
def _net_input_fn():
    fn = _lib.lib().dn_debug_network_input
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    return fn


class _Block:
    """the resized block and the ratio block of an (n, h, w) forward of a model: fill with 0xFF, run, read"""

    def __init__(self, m, n, h, w):
        dev = torch.device("cuda:0")
        handle = m._plan(dev)
        self.ws = m._buffers_for(n, h, w, dev)["ws"]
        base = self.ws.data_ptr()
        pr, ps = C.c_void_p(), C.c_void_p()
        _lib.check(_net_input_fn()(C.c_void_p(handle), C.c_void_p(base), n, C.byref(pr), C.byref(ps)), "dn_debug_network_input")
        W, H = m.graph.size
        self.shape = (n, 3, H, W)
        self.ro, self.rbytes, self.so, self.sbytes = pr.value - base, n * 3 * H * W * 4, ps.value - base, n * 8
        assert 0 <= self.ro and self.ro + self.rbytes <= self.ws.numel() and 0 <= self.so and self.so + self.sbytes <= self.ws.numel()

    def fill(self):
        self.ws[self.ro:self.ro + self.rbytes].fill_(255)
        self.ws[self.so:self.so + self.sbytes].fill_(255)
        torch.cuda.synchronize()

    def resized(self):
        torch.cuda.synchronize()
        return self.ws[self.ro:self.ro + self.rbytes].view(torch.float32).view(self.shape)

    def scale(self):
        torch.cuda.synchronize()
        return self.ws[self.so:self.so + self.sbytes].view(torch.float32).view(-1, 2).cpu().numpy()


def _check_block(blk, ref, e, h, w, what, scale=True):
    got = blk.resized().cpu().numpy()
    unwritten = int((got.view(np.int32) == -1).sum())
    assert unwritten == 0, f"{what}: {unwritten} of {got.size} elements of the resized block not written"
    r = np.abs(got.astype(np.float64) - ref) / e
    k = np.unravel_index(int(np.argmax(np.where(np.isnan(r), np.inf, r))), r.shape)
    print(f"\n{what}: max |device - ref| / E = {float(r[k]):.3f} at {k}")
    assert not (~(r <= 1.0)).any(), f"{what}: {int((~(r <= 1.0)).sum())} elements over the bound, worst {float(r[k]):.3g} at (image, channel, y, x) {k}: " \
                                    f"device {got[k]!r} ref {ref[k]!r} E {e[k]:.3g}"
    if scale:
        n, _, oh, ow = got.shape
        want = np.tile(np.array([np.float32(w) / np.float32(ow), np.float32(h) / np.float32(oh)], dtype=np.float32), (n, 1))
        sc = blk.scale()
        assert np.array_equal(sc.view(np.int32), want.view(np.int32)), f"{what}: scale_xy {sc[(sc.view(np.int32) != want.view(np.int32)).any(1)][:4]} " \
                                                                       f"at images {np.nonzero((sc.view(np.int32) != want.view(np.int32)).any(1))[0][:8]}, want {want[0]}"


def _v2():
    return models.load_synthetic(models.ssd_lite_mobilenet_v2(image_size=V2_SIZE, num_classes=3), 0).to("cuda:0")


@pytest.fixture(scope="module")
def v2_160():
    m = _v2()
    yield m
    m.release()


def _both_paths(m, case, size):
    name, h, w, n = case
    img, ref, e = _float_case(case, size)
    blk = _Block(m, n, h, w)
    blk.fill()
    m.forward_heads(torch.from_numpy(img).cuda())
    _check_block(blk, ref, e, h, w, f"{name} float")
    u8, ref8, e8 = _u8_case(case, size)
    u8_d = torch.from_numpy(u8).cuda()
    blk.fill()
    m.forward_uint8(u8_d)
    _check_block(blk, ref8, e8, h, w, f"{name} uint8")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_resized_block_and_ratios_are_the_reference(case, v2_160):
    _both_paths(v2_160, case, V2_SIZE)


@pytest.mark.gpu
def test_resized_block_of_the_v3_model():
    m = models.load_synthetic(models.ssdlite320_mobilenet_v3_large(num_classes=21), 0).to("cuda:0")
    _both_paths(m, CASES[IDS.index("375x500")], 320)
    m.release()


@pytest.mark.gpu
def test_uint8_at_the_network_size_is_a_plain_conversion(v2_160):
    """weights exactly (1, 0): the block equals u8 / 255 in float32 bit for bit"""
    n = 2
    u8 = torch.from_numpy(rr.noise_u8(7, n, V2_SIZE, V2_SIZE)).cuda()
    blk = _Block(v2_160, n, V2_SIZE, V2_SIZE)
    blk.fill()
    v2_160.forward_uint8(u8)
    got = blk.resized()
    assert int((got.view(torch.int32) == -1).sum()) == 0
    # the correctly rounded fp32 quotient, computed on the host (a device-side division by a constant may be a multiplication by 1 / 255)
    want = np.ascontiguousarray(u8.cpu().numpy().transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255)
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("n,h,w", [(3, 97, 131), (33, 48, 64)])
def test_boxes_map_back_by_the_fp32_ratio(n, h, w, v2_160):
    """forward_batch on (h, w) images == forward_batch on the device's own resized block (no resize), boxes times the fp32 ratio of
    resize_boxes (transform.py:280-291), bit for bit; 33 images run as two sub-batch chains with their own rows of the ratio block"""
    m = v2_160
    img = torch.from_numpy(rr.noise(31 + n, n, h, w)).cuda()
    blk = _Block(m, n, h, w)
    blk.fill()
    first = [t.clone() for t in m.forward_batch(img)]
    block = blk.resized().clone()
    sc = blk.scale()
    assert int((block.view(torch.int32) == -1).sum()) == 0
    ratio = np.array([np.float32(w) / np.float32(V2_SIZE), np.float32(h) / np.float32(V2_SIZE)], dtype=np.float32)
    assert np.array_equal(sc.view(np.int32), np.tile(ratio, (n, 1)).view(np.int32)), sc
    second = [t.clone() for t in m.forward_batch(block)]
    assert int(first[3].sum()) > 0
    assert torch.equal(first[3], second[3]), "counts"
    assert torch.equal(first[2], second[2]), "labels"
    assert torch.equal(first[1], second[1]), "scores"
    r4 = torch.from_numpy(np.array([ratio[0], ratio[1], ratio[0], ratio[1]], dtype=np.float32)).cuda()
    assert torch.equal(first[0].view(torch.int32), (second[0] * r4).view(torch.int32)), "boxes"
