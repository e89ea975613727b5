"""DN_PW_DW_LDS (pwdirect.hip pw_dw_direct_lds_kernel): the first inverted-residual block -- depthwise 3 x 3 computed into the B fragments of the
1 x 1 projection behind it -- with its input staged through LDS in bands of DN_PW_DW_BAND pixels, against the body that gathers nine taps per
pixel from global memory (DN_PW_DW_LDS=0). The contract of both is bit identity with dn_depthwise_conv followed by dn_pointwise_conv on the
same tensors, so every case calls dn_depthwise_pointwise under both knob values and compares with that pair by torch.equal. The knob is read
at the launch; the model-level tests build a fresh model (plan, captured graph) per value.

Inputs are random fp16 values of both signs with a few +-large ones (hundreds, against a typical 1): a pad row or column that is not zero
shows up as a different rounding of the depthwise sum. Shapes are the smallest that reach each edge of the staging -- one tile, a ragged last
tile, bands that end in the middle of a row, maps one pixel wide or high, row lengths that are no multiple of the 32-pixel tile, nine images
(the XCD grouping with a short last group), maps just below / at / above one band and above two -- plus the two real maps at two images.
"""
import ctypes as C
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# pixels per band: the library's constant (include/demonet_hip.h), the only place it is written down
BAND = int(re.search(r"^#define DN_PW_DW_BAND (\d+)$", open(os.path.join(ROOT, "include", "demonet_hip.h")).read(), re.M).group(1))
RELU, RELU6, HSWISH, NONE = 1, 2, 3, 0      # demonet_hip.h DN_ACT_*


def _lib():
    from demonet_amd import _lib as L
    return L, L.lib()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


_PROBLEMS = {}


def _problem(n, h, w, c, cout, act_dw, act, res):
    """Device tensors and the two-launch result (dn_depthwise_conv, then dn_pointwise_conv), made once per case and left unchanged."""
    key = (n, h, w, c, cout, act_dw, act, res)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    L, lib = _lib()
    g = torch.Generator().manual_seed(n * 7919 + h * 131 + w * 17 + c + cout * 3 + act_dw * 5 + act)
    x = torch.randn(n, h, w, c, generator=g)
    big = torch.rand(n, h, w, c, generator=g) < 0.02
    x = torch.where(big, x * 300.0, x).half().cuda()
    wd = (torch.randn(9, c, generator=g) / 3).half().cuda()
    bd = torch.randn(c, generator=g).cuda()
    wp = (torch.randn(cout, c, generator=g) / c ** 0.5).half().cuda()
    bp = torch.randn(cout, generator=g).cuda()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    mid = torch.zeros(n, h, w, c, dtype=torch.half, device="cuda")
    ref = torch.zeros(n, h, w, cout, dtype=torch.half, device="cuda")
    L.check(lib.dn_depthwise_conv(_ptr(x), _ptr(wd), _ptr(bd), _ptr(mid), n, h, w, c, 3, 1, 1, act_dw, stream), "dn_depthwise_conv")
    L.check(lib.dn_pointwise_conv(_ptr(mid), _ptr(wp), None, _ptr(bp), _ptr(x) if res else None, None, _ptr(ref), n * h * w, c, cout, h * w, act, 0, 0,
                                  stream), "dn_pointwise_conv")
    torch.cuda.synchronize()
    assert torch.isfinite(ref.float()).all() and float(ref.float().abs().max()) > 1.0
    _PROBLEMS[key] = dict(x=x, wd=wd, bd=bd, wp=wp, bp=bp, ref=ref)
    return _PROBLEMS[key]


def _fused(p, n, h, w, c, cout, act_dw, act, res):
    L, lib = _lib()
    out = torch.full((n, h, w, cout), float("nan"), dtype=torch.half, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.dn_depthwise_pointwise(_ptr(p["x"]), _ptr(p["wd"]), _ptr(p["bd"]), _ptr(p["wp"]), _ptr(p["bp"]), _ptr(out), n, h, w, c, cout, act_dw, act,
                                       int(res), stream), "dn_depthwise_pointwise")
    torch.cuda.synchronize()
    assert L.debug_last_kernel() == f"pw_dw_direct_kernel<{c // 16}>"
    return out


def _check(monkeypatch, n, h, w, c, cout, act_dw=HSWISH, act=RELU, res=False, xcd="1"):
    monkeypatch.setenv("DN_XCD", xcd)
    p = _problem(n, h, w, c, cout, act_dw, act, res)
    for flag in ("0", "1"):
        monkeypatch.setenv("DN_PW_DW_LDS", flag)
        got = _fused(p, n, h, w, c, cout, act_dw, act, res)
        bad = (got.view(torch.int16) != p["ref"].view(torch.int16)).nonzero()
        assert bad.numel() == 0, f"DN_PW_DW_LDS={flag}: {bad.shape[0]} values differ from the two launches, first at (n, y, x, c) = {bad[0].tolist()}"


GEOMETRY = [
    # n, h, w
    (1, 4, 8),            # the smallest map: hw = 32, one tile
    (3, 5, 7),            # hw = 35: a ragged last tile, rows that end inside a tile
    (1, 32, 1),           # one pixel wide: both horizontal neighbours outside for every pixel
    (1, 1, 40),           # one pixel high: both vertical neighbours outside
    (1, 6, 33),           # rows that straddle tiles
    (2, 9, 37),
    (9, 6, 33),           # nine images: two per XCD group, the last group short
]


@pytest.mark.parametrize("c,cout", [(16, 16), (32, 16)])
@pytest.mark.parametrize("n,h,w", GEOMETRY)
def test_small_maps(n, h, w, c, cout, monkeypatch):
    _check(monkeypatch, n, h, w, c, cout, res=(c == cout))


@pytest.mark.parametrize("c", [16, 32])
def test_nine_images_plain_mapping(c, monkeypatch):
    """DN_XCD=0: workgroups in image order"""
    _check(monkeypatch, 9, 6, 33, c, 16, xcd="0")


# maps of one row band minus a bit, exactly one band, one band and a bit, two bands and a bit: 16-pixel rows, so that bands end on and off a row's end
@pytest.mark.parametrize("c", [16, 32])
@pytest.mark.parametrize("pixels", [BAND - 16, BAND, BAND + 16, 2 * BAND + 16])
def test_maps_around_the_band_length(pixels, c, monkeypatch):
    assert pixels % 16 == 0
    _check(monkeypatch, 2, pixels // 16, 16, c, c, res=True)


def test_bands_that_end_mid_row(monkeypatch):
    """37-pixel rows: no band boundary falls on a row's end, the last band is ragged"""
    h = (2 * BAND + 100) // 37
    _check(monkeypatch, 2, h, 37, 16, 16, res=True)


@pytest.mark.parametrize("c,cout,res", [(16, 8, False), (16, 16, False), (16, 16, True), (16, 24, False), (16, 32, False),
                                        (32, 16, False), (32, 32, False), (32, 32, True)])
def test_output_widths_and_residual(c, cout, res, monkeypatch):
    """a residual needs cout == cin"""
    _check(monkeypatch, 3, 9, 37, c, cout, res=res)


@pytest.mark.parametrize("act_dw,act", [(RELU, NONE), (HSWISH, RELU), (RELU6, NONE), (NONE, HSWISH), (RELU, RELU6)])
@pytest.mark.parametrize("c", [16, 32])
def test_activations(act_dw, act, c, monkeypatch):
    _check(monkeypatch, 2, 9, 37, c, c, act_dw=act_dw, act=act, res=True)


@pytest.mark.parametrize("h,c,cout,act_dw", [(160, 16, 16, RELU), (150, 32, 16, RELU6)])
def test_real_maps(h, c, cout, act_dw, monkeypatch):
    """the V3 block (160 x 160 x 16, ReLU, residual) and the V2 block (150 x 150 x 32 -> 16, ReLU6) at two images"""
    _check(monkeypatch, 2, h, h, c, cout, act_dw=act_dw, act=NONE, res=(c == cout))


@pytest.mark.parametrize("c", [16, 32])
def test_wide_map_takes_the_global_taps(c, monkeypatch):
    """A band and two halos of w + 1 pixels of a 1100-pixel row do not fit the LDS body's 64 KB ((640 + 2 * 1104) * 32 bytes): the launch takes the
    body with the global taps under either knob value, and still matches."""
    _check(monkeypatch, 1, 3, 1100, c, 16)


def test_refuses_what_the_kernel_does_not_cover():
    L, lib = _lib()
    x = torch.zeros(1, 8, 8, 64, dtype=torch.half, device="cuda")
    f = torch.zeros(64, device="cuda")
    for n, h, w, c, cout, res in [(1, 8, 8, 24, 16, 0), (1, 8, 8, 16, 40, 0), (1, 4, 4, 16, 16, 0), (1, 8, 8, 16, 8, 1)]:
        rc = lib.dn_depthwise_pointwise(_ptr(x), _ptr(x), _ptr(f), _ptr(x), _ptr(f), _ptr(x), n, h, w, c, cout, 1, 0, res, None)
        assert rc == -4, (n, h, w, c, cout, res, rc)          # DN_E_UNSUPPORTED
    assert lib.dn_depthwise_pointwise(None, _ptr(x), _ptr(f), _ptr(x), _ptr(f), _ptr(x), 1, 8, 8, 16, 16, 1, 0, 0, None) == -1      # DN_E_INVALID


def _heads(monkeypatch, env):
    from demonet_amd import models, synth
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    imgs = torch.from_numpy(synth.images(29, 2, 320, 320)).cuda()
    m = models.load_synthetic(models.ssdlite320_mobilenet_v3_large(num_classes=91), 0).cuda()
    return [t.clone() for t in m.forward_heads(imgs)]


def test_model_heads_bit_identical(monkeypatch):
    """ssdlite320_mobilenet_v3_large, two images: every head output equal bit for bit under both knob values, and with NaN patterns left in every
    LDS byte and vector register in front of every launch (DN_POISON=1, plain launches): the LDS body reads nothing it has not written."""
    base = _heads(monkeypatch, {"DN_PW_DW_LDS": "0"})
    lds = _heads(monkeypatch, {"DN_PW_DW_LDS": "1"})
    poisoned = _heads(monkeypatch, {"DN_PW_DW_LDS": "1", "DN_POISON": "1", "DN_GRAPH": "0"})
    assert all(torch.isfinite(t.float()).all() for t in lds) and float(lds[0].abs().max()) > 1.0
    for other in (lds, poisoned):
        assert len(other) == len(base) and all(torch.equal(a, b) for a, b in zip(other, base))
