"""GPU tests (-m gpu) of the per-tap body of the fused 16 -> 64 -> cout stride-2 block (expdw_direct.hip, DN_EXPDW_DIRECT=1, the default where it
applies): the expanded value of every tap comes out of the matrix cores and goes straight into the depthwise sum. Same operands, same K order and
same rounding points as the tiled bodies of expdw.hip, so every output is held to them BIT FOR BIT: to expdw_one_kernel / expdw_kernel<..., ONE>
(DN_EXPDW_DIRECT=0) and to one workgroup per tile (DN_EXPDW_DIRECT=0, DN_EXPDW_PERSIST=0)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

NONE, RELU, RELU6, HSWISH = 0, 1, 2, 3


def _lib():
    from demonet_amd import _lib as L
    return L, L.lib()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _choice(L, n, h, w, cin, cexp, cout, k, s, act1, act2, res):
    return L.debug_choice("expdw", n, h, w, cin, cexp, cout, k, s, act1, act2, int(res), 0)


def _run(monkeypatch, n, h, w, cin, cexp, cout, k=3, s=2, act1=RELU, act2=RELU, res=False, direct=True):
    """The block under DN_EXPDW_DIRECT=1, =0 and =0 with DN_EXPDW_PERSIST=0: output pre-filled with NaN, run twice (the second run starts from a used
    LDS / L2 state), finite afterwards, all three equal. direct: what the choice export must say about the shape under the default knob."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(h * 5 + w + cout + n)
    x = torch.randn(n, h, w, cin, generator=g).half().cuda()
    w1 = (torch.randn(cexp, cin, generator=g) / cin ** 0.5).half().cuda()
    b1 = (torch.randn(cexp, generator=g) * 0.1).cuda()
    wd = (torch.randn(k * k, cexp, generator=g) / k).half().cuda()
    bd = (torch.randn(cexp, generator=g) * 0.1).cuda()
    w3 = (torch.randn(cout, cexp, generator=g) / cexp ** 0.5).half().cuda()
    b3 = (torch.randn(cout, generator=g) * 0.1).cuda()
    pad = (k - 1) // 2
    ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    outs = {}
    for key, env in (("direct", {"DN_EXPDW_DIRECT": "1", "DN_EXPDW_PERSIST": "1"}), ("tiled", {"DN_EXPDW_DIRECT": "0", "DN_EXPDW_PERSIST": "1"}),
                     ("per_tile", {"DN_EXPDW_DIRECT": "0", "DN_EXPDW_PERSIST": "0"})):
        for kk, v in env.items():
            monkeypatch.setenv(kk, v)
        choice = _choice(L, n, h, w, cin, cexp, cout, k, s, act1, act2, res)
        assert choice["body"] == ("direct" if key == "direct" and direct else "tiled"), (key, choice)
        out = torch.full((n, ho, wo, cout), float("nan"), dtype=torch.half, device="cuda")
        for _ in range(2):
            L.check(lib.dn_expand_depthwise(_ptr(x), _ptr(w1), _ptr(b1), _ptr(wd), _ptr(bd), _ptr(w3), _ptr(b3), _ptr(out), None,
                                            n, h, w, cin, cexp, cout, k, s, act1, act2, int(res),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dn_expand_depthwise")
            assert L.debug_last_kernel() == choice["label"]
        torch.cuda.synchronize()
        outs[key] = out
    assert torch.isfinite(outs["direct"].float()).all()
    assert float(outs["direct"].float().abs().max()) > 0.5
    for key in ("tiled", "per_tile"):
        bad = (outs["direct"] != outs[key])
        assert torch.equal(outs["direct"], outs[key]), (key, int(bad.sum()), bad.nonzero()[:4].tolist())


@pytest.mark.parametrize("n,h,w,cout", [
    (1, 8, 8, 24),          # one tile, smaller than a band
    (2, 36, 44, 24),        # ragged last tile of an image
    (2, 35, 43, 24),        # odd sizes: bottom and right taps outside, top and left pads too
    (3, 10, 160, 24),       # the real row width; a band count that does not divide the rows
    (9, 20, 24, 24),        # grouped mapping (>= 8 images), ragged last group
    (12, 36, 44, 24),
    (2, 160, 160, 24),      # the real map
    (2, 36, 44, 16),
    (2, 35, 43, 32),
])
def test_direct_body_bit_identical(n, h, w, cout, monkeypatch):
    _run(monkeypatch, n, h, w, 16, 64, cout)


@pytest.mark.parametrize("act1", [NONE, RELU, RELU6, HSWISH])
@pytest.mark.parametrize("act2", [NONE, RELU, RELU6, HSWISH])
def test_every_activation_pair(act1, act2, monkeypatch):
    _run(monkeypatch, 2, 35, 43, 16, 64, 24, act1=act1, act2=act2)


@pytest.mark.parametrize("band", [1, 2, 3])
def test_other_band_heights(band, monkeypatch):
    """DN_EXPDW_DIRECT_BAND (output rows per band, default 4): 18 output rows in bands of 1, 2 and 3"""
    monkeypatch.setenv("DN_EXPDW_DIRECT_BAND", str(band))
    _run(monkeypatch, 2, 35, 43, 16, 64, 24)


@pytest.mark.parametrize("n,h,w,cin,cexp,cout,s,res", [
    (2, 36, 44, 24, 64, 24, 2, False),      # cin 24
    (2, 36, 44, 16, 64, 16, 1, True),       # stride 1 with a residual
    (2, 36, 44, 16, 64, 40, 2, False),      # cout above 32
    (2, 36, 44, 16, 128, 24, 2, False),     # two chunks
    (1, 4, 700, 16, 64, 24, 2, False),      # one output row of a 700-wide map needs 67 KB of input rows: no band fits LDS
])
def test_shapes_outside_the_list_take_the_old_body(n, h, w, cin, cexp, cout, s, res, monkeypatch):
    _run(monkeypatch, n, h, w, cin, cexp, cout, s=s, res=res, direct=False)


def _heads(monkeypatch, env):
    from demonet_amd import models, synth
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    imgs = torch.from_numpy(synth.images(29, 2, 320, 320)).cuda()
    m = models.load_synthetic(models.ssdlite320_mobilenet_v3_large(num_classes=91), 0).cuda()
    return [t.clone() for t in m.forward_heads(imgs)]


def test_model_heads_bit_identical(monkeypatch):
    """ssdlite320_mobilenet_v3_large, two images: the 160 x 160 block (16 -> 64 -> 24, ReLU) takes the new body, every head output equals the old
    body's bit for bit, also with NaN patterns left in every LDS byte and vector register in front of every launch (DN_POISON=1, plain launches)."""
    L, _ = _lib()
    monkeypatch.setenv("DN_EXPDW_DIRECT", "1")
    choice = _choice(L, 2, 160, 160, 16, 64, 24, 3, 2, RELU, RELU, False)
    assert (choice["body"], choice["band"]) == ("direct", 4)
    base = _heads(monkeypatch, {"DN_EXPDW_DIRECT": "0"})
    new = _heads(monkeypatch, {"DN_EXPDW_DIRECT": "1"})
    poisoned = _heads(monkeypatch, {"DN_EXPDW_DIRECT": "1", "DN_POISON": "1", "DN_GRAPH": "0"})
    assert all(torch.isfinite(t.float()).all() for t in new) and float(new[0].abs().max()) > 1.0
    for other in (new, poisoned):
        assert len(other) == len(base) and all(torch.equal(a, b) for a, b in zip(other, base))
