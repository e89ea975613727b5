"""GPU tests (-m gpu) of the row-reuse body of the fused 24 -> 72 -> cout stride-1 block (expdw_rows.hip, DN_EXPDW_ROWS=1, the default where it applies):
a wave walks down a 32-lane column strip, expands every input row once and keeps the last three expanded rows in registers. Same operands, same K order,
same rounding points and same tap order as the tiled bodies of expdw.hip, so every output is held to them BIT FOR BIT: to expdw_one_kernel /
expdw_kernel<..., ONE> (DN_EXPDW_ROWS=0) and to one workgroup per tile (DN_EXPDW_ROWS=0, DN_EXPDW_PERSIST=0)."""
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


def _choice(L, n, h, w, cin, cexp, cout, k, s, act1, act2, res, pool=0):
    return L.debug_choice("expdw", n, h, w, cin, cexp, cout, k, s, act1, act2, int(res), pool)


def _run(monkeypatch, n, h, w, cin=24, cexp=72, cout=24, k=3, s=1, act1=RELU, act2=RELU, res=True, rows=True):
    """The block under DN_EXPDW_ROWS=1, =0 and =0 with DN_EXPDW_PERSIST=0: output pre-filled with NaN, run twice (the second run starts from a used
    LDS / L2 state), finite afterwards, all three equal. rows: what the choice export must say about the shape under the default knob."""
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
    for key, env in (("rows", {"DN_EXPDW_ROWS": "1", "DN_EXPDW_PERSIST": "1"}), ("tiled", {"DN_EXPDW_ROWS": "0", "DN_EXPDW_PERSIST": "1"}),
                     ("per_tile", {"DN_EXPDW_ROWS": "0", "DN_EXPDW_PERSIST": "0"})):
        for kk, v in env.items():
            monkeypatch.setenv(kk, v)
        choice = _choice(L, n, h, w, cin, cexp, cout, k, s, act1, act2, res)
        assert choice["body"] == ("rows" if key == "rows" and rows else "tiled"), (key, choice)
        out = torch.full((n, ho, wo, cout), float("nan"), dtype=torch.half, device="cuda")
        for _ in range(2):
            L.check(lib.dn_expand_depthwise(_ptr(x), _ptr(w1), _ptr(b1), _ptr(wd), _ptr(bd), _ptr(w3), _ptr(b3), _ptr(out), None,
                                            n, h, w, cin, cexp, cout, k, s, act1, act2, int(res),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dn_expand_depthwise")
            assert L.debug_last_kernel() == choice["label"]
        torch.cuda.synchronize()
        outs[key] = out
    assert torch.isfinite(outs["rows"].float()).all()
    assert float(outs["rows"].float().abs().max()) > 0.5
    for key in ("tiled", "per_tile"):
        bad = (outs["rows"] != outs[key])
        assert torch.equal(outs["rows"], outs[key]), (key, int(bad.sum()), bad.nonzero()[:4].tolist())


@pytest.mark.parametrize("n,h,w", [
    (1, 1, 1),              # fewer rows than the ring, narrower than a strip
    (1, 2, 5),
    (2, 7, 30),             # the last valid lane of a strip
    (2, 9, 31),             # ... and one pixel into the next
    (2, 11, 61),            # two strip seams, rows not a multiple of 3 or of the band
    (3, 10, 80),            # the real width, a band count that does not divide the rows
    (9, 12, 20),            # grouped mapping (>= 8 images), ragged last group
    (2, 80, 80),            # the real map
])
def test_rows_body_bit_identical(n, h, w, monkeypatch):
    _run(monkeypatch, n, h, w)


@pytest.mark.parametrize("cout", [16, 32])
def test_other_output_widths_without_a_residual(cout, monkeypatch):
    _run(monkeypatch, 2, 9, 31, cout=cout, res=False)


@pytest.mark.parametrize("res", [True, False])
def test_with_and_without_a_residual(res, monkeypatch):
    _run(monkeypatch, 2, 9, 31, res=res)


@pytest.mark.parametrize("act1", [NONE, RELU, RELU6, HSWISH])
@pytest.mark.parametrize("act2", [NONE, RELU, RELU6, HSWISH])
def test_every_activation_pair(act1, act2, monkeypatch):
    _run(monkeypatch, 2, 9, 31, act1=act1, act2=act2)


@pytest.mark.parametrize("band", [1, 2, 3, 7])
def test_other_band_heights(band, monkeypatch):
    """DN_EXPDW_ROWS_BAND (output rows per band): 11 rows in bands of 1, 2, 3 and 7"""
    monkeypatch.setenv("DN_EXPDW_ROWS_BAND", str(band))
    L, _ = _lib()
    monkeypatch.setenv("DN_EXPDW_ROWS", "1")
    choice = _choice(L, 2, 11, 61, 24, 72, 24, 3, 1, RELU, RELU, True)
    assert (choice["body"], choice["band"]) == ("rows", band)
    _run(monkeypatch, 2, 11, 61)


@pytest.mark.parametrize("cin,cexp,cout,k,s,res", [
    (24, 72, 24, 3, 2, False),      # stride 2 with the same channels
    (24, 64, 24, 3, 1, True),       # cexp 64
    (24, 144, 24, 3, 1, True),      # cexp 144: two chunks
    (16, 72, 16, 3, 1, True),       # cin 16
    (32, 72, 32, 3, 1, True),       # cin 32
    (24, 72, 40, 3, 1, False),      # cout above 32
    (24, 72, 24, 5, 1, True),       # k = 5
])
def test_shapes_outside_the_list_take_the_old_body(cin, cexp, cout, k, s, res, monkeypatch):
    _run(monkeypatch, 2, 9, 31, cin=cin, cexp=cexp, cout=cout, k=k, s=s, res=res, rows=False)


def test_pooled_sums_keep_the_old_body(monkeypatch):
    """(a launch with a project stage never carries pooled sums, so the choice export is where this can be asked)"""
    L, _ = _lib()
    monkeypatch.setenv("DN_EXPDW_ROWS", "1")
    assert _choice(L, 2, 9, 31, 24, 72, 24, 3, 1, RELU, RELU, True, pool=0)["body"] == "rows"
    assert _choice(L, 2, 9, 31, 24, 72, 24, 3, 1, RELU, RELU, True, pool=1)["body"] == "tiled"


def _heads(monkeypatch, env):
    from demonet_amd import models, synth
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    imgs = torch.from_numpy(synth.images(29, 2, 320, 320)).cuda()
    m = models.load_synthetic(models.ssdlite320_mobilenet_v3_large(num_classes=91), 0).cuda()
    return [t.clone() for t in m.forward_heads(imgs)]


def test_model_heads_bit_identical(monkeypatch):
    """ssdlite320_mobilenet_v3_large, two images: the 80 x 80 block (24 -> 72 -> 24, ReLU, residual) takes the new body, every head output equals the old
    body's bit for bit, also with NaN patterns left in every LDS byte and vector register in front of every launch (DN_POISON=1, plain launches)."""
    L, _ = _lib()
    monkeypatch.setenv("DN_EXPDW_ROWS", "1")
    assert _choice(L, 2, 80, 80, 24, 72, 24, 3, 1, RELU, RELU, True)["body"] == "rows"
    base = _heads(monkeypatch, {"DN_EXPDW_ROWS": "0"})
    new = _heads(monkeypatch, {"DN_EXPDW_ROWS": "1"})
    poisoned = _heads(monkeypatch, {"DN_EXPDW_ROWS": "1", "DN_POISON": "1", "DN_GRAPH": "0"})
    assert all(torch.isfinite(t.float()).all() for t in new) and float(new[0].abs().max()) > 1.0
    for other in (new, poisoned):
        assert len(other) == len(base) and all(torch.equal(a, b) for a, b in zip(other, base))
