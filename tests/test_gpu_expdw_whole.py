"""GPU tests (-m gpu) of the whole-width form of the tiled fused-block body (expdw_whole.hip; a flag of expdw_choose's TILED answer, DN_EXPDW_WHOLE:
1 = the two widths of the 20 x 20 blocks of MobileNetV3, 0 = never, 2 = wherever the form can run): the phases of expdw_kernel walked once per 5 x 10
tile over every expanded channel instead of once per 64-channel chunk. Same operands, same K steps in the same order, same rounding points, same tap
order: every output is held to the chunk loop (DN_EXPDW_WHOLE=0) BIT FOR BIT."""
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


def _query(n, h, w, cin, cexp, cout, k, s, act1, act2, res, pool=0):
    return (n, h, w, cin, cexp, cout, k, s, act1, act2, int(res), pool)


def _run(monkeypatch, n, h, w, cin=80, cexp=200, cout=80, k=3, s=1, act1=HSWISH, act2=HSWISH, res=True, whole=True):
    """The block under DN_EXPDW_WHOLE=2 and =0: output pre-filled with NaN, run twice (the second run starts from a used LDS / L2 state), finite
    afterwards, both equal. whole: what the "expdw_whole" query must say about the shape under DN_EXPDW_WHOLE=2; the "expdw" query (label, body, band,
    tile) must not depend on the knob. cout 0: no project stage (the output has cexp channels)."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(h * 5 + w + cexp + n)
    x = torch.randn(n, h, w, cin, generator=g).half().cuda()
    w1 = (torch.randn(cexp, cin, generator=g) / cin ** 0.5).half().cuda()
    b1 = (torch.randn(cexp, generator=g) * 0.1).cuda()
    wd = (torch.randn(k * k, cexp, generator=g) / k).half().cuda()
    bd = (torch.randn(cexp, generator=g) * 0.1).cuda()
    w3 = (torch.randn(cout, cexp, generator=g) / cexp ** 0.5).half().cuda() if cout else None
    b3 = (torch.randn(cout, generator=g) * 0.1).cuda() if cout else None
    pad = (k - 1) // 2
    ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    q = _query(n, h, w, cin, cexp, cout, k, s, act1, act2, res)
    outs, labels = {}, {}
    for knob in (2, 0):
        monkeypatch.setenv("DN_EXPDW_WHOLE", str(knob))
        labels[knob] = L.debug_choice("expdw", *q)
        flag = L.debug_choice("expdw_whole", *q)
        assert flag["whole"] == int(whole and knob == 2), (knob, flag)
        assert (flag["lds"] > 0) == bool(flag["whole"]) and flag["lds"] <= 80 * 1024
        out = torch.full((n, ho, wo, cout or cexp), float("nan"), dtype=torch.half, device="cuda")
        for _ in range(2):
            L.check(lib.dn_expand_depthwise(_ptr(x), _ptr(w1), _ptr(b1), _ptr(wd), _ptr(bd), _ptr(w3), _ptr(b3), _ptr(out), None,
                                            n, h, w, cin, cexp, cout, k, s, act1, act2, int(res),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dn_expand_depthwise")
            assert L.debug_last_kernel() == labels[knob]["label"]
        torch.cuda.synchronize()
        outs[knob] = out
    assert labels[2] == labels[0] and labels[0]["body"] == "tiled"
    assert torch.isfinite(outs[2].float()).all()
    assert float(outs[2].float().abs().max()) > 0.5
    bad = outs[2] != outs[0]
    assert torch.equal(outs[2], outs[0]), (int(bad.sum()), bad.nonzero()[:4].tolist())


# expanded widths: 200 (64 + 64 + 64 + a tail chunk of 8), 184 (tail of 56), 136 (64 + 64 + 8), 128 (no tail), 72 (64 + 8); cin = cout = 80, residual
WIDTHS = [200, 184, 136, 128, 72]
# maps: one whole 5 x 10 tile, ragged tiles in both directions, the real map (2 x 4 tiles)
MAPS = [(5, 10), (7, 13), (20, 20)]


@pytest.mark.parametrize("cexp", WIDTHS)
@pytest.mark.parametrize("h,w", MAPS)
@pytest.mark.parametrize("n", [1, 3])
def test_whole_form_bit_identical(n, h, w, cexp, monkeypatch):
    _run(monkeypatch, n, h, w, cexp=cexp)


@pytest.mark.parametrize("cexp", [48, 224])
def test_the_narrowest_and_the_widest_block_the_form_takes(cexp, monkeypatch):
    """48: the narrowest E tile that holds the staged 80-channel output, two channel tiles shared by four waves each; 224: seven full channel tiles, the
    LDS limit"""
    _run(monkeypatch, 2, 7, 13, cexp=cexp)


@pytest.mark.parametrize("w,cout,cexp", [(13, 80, 200), (13, 96, 184), (10, 24, 200), (13, 128, 136), (10, 8, 8)])
def test_without_a_residual(w, cout, cexp, monkeypatch):
    """also output widths other than the input's: one, three and four channel tiles of the projection (cout 128: all eight waves hold a unit; cout 24 and 8 on
    a map of at most 10 columns: wider maps give them the 10 x 10 tile; 8 -> 8: one channel group, one K step with an empty upper half)"""
    _run(monkeypatch, 2, 7, w, cexp=cexp, cout=cout, res=False)


@pytest.mark.parametrize("act1", [NONE, RELU, RELU6, HSWISH])
@pytest.mark.parametrize("act2", [NONE, RELU, RELU6, HSWISH])
def test_every_activation_pair(act1, act2, monkeypatch):
    _run(monkeypatch, 1, 5, 10, act1=act1, act2=act2)


@pytest.mark.parametrize("n", [9, 13])
def test_a_batch_that_is_no_multiple_of_the_xcd_grouping(n, monkeypatch):
    """8 images or more take the grouped mapping: 9 and 13 images leave ragged last groups"""
    _run(monkeypatch, n, 7, 13)
    _run(monkeypatch, n, 20, 20, cexp=184)


@pytest.mark.parametrize("name,kw", [
    ("stride 2", dict(s=2, res=False)),
    ("5x5 kernel", dict(k=5)),
    ("no project stage", dict(cout=0, res=False)),
    ("an expanded width beyond the LDS limit: 232", dict(cexp=232)),
    ("... and 480", dict(cexp=480)),
    ("the 10 x 10 tile (cout 64)", dict(cout=64, res=False)),
    ("cin 72: the same 88-half X rows, four full K steps", dict(cin=72, cout=72)),
    ("cin 64 (and the 10 x 10 tile)", dict(cin=64, cout=64)),
    ("40 channels: the staged tile does not fit the dead E rows", dict(cexp=40)),
], ids=lambda v: v if isinstance(v, str) else "")
def test_shapes_that_keep_the_chunk_loop(name, kw, monkeypatch):
    _run(monkeypatch, 2, 20, 20, whole=False, **kw)


def test_the_5x5_tile_keeps_the_chunk_loop(monkeypatch):
    _run(monkeypatch, 2, 5, 5, whole=False)


def test_pooled_sums_keep_the_chunk_loop(monkeypatch):
    """(a launch with a project stage never carries pooled sums, so the choice export is where this can be asked)"""
    L, _ = _lib()
    monkeypatch.setenv("DN_EXPDW_WHOLE", "2")
    assert L.debug_choice("expdw_whole", *_query(2, 20, 20, 80, 200, 80, 3, 1, HSWISH, HSWISH, True, pool=0))["whole"] == 1
    assert L.debug_choice("expdw_whole", *_query(2, 20, 20, 80, 200, 80, 3, 1, HSWISH, HSWISH, True, pool=1))["whole"] == 0
    assert L.debug_choice("expdw_whole", *_query(2, 20, 20, 80, 200, 0, 3, 1, HSWISH, HSWISH, False, pool=1))["whole"] == 0


def _heads(monkeypatch, env):
    from demonet_amd import models, synth
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    imgs = torch.from_numpy(synth.images(29, 2, 320, 320)).cuda()
    m = models.load_synthetic(models.ssdlite320_mobilenet_v3_large(num_classes=91), 0).cuda()
    return [t.clone() for t in m.forward_heads(imgs)]


def test_model_heads_bit_identical(monkeypatch):
    """ssdlite320_mobilenet_v3_large, two images: the three 20 x 20 blocks (80 -> 200 -> 80 once, 80 -> 184 -> 80 twice, hard-swish, residual) take the
    whole-width form by default, every head output equals the chunk loop's bit for bit, also with NaN patterns left in every LDS byte and vector
    register in front of every launch (DN_POISON=1, plain launches)."""
    L, _ = _lib()
    monkeypatch.setenv("DN_EXPDW_WHOLE", "1")
    for cexp in (200, 184):
        assert L.debug_choice("expdw_whole", *_query(2, 20, 20, 80, cexp, 80, 3, 1, HSWISH, HSWISH, True))["whole"] == 1
    base = _heads(monkeypatch, {"DN_EXPDW_WHOLE": "0"})
    new = _heads(monkeypatch, {"DN_EXPDW_WHOLE": "1"})
    poisoned = _heads(monkeypatch, {"DN_EXPDW_WHOLE": "1", "DN_POISON": "1", "DN_GRAPH": "0"})
    assert all(torch.isfinite(t.float()).all() for t in new) and float(new[0].abs().max()) > 1.0
    for other in (new, poisoned):
        assert len(other) == len(base) and all(torch.equal(a, b) for a, b in zip(other, base))
