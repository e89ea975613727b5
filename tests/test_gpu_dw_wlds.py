"""DN_DW_WLDS (depthwise.hip dw_body<.., WLDS>): the depthwise launches with their weights and biases in LDS and their input rows through raw
buffer loads, against the per-thread weight loads (DN_DW_WLDS=0) -- the same taps in the same order, so outputs, pooled partial rows and
squeeze-excitation scales must be equal bit for bit -- and against fp32 torch at the 4e-3 of tests/test_gpu_kernels.py.

Shapes: the smallest that reach each edge -- channel-group counts that are no power of two (72 / 8 = 9, 120 / 8 = 15: a workgroup's 256 items
straddle rows and end ragged), odd maps under stride 2, one wide launch (672 channels), the largest weight image that must still launch
(5 x 5 x 1024 channels: 51 KB + bias + the pooling scratch), 1 / 3 / 9 images (nine: ragged XCD groups; also with the grouping off).
DN_DW_WLDS=1 (the default) takes the LDS body for launches of at most 128 channels, with or without the squeeze-excitation tail; DN_DW_WLDS=2 also for
the wider ones, wherever the weight image fits -- so every case runs both values against 0.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _lib():
    from demonet_amd import _lib as L
    return L, L.lib()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _act(x, act):
    return [lambda v: v, F.relu, F.relu6, F.hardswish][act](x)


_PROBLEMS = {}


def _problem(n, h, w, c, k, s, act, sq):
    """Inputs on the device and the fp32 reference, made once per shape and left unchanged."""
    key = (n, h, w, c, k, s, act, sq)
    if key not in _PROBLEMS:
        g = torch.Generator().manual_seed(h * 131 + w * 17 + c + k + s)
        x = torch.randn(n, c, h, w, generator=g).half()
        wt = (torch.randn(c, 1, k, k, generator=g) / k).half()
        b = torch.randn(c, generator=g)
        pad = (k - 1) // 2
        ref = _act(F.conv2d(x.float(), wt.float(), b, s, pad, 1, c), act)
        p = dict(x=x.permute(0, 2, 3, 1).contiguous().cuda(), w=wt.view(c, k * k).t().contiguous().cuda(), b=b.cuda(), ref=ref, pad=pad)
        if sq:
            w1 = (torch.randn(sq, c, generator=g) / c ** 0.5).half()          # fc1 [sq][c], fc2 [c][sq]: stored transposed, fp16
            w2 = (torch.randn(c, sq, generator=g) / sq ** 0.5).half()
            b1, b2 = torch.randn(sq, generator=g) * 0.1, torch.randn(c, generator=g) * 0.1
            mean = ref.mean(dim=(2, 3))
            z = F.relu(mean @ w1.float().t() + b1)
            p.update(w1t=w1.t().contiguous().cuda(), w2t=w2.t().contiguous().cuda(), b1=b1.cuda(), b2=b2.cuda(),
                     scale_ref=F.hardsigmoid(z @ w2.float().t() + b2))
        _PROBLEMS[key] = p
    return _PROBLEMS[key]


def _run(n, h, w, c, k, s, act, mode, sq, monkeypatch, wlds, xcd="1"):
    """-> (out [n][ho][wo][c] fp16, partial rows or None, scale or None) under DN_DW_WLDS=wlds"""
    L, lib = _lib()
    monkeypatch.setenv("DN_DW_WLDS", wlds)
    monkeypatch.setenv("DN_XCD", xcd)
    p = _problem(n, h, w, c, k, s, act, sq if mode == "se" else 0)
    ho, wo = p["ref"].shape[-2:]
    out = torch.zeros(n, ho, wo, c, dtype=torch.half, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if mode == "none":
        L.check(lib.dn_depthwise_conv(_ptr(p["x"]), _ptr(p["w"]), _ptr(p["b"]), _ptr(out), n, h, w, c, k, s, p["pad"], act, stream), "dn_depthwise_conv")
        torch.cuda.synchronize()
        return out, None, None
    blocks = lib.dn_depthwise_pool_blocks(h, w, c, k, s, p["pad"])
    assert blocks > 0
    rows = torch.full((n, blocks, c), float("nan"), device="cuda")
    scale = counter = None
    if mode == "se":
        scale = torch.full((n, c), float("nan"), device="cuda")
        counter = torch.zeros(n, dtype=torch.int32, device="cuda")
    rc = lib.dn_depthwise_conv_pool(_ptr(p["x"]), _ptr(p["w"]), _ptr(p["b"]), _ptr(out), n, h, w, c, k, s, p["pad"], act, _ptr(rows),
                                    _ptr(p.get("w1t")) if scale is not None else None, _ptr(p.get("b1")) if scale is not None else None,
                                    _ptr(p.get("w2t")) if scale is not None else None, _ptr(p.get("b2")) if scale is not None else None,
                                    _ptr(scale), _ptr(counter), sq if scale is not None else 0, stream)
    L.check(rc, "dn_depthwise_conv_pool")
    torch.cuda.synchronize()
    if counter is not None:
        assert int(counter.abs().sum()) == 0          # left at zero for the next forward
    return out, rows, scale


def _check(n, h, w, c, k, s, act, mode, sq, monkeypatch, xcd="1"):
    base = _run(n, h, w, c, k, s, act, mode, sq, monkeypatch, "0", xcd)
    p = _problem(n, h, w, c, k, s, act, sq if mode == "se" else 0)
    ref = p["ref"]
    for wlds in ("1", "2"):
        got = _run(n, h, w, c, k, s, act, mode, sq, monkeypatch, wlds, xcd)
        assert torch.equal(got[0].view(torch.int16), base[0].view(torch.int16)), f"DN_DW_WLDS={wlds}: output bits differ"
        if mode != "none":
            assert torch.equal(got[1].view(torch.int32), base[1].view(torch.int32)), f"DN_DW_WLDS={wlds}: pooled partial rows differ"
        if mode == "se":
            assert torch.equal(got[2].view(torch.int32), base[2].view(torch.int32)), f"DN_DW_WLDS={wlds}: SE scales differ"
        torch.testing.assert_close(got[0].cpu().float().permute(0, 3, 1, 2), ref.half().float(), rtol=4e-3, atol=4e-3)
        if mode != "none":
            # the rows sum the fp32 accumulators (inputs and weights are exact fp16 values): against the fp32 reference only the order of at most
            # ho * wo * k * k fp32 additions differs -- <= 1600 * 25 * 2^-24 relative to values of order 1, far below 1e-2
            torch.testing.assert_close(got[1].sum(dim=1).cpu(), ref.sum(dim=(2, 3)), rtol=1e-3, atol=1e-2)
        if mode == "se":
            torch.testing.assert_close(got[2].cpu(), p["scale_ref"], rtol=1e-4, atol=1e-4)      # fp32 FCs on fp16 weights: summation order only


CASES = [
    # n, h, w, c, k, s, act, mode, squeeze
    (1, 7, 5, 72, 3, 1, 1, "none", 0),
    (3, 7, 5, 72, 3, 2, 2, "pool", 0),
    (1, 13, 9, 72, 5, 2, 1, "se", 24),          # odd map under stride 2, small SE tail
    (3, 13, 9, 120, 3, 2, 3, "none", 0),
    (3, 10, 10, 120, 5, 1, 3, "se", 32),        # two workgroups per image, small tail
    (9, 10, 10, 120, 5, 1, 0, "pool", 0),       # nine images: ragged XCD groups; identity activation
    (9, 10, 10, 72, 5, 2, 1, "se", 24),
    (9, 13, 9, 120, 3, 1, 2, "none", 0),
    (3, 10, 10, 72, 3, 1, 3, "se", 24),
    (1, 7, 5, 120, 5, 2, 0, "pool", 0),
    (3, 6, 6, 672, 5, 1, 3, "pool", 0),         # wide: 84 groups, three copy batches
    (1, 6, 6, 672, 3, 1, 3, "none", 0),
    (3, 4, 4, 1024, 5, 1, 1, "pool", 0),        # the 51 KB weight image + bias + pooling scratch
    (1, 4, 4, 1024, 5, 2, 3, "none", 0),
    (3, 40, 40, 120, 5, 1, 3, "se", 32),        # the 40 x 40 block of the V3 plan: 24 workgroups per image
    (1, 40, 40, 120, 5, 1, 1, "none", 0),
    (3, 10, 10, 480, 3, 1, 3, "se", 120),       # the large tail (what the plan sends here under DN_SE_IN_DW=1)
    (1, 7, 5, 480, 5, 1, 3, "se", 120),
]


@pytest.mark.parametrize("n,h,w,c,k,s,act,mode,sq", CASES)
def test_dw_wlds_bit_identical(n, h, w, c, k, s, act, mode, sq, monkeypatch):
    if sq == 120:
        monkeypatch.setenv("DN_SE_IN_DW", "1")
    _check(n, h, w, c, k, s, act, mode, sq, monkeypatch)


@pytest.mark.parametrize("n,h,w,c,k,s,act,mode,sq", [(9, 10, 10, 120, 5, 1, 3, "se", 32), (9, 13, 9, 72, 3, 2, 1, "pool", 0), (9, 7, 5, 120, 5, 2, 2, "none", 0)])
def test_dw_wlds_plain_image_mapping(n, h, w, c, k, s, act, mode, sq, monkeypatch):
    """nine images with DN_XCD=0: blockIdx.y is the image"""
    _check(n, h, w, c, k, s, act, mode, sq, monkeypatch, xcd="0")


@pytest.mark.parametrize("c,k,s,mode,sq", [(72, 3, 1, "pool", 0), (120, 5, 2, "none", 0), (120, 5, 1, "se", 32)])
def test_dw_wlds_reads_no_uncopied_lds(c, k, s, mode, sq, monkeypatch):
    """Other launches leave NaN in LDS first: the 5 x 5 x 1024-channel depthwise with NaN weights and biases, forced onto the LDS body
    (DN_DW_WLDS=2: 1024 channels are beyond the default's 128), once plain -- a 55 KB image of NaN weights and biases from the start of a
    workgroup's LDS -- and once pooled: the same image followed by red[] (62 KB), whose per-thread sums are NaN as well. 512 workgroups each,
    two fit a compute unit. A weight, bias or red[] slot that the launch under test reads without having written it would now be NaN.
    (The library has no kernel that reads LDS it has not written, so the poison cannot be read back; what sends the poisoning launches through
    LDS is the knob value set for them -- dw_wlds_bytes: 2 = wherever the image fits -- and their NaN outputs and pooled rows show they ran.)"""
    L, lib = _lib()
    n, h, w = 3, 10, 10
    base = _run(n, h, w, c, k, s, 1, mode, sq, monkeypatch, "0")
    nan_w = torch.full((25, 1024), float("nan"), dtype=torch.half, device="cuda")
    nan_b = torch.full((1024,), float("nan"), device="cuda")
    px = torch.zeros(64, 8, 8, 1024, dtype=torch.half, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pblocks = lib.dn_depthwise_pool_blocks(8, 8, 1024, 5, 1, 2)
    for wlds in ("1", "2"):
        pout = torch.zeros_like(px)
        prow = torch.zeros(64, pblocks, 1024, device="cuda")
        monkeypatch.setenv("DN_DW_WLDS", "2")
        L.check(lib.dn_depthwise_conv(_ptr(px), _ptr(nan_w), _ptr(nan_b), _ptr(pout), 64, 8, 8, 1024, 5, 1, 2, 0, stream), "dn_depthwise_conv")
        L.check(lib.dn_depthwise_conv_pool(_ptr(px), _ptr(nan_w), _ptr(nan_b), _ptr(pout), 64, 8, 8, 1024, 5, 1, 2, 0, _ptr(prow),
                                           None, None, None, None, None, None, 0, stream), "dn_depthwise_conv_pool")
        got = _run(n, h, w, c, k, s, 1, mode, sq, monkeypatch, wlds)
        assert torch.isnan(pout.float()).all() and torch.isnan(prow).all()
        for a, b in zip(got, base):
            if a is not None:
                assert torch.isfinite(a.float()).all() and torch.equal(a, b)


def test_dw_wlds_model_heads_bit_identical(monkeypatch):
    """ssdlite320_mobilenet_v3_large, three images, forward_heads: every head output equal bit for bit under both knob values."""
    from demonet_amd import models, synth
    imgs = torch.from_numpy(synth.images(29, 3, 320, 320)).cuda()
    res = {}
    for wlds in ("0", "1", "2"):
        monkeypatch.setenv("DN_DW_WLDS", wlds)
        m = models.load_synthetic(models.ssdlite320_mobilenet_v3_large(num_classes=91), 0).cuda()
        res[wlds] = [t.clone() for t in m.forward_heads(imgs)]
    for wlds in ("1", "2"):
        assert len(res[wlds]) == len(res["0"]) and all(torch.equal(a, b) for a, b in zip(res[wlds], res["0"]))
    assert all(torch.isfinite(t.float()).all() for t in res["1"])
