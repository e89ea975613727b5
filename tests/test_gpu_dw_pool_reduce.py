"""The squeeze-excitation pooling of the depthwise launches (depthwise.hip dw_body, POOL 1 and 2): a workgroup's partial row, recomputed on the host from
the device's own fp16 outputs in the documented order, must equal the device's row bit for bit.

The order (dw_body): item i = bx * 256 + tid of image n is channel group i % C8 (C8 = c / 8) of strip i / C8, strips row-major over (output row, TW
columns; TW = 4 at stride 1, 2 at stride 2); a thread adds its strip's outputs column by column to a zero; thread tid < C8 of the workgroup then adds the
per-thread sums u = tid, tid + C8, ... < 256 in that order to a zero, one fp32 accumulator per channel, and writes pool[n][bx][8 (i % C8) ..].
Whatever is done to that last loop (a form that reads the rows from LDS in batches of eight was built, measured level and not kept: profiles/pw_wstat_proj_ab.txt),
the additions keep this order: the pooled rows, and with them the squeeze-excitation scales and everything behind them, are pinned to it bit for bit.

A thread sums its fp32 accumulators, not the rounded outputs, so the inputs are chosen such that the two are the same numbers: per channel ONE tap of the
filter is +-1, +-2 or +-4 and all others are zero, the bias is zero, the activation is none or ReLU -- every accumulator is then +-2^j x for an input
value x and exact in fp16. The inputs spread over 2^-8 .. 2^8 with 11-bit mantissas, so fp32 sums of 4 and then 2 .. 256 of them round, and round
differently in another order (the test checks that about its own data: the rows summed in reverse order differ).

Shapes: C8 = 15 and 9 (the 40 x 40 launches of the V3 plan: 17 - 18 and 28 - 29 rows per thread), 84 and 128 (3 - 4 and 2 rows), 1 (one thread adds
all 256 rows); 1 and 9 images; with the squeeze-excitation tail (POOL 2: rows published for the image's last workgroup) and without (POOL 1); weights
through LDS (DN_DW_WLDS=2) and per thread (0).

The host rule was validated in one session against the rows of commit c2936d5 (the sequential loop, which is also what this tree runs) and against the
batched loop that was not kept: all 40 cases equal bit for bit on both.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _lib():
    from demonet_amd import _lib as L
    return L, L.lib()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


_PROBLEMS = {}


def _problem(n, h, w, c, k, sq):
    key = (n, h, w, c, k, sq)
    if key not in _PROBLEMS:
        g = torch.Generator().manual_seed(h * 131 + w * 17 + c + k)
        x = (torch.randn(n, h, w, c, generator=g) * torch.exp2(torch.randint(-8, 9, (n, h, w, c), generator=g).float())).half()
        wt = torch.zeros(k * k, c)
        tap = torch.randint(0, k * k, (c,), generator=g)
        val = torch.tensor([1.0, 2.0, 4.0])[torch.randint(0, 3, (c,), generator=g)] * (torch.randint(0, 2, (c,), generator=g) * 2 - 1).float()
        wt[tap, torch.arange(c)] = val
        p = dict(x=x.cuda(), w=wt.half().cuda(), b=torch.zeros(c).cuda())
        if sq:
            p.update(w1t=(torch.randn(c, sq, generator=g) / c ** 0.5).half().cuda(), w2t=(torch.randn(sq, c, generator=g) / sq ** 0.5).half().cuda(),
                     b1=(torch.randn(sq, generator=g) * 0.1).cuda(), b2=(torch.randn(c, generator=g) * 0.1).cuda())
        _PROBLEMS[key] = p
    return _PROBLEMS[key]


def _host_rows(out, blocks, s, reverse=False):
    """out [n][ho][wo][c] fp16 (numpy) -> [n][blocks][c] fp32 by the kernel's rule; reverse: the last loop backwards (the order check of the test's own data)"""
    n, ho, wo, c = out.shape
    c8, tw = c // 8, (4 if s == 1 else 2)
    xsn = (wo + tw - 1) // tw
    idx = np.arange(blocks * 256)
    q1, cg = idx // c8, idx % c8
    oy, xs = q1 // xsn, q1 % xsn
    valid = oy < ho
    o32 = out.astype(np.float32).reshape(n, ho, wo, c8, 8)
    psum = np.zeros((n, blocks * 256, 8), dtype=np.float32)
    for t in range(tw):
        ox = xs * tw + t
        ok = valid & (ox < wo)
        v = np.zeros_like(psum)
        v[:, ok] = o32[:, oy[ok], ox[ok], cg[ok]]
        psum = (psum + v).astype(np.float32)          # (+ 0.0 where the kernel adds nothing: the same number)
    psum = psum.reshape(n, blocks, 256, 8)
    rows = np.zeros((n, blocks, c), dtype=np.float32)
    for bx in range(blocks):
        for tid in range(c8):
            us = list(range(tid, 256, c8))
            acc = np.zeros((n, 8), dtype=np.float32)
            for u in (reversed(us) if reverse else us):
                acc = (acc + psum[:, bx, u]).astype(np.float32)
            cgp = (bx * 256 + tid) % c8
            rows[:, bx, cgp * 8:cgp * 8 + 8] = acc
    return rows


SHAPES = [(10, 10, 120, 5, 1), (13, 9, 72, 5, 2), (6, 6, 672, 5, 1), (4, 4, 1024, 5, 1), (3, 3, 8, 3, 1)]


@pytest.mark.parametrize("wlds", ["0", "2"])
@pytest.mark.parametrize("tail", [False, True], ids=["pool1", "pool2"])
@pytest.mark.parametrize("n", [1, 9])
@pytest.mark.parametrize("h,w,c,k,s", SHAPES)
def test_pooled_rows_equal_the_documented_order(h, w, c, k, s, n, tail, wlds, monkeypatch):
    L, lib = _lib()
    monkeypatch.setenv("DN_DW_WLDS", wlds)
    sq = {120: 32, 72: 24, 672: 168, 1024: 256, 8: 8}[c] if tail else 0
    p = _problem(n, h, w, c, k, sq)
    pad = (k - 1) // 2
    act = 1 if c in (120, 1024) else 0
    ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    out = torch.zeros(n, ho, wo, c, dtype=torch.half, device="cuda")
    blocks = lib.dn_depthwise_pool_blocks(h, w, c, k, s, pad)
    assert blocks > 0
    rows = torch.full((n, blocks, c), float("nan"), device="cuda")
    scale = torch.full((n, c), float("nan"), device="cuda") if tail else None
    counter = torch.zeros(n, dtype=torch.int32, device="cuda") if tail else None
    rc = lib.dn_depthwise_conv_pool(_ptr(p["x"]), _ptr(p["w"]), _ptr(p["b"]), _ptr(out), n, h, w, c, k, s, pad, act, _ptr(rows),
                                    _ptr(p.get("w1t")) if tail else None, _ptr(p.get("b1")) if tail else None, _ptr(p.get("w2t")) if tail else None,
                                    _ptr(p.get("b2")) if tail else None, _ptr(scale), _ptr(counter), sq, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    L.check(rc, "dn_depthwise_conv_pool")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    got = rows.cpu().numpy()
    # the outputs are what the construction says: one tap times its weight (so the accumulators the kernel pooled are these fp16 numbers)
    xp = torch.nn.functional.pad(p["x"].cpu().float().permute(0, 3, 1, 2), (pad, pad, pad, pad))
    ref = torch.nn.functional.conv2d(xp, p["w"].cpu().float().t().reshape(c, 1, k, k), None, s, 0, 1, c)
    ref = (torch.relu(ref) if act else ref).permute(0, 2, 3, 1)
    assert torch.equal(ref.half().float(), ref) and torch.equal(torch.from_numpy(o).float(), ref)
    want = _host_rows(o, blocks, s)
    assert np.isfinite(got).all() and np.array_equal(got.view(np.int32), want.view(np.int32)), "pooled partial rows differ from the documented order"
    if c <= 120 and n == 9:
        assert not np.array_equal(_host_rows(o, blocks, s, reverse=True).view(np.int32), want.view(np.int32))      # the data does tell orders apart
    if tail:
        assert int(counter.abs().sum()) == 0 and bool(torch.isfinite(scale).all())
