"""DN_PW_WSTAT_PROJ (pwdirect.hip pw_wstat_kernel<.., PROJ = true>): the weight-stationary body behind the launches labelled pw_direct_kernel<KSF, 1>
-- the narrow projections (cin <= 128, cout <= 64, hw % 32 == 0) with or without squeeze-excitation scale and residual -- against the register-direct
body (DN_PW_WSTAT_PROJ=0): same K order, same rounding points, so the outputs must be equal bit for bit (int16 view); and against fp32 torch at the
4e-3 of tests/test_gpu_kernels.py. DN_PW_WSTAT_PROJ=2 takes the new body wherever it can run (the default, 1, only from 51 200 rows).

Shapes: (cin, cout) = (72, 40) and (120, 40), the projections of the V3 plan (K % 16 == 8; a second channel tile of 8); (16, 8) and (24, 24): a single
channel tile, one K step with and without a tail; (128, 64): K % 16 == 0, both tiles full, the largest LDS image (68 KB). Images of 32, 64 and 1600 rows,
1 / 3 / 9 of them (nine: XCD groups of two images, the last groups short or empty; also with the grouping off). Each case runs the new body twice:
with the default grid (every wave at most one tile at these sizes; 1 or 3 tiles leave the only workgroup's last waves without work) and with
DN_PW_WSTAT_PROJ_WGS=16 (16 workgroups in all: a wave walks up to 25 tiles of 1600-row images, so tile t + 1 -- x, scale row and residual -- is
requested under tile t, and waves of one workgroup end with different tile counts). The scale rows differ per image, so a tile that took another
image's row would differ from the reference.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from demonet_amd.plan import fragment_major

pytestmark = pytest.mark.gpu


def _lib():
    from demonet_amd import _lib as L
    return L, L.lib()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


_PROBLEMS = {}


def _problem(cin, cout, hw, n):
    """Inputs on the device and the four fp32 pre-activation references (scale x residual is applied per run), made once per shape and left unchanged."""
    key = (cin, cout, hw, n)
    if key not in _PROBLEMS:
        m = n * hw
        g = torch.Generator().manual_seed(m * 31 + cin * 7 + cout)
        x = torch.randn(m, cin, generator=g).half()
        w = (torch.randn(cout, cin, generator=g) / cin ** 0.5).half()
        b = torch.randn(cout, generator=g)
        r = torch.randn(m, cout, generator=g).half()
        s = torch.rand(n, cin, generator=g) + 0.25 * torch.arange(n)[:, None]          # every image its own scale row
        xs = (x.float().view(n, hw, cin) * s[:, None, :]).half().float().view(m, cin)    # the kernels round the scaled input to fp16
        pre = {False: x.float() @ w.float().t() + b, True: xs @ w.float().t() + b}
        _PROBLEMS[key] = dict(x=x.cuda(), w=w.cuda(), wf=torch.from_numpy(fragment_major(w.numpy())).cuda(), b=b.cuda(), r=r.cuda(), s=s.cuda(), rcpu=r.float(), pre=pre)
    return _PROBLEMS[key]


def _run(p, cin, cout, hw, n, act, se, res):
    L, lib = _lib()
    m = n * hw
    out = torch.full((m + 64, cout), -777.0, dtype=torch.half, device="cuda")           # 64 guard rows behind the tensor
    L.check(lib.dn_pointwise_conv(_ptr(p["x"]), _ptr(p["w"]), _ptr(p["wf"]), _ptr(p["b"]), _ptr(p["r"] if res else None), _ptr(p["s"] if se else None), _ptr(out),
                                  m, cin, cout, hw, act, 0, 0, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dn_pointwise_conv")
    torch.cuda.synchronize()
    assert bool((out[m:] == -777.0).all()), "rows behind the tensor were written"
    return out[:m]


def _check(monkeypatch, cin, cout, hw, n, xcd="1"):
    L, _ = _lib()
    m = n * hw
    p = _problem(cin, cout, hw, n)
    monkeypatch.setenv("DN_XCD", xcd)
    monkeypatch.setenv("DN_PW_WSTAT_PROJ", "2")
    for se in (False, True):
        for res in (False, True):
            # the launch keeps its label and parameters; proj tells the bodies apart
            got = L.debug_choice("pw", m, cin, cout, hw, 0, 0, int(se), int(res), 1)
            if cout >= 64 and m >= 3200 and not se and not res:
                # (an expansion-shaped launch: the older rule of pw_choose has taken it for pw_wstat_kernel under either knob value; the runs below then compare that kernel with itself)
                assert (got["kernel"], got["proj"]) == ("pw_wstat_kernel", 0), got
                continue
            assert (got["kernel"], got["k"], got["t"], got["proj"]) == ("pw_direct_kernel", cin // 16, 1, 1), got
    for act in (0, 1):
        for se in (False, True):
            for res in (False, True):
                monkeypatch.setenv("DN_PW_WSTAT_PROJ", "0")
                monkeypatch.delenv("DN_PW_WSTAT_PROJ_WGS", raising=False)
                base = _run(p, cin, cout, hw, n, act, se, res)
                ref = F.relu(p["pre"][se]) if act else p["pre"][se]
                if res:
                    ref = ref + p["rcpu"]
                torch.testing.assert_close(base.cpu().float(), ref.half().float(), rtol=4e-3, atol=4e-3)
                monkeypatch.setenv("DN_PW_WSTAT_PROJ", "2")
                for wgs in (None, "16"):
                    if wgs:
                        monkeypatch.setenv("DN_PW_WSTAT_PROJ_WGS", wgs)
                    got = _run(p, cin, cout, hw, n, act, se, res)
                    assert torch.equal(got.view(torch.int16), base.view(torch.int16)), f"act={act} se={se} res={res} wgs={wgs}: output bits differ"
                    torch.testing.assert_close(got.cpu().float(), ref.half().float(), rtol=4e-3, atol=4e-3)


SHAPES = [(72, 40), (120, 40), (16, 8), (128, 64), (24, 24)]
IMAGES = [(hw, n) for hw in (32, 64, 1600) for n in (1, 3, 9)]


@pytest.mark.parametrize("hw,n", IMAGES)
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_pw_wstat_proj_bit_identical(cin, cout, hw, n, monkeypatch):
    """the four combinations of scale and residual, no activation and ReLU, the default grid and 16 workgroups"""
    _check(monkeypatch, cin, cout, hw, n)


@pytest.mark.parametrize("cin,cout,hw", [(120, 40, 1600), (72, 40, 64), (128, 64, 32)])
def test_pw_wstat_proj_plain_image_mapping(cin, cout, hw, monkeypatch):
    """nine images with DN_XCD=0: one group of rows, workgroups walk all of it"""
    _check(monkeypatch, cin, cout, hw, 9, xcd="0")


def test_default_rule_takes_the_body_from_its_row_threshold(monkeypatch):
    """DN_PW_WSTAT_PROJ=1 (default): from 51 200 rows (choice.h PW_WSTAT_PROJ_MIN_ROWS); never where a tile could straddle two images or the layer is wider"""
    L, _ = _lib()
    monkeypatch.delenv("DN_PW_WSTAT_PROJ", raising=False)
    q = lambda m, cin, cout, hw, se=1, res=1: L.debug_choice("pw", m, cin, cout, hw, 0, 0, se, res, 1)
    assert q(64 * 1600, 120, 40, 1600)["proj"] == 1 and q(32 * 1600, 72, 40, 1600, 1, 0)["proj"] == 1
    assert q(31 * 1600, 120, 40, 1600)["proj"] == 0
    assert q(64 * 1600, 120, 40, 1600, 0, 0)["proj"] == 1
    assert q(64 * 1610, 120, 40, 1610, 0, 0)["proj"] == 0           # hw % 32 != 0
    assert q(64 * 1600, 120, 72, 1600, 0, 1)["proj"] == 0           # three channel tiles
    assert q(64 * 1600, 120, 40, 1600)["kernel"] == "pw_direct_kernel" and q(64 * 1600, 120, 40, 1600)["k"] == 7
    monkeypatch.setenv("DN_PW_WSTAT_PROJ", "0")
    assert q(64 * 1600, 120, 40, 1600)["proj"] == 0


def _heads(monkeypatch, env):
    from demonet_amd import models, synth
    for k in ("DN_PW_WSTAT_PROJ", "DN_POISON", "DN_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    imgs = torch.from_numpy(synth.images(29, 2, 320, 320)).cuda()
    m = models.load_synthetic(models.ssdlite320_mobilenet_v3_large(num_classes=91), 0).cuda()
    return [t.clone() for t in m.forward_heads(imgs)]


def test_model_heads_bit_identical(monkeypatch):
    """ssdlite320_mobilenet_v3_large, two images: every head output equal bit for bit with the knob at 0, at its default, at 2 (where the three
    SE-scaled projections of the 40 x 40 maps take the new body at this batch) and at 2 with NaN patterns left in every LDS byte and vector
    register in front of every launch (DN_POISON=1, plain launches): the body reads nothing it has not written."""
    base = _heads(monkeypatch, {"DN_PW_WSTAT_PROJ": "0"})
    assert all(torch.isfinite(t.float()).all() for t in base) and float(base[0].abs().max()) > 1.0
    for env in ({}, {"DN_PW_WSTAT_PROJ": "2"}, {"DN_PW_WSTAT_PROJ": "2", "DN_POISON": "1", "DN_GRAPH": "0"}):
        other = _heads(monkeypatch, env)
        assert len(other) == len(base) and all(torch.equal(a, b) for a, b in zip(other, base)), env
