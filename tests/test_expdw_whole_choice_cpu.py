"""The whole-width flag of the tiled fused-block body (expdw_choose, csrc/choice.h section (h); the kernel is csrc/expdw_whole.hip), without a GPU:
dn_debug_choice("expdw_whole", ...) answers whole= and lds= for the twelve numbers of the "expdw" query, and the "expdw" query itself (label, body,
band, tile) does not know the flag. DN_EXPDW_WHOLE: 1 (default) = the two expanded widths of the 20 x 20 blocks of MobileNetV3 (measured faster), 0 =
never, 2 = wherever the form can run: 3x3 stride 1 on the 5 x 10 tile, cin 80, a project stage, no pooled sums, an LDS of at most 80 KB."""
import pytest

from demonet_amd import _lib

HSWISH = 3


def _lds(cexp):
    """expdw_whole_lds: D[64][round16(cexp) + 8] over X [96][88] + 8, E[96][cexp or cexp + 8], nine weight rows (halfs); depthwise bias and 256 project biases (floats)"""
    front = max(96 * 88 + 8, 64 * ((cexp + 15) // 16 * 16 + 8))
    erow = cexp if (cexp // 8) % 2 else cexp + 8       # an odd number of 16-byte pieces per E row
    return (front + 96 * erow + 9 * cexp) * 2 + (cexp + 256) * 4


def _ask(monkeypatch, family, query, knob):
    for k in ("DIRECT", "ROWS", "PERSIST", "ONE", "WHOLE"):
        monkeypatch.delenv("DN_EXPDW_" + k, raising=False)
    if knob is not None:
        monkeypatch.setenv("DN_EXPDW_WHOLE", str(knob))
    return _lib.debug_choice(family, *query)


def _block(n, cexp, **kw):
    d = dict(n=n, h=20, w=20, cin=80, cexp=cexp, cout=80, k=3, s=1, act1=HSWISH, act2=HSWISH, res=1, pool=0)
    d.update(kw)
    return (d["n"], d["h"], d["w"], d["cin"], d["cexp"], d["cout"], d["k"], d["s"], d["act1"], d["act2"], d["res"], d["pool"])


def test_the_lds_of_the_zoo_blocks_keeps_two_workgroups_per_cu():
    assert _lds(200) == 71472 and _lds(184) == 66000 and _lds(224) <= 80 * 1024 < _lds(232)


# ops 24 - 26 (80 -> 200 -> 80) and 27 - 29, 30 - 32 (80 -> 184 -> 80) of the V3 plan, at both batch sizes of the golden plan signature
@pytest.mark.parametrize("n", [16, 64])
@pytest.mark.parametrize("op,cexp", [(24, 200), (27, 184), (30, 184)])
def test_the_zoo_blocks_take_the_form_by_default(n, op, cexp, monkeypatch):
    q = _block(n, cexp)
    label = dict(label="expdw_kernel<3,1,5,10,5,true,true>", body="tiled", band=0, tile="5x10")
    for knob, whole in ((None, 1), (1, 1), (2, 1), (0, 0)):
        assert _ask(monkeypatch, "expdw_whole", q, knob) == dict(whole=whole, lds=_lds(cexp) if whole else 0), (q, knob)
        assert _ask(monkeypatch, "expdw", q, knob) == label, (q, knob)


@pytest.mark.parametrize("cexp", [48, 72, 128, 136, 192, 224])
def test_other_widths_take_it_only_on_request(cexp, monkeypatch):
    q = _block(64, cexp)
    assert _ask(monkeypatch, "expdw_whole", q, None) == dict(whole=0, lds=0)
    assert _ask(monkeypatch, "expdw_whole", q, 2) == dict(whole=1, lds=_lds(cexp))
    assert _ask(monkeypatch, "expdw", q, 2) == _ask(monkeypatch, "expdw", q, 0)


REFUSED = [
    ("stride 2", _block(64, 200, s=2, res=0), "expdw_kernel<3,2,5,10,5,true,true>"),
    ("the stride-2 block in front of them", _block(64, 240, h=40, w=40, cin=40, s=2, res=0), "expdw_kernel<3,2,5,10,2,true,true>"),
    ("5x5 kernel", _block(64, 200, k=5), "expdw_kernel<5,1,5,10,5,true,true>"),
    ("no project stage", _block(64, 200, cout=0, res=0), "expdw_kernel<3,1,10,10,5,true,false>"),
    ("pooled sums", _block(64, 200, cout=0, res=0, pool=1), "expdw_kernel<3,1,10,10,5,true,false>"),
    ("232 channels: 80.5 KB", _block(64, 232), "expdw_kernel<3,1,5,10,5,true,true>"),
    ("480 channels", _block(64, 480), "expdw_kernel<3,1,5,10,5,true,true>"),
    ("the 10 x 10 tile", _block(64, 200, cout=64, res=0), "expdw_kernel<3,1,10,10,5,true,true>"),
    ("the 5 x 5 tile", _block(64, 200, h=5, w=5), "expdw_kernel<3,1,5,5,5,true,true>"),
    ("cin 72", _block(64, 200, cin=72, cout=72), "expdw_kernel<3,1,5,10,5,true,true>"),
    ("cin 64 (and with cout 64 the 10 x 10 tile)", _block(64, 200, cin=64, cout=64), "expdw_kernel<3,1,10,10,5,true,true>"),
    ("40 channels: the staged output tile does not fit the dead E rows", _block(64, 40), "expdw_kernel<3,1,5,10,5,true,true>"),
    ("cin 96", _block(64, 200, cin=96, cout=96), "expdw_kernel<3,1,5,10,6,true,true>"),
    ("no expand stage", _block(64, 80, act1=-1), "expdw_kernel<3,1,5,10,2,false,true>"),
]


@pytest.mark.parametrize("name,query,label", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_shapes(name, query, label, monkeypatch):
    for knob in (None, 2):
        assert _ask(monkeypatch, "expdw_whole", query, knob) == dict(whole=0, lds=0), (name, knob)
        got = _ask(monkeypatch, "expdw", query, knob)
        assert got["label"] == label and got["body"] == "tiled" and got == _ask(monkeypatch, "expdw", query, 0), (name, knob, got)
