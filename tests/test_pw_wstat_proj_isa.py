"""CPU-side check of the compiled code (no GPU: hipcc cross-compiles) of the weight-stationary projection body and the pooling depthwise launches in front of it.

pw_wstat_kernel<KS1, RT, true> (pwdirect.hip; the body behind the launches labelled pw_direct_kernel<KS1 - 1, 1> under DN_PW_WSTAT_PROJ): sixteen
instantiations, KS1 = 2 .. 9 K steps x RT = 1 or 2 channel tiles. Its schedule depends on a counted wait (a tile's 2 RT stores stay in flight behind
the next tile's LDS-DMA): a spill reload would be a vector-memory operation inside that count, so no scratch; and its LDS image ((RT + 4) K steps + 4 x
(1 + residual pieces) KB: 46 KB at 72 -> 40, 64 KB at 120 -> 40) lets two workgroups share a compute unit, i.e. two waves per SIMD: at most 256 registers.
Figures at the time of writing: <5,2,true> 178 registers, <8,2,true> 233, <9,2,true> 253; no scratch anywhere.

dw_kernel<K, S, TW, POOL, WLDS> with POOL != 0 (depthwise.hip): the pooling instantiations keep their register budgets (waves per SIMD) -- the LDS body
128 (four), the per-thread body 128 for 3 x 3 (four) and 168 for 5 x 5 (three) -- and stay without scratch (tests/test_dw_wlds_isa.py holds the latter
for every instantiation). Whatever the reduction behind the row loop becomes (a batched form needed 64 registers there), it must fit these.
"""
import re

import pytest

from test_isa_lint import _BUILD_EXTRA, _asm, _kernels

PROJ = [(ks1, rt) for ks1 in range(2, 10) for rt in (1, 2)]


def _vgprs(m):
    return int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m).group(1))


@pytest.mark.parametrize("ks1,rt", PROJ, ids=lambda v: str(v))
def test_projection_body_has_no_scratch_and_fits_two_waves_per_simd(ks1, rt, tmp_path):
    text = _asm("pwdirect.hip", tmp_path, _BUILD_EXTRA["pwdirect.hip"])
    kernels, meta = _kernels(text)
    pat = f"pw_wstat_kernelILi{ks1}ELi{rt}ELb1EE"
    hits = [n for n in meta if pat in n]
    assert len(hits) == 1, (pat, [n for n in meta if "pw_wstat_kernel" in n])
    m = meta[hits[0]]
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", m), "scratch: " + re.search(r"\.amdhsa_private_segment_fixed_size \d+", m).group(0)
    assert _vgprs(m) <= 256
    body = "\n".join(kernels[hits[0]])
    assert "scratch_" not in body
    assert "global_load_lds_dwordx4" in body
    assert re.search(rf"s_waitcnt vmcnt\({2 * rt}\)", body), f"the counted wait vmcnt({2 * rt}) is missing"
    assert len(re.findall(r"\bv_mfma_f32_32x32x16_f16\b", body)) == ks1 * rt
    assert "v_fma_mixlo_f16" not in body and "v_fma_mixhi_f16" not in body          # the scale is v_mul_f32 + a conversion: pw_direct_kernel's rounding


def test_every_projection_instantiation_is_listed(tmp_path):
    text = _asm("pwdirect.hip", tmp_path, _BUILD_EXTRA["pwdirect.hip"])
    _, meta = _kernels(text)
    assert len([n for n in meta if re.search(r"pw_wstat_kernelILi\dELi\dELb1EE", n)]) == len(PROJ)


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("pool", [1, 2])
@pytest.mark.parametrize("wlds", [False, True])
def test_pooling_depthwise_keeps_its_register_budget(k, s, pool, wlds, tmp_path):
    text = _asm("depthwise.hip", tmp_path, _BUILD_EXTRA["depthwise.hip"])
    _, meta = _kernels(text)
    pat = f"dw_kernelILi{k}ELi{s}ELi{4 if s == 1 else 2}ELi{pool}ELb{int(wlds)}EE"
    hits = [v for n, v in meta.items() if pat in n]
    assert len(hits) == 1, pat
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", hits[0]), pat
    assert _vgprs(hits[0]) <= (128 if (wlds or k == 3) else 168), (pat, _vgprs(hits[0]))
