"""CPU-side check of the compiled whole-width fused-block kernel (no GPU: hipcc cross-compiles; csrc/expdw_whole.hip built with the flags of
demonet_amd/build.py): its three instantiations have no scratch and fit the 128-register budget of four waves per SIMD (two 512-thread workgroups per
CU: the launch of the 20 x 20 blocks must stay one residency round), and they carry the four barriers of the four phases -- the multi-chunk
instantiations of the chunk loop they stand in for spill 12 - 36 B per lane.

Figures at the time of writing: 97 vector registers for <200> and <184>, 112 for <0>, ScratchSize 0."""
import re

import pytest

from demonet_amd import build as B

from test_isa_lint import _asm, _kernels


# expdw_whole_kernel<CEXP>: the two widths of the zoo as compile-time constants, 0 = the launch's width
INSTANCES = [200, 184, 0]


def _whole(tmp_path, cexp):
    text = _asm("expdw_whole.hip", tmp_path, tuple(B.EXTRA["expdw_whole.hip"]))
    kernels, meta = _kernels(text)
    assert len([k for k in meta if "expdw_whole_kernel" in k]) == len(INSTANCES), list(meta)
    names = [k for k in meta if "expdw_whole_kernelILi%dEE" % cexp in k]
    assert len(names) == 1, list(meta)
    return kernels[names[0]], meta[names[0]]


@pytest.mark.parametrize("cexp", INSTANCES)
def test_whole_kernel_has_no_scratch(cexp, tmp_path):
    _, m = _whole(tmp_path, cexp)
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", m), "scratch: " + re.search(r"\.amdhsa_private_segment_fixed_size \d+", m).group(0)
    assert not re.search(r"\.amdhsa_uses_dynamic_stack 1\b", m)


@pytest.mark.parametrize("cexp", INSTANCES)
def test_whole_kernel_runs_at_four_waves_per_simd(cexp, tmp_path):
    _, m = _whole(tmp_path, cexp)
    assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m).group(1)) <= 128


@pytest.mark.parametrize("cexp", INSTANCES)
def test_whole_kernel_has_one_barrier_per_phase(cexp, tmp_path):
    lines, _ = _whole(tmp_path, cexp)
    ops = [ln.split(";")[0].split() for ln in lines]
    ops = [o[0] for o in ops if o]
    assert ops.count("s_barrier") == 4
    # three row tiles x six K steps of the expand; the K steps of the projection: ceil(cexp / 16), all fourteen behind tests for the runtime width
    assert sum(o.startswith("v_mfma_f32_32x32x16_f16") for o in ops) == 3 * 6 + ((cexp + 15) // 16 if cexp else 14)
