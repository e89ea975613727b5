"""CPU-side check of the compiled depthwise launches (no GPU: hipcc cross-compiles): the dw_kernel instantiations that the V3 and V2 plans dispatch
with default knobs have no scratch -- checked for EVERY instantiation of both bodies, so the check does not depend on which launch the channel rule
sends where (the lists below are what the plans dispatch at the time of writing, for the reader).

dw_kernel<K, S, TW, POOL, WLDS>: WLDS = true for launches of at most 128 channels (DN_DW_WLDS=1, depthwise.hip dw_wlds_bytes). Dispatched:
  ssdlite320_mobilenet_v3_large   <5,2,2,2,true> (72 ch, 80 x 80)  <5,1,4,2,true> (120 ch, 40 x 40, twice)  <3,1,4,1,false> (480 / 672 ch, 20 x 20)
                                  <5,2,2,1,false> (672 ch)  <5,1,4,1,false> (480 ch, 10 x 10, twice)
  ssd_lite_mobilenet_v2 (300)     <3,1,4,0,true> (32 ch, 150 x 150)  <3,2,2,0,false> (576 ch)  <3,1,4,0,false> (960 ch, three times)

Figures at the time of writing (ScratchSize, bytes per lane): every instantiation 0 -- <5,1,4,*,true> 108 - 114 registers at four waves per SIMD where
the per-thread form needs 168 at three. (Before the LDS body existed, <3,1,4,1/2> and <5,1,4,1/2> of the per-thread form carried one 4-byte spill: the
strip's first output column held across the row loop at the 128- / 168-register caps; the pooling variants now compute it again behind the loop.)
"""
import re

import pytest

from test_isa_lint import _BUILD_EXTRA, _asm, _kernels

# (K, S, TW, POOL, WLDS): every instantiation of both bodies -- a superset of what any plan dispatches, whatever the channel rule of dw_wlds_bytes sends where
ALL = [(k, s, 4 if s == 1 else 2, pool, wlds) for k in (3, 5) for s in (1, 2) for pool in (0, 1, 2) for wlds in (False, True)]
WLDS_ALL = [i for i in ALL if i[4]]


def _meta_of(meta, inst):
    k, s, tw, pool, wlds = inst
    pat = f"dw_kernelILi{k}ELi{s}ELi{tw}ELi{pool}ELb{int(wlds)}EE"
    hits = [v for name, v in meta.items() if pat in name]
    assert len(hits) == 1, (pat, [n for n in meta if "dw_kernel" in n])
    return hits[0]


def test_every_dw_kernel_instantiation_is_listed(tmp_path):
    text = _asm("depthwise.hip", tmp_path, _BUILD_EXTRA["depthwise.hip"])
    _, meta = _kernels(text)
    assert len([n for n in meta if "dw_kernelILi" in n]) == len(ALL)


@pytest.mark.parametrize("inst", ALL, ids=lambda i: "dw_kernel<%d,%d,%d,%d,%s>" % (i[0], i[1], i[2], i[3], str(i[4]).lower()))
def test_dispatched_dw_kernels_have_no_scratch(inst, tmp_path):
    text = _asm("depthwise.hip", tmp_path, _BUILD_EXTRA["depthwise.hip"])
    _, meta = _kernels(text)
    m = _meta_of(meta, inst)
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", m), "scratch: " + re.search(r"\.amdhsa_private_segment_fixed_size \d+", m).group(0)


def test_lds_body_runs_at_four_waves_per_simd(tmp_path):
    """the 5 x 5 LDS instantiations fit the 128-register budget of four waves per SIMD (the per-thread form: 142 - 168 registers, three waves)"""
    text = _asm("depthwise.hip", tmp_path, _BUILD_EXTRA["depthwise.hip"])
    _, meta = _kernels(text)
    for inst in WLDS_ALL:
        m = _meta_of(meta, inst)
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m).group(1)) <= 128, inst
