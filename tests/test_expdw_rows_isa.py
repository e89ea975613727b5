"""Compile-time requirements of the row-reuse body of the fused 24 -> 72 -> cout block (demonet_amd/csrc/expdw_rows.hip), read from the gfx950 assembly of the
file as it is built (cross-compiles without a GPU): no scratch, at most 168 registers (three waves per SIMD: the ring of three expanded rows costs the
fourth), at most the one set-up barrier, and no inline-asm instruction that reads a matrix result inside its hazard window. Helpers: tests/test_isa_lint.py."""
import os
import re
import sys

import test_isa_lint as lint

SRC = "expdw_rows.hip"
EXTRA = ("-mllvm", "-amdgpu-mfma-vgpr-form=1")      # demonet_amd/build.py compiles the file with it
VGPR_BUDGET = 168                                   # 512 registers per SIMD lane / 3 waves, in allocation units of 8


def _rows(tmp_path):
    text = lint._asm(SRC, tmp_path, EXTRA)
    kernels, meta = lint._kernels(text)
    names = [k for k in kernels if "expdw_rows_kernel" in k]
    assert len(names) == 4, list(kernels)             # one instantiation per expand activation
    return text, kernels, meta, names


def test_build_compiles_the_file_with_the_flags_scanned_here():
    sys.path.insert(0, lint.ROOT)
    from demonet_amd import build
    assert SRC in build.SOURCES and tuple(build.EXTRA[SRC]) == EXTRA


def test_no_scratch_and_three_waves_per_simd(tmp_path):
    _, _, meta, names = _rows(tmp_path)
    for name in names:
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", meta[name]), f"{name}: scratch"
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta[name]).group(1))
        assert vgpr <= VGPR_BUDGET, f"{name}: {vgpr} registers"


def test_at_most_the_set_up_barrier(tmp_path):
    _, kernels, _, names = _rows(tmp_path)
    for name in names:
        ops = [lint._operands(l)[0] for l in kernels[name]]
        assert sum(1 for o in ops if o == "s_barrier") <= 1, name


def test_no_inline_asm_reads_a_matrix_result_inside_its_hazard_window(tmp_path):
    sys.path.insert(0, os.path.join(lint.ROOT, "tools"))
    from mfma_hazard_scan import asm_hazards
    text, _, _, _ = _rows(tmp_path)
    assert "v_mfma" in text
    bad = asm_hazards(text)
    assert not bad, f"{len(bad)} inline-asm reads of a matrix result inside its hazard window, first: {bad[0]}"
