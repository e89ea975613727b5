"""What expdw_choose (csrc/choice.h) answers for a fused inverted-residual launch, without a GPU: dn_debug_choice("expdw", ...) is the function
launch_expdw asks, so label=, body=, band= and tile= here are what a launch notes and runs (tests/test_gpu_kernels.py::test_expand_depthwise and the
_run of tests/test_gpu_expdw_direct.py / test_gpu_expdw_rows.py hold the launcher to it on the GPU).

Expected values. The fused blocks of the four zoo models: their labels in tests/golden/plan_signature.json. Every other row: the label that
dn_expand_depthwise's launch noted on an MI355X for that shape and those knobs BEFORE the choice function existed (the template ladder of
launch_expdw), with the body= / band= that dn_debug_choice answered then; tile= is the tile inside the label. Each shape stands under the default
knobs and under each of DN_EXPDW_DIRECT / ROWS / PERSIST / ONE = 0 that changes its answer (ONE=0 with ROWS=0 where the pair says more than either).
Two rows (one case, on two maps) differ from that record on purpose and say so."""
import json
import os
import re

import pytest

from demonet_amd import _lib

KNOBS = ("DIRECT", "ROWS", "PERSIST", "ONE")


def _ask(monkeypatch, query, knobs):
    for k in KNOBS:
        monkeypatch.delenv("DN_EXPDW_" + k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv("DN_EXPDW_" + k, str(v))
    return _lib.debug_choice("expdw", *query)


def _tile(label):
    return "%sx%s" % tuple(re.match(r"expdw(?:_one)?_kernel<\d+,\d+,(\d+),(\d+),", label).groups())


# (n, h, w, cin, cexp, cout [0: no project stage], k, stride, act1 [-1: no expand stage], act2, has_res, pool), knobs (DN_EXPDW_<name>), label, body, band
TABLE = [
    # ---- the shapes of test_expand_depthwise (tests/test_gpu_kernels.py)
    ((2, 36, 44, 16, 64, 0, 3, 2, 1, 1, 0, 0), dict(), 'expdw_kernel<3,2,5,10,2,true,false>', 'tiled', 0),
    ((1, 40, 40, 24, 72, 0, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,8,16,2,true,false>', 'tiled', 0),
    ((2, 40, 40, 24, 72, 0, 5, 2, 1, 1, 0, 1), dict(), 'expdw_kernel<5,2,5,10,2,true,false>', 'tiled', 0),
    ((2, 20, 20, 40, 120, 0, 5, 1, 1, 1, 0, 1), dict(), 'expdw_kernel<5,1,10,10,2,true,false>', 'tiled', 0),
    ((1, 20, 20, 80, 200, 0, 3, 1, 3, 3, 0, 0), dict(), 'expdw_kernel<3,1,10,10,5,true,false>', 'tiled', 0),
    ((2, 20, 20, 112, 672, 0, 3, 1, 3, 3, 0, 1), dict(), 'expdw_kernel<3,1,10,10,8,true,false>', 'tiled', 0),
    ((2, 10, 10, 80, 480, 0, 5, 1, 3, 3, 0, 1), dict(), 'expdw_kernel<5,1,5,10,5,true,false>', 'tiled', 0),
    ((2, 5, 5, 40, 104, 0, 3, 2, 2, 2, 0, 0), dict(), 'expdw_kernel<3,2,5,5,2,true,false>', 'tiled', 0),
    ((2, 19, 19, 64, 384, 0, 3, 1, 2, 2, 0, 0), dict(), 'expdw_kernel<3,1,10,10,8,true,false>', 'tiled', 0),
    ((2, 3, 3, 128, 256, 0, 3, 2, 1, 1, 0, 0), dict(), 'expdw_kernel<3,2,5,5,8,true,false>', 'tiled', 0),
    ((2, 40, 48, 16, 16, 16, 3, 1, -1, 1, 1, 0), dict(), 'expdw_kernel<3,1,8,16,2,false,true>', 'tiled', 0),
    ((2, 36, 44, 16, 64, 24, 3, 2, 1, 1, 0, 0), dict(), 'expdw_kernel<3,2,5,10,2,true,true>', 'direct', 4),
    ((2, 36, 44, 16, 64, 24, 3, 2, 1, 1, 0, 0), dict(DIRECT=0), 'expdw_kernel<3,2,5,10,2,true,true>', 'tiled', 0),
    ((1, 40, 40, 24, 72, 24, 3, 1, 1, 1, 1, 0), dict(), 'expdw_one_kernel<3,1,8,16,2>', 'rows', 5),
    ((1, 40, 40, 24, 72, 24, 3, 1, 1, 1, 1, 0), dict(ROWS=0), 'expdw_one_kernel<3,1,8,16,2>', 'tiled', 0),
    ((1, 40, 40, 24, 72, 24, 3, 1, 1, 1, 1, 0), dict(PERSIST=0), 'expdw_kernel<3,1,8,16,2,true,true>', 'rows', 5),
    ((1, 40, 40, 24, 72, 24, 3, 1, 1, 1, 1, 0), dict(ONE=0, ROWS=0), 'expdw_kernel<3,1,8,16,2,true,true>', 'tiled', 0),
    # THE ONE ROW THAT DIFFERS FROM THE RECORD. With DN_EXPDW_ONE=0 the 72-channel block runs as two chunks on expdw_kernel<3,1,8,16,2,true,true> (the row above),
    # and that is the label the row-reuse body stands behind. The ladder labelled this launch expdw_one_kernel<3,1,8,16,2>: its copy of the persistent
    # form's rule left out that a 72-channel block needs DN_EXPDW_ONE.
    ((1, 40, 40, 24, 72, 24, 3, 1, 1, 1, 1, 0), dict(ONE=0), 'expdw_kernel<3,1,8,16,2,true,true>', 'rows', 5),
    ((2, 38, 38, 32, 96, 40, 3, 1, 2, 2, 0, 0), dict(), 'expdw_kernel<3,1,8,16,2,true,true>', 'tiled', 0),
    # ---- tests/test_gpu_expdw_rows.py: the row-reuse body's shapes, and test_shapes_outside_the_list_take_the_old_body
    ((2, 9, 31, 24, 72, 24, 3, 1, 1, 1, 1, 0), dict(), 'expdw_kernel<3,1,10,10,2,true,true>', 'rows', 5),
    ((2, 9, 31, 24, 72, 24, 3, 1, 1, 1, 1, 0), dict(ROWS=0), 'expdw_kernel<3,1,10,10,2,true,true>', 'tiled', 0),
    ((2, 9, 31, 24, 72, 16, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,10,10,2,true,true>', 'rows', 5),
    ((2, 9, 31, 24, 72, 16, 3, 1, 1, 1, 0, 0), dict(ROWS=0), 'expdw_kernel<3,1,10,10,2,true,true>', 'tiled', 0),
    ((2, 80, 80, 24, 72, 24, 3, 1, 1, 1, 1, 0), dict(), 'expdw_one_kernel<3,1,8,16,2>', 'rows', 5),
    ((2, 80, 80, 24, 72, 24, 3, 1, 1, 1, 1, 0), dict(ROWS=0), 'expdw_one_kernel<3,1,8,16,2>', 'tiled', 0),
    ((2, 80, 80, 24, 72, 24, 3, 1, 1, 1, 1, 0), dict(PERSIST=0), 'expdw_kernel<3,1,8,16,2,true,true>', 'rows', 5),
    ((2, 80, 80, 24, 72, 24, 3, 1, 1, 1, 1, 0), dict(ONE=0, ROWS=0), 'expdw_kernel<3,1,8,16,2,true,true>', 'tiled', 0),
    ((2, 80, 80, 24, 72, 24, 3, 1, 1, 1, 1, 0), dict(ONE=0), 'expdw_kernel<3,1,8,16,2,true,true>', 'rows', 5),      # (differs from the record like the 40 x 40 row above)
    ((2, 9, 31, 24, 72, 24, 3, 2, 1, 1, 0, 0), dict(), 'expdw_kernel<3,2,8,8,2,true,true>', 'tiled', 0),
    ((2, 9, 31, 24, 64, 24, 3, 1, 1, 1, 1, 0), dict(), 'expdw_kernel<3,1,10,10,2,true,true>', 'tiled', 0),
    ((2, 9, 31, 24, 144, 24, 3, 1, 1, 1, 1, 0), dict(), 'expdw_kernel<3,1,10,10,2,true,true>', 'tiled', 0),
    ((2, 9, 31, 16, 72, 16, 3, 1, 1, 1, 1, 0), dict(), 'expdw_kernel<3,1,10,10,2,true,true>', 'tiled', 0),
    ((2, 9, 31, 32, 72, 32, 3, 1, 1, 1, 1, 0), dict(), 'expdw_kernel<3,1,10,10,2,true,true>', 'tiled', 0),
    ((2, 9, 31, 24, 72, 40, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,10,10,2,true,true>', 'tiled', 0),
    ((2, 9, 31, 24, 72, 24, 5, 1, 1, 1, 1, 0), dict(), 'expdw_kernel<5,1,10,10,2,true,true>', 'tiled', 0),
    # ---- tests/test_gpu_expdw_direct.py: the per-tap body's shapes, and test_shapes_outside_the_list_take_the_old_body
    ((2, 35, 43, 16, 64, 24, 3, 2, 1, 1, 0, 0), dict(), 'expdw_kernel<3,2,5,10,2,true,true>', 'direct', 4),
    ((2, 35, 43, 16, 64, 24, 3, 2, 1, 1, 0, 0), dict(DIRECT=0), 'expdw_kernel<3,2,5,10,2,true,true>', 'tiled', 0),
    ((2, 160, 160, 16, 64, 24, 3, 2, 1, 1, 0, 0), dict(), 'expdw_one_kernel<3,2,8,8,2>', 'direct', 4),
    ((2, 160, 160, 16, 64, 24, 3, 2, 1, 1, 0, 0), dict(DIRECT=0), 'expdw_one_kernel<3,2,8,8,2>', 'tiled', 0),
    ((2, 160, 160, 16, 64, 24, 3, 2, 1, 1, 0, 0), dict(PERSIST=0), 'expdw_kernel<3,2,8,8,2,true,true>', 'direct', 4),
    ((1, 8, 8, 16, 64, 24, 3, 2, 1, 1, 0, 0), dict(), 'expdw_kernel<3,2,5,5,2,true,true>', 'direct', 4),
    ((1, 8, 8, 16, 64, 24, 3, 2, 1, 1, 0, 0), dict(DIRECT=0), 'expdw_kernel<3,2,5,5,2,true,true>', 'tiled', 0),
    ((2, 36, 44, 24, 64, 24, 3, 2, 1, 1, 0, 0), dict(), 'expdw_kernel<3,2,5,10,2,true,true>', 'tiled', 0),
    ((2, 36, 44, 16, 64, 16, 3, 1, 1, 1, 1, 0), dict(), 'expdw_one_kernel<3,1,8,16,2>', 'tiled', 0),
    ((2, 36, 44, 16, 64, 16, 3, 1, 1, 1, 1, 0), dict(PERSIST=0), 'expdw_kernel<3,1,8,16,2,true,true>', 'tiled', 0),
    ((2, 36, 44, 16, 64, 40, 3, 2, 1, 1, 0, 0), dict(), 'expdw_kernel<3,2,5,10,2,true,true>', 'tiled', 0),
    ((2, 36, 44, 16, 128, 24, 3, 2, 1, 1, 0, 0), dict(), 'expdw_kernel<3,2,5,10,2,true,true>', 'tiled', 0),
    ((1, 4, 700, 16, 64, 24, 3, 2, 1, 1, 0, 0), dict(), 'expdw_one_kernel<3,2,8,8,2>', 'tiled', 0),
    ((1, 4, 700, 16, 64, 24, 3, 2, 1, 1, 0, 0), dict(PERSIST=0), 'expdw_kernel<3,2,8,8,2,true,true>', 'tiled', 0),
    # ---- one shape per rung of the expand's K steps and X row width, with a project stage (cin 16, 32, 40: 24, 40, 56 halfs per row; 64: five
    # steps; 80: 88 halfs; 88: five steps; 96: 104 halfs; 112: all eight) ...
    ((1, 16, 16, 16, 128, 24, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,8,16,2,true,true>', 'tiled', 0),
    ((1, 16, 16, 32, 128, 24, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,8,16,2,true,true>', 'tiled', 0),
    ((1, 16, 16, 40, 128, 24, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,8,16,2,true,true>', 'tiled', 0),
    ((1, 16, 16, 64, 128, 24, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,8,16,5,true,true>', 'tiled', 0),
    ((1, 16, 16, 80, 128, 24, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,8,16,5,true,true>', 'tiled', 0),
    ((1, 16, 16, 88, 128, 24, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,8,16,5,true,true>', 'tiled', 0),
    ((1, 16, 16, 96, 128, 24, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,8,16,6,true,true>', 'tiled', 0),
    ((1, 16, 16, 112, 128, 24, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,8,16,8,true,true>', 'tiled', 0),
    # ... and without one (no five-step rung but for 88 halfs, no six-step rung)
    ((1, 16, 16, 8, 128, 0, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,8,16,2,true,false>', 'tiled', 0),
    ((1, 16, 16, 32, 128, 0, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,8,16,2,true,false>', 'tiled', 0),
    ((1, 16, 16, 40, 128, 0, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,8,16,2,true,false>', 'tiled', 0),
    ((1, 16, 16, 64, 128, 0, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,8,16,8,true,false>', 'tiled', 0),
    ((1, 16, 16, 80, 128, 0, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,8,16,5,true,false>', 'tiled', 0),
    ((1, 16, 16, 96, 128, 0, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,8,16,8,true,false>', 'tiled', 0),
    ((1, 16, 16, 128, 128, 0, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,8,16,8,true,false>', 'tiled', 0),
    # ---- 20 x 20 maps: 10 x 10 tiles while the project stage's (pixel tile x channel tile) units fit the 8 waves (cout 64: 4 x 2), 5 x 10 beyond
    # (cout 80: 4 x 3 -> 2 x 3); stride 2: 5 x 10
    ((1, 20, 20, 80, 200, 64, 3, 1, 3, 3, 0, 0), dict(), 'expdw_kernel<3,1,10,10,5,true,true>', 'tiled', 0),
    ((1, 20, 20, 80, 200, 80, 3, 1, 3, 3, 1, 0), dict(), 'expdw_kernel<3,1,5,10,5,true,true>', 'tiled', 0),
    ((1, 40, 40, 40, 240, 80, 3, 2, 3, 3, 0, 0), dict(), 'expdw_kernel<3,2,5,10,2,true,true>', 'tiled', 0),
    # ---- 5 x 5, 5 x 10 and 10 x 10 maps
    ((1, 5, 5, 80, 200, 80, 3, 1, 3, 3, 1, 0), dict(), 'expdw_kernel<3,1,5,5,5,true,true>', 'tiled', 0),
    ((1, 5, 10, 80, 200, 80, 3, 1, 3, 3, 1, 0), dict(), 'expdw_kernel<3,1,5,10,5,true,true>', 'tiled', 0),
    ((1, 10, 10, 80, 200, 80, 5, 1, 3, 3, 1, 0), dict(), 'expdw_kernel<5,1,5,10,5,true,true>', 'tiled', 0),
    ((1, 10, 10, 16, 64, 24, 3, 2, 1, 1, 0, 0), dict(), 'expdw_kernel<3,2,5,5,2,true,true>', 'direct', 4),
    ((1, 10, 10, 16, 64, 24, 3, 2, 1, 1, 0, 0), dict(DIRECT=0), 'expdw_kernel<3,2,5,5,2,true,true>', 'tiled', 0),
    ((1, 10, 10, 24, 72, 24, 3, 1, 1, 1, 1, 0), dict(), 'expdw_kernel<3,1,5,10,2,true,true>', 'rows', 5),
    ((1, 10, 10, 24, 72, 24, 3, 1, 1, 1, 1, 0), dict(ROWS=0), 'expdw_kernel<3,1,5,10,2,true,true>', 'tiled', 0),
    # ---- the single-chunk full blocks the two other bodies refuse: the persistent form on the 8 x 16 tiles while the tile's output buffer fits the
    # 80 KB (cout 56), one workgroup per tile beyond (cout 64), on other tiles, for 5 x 5 kernels and for 56-half rows (cin 40)
    ((2, 38, 38, 32, 64, 32, 3, 1, 2, 2, 1, 0), dict(), 'expdw_one_kernel<3,1,8,16,2>', 'tiled', 0),
    ((2, 38, 38, 32, 64, 32, 3, 1, 2, 2, 1, 0), dict(PERSIST=0), 'expdw_kernel<3,1,8,16,2,true,true>', 'tiled', 0),
    ((2, 36, 44, 16, 72, 24, 3, 2, 1, 1, 0, 0), dict(), 'expdw_kernel<3,2,5,10,2,true,true>', 'tiled', 0),
    ((2, 36, 44, 40, 64, 24, 3, 2, 1, 1, 0, 0), dict(), 'expdw_kernel<3,2,5,10,2,true,true>', 'tiled', 0),
    ((2, 36, 44, 40, 72, 24, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,8,16,2,true,true>', 'tiled', 0),
    ((2, 36, 44, 16, 64, 24, 5, 2, 1, 1, 0, 0), dict(), 'expdw_kernel<5,2,5,10,2,true,true>', 'tiled', 0),
    ((2, 36, 44, 16, 64, 48, 3, 2, 1, 1, 0, 0), dict(), 'expdw_kernel<3,2,5,10,2,true,true>', 'tiled', 0),
    ((2, 36, 44, 16, 64, 56, 3, 2, 1, 1, 0, 0), dict(), 'expdw_kernel<3,2,5,10,2,true,true>', 'tiled', 0),
    ((2, 40, 40, 32, 64, 56, 3, 1, 1, 1, 0, 0), dict(), 'expdw_one_kernel<3,1,8,16,2>', 'tiled', 0),
    ((2, 40, 40, 32, 64, 56, 3, 1, 1, 1, 0, 0), dict(PERSIST=0), 'expdw_kernel<3,1,8,16,2,true,true>', 'tiled', 0),
    ((2, 40, 40, 32, 64, 64, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,8,16,2,true,true>', 'tiled', 0),
    ((2, 40, 40, 16, 32, 16, 3, 1, 1, 1, 1, 0), dict(), 'expdw_one_kernel<3,1,8,16,2>', 'tiled', 0),
    ((2, 40, 40, 16, 32, 16, 3, 1, 1, 1, 1, 0), dict(PERSIST=0), 'expdw_kernel<3,1,8,16,2,true,true>', 'tiled', 0),
    # ---- the same on the 8 x 8 tiles of stride 2: 16 -> 72 (the wide variant; DN_EXPDW_ONE=0: two chunks, so not persistent either), cin 40, 5 x 5,
    # cout 40 / 48 inside the 80 KB and 56 beyond, cin 24, two chunks, pooled sums without a project stage; cin 40 -> 72 at stride 1
    ((2, 64, 64, 16, 72, 24, 3, 2, 1, 1, 0, 0), dict(), 'expdw_one_kernel<3,2,8,8,2>', 'tiled', 0),
    ((2, 64, 64, 16, 72, 24, 3, 2, 1, 1, 0, 0), dict(PERSIST=0), 'expdw_kernel<3,2,8,8,2,true,true>', 'tiled', 0),
    ((2, 64, 64, 16, 72, 24, 3, 2, 1, 1, 0, 0), dict(ONE=0), 'expdw_kernel<3,2,8,8,2,true,true>', 'tiled', 0),
    ((2, 64, 64, 40, 64, 24, 3, 2, 1, 1, 0, 0), dict(), 'expdw_kernel<3,2,8,8,2,true,true>', 'tiled', 0),
    ((2, 64, 64, 16, 64, 24, 5, 2, 1, 1, 0, 0), dict(), 'expdw_kernel<5,2,8,8,2,true,true>', 'tiled', 0),
    ((2, 64, 64, 16, 64, 40, 3, 2, 1, 1, 0, 0), dict(), 'expdw_one_kernel<3,2,8,8,2>', 'tiled', 0),
    ((2, 64, 64, 16, 64, 40, 3, 2, 1, 1, 0, 0), dict(PERSIST=0), 'expdw_kernel<3,2,8,8,2,true,true>', 'tiled', 0),
    ((2, 64, 64, 16, 64, 48, 3, 2, 1, 1, 0, 0), dict(), 'expdw_one_kernel<3,2,8,8,2>', 'tiled', 0),
    ((2, 64, 64, 16, 64, 48, 3, 2, 1, 1, 0, 0), dict(PERSIST=0), 'expdw_kernel<3,2,8,8,2,true,true>', 'tiled', 0),
    ((2, 64, 64, 16, 64, 56, 3, 2, 1, 1, 0, 0), dict(), 'expdw_kernel<3,2,8,8,2,true,true>', 'tiled', 0),
    ((2, 64, 64, 24, 64, 24, 3, 2, 1, 1, 0, 0), dict(), 'expdw_kernel<3,2,8,8,2,true,true>', 'tiled', 0),
    ((2, 64, 64, 16, 128, 24, 3, 2, 1, 1, 0, 0), dict(), 'expdw_kernel<3,2,8,8,2,true,true>', 'tiled', 0),
    ((2, 64, 64, 16, 64, 0, 3, 2, 1, 1, 0, 1), dict(), 'expdw_kernel<3,2,8,8,2,true,false>', 'tiled', 0),
    ((2, 64, 64, 40, 72, 24, 3, 1, 1, 1, 0, 0), dict(), 'expdw_kernel<3,1,8,16,2,true,true>', 'tiled', 0),
]


def _id(row):
    query, knobs = row[0], row[1]
    return "-".join(str(v) for v in query) + "".join("-%s%d" % kv for kv in sorted(knobs.items()))


@pytest.mark.parametrize("query,knobs,label,body,band", TABLE, ids=[_id(r) for r in TABLE])
def test_choice_of_a_shape(query, knobs, label, body, band, monkeypatch):
    got = _ask(monkeypatch, query, knobs)
    assert got == dict(label=label, body=body, band=band, tile=_tile(label)), (query, knobs)


def test_the_table_has_no_duplicate_rows():
    keys = [(r[0], tuple(sorted(r[1].items()))) for r in TABLE]
    assert len(set(keys)) == len(keys)


# ---- the zoo: every fused block of the factory models, from the graph (shape) and the golden plan signature (label), at both batch sizes of the golden
def _zoo_blocks():
    from demonet_amd import models
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_signature.json")))
    blocks = []
    for name in ("ssdlite320_mobilenet_v3_large", "ssd_lite_mobilenet_v2", "ssd300_vgg16", "ssd512_vgg16"):
        g = getattr(models, name)(num_classes=91).graph
        for n, ops in sorted(golden[name]["ops"].items()):
            i = 0
            while i < len(ops):
                label, owner = ops[i]
                if not label.startswith("expdw"):
                    i += 1
                    continue
                nodes = [g.nodes[j] for j in range(len(ops)) if ops[j][1] == owner and ops[j][0] == label]
                i += len(nodes)
                dwi = [j for j, nd in enumerate(nodes) if nd.op == "dw"]
                assert len(dwi) == 1 and all(nd.op == "pw" for j, nd in enumerate(nodes) if j != dwi[0]), (name, owner)
                d = nodes[dwi[0]]
                e = nodes[0] if dwi[0] == 1 else None
                pj = nodes[-1] if dwi[0] == len(nodes) - 2 else None
                assert d.pad == (d.k - 1) // 2
                tin = g.tensors[nodes[0].inp]
                query = (int(n), tin.h, tin.w, tin.c, d.cin, pj.cout if pj else 0, d.k, d.stride, e.act if e else -1, d.act, int(bool(pj) and pj.residual >= 0), int(d.pool >= 0))
                blocks.append(pytest.param(query, label, id="%s-n%s-op%d" % (name, n, owner)))
    return blocks


ZOO = _zoo_blocks()
# the two blocks that take another body by default (DN_EXPDW_DIRECT, DN_EXPDW_ROWS): (cin, cexp, cout, k, stride, has_res) -> body, band
ZOO_OTHER_BODIES = {(16, 64, 24, 3, 2, 0): ("direct", 4), (24, 72, 24, 3, 1, 1): ("rows", 5)}


def test_the_zoo_has_fused_blocks():
    assert len(ZOO) == 2 * (6 + 12)         # MobileNetV3: 6 fused blocks, MobileNetV2: 12, the VGG models: none; at n = 16 and n = 64


@pytest.mark.parametrize("query,label", ZOO)
def test_choice_of_a_zoo_block(query, label, monkeypatch):
    n, h, w, cin, cexp, cout, k, s, act1, act2, res, pool = query
    body, band = ZOO_OTHER_BODIES.get((cin, cexp, cout, k, s, res), ("tiled", 0))
    assert _ask(monkeypatch, query, {}) == dict(label=label, body=body, band=band, tile=_tile(label)), query
    # neither of the two other bodies shows in the label
    assert _ask(monkeypatch, query, dict(DIRECT=0, ROWS=0)) == dict(label=label, body="tiled", band=0, tile=_tile(label)), query
