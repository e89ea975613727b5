"""Every 32-bit addressing guard of the kernel-choice functions at its edge, on both sides, without a GPU.

dn_debug_choice (include/demonet_hip_debug.h) answers for a shape what pw_choose / conv_choose / pw_group_choose / stem_choose, the depthwise
launcher's range tests and head_fused_level_supported decide. For every guard: the last shape inside the limit and the first shape outside give
the two outcomes the inventory states, and the limit sits where the kernel's arithmetic needs it -- the size of the array the kernel addresses with
32-bit arithmetic (in the unit the kernel counts in: bytes, elements, or images of a grid axis), computed HERE from the inventory's formula and not
from the guard, is representable in the kernel's type at the inside shape and, times the slack the inventory records for the guard (1: the guard
is tight; 2: it keeps one power of two in hand), is not at the outside shape. A guard moved by a factor of two in either direction flips one of
the two outcomes."""
import pytest

from demonet_amd import _lib

I32, U32, GRID_YZ = 2 ** 31 - 1, 2 ** 32 - 1, 65535


def pw(m, cin, cout, wfrag=0, act=0, fp32=0):
    return ("pw", m, cin, cout, m, act, fp32, 0, 0, wfrag)


def conv(n, h, w, cin, cout, k=3, stride=1, pad=1, use=0, cout_b=0, act=1):
    return ("conv", n, h, w, cin, cout, k, stride, pad, 1, act, 1, use, cout_b)


def stem(h, w, cout, stride, act, split_ok):
    return ("stem", 1, h, w, cout, stride, 1, act, split_ok)


def dw(h, w=16, c=8, n=1):
    return ("dw", n, h, w, c, 3, 1, 1)


def headfuse(n, hw, c):
    return ("headfuse", n, hw, hw, c, 546, 24, 3234 * 91, 3234 * 4)


# id, (inside query, expected), (outside query, expected), size(query) in the kernel's unit, the type's largest value, slack
GUARDS = [
    # choice.h pw_tile: x is read at 32-bit byte offsets (row * K + chunk) * 2 + 2 k0 in the bound-test-free K loop: x bytes = m cin 2
    ("fk_rows", (pw(1597830, 672, 32), dict(kernel="pw_kernel", tile="128x32", pf=4, fk=1)), (pw(1597831, 672, 32), dict(kernel="pw_kernel", tile="128x32", pf=4, fk=0)),
     lambda q: q[1] * q[2] * 2, I32, 1),
    # ... and the weights the same way: cout cin 2 bytes (a weight array of 2 GB: no GPU case)
    ("fk_weights", (pw(64, 8659200, 124), dict(kernel="pw_kernel", fk=1)), (pw(64, 8659232, 124), dict(kernel="pw_kernel", fk=0)), lambda q: q[3] * q[2] * 2, I32, 1),
    # choice.h pw_group_choose: the same loop in the grouped head launch
    ("fk_group_rows", (("pw_group", 0, 1, 1597830, 672, 546, 400), dict(kernel="pw_group_kernel", fk=1)), (("pw_group", 0, 1, 1597831, 672, 546, 400), dict(kernel="pw_group_kernel", fk=0)),
     lambda q: q[3] * q[4] * 2, I32, 1),
    # choice.h pw_wstat_supported: the output is a raw buffer of (int)(m cout 2) bytes, a masked store carries the offset 0x80000000
    ("wstat_out", (pw(2 ** 24 - 1, 16, 64, wfrag=1, act=1), dict(kernel="pw_wstat_kernel", k=2, t=2)), (pw(2 ** 24, 16, 64, wfrag=1, act=1), dict(kernel="pw_direct_kernel", k=1, t=1)),
     lambda q: q[1] * q[3] * 2, I32, 1),
    # choice.h patch_shape: conv_patch_kernel has the image on grid.z
    ("patch_images", (conv(65535, 4, 4, 64, 64), dict(kernel="conv_patch_resident_kernel")), (conv(65536, 4, 4, 64, 64), dict(kernel="pw_kernel", tile="128x64", conv=1)),
     lambda q: q[1], GRID_YZ, 1),
    # choice.h patch_resident_shape: the output is a raw buffer of n h w cout 2 bytes, a masked store carries the offset 0xFFFFFFF0
    ("resident_out", (conv(8191, 64, 64, 64, 64), dict(kernel="conv_patch_resident_kernel")), (conv(8192, 64, 64, 64, 64), dict(kernel="conv_patch_kernel")),
     lambda q: q[1] * q[2] * q[3] * q[5] * 2, 0xFFFFFFF0 - 1, 1),
    # ... and a patch pixel is read at the int byte offset (iy W + ix) 128 + chunk 16 inside its image: h w 128 bytes
    ("resident_image", (conv(1, 4095, 4096, 64, 64), dict(kernel="conv_patch_resident_kernel")), (conv(1, 4096, 4096, 64, 64), dict(kernel="conv_patch_kernel")),
     lambda q: q[2] * q[3] * 128, I32, 1),
    # choice.h halo_shape: the input is a raw buffer of (int)(m cin 2) bytes; rows in front of the tensor wrap to offsets beyond it
    ("halo_in", (conv(32767, 16, 16, 128, 128), dict(kernel="conv_halo_kernel", halo=2, head=0)), (conv(32768, 16, 16, 128, 128), dict(kernel="conv_patch_kernel")),
     lambda q: q[1] * q[2] * q[3] * q[4] * 2, I32, 1),
    # ... the head form of the same kernel: beyond the limit the level goes to the group launch (conv_choose answers "none")
    ("halo_head_in", (conv(32767, 16, 16, 128, 324, use=2, cout_b=24, act=0), dict(kernel="conv_halo_kernel", halo=2, head=1)),
     (conv(32768, 16, 16, 128, 324, use=2, cout_b=24, act=0), dict(kernel="none")), lambda q: q[1] * q[2] * q[3] * q[4] * 2, I32, 1),
    # ... its weights at unsigned byte offsets row 9 cin 2 (a weight array of 4 GB: no GPU case)
    ("halo_weights", (conv(1, 16, 16, 16384, 14336), dict(kernel="conv_halo_kernel", halo=1)), (conv(1, 16, 16, 16384, 14592), dict(kernel="pw_kernel", conv=1)),
     lambda q: q[5] * 9 * q[4] * 2, U32, 1),
    # choice.h conv_glds_shape: an input pixel at the int byte offset (((img H + iy) W + ix) cin + chunk 8) 2
    ("glds_in", (conv(131071, 8, 8, 128, 256, k=1, pad=0), dict(kernel="conv_glds_kernel")), (conv(131072, 8, 8, 128, 256, k=1, pad=0), dict(kernel="pw_direct_kernel", k=8, t=1)),
     lambda q: q[1] * q[2] * q[3] * q[4] * 2, I32, 1),
    # ... its weights at unsigned byte offsets (a weight array of 4 GB: no GPU case); 3 x 3 stride 2, which the run-staged tile does not take
    ("glds_weights", (conv(1, 16, 16, 16384, 14336, stride=2), dict(kernel="conv_glds_kernel")), (conv(1, 16, 16, 16384, 14592, stride=2), dict(kernel="pw_kernel", conv=1)),
     lambda q: q[5] * 9 * q[4] * 2, U32, 1),
    # launch_conv_pool asks conv_choose about ONE image: the batch does not move the choice (the launcher walks it in image ranges)
    ("pool_batch", (conv(255, 128, 128, 256, 256, use=1), dict(kernel="conv_halo_kernel", halo=1, pool=1)), (conv(257, 128, 128, 256, 256, use=1), dict(kernel="conv_halo_kernel", halo=1, pool=1)),
     None, None, None),
    # choice.h stem_choose, split-operand stem: the image is a raw buffer of 3 h w 4 bytes read at int byte offsets, a masked load carries 0x80000000
    ("stem_split_in", (stem(10922, 8192, 16, 2, 3, 1), dict(kernel="stem_split_kernel")), (stem(10923, 8192, 16, 2, 3, 1), dict(kernel="stem3s2_kernel")),
     lambda q: 3 * q[2] * q[3] * 4, I32, 2),
    # ... its output a raw buffer of ho wo cout 2 bytes
    ("stem_split_out", (stem(2047, 4096, 64, 1, 1, 1), dict(kernel="stem_split_kernel")), (stem(2048, 4096, 64, 1, 1, 1), dict(kernel="stem_mfma64p_kernel")),
     lambda q: q[2] * q[3] * q[4] * 2, I32, 2),
    # fp32 matrix-core stem: a tap at the int ELEMENT offset c h w + ...: 3 h w floats
    ("stem_mfma_in", (stem(21845, 16384, 64, 1, 1, 0), dict(kernel="stem_mfma64_kernel")), (stem(21846, 16384, 64, 1, 1, 0), dict(kernel="stem_kernel")),
     lambda q: 3 * q[2] * q[3], I32, 2),
    # ... pipelined form: the output is a raw buffer of (int)(h w 128) bytes
    ("stem_pipe_out", (stem(4095, 4096, 64, 1, 1, 0), dict(kernel="stem_mfma64p_kernel")), (stem(4096, 4096, 64, 1, 1, 0), dict(kernel="stem_mfma64_kernel")),
     lambda q: q[2] * q[3] * 128, I32, 1),
    # depthwise.hip dw_fill: a row of an image at the int element offset iy w c
    ("dw_image", (dw(2 ** 24 - 1), dict(kernel="dw_kernel<3,1,4>", range=1, wlds=0)), (dw(2 ** 24), dict(kernel="dw_kernel<3,1,4>", range=0)), lambda q: q[2] * q[3] * q[4], I32, 1),
    # depthwise.hip dw_wlds_bytes: the image as a raw buffer of (int)(h w c 2) bytes, a padding tap carries the offset 0x80000000
    ("dw_wlds_image", (dw(2 ** 23 - 1), dict(kernel="dw_kernel<3,1,4>", range=1, wlds=3 * 3 * 8 * 2 + 8 * 4)), (dw(2 ** 23), dict(kernel="dw_kernel<3,1,4>", range=1, wlds=0)),
     lambda q: q[2] * q[3] * q[4] * 2, I32, 1),
    # headfuse.hip head_fused_level_supported: x at unsigned byte offsets (row C + chunk) 2
    ("headfuse_in", (headfuse(7989, 20, 672), dict(supported=1)), (headfuse(7990, 20, 672), dict(supported=0)), lambda q: q[1] * q[2] * q[3] * q[4] * 2, U32, 1),
    # ... and an output row at the unsigned ELEMENT offset img out_img_stride + pix nc
    ("headfuse_out", (headfuse(14594, 5, 32), dict(supported=1)), (headfuse(14595, 5, 32), dict(supported=0)), lambda q: q[1] * q[7], U32 - 1, 1),
    # headfuse.hip head_fused_post_supported: a score of the softmax epilogue at the 32-bit byte offset ((n (K - 1) + class) A + anchor) 4
    ("headpost_scores", (("headpost", 3689, 20, 20, 6, 91, 3234), dict(supported=1)), (("headpost", 3690, 20, 20, 6, 91, 3234), dict(supported=0)),
     lambda q: q[1] * (q[5] - 1) * q[6] * 4, U32, 1),
    # convbig.hip launch_patch_resident: the block count is an int kernel argument (it refuses 2^30 and more; 65 535 images are the most patch_shape admits)
    ("resident_blocks", (("patch_blocks", 65535, 2048, 2048), dict(launched=1)), (("patch_blocks", 65535, 2048, 2064), dict(launched=0)),
     lambda q: -(-q[2] // 16) * -(-q[3] // 16) * q[1], I32, 2),
]


@pytest.mark.parametrize("gid,inside,outside,size,limit,slack", GUARDS, ids=[g[0] for g in GUARDS])
def test_guard_sits_at_the_edge_of_the_kernels_arithmetic(gid, inside, outside, size, limit, slack):
    for query, want in (inside, outside):
        got = _lib.debug_choice(*query)
        assert {k: got.get(k) for k in want} == want, (gid, query, got)
    if size is not None:
        assert size(inside[0]) <= limit, (gid, "the inside shape does not fit the kernel's type", size(inside[0]), limit)
        assert size(outside[0]) * slack > limit, (gid, "the outside shape still fits: the guard is tighter than recorded", size(outside[0]), slack, limit)
        assert slack == 1 or size(outside[0]) * slack // 2 <= limit, (gid, "more slack than recorded")


def test_edge_shapes_are_adjacent():
    """Inside and outside differ by one step of the one dimension that is varied (a row, an image, an image line, 32 input channels, a 256-channel tile)."""
    for gid, (qi, _), (qo, _), *_ in GUARDS:
        diff = {(a, b) for a, b in zip(qi, qo) if a != b}       # (a 1x1 problem of one image names its rows twice: m and hw)
        assert len(diff) == 1, gid
        (a, b), = diff
        step = 16 if gid == "resident_blocks" else 2 if gid == "pool_batch" else 32 if gid == "fk_weights" else 256 if gid in ("halo_weights", "glds_weights") else 1
        assert b - a == step, gid


def test_row_counts_are_refused_before_they_overflow():
    """int m = n * ho * wo: dn_debug_choice refuses what launch_conv refuses (2^31 rows or more); the depthwise launcher's n * ho likewise."""
    with pytest.raises(RuntimeError, match="2\\^31 rows"):
        _lib.debug_choice(*conv(2 ** 19, 64, 64, 64, 64))
    assert _lib.debug_choice("dw", 2 ** 19, 2 ** 12, 1, 8, 3, 1, 1)["range"] == 0
    assert _lib.debug_choice("dw", 2 ** 19 - 1, 2 ** 12, 1, 8, 3, 1, 1)["range"] == 1
    # (n + 7) ho wo: the XCD grouping rounds the batch up to 8 groups of images
    assert _lib.debug_choice(*conv(2 ** 19 - 8, 64, 64, 64, 64))["kernel"] != "none"
    with pytest.raises(RuntimeError, match="2\\^31 rows"):
        _lib.debug_choice(*conv(2 ** 19 - 7, 64, 64, 64, 64))


def test_unknown_family_is_an_error():
    with pytest.raises(RuntimeError, match="unknown family"):
        _lib.debug_choice("nothing", 1)
