"""Surface composition (demonet_amd/compose.py, dn_compose) without a GPU: the reference of tests/compose_ref.py against hand-computed
cases and float64 block means, the scenes of tests/test_gpu_compose.py against six wrong resamplers, the wall geometry of compose.grid, and every
refusal of the host validation -- nothing here reaches a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import compose_ref as ref
import regions_ref as rr
from demonet_amd import _lib, compose, osd
from demonet_amd.frames import FrameBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(("nv12", "bt709", False), ("i420", "bt709", False)),            # plane-wise
         (("i420", "bt601", False), ("nv12", "bt709", True)),             # YUV -> YUV across matrix and range: through RGB
         (("nv12", "bt601", True), ("bgr24", "bt709", False)), (("rgb24", "bt709", False), ("i420", "bt601", False)),
         (("bgr24", "bt709", False), ("rgb24", "bt709", False))]


# ---------------------------------------------------------------------------------------------------------------- 1. the filter
def test_hand_computed_cases():
    p = np.array([[10, 20, 40]], np.int64)
    assert ref.weights(3, 2).tolist() == [[2, 1, 0], [0, 1, 2]]
    assert ref.area(p, 1, 2).tolist() == [[(2 * 10 + 20 + 1) // 3, (20 + 2 * 40 + 1) // 3]]
    assert ref.area(np.array([[0, 0], [1, 1]]), 1, 1).tolist() == [[1]]              # 2 / 4 rounds half up
    assert ref.area(np.array([[0, 0], [0, 1]]), 1, 1).tolist() == [[0]]
    assert ref.area(np.array([[0, 0, 1, 1]]), 1, 2).tolist() == [[0, 1]]
    assert ref.area(np.array([[7, 9]]), 1, 3).tolist() == [[7, 8, 9]]                # an upscale: nearest with a blended seam
    for s, d in ((260, 97), (97, 131), (200, 7), (5, 5), (1, 9)):
        w = ref.weights(s, d)
        assert (w.sum(1) == s).all() and (w.sum(0) == d).all() and (w >= 0).all()


def test_one_to_one_is_the_identity_and_constants_stay():
    rng = np.random.default_rng(3)
    p = rng.integers(0, 256, (37, 53))
    assert np.array_equal(ref.area(p, 37, 53), p)
    for s, d in ((260, 97), (260, 13), (260, 1), (97, 131), (200, 7)):
        for v in (0, 1, 127, 254, 255):
            assert (ref.area(np.full((s, 5), v), d, 3) == v).all() and (ref.area(np.full((4, s), v), 6, d) == v).all()


@pytest.mark.parametrize("ky,kx", [(2, 2), (4, 4), (1, 3), (16, 2), (5, 20)])
def test_integer_ratios_equal_the_rounded_block_mean(ky, kx):
    rng = np.random.default_rng(ky * 31 + kx)
    p = rng.integers(0, 256, (ky * 9, kx * 11))
    mean = p.reshape(9, ky, 11, kx).astype(np.float64).sum((1, 3)) / (ky * kx)        # (sums of bytes: exact in float64)
    assert np.array_equal(ref.area(p, 9, 11), np.floor(mean + 0.5).astype(np.int64))


# ---------------------------------------------------------------------------------------------------------------- 2. the scenes
def _scene(src, dst, items_of):
    sp = [ref.noise_planes(src[0], 940 + i, h, w) for i, (h, w) in enumerate(rr.SIZES)]
    dp = [ref.noise_planes(dst[0], 950 + i, h, w) for i, (h, w) in enumerate(ref.DST_SIZES)]
    return sp, dp, items_of(rr.SIZES)


@pytest.mark.parametrize("items_of", [ref.mixed_items, ref.second_items], ids=["mixed", "second"])
@pytest.mark.parametrize("src,dst", PAIRS, ids=["{}-{}".format(s[0], d[0]) for s, d in PAIRS])
def test_the_scenes_tell_the_reference_from_every_wrong_resampler(src, dst, items_of):
    sp, dp, items = _scene(src, dst, items_of)
    want = ref.compose(sp, dp, items, src, dst)
    assert any(not np.array_equal(a, b) for w, d in zip(want, dp) for a, b in zip(w, d))
    for m in ref.MISTAKES:
        if not ref.applies(m, src, dst):
            continue
        got = ref.compose(sp, dp, items, src, dst, mistake=m)
        assert any(not np.array_equal(a, b) for w, g in zip(want, got) for a, b in zip(w, g)), m


def test_the_scenes_are_legal_for_every_pair_and_leave_payload_uncovered():
    for items_of in (ref.mixed_items, ref.second_items):
        items = ref.api_items(items_of(rr.SIZES))
        raw, norm, tiles = compose.item_records(items, rr.SIZES, ref.DST_SIZES, True, True, 16)
        assert len(norm) == len(items) and tiles >= len(items) and len(raw) == 16 + 16 * 48
        covered = np.zeros(ref.DST_SIZES[0], bool)
        for s, sr, d, (x, y, w, h) in norm:
            if d == 0:
                covered[y:y + h, x:x + w] = True
        assert covered.any() and not covered.all()
    mixed = ref.mixed_items(rr.SIZES)
    ratios = [(sr[2] / dr[2], sr[3] / dr[3]) for _, sr, _, dr in mixed]
    assert (2.0, 2.0) in ratios and (4.0, 4.0) in ratios and (1.0, 1.0) in ratios and any(a >= 16 for a, _ in ratios)
    assert any(dr[2:] == (1, 1) for *_, dr in mixed) and any((dr[0] + dr[2]) % 2 == 1 for *_, dr in mixed)
    assert sum(1 for _, _, d, _ in mixed if d == 1) == 4


# ---------------------------------------------------------------------------------------------------------------- 3. grid
@pytest.mark.parametrize("dst_size", [(2160, 3840), (1081, 1919), (67, 91)])
@pytest.mark.parametrize("fit", ["contain", "stretch"])
def test_grid_geometry(dst_size, fit):
    sizes = [(1080, 1920), (720, 1280), (480, 640), (97, 131), (200, 260), (1920, 1080)]
    items = compose.grid(sizes, dst_size, 2, 3, fit=fit, margin=1, yuv=True)
    H, W = dst_size
    assert [it.src for it in items] == list(range(6)) and all(it.dst == 0 and it.src_rect is None for it in items)
    for i, it in enumerate(items):
        x, y, w, h = it.dst_rect
        r, c = divmod(i, 3)
        assert x % 2 == 0 and y % 2 == 0 and w >= 1 and h >= 1
        assert c * W // 3 <= x and x + w <= (c + 1) * W // 3 and r * H // 2 <= y and y + h <= (r + 1) * H // 2       # inside its cell
        if fit == "contain" and min(w, h) > 8:
            sh, sw = sizes[i]
            assert abs(w * sh - h * sw) <= max(sh, sw)            # the source's aspect, to within one destination pixel
    # legal as it stands on a 4:2:0 wall: no overlap, chroma samples included
    compose.item_records(items, sizes, [dst_size], True, True, 8)
    with pytest.raises(ValueError, match="sources"):
        compose.grid(sizes, dst_size, 1, 3)
    with pytest.raises(ValueError, match="fit"):
        compose.grid(sizes, dst_size, 2, 3, fit="cover")
    with pytest.raises(ValueError, match="without a pixel"):
        compose.grid(sizes, (4, 6), 2, 3, margin=2)


def test_grid_of_a_full_hd_wall():
    items = compose.grid([(1080, 1920)] * 64, (2160, 3840), 8, 8)
    assert [it.dst_rect for it in items[:2]] == [(0, 0, 480, 270), (480, 0, 480, 270)] and items[63].dst_rect == (3360, 1890, 480, 270)
    odd = compose.grid([(1080, 1920)] * 2, (270, 961), 1, 2, yuv=False)
    assert odd[1].dst_rect[0] == 480 and compose.grid([(1080, 1920)] * 2, (270, 963), 1, 2, yuv=True)[1].dst_rect[0] == 482


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def test_set_refuses_each_malformed_item_by_name():
    S, D = rr.SIZES, ref.DST_SIZES
    ok = (0, 0, (0, 0, 40, 30))

    def bad(item, match, src_yuv=True, dst_yuv=True, before=(ok,)):
        with pytest.raises(ValueError, match=match):
            compose.item_records(list(before) + [item], S, D, src_yuv, dst_yuv, 8)
    bad((0, 0, (130, 0, 40, 30)), "item 1: the destination rectangle .* outside")
    bad((0, 1, (60, 40, 32, 32)), "item 1: the destination rectangle .* outside")
    bad((0, 1, (0, 0, 10, 10), (250, 0, 11, 10)), "item 1: the source rectangle .* outside")
    bad((0, 1, (0, 0, 10, 10), (-2, 0, 11, 10)), "item 1: the source rectangle .* outside")
    bad((0, 0, (20, 10, 40, 30)), "item 1: .* overlaps item 0")
    bad((0, 0, (0, 28, 10, 10)), "item 1: .* overlaps item 0")
    compose.item_records([ok, (0, 0, (0, 30, 10, 10)), (0, 0, (40, 0, 10, 10)), (0, 1, (0, 0, 40, 30))], S, D, True, True, 8)      # touching, and another surface
    bad((0, 0, (51, 40, 10, 10)), "item 1: odd origin")
    bad((0, 0, (50, 41, 10, 10)), "item 1: odd origin")
    bad((0, 0, (50, 40, 10, 10), (1, 0, 10, 10)), "item 1: odd origin .* source")
    compose.item_records([ok, (0, 0, (51, 41, 10, 10), (1, 1, 10, 10))], S, D, False, False, 8)          # packed RGB on both sides: any origin
    bad((2, 0, (50, 40, 10, 10)), "item 1: source index 2")
    bad((0, -1, (50, 40, 10, 10)), "item 1: destination index -1")
    bad((0, 0, (50, 40, 0, 10)), "item 1: the destination rectangle is 0 x 10")
    bad((0, 0, (50.0, 40, 10, 10)), "item 1: the destination rectangle must be four ints")
    bad("nonsense", "item 1: expected an Item")
    with pytest.raises(ValueError, match="capacity"):
        compose.item_records([ok] * 9, S, D, True, True, 8)
    with pytest.raises(ValueError, match=r"item 0: .*at most 2\^24"):
        compose.item_records([(0, 0, (0, 0, 1, 1))], [(4097, 4096)], D, True, True, 8)
    compose.item_records([(0, 0, (0, 0, 1, 1))], [(4096, 4096)], D, True, True, 8)
    with pytest.raises(ValueError, match="a side takes"):
        compose.item_records([(0, 0, (0, 0, 1, 1))], [(1, 40000)], D, False, True, 8)


def test_a_chroma_only_overlap_is_refused():
    """An odd-width item (0, 0, 41, 30) owns chroma column 20, which also covers luma column 41. A neighbour at the even column 42 is free; one at
    41 shares no luma pixel but that chroma sample. On a 4:2:0 destination it is refused (there for its odd origin, which is what keeps two
    even-origin rectangles that are disjoint in luma disjoint in chroma as well); on a packed destination it is legal. The chroma footprints are
    compared all the same, and the comparison sees this pair."""
    S, D = rr.SIZES, ref.DST_SIZES
    compose.item_records([(0, 0, (0, 0, 41, 30)), (0, 0, (42, 0, 10, 10))], S, D, True, True, 8)
    compose.item_records([(0, 0, (0, 0, 41, 30)), (0, 0, (41, 0, 10, 10))], S, D, True, False, 8)
    with pytest.raises(ValueError, match="item 1: odd origin"):
        compose.item_records([(0, 0, (0, 0, 41, 30)), (0, 0, (41, 0, 10, 10))], S, D, True, True, 8)
    assert not compose._overlap((0, 0, 41, 30), (41, 0, 10, 10))
    assert compose._overlap(compose._chroma((0, 0, 41, 30)), compose._chroma((41, 0, 10, 10)))
    assert not compose._overlap(compose._chroma((0, 0, 41, 30)), compose._chroma((42, 0, 10, 10)))
    assert compose._overlap(compose._chroma((0, 0, 40, 29)), compose._chroma((0, 29, 10, 10))) and not compose._overlap((0, 0, 40, 29), (0, 29, 10, 10))


def test_many_items_are_validated_quickly_and_overlaps_are_found_across_buckets():
    import time
    items = ref.api_items(ref.many_items(rr.SIZES))
    size = [(48 * 34, 48 * 34)]
    t0 = time.perf_counter()
    raw, norm, tiles = compose.item_records(items, rr.SIZES, size, True, True, 4096)
    assert time.perf_counter() - t0 < 2.0                      # (a comparison of every pair would be 2.6 million rectangle tests)
    assert len(norm) == 2304 and tiles == 9216 and np.frombuffer(raw, np.int32)[4 + 12 * 2303 + 10] == 9212
    big = [(2000, 2000)]
    with pytest.raises(ValueError, match="item 2: .* overlaps item 0"):           # a rectangle over several buckets against one far from its origin
        compose.item_records([(0, 0, (10, 10, 900, 900)), (0, 0, (1000, 0, 100, 100)), (0, 0, (900, 700, 40, 40))], rr.SIZES, big, True, True, 8)
    with pytest.raises(ValueError, match="item 1: .* overlaps item 0"):
        compose.item_records([(0, 0, (250, 250, 10, 10)), (0, 0, (256, 256, 10, 10))], rr.SIZES, big, True, True, 8)         # across a bucket edge
    compose.item_records([(0, 0, (0, 0, 256, 256)), (0, 0, (256, 0, 256, 256)), (0, 0, (0, 256, 257, 255)), (0, 0, (258, 256, 10, 10))], rr.SIZES, big, True, True, 8)


def _batch(sizes, fmt="nv12", matrix="bt709", full=False, device="cuda:0"):
    """a FrameBatch that says it holds frames of these sizes (host state only: nothing here is on a device)"""
    b = FrameBatch(len(sizes), device, format=fmt, matrix=matrix, full_range=full)
    b.sizes, b.table = list(sizes), torch.zeros(1)
    return b


def _set_state(comp, src, dst, items):
    """what Compositor.set remembers, without the upload"""
    _, comp.items, comp.tiles = compose.item_records(items, src.sizes, dst.sizes, src.format in ref.YUV, dst.format in ref.YUV, comp.capacity)
    comp.table = torch.zeros(1)
    comp.src_sizes, comp.dst_sizes = list(src.sizes), list(dst.sizes)
    comp.src_space, comp.dst_space = (src.format_code, src.color_code), (dst.format_code, dst.color_code)


def test_a_call_refuses_stale_sizes_wrong_objects_and_devices_before_the_library_is_touched(monkeypatch):
    def boom():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", boom)
    comp = compose.Compositor(8, "cuda:0")
    src, dst = _batch(rr.SIZES), _batch(ref.DST_SIZES)
    with pytest.raises(ValueError, match="no items yet"):
        comp(src, dst)
    _set_state(comp, src, dst, ref.api_items(ref.mixed_items(rr.SIZES))[:8])
    compose.check_compose("test", comp, src, dst)
    with pytest.raises(ValueError, match="stale sizes: .* source"):
        comp(_batch([rr.SIZES[0], (96, 130)]), dst)
    with pytest.raises(ValueError, match="stale sizes: .* destination"):
        comp(src, _batch([(128, 160), (68, 92)]))
    with pytest.raises(ValueError, match="format / colour code"):
        comp(_batch(rr.SIZES, "i420"), dst)
    with pytest.raises(ValueError, match="format / colour code"):
        comp(src, _batch(ref.DST_SIZES, "nv12", "bt601"))
    with pytest.raises(ValueError, match="must be a FrameBatch"):
        comp(torch.zeros(4), dst)
    with pytest.raises(ValueError, match="is on cuda:1"):
        comp(_batch(rr.SIZES, device="cuda:1"), dst)
    with pytest.raises(ValueError, match="two batches"):
        comp(src, src)
    unset = _batch(rr.SIZES)
    unset.table = None
    with pytest.raises(ValueError, match="names no frames yet"):
        comp(unset, dst)
    with pytest.raises(ValueError, match="clear must be three ints"):
        comp(src, dst, clear=(0, 0, 256))
    with pytest.raises(ValueError, match="go together"):
        compose.check_composition(comp, None, src, "track_frames")
    with pytest.raises(ValueError, match="expected a Compositor"):
        compose.check_composition(object(), dst, src, "track_frames")
    compose.check_composition(None, None, src, "track_frames")
    for cap in (0, 65537, 2.0, True):
        with pytest.raises(ValueError, match="capacity"):
            compose.Compositor(cap, "cuda:0")
    cpu = compose.Compositor(4, "cpu")
    with pytest.raises(ValueError, match="is on cuda:0"):
        cpu.set([], src, dst)
    host_src, host_dst = _batch(rr.SIZES, device="cpu"), _batch(ref.DST_SIZES, device="cpu")
    with pytest.raises(ValueError, match="item 0"):
        cpu.set([(0, 0, (0, 0, 500, 10))], host_src, host_dst)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cpu.set([(0, 0, (0, 0, 50, 10))], host_src, host_dst)


# ---------------------------------------------------------------------------------------------------------------- 5. ABI and colour
def test_the_records_match_the_header(tmp_path):
    fields = ["src", "sx0", "sy0", "sw", "sh", "dst", "dx0", "dy0", "dw", "dh", "tile0", "reserved"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "demonet_hip.h"\n'
                   '_Static_assert(sizeof(dn_compose_item) == 48 && sizeof(dn_compose_header) == 16 && sizeof(dn_frame) == 48, "sizes");\n'
                   'int main(){printf("%zu %zu", sizeof(dn_compose_item), sizeof(dn_compose_header));\n'
                   + "".join('printf(" %zu", offsetof(dn_compose_item, {}));\n'.format(f) for f in fields)
                   + 'printf(" %zu %zu\\n", offsetof(dn_compose_header, n_items), offsetof(dn_compose_header, n_tiles));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert a[:2] == [C.sizeof(_lib.ComposeItem), C.sizeof(_lib.ComposeHeader)] == [48, 16]
    assert a[2:14] == [getattr(_lib.ComposeItem, f).offset for f in fields]
    assert a[14:] == [_lib.ComposeHeader.n_items.offset, _lib.ComposeHeader.n_tiles.offset]
    raw, norm, tiles = compose.item_records([(1, 0, (2, 4, 33, 65), (6, 8, 10, 12))], rr.SIZES, ref.DST_SIZES, True, True, 2)
    words = np.frombuffer(raw, np.int32)
    assert words[:4].tolist() == [1, 6, 0, 0] and tiles == 6
    assert words[4:16].tolist() == [1, 6, 8, 10, 12, 0, 2, 4, 33, 65, 0, 0] and not words[16:].any()


def test_the_forward_matrix_is_the_overlays():
    for matrix, full in (("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)):
        assert ref.forward_coeffs(matrix, full) == osd.forward_coeffs(matrix, full)
        cy, cu, cv, yo = ref.forward_coeffs(matrix, full)
        for rgb in ((0, 0, 0), (255, 255, 255), (255, 0, 0), (12, 200, 97)):
            px = np.array(rgb, np.int64)
            assert (int(ref.component(cy, px, yo)), int(ref.component(cu, px, 128)), int(ref.component(cv, px, 128))) == osd.to_surface(
                rgb, "nv12", matrix, full)
    # the table the kernel file carries is this one
    text = open(os.path.join(ROOT, "demonet_amd", "csrc", "compose.hip")).read()
    for matrix, full in (("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)):
        cy, cu, cv, yo = osd.forward_coeffs(matrix, full)
        want = "CpForward{{{{{}}}, {{{}}}, {{{}}}, {}}}".format(", ".join(map(str, cy)), ", ".join(map(str, cu)), ", ".join(map(str, cv)), yo)
        assert want in text, want
