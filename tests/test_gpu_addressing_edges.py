"""GPU tests (-m gpu): every 32-bit addressing guard that a stand-alone entry point reaches, run just inside and just outside its limit
(tests/test_addressing_edges_cpu.py holds the limits themselves to the kernels' arithmetic without a GPU).

Every case: inputs from a seeded device generator (i.i.d. normal: not periodic, so a row read from another image shows); the output lies
between two guard regions, everything pre-filled with 0xFF bytes; afterwards the guard regions are intact, no output element is still
0xFFFF / 0xFFFFFFFF (a NaN pattern that no sum of finite values produces), dn_debug_last_kernel names the kernel the inventory gives for that side
of the edge, EVERY element is compared on the device, in chunks, with a plain fp32 torch evaluation of the operation on the fp16-rounded
operands (tolerances of tests/test_gpu_kernels.py: 4e-3 after rounding the reference to fp16, 2e-3 for fp32 head rows), and sampled regions --
the first and last tile, the rows on both sides of every multiple of 2^31 and 2^32 bytes in the input and output arrays, the seam between two
image ranges of launch_conv_pool -- are copied to the host with their halo and held to float64 math at the same tolerances: that checks the
device reference as well, at the places where a wrapped offset would land. No whole tensor travels to the host.

The outside shape of a GPU case is a few rows or images beyond the first outside shape (which the CPU file tests), so that its arrays CROSS the
2^31 / 2^32-byte line instead of ending on it. Where two kernels share a label (the K loop with and without bound tests, the depthwise launch
with and without its weights in LDS) dn_debug_choice tells the sides apart. DN_EDGE_PROFILE=<file>: one line per case is appended to it."""
import ctypes as C
import os
import time

import pytest
import torch
import torch.nn.functional as F

from demonet_amd.plan import fragment_major

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 1 << 16                      # bytes in front of and behind every output
LINES = (1 << 31, 1 << 32)
ROWS = 1 << 20                       # rows of a 1x1 problem per reference chunk
PIX = 1 << 19                        # pixels of a convolution per reference chunk
E_INVALID, E_UNSUPPORTED = -1, -4


def _lib():
    from demonet_amd import _lib as L
    return L, L.lib()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _act(x, act):
    return [lambda v: v, F.relu, F.relu6, F.hardswish][act](x)


@pytest.fixture(autouse=True)
def _free_device_memory():
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a device fault is sticky: nothing more may be started on this GPU from this process
        pytest.exit("device error after a case, stopping: %s" % e, returncode=3)
    torch.cuda.empty_cache()


class Out:
    """nbytes of output between two guard regions, all of it 0xFF."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.raw = torch.full((GUARD + nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        assert self.raw.data_ptr() % 256 == 0

    @property
    def ptr(self):
        return C.c_void_p(self.raw.data_ptr() + GUARD)

    def view(self, dtype, *shape):
        return self.raw[GUARD:GUARD + self.nbytes].view(dtype).view(*shape)

    def guards_intact(self):
        return bool((self.raw[:GUARD] == 0xFF).all()) and bool((self.raw[GUARD + self.nbytes:] == 0xFF).all())

    def untouched(self):
        return bool((self.raw[GUARD:GUARD + self.nbytes] == 0xFF).all())


def _unwritten(t):
    """Elements of an fp16 / fp32 tensor that still hold the 0xFF fill."""
    return int((t.view(torch.int16 if t.dtype == torch.half else torch.int32) == -1).sum())


def _worst(got, ref, tol):
    """max |got - ref| / (tol + tol |ref|): assert_close(rtol=tol, atol=tol) passes iff this is <= 1. A NaN on either side counts as infinite."""
    r = (got.double() - ref.double()).abs() / (tol + tol * ref.double().abs())
    return float(torch.nan_to_num(r, nan=float("inf")).max()) if r.numel() else 0.0


def _line_rows(nbytes, row_bytes):
    """Rows on both sides of every 2^31 / 2^32-byte line inside an array of nbytes made of rows of row_bytes."""
    rows = set()
    for line in LINES:
        for b in range(line, nbytes, line):
            r = b // row_bytes                                  # the row that holds byte b (it straddles the line, or starts on it)
            rows.update((r - 1, r, r + 1))
    return {r for r in rows if 0 <= r < nbytes // row_bytes}


class Case:
    def __init__(self, name, shape):
        self.name, self.shape, self.t0 = name, shape, time.time()
        self.arrays, self.label, self.whole, self.sampled, self.note = {}, "", 0.0, 0.0, ""

    def finish(self):
        wall = time.time() - self.t0
        line = "%-28s %-44s %-34s %6.1f s  whole %.3f  sampled %.3f  %s%s" % (
            self.name, self.shape, self.label, wall, self.whole, self.sampled, "  ".join("%s %d B" % kv for kv in self.arrays.items()), self.note and "  [" + self.note + "]")
        print(line)
        path = os.environ.get("DN_EDGE_PROFILE")
        if path:
            with open(path, "a") as f:
                f.write(line + "\n")
        assert self.whole <= 1.0 and self.sampled <= 1.0, line


# ---------------------------------------------------------------------------------------------------------------- 1x1 convolutions
def _pointwise_case(name, m, hw, cin, cout, act, fp32, wfrag, label, choice, res=False, se=False):
    """dn_pointwise_conv on m rows in images of hw rows; choice: what dn_debug_choice must say about the shape (tells apart what shares a label)."""
    L, lib = _lib()
    got_choice = L.debug_choice("pw", m, cin, cout, hw, act, int(fp32), int(se), int(res), int(wfrag))
    assert {k: got_choice[k] for k in choice} == choice, got_choice
    case = Case(name, "m=%d cin=%d cout=%d hw=%d%s%s%s" % (m, cin, cout, hw, " fp32" if fp32 else "", " +res" if res else "", " +se" if se else ""))
    g = _gen(m % 100003 + cin)
    x = torch.randn(m, cin, dtype=torch.half, device=DEV, generator=g)
    w = (torch.randn(cout, cin, device=DEV, generator=g) / cin ** 0.5).half()
    b = torch.randn(cout, device=DEV, generator=g)
    wf = torch.from_numpy(fragment_major(w.cpu().numpy())).to(DEV) if wfrag else None
    nimg, esz = m // hw, 4 if fp32 else 2
    r = torch.randn(m, cout, dtype=torch.half, device=DEV, generator=g) if res else None
    sc = torch.rand(nimg, cin, device=DEV, generator=g) if se else None
    extra = 7 * cout if fp32 else 0                      # fp32 head rows go into a larger per-image anchor array
    stride = hw * cout + extra
    out = Out(nimg * stride * esz)
    case.arrays = dict(x=x.numel() * 2, w=w.numel() * 2, out=out.nbytes, **({"residual": r.numel() * 2} if res else {}))
    L.check(lib.dn_pointwise_conv(_ptr(x), _ptr(w), _ptr(wf), _ptr(b), _ptr(r), _ptr(sc), out.ptr, m, cin, cout, hw, act, int(fp32), stride if fp32 else 0, _stream()),
            "dn_pointwise_conv")
    torch.cuda.synchronize()
    case.label = L.debug_last_kernel()
    assert case.label == label
    assert out.guards_intact()
    o = out.view(torch.float if fp32 else torch.half, nimg, stride)
    if fp32:
        assert bool((o[:, hw * cout:].view(torch.int32) == -1).all())          # nothing written outside the level's slice
    rows = o[:, :hw * cout].reshape(m, cout) if fp32 else o.view(m, cout)      # (one image when fp32: the reshape is a view)
    tol = 2e-3 if fp32 else 4e-3
    wt = w.float().t().contiguous()
    for r0 in range(0, m, ROWS):
        gotc = rows[r0:r0 + ROWS]
        assert _unwritten(gotc) == 0
        ref = _act(_scaled(x[r0:r0 + ROWS], sc, r0, hw).float() @ wt + b, act)
        if res:
            ref = ref + r[r0:r0 + ROWS].float()
        case.whole = max(case.whole, _worst(gotc.float(), ref if fp32 else ref.half().float(), tol))
    # sampled rows on the host in float64: first and last tile, both sides of every 2^31 / 2^32-byte line of x and of the output
    pick = set(range(min(m, 128))) | set(range(max(m - 128, 0), m)) | _line_rows(m * cin * 2, cin * 2) | _line_rows(m * cout * esz, cout * esz)
    if res:
        pick |= _line_rows(m * cout * 2, cout * 2)
    idx = torch.tensor(sorted(pick), device=DEV)
    xs = x[idx].cpu().double()
    if se:          # the kernel rounds the scaled input to fp16
        xs = (x[idx].float() * sc[idx // hw]).half().cpu().double()
    ref64 = _act(xs @ w.cpu().double().t() + b.cpu().double(), act)
    if res:
        ref64 = ref64 + r[idx].cpu().double()
    ref64 = ref64.float() if fp32 else ref64.half().float()
    case.sampled = _worst(rows[idx].cpu().float(), ref64, tol)
    case.note = "%d sampled rows" % len(pick)
    case.finish()


def _scaled(xc, sc, r0, hw):
    """rows r0 .. of x times their image's squeeze-excitation scale, rounded to fp16 as the kernels round it"""
    if sc is None:
        return xc
    img = (torch.arange(r0, r0 + xc.shape[0], device=DEV) // hw)
    return (xc.float() * sc[img]).half()


def test_pointwise_wstat_at_its_store_offset_limit_inside():
    """pw_wstat_kernel: output of 2^31 - 128 bytes (m cout 2 < 2^31 - 1), 255 images in XCD groups of 32."""
    _pointwise_case("pw_wstat inside", (1 << 24) - 1, 65793, 16, 64, 1, False, True, "pw_wstat_kernel<2,2>", dict(kernel="pw_wstat_kernel"))


def test_pointwise_wstat_at_its_store_offset_limit_outside():
    """One image of 65536 rows beyond 2^24 rows: pw_direct_kernel (64-bit addresses), the output crosses the 2^31-byte line at row 2^24."""
    _pointwise_case("pw_wstat outside", 257 << 16, 1 << 16, 16, 64, 1, False, True, "pw_direct_kernel<1,1>", dict(kernel="pw_direct_kernel"))


def test_pointwise_residual_across_the_line():
    """The outside shape with a residual (pw_direct_kernel): residual and output of 2^31 + 2^23 bytes, rows on both sides of the line sampled in both."""
    _pointwise_case("pw residual outside", 257 << 16, 1 << 16, 16, 64, 0, False, True, "pw_direct_kernel<1,1>", dict(kernel="pw_direct_kernel"), res=True)


def test_pointwise_scaled_input_across_the_line():
    """The K loop's outside shape with a squeeze-excitation scale and a residual, fp16 output: the bound-tested loop scales x (2^31 + 85 888 bytes) behind each load."""
    _pointwise_case("pw fast-K outside se", 1597894, 1597894, 672, 32, 0, False, False, "pw_kernel<128,32,4,1,false,32,4>", dict(kernel="pw_kernel", fk=0), res=True, se=True)


def test_pointwise_fast_k_loop_at_its_input_limit_inside():
    """The K loop without bound tests (32-bit byte offsets into x): m cin = 2^30 - 64, fp32 rows, cin = 672 (pw_direct_supported declines it)."""
    _pointwise_case("pw fast-K inside", 1597830, 1597830, 672, 24, 0, True, False, "pw_kernel<128,32,4,1,false,32,4>", dict(kernel="pw_kernel", fk=1))


def test_pointwise_fast_k_loop_at_its_input_limit_outside():
    """64 rows beyond: the bound-tested K loop of the same tile (64-bit addresses); x crosses the 2^31-byte line inside row 1597830."""
    _pointwise_case("pw fast-K outside", 1597894, 1597894, 672, 24, 0, True, False, "pw_kernel<128,32,4,1,false,32,4>", dict(kernel="pw_kernel", fk=0))


# ---------------------------------------------------------------------------------------------------------------- dense convolutions
def _conv_ref_dev(x, wt, b, act, i0, i1, r0, r1, k, pooled):
    """fp32 on the device: rows [r0, r1) of images [i0, i1) of the k x k "same" (k = 1: 1x1) convolution of x [n][h][w][cin] with wt [cout][k][k][cin]."""
    h = x.shape[1]
    if k == 1:
        y = x[i0:i1, r0:r1].float() @ wt[:, 0, 0, :].float().t()
    else:
        xs = x[i0:i1, max(r0 - 1, 0):min(r1 + 1, h)].float()
        xs = F.pad(xs, (0, 0, 1, 1, 1 if r0 == 0 else 0, 1 if r1 == h else 0))
        rr, ww = r1 - r0, x.shape[2]
        y = None
        for ky in range(3):
            for kx in range(3):
                t = xs[:, ky:ky + rr, kx:kx + ww, :] @ wt[:, ky, kx, :].float().t()
                y = t if y is None else y + t
    y = _act(y + b, act)
    if pooled:
        n_, rr, ww, c = y.shape
        y = y.view(n_, rr // 2, 2, ww // 2, 2, c).amax(dim=(2, 4))
    return y


def _conv_ref_host(x, wt, b, act, img, r0, r1, k, pooled):
    """float64 on the host: the same band through F.conv2d, from the band's rows and their halo only."""
    h = x.shape[1]
    p = k // 2
    xs = x[img, max(r0 - p, 0):min(r1 + p, h)].cpu().double().permute(2, 0, 1)[None]
    xs = F.pad(xs, (p, p, p if r0 == 0 else 0, p if r1 == h else 0))
    y = _act(F.conv2d(xs, wt.cpu().double().permute(0, 3, 1, 2), b.cpu().double()), act)
    if pooled:
        y = F.max_pool2d(y, 2, 2)
    return y[0].permute(1, 2, 0)


def _bands(n, h, rows, even):
    """Global image rows (image * h + row) -> the bands (image, r0, r1) to sample: whole images when they are small, else four rows around the row."""
    out = set()
    for R in rows:
        img, r = divmod(R, h)
        if h <= 64:
            out.add((img, 0, h))
        else:
            r0 = max(r - 2, 0)
            r0 -= r0 & 1 if even else 0
            out.add((img, r0, min(r0 + 4, h)))
    return sorted(out)


def _dense_case(name, n, h, w, cin, cout, k, act, label, pooled=False, keep_map=False, seams=()):
    """dn_dense_conv (k x k "same", stride 1), or with pooled dn_debug_conv_pool (+ MaxPool2d(2, 2); keep_map: the full-resolution map as well)."""
    L, lib = _lib()
    case = Case(name, "n=%d %dx%d %d->%d k=%d%s" % (n, h, w, cin, cout, k, " +pool" if pooled else ""))
    g = _gen(n % 100003 + h + cin)
    x = torch.randn(n, h, w, cin, dtype=torch.half, device=DEV, generator=g)
    wt = (torch.randn(cout, k, k, cin, device=DEV, generator=g) / (k * cin ** 0.5)).half()
    b = torch.randn(cout, device=DEV, generator=g)
    z = torch.zeros(64, dtype=torch.uint8, device=DEV)
    outs = []                                                # (Out, pooled?) of every array the call writes
    if pooled:
        outs.append((Out(n * (h // 2) * (w // 2) * cout * 2), True))
        if keep_map:
            outs.append((Out(n * h * w * cout * 2), False))
        rc = lib.dn_debug_conv_pool(_ptr(x), _ptr(wt), _ptr(b), _ptr(z), outs[0][0].ptr, outs[1][0].ptr if keep_map else None, n, h, w, cin, cout, act, _stream())
        L.check(rc, "dn_debug_conv_pool")
    else:
        outs.append((Out(n * h * w * cout * 2), False))
        rc = lib.dn_dense_conv(_ptr(x), _ptr(wt), _ptr(b), _ptr(z), outs[0][0].ptr, n, h, w, cin, cout, k, 1, k // 2, 1, act, _stream())
        L.check(rc, "dn_dense_conv")
    torch.cuda.synchronize()
    case.label = L.debug_last_kernel()
    case.arrays = dict(x=x.numel() * 2, w=wt.numel() * 2, **{("pool_out" if p else "out"): o.nbytes for o, p in outs})
    assert case.label == label
    views = []
    for o, p in outs:
        assert o.guards_intact()
        views.append((o.view(torch.half, n, h // 2, w // 2, cout) if p else o.view(torch.half, n, h, w, cout), p))
    # every element, on the device: chunks of whole images, or of row bands of one image
    per = max(1, PIX // (h * w))
    band = h if h * w <= PIX else max(2, (PIX // w) & ~1)
    for i0 in range(0, n, per):
        i1 = min(i0 + per, n)
        for r0 in range(0, h, band):
            r1 = min(r0 + band, h)
            full = _conv_ref_dev(x, wt, b, act, i0, i1, r0, r1, k, False)
            for v, p in views:
                ref = full.view(i1 - i0, (r1 - r0) // 2, 2, w // 2, 2, cout).amax(dim=(2, 4)) if p else full
                gotc = v[i0:i1, r0 // 2:r1 // 2] if p else v[i0:i1, r0:r1]
                assert _unwritten(gotc) == 0
                case.whole = max(case.whole, _worst(gotc.float(), ref.half().float(), 4e-3))
            del full
    # sampled bands on the host in float64: first and last rows, both sides of every 2^31 / 2^32-byte line of the input and of every output, the seams
    rows = {0, n * h - 1} | _line_rows(x.numel() * 2, w * cin * 2) | set(seams)
    for o, p in outs:
        rows |= {2 * r for r in _line_rows(o.nbytes, (w // 2) * cout * 2)} if p else _line_rows(o.nbytes, w * cout * 2)
    bands = _bands(n, h, rows, pooled)
    for img, r0, r1 in bands:
        for v, p in views:
            ref64 = _conv_ref_host(x, wt, b, act, img, r0, r1, k, p).half().float()
            gotb = (v[img, r0 // 2:r1 // 2] if p else v[img, r0:r1]).cpu().float()
            case.sampled = max(case.sampled, _worst(gotb, ref64, 4e-3))
    case.note = "%d sampled bands" % len(bands)
    case.finish()


def test_conv_halo_at_its_input_descriptor_limit_inside():
    """conv_halo_kernel<3,8,2>: the input as a raw buffer of 2^31 - 65536 bytes (m cin 2 < 2^31)."""
    _dense_case("conv_halo inside", 32767, 16, 16, 128, 128, 3, 1, "conv_halo_kernel<3,8,2>")


def test_conv_halo_at_its_input_descriptor_limit_outside():
    """Four images more: conv_patch_kernel (an image per grid.z, 64-bit image base); input and output cross the 2^31-byte line at image 32768."""
    _dense_case("conv_halo outside", 32771, 16, 16, 128, 128, 3, 1, "conv_patch_kernel")


def test_conv_patch_resident_at_its_output_descriptor_limit_inside():
    """conv_patch_resident_kernel: the output as a raw buffer of 2^32 - 2^19 bytes (< 0xFFFFFFF0); both arrays cross the 2^31-byte line at image 4096."""
    _dense_case("patch_resident out inside", 8191, 64, 64, 64, 64, 3, 1, "conv_patch_resident_kernel")


def test_conv_patch_resident_at_its_output_descriptor_limit_outside():
    """Two images more: conv_patch_kernel; both arrays cross the 2^31-byte line at image 4096 and the 2^32-byte line at image 8192."""
    _dense_case("patch_resident out outside", 8193, 64, 64, 64, 64, 3, 1, "conv_patch_kernel")


def test_conv_patch_resident_at_its_image_offset_limit_inside():
    """conv_patch_resident_kernel: one image of 2^31 - 2^19 bytes (h w 128 < 2^31: int byte offsets inside the image)."""
    _dense_case("patch_resident image inside", 1, 4095, 4096, 64, 64, 3, 1, "conv_patch_resident_kernel")


def test_conv_patch_resident_at_its_image_offset_limit_outside():
    """Two image lines more: conv_patch_kernel (64-bit offsets); the image crosses the 2^31-byte line at line 4096."""
    _dense_case("patch_resident image outside", 1, 4097, 4096, 64, 64, 3, 1, "conv_patch_kernel")


def test_conv_patch_kernels_at_the_grid_z_limit_inside():
    """65535 images: the last batch the patch kernels take (conv_patch_kernel has the image on grid.z)."""
    _dense_case("patch images inside", 65535, 4, 4, 64, 64, 3, 1, "conv_patch_resident_kernel")


def test_conv_patch_kernels_at_the_grid_z_limit_outside():
    """65536 images: the implicit-GEMM tile."""
    _dense_case("patch images outside", 65536, 4, 4, 64, 64, 3, 1, "pw_kernel<128,64,4,1,true,32>")


def test_conv_glds_at_its_input_offset_limit_inside():
    """conv_glds_kernel (a dense 1x1 on the 256 x 256 tile): int byte offsets into 2^31 - 16384 bytes of input; the output crosses the 2^31-byte line."""
    _dense_case("conv_glds inside", 131071, 8, 8, 128, 256, 1, 1, "conv_glds_kernel")


def test_conv_glds_at_its_input_offset_limit_outside():
    """Six images more: the pointwise family serves it (pw_direct_kernel, 64-bit addresses); the input crosses 2^31, the output 2^31 and 2^32."""
    _dense_case("conv_glds outside", 131077, 8, 8, 128, 256, 1, 1, "pw_direct_kernel<8,1>")


def test_conv_pool_just_below_one_image_range():
    """launch_conv_pool, conv3_3 of ssd512 (256 -> 256 on 128 x 128): 255 images are 2^31 - 2^23 bytes of input, one launch."""
    _dense_case("conv_pool one range", 255, 128, 128, 256, 256, 3, 1, "conv_halo_kernel<3,4,4>", pooled=True)


def test_conv_pool_two_image_ranges_with_a_remainder():
    """257 images go out as 255 + 2: the second launch starts at image 255, its input 2^23 bytes in front of the 2^31-byte line. The seam (the
    last image line of image 254, the first of image 255) and the line are sampled; the full-resolution map (2^31 + 2^24 bytes) is written too."""
    _dense_case("conv_pool two ranges", 257, 128, 128, 256, 256, 3, 1, "conv_halo_kernel<3,4,4>", pooled=True, keep_map=True, seams=(255 * 128 - 1, 255 * 128))


# ---------------------------------------------------------------------------------------------------------------- depthwise convolutions
def _dw_ref_dev(x, wd, b, act, r0, r1):
    h, w = x.shape[1], x.shape[2]
    xs = x[:, max(r0 - 1, 0):min(r1 + 1, h)].float()
    xs = F.pad(xs, (0, 0, 1, 1, 1 if r0 == 0 else 0, 1 if r1 == h else 0))
    y = torch.zeros(x.shape[0], r1 - r0, w, x.shape[3], device=DEV) + b
    for ky in range(3):
        for kx in range(3):
            y = y + xs[:, ky:ky + r1 - r0, kx:kx + w, :] * wd[ky * 3 + kx].float()
    return _act(y, act)


def _dw_ref_host(x, wd, b, act, img, r0, r1):
    h, c = x.shape[1], x.shape[3]
    xs = x[img, max(r0 - 1, 0):min(r1 + 1, h)].cpu().double().permute(2, 0, 1)[None]
    xs = F.pad(xs, (1, 1, 1 if r0 == 0 else 0, 1 if r1 == h else 0))
    wt = wd.cpu().double().t().reshape(c, 1, 3, 3)
    return _act(F.conv2d(xs, wt, b.cpu().double(), 1, 0, 1, c), act)[0].permute(1, 2, 0)


def _depthwise_case(name, n, h, w, c, act, choice, xcd=None, monkeypatch=None):
    """dn_depthwise_conv, 3 x 3 stride 1 pad 1."""
    L, lib = _lib()
    if xcd is not None:
        monkeypatch.setenv("DN_XCD", xcd)
    got_choice = L.debug_choice("dw", n, h, w, c, 3, 1, 1)
    assert got_choice["range"] == 1 and (got_choice["wlds"] > 0) == choice, got_choice
    case = Case(name, "n=%d %dx%d c=%d%s" % (n, h, w, c, "" if xcd is None else " DN_XCD=" + xcd))
    g = _gen(n % 100003 + h % 1009 + c)
    x = torch.randn(n, h, w, c, dtype=torch.half, device=DEV, generator=g)
    wd = (torch.randn(9, c, device=DEV, generator=g) / 3).half()
    b = torch.randn(c, device=DEV, generator=g)
    out = Out(x.numel() * 2)
    case.arrays = dict(x=x.numel() * 2, out=out.nbytes)
    L.check(lib.dn_depthwise_conv(_ptr(x), _ptr(wd), _ptr(b), out.ptr, n, h, w, c, 3, 1, 1, act, _stream()), "dn_depthwise_conv")
    torch.cuda.synchronize()
    case.label = L.debug_last_kernel()
    assert case.label == "dw_kernel<3,1,4>"
    assert out.guards_intact()
    v = out.view(torch.half, n, h, w, c)
    per = max(1, (1 << 22) // (h * w))
    band = h if h * w <= (1 << 22) else (1 << 22) // w
    for i0 in range(0, n, per):
        for r0 in range(0, h, band):
            r1 = min(r0 + band, h)
            gotc = v[i0:i0 + per, r0:r1]
            assert _unwritten(gotc) == 0
            case.whole = max(case.whole, _worst(gotc.float(), _dw_ref_dev(x[i0:i0 + per], wd, b, act, r0, r1).half().float(), 4e-3))
    rows = {0, n * h - 1} | _line_rows(x.numel() * 2, w * c * 2)
    bands = _bands(n, h, rows, False)
    for img, r0, r1 in bands:
        case.sampled = max(case.sampled, _worst(v[img, r0:r1].cpu().float(), _dw_ref_host(x, wd, b, act, img, r0, r1).half().float(), 4e-3))
    case.note = "%d sampled bands, wlds=%d" % (len(bands), got_choice["wlds"])
    case.finish()


def test_depthwise_weights_in_lds_at_the_descriptor_limit_inside():
    """One image of h w c = 2^30 - 128: the image is a raw buffer of 2^31 - 256 bytes, weights in LDS."""
    _depthwise_case("dw wlds inside", 1, (1 << 23) - 1, 16, 8, 1, True)


def test_depthwise_weights_in_lds_at_the_descriptor_limit_outside():
    """h w c = 2^30: per-thread weight loads and pointer arithmetic (the same label)."""
    _depthwise_case("dw wlds outside", 1, 1 << 23, 16, 8, 1, False)


def test_depthwise_at_the_image_index_limit_inside():
    """One image of h w c = 2^31 - 128 elements, the last one the kernel's int element offsets reach; it crosses the 2^31-byte line at line 2^23."""
    _depthwise_case("dw image inside", 1, (1 << 24) - 1, 16, 8, 1, False)


def test_depthwise_at_the_image_index_limit_is_refused_outside():
    """h w c = 2^31: refused, the error names the range, nothing is written."""
    L, lib = _lib()
    h = 1 << 24
    assert L.debug_choice("dw", 1, h, 16, 8, 3, 1, 1)["range"] == 0        # (only then is the call made: it must stop in the launcher)
    x = torch.zeros(1 << 20, dtype=torch.half, device=DEV)
    out = Out(1 << 20)
    rc = lib.dn_depthwise_conv(_ptr(x), _ptr(x), _ptr(x.view(torch.float)), out.ptr, 1, h, 16, 8, 3, 1, 1, 1, _stream())
    err = lib.dn_last_error().decode()
    torch.cuda.synchronize()
    assert rc == E_INVALID and "index range" in err and "2^31" in err, (rc, err)
    assert out.untouched() and out.guards_intact()


def test_depthwise_many_images_on_the_plain_grid(monkeypatch):
    """65535 images with DN_XCD=0 (the image on grid.y)."""
    _depthwise_case("dw images DN_XCD=0", 65535, 4, 4, 8, 1, True, xcd="0", monkeypatch=monkeypatch)


def test_depthwise_pooled_sums_at_the_descriptor_limit():
    """dn_depthwise_conv_pool on the largest image that keeps its weights in LDS: the output as above, and the per-workgroup channel sums
    (131 072 partial rows, fp32) against the sum of the fp32 reference (tolerance of the pooled sums in tests/test_gpu_kernels.py)."""
    L, lib = _lib()
    n, h, w, c = 1, (1 << 23) - 1, 16, 8
    assert L.debug_choice("dw", n, h, w, c, 3, 1, 1) == dict(kernel="dw_kernel<3,1,4>", range=1, wlds=176)
    case = Case("dw pooled wlds inside", "n=%d %dx%d c=%d +sums" % (n, h, w, c))
    g = _gen(h % 1009 + c + 1)
    x = torch.randn(n, h, w, c, dtype=torch.half, device=DEV, generator=g)
    wd = (torch.randn(9, c, device=DEV, generator=g) / 3).half()
    b = torch.randn(c, device=DEV, generator=g)
    blocks = lib.dn_depthwise_pool_blocks(h, w, c, 3, 1, 1)
    out, pool = Out(x.numel() * 2), Out(n * blocks * c * 4)
    case.arrays = dict(x=x.numel() * 2, out=out.nbytes, pool=pool.nbytes)
    L.check(lib.dn_depthwise_conv_pool(_ptr(x), _ptr(wd), _ptr(b), out.ptr, n, h, w, c, 3, 1, 1, 1, pool.ptr, None, None, None, None, None, None, 0, _stream()),
            "dn_depthwise_conv_pool")
    torch.cuda.synchronize()
    case.label = L.debug_last_kernel()
    assert case.label == "dw_kernel<3,1,4>" and out.guards_intact() and pool.guards_intact()
    v, pv = out.view(torch.half, n, h, w, c), pool.view(torch.float, n, blocks, c)
    assert _unwritten(pv) == 0
    band, sums = (1 << 22) // w, torch.zeros(c, dtype=torch.double, device=DEV)
    for r0 in range(0, h, band):
        r1 = min(r0 + band, h)
        ref = _dw_ref_dev(x, wd, b, 1, r0, r1)
        sums += ref.double().sum(dim=(0, 1, 2))
        assert _unwritten(v[:, r0:r1]) == 0
        case.whole = max(case.whole, _worst(v[:, r0:r1].float(), ref.half().float(), 4e-3))
    got = pv.double().sum(dim=(0, 1))
    case.sampled = float(((got - sums).abs() / (2e-2 + 2e-3 * sums.abs())).max())
    case.note = "sampled = worst channel sum against the fp32 reference's, / (2e-2 + 2e-3 |sum|)"
    case.finish()


def test_expand_depthwise_at_the_grid_z_limit_inside():
    """65535 images, the last batch dn_expand_depthwise takes: expand 16 -> 64, depthwise 3 x 3 on 5 x 5 maps."""
    L, lib = _lib()
    n, hw, cin, cexp = 65535, 5, 16, 64
    case = Case("expdw images inside", "n=%d %dx%d %d->%d" % (n, hw, hw, cin, cexp))
    g = _gen(n + cexp)
    x = torch.randn(n, hw, hw, cin, dtype=torch.half, device=DEV, generator=g)
    w1 = (torch.randn(cexp, cin, device=DEV, generator=g) / cin ** 0.5).half()
    b1 = torch.randn(cexp, device=DEV, generator=g) * 0.1
    wd = (torch.randn(9, cexp, device=DEV, generator=g) / 3).half()
    bd = torch.randn(cexp, device=DEV, generator=g) * 0.1
    out = Out(n * hw * hw * cexp * 2)
    case.arrays = dict(x=x.numel() * 2, out=out.nbytes)
    L.check(lib.dn_expand_depthwise(_ptr(x), _ptr(w1), _ptr(b1), _ptr(wd), _ptr(bd), None, None, out.ptr, None, n, hw, hw, cin, cexp, 0, 3, 1, 1, 1, 0, _stream()),
            "dn_expand_depthwise")
    torch.cuda.synchronize()
    case.label = L.debug_last_kernel()
    assert case.label == "expdw_kernel<3,1,5,5,2,true,false>" and out.guards_intact()
    v = out.view(torch.half, n, hw, hw, cexp)
    for i0 in range(0, n, 1 << 14):
        e = F.relu(x[i0:i0 + (1 << 14)].float() @ w1.float().t() + b1).half()          # the expanded activation is rounded to fp16 where the unfused path stores it
        assert _unwritten(v[i0:i0 + (1 << 14)]) == 0
        case.whole = max(case.whole, _worst(v[i0:i0 + (1 << 14)].float(), _dw_ref_dev(e, wd, bd, 1, 0, hw).half().float(), 4e-3))
    for img in (0, n - 1):
        e = F.relu(x[img].cpu().double() @ w1.cpu().double().t() + b1.cpu().double()).half()[None]
        ref64 = _dw_ref_host(e, wd, bd, 1, 0, 0, hw).half().float()
        case.sampled = max(case.sampled, _worst(v[img].cpu().float(), ref64, 4e-3))
    case.finish()


def test_depthwise_refuses_more_image_slots_than_grid_y_holds(monkeypatch):
    """65536 images with DN_XCD=0: refused by the launcher, the error names the limit, nothing is written."""
    L, lib = _lib()
    monkeypatch.setenv("DN_XCD", "0")
    x = torch.zeros(1 << 20, dtype=torch.half, device=DEV)
    out = Out(1 << 20)
    rc = lib.dn_depthwise_conv(_ptr(x), _ptr(x), _ptr(x.view(torch.float)), out.ptr, 65536, 2, 2, 8, 3, 1, 1, 1, _stream())
    err = lib.dn_last_error().decode()
    torch.cuda.synchronize()
    assert rc == E_INVALID and "65535" in err and "grid.y" in err, (rc, err)
    assert out.untouched() and out.guards_intact()


# ---------------------------------------------------------------------------------------------------------------- grid and count refusals
def test_expand_depthwise_refuses_more_than_65535_images():
    L, lib = _lib()
    x = torch.zeros(1 << 16, dtype=torch.half, device=DEV)
    f = torch.zeros(1 << 12, device=DEV)
    out = Out(1 << 16)
    rc = lib.dn_expand_depthwise(_ptr(x), _ptr(x), _ptr(f), _ptr(x), _ptr(f), None, None, out.ptr, None, 65536, 5, 5, 16, 64, 0, 3, 1, 1, 1, 0, _stream())
    err = lib.dn_last_error().decode()
    torch.cuda.synchronize()
    assert rc == E_INVALID and "grid too large" in err, (rc, err)
    assert out.untouched() and out.guards_intact()


def test_crop_augment_and_sgd_refuse_counts_above_65535():
    L, lib = _lib()
    x = torch.zeros(1 << 12, device=DEV)
    out = Out(1 << 16)
    rc = lib.dn_crop_tiles(_ptr(x), 64, 64, _ptr(x), 65536, 8, 8, out.ptr, _stream())
    assert rc == E_INVALID and "65535" in lib.dn_last_error().decode()
    host = (C.c_void_p * 1)(x.data_ptr())
    sizes = (C.c_int32 * 2)(8, 8)
    params = (C.c_int32 * 64)()
    rc = lib.dn_augment_batch(host, sizes, params, 65536, 8, 8, out.ptr, _ptr(x), 1 << 12, _stream())
    assert rc == E_UNSUPPORTED and "65535" in lib.dn_last_error().decode()
    rc = lib.dn_sgd_step(_ptr(x), 65536, 1, L.SgdHyper(), None, 0, None, 0.0, out.ptr, _stream())
    assert rc == E_UNSUPPORTED and "65535" in lib.dn_last_error().decode()
    torch.cuda.synchronize()
    assert out.untouched() and out.guards_intact()


# ---------------------------------------------------------------------------------------------------------------- stems
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _stem_ref_dev(img, wmat, b, act, s, r0, r1):
    """fp32 on the device: output rows [r0, r1) of the 3 x 3 pad-1 stride-s stem on the normalised image (zero padding AFTER the normalisation), as a
    [pixels][27] patch matrix times the [27][cout] weights."""
    h, w = img.shape[1:]
    wo = (w - 1) // s + 1
    i0, i1 = r0 * s - 1, (r1 - 1) * s + 1
    lo, hi = max(i0, 0), min(i1, h - 1)
    mean, inv = torch.tensor(MEAN, device=DEV)[:, None, None], (1.0 / torch.tensor(STD, device=DEV))[:, None, None]
    xn = F.pad((img[:, lo:hi + 1] - mean) * inv, (1, 1, lo - i0, i1 - hi))
    rr = r1 - r0
    cols = [xn[c, ky:ky + s * (rr - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s] for c in range(3) for ky in range(3) for kx in range(3)]
    return _act(torch.stack(cols, -1) @ wmat + b, act)


def _stem_ref_host(img, wmat, b, act, s, r0, r1):
    """float64 on the host, through F.conv2d, from the band's input lines only."""
    h, w = img.shape[1:]
    i0, i1 = r0 * s - 1, (r1 - 1) * s + 1
    lo, hi = max(i0, 0), min(i1, h - 1)
    mean, inv = torch.tensor(MEAN, dtype=torch.float32)[:, None, None], (1.0 / torch.tensor(STD, dtype=torch.float32))[:, None, None]
    xn = ((img[:, lo:hi + 1].cpu() - mean) * inv).double()          # (the normalisation in fp32, as the kernels do it; everything behind it in float64)
    xn = F.pad(xn, (1, 1, lo - i0, i1 - hi))
    wt = wmat.cpu().double().t().reshape(-1, 3, 3, 3)
    return _act(F.conv2d(xn[None], wt, b.cpu().double(), s), act)[0].permute(1, 2, 0)


def _stem_case(name, h, w, cout, s, act, split_ok, label):
    import math
    L, lib = _lib()
    assert L.debug_choice("stem", 1, h, w, cout, s, 1, act, split_ok)["kernel"] == label.split("<")[0]
    case = Case(name, "%dx%d 3->%d stride %d" % (h, w, cout, s))
    g = _gen(h + w + cout)
    img = torch.rand(3, h, w, device=DEV, generator=g)
    wmat = torch.randn(27, cout, device=DEV, generator=g) / 27 ** 0.5
    b = torch.randn(cout, device=DEV, generator=g) * 0.1
    scale_log2 = 15 - math.frexp(max(float(wmat.abs().max()), float(b.abs().max())))[1]
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    out = Out(ho * wo * cout * 2)
    case.arrays = dict(image=img.numel() * 4, out=out.nbytes)
    mean3, std3 = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    L.check(lib.dn_debug_stem(_ptr(img), _ptr(wmat), _ptr(b), out.ptr, 1, h, w, cout, s, 1, act, mean3, std3, split_ok, scale_log2, _stream()), "dn_debug_stem")
    torch.cuda.synchronize()
    case.label = L.debug_last_kernel()
    assert case.label == label and out.guards_intact()
    v = out.view(torch.half, ho, wo, cout)
    band = max(1, PIX // wo)
    for r0 in range(0, ho, band):
        r1 = min(r0 + band, ho)
        assert _unwritten(v[r0:r1]) == 0
        case.whole = max(case.whole, _worst(v[r0:r1].float(), _stem_ref_dev(img, wmat, b, act, s, r0, r1).half().float(), 4e-3))
    # sampled bands: first and last lines, both sides of every 2^31 / 2^32-byte line of the output and (line of a plane -> output line) of the image
    rows = {0, ho - 1} | _line_rows(out.nbytes, wo * cout * 2) | {(r % h) // s for r in _line_rows(img.numel() * 4, w * 4)}
    bands = _bands(1, ho, {min(r, ho - 1) for r in rows}, False)
    for _, r0, r1 in bands:
        case.sampled = max(case.sampled, _worst(v[r0:r1].cpu().float(), _stem_ref_host(img, wmat, b, act, s, r0, r1).half().float(), 4e-3))
    case.note = "%d sampled bands" % len(bands)
    case.finish()


def test_stem_split_at_its_image_descriptor_limit_inside():
    """stem_split_kernel<16,2>: the image as a raw buffer of 3 h w 4 = 2^30 - 65 536 bytes (3 h w < 2^28)."""
    _stem_case("stem split image inside", 10922, 8192, 16, 2, 3, 1, "stem_split_kernel<16,2>")


def test_stem_split_at_its_image_descriptor_limit_outside():
    """One image line more: stem3s2_kernel (64-bit plane and line bases)."""
    _stem_case("stem split image outside", 10923, 8192, 16, 2, 3, 1, "stem3s2_kernel<16>")


def test_stem_split_at_its_output_descriptor_limit_inside():
    """stem_split_kernel<64,1>: the output as a raw buffer of ho wo 64 2 = 2^30 - 2^19 bytes (ho wo cout < 2^29)."""
    _stem_case("stem split out inside", 2047, 4096, 64, 1, 1, 1, "stem_split_kernel<64,1>")


def test_stem_split_at_its_output_descriptor_limit_outside():
    """One image line more: the fp32 matrix-core stem, pipelined form."""
    _stem_case("stem split out outside", 2048, 4096, 64, 1, 1, 1, "stem_mfma64p_kernel")


def test_stem_pipelined_at_its_output_descriptor_limit_inside():
    """stem_mfma64p_kernel: the output as a raw buffer of h w 128 = 2^31 - 2^19 bytes (h w < 2^24)."""
    _stem_case("stem pipe out inside", 4095, 4096, 64, 1, 1, 0, "stem_mfma64p_kernel")


def test_stem_pipelined_at_its_output_descriptor_limit_outside():
    """Two image lines more: stem_mfma64_kernel (64-bit output offsets); the output crosses the 2^31-byte line at line 4096.
    (The limit of that kernel itself, 3 h w < 2^30, needs an output of 45 GB: CPU case only.)"""
    _stem_case("stem pipe out outside", 4097, 4096, 64, 1, 1, 0, "stem_mfma64_kernel")


# ---------------------------------------------------------------------------------------------------------------- one model-level case
def _plan_labels(m, imgs):
    """per op: the label of the launch it took part in (dn_profile_op_info after one profiled forward_batch)"""
    from demonet_amd import _lib
    L = _lib.lib()
    h = C.c_void_p(m._plan(imgs.device))
    _lib.check(L.dn_profile_begin(h))
    m.forward_batch(imgs, persistent_input=True)
    nseg = len(m.graph.nodes) + 4
    _lib.check(L.dn_profile_end(h, (C.c_float * nseg)(), nseg))
    label, owner, out = C.create_string_buffer(96), C.c_int32(), []
    for i in range(len(m.graph.nodes)):
        _lib.check(L.dn_profile_op_info(h, i, label, 96, C.byref(owner)))
        out.append(label.value.decode())
    torch.cuda.synchronize()
    m._bufs.clear()                  # (the workspace of this batch shape)
    torch.cuda.empty_cache()
    return out


def test_model_batch_past_the_run_staged_tile_limit():
    """ssd300_vgg16 in one chain: conv2_2 (128 -> 128 on 150 x 150) is the first launch of any plan of the zoo, at its default size, that an
    addressing guard moves (7.8 GB of workspace, against 14.2 GB for ssdlite320_mobilenet_v3_large at 2331 images and 15.4 GB for
    ssd512_vgg16 at 256) -- at 373 images its input is 2^31 + 996 352 bytes and conv_halo_kernel<3,8,2> gives way to conv_patch_kernel. The
    head outputs of every image of the 373-image batch agree with the same images run in batches of 8 within the tolerance between kernel
    variants of tests/test_gpu_model.py."""
    from demonet_amd import _lib, models
    LOGIT_ATOL, LOGIT_RTOL = 6e-2, 1e-2
    N = 373
    case = Case("model ssd300 one chain", "n=%d against batches of 8" % N)
    dev = torch.device("cuda:0")
    m = models.load_synthetic(models.ssd300_vgg16(num_classes=91), 0).to(dev)
    op = next(i for i, nd in enumerate(m.graph.nodes) if nd.op == "conv" and nd.cin == 128 and nd.cout == 128 and m.graph.t(nd.out).h == 150)
    imgs = torch.rand(N, 3, 300, 300, device=dev, generator=_gen(N))
    h = C.c_void_p(m._plan(dev))
    _lib.check(_lib.lib().dn_set_chains(h, 1))
    small, inside, outside = _plan_labels(m, imgs[:8]), _plan_labels(m, imgs[:N - 1]), _plan_labels(m, imgs)
    print("labels that differ between %d and %d images:" % (N - 1, N), [(i, a, b) for i, (a, b) in enumerate(zip(inside, outside)) if a != b])
    assert small[op] == inside[op] == "conv_halo_kernel<3,8,2>" and outside[op] == "conv_patch_kernel", (small[op], inside[op], outside[op])
    case.label = outside[op]
    case.arrays = dict(workspace=int(_lib.lib().dn_workspace_bytes(h, N)), images=imgs.numel() * 4)
    logits, reg = m.forward_heads(imgs)
    m._bufs.clear()
    torch.cuda.empty_cache()
    for i0 in range(0, N, 8):
        lo, rg = m.forward_heads(imgs[i0:i0 + 8].contiguous())
        for got, ref in ((logits[i0:i0 + 8], lo), (reg[i0:i0 + 8], rg)):
            r = (got - ref).abs() / (LOGIT_ATOL + LOGIT_RTOL * ref.abs())
            case.whole = max(case.whole, float(torch.nan_to_num(r, nan=float("inf")).max()))
    case.note = "whole = worst |big - small| / (LOGIT_ATOL + LOGIT_RTOL |small|) over both head arrays"
    case.finish()


def test_forward_refuses_a_chain_of_two_to_the_31_rows():
    """int m = n * hw in the launchers: dn_forward_heads refuses 20 965 images of 320 x 320 in one chain ((n + 7) 102 400 = 2^31 + 49 152 rows with the
    XCD rounding) before it looks at the workspace or launches anything, and takes the question for 20 964 (whose workspace is then too small)."""
    from demonet_amd import _lib, models
    dev = torch.device("cuda:0")
    m = models.load_synthetic(models.ssdlite320_mobilenet_v3_large(num_classes=91), 0).to(dev)
    L = _lib.lib()
    h = C.c_void_p(m._plan(dev))
    _lib.check(L.dn_set_chains(h, 1))
    img, ws = torch.zeros(1 << 12, device=dev), Out(1 << 16)
    rc = L.dn_forward_heads(h, _ptr(img), 20965, 320, 320, ws.ptr, ws.nbytes, _stream())
    assert rc == E_INVALID and "2^31 rows" in L.dn_last_error().decode(), (rc, L.dn_last_error())
    rc = L.dn_forward_heads(h, _ptr(img), 20964, 320, 320, ws.ptr, ws.nbytes, _stream())
    assert rc == -3 and "workspace" in L.dn_last_error().decode(), (rc, L.dn_last_error())         # DN_E_WORKSPACE
    torch.cuda.synchronize()
    assert ws.untouched() and ws.guards_intact()
