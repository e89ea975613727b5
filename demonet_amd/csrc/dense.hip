// VGG-path helpers and input resize: max-pool, L2-normalise x scale, bilinear resize. The dense kxk convolution
// itself is the implicit-GEMM instantiation of the MFMA kernel in pointwise.hip.
//
// reference ops replaced: nn.MaxPool2d (ssd_vgg16.py:34-37,85), F.normalize * scale_weight (ssd_vgg16.py:101),
//   F.interpolate(mode='bilinear', align_corners=False) (transform.py:52-53).
#include "common.h"
#include "frametap.h"

namespace {

__global__ __launch_bounds__(256) void maxpool_kernel(const half_t* __restrict__ x, half_t* __restrict__ out, int n, int h, int w,
                                                     int c, int k, int stride, int pad, int ho, int wo) {
    const int C8 = c >> 3;
    long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int cg = (int)(idx % C8);
    idx /= C8;
    const int ox = (int)(idx % wo);
    idx /= wo;
    const int oy = (int)(idx % ho);
    const int nn = (int)(idx / ho);
    if (nn >= n) return;
    float m[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
    for (int ky = 0; ky < k; ++ky) {
        const int iy = oy * stride - pad + ky;
        if (iy < 0 || iy >= h) continue;
        for (int kx = 0; kx < k; ++kx) {
            const int ix = ox * stride - pad + kx;
            if (ix < 0 || ix >= w) continue;
            const half8 v = *reinterpret_cast<const half8*>(x + ((size_t)(nn * h + iy) * w + ix) * c + cg * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], (float)v[e]);
        }
    }
    half8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)m[e];
    *reinterpret_cast<half8*>(out + ((size_t)(nn * ho + oy) * wo + ox) * c + cg * 8) = o;
}

// one wave per pixel: x / max(||x||_2, 1e-12) * scale[c]
__global__ __launch_bounds__(256) void l2norm_kernel(const half_t* __restrict__ x, const float* __restrict__ scale,
                                                    half_t* __restrict__ out, long pixels, int c) {
    const int lane = threadIdx.x & 63;
    const long px = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (px >= pixels) return;
    const half_t* p = x + (size_t)px * c;
    float ss = 0.f;
    for (int c0 = lane * 8; c0 < c; c0 += 512) {
        const half8 v = *reinterpret_cast<const half8*>(p + c0);
#pragma unroll
        for (int e = 0; e < 8; ++e) ss += (float)v[e] * (float)v[e];
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) ss += __shfl_xor(ss, d);
    const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
    for (int c0 = lane * 8; c0 < c; c0 += 512) {
        const half8 v = *reinterpret_cast<const half8*>(p + c0);
        half8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)v[e] * inv * scale[c0 + e]);
        *reinterpret_cast<half8*>(out + (size_t)px * c + c0) = o;
    }
}

__global__ __launch_bounds__(256) void resize_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                    float* __restrict__ scale_xy, int planes, int h, int w, int oh, int ow) {
    long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < planes / 3) {      // one entry per image
        if (scale_xy) {
            scale_xy[2 * idx] = (float)w / (float)ow;
            scale_xy[2 * idx + 1] = (float)h / (float)oh;
        }
    }
    const int ox = (int)(idx % ow);
    idx /= ow;
    const int oy = (int)(idx % oh);
    const long pl = idx / oh;
    if (pl >= planes) return;
    const float rh = (float)h / (float)oh, rw = (float)w / (float)ow;
    const float sy = fmaxf(rh * ((float)oy + 0.5f) - 0.5f, 0.f);
    const float sx = fmaxf(rw * ((float)ox + 0.5f) - 0.5f, 0.f);
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly = fminf(fmaxf(sy - (float)y0, 0.f), 1.f), lx = fminf(fmaxf(sx - (float)x0, 0.f), 1.f);
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float* p = in + (size_t)pl * h * w;
    out[((size_t)pl * oh + oy) * ow + ox] = bilerp(p[(size_t)y0 * w + x0], p[(size_t)y0 * w + x1], p[(size_t)y1 * w + x0],
                                                   p[(size_t)y1 * w + x1], hx, lx, hy, ly);
}


// Decoder output straight into the network input: [n][h][w][3] uint8 (HWC, RGB) -> x/255 (ToTensor) -> bilinear resize to the
// network size (transform.py:27-53, align_corners=False; same arithmetic as resize_kernel) -> [n][3][oh][ow] fp32 planes.
// With (h, w) == (oh, ow) the interpolation weights are exactly (1, 0): a plain conversion.
__global__ __launch_bounds__(256) void u8hwc_kernel(const unsigned char* __restrict__ in, float* __restrict__ out,
                                                    float* __restrict__ scale_xy, int n, int h, int w, int oh, int ow) {
    long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < n && scale_xy) {
        scale_xy[2 * idx] = (float)w / (float)ow;
        scale_xy[2 * idx + 1] = (float)h / (float)oh;
    }
    const int ox = (int)(idx % ow);
    idx /= ow;
    const int oy = (int)(idx % oh);
    const long img = idx / oh;
    if (img >= n) return;
    const float rh = (float)h / (float)oh, rw = (float)w / (float)ow;
    const float sy = fmaxf(rh * ((float)oy + 0.5f) - 0.5f, 0.f);
    const float sx = fmaxf(rw * ((float)ox + 0.5f) - 0.5f, 0.f);
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly = fminf(fmaxf(sy - (float)y0, 0.f), 1.f), lx = fminf(fmaxf(sx - (float)x0, 0.f), 1.f);
    const float hy = 1.f - ly, hx = 1.f - lx;
    const unsigned char* p = in + (size_t)img * h * w * 3;
    const unsigned char* p00 = p + ((size_t)y0 * w + x0) * 3;
    const unsigned char* p01 = p + ((size_t)y0 * w + x1) * 3;
    const unsigned char* p10 = p + ((size_t)y1 * w + x0) * 3;
    const unsigned char* p11 = p + ((size_t)y1 * w + x1) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = (float)p00[c] / 255.f, b = (float)p01[c] / 255.f, cc = (float)p10[c] / 255.f, d = (float)p11[c] / 255.f;
        out[(((size_t)img * 3 + c) * oh + oy) * ow + ox] = bilerp(a, b, cc, d, hx, lx, hy, ly);
    }
}

// Video surfaces straight into the network input (dn_forward_frames, include/demonet_hip.h): one dn_frame record per image, read from
// DEVICE memory at run time, every image with its own planes, pitches and size. Each of the four bilinear taps is converted to 8-bit RGB in
// integer arithmetic as it is read (1 luma + 2 chroma bytes; chroma sample (x >> 1, y >> 1)); from there on the arithmetic is u8hwc_kernel's,
// expression for expression, so the block equals what u8hwc_kernel writes from the converted frame, bit for bit.
// (FrameColor, frame_tap and bilerp: frametap.h, shared with crops.hip)
template <int FMT>
__global__ __launch_bounds__(256) void frames_kernel(const dn_frame* __restrict__ frames, float* __restrict__ out, float* __restrict__ scale_xy,
                                                     int n, int oh, int ow, FrameColor k) {
    long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int ox = (int)(idx % ow);
    idx /= ow;
    const int oy = (int)(idx % oh);
    const long img = idx / oh;
    if (img >= n) return;
    const dn_frame f = frames[img];
    const int h = f.height, w = f.width;
    if (ox == 0 && oy == 0) {       // always: a ratio of exactly 1 maps the boxes back unchanged
        scale_xy[2 * img] = (float)w / (float)ow;
        scale_xy[2 * img + 1] = (float)h / (float)oh;
    }
    const float rh = (float)h / (float)oh, rw = (float)w / (float)ow;
    const float sy = fmaxf(rh * ((float)oy + 0.5f) - 0.5f, 0.f);
    const float sx = fmaxf(rw * ((float)ox + 0.5f) - 0.5f, 0.f);
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly = fminf(fmaxf(sy - (float)y0, 0.f), 1.f), lx = fminf(fmaxf(sx - (float)x0, 0.f), 1.f);
    const float hy = 1.f - ly, hx = 1.f - lx;
    float a[3], b[3], cc[3], d[3];
    frame_tap<FMT>(f, x0, y0, k, a);
    frame_tap<FMT>(f, x1, y0, k, b);
    frame_tap<FMT>(f, x0, y1, k, cc);
    frame_tap<FMT>(f, x1, y1, k, d);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        out[(((size_t)img * 3 + c) * oh + oy) * ow + ox] = bilerp(a[c], b[c], cc[c], d[c], hx, lx, hy, ly);
}

// Regions of video surfaces (dn_forward_regions): network image i is the rectangle regions[i] of frames[regions[i].frame], mirrored left-right
// when flagged. frames_kernel's arithmetic in REGION coordinates (the second tap clamps at the region's edge); a tap at region pixel (xr, yr)
// reads frame pixel (r.x0 + (flip ? w - 1 - xr : xr), r.y0 + yr) through frame_tap, so chroma is sampled in frame coordinates. A region of
// exactly the network size has sy = oy, sx = ox and weights (1, 0): bilerp returns its first tap unchanged (1 * a + 0 * b = a for the
// finite, non-negative taps), so that case reads one tap -- the tiles of sliced inference at the default tile size.
template <int FMT>
__global__ __launch_bounds__(256) void frame_regions_kernel(const dn_frame* __restrict__ frames, const dn_region* __restrict__ regions,
                                                            float* __restrict__ out, float* __restrict__ scale_xy, int n, int oh, int ow, FrameColor k) {
    long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int ox = (int)(idx % ow);
    idx /= ow;
    const int oy = (int)(idx % oh);
    const long img = idx / oh;
    if (img >= n) return;
    const dn_region r = regions[img];
    const dn_frame f = frames[r.frame];
    const int h = r.height, w = r.width;
    const bool flip = (r.flags & DN_REGION_HFLIP) != 0;
    if (ox == 0 && oy == 0) {
        scale_xy[2 * img] = (float)w / (float)ow;
        scale_xy[2 * img + 1] = (float)h / (float)oh;
    }
    float* o = out + ((size_t)img * 3 * oh + oy) * ow + ox;
    const size_t plane = (size_t)oh * ow;
    if (h == oh && w == ow) {
        float a[3];
        frame_tap<FMT>(f, r.x0 + (flip ? w - 1 - ox : ox), r.y0 + oy, k, a);
        o[0] = a[0]; o[plane] = a[1]; o[2 * plane] = a[2];
        return;
    }
    const float rh = (float)h / (float)oh, rw = (float)w / (float)ow;
    const float sy = fmaxf(rh * ((float)oy + 0.5f) - 0.5f, 0.f);
    const float sx = fmaxf(rw * ((float)ox + 0.5f) - 0.5f, 0.f);
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly = fminf(fmaxf(sy - (float)y0, 0.f), 1.f), lx = fminf(fmaxf(sx - (float)x0, 0.f), 1.f);
    const float hy = 1.f - ly, hx = 1.f - lx;
    const int X0 = r.x0 + (flip ? w - 1 - x0 : x0), X1 = r.x0 + (flip ? w - 1 - x1 : x1);
    const int Y0 = r.y0 + y0, Y1 = r.y0 + y1;
    float a[3], b[3], cc[3], d[3];
    frame_tap<FMT>(f, X0, Y0, k, a);
    frame_tap<FMT>(f, X1, Y0, k, b);
    frame_tap<FMT>(f, X0, Y1, k, cc);
    frame_tap<FMT>(f, X1, Y1, k, d);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = bilerp(a[c], b[c], cc[c], d[c], hx, lx, hy, ly);
}

}  // namespace

int launch_maxpool(const half_t* x, half_t* out, int n, int h, int w, int c, int k, int stride, int pad, int ho, int wo,
                   hipStream_t s) {
    DN_REQUIRE(c % 8 == 0, "maxpool: c=%d must be a multiple of 8", c);
    const long threads = (long)n * ho * wo * (c / 8);
    dn_note_kernel("maxpool_kernel");
    hipLaunchKernelGGL(maxpool_kernel, dim3(dn_cdiv(threads, 256)), dim3(256), 0, s, x, out, n, h, w, c, k, stride, pad, ho, wo);
    return DN_OK;
}

int launch_l2norm(const half_t* x, const float* scale, half_t* out, long pixels, int c, hipStream_t s) {
    DN_REQUIRE(c % 8 == 0, "l2norm: c=%d must be a multiple of 8", c);
    dn_note_kernel("l2norm_kernel");
    hipLaunchKernelGGL(l2norm_kernel, dim3(dn_cdiv(pixels, 4)), dim3(256), 0, s, x, scale, out, pixels, c);
    return DN_OK;
}

int launch_resize_bilinear(const float* in, float* out, float* scale_xy, int n, int h, int w, int oh, int ow, hipStream_t s) {
    const long threads = (long)n * 3 * oh * ow;
    hipLaunchKernelGGL(resize_kernel, dim3(dn_cdiv(threads, 256)), dim3(256), 0, s, in, out, scale_xy, n * 3, h, w, oh, ow);
    return DN_OK;
}

int launch_u8hwc_to_planar(const unsigned char* in, float* out, float* scale_xy, int n, int h, int w, int oh, int ow, hipStream_t s) {
    const long threads = (long)n * oh * ow;
    dn_note_kernel("u8hwc_kernel");
    hipLaunchKernelGGL(u8hwc_kernel, dim3(dn_cdiv(threads, 256)), dim3(256), 0, s, in, out, scale_xy, n, h, w, oh, ow);
    return DN_OK;
}

bool dn_frame_codes_known(int format, int color) {
    FrameColor k;
    return format >= DN_FRAME_NV12 && format <= DN_FRAME_BGR24 && color >= 0 && frame_color(color, &k);
}

int launch_frames_to_planar(const dn_frame* frames, int format, int color, float* out, float* scale_xy, int n, int oh, int ow, hipStream_t s) {
    FrameColor k;
    if (!dn_frame_codes_known(format, color) || !frame_color(color, &k)) {
        dn_set_error("frames: unknown format %d or colour code 0x%x", format, color);
        return DN_E_UNSUPPORTED;
    }
    const long threads = (long)n * oh * ow;
    const dim3 grid(dn_cdiv(threads, 256)), block(256);
    dn_note_kernel("frames_kernel<%d>", format);
    switch (format) {
        case DN_FRAME_NV12: hipLaunchKernelGGL(frames_kernel<DN_FRAME_NV12>, grid, block, 0, s, frames, out, scale_xy, n, oh, ow, k); break;
        case DN_FRAME_I420: hipLaunchKernelGGL(frames_kernel<DN_FRAME_I420>, grid, block, 0, s, frames, out, scale_xy, n, oh, ow, k); break;
        case DN_FRAME_RGB24: hipLaunchKernelGGL(frames_kernel<DN_FRAME_RGB24>, grid, block, 0, s, frames, out, scale_xy, n, oh, ow, k); break;
        default: hipLaunchKernelGGL(frames_kernel<DN_FRAME_BGR24>, grid, block, 0, s, frames, out, scale_xy, n, oh, ow, k); break;
    }
    return DN_OK;
}

int launch_regions_to_planar(const dn_frame* frames, const dn_region* regions, int format, int color, float* out, float* scale_xy, int n, int oh,
                             int ow, hipStream_t s) {
    FrameColor k;
    if (!dn_frame_codes_known(format, color) || !frame_color(color, &k)) {
        dn_set_error("regions: unknown format %d or colour code 0x%x", format, color);
        return DN_E_UNSUPPORTED;
    }
    const long threads = (long)n * oh * ow;
    const dim3 grid(dn_cdiv(threads, 256)), block(256);
    dn_note_kernel("frame_regions_kernel<%d>", format);
    switch (format) {
        case DN_FRAME_NV12: hipLaunchKernelGGL(frame_regions_kernel<DN_FRAME_NV12>, grid, block, 0, s, frames, regions, out, scale_xy, n, oh, ow, k); break;
        case DN_FRAME_I420: hipLaunchKernelGGL(frame_regions_kernel<DN_FRAME_I420>, grid, block, 0, s, frames, regions, out, scale_xy, n, oh, ow, k); break;
        case DN_FRAME_RGB24: hipLaunchKernelGGL(frame_regions_kernel<DN_FRAME_RGB24>, grid, block, 0, s, frames, regions, out, scale_xy, n, oh, ow, k); break;
        default: hipLaunchKernelGGL(frame_regions_kernel<DN_FRAME_BGR24>, grid, block, 0, s, frames, regions, out, scale_xy, n, oh, ow, k); break;
    }
    return DN_OK;
}


// ---- DN_POISON (correctness tooling, tests/test_gpu_pipeline.py::test_results_do_not_depend_on_stale_lds_or_registers): a launch that
// leaves NaN patterns in every LDS byte and every vector register (VGPR and AGPR) of the compute units it lands on. plan.hip puts one in
// front of every launch of a forward when the knob is set: a kernel that reads LDS or a register it has not written itself then
// produces a different (NaN) result than in an undisturbed run. One 256-thread workgroup takes a whole CU (160 KB of LDS, 512
// registers per lane: one wave per SIMD); 1024 of them pass over every CU.
__global__ __launch_bounds__(256, 1) void poison_kernel(unsigned* sink) {
    extern __shared__ unsigned poison_lds[];
    for (int i = threadIdx.x; i < 160 * 1024 / 4; i += 256) poison_lds[i] = 0x7fc0dead;
    unsigned v = 0x7fc0dead;
    // every architectural VGPR and AGPR of the wave
#define PZ4(b) "v_mov_b32 v" #b ", %0\n\tv_accvgpr_write_b32 a" #b ", %0\n\t"
#define PZ(n) asm volatile("v_mov_b32 v" #n ", %0\n\tv_accvgpr_write_b32 a" #n ", %0" :: "v"(v) : "v" #n, "a" #n);
#define PZ8(a, b, c, d, e, f, g, h) PZ(a) PZ(b) PZ(c) PZ(d) PZ(e) PZ(f) PZ(g) PZ(h)
    PZ8(8, 9, 10, 11, 12, 13, 14, 15) PZ8(16, 17, 18, 19, 20, 21, 22, 23) PZ8(24, 25, 26, 27, 28, 29, 30, 31)
    PZ8(32, 33, 34, 35, 36, 37, 38, 39) PZ8(40, 41, 42, 43, 44, 45, 46, 47) PZ8(48, 49, 50, 51, 52, 53, 54, 55) PZ8(56, 57, 58, 59, 60, 61, 62, 63)
    PZ8(64, 65, 66, 67, 68, 69, 70, 71) PZ8(72, 73, 74, 75, 76, 77, 78, 79) PZ8(80, 81, 82, 83, 84, 85, 86, 87) PZ8(88, 89, 90, 91, 92, 93, 94, 95)
    PZ8(96, 97, 98, 99, 100, 101, 102, 103) PZ8(104, 105, 106, 107, 108, 109, 110, 111) PZ8(112, 113, 114, 115, 116, 117, 118, 119)
    PZ8(120, 121, 122, 123, 124, 125, 126, 127) PZ8(128, 129, 130, 131, 132, 133, 134, 135) PZ8(136, 137, 138, 139, 140, 141, 142, 143)
    PZ8(144, 145, 146, 147, 148, 149, 150, 151) PZ8(152, 153, 154, 155, 156, 157, 158, 159) PZ8(160, 161, 162, 163, 164, 165, 166, 167)
    PZ8(168, 169, 170, 171, 172, 173, 174, 175) PZ8(176, 177, 178, 179, 180, 181, 182, 183) PZ8(184, 185, 186, 187, 188, 189, 190, 191)
    PZ8(192, 193, 194, 195, 196, 197, 198, 199) PZ8(200, 201, 202, 203, 204, 205, 206, 207) PZ8(208, 209, 210, 211, 212, 213, 214, 215)
    PZ8(216, 217, 218, 219, 220, 221, 222, 223) PZ8(224, 225, 226, 227, 228, 229, 230, 231) PZ8(232, 233, 234, 235, 236, 237, 238, 239)
    PZ8(240, 241, 242, 243, 244, 245, 246, 247) PZ8(248, 249, 250, 251, 252, 253, 254, 255)
#undef PZ8
#undef PZ
#undef PZ4
    __syncthreads();
    if (sink && poison_lds[threadIdx.x] == 1u) sink[0] = v;      // (keeps the LDS stores alive; never true)
}

int launch_poison(hipStream_t s) {
    DN_HIP_CHECK(dn_allow_big_lds(reinterpret_cast<const void*>(poison_kernel)));
    hipLaunchKernelGGL(poison_kernel, dim3(1024), dim3(256), 160 * 1024, s, (unsigned*)nullptr);
    return DN_OK;
}
