// Backward through one SSDLite head of one pyramid level: gradients of the folded head parameters.
//
// Differentiates   depthwise 3x3 + BN + ReLU6 -> 1x1 conv with bias   (reference: ssd_mobilenetv3.py:27-36; the V2 hub model's
// MultiBoxLiteHead, box_head.py:24-56, whose last level is a bare 1x1: wd == NULL below). With x the level's feature map
// [n][h][w][c] fp16, the folded weights the forward used (wd' [9][c] fp16, bd' [c] fp32, W1' [cout][c] fp16) and dy the fp32
// gradient of the head output, read IN PLACE from the [n][A][K] / [n][A][4] gradient tensor (row of pixel p of image i at
// i * dy_img_stride + p * cout, as the forward's fp32 head epilogue addresses it):
//
//   z  = wd' (*) x + bd'          fp32, recomputed (the fused head launch never stores it)        hg_prep_kernel
//   h  = fp16(min(max(z, 0), 6))  what the forward's 1x1 consumed; mask = 0 < z < 6, one byte    hg_prep_kernel
//   g_b1[o]    = sum_p dy[p][o]                       fp32 sums of the unrounded dy              hg_w1_kernel (staging threads)
//   g_W1[o][c] = sum_p dy[p][o] * h[p][c]             v_mfma_f32_32x32x16_f16, K = pixels        hg_w1_kernel
//   dh[p][c]   = sum_o dy[p][o] * W1'[o][c]           v_mfma_f32_32x32x16_f16, K = cout          hg_dz_kernel
//   dz         = dh where mask, else 0                in the accumulators, never stored          hg_dz_kernel epilogue
//   g_bd[c]    = sum_p dz[p][c],  g_wd[t][c] = sum_p dz[p][c] * x[p + t][c]                      hg_dz_kernel epilogue
//
// Small gradients. dy is a softmax gradient divided by the number of foreground anchors: most of it lies below fp16's normal
// range. The matrix operand is therefore fp16(dy * 2^k) with ONE power of two per call, taken on the device from max|dy| over the
// call's rows (hg_max_kernel: per-workgroup maxima, no atomics, no host synchronisation) so that the largest magnitude lands in
// [2^13, 2^14); the fp32 epilogues multiply by 2^-k, which is exact. Values more than 2^27 below the maximum become fp16
// subnormals (absolute error <= 2^-25 * 2^-k each), which tests/head_grad_ref.py carries as its own term.
//
// Determinism. No atomics anywhere. The pixel reduction of g_W1 / g_b1 is split over gridDim.z chunks, that of g_wd / g_bd over the
// 64-pixel tiles; every workgroup writes its partial sums to its own slot of the workspace and hg_reduce_kernel adds the slots
// in index order. Within a workgroup every sum has a fixed order too, so two runs give the same bits.
//
// Bounds. Every global access is guarded by (pixel < P, channel < c, output < cout); tiles are 64 wide on every axis and the
// ragged edges contribute zeros to the MFMA operands.
#include "common.h"
#include <math.h>

namespace {

constexpr int HG_MAXBLK = 128;       // workgroups (= partial maxima) of hg_max_kernel
constexpr int HG_LD = 40;            // LDS row stride in halfs of a [64][32] operand tile: 80 bytes keeps the 16-byte fragment reads aligned
constexpr int HG_MAX_SPLIT = 16;

struct HgShape {
    int n, h, w, c, cout, hw, P;
    long dy_img_stride;
};

// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hg_max_kernel(const float* __restrict__ dy, HgShape s, float* __restrict__ maxpart) {
    __shared__ float red[256];
    const size_t per_img = (size_t)s.hw * s.cout, total = per_img * s.n;
    float m = 0.f;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t img = e / per_img, rem = e - img * per_img;
        const float v = fabsf(dy[img * (size_t)s.dy_img_stride + rem]);
        m = (v < INFINITY && v > m) ? v : m;      // NaN and inf do not steer the scale
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + st]);
        __syncthreads();
    }
    if (threadIdx.x == 0) maxpart[blockIdx.x] = red[0];
}

// 2^k with max|dy| * 2^k in [2^13, 2^14) (k clamped so that 2^k and 2^-k are normal floats); all threads of the workgroup call it
__device__ __forceinline__ void hg_scale(const float* __restrict__ maxpart, float* sh, float& scale, float& unscale) {
    if (threadIdx.x < HG_MAXBLK) sh[threadIdx.x] = maxpart[threadIdx.x];
    __syncthreads();
    float m = 0.f;
    for (int i = 0; i < HG_MAXBLK; ++i) m = fmaxf(m, sh[i]);
    int k = 0;
    if (m > 0.f) {
        int e;
        frexpf(m, &e);                      // m = f * 2^e, f in [0.5, 1)
        k = 14 - e;
        k = k > 120 ? 120 : (k < -100 ? -100 : k);
    }
    scale = ldexpf(1.f, k);
    unscale = ldexpf(1.f, -k);
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------------------------------------
// z, h and the ReLU6 mask of every (pixel, channel): one thread per pixel and 8 channels. Taps in (ky, kx) order, fp32 fma.
__global__ __launch_bounds__(256) void hg_prep_kernel(const half_t* __restrict__ x, const half_t* __restrict__ wd, const float* __restrict__ bd,
                                                      HgShape s, half_t* __restrict__ hbuf, unsigned char* __restrict__ mask) {
    const int c8 = s.c >> 3;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)s.P * c8) return;
    const int p = (int)(idx / c8), g = (int)(idx - (size_t)p * c8);
    const int img = p / s.hw, pix = p - img * s.hw, y = pix / s.w, xx = pix - y * s.w;
    float z[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = bd[g * 8 + j];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int yy = y + ky - 1, xc = xx + kx - 1;
            if (yy < 0 || yy >= s.h || xc < 0 || xc >= s.w) continue;
            const half8 xv = *reinterpret_cast<const half8*>(x + ((size_t)(img * s.h + yy) * s.w + xc) * s.c + g * 8);
            const half8 wv = *reinterpret_cast<const half8*>(wd + (size_t)(ky * 3 + kx) * s.c + g * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) z[j] = fmaf((float)xv[j], (float)wv[j], z[j]);
        }
    half8 hv;
    unsigned char mk[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        hv[j] = (half_t)fminf(fmaxf(z[j], 0.f), 6.f);
        mk[j] = (z[j] > 0.f && z[j] < 6.f) ? 1 : 0;
    }
    *reinterpret_cast<half8*>(hbuf + (size_t)p * s.c + g * 8) = hv;
    uint2 mv;
    mv.x = mk[0] | (mk[1] << 8) | (mk[2] << 16) | ((unsigned)mk[3] << 24);
    mv.y = mk[4] | (mk[5] << 8) | (mk[6] << 16) | ((unsigned)mk[7] << 24);
    *reinterpret_cast<uint2*>(mask + (size_t)p * s.c + g * 8) = mv;
}

// ------------------------------------------------------------------------------------------------------------------------------
// g_W1 / g_b1 partials of one pixel chunk: C[o][c] = sum_p dy[p][o] h[p][c]. Workgroup tile 64 (o) x 64 (c), four waves of 32 x 32,
// K = 32 pixels per stage. grid (c tiles, o tiles, chunks). Each thread gathers, for ONE output o (and one channel c), the 8
// consecutive pixels of a fragment's k run: the loads of a wave are 64 consecutive floats (halfs) of a dy (h) row.
__global__ __launch_bounds__(256) void hg_w1_kernel(const float* __restrict__ dy, const half_t* __restrict__ hbuf, HgShape s,
                                                    const float* __restrict__ maxpart, int chunk, float* __restrict__ w1out,
                                                    float* __restrict__ b1out) {
    __shared__ __attribute__((aligned(16))) half_t As[64 * HG_LD];
    __shared__ __attribute__((aligned(16))) half_t Bs[64 * HG_LD];
    __shared__ float red[256];
    float scale, unscale;
    hg_scale(maxpart, red, scale, unscale);
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wr = wv >> 1, wc = wv & 1, r = lane & 31, hh = lane >> 5;
    const int c0 = blockIdx.x * 64, o0 = blockIdx.y * 64;
    const int p_begin = blockIdx.z * chunk, p_end = min(s.P, p_begin + chunk);
    const int oo = t & 63, kq = t >> 6;
    const int o = o0 + oo, cc = c0 + oo;
    const bool o_ok = o < s.cout, c_ok = cc < s.c;
    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    float bsum = 0.f;
    for (int p0 = p_begin; p0 < p_end; p0 += 32) {
        half8 av, bv;
        const int pb = p0 + kq * 8;
        int img = pb / s.hw, pix = pb - img * s.hw;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int p = pb + i;
            float v = 0.f;
            half_t hv = (half_t)0.f;
            if (p < p_end) {
                if (o_ok) v = dy[(size_t)img * (size_t)s.dy_img_stride + (size_t)pix * s.cout + o];
                if (c_ok) hv = hbuf[(size_t)p * s.c + cc];
            }
            bsum += v;
            av[i] = (half_t)(v * scale);
            bv[i] = hv;
            if (++pix == s.hw) { pix = 0; ++img; }
        }
        __syncthreads();
        *reinterpret_cast<half8*>(&As[oo * HG_LD + kq * 8]) = av;
        *reinterpret_cast<half8*>(&Bs[oo * HG_LD + kq * 8]) = bv;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const half8 a = *reinterpret_cast<const half8*>(&As[(wr * 32 + r) * HG_LD + kk * 16 + 8 * hh]);
            const half8 b = *reinterpret_cast<const half8*>(&Bs[(wc * 32 + r) * HG_LD + kk * 16 + 8 * hh]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
        }
    }
    // C row = (reg & 3) + 8 (reg >> 2) + 4 hh, column = r
    const int col = c0 + wc * 32 + r;
    float* dst = w1out + (size_t)blockIdx.z * s.cout * s.c;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = o0 + wr * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
        if (row < s.cout && col < s.c) dst[(size_t)row * s.c + col] = acc[i] * unscale;
    }
    __syncthreads();
    red[t] = bsum;
    __syncthreads();
    if (blockIdx.x == 0 && t < 64 && o_ok) b1out[(size_t)blockIdx.z * s.cout + o] = ((red[t] + red[64 + t]) + red[128 + t]) + red[192 + t];
}

// ------------------------------------------------------------------------------------------------------------------------------
// dh = dy W1' on a 64 (pixel) x 64 (channel) tile, K = cout in stages of 32; then, in the accumulators: the ReLU6 mask, and the
// tile's contribution to g_bd and to the nine taps of g_wd. grid (c tiles, pixel tiles); zpart [pixel tile][10][c] (9 taps, then g_bd).
__global__ __launch_bounds__(256) void hg_dz_kernel(const float* __restrict__ dy, const half_t* __restrict__ w1, const half_t* __restrict__ x,
                                                    const unsigned char* __restrict__ mask, HgShape s, const float* __restrict__ maxpart,
                                                    float* __restrict__ zpart) {
    __shared__ __attribute__((aligned(16))) half_t As[64 * HG_LD];
    __shared__ __attribute__((aligned(16))) half_t Bs[64 * HG_LD];
    __shared__ float red[4 * 10 * 64];
    float scale, unscale;
    hg_scale(maxpart, red, scale, unscale);
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wr = wv >> 1, wc = wv & 1, r = lane & 31, hh = lane >> 5;
    const int c0 = blockIdx.x * 64, p0 = blockIdx.y * 64;
    const int ak = t & 31, aq = t >> 5;          // A staging: output ak of the stage, pixels aq * 8 .. + 7
    const int bc = t & 63, bq = t >> 6;          // B staging: channel bc, outputs bq * 8 .. + 7 of the stage
    size_t rowoff[8];
    {
        const int pb = p0 + aq * 8;
        int img = pb / s.hw, pix = pb - img * s.hw;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            rowoff[i] = (size_t)img * (size_t)s.dy_img_stride + (size_t)pix * s.cout;
            if (++pix == s.hw) { pix = 0; ++img; }
        }
    }
    const bool c_ok = c0 + bc < s.c;
    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int ok = 0; ok < s.cout; ok += 32) {
        float av[8];
        half8 bv;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int p = p0 + aq * 8 + i, o = ok + ak;
            av[i] = (p < s.P && o < s.cout) ? dy[rowoff[i] + o] : 0.f;
            const int ob = ok + bq * 8 + i;
            bv[i] = (ob < s.cout && c_ok) ? w1[(size_t)ob * s.c + c0 + bc] : (half_t)0.f;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) As[(aq * 8 + i) * HG_LD + ak] = (half_t)(av[i] * scale);
        *reinterpret_cast<half8*>(&Bs[bc * HG_LD + bq * 8]) = bv;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const half8 a = *reinterpret_cast<const half8*>(&As[(wr * 32 + r) * HG_LD + kk * 16 + 8 * hh]);
            const half8 b = *reinterpret_cast<const half8*>(&Bs[(wc * 32 + r) * HG_LD + kk * 16 + 8 * hh]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
        }
    }
    // the lane holds 16 pixels of ONE channel: rows (reg & 3) + 8 (reg >> 2) + 4 hh of the wave's 32 x 32 tile
    const int col = c0 + wc * 32 + r;
    float sum[10];
#pragma unroll
    for (int q = 0; q < 10; ++q) sum[q] = 0.f;
    if (col < s.c) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int p = p0 + wr * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
            if (p >= s.P) continue;
            if (!mask[(size_t)p * s.c + col]) continue;
            const float dz = acc[i] * unscale;
            const int img = p / s.hw, pix = p - img * s.hw, y = pix / s.w, xx = pix - y * s.w;
            sum[9] += dz;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int yy = y + ky - 1, xc = xx + kx - 1;
                    if (yy < 0 || yy >= s.h || xc < 0 || xc >= s.w) continue;
                    sum[ky * 3 + kx] = fmaf(dz, (float)x[((size_t)(img * s.h + yy) * s.w + xc) * s.c + col], sum[ky * 3 + kx]);
                }
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 10; ++q) red[((wr * 2 + hh) * 10 + q) * 64 + wc * 32 + r] = sum[q];
    __syncthreads();
    for (int idx = t; idx < 640; idx += 256) {
        const int q = idx >> 6, cl = idx & 63;
        if (c0 + cl < s.c)
            zpart[((size_t)blockIdx.y * 10 + q) * s.c + c0 + cl] =
                ((red[(0 * 10 + q) * 64 + cl] + red[(1 * 10 + q) * 64 + cl]) + red[(2 * 10 + q) * 64 + cl]) + red[(3 * 10 + q) * 64 + cl];
    }
}

// out[i] = part[0][i] + part[1][i] + ... in slot order; slots lie `stride` floats apart
__global__ __launch_bounds__(256) void hg_reduce_kernel(const float* __restrict__ part, int slots, size_t stride, size_t count, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    float v = 0.f;
    for (int sl = 0; sl < slots; ++sl) v += part[(size_t)sl * stride + i];
    out[i] = v;
}

int hg_split(int P, int c, int cout) {
    const long tiles = (long)dn_cdiv(c, 64) * dn_cdiv(cout, 64);
    long sp = 1024 / tiles;
    sp = sp < 1 ? 1 : (sp > HG_MAX_SPLIT ? HG_MAX_SPLIT : sp);
    const long by_p = dn_cdiv(P, 128);
    return (int)(sp > by_p ? by_p : sp);
}

struct HgWorkspace {
    float* maxpart; half_t* hbuf; unsigned char* mask; float* w1part; float* b1part; float* zpart;
    size_t bytes;
};

HgWorkspace hg_workspace(void* base, int P, int c, int cout, bool dw) {
    HgWorkspace k;
    char* p = reinterpret_cast<char*>(base);
    size_t off = 0;
    auto take = [&](size_t b) { char* q = p + off; off += a256(b); return q; };
    const int sp = hg_split(P, c, cout);
    k.maxpart = reinterpret_cast<float*>(take(HG_MAXBLK * 4));
    k.hbuf = reinterpret_cast<half_t*>(take(dw ? (size_t)P * c * 2 : 0));
    k.mask = reinterpret_cast<unsigned char*>(take(dw ? (size_t)P * c : 0));
    k.w1part = reinterpret_cast<float*>(take(sp > 1 ? (size_t)sp * cout * c * 4 : 0));
    k.b1part = reinterpret_cast<float*>(take(sp > 1 ? (size_t)sp * cout * 4 : 0));
    k.zpart = reinterpret_cast<float*>(take(dw ? (size_t)dn_cdiv(P, 64) * 10 * c * 4 : 0));
    k.bytes = off;
    return k;
}

bool hg_sizes_ok(int n, int h, int w, int c, int cout) {
    return n > 0 && h > 0 && w > 0 && c > 0 && cout > 0 && (long)n * h * w <= (1l << 24) && h <= 4096 && w <= 4096 && c <= 65536;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) size_t dn_lite_head_backward_workspace_bytes(int n, int h, int w, int c, int cout, int depthwise) {
    if (!hg_sizes_ok(n, h, w, c, cout) || cout > 6 * DN_MAX_CLASSES) return 0;
    return hg_workspace(nullptr, n * h * w, c, cout, depthwise != 0).bytes;
}

extern "C" __attribute__((visibility("default"))) int dn_lite_head_backward(const void* x, const void* wd, const float* bd, const void* w1, const float* dy,
                                                                           int64_t dy_img_stride, int n, int h, int w, int c, int cout, float* g_wd,
                                                                           float* g_bd, float* g_w1, float* g_b1, void* workspace, size_t workspace_bytes,
                                                                           void* stream) {
    DN_REQUIRE(hg_sizes_ok(n, h, w, c, cout), "dn_lite_head_backward: bad sizes n=%d h=%d w=%d c=%d cout=%d", n, h, w, c, cout);
    DN_REQUIRE(x && w1 && dy && g_w1 && g_b1 && workspace, "dn_lite_head_backward: null argument");
    const bool dw = wd != nullptr;
    DN_REQUIRE(!dw || (bd && g_wd && g_bd), "dn_lite_head_backward: a depthwise stage needs bd, g_wd and g_bd");
    DN_REQUIRE(dy_img_stride >= (int64_t)h * w * cout, "dn_lite_head_backward: dy_img_stride %lld is smaller than the level's %lld columns",
               (long long)dy_img_stride, (long long)h * w * cout);
    if (c % 8 != 0 || cout > 6 * DN_MAX_CLASSES) {
        dn_set_error("dn_lite_head_backward: c=%d must be a multiple of 8 and cout=%d at most %d", c, cout, 6 * DN_MAX_CLASSES);
        return DN_E_UNSUPPORTED;
    }
    DN_REQUIRE(((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(wd) | reinterpret_cast<size_t>(w1) | reinterpret_cast<size_t>(workspace)) & 15) == 0 &&
                   ((reinterpret_cast<size_t>(dy) | reinterpret_cast<size_t>(bd) | reinterpret_cast<size_t>(g_wd) | reinterpret_cast<size_t>(g_bd) |
                     reinterpret_cast<size_t>(g_w1) | reinterpret_cast<size_t>(g_b1)) & 3) == 0,
               "dn_lite_head_backward: x, wd, w1 and the workspace must be 16-byte aligned, the fp32 arrays 4-byte aligned");
    const int P = n * h * w;
    const HgWorkspace k = hg_workspace(workspace, P, c, cout, dw);
    if (workspace_bytes < k.bytes) {
        dn_set_error("dn_lite_head_backward: workspace of %zu B, %zu B needed", workspace_bytes, k.bytes);
        return DN_E_WORKSPACE;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const HgShape sh{n, h, w, c, cout, h * w, P, (long)dy_img_stride};
    hipLaunchKernelGGL(hg_max_kernel, dim3(HG_MAXBLK), dim3(256), 0, s, dy, sh, k.maxpart);
    const half_t* hsrc = reinterpret_cast<const half_t*>(x);      // no depthwise stage: h = x
    if (dw) {
        hipLaunchKernelGGL(hg_prep_kernel, dim3(dn_cdiv((long)P * (c / 8), 256)), dim3(256), 0, s, reinterpret_cast<const half_t*>(x),
                           reinterpret_cast<const half_t*>(wd), bd, sh, k.hbuf, k.mask);
        hsrc = k.hbuf;
    }
    const int sp = hg_split(P, c, cout);
    const int chunk = dn_cdiv(dn_cdiv(P, sp), 32) * 32;
    hipLaunchKernelGGL(hg_w1_kernel, dim3(dn_cdiv(c, 64), dn_cdiv(cout, 64), sp), dim3(256), 0, s, dy, hsrc, sh, k.maxpart, chunk,
                       sp > 1 ? k.w1part : g_w1, sp > 1 ? k.b1part : g_b1);
    if (sp > 1) {
        hipLaunchKernelGGL(hg_reduce_kernel, dim3(dn_cdiv((long)cout * c, 256)), dim3(256), 0, s, k.w1part, sp, (size_t)cout * c, (size_t)cout * c, g_w1);
        hipLaunchKernelGGL(hg_reduce_kernel, dim3(dn_cdiv(cout, 256)), dim3(256), 0, s, k.b1part, sp, (size_t)cout, (size_t)cout, g_b1);
    }
    if (dw) {
        const int pt = dn_cdiv(P, 64);
        hipLaunchKernelGGL(hg_dz_kernel, dim3(dn_cdiv(c, 64), pt), dim3(256), 0, s, dy, reinterpret_cast<const half_t*>(w1),
                           reinterpret_cast<const half_t*>(x), k.mask, sh, k.maxpart, k.zpart);
        hipLaunchKernelGGL(hg_reduce_kernel, dim3(dn_cdiv((long)9 * c, 256)), dim3(256), 0, s, k.zpart, pt, (size_t)10 * c, (size_t)9 * c, g_wd);
        hipLaunchKernelGGL(hg_reduce_kernel, dim3(dn_cdiv(c, 256)), dim3(256), 0, s, k.zpart + (size_t)9 * c, pt, (size_t)10 * c, (size_t)c, g_bd);
    }
    DN_HIP_CHECK(hipGetLastError());
    dn_note_kernel("hg_w1_kernel");
    return DN_OK;
}
