// Fused expand + depthwise 3x3 stride 1 + project (+ residual) for the multi-chunk blocks of the 20 x 20 maps (80 -> 200 -> 80, 80 -> 184 -> 80 of
// MobileNetV3): the tiled body of expdw.hip with its phases walked ONCE per 5 x 10 tile over the whole expanded width instead of once per 64-channel
// chunk. A flag of the TILED choice (expdw_choose, choice.h: `whole`, DN_EXPDW_WHOLE); same reference ops (mobilenetv3.py:72-95, BN folded).
//
// Why: 64 images x 8 tiles are 512 workgroups = one residency round at two per CU, so the launch lasts one workgroup's life, and that life was the
// chunk loop: per 64 channels a weights-to-LDS + expand phase, a depthwise phase and a zero-fill + project phase, each behind a barrier that exposes
// a latency nothing covers (14 - 16 barriers for 200 / 184 channels, a whole pass for the 8-channel tail of 200). Here:
//   1. the input region (7 x 12 pixels x 80 channels + the bias column), ALL depthwise weights / biases and the project bias go to LDS; one barrier;
//   2. expand: wave w owns channel tile w of the ceil(cexp / 32) <= 7 tiles (its A fragments are requested once, at the top, and land under the
//      staging) and runs the three 32-row tiles back to back on three accumulators: 18 matrix steps, one wait for the results, then the
//      activations. E[96][cexp] holds every expanded channel, rows WITHOUT padding where cexp / 8 is odd (200, 184): the depthwise reads below are
//      then linear in the thread index. The residual pixels of the wave's output unit leave X for registers; one barrier;
//   3. depthwise: a thread owns (channel group of 8, output column, rows 0 - 2 [waves 0 - 3] or 3 - 4 [waves 4 - 7]): nine weight pieces and the
//      bias once, 15 E reads for three outputs or 12 for two (each E value feeds up to three outputs), the taps of every output still in (ky, kx)
//      order; the result goes to D[64][cexp16 + 8] laid over the dead X region; one barrier;
//   4. project over all expanded channels in ascending 16-deep steps on the six (row tile, channel tile) units; + b3 and the residual in fp32, one
//      rounding, the tile through LDS (over the dead E) and out as row-contiguous 16-byte pieces; one barrier.
// Same operands, same K steps in the same order, same rounding points and the same tap order as expdw_kernel's chunk loop (the all-zero K steps
// behind a short last chunk are dropped: they add +0 to an accumulator that started at +0): outputs are bit-identical (tests/test_gpu_expdw_whole.py).
#include <algorithm>
#include <type_traits>

#include "choice.h"

namespace {

constexpr int WH_NT = EXPDW_NT;                         // 8 waves; two workgroups per CU
constexpr int WH_CIN = EXPDW_WHOLE_CIN, WH_XW = WH_CIN + 8, WH_KSF = WH_CIN / 16;
constexpr int WH_OH = EXPDW_WHOLE_OH, WH_OW = EXPDW_WHOLE_OW, WH_IH = WH_OH + 2, WH_IW = WH_OW + 2, WH_NPIX = WH_IH * WH_IW;
constexpr int WH_ROWS = expdw_region_rows(3, 1, WH_OH, WH_OW), WH_RT = WH_ROWS / 32;
constexpr int WH_DROWS = EXPDW_WHOLE_DROWS, WH_PRT = WH_DROWS / 32;
constexpr int WH_NKS = EXPDW_WHOLE_CEXP_MAX / 16;       // most 16-deep K steps of the projection
static_assert(WH_CIN % 16 == 0 && WH_RT == 3 && WH_PRT == 2 && WH_ROWS == EXPDW_WHOLE_ROWS, "expdw_whole_lds (choice.h) sizes the LDS of this geometry");
static_assert((EXPDW_WHOLE_CEXP_MAX + 31) / 32 <= WH_NT / 64, "one channel tile of the expand per wave");
static_assert(WH_OH == 5 && WH_NT == 512, "the depthwise phase splits a column into rows 0 - 2 and 3 - 4, 256 threads each");

template <typename V, int N>
__device__ __forceinline__ void wh_act(V& v, int act) {     // (expdw.hip act_n: one uniform switch per N values)
    if (act == DN_ACT_RELU) {
#pragma unroll
        for (int e = 0; e < N; ++e) v[e] = dn_relu(v[e]);
    } else if (act == DN_ACT_RELU6) {
#pragma unroll
        for (int e = 0; e < N; ++e) v[e] = dn_relu6(v[e]);
    } else if (act == DN_ACT_HSWISH) {
#pragma unroll
        for (int e = 0; e < N; ++e) v[e] = v[e] * dn_relu6(v[e] + 3.f) * (1.f / 6.f);
    }
}

// CEXP: the expanded width as a compile-time constant for the two widths of the zoo (every LDS offset of the depthwise phase becomes an immediate, the
// K loop of the projection has no tests: 1 034 -> 810 / 840 vector instructions per wave), 0 = the launch's (any width the form can run)
template <int CEXP>
__global__ __launch_bounds__(WH_NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void expdw_whole_kernel(ExpDwArgs a, int tiles_x) {
    extern __shared__ __attribute__((aligned(16))) half_t lds[];
    const int cexp = CEXP ? CEXP : a.cexp, ng = cexp >> 3;
    const int DW = ((cexp + 15) & ~15) + 8;                 // halfs per D row: an odd number of 16-byte pieces (conflict-free B-fragment reads)
    const int EWS = expdw_whole_erow(cexp);                 // halfs per E row: cexp for the blocks of the zoo (200, 184: 25 and 23 pieces)
    half_t* Xs = lds;                                       // [ROWS][XW] + 8 zero halfs; dead behind the expand:
    half_t* Ds = lds;                                       // [DROWS][DW] depthwise output, the projection's B rows
    half_t* Es = lds + expdw_whole_front_halfs(cexp);       // [ROWS][EWS]; dead behind the depthwise: Os, the finished tile [OH * OW][cout]
    half_t* Wd = Es + WH_ROWS * EWS;                        // [9][cexp]
    float* Bd = reinterpret_cast<float*>(Wd + 9 * cexp);    // [cexp]
    float* B3s = Bd + cexp;                                 // [256]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    int n, tx;
    if (a.xq > 0) {                                         // XCD grouping (common.h): blockIdx.x % 8 = the group of a.xq images
        n = (blockIdx.x & 7) * a.xq + blockIdx.z;
        tx = blockIdx.x >> 3;
    } else {
        n = blockIdx.z;
        tx = blockIdx.x;
    }
    if (n >= a.n) return;
    const int ty = blockIdx.y;
    const int oy0 = ty * WH_OH, ox0 = tx * WH_OW;
    const int iy0 = oy0 - 1, ix0 = ox0 - 1;

    // ---- the wave's A fragments of the expand: channel tile ct, all K steps; the last step carries the bias pair at column cin (expdw.hip)
    const int CT = (cexp + 31) >> 5, rstep = (WH_NT / 64) / CT;         // waves ct, ct + CT, ... share a channel tile and split the row tiles
    const int ct = wave % CT, rt0 = wave / CT;
    const bool xunit = rt0 < rstep;
    half8 wf[WH_KSF], wlast;
    {
        const int ch = min(ct * 32 + r, cexp - 1);
        const half_t* wrow = a.w1 + (size_t)ch * WH_CIN;
#pragma unroll
        for (int ks = 0; ks < WH_KSF; ++ks) wf[ks] = *reinterpret_cast<const half8*>(wrow + ks * 16 + hh * 8);
        const float b = a.b1[ch];
        const half_t hi = (half_t)b;
        const half_t lo = (half_t)(b - (float)hi);
        const half8 bw = {hi, lo, 0, 0, 0, 0, 0, 0};
        const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
        wlast = hh ? zero8 : bw;
    }

    // ---- 1. input region, depthwise weights / biases, project bias -> LDS
    {
        // the 84 pixels of the region in 16-byte pieces, two per thread; the rows behind them (the padding of the third 32-row tile) and the 8 halfs behind the
        // last row are zeros
        constexpr int XC8 = WH_XW / 8, C8 = WH_CIN / 8, NCHK = WH_NPIX * XC8, NU = (NCHK + WH_NT - 1) / WH_NT, NZP = (WH_ROWS - WH_NPIX) * XC8 + 1;
        static_assert(NZP <= WH_NT, "one zero piece per thread");
        const half_t* xin = a.x + (size_t)n * a.H * a.W * WH_CIN;
        uint4 v[NU];
        int dst[NU];
        bool ok[NU], one[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int idx = tid + WH_NT * u;
            const int pix = idx / XC8, q = idx - pix * XC8;
            const int py = pix / WH_IW, px = pix - py * WH_IW;
            const int gy = iy0 + py, gx = ix0 + px;
            const bool inside = idx < NCHK && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
            dst[u] = idx < NCHK ? pix * WH_XW + q * 8 : -1;
            ok[u] = inside && q < C8;
            one[u] = inside && q == C8;
            v[u] = *reinterpret_cast<const uint4*>(xin + (ok[u] ? ((size_t)gy * a.W + gx) * WH_CIN + q * 8 : (size_t)0));
        }
        const int wtap = tid / ng, wc8 = tid - wtap * ng;                   // 9 * ng <= NT pieces of the depthwise weights (expdw_whole_supported)
        const uint4 wdreg = *reinterpret_cast<const uint4*>(a.wd + (size_t)min(wtap, 8) * cexp + wc8 * 8);
        const float bdreg = a.bd[min(tid, cexp - 1)];
        const float b3reg = a.b3[min(tid & 255, a.cout - 1)];
        if (tid < NZP) *reinterpret_cast<uint4*>(&Xs[WH_NPIX * WH_XW + tid * 8]) = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int u = 0; u < NU; ++u)
            if (dst[u] >= 0) *reinterpret_cast<uint4*>(&Xs[dst[u]]) = ok[u] ? v[u] : make_uint4(one[u] ? 0x3c003c00u : 0u, 0, 0, 0);
        if (wtap < 9) *reinterpret_cast<uint4*>(&Wd[wtap * cexp + wc8 * 8]) = wdreg;
        if (tid < cexp) Bd[tid] = bdreg;
        if (tid < 256) B3s[tid] = tid < a.cout ? b3reg : 0.f;
    }
    __syncthreads();

    // ---- 2. expand: E[pixel][channel] = act1(X . W1 + b1) rounded to fp16; a pixel outside the image expands to act1(0) = 0
    const int pct = (a.cout + 31) >> 5;
    const int prt = wave % WH_PRT, pc = wave / WH_PRT;      // project unit of the wave: (32-pixel row tile, 32-channel tile)
    const bool punit = pc < pct;
    const int opix = prt * 32 + r;
    const int poy = opix / WH_OW, pox = opix - poy * WH_OW;
    half4 res[4];
    {
        floatx16 acc[WH_RT];
#pragma unroll
        for (int i = 0; i < WH_RT; ++i) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
            const int rt = rt0 + i * rstep;
            if (xunit && rt < WH_RT) {
                const half_t* xrow = &Xs[(rt * 32 + r) * WH_XW + hh * 8];
#pragma unroll
                for (int ks = 0; ks < WH_KSF; ++ks)
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[ks], *reinterpret_cast<const half8*>(xrow + ks * 16), acc[i], 0, 0, 0);
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wlast, *reinterpret_cast<const half8*>(xrow + WH_KSF * 16), acc[i], 0, 0, 0);
            }
        }
        asm volatile("s_nop 7\n\ts_nop 3" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]));      /* matrix result -> activation switch: every branch path gets its wait states (expdw.hip) */
#pragma unroll
        for (int i = 0; i < WH_RT; ++i) {
            const int rt = rt0 + i * rstep;
            if (xunit && rt < WH_RT) {
                wh_act<floatx16, 16>(acc[i], a.act1);
                half_t* erow = &Es[(rt * 32 + r) * EWS + ct * 32 + 4 * hh];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (ct * 32 + 8 * g < cexp) {           // (a group beyond cexp would land in the next row)
                        half4 hv;
#pragma unroll
                        for (int e = 0; e < 4; ++e) hv[e] = (half_t)acc[i][4 * g + e];
                        *reinterpret_cast<half4*>(erow + 8 * g) = hv;
                    }
                }
            }
        }
        // the residual pixels of this wave's output unit leave X now: D is laid over the region
        if (a.has_res && punit) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = pc * 32 + 8 * g + 4 * hh;
                res[g] = *reinterpret_cast<const half4*>(&Xs[((min(poy, WH_OH - 1) + 1) * WH_IW + pox + 1) * WH_XW + min(c, a.cout - 4)]);
            }
        }
    }
    __syncthreads();

    // ---- 3. depthwise: item = (channel group cg, output column ox), consecutive threads on consecutive groups, then columns; waves 0 - 3 rows 0 - 2, waves
    //         4 - 7 rows 3 - 4 (a uniform split: one half of the waves does not carry a third output that does not exist)
    auto depthwise = [&](auto nout_c, int oyb) {
        constexpr int NOUT = decltype(nout_c)::value;
        for (int item = tid & 255; item < WH_OW * ng; item += 256) {
            const int ox = item / ng, cg = item - ox * ng;
            uint4 wv[9];
#pragma unroll
            for (int tp = 0; tp < 9; ++tp) wv[tp] = *reinterpret_cast<const uint4*>(&Wd[tp * cexp + cg * 8]);
            float acc[NOUT][8];
            {
                const float4 b0 = *reinterpret_cast<const float4*>(&Bd[cg * 8]), b1 = *reinterpret_cast<const float4*>(&Bd[cg * 8 + 4]);
#pragma unroll
                for (int o = 0; o < NOUT; ++o) {
                    acc[o][0] = b0.x; acc[o][1] = b0.y; acc[o][2] = b0.z; acc[o][3] = b0.w; acc[o][4] = b1.x; acc[o][5] = b1.y; acc[o][6] = b1.z; acc[o][7] = b1.w;
                }
            }
            // input row oyb + j feeds output o = j - ky through tap row ky: every output still sees its taps in (ky, kx) order
            const half_t* ebase = Es + (oyb * WH_IW + ox) * EWS + cg * 8;
#pragma unroll
            for (int j = 0; j < NOUT + 2; ++j) {
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const uint4 ev = *reinterpret_cast<const uint4*>(ebase + (j * WH_IW + kx) * EWS);
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky) {
                        const int o = j - ky;
                        if (o >= 0 && o < NOUT) fma_mix_h8(acc[o], ev, wv[ky * 3 + kx]);
                    }
                }
            }
#pragma unroll
            for (int o = 0; o < NOUT; ++o) {
                wh_act<float[8], 8>(acc[o], a.act2);
                half8 hv;
#pragma unroll
                for (int e = 0; e < 8; ++e) hv[e] = (half_t)acc[o][e];
                *reinterpret_cast<half8*>(&Ds[((oyb + o) * WH_OW + ox) * DW + cg * 8]) = hv;
            }
        }
    };
    if (wave < 4) depthwise(std::integral_constant<int, 3>(), 0);
    else depthwise(std::integral_constant<int, 2>(), 3);
    // the projection's A fragments: requested here, they land while the slower waves finish the depthwise
    const int nks = (cexp + 15) >> 4;
    half8 w3f[WH_NKS];
    if (punit) {
        const int co = min(pc * 32 + r, a.cout - 1);
#pragma unroll
        for (int ks = 0; ks < WH_NKS; ++ks)
            if (ks < nks) w3f[ks] = *reinterpret_cast<const half8*>(a.w3 + (size_t)co * cexp + min(ks * 16 + hh * 8, cexp - 8));
    }
    __syncthreads();

    // ---- 4. project: one accumulator per unit over all expanded channels in ascending 16-deep steps; the tile leaves through LDS
    half_t* Os = Es;
    if (punit) {
        floatx16 pacc;
#pragma unroll
        for (int e = 0; e < 16; ++e) pacc[e] = 0.f;
        const bool cok = pc * 32 + r < a.cout;
        const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
        const half_t* drow = &Ds[opix * DW + hh * 8];
#pragma unroll
        for (int ks = 0; ks < WH_NKS; ++ks) {
            if (ks < nks) {
                const bool kok = ks * 16 + hh * 8 < cexp;   // (the columns of D behind cexp are never written)
                const half8 w = (cok && kok) ? w3f[ks] : zero8;
                const half8 d = *reinterpret_cast<const half8*>(drow + ks * 16);
                pacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(w, kok ? d : zero8, pacc, 0, 0, 0);
            }
        }
        asm volatile("s_nop 7\n\ts_nop 3" : "+v"(pacc));
        if (opix < WH_OH * WH_OW) {
            half_t* orow = Os + opix * a.cout;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = pc * 32 + 8 * g + 4 * hh;
                if (c < a.cout) {           // cout % 8 == 0: the 4-channel group is entirely in range
                    const float4 b = *reinterpret_cast<const float4*>(&B3s[c]);
                    float v[4] = {pacc[4 * g + 0] + b.x, pacc[4 * g + 1] + b.y, pacc[4 * g + 2] + b.z, pacc[4 * g + 3] + b.w};
                    if (a.has_res) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] += (float)res[g][e];
                    }
                    half4 hv;
#pragma unroll
                    for (int e = 0; e < 4; ++e) hv[e] = (half_t)v[e];
                    *reinterpret_cast<half4*>(orow + c) = hv;
                }
            }
        }
    }
    __syncthreads();
    const int oc8 = a.cout >> 3;
    for (int i = tid; i < WH_OH * WH_OW * oc8; i += WH_NT) {
        const int px = (int)fd_div((unsigned)i, a.fd_oc8), c8 = i - px * oc8;
        const int py = px / WH_OW, pxx = px - py * WH_OW;
        const int y = oy0 + py, x = ox0 + pxx;
        if (y < a.Ho && x < a.Wo)
            *reinterpret_cast<uint4*>(a.out + (((size_t)n * a.Ho + y) * a.Wo + x) * a.cout + c8 * 8) = *reinterpret_cast<const uint4*>(Os + px * a.cout + c8 * 8);
    }
}

}  // namespace

// `a` with the launcher-owned fields filled (launch_expdw); lds = expdw_choose's lds_w
int launch_expdw_whole(const ExpDwArgs& a, size_t lds, hipStream_t s) {
    const int tiles_x = dn_cdiv(a.Wo, WH_OW), tiles_y = dn_cdiv(a.Ho, WH_OH);
    const dim3 grid(a.xq > 0 ? 8 * tiles_x : tiles_x, tiles_y, a.xq > 0 ? a.xq : a.n);
    auto launch = [&](auto kernel) -> int {
        DN_HIP_CHECK(dn_allow_big_lds(reinterpret_cast<const void*>(kernel)));
        hipLaunchKernelGGL(kernel, grid, dim3(WH_NT), lds, s, a, tiles_x);
        return DN_OK;
    };
    if (a.cexp == 200) return launch(expdw_whole_kernel<200>);
    if (a.cexp == 184) return launch(expdw_whole_kernel<184>);
    return launch(expdw_whole_kernel<0>);
}
