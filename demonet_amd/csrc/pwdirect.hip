// Pointwise (1x1) convolution for short reductions (cin <= 256), register-direct: no LDS, no barriers.
//
// reference ops replaced: the expand / project ConvBNActivation 1x1 convs of InvertedResidual (mobilenetv3.py:72-95, BN folded),
//   the 1x1 convs of _extra_block (ssd_mobilenetv3.py:39-54) and of the V2 ExtraBlocks (backbone.py:100-111) -- the same layers
//   pointwise.hip's tiled kernel serves; this file is only a different schedule for them.
//
// Why: on these layers the tiled kernel is not bound by HBM or by the matrix cores but by VALU issue (tools/valu.sh: ~400 vector
// instructions per wave for 1024 outputs -- staging addresses, guards, the LDS round trips of operands and of the output tile, a
// bias add and an activation select per element; a wave64 VALU instruction holds its SIMD for 4 cycles). Here a wave owns 32
// pixels x (32 * TC) channels and
//   * both MFMA operands go from global memory / L2 straight into registers in fragment order (lane (r, hh) of
//     v_mfma_f32_32x32x16_f16 needs 16 contiguous bytes of row r: one global_load_dwordx4 with an immediate offset per K step,
//     every load of the wave requested before the first use -- ONE exposed memory round trip);
//   * the bias rides in the reduction: two extra K columns hold (1, 1) on the pixel side and (hi, lo) = the fp32 bias split into
//     two fp16 values on the weight side (|b - hi - lo| <= 2^-22 |b|), so the accumulator starts life as conv + bias;
//   * the activation is ONE uniform switch per 16-value accumulator, not a select per element;
//   * v_permlane32_swap turns the accumulator layout (4 channels per lane and register group) into 8-channel runs: the tile leaves as
//     two 16-byte stores per lane, each instruction writing 32 contiguous bytes per pixel, without an LDS transpose.
// The residual (fp16, NHWC) is requested up front in the accumulator layout and added in fp32 before the single rounding
// (mobilenetv3.py:97-99 computes act(conv + bias) + x).
#include <algorithm>

#include "common.h"
#include "choice.h"

__device__ const uint4 g_pwdw_zero16 = {0u, 0u, 0u, 0u};      // what a tap outside the image reads

namespace {

typedef unsigned uint2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void act16(floatx16& v, int act) {
    // `v` comes straight from a matrix instruction and the first thing that happens to it is a scalar branch on `act`: hipcc's hazard recognizer gives the
    // straight path its 12 wait states but undercounts some of the branch paths (5 - 7: tools/mfma_hazard_scan.py --all). Twelve explicit wait states in
    // front of the switch cover every path (the matrix instruction runs under them; other waves issue meanwhile).
    asm volatile("s_nop 7\n\ts_nop 3" : "+v"(v));       // (tied to the accumulator: otherwise hipcc schedules it in front of the last matrix instruction)
    if (act == DN_ACT_RELU) {
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = dn_relu(v[e]);
    } else if (act == DN_ACT_RELU6) {
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = dn_relu6(v[e]);
    } else if (act == DN_ACT_HSWISH) {
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = v[e] * dn_relu6(v[e] + 3.f) * (1.f / 6.f);
    }
}

// KSF: full 16-deep K steps (cin >> 4, exact: no guards in the load / MFMA sequences); TC: 32-channel tiles per wave.
// Workgroup = 4 waves = (4 >> wc_log) row tiles of 32 pixels x (1 << wc_log) channel blocks of 32 * TC channels.
template <int KSF, int TC>
__global__ __launch_bounds__(256) void pw_direct_kernel(PwArgs a, int tiles, int wc_log) {
    constexpr int KSM = KSF > 0 ? KSF : 1;
    const int lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wc = wave & ((1 << wc_log) - 1), wp = wave >> wc_log;
    const int BP = 32 * (4 >> wc_log), BC = (32 * TC) << wc_log;
    const int K = a.cin, NC = a.cout;
    // row tile / channel block of this workgroup; XCD grouping as in pointwise.hip (pw_tile_rows): the workgroups with equal
    // (flat index % 8) own the rows of one group of a.xq images
    int m0, mend, by;
    {
        const int flat = blockIdx.x;
        if (a.xq > 0) {
            const int g = flat & 7, w = flat >> 3;
            by = w / tiles;
            const int t = w - by * tiles;
            const int r0 = g * a.xq * a.hw;
            mend = min(a.m, r0 + a.xq * a.hw);
            m0 = r0 + t * BP;
        } else {
            by = flat / tiles;
            m0 = (flat - by * tiles) * BP;
            mend = a.m;
        }
    }
    const int mrow0 = m0 + wp * 32;
    const int n_base = by * BC + wc * 32 * TC;
    if (mrow0 >= mend || n_base >= NC) return;            // wave-uniform
    const int row = mrow0 + r;
    const int rowc = min(row, mend - 1);
    // KSF full 16-deep steps; then ONE last step: the K tail (cin % 16 == 8) and the bias columns

    // ---- every load of the wave, up front
    const half_t* xp = a.x + (size_t)rowc * K + hh * 8;
    const half_t* wpt[TC];
    int nrow[TC];
#pragma unroll
    for (int i = 0; i < TC; ++i) {
        nrow[i] = min(n_base + i * 32 + r, NC - 1);
        wpt[i] = a.w + (size_t)nrow[i] * K + hh * 8;
    }
    half8 xf[KSM], wf[TC][KSM];
#pragma unroll
    for (int ks = 0; ks < KSF; ++ks) {
        xf[ks] = *reinterpret_cast<const half8*>(xp + ks * 16);
#pragma unroll
        for (int i = 0; i < TC; ++i) wf[i][ks] = *reinterpret_cast<const half8*>(wpt[i] + ks * 16);
    }
    // squeeze-excitation scale of the wave's image (a 32-row tile never straddles two images here: hw % 32 == 0, pw_direct_supported),
    // requested with the operands: s[k] for this lane's columns of every step
    const bool has_se = a.se != nullptr;
    float4 sv[KSM][2], svl[2];
    const float* sp = has_se ? a.se + (size_t)(mrow0 / a.hw) * K + hh * 8 : nullptr;
    if (has_se) {
#pragma unroll
        for (int ks = 0; ks < KSF; ++ks) {
            sv[ks][0] = *reinterpret_cast<const float4*>(sp + ks * 16);
            sv[ks][1] = *reinterpret_cast<const float4*>(sp + ks * 16 + 4);
        }
    }
    // last step: this lane's columns kb .. kb+7; kb < K: data (address clamped, value selected below); kb == K: the bias columns
    const int kb = KSF * 16 + hh * 8;
    const int kcl = min(kb, K - 8) - hh * 8;
    half8 xl = *reinterpret_cast<const half8*>(xp + kcl);
    if (has_se) {
        svl[0] = *reinterpret_cast<const float4*>(sp + kcl);
        svl[1] = *reinterpret_cast<const float4*>(sp + kcl + 4);
    }
    half8 wl[TC];
    float bl[TC];
#pragma unroll
    for (int i = 0; i < TC; ++i) {
        wl[i] = *reinterpret_cast<const half8*>(wpt[i] + kcl);
        bl[i] = a.bias[nrow[i]];
    }
    uint2 rres[TC][4];
    const bool has_res = a.residual != nullptr;
    if (has_res) {
        const half_t* rp = a.residual + (size_t)rowc * NC;
#pragma unroll
        for (int i = 0; i < TC; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                rres[i][g] = *reinterpret_cast<const uint2*>(rp + min(n_base + i * 32 + 8 * g + 4 * hh, NC - 4));
    }
    if (has_se) {
        // (half)((float)x * s): the rounding of the tiled kernel's squeeze-excitation path (pointwise.hip load_into)
        auto scale8 = [](half8 v, const float4& s0, const float4& s1) {
            const float s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (half_t)((float)v[e] * s[e]);
            return v;
        };
#pragma unroll
        for (int ks = 0; ks < KSF; ++ks) xf[ks] = scale8(xf[ks], sv[ks][0], sv[ks][1]);
        xl = scale8(xl, svl[0], svl[1]);
    }
    {
        const bool data = kb < K, bcol = kb == K;
        const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
        const half8 ones = {(half_t)1.f, (half_t)1.f, 0, 0, 0, 0, 0, 0};
        xl = data ? xl : (bcol ? ones : zero8);
#pragma unroll
        for (int i = 0; i < TC; ++i) {
            const half_t hi = (half_t)bl[i];
            const half_t lo = (half_t)(bl[i] - (float)hi);
            const half8 bw = {hi, lo, 0, 0, 0, 0, 0, 0};
            wl[i] = data ? wl[i] : (bcol ? bw : zero8);
        }
    }

    // ---- the reduction
    floatx16 acc[TC];
#pragma unroll
    for (int i = 0; i < TC; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KSF; ++ks) {
#pragma unroll
        for (int i = 0; i < TC; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[i][ks], xf[ks], acc[i], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < TC; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[i], xl, acc[i], 0, 0, 0);

    // ---- epilogue: lane = pixel r; registers 4g .. 4g+3 of tile i = channels n_base + 32 i + 8g + 4hh .. +3
    half_t* orow = reinterpret_cast<half_t*>(a.out) + (size_t)row * NC + hh * 8;
#pragma unroll
    for (int i = 0; i < TC; ++i) {
        const int nt = n_base + i * 32;
        if (nt >= NC) break;                               // wave-uniform
        act16(acc[i], a.act);
        if (has_res) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const half4 rr = __builtin_bit_cast(half4, rres[i][g]);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][4 * g + e] += (float)rr[e];
            }
        }
        uint2v p[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            half4 hv;
#pragma unroll
            for (int e = 0; e < 4; ++e) hv[e] = (half_t)acc[i][4 * g + e];
            p[g] = __builtin_bit_cast(uint2v, hv);
        }
        // lanes r / r + 32 hold the two halves of every 8-channel group of pixel r: swap so that lane r ends up with channels
        // 0..15 and lane r + 32 with channels 16..31 of the tile (v_permlane32_swap: upper half of the first operand <-> lower half of the second)
        uint4 lo4, hi4;
        {
            // (round 3: groups (0, 1) and (2, 3) are paired, so that lane r ends up with channels 0..7 / 16..23 and lane r + 32 with 8..15 /
            // 24..31: each store instruction then writes 32 CONTIGUOUS bytes per pixel -- whole sectors -- instead of two 16-byte pieces
            // 32 bytes apart)
            const uint2v s0 = __builtin_amdgcn_permlane32_swap(p[0][0], p[1][0], false, false);
            const uint2v s1 = __builtin_amdgcn_permlane32_swap(p[0][1], p[1][1], false, false);
            const uint2v s2 = __builtin_amdgcn_permlane32_swap(p[2][0], p[3][0], false, false);
            const uint2v s3 = __builtin_amdgcn_permlane32_swap(p[2][1], p[3][1], false, false);
            lo4 = make_uint4(s0[0], s1[0], s0[1], s1[1]);
            hi4 = make_uint4(s2[0], s3[0], s2[1], s3[1]);
        }
        const int c0 = nt + hh * 8;
        if (row < mend) {
            if (c0 < NC) *reinterpret_cast<uint4*>(orow + nt) = lo4;
            if (c0 + 16 < NC) *reinterpret_cast<uint4*>(orow + nt + 16) = hi4;
        }
    }
}

// Streaming variant for the WIDE expansions (round 3): 112 -> 672 and 80 -> 480 on the 20 x 20 maps. pw_direct_kernel<7, 2> needs 186
// registers for "every operand of the wave up front" (2 waves per SIMD) and puts 8 800 waves through the chip in 4.3 rounds (24 us for a
// 40 MB layer). Here a wave keeps its 32 pixel rows (the B fragments) for a RUN of channel tiles and streams the weight tiles through two
// register sets: tile t + 1 is requested before the matrix instructions of tile t are issued, so after the first tile no round trip is
// exposed, and 800 pixel tiles x 3 channel runs = 2 400 waves fit the chip at once (~150 registers, 3 waves per SIMD). The four waves of a
// workgroup walk the same weight tiles at the same time (three of the four reads hit L1). Per-tile arithmetic, bias-in-the-reduction and
// the permlane epilogue are pw_direct_kernel's: the outputs are bit-identical to it. No squeeze-excitation scale, no residual (the
// expansions have neither).
// PX (round 4): 32-pixel tiles per wave. The four waves of a workgroup walk the same weight tiles, and every wave pulls them through the CU's
// L1 by itself: 13 M cache accesses (850 MB) for a 40 MB layer, and with the weight requests taken out the 112 -> 672 launch drops from 20.8 to
// 15.3 us (tools/time_pw.py on an ablated build) -- the L1's 64 B per clock, not L2 or HBM, is what the stream costs. With two pixel tiles per
// wave a weight fragment feeds two matrix instructions: half the L1 traffic per output.
template <int KSF, int PX>
__global__ __launch_bounds__(256) void pw_stream_kernel(PwArgs a, int tiles, int tiles_per_run) {
    constexpr int KSM = KSF > 0 ? KSF : 1;
    const int lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int K = a.cin, NC = a.cout;
    int m0, mend, by;
    {
        const int flat = blockIdx.x;
        if (a.xq > 0) {
            const int g = flat & 7, w = flat >> 3;
            by = w / tiles;
            const int t = w - by * tiles;
            const int r0 = g * a.xq * a.hw;
            mend = min(a.m, r0 + a.xq * a.hw);
            m0 = r0 + t * (128 * PX);
        } else {
            by = flat / tiles;
            m0 = (flat - by * tiles) * (128 * PX);
            mend = a.m;
        }
    }
    const int mrow0 = m0 + wave * (32 * PX);
    const int ctiles = (NC + 31) >> 5;
    const int ct0 = by * tiles_per_run, ct1 = min(ctiles, ct0 + tiles_per_run);
    if (mrow0 >= mend || ct0 >= ct1) return;               // wave-uniform
    const int kb = KSF * 16 + hh * 8;
    const int kcl = min(kb, K - 8) - hh * 8;
    const bool data = kb < K, bcol = kb == K;
    const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    half8 wf[2][KSM], wl[2];
    float bl[2];
    auto request = [&](const int ct, const int buf) {
        const int nrow = min(ct * 32 + r, NC - 1);
        const half_t* wp = a.w + (size_t)nrow * K + hh * 8;
#pragma unroll
        for (int ks = 0; ks < KSF; ++ks) wf[buf][ks] = *reinterpret_cast<const half8*>(wp + ks * 16);
        wl[buf] = *reinterpret_cast<const half8*>(wp + kcl);
        bl[buf] = a.bias[nrow];
    };
    half8 xf[PX][KSM], xl[PX];
    int row[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        row[j] = mrow0 + 32 * j + r;
        const half_t* xp = a.x + (size_t)min(row[j], mend - 1) * K + hh * 8;
#pragma unroll
        for (int ks = 0; ks < KSF; ++ks) xf[j][ks] = *reinterpret_cast<const half8*>(xp + ks * 16);
        xl[j] = *reinterpret_cast<const half8*>(xp + kcl);
    }
    request(ct0, 0);
    {
        const half8 ones = {(half_t)1.f, (half_t)1.f, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < PX; ++j) xl[j] = data ? xl[j] : (bcol ? ones : zero8);
    }
    auto tile = [&](const int ct, const int buf) {
        half8 wlast;
        {
            const half_t hi = (half_t)bl[buf];
            const half_t lo = (half_t)(bl[buf] - (float)hi);
            const half8 bw = {hi, lo, 0, 0, 0, 0, 0, 0};
            wlast = data ? wl[buf] : (bcol ? bw : zero8);
        }
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            floatx16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KSF; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[buf][ks], xf[j][ks], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wlast, xl[j], acc, 0, 0, 0);
            act16(acc, a.act);
            uint2v p[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                half4 hv;
#pragma unroll
                for (int e = 0; e < 4; ++e) hv[e] = (half_t)acc[4 * g + e];
                p[g] = __builtin_bit_cast(uint2v, hv);
            }
            const uint2v s0 = __builtin_amdgcn_permlane32_swap(p[0][0], p[1][0], false, false);
            const uint2v s1 = __builtin_amdgcn_permlane32_swap(p[0][1], p[1][1], false, false);
            const uint2v s2 = __builtin_amdgcn_permlane32_swap(p[2][0], p[3][0], false, false);
            const uint2v s3 = __builtin_amdgcn_permlane32_swap(p[2][1], p[3][1], false, false);
            const uint4 lo4 = make_uint4(s0[0], s1[0], s0[1], s1[1]), hi4 = make_uint4(s2[0], s3[0], s2[1], s3[1]);
            const int nt = ct * 32, c0 = nt + hh * 8;
            half_t* orow = reinterpret_cast<half_t*>(a.out) + (size_t)row[j] * NC + hh * 8;
            if (row[j] < mend) {
                if (c0 < NC) *reinterpret_cast<uint4*>(orow + nt) = lo4;
                if (c0 + 16 < NC) *reinterpret_cast<uint4*>(orow + nt + 16) = hi4;
            }
        }
    };
    // (the requests are UNCONDITIONAL, with a clamped tile index: behind a branch the compiler cannot count which loads are outstanding at
    // the join and waits for all of them -- vmcnt(0) before the first matrix instruction, i.e. no overlap at all; the price is one
    // redundant tile request at the end of a run)
    // (and pinned in front of the matrix instructions: left alone the scheduler sinks the next tile's loads below the current tile's MFMAs)
    for (int ct = ct0; ct < ct1; ct += 2) {
        request(min(ct + 1, ct1 - 1), 1);
        __builtin_amdgcn_sched_barrier(0);
        tile(ct, 0);
        if (ct + 1 < ct1) {
            request(min(ct + 2, ct1 - 1), 0);
            __builtin_amdgcn_sched_barrier(0);
            tile(ct + 1, 1);
        }
    }
}

template <int KSF, int PX>
int launch_stream_t(const PwArgs& a, int runs, int tiles_per_run, hipStream_t s) {
    const int tiles = a.xq > 0 ? dn_cdiv((long)a.xq * a.hw, 128 * PX) : dn_cdiv(a.m, 128 * PX);
    const dim3 grid((unsigned)(a.xq > 0 ? 8 * tiles : tiles) * runs);
    dn_note_kernel("pw_stream_kernel<%d,%d>", KSF, PX);
    hipLaunchKernelGGL((pw_stream_kernel<KSF, PX>), grid, dim3(256), 0, s, a, tiles, tiles_per_run);
    return DN_OK;
}

// Depthwise 3x3 (stride 1, pad 1) + the 1x1 projection behind it in ONE launch, register-direct: the first block of the MobileNets
// (mobilenetv3.py:61-99 with expanded == input channels: depthwise -> project (+ residual); mobilenetv2.py:57-84 with expand_ratio 1).
// Lane (r, hh) of the projection's B fragment holds 8 channels of ONE pixel -- exactly what a depthwise thread produces -- so the
// depthwise is computed straight into the fragment: nine 16-byte taps per lane and K step (neighbouring pixels, same channels; the
// wave covers 32 consecutive pixels of a row, the taps overlap in L1), bias first, taps in (ky, kx) order through v_fma_mix_f32,
// activation, ONE rounding to fp16 -- the arithmetic of dw_kernel, bit for bit -- and the value never exists in HBM: on the 160 x 160
// map that is 52 MB written and 52 MB read back per 64 images, and the residual (the block's input) is the centre tap's line.
// The projection (bias in the reduction, permlane epilogue) is pw_direct_kernel<KSF, 1>'s.
struct PwDwArgs {
    PwArgs pw;                       // x = the depthwise INPUT [n][h][w][cin]; cin == depthwise channels; residual: null or == x
    const half_t* wd; const float* bd;      // depthwise weights [9][cin] fp16, bias [cin] fp32
    int h, w, act_dw;
    float inv_hw;                    // 1 / (h w): image of a row by a corrected float quotient
    FastDiv fd_w;
};

template <int KSF>
__global__ __launch_bounds__(256) void pw_dw_direct_kernel(PwDwArgs q, int tiles) {
    const PwArgs& a = q.pw;
    const int lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int K = a.cin, NC = a.cout;
    int m0, mend;
    {
        const int flat = blockIdx.x;
        if (a.xq > 0) {
            const int g = flat & 7, t = flat >> 3;
            const int r0 = g * a.xq * a.hw;
            mend = min(a.m, r0 + a.xq * a.hw);
            m0 = r0 + t * 128;
        } else {
            m0 = flat * 128;
            mend = a.m;
        }
    }
    const int mrow0 = m0 + wave * 32;
    if (mrow0 >= mend) return;                             // wave-uniform
    const int row = mrow0 + r;
    const int rowc = min(row, mend - 1);
    // position of this lane's pixel inside its image: the wave's first row by a corrected float quotient (wave-uniform), then at most
    // one wrap for the lane (hw >= 32)
    int rem;
    {
        int q0 = (int)((float)mrow0 * q.inv_hw);
        int r0 = mrow0 - q0 * a.hw;
        while (r0 < 0) r0 += a.hw;                            // (the float quotient is off by at most a few units even for 2^31 rows)
        while (r0 >= a.hw) r0 -= a.hw;
        rem = r0 + (rowc - mrow0);
        if (rem >= a.hw) rem -= a.hw;
    }
    const int py = (int)fd_div((unsigned)rem, q.fd_w), px = rem - py * q.w;
    // the projection's operands that do not depend on the depthwise: requested first
    const int nrow = min(r, NC - 1);
    const half_t* wpt = a.w + (size_t)nrow * K + hh * 8;
    half8 wf[KSF];
#pragma unroll
    for (int ks = 0; ks < KSF; ++ks) wf[ks] = *reinterpret_cast<const half8*>(wpt + ks * 16);
    const int kb = KSF * 16 + hh * 8;                      // == K + 8 hh: hh = 0 carries the bias columns, hh = 1 zeros
    const float bl = a.bias[nrow];
    uint2 rres[4];
    const bool has_res = a.residual != nullptr;
    if (has_res) {
        const half_t* rp = a.residual + (size_t)rowc * NC;
#pragma unroll
        for (int g = 0; g < 4; ++g) rres[g] = *reinterpret_cast<const uint2*>(rp + min(8 * g + 4 * hh, NC - 4));
    }
    // ---- depthwise into the B fragments
    typedef const __attribute__((address_space(1))) half8* gp8;
    const gp8 zero = (gp8)(&g_pwdw_zero16);
    const half_t* xpix = a.x + (size_t)rowc * K + hh * 8;           // this lane's channels of its own pixel
    half8 xf[KSF];
#pragma unroll
    for (int ks = 0; ks < KSF; ++ks) {
        // The launch is bound by the vector-memory pipe (22 wave-wide loads per wave for two MFMAs), and the depthwise weights / bias are the
        // same for every pixel: both 8-channel halves of a tap come through the scalar cache (uniform address, constant address space) and
        // the lane picks its half with selects -- nine vector loads less per lane.
        typedef unsigned u4v __attribute__((ext_vector_type(4)));
        typedef float f4v __attribute__((ext_vector_type(4)));
        typedef const __attribute__((address_space(4))) u4v* cp4;
        typedef const __attribute__((address_space(4))) f4v* cpf4;
        half8 xin[9];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int iy = py + ky - 1, ix = px + kx - 1;
                const bool ok = iy >= 0 && iy < q.h && ix >= 0 && ix < q.w;
                xin[ky * 3 + kx] = *(ok ? (gp8)(xpix + ks * 16 + ((ky - 1) * q.w + (kx - 1)) * K) : zero);
            }
        float acc[8];
        {
            const cpf4 bp = (cpf4)(q.bd + ks * 16);
            const f4v c0 = bp[0], c1 = bp[1], c2 = bp[2], c3 = bp[3];
#pragma unroll
            for (int e = 0; e < 4; ++e) { acc[e] = hh ? c2[e] : c0[e]; acc[4 + e] = hh ? c3[e] : c1[e]; }
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            // this tap's weights: both halves sit in scalar registers, the lane's half is selected right before its use (nine selected
            // fragments held at once cost 32 registers and three waves of occupancy)
            const cp4 wp = (cp4)(q.wd + t * K + ks * 16);
            const u4v w0 = wp[0], w1 = wp[1];
            const uint4 wsel = make_uint4(hh ? w1[0] : w0[0], hh ? w1[1] : w0[1], hh ? w1[2] : w0[2], hh ? w1[3] : w0[3]);
            fma_mix_h8(acc, *reinterpret_cast<const uint4*>(&xin[t]), wsel);
        }
        dn_act_n<float[8], 8>(acc, q.act_dw);
#pragma unroll
        for (int e = 0; e < 8; ++e) xf[ks][e] = (half_t)acc[e];
    }
    // ---- the projection: KSF full steps, then the bias step (pw_direct_kernel's last step with kb >= K)
    const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    const half8 ones = {(half_t)1.f, (half_t)1.f, 0, 0, 0, 0, 0, 0};
    const half_t bhi = (half_t)bl;
    const half8 bw = {bhi, (half_t)(bl - (float)bhi), 0, 0, 0, 0, 0, 0};
    const bool bcol = kb == K;
    floatx16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KSF; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[ks], xf[ks], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(bcol ? bw : zero8, bcol ? ones : zero8, acc, 0, 0, 0);
    act16(acc, a.act);
    if (has_res) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const half4 rr = __builtin_bit_cast(half4, rres[g]);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[4 * g + e] += (float)rr[e];
        }
    }
    uint2v p[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        half4 hv;
#pragma unroll
        for (int e = 0; e < 4; ++e) hv[e] = (half_t)acc[4 * g + e];
        p[g] = __builtin_bit_cast(uint2v, hv);
    }
    uint4 lo4, hi4;
    {
        const uint2v s0 = __builtin_amdgcn_permlane32_swap(p[0][0], p[1][0], false, false);
        const uint2v s1 = __builtin_amdgcn_permlane32_swap(p[0][1], p[1][1], false, false);
        const uint2v s2 = __builtin_amdgcn_permlane32_swap(p[2][0], p[3][0], false, false);
        const uint2v s3 = __builtin_amdgcn_permlane32_swap(p[2][1], p[3][1], false, false);
        lo4 = make_uint4(s0[0], s1[0], s0[1], s1[1]);
        hi4 = make_uint4(s2[0], s3[0], s2[1], s3[1]);
    }
    half_t* orow = reinterpret_cast<half_t*>(a.out) + (size_t)row * NC + hh * 8;
    const int c0 = hh * 8;
    if (row < mend) {
        if (c0 < NC) *reinterpret_cast<uint4*>(orow) = lo4;
        if (c0 + 16 < NC) *reinterpret_cast<uint4*>(orow + 16) = hi4;
    }
}

// The same launch with its input staged through LDS (DN_PW_DW_LDS, default on; 0 = the body above). Above, a wave asks the L1 for every
// input line up to ten times (nine taps of neighbouring pixels, then the centre line once more in the accumulator's layout as the residual):
// 9.5 KB requested for 1 KB of unique input per 32-pixel tile, on 64-bit addresses with a select each, by waves that live for one round trip.
// Here a workgroup owns a BAND of consecutive pixels of one image in flattened (y, x) order (DN_PW_DW_BAND pixels; the last band of an image
// is short, no band crosses an image, and the XCD grouping is the launcher's: xcd_image_of):
//   * the band plus `halo` >= W + 1 pixels either side enters LDS once, as whole 128-byte lines (the halo is a multiple of 4 pixels): 16-byte
//     loads through a per-image raw buffer -- what lies above or below the image reads as zeros, so the pad rows need no test -- and ds_write_b128;
//   * a wave walks the band's 32-pixel tiles (tile = wave, wave + 4, ...): the projection's weight fragment, the bias columns and the depthwise
//     weights / bias of the lane's channel half (selected ONCE, kept in registers) are set up once per band and not once per 32 pixels;
//   * the nine taps are ds_read_b128 at per-lane offsets that do not change from tile to tile (one 32-bit add per tap); columns -1 and W are
//     masked by ADDRESS -- the lane reads a zero slot instead -- so no select touches freshly loaded data;
//   * the residual is the staged centre pixel read in the accumulator's layout (ds_read_b64): the global residual loads are gone.
// Swizzle: ds_read_b128 serves a wave in four groups of 16 lanes ({0-3, 12-15, 20-27} + ...) over 64 banks = 16 chunks of 16 bytes. A wave's tap
// is 1 KB of consecutive chunks (2 KSF per pixel), lane (r, hh) on chunk 2 KSF (s + r) + 2 ks + hh: within a group the chunks collide in pairs
// (KSF = 1) or fours (KSF = 2) whatever the tap's shift s. Chunk c is therefore kept at c ^ ((c >> 4) & (2 KSF - 1)): the pixels of a group that
// share (pixel mod 8 / KSF) differ in exactly the bits that are folded in, every tap of every tile is conflict-free, and because a wave's next
// tile is 128 pixels further the folded bits are per-lane constants (they live in the tap offsets).
// Arithmetic: bias first, taps in (ky, kx) order through v_fma_mix_f32, dn_act_n, one rounding, the projection with its bias step, act16, the
// residual in fp32, the permlane epilogue -- the body above, value for value; tests/test_gpu_pw_dw_lds.py holds both to the two-launch pair bit for bit.
// Measured (profiles/pw_dw_lds_ab.txt; 64 images, 160 x 160 x 16): 35.3 -> 25.9 us per launch with one forward at a time, 47.3 -> 40.1 with three
// in flight (rocprofv3); vector-memory read instructions 768 000 -> 102 400 per launch (15 per 32-pixel tile -> 10 per wave and band), L1 accesses
// 17.4 M -> 2.25 M; LDS: 3.0 M cycles of which 0.33 M bank conflicts (the 8-byte residual reads, two-way; the taps have none). 122 registers, no
// scratch, four workgroups per compute unit. What the loop leaves per tile is about 160 vector instructions, 72 of them the depthwise multiply-adds:
// the launch is closer to vector-issue than to its memory bound now. Band length: 640 pixels on the 160-wide map (31 KB: halo 1.5 x) beat 320, 512,
// 800 and 1280 alone on the chip (30.6 against 35.5 / 32.1 / 34.0 / 35.1 us); keeping the depthwise weights in scalar registers and selecting
// per tile (91 registers, five workgroups per compute unit) was slower (36.3 us): residency is not what this launch lacks.
constexpr int PW_DW_LDS_MAX = 64 * 1024;      // LDS of a workgroup: band + two halos + the zero slot (launch_pw_dw_direct falls back to the body above beyond it)

__device__ __forceinline__ void fma_mix_h8_from(float (&acc)[8], const float (&c)[8], const uint4& e, const uint4& w) {
    // acc = c + e * w: fma_mix_h8's first step without the copy of c
    const unsigned ee[4] = {e.x, e.y, e.z, e.w}, ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        asm volatile("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,1,0]" : "=v"(acc[2 * i]) : "v"(ee[i]), "v"(ww[i]), "v"(c[2 * i]));
        asm volatile("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,1,0]" : "=v"(acc[2 * i + 1]) : "v"(ee[i]), "v"(ww[i]), "v"(c[2 * i + 1]));
    }
}

template <int KSF>
__global__ __launch_bounds__(256, KSF == 1 ? 4 : 2) void pw_dw_direct_lds_kernel(PwDwArgs q, int n, int bands, int band, int halo) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pdl_lds[];
    constexpr int PB = 32 * KSF;                           // bytes per pixel
    constexpr unsigned SWM = 2 * KSF - 1;                  // chunk bits of a pixel: byte address A lives at A ^ (((A >> 8) & SWM) << 4)
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const PwArgs& a = q.pw;
    const int lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int K = 16 * KSF;
    const int NC = a.cout;
    int img, bi;
    if (!xcd_image_of(blockIdx.x, bands, a.xq, n, img, bi)) return;      // workgroup-uniform
    const int b0 = bi * band, blen = min(band, a.hw - b0);               // the band: pixels [b0, b0 + blen) of the image
    const int nslots = blen + 2 * halo;                                  // slot s holds pixel b0 - halo + s
    const unsigned zoff = (unsigned)nslots * PB;                         // the zero slot: 64 bytes, so that a K step's chunk bit stays inside it
    // ---- staging: every 16-byte chunk of the slots, eight requests per thread in flight (a 640-pixel band of the 160-wide map: one batch)
    {
        const __amdgpu_buffer_rsrc_t xrs =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(a.x + (size_t)img * a.hw * K), 0, a.hw * PB, 0x00020000);
        const int chunks = nslots * (2 * KSF);
        const unsigned g0 = (unsigned)((b0 - halo) * PB);                // byte offset of slot 0 in the image: "negative" = far out of range = zeros
        for (int c0 = threadIdx.x; c0 < chunks; c0 += 8 * 256) {
            u32x4 v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c = c0 + i * 256;
                v[i] = __builtin_amdgcn_raw_buffer_load_b128(xrs, c < chunks ? g0 + (unsigned)c * 16u : 0x80000000u, 0, 0);
            }
            // (pinned: left alone, every request sinks into the guarded store that uses it, one round trip after the other)
            asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]));
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const unsigned A = (unsigned)(c0 + i * 256) * 16u;
                if (c0 + i * 256 < chunks) *reinterpret_cast<u32x4*>(pdl_lds + (A ^ (((A >> 8) & SWM) << 4))) = v[i];
            }
        }
        if (threadIdx.x < 4) *reinterpret_cast<u32x4*>(pdl_lds + zoff + threadIdx.x * 16) = u32x4{0u, 0u, 0u, 0u};
    }
    // ---- once per band: the projection's operands, the depthwise weights / bias of this lane's channel half
    const int nrow = min(r, NC - 1);
    const half_t* wpt = a.w + (size_t)nrow * K + hh * 8;
    half8 wf[KSF];
#pragma unroll
    for (int ks = 0; ks < KSF; ++ks) wf[ks] = *reinterpret_cast<const half8*>(wpt + ks * 16);
    const float bl = a.bias[nrow];
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    typedef float f4v __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(4))) u4v* cp4;
    typedef const __attribute__((address_space(4))) f4v* cpf4;
    uint4 wsel[KSF][9];
    float bsel[KSF][8];
#pragma unroll
    for (int ks = 0; ks < KSF; ++ks) {
        const cpf4 bp = (cpf4)(q.bd + ks * 16);
        const f4v c0 = bp[0], c1 = bp[1], c2 = bp[2], c3 = bp[3];
#pragma unroll
        for (int e = 0; e < 4; ++e) { bsel[ks][e] = hh ? c2[e] : c0[e]; bsel[ks][4 + e] = hh ? c3[e] : c1[e]; }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const cp4 wp = (cp4)(q.wd + t * K + ks * 16);
            const u4v w0 = wp[0], w1 = wp[1];
            wsel[ks][t] = make_uint4(hh ? w1[0] : w0[0], hh ? w1[1] : w0[1], hh ? w1[2] : w0[2], hh ? w1[3] : w0[3]);
        }
    }
    const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    const half8 ones = {(half_t)1.f, (half_t)1.f, 0, 0, 0, 0, 0, 0};
    const half_t bhi = (half_t)bl;
    const half8 bw = {bhi, (half_t)(bl - (float)bhi), 0, 0, 0, 0, 0, 0};
    const bool bcol = hh == 0;                             // (kb == K: hh = 0 carries the bias columns, hh = 1 zeros)
    const half8 wlast = bcol ? bw : zero8, xlast = bcol ? ones : zero8;
    const bool has_res = a.residual != nullptr;
    // per-lane tap offsets relative to the lane's own slot: the tap's pixel shift plus this lane's chunk with the swizzle bits of the tap's slot
    // folded in. Those bits are bits 3 (KSF = 1) / 2..3 (KSF = 2) of the slot index, and a wave's tiles are 128 slots apart: constants.
    int toff[9], roff;
    {
        const int s0 = wave * 32 + r + halo;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int d = (t / 3 - 1) * q.w + (t % 3 - 1);
            const unsigned sw = (((unsigned)(s0 + d) * PB >> 8) & SWM) << 4;
            toff[t] = d * PB + (int)((unsigned)(hh * 16) ^ sw);
        }
        roff = (int)((((unsigned)s0 * PB >> 8) & SWM) << 4);            // the centre slot's bits, for the residual's chunks
    }
    __syncthreads();
    half_t* const obase = reinterpret_cast<half_t*>(a.out) + ((size_t)img * a.hw + b0) * NC + hh * 8;
    const int ntiles = (blen + 31) >> 5;
    for (int t = wave; t < ntiles; t += 4) {
        const int pl = t * 32 + r, plc = min(pl, blen - 1);               // this lane's pixel in the band (a ragged last tile: clamped, not stored)
        const unsigned p = (unsigned)(b0 + plc);
        const int px = (int)(p - fd_div(p, q.fd_w) * (unsigned)q.w);
        const bool okl = px > 0, okr = px < q.w - 1;
        const unsigned S = (unsigned)(plc + halo) * PB;
        // (a clamped lane keeps the offsets of its unclamped slot: its folded bits may differ from its slot's, which only permutes the chunks of pixels
        // that ARE staged -- the lane's values are never stored)
        unsigned ad[9];
#pragma unroll
        for (int tp = 0; tp < 9; ++tp) {
            const unsigned A = S + (unsigned)toff[tp];
            ad[tp] = (tp % 3 == 0) ? (okl ? A : zoff) : (tp % 3 == 2) ? (okr ? A : zoff) : A;
        }
        half8 xf[KSF];
#pragma unroll
        for (int ks = 0; ks < KSF; ++ks) {
            half8 xin[9];
            // (chunk 2 ks + hh with the slot's bits folded in: everything else in the address is a multiple of 64, so the K step is bit 5)
#pragma unroll
            for (int tp = 0; tp < 9; ++tp) xin[tp] = *reinterpret_cast<const half8*>(pdl_lds + (ad[tp] ^ (unsigned)(ks * 32)));
            float acc[8];
            fma_mix_h8_from(acc, bsel[ks], *reinterpret_cast<const uint4*>(&xin[0]), wsel[ks][0]);
#pragma unroll
            for (int tp = 1; tp < 9; ++tp) fma_mix_h8(acc, *reinterpret_cast<const uint4*>(&xin[tp]), wsel[ks][tp]);
            dn_act_n<float[8], 8>(acc, q.act_dw);
#pragma unroll
            for (int e = 0; e < 8; ++e) xf[ks][e] = (half_t)acc[e];
        }
        uint2 rres[2 * KSF];
        if (has_res) {
            // channels 8 g + 4 hh .. + 3 of the centre pixel = chunk g, bytes 8 hh .. (a residual means cout == cin: groups beyond 2 KSF do not exist)
#pragma unroll
            for (int g = 0; g < 2 * KSF; ++g) rres[g] = *reinterpret_cast<const uint2*>(pdl_lds + S + ((unsigned)(g * 16) ^ (unsigned)roff) + hh * 8);
        }
        floatx16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KSF; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[ks], xf[ks], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wlast, xlast, acc, 0, 0, 0);
        act16(acc, a.act);
        if (has_res) {
#pragma unroll
            for (int g = 0; g < 2 * KSF; ++g) {
                const half4 rr = __builtin_bit_cast(half4, rres[g]);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[4 * g + e] += (float)rr[e];
            }
        }
        uint2v pk[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            half4 hv;
#pragma unroll
            for (int e = 0; e < 4; ++e) hv[e] = (half_t)acc[4 * g + e];
            pk[g] = __builtin_bit_cast(uint2v, hv);
        }
        const uint2v s0 = __builtin_amdgcn_permlane32_swap(pk[0][0], pk[1][0], false, false);
        const uint2v s1 = __builtin_amdgcn_permlane32_swap(pk[0][1], pk[1][1], false, false);
        const uint2v s2 = __builtin_amdgcn_permlane32_swap(pk[2][0], pk[3][0], false, false);
        const uint2v s3 = __builtin_amdgcn_permlane32_swap(pk[2][1], pk[3][1], false, false);
        const uint4 lo4 = make_uint4(s0[0], s1[0], s0[1], s1[1]), hi4 = make_uint4(s2[0], s3[0], s2[1], s3[1]);
        half_t* orow = obase + (size_t)pl * NC;
        const int c0 = hh * 8;
        if (pl < blen) {
            if (c0 < NC) *reinterpret_cast<uint4*>(orow) = lo4;
            if (c0 + 16 < NC) *reinterpret_cast<uint4*>(orow + 16) = hi4;
        }
    }
}


// Weight-stationary variant for the EXPANSIONS (round 6): cin <= 128, no squeeze-excitation scale, no residual -- 24 -> 72 on the 80 x 80 map,
// 40 -> 120, 80 -> 480, 112 -> 672 (mobilenetv3.py:76 expand ConvBNActivation) and the V2 expansions that run as launches of their own.
// What the lab (tools/pw_lab.hip, ablations + in-kernel stamps, LAB_NOTEBOOK R6) found about pw_stream_kernel on 112 -> 672 (17.2 us by rocprofv3):
// 6.5 us remain with every memory operation removed, the weight requests cost 4.5, the stores 5.1, the x requests 3.2 -- and they ADD, because (a) a
// wave's fragment loads are 32-byte pieces of 32 different rows per instruction (32 tag lookups each; with 8 - 12 waves per CU the lines leave L1
// between the K steps that use them: 13 M L1 accesses for a 40 MB layer), (b) loads and stores retire in order, so the wait for the next weight
// tile is also a wait for the previous tile's stores, (c) one round of workgroups runs load | compute | store in lockstep over the chip.
// Here
//   * a wave keeps the A fragments of its RUN of RT channel tiles in registers for its whole life (staged once per workgroup through LDS from
//     the fragment-major copy: 1 KB contiguous per LDS-DMA instruction; the bias joins as the (hi, lo) columns of the last K step);
//   * it walks over 32-row pixel tiles: a tile of x is 64 cin CONTIGUOUS bytes, fetched by LDS-DMA as whole cache lines into the wave's own LDS
//     buffer and read back as B fragments with ds_read_b128 -- the next tile's DMA is in flight during the matrix + epilogue work of this one;
//   * no vector-memory load is waited for inside a tile, and the wait at the end of a tile is COUNTED: this tile's stores (buffer stores with an
//     out-of-range offset for masked lanes, so their number is fixed) stay in flight behind it;
//   * the tile leaves as 64-byte pieces (v_permlane32_swap + v_permlane16_swap: four lanes per pixel row and store instruction).
// Arithmetic per output = pw_direct_kernel's (same K order, bias in the reduction, one rounding): bit-identical to it (test_pointwise_wstat_*).
__device__ __forceinline__ void pw_glds16(const void* gsrc, unsigned dst) {
    // LDS-DMA behind the compiler's back (headfuse.hip: as a builtin every later ds_read would wait for vmcnt(0)); M0 saved and restored
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(dst) : "memory");
}

//
// PROJ (the narrow projections, cout <= 64: runs == 1, RT = every channel tile of the layer; pw_wstat_proj_supported): the same walk with pw_direct_kernel<KSF, 1>'s
// squeeze-excitation scale and residual. hw % 32 == 0, so a tile lies inside one image: the K floats of that image's scale row and the tile's residual rows
// (32 x cout x 2 contiguous bytes) are requested WITH the tile's x into the wave's buffer ([x: ksw KB][scale: 1 KB][residual: 64 cout bytes in 1 KB pieces]) and
// read back with it -- the scale row in front of the B fragments ((half)((float)x * s): v_mul_f32 + v_cvt_f16_f32, the rounding of pw_direct_kernel), the residual in
// the accumulator layout, added in fp32 behind the activation. Same K order, same rounding points: bit-identical to pw_direct_kernel (tests/test_gpu_pw_wstat_proj.py).
template <int KS1, int RT, bool PROJ>
__global__ __launch_bounds__(256) void pw_wstat_kernel(PwArgs a, int runs, int wg_per_group) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pws_lds[];
    constexpr int KSF = KS1 - 1;
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int K = a.cin, NC = a.cout;
    const int ksw = (K + 15) >> 4;                       // K steps of the fragment-major copy (a tail step holds zeros in its upper half)
    // XCD grouping as everywhere (pw_tile_rows): the workgroups with equal (flat index % 8) own the rows of one group of a.xq images
    int r0, mend, w;
    if (a.xq > 0) {
        const int g = blockIdx.x & 7;
        w = blockIdx.x >> 3;
        r0 = g * a.xq * a.hw;
        mend = min(a.m, r0 + a.xq * a.hw);
    } else {
        w = blockIdx.x; r0 = 0; mend = a.m;
    }
    const int run = w % runs, wgq = w / runs;
    const int Q = (wg_per_group / runs) * 4;             // pixel tiles between two tiles of one wave
    const int n_units = mend > r0 ? (mend - r0 + 31) >> 5 : 0;
    const int ctiles = (NC + 31) >> 5;
    const int ct0 = run * RT;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)pws_lds;
    const int rkb = PROJ ? (NC * 64 + 1023) >> 10 : 0;                                // PROJ: 1 KB pieces of a tile's residual rows
    const int wbuf = (ksw + (PROJ ? 1 + rkb : 0)) * 1024;
    const unsigned xoff = (unsigned)(RT * ksw * 1024 + wave * wbuf);                // this wave's x buffer: ksw pieces of 1 KB >= 64 K bytes
    const unsigned soff = xoff + (unsigned)ksw * 1024u, roff = soff + 1024u;        // PROJ: the scale row and the residual rows behind it
    const bool has_se = PROJ && a.se != nullptr, has_res = PROJ && a.residual != nullptr;
    auto dma_x = [&](int u) {
        const long row0 = (long)r0 + (long)u * 32;
        const unsigned char* src = reinterpret_cast<const unsigned char*>(a.x + row0 * K);
        const unsigned lim = (unsigned)min((long)(a.m - row0) * K * 2 - 16, 0x7fffffffL);           // the last 16 bytes of the tensor
#pragma unroll 1
        for (int p = 0; p < ksw; ++p) pw_glds16(src + min((unsigned)(p * 1024 + lane * 16), lim), lds0 + xoff + p * 1024);
        if constexpr (PROJ) {
            if (has_se) {        // (the lanes beyond the row's 4 K bytes fetch its last 16 again)
                const unsigned char* ssrc = reinterpret_cast<const unsigned char*>(a.se + (size_t)((int)row0 / a.hw) * K);
                pw_glds16(ssrc + min((unsigned)(lane * 16), (unsigned)(K * 4 - 16)), lds0 + soff);
            }
            if (has_res) {
                const unsigned char* rsrc = reinterpret_cast<const unsigned char*>(a.residual + row0 * NC);
                const unsigned rlim = (unsigned)min((long)(a.m - row0) * NC * 2 - 16, 0x7fffffffL);
#pragma unroll 1
                for (int p = 0; p < rkb; ++p) pw_glds16(rsrc + min((unsigned)(p * 1024 + lane * 16), rlim), lds0 + roff + p * 1024);
            }
        }
    };
    int u = wgq * 4 + wave;
    if (u < n_units) dma_x(u);
    {
        const unsigned char* wsrc = reinterpret_cast<const unsigned char*>(a.wfrag) + (size_t)ct0 * ksw * 1024 + lane * 16;
        const int pieces = max(min(RT, ctiles - ct0), 0) * ksw;
#pragma unroll 1
        for (int p = wave; p < pieces; p += 4) pw_glds16(wsrc + (size_t)p * 1024, lds0 + p * 1024);
    }
    float bl[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) bl[t] = a.bias[min((ct0 + t) * 32 + r, NC - 1)];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int kb = KSF * 16 + hh * 8;                    // first column of this lane in the last step: < K data, == K the bias columns, > K nothing
    const bool data = kb < K, bcol = kb == K;
    const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    half8 wf[RT][KS1];
    {
        const half8* wl = reinterpret_cast<const half8*>(pws_lds) + lane;
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            const int tt = min(t, max(ctiles - ct0 - 1, 0));                          // (a run's tiles beyond the last: a valid tile again, never stored)
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks) wf[t][ks] = wl[(tt * ksw + min(ks, ksw - 1)) * 64];
            const half_t hi = (half_t)bl[t];
            const half8 bw = {hi, (half_t)(bl[t] - (float)hi), 0, 0, 0, 0, 0, 0};
            wf[t][KSF] = data ? wf[t][KSF] : (bcol ? bw : zero8);
        }
    }
    const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(a.out, 0, (int)((unsigned)a.m * (unsigned)NC * 2u), 0x00020000);
    const half8 ones = {(half_t)1.f, (half_t)1.f, 0, 0, 0, 0, 0, 0};
    const unsigned xrd = xoff + (unsigned)r * (unsigned)K * 2u;                       // this lane's row in the wave's x buffer
    const unsigned xlast = (unsigned)min(kb, K - 8) * 2u;
    const int colq = 8 * ((lane >> 5) + 2 * ((lane >> 4) & 1));
    const int act = a.act;
    for (; u < n_units; u += Q) {
        half8 xf[KS1];
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) xf[ks] = *reinterpret_cast<const half8*>(pws_lds + xrd + (ks < KSF ? (unsigned)(ks * 32 + hh * 16) : xlast));
        float4 sv[PROJ ? KS1 : 1][2];
        uint2 rres[RT][4];
        if constexpr (PROJ) {
            if (has_se) {
#pragma unroll
                for (int ks = 0; ks < KS1; ++ks) {        // this lane's columns of the step: what pw_direct_kernel reads from a.se
                    const float4* sp = reinterpret_cast<const float4*>(pws_lds + soff + (ks < KSF ? (unsigned)(ks * 64 + hh * 32) : 2u * xlast));
                    sv[ks][0] = sp[0]; sv[ks][1] = sp[1];
                }
            }
            if (has_res) {
                const unsigned char* rp = pws_lds + roff + (unsigned)r * (unsigned)NC * 2u;
#pragma unroll
                for (int t = 0; t < RT; ++t)
#pragma unroll
                    for (int g = 0; g < 4; ++g) rres[t][g] = *reinterpret_cast<const uint2*>(rp + min((ct0 + t) * 32 + 8 * g + 4 * hh, NC - 4) * 2);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (u + Q < n_units) dma_x(u + Q);
        if constexpr (PROJ) {
            if (has_se) {
#pragma unroll
                for (int ks = 0; ks < KS1; ++ks) {
                    const float s[8] = {sv[ks][0].x, sv[ks][0].y, sv[ks][0].z, sv[ks][0].w, sv[ks][1].x, sv[ks][1].y, sv[ks][1].z, sv[ks][1].w};
#pragma unroll
                    for (int e = 0; e < 8; ++e) xf[ks][e] = (half_t)((float)xf[ks][e] * s[e]);
                }
            }
        }
        xf[KSF] = data ? xf[KSF] : (bcol ? ones : zero8);
        const int rr = r0 + u * 32 + (lane & 15);
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            floatx16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[t][ks], xf[ks], acc, 0, 0, 0);
            act16(acc, act);
            if constexpr (PROJ) {
                if (has_res) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const half4 rq = __builtin_bit_cast(half4, rres[t][g]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[4 * g + e] += (float)rq[e];
                    }
                }
            }
            uint2v p[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                half4 hv;
#pragma unroll
                for (int e = 0; e < 4; ++e) hv[e] = (half_t)acc[4 * g + e];
                p[g] = __builtin_bit_cast(uint2v, hv);
            }
            // permlane32: lane r <- channels 0..7 / 16..23, lane r + 32 <- 8..15 / 24..31 of pixel r (pw_direct_kernel); permlane16 on top: rows 0..15 of
            // the tile end up in one register set with FOUR lanes per row (64 contiguous bytes per row and store instruction), rows 16..31 in the other
            const uint2v s0 = __builtin_amdgcn_permlane32_swap(p[0][0], p[1][0], false, false);
            const uint2v s1 = __builtin_amdgcn_permlane32_swap(p[0][1], p[1][1], false, false);
            const uint2v s2 = __builtin_amdgcn_permlane32_swap(p[2][0], p[3][0], false, false);
            const uint2v s3 = __builtin_amdgcn_permlane32_swap(p[2][1], p[3][1], false, false);
            const uint2v q0 = __builtin_amdgcn_permlane16_swap(s0[0], s2[0], false, false);
            const uint2v q1 = __builtin_amdgcn_permlane16_swap(s1[0], s3[0], false, false);
            const uint2v q2 = __builtin_amdgcn_permlane16_swap(s0[1], s2[1], false, false);
            const uint2v q3 = __builtin_amdgcn_permlane16_swap(s1[1], s3[1], false, false);
            const u32x4 lo4 = {q0[0], q1[0], q2[0], q3[0]}, hi4 = {q0[1], q1[1], q2[1], q3[1]};
            const int col = (ct0 + t) * 32 + colq;
            const unsigned off = ((unsigned)rr * (unsigned)NC + (unsigned)col) * 2u;
            const bool okc = col < NC;
            __builtin_amdgcn_raw_buffer_store_b128(lo4, ors, (okc && rr < mend) ? off : 0x80000000u, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(hi4, ors, (okc && rr + 16 < mend) ? off + 32u * (unsigned)NC : 0x80000000u, 0, 0);
        }
        // the next tile of x must have landed; this tile's 2 RT stores stay in flight (always issued: masked lanes carry an out-of-range offset)
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * RT) : "memory");
    }
}

template <int KS1, int RT>
int launch_wstat_proj_t(const PwArgs& a, hipStream_t s) {
    const int groups = a.xq > 0 ? 8 : 1;
    const long rows = a.xq > 0 ? (long)a.xq * a.hw : a.m;
    const int units = dn_cdiv(rows, 32);
    const int ksw = dn_cdiv(a.cin, 16);
    const int lds = (RT * ksw + 4 * (ksw + 1 + dn_cdiv(a.cout * 64, 1024))) * 1024;
    // workgroups per group of rows: two per compute unit (64 KB of LDS at 120 -> 40), fewer when there are not that many pixel tiles. Measured at 400 tiles per
    // group (profiles/pw_wstat_proj_ab.txt, 120 -> 40 / 72 -> 40, us): 64 per group 11.15 / 7.92, 50 (every wave two tiles) 10.98 / 8.18, 32 12.10 / 9.29, 96 12.27 / 9.14.
    // DN_PW_WSTAT_PROJ_WGS (workgroups per launch) is there for that sweep and for the tests, which shrink the grid so that a wave walks many tiles.
    const int wpg = std::max(1, std::min(std::max(1, dn_knob("DN_PW_WSTAT_PROJ_WGS", 512)) / groups, dn_cdiv(units, 4)));
    if (lds > 64 * 1024) DN_HIP_CHECK(dn_allow_big_lds(reinterpret_cast<const void*>(pw_wstat_kernel<KS1, RT, true>)));
    // The label stays that of the launch whose body this replaces (pw_direct_kernel<KSF, 1>): the plan's launch list, its owners and bench.py's families
    // know the launch by it (tests/test_gpu_plan_signature.py).
    dn_note_kernel("pw_direct_kernel<%d,%d>", KS1 - 1, 1);
    hipLaunchKernelGGL((pw_wstat_kernel<KS1, RT, true>), dim3((unsigned)(groups * wpg)), dim3(256), lds, s, a, 1, wpg);
    return DN_OK;
}

template <int KS1, int RT>
int launch_wstat_t(const PwArgs& a, hipStream_t s) {
    const int ctiles = dn_cdiv(a.cout, 32), runs = dn_cdiv(ctiles, RT);
    const int groups = a.xq > 0 ? 8 : 1;
    const long rows = a.xq > 0 ? (long)a.xq * a.hw : a.m;
    const int units = dn_cdiv(rows, 32);
    // two workgroups per compute unit (188 registers at KS1 RT = 24: two waves per SIMD), fewer when there are not that many pixel tiles
    int wpg = std::min(512 / groups, dn_cdiv(units, 4) * runs);
    wpg = std::max(runs, wpg / runs * runs);
    const int ksw = dn_cdiv(a.cin, 16);
    const int lds = (RT + 4) * ksw * 1024;
    dn_note_kernel("pw_wstat_kernel<%d,%d>", KS1, RT);
    hipLaunchKernelGGL((pw_wstat_kernel<KS1, RT, false>), dim3((unsigned)(groups * wpg)), dim3(256), lds, s, a, runs, wpg);
    return DN_OK;
}

template <int KSF, int TC>
int launch_t(const PwArgs& a, int wc_log, hipStream_t s) {
    const int BP = 32 * (4 >> wc_log), BC = (32 * TC) << wc_log;
    const int tiles = a.xq > 0 ? dn_cdiv((long)a.xq * a.hw, BP) : dn_cdiv(a.m, BP);
    const dim3 grid((unsigned)(a.xq > 0 ? 8 * tiles : tiles) * dn_cdiv(a.cout, BC));
    dn_note_kernel("pw_direct_kernel<%d,%d>", KSF, TC);
    hipLaunchKernelGGL((pw_direct_kernel<KSF, TC>), grid, dim3(256), 0, s, a, tiles, wc_log);
    return DN_OK;
}

}  // namespace

bool pw_dw_direct_supported(const PwArgs& a, const DwArgs& d) {
    return dn_knob("DN_PW_DW", 1) != 0 && pw_direct_supported(a) && !a.se && (a.cin == 16 || a.cin == 32) && a.cout <= 32 && d.c == a.cin && d.k == 3 &&
           d.stride == 1 && d.pad == 1 && !d.pool && d.ho == d.h && d.wo == d.w_ && a.hw == d.h * d.w_ && (!a.residual || (a.residual == d.x && a.cout == a.cin)) &&
           a.hw >= 32 && fd_ok((unsigned long long)a.hw, (unsigned)d.w_);
}

// The LDS body's geometry (pw_dw_direct_lds_kernel): band length, halo and LDS bytes of a workgroup; false where the staging does not fit
// (a band plus two halos of W + 1 pixels beyond PW_DW_LDS_MAX: very wide maps) or the per-image raw buffer's 32-bit byte offsets would not hold.
struct PwDwLds { int band, halo, bands, lds; };
static bool pw_dw_lds_geometry(const PwArgs& a, const DwArgs& d, PwDwLds& g) {
    const int pb = a.cin * 2;
    g.band = std::max(32, dn_knob("DN_PW_DW_BAND", DN_PW_DW_BAND) & ~31);      // (whole 32-pixel tiles: only an image's last band is ragged)
    g.halo = (d.w_ + 1 + 3) & ~3;
    g.bands = dn_cdiv(a.hw, g.band);
    const long lds = ((long)std::min(g.band, a.hw) + 2L * g.halo) * pb + 64;
    g.lds = (int)std::min(lds, (long)PW_DW_LDS_MAX + 1);
    return lds <= PW_DW_LDS_MAX && (long)a.hw * pb < (1L << 31) && (long)(d.n + 7) * g.bands < (1L << 31);
}

int launch_pw_dw_direct(const PwArgs& a, const DwArgs& d, hipStream_t s) {
    DN_REQUIRE(pw_dw_direct_supported(a, d), "depthwise + pointwise (direct): unsupported cin=%d cout=%d", a.cin, a.cout);
    PwDwArgs q{};
    q.pw = a;
    q.pw.x = d.x;
    q.wd = d.w; q.bd = d.bias; q.h = d.h; q.w = d.w_; q.act_dw = d.act;
    q.inv_hw = 1.0f / (float)a.hw; q.fd_w = fastdiv((unsigned)d.w_);
    dn_note_kernel("pw_dw_direct_kernel<%d>", a.cin / 16);
    PwDwLds g;
    if (dn_knob("DN_PW_DW_LDS", 1) != 0 && a.m == (long)d.n * a.hw && pw_dw_lds_geometry(a, d, g)) {
        const dim3 grid((unsigned)(a.xq > 0 ? 8 * a.xq : d.n) * g.bands);
        if (a.cin == 16) hipLaunchKernelGGL((pw_dw_direct_lds_kernel<1>), grid, dim3(256), g.lds, s, q, d.n, g.bands, g.band, g.halo);
        else hipLaunchKernelGGL((pw_dw_direct_lds_kernel<2>), grid, dim3(256), g.lds, s, q, d.n, g.bands, g.band, g.halo);
        return DN_OK;
    }
    const int tiles = a.xq > 0 ? dn_cdiv((long)a.xq * a.hw, 128) : dn_cdiv(a.m, 128);
    const dim3 grid((unsigned)(a.xq > 0 ? 8 * tiles : tiles));
    if (a.cin == 16) hipLaunchKernelGGL((pw_dw_direct_kernel<1>), grid, dim3(256), 0, s, q, tiles);
    else hipLaunchKernelGGL((pw_dw_direct_kernel<2>), grid, dim3(256), 0, s, q, tiles);
    return DN_OK;
}

// the pwdirect.hip arms of launch_pointwise's switch (choice.h: pw_choose)
int launch_pw_direct(const PwArgs& a, const PwChoice& c, hipStream_t s) {
    const int ctiles = dn_cdiv(a.cout, 32);
    if (c.kernel == PwChoice::PW_WSTAT) {
        switch (c.k * 10 + c.t) {
#define DN_PWS_CASE(k, t) case k * 10 + t: return launch_wstat_t<k, t>(a, s);
            DN_PWS_CASE(2, 2) DN_PWS_CASE(2, 3) DN_PWS_CASE(2, 4) DN_PWS_CASE(3, 2) DN_PWS_CASE(3, 3) DN_PWS_CASE(3, 4) DN_PWS_CASE(4, 2) DN_PWS_CASE(4, 3) DN_PWS_CASE(4, 4)
            DN_PWS_CASE(5, 2) DN_PWS_CASE(5, 3) DN_PWS_CASE(5, 4) DN_PWS_CASE(6, 2) DN_PWS_CASE(6, 3) DN_PWS_CASE(6, 4) DN_PWS_CASE(7, 2) DN_PWS_CASE(7, 3)
            DN_PWS_CASE(8, 2) DN_PWS_CASE(8, 3) DN_PWS_CASE(9, 2)
#undef DN_PWS_CASE
        }
    } else if (c.kernel == PwChoice::PW_STREAM) {
        // channel runs sized so that all waves are resident at once
        const long ptiles = dn_cdiv(a.m, 32 * c.t);
        int runs = (int)std::max(1L, std::min((long)ctiles, (long)2800 / ptiles));
        const int per = dn_cdiv(ctiles, runs);
        runs = dn_cdiv(ctiles, per);
        switch (c.k * 10 + c.t) {
            case 42: return launch_stream_t<4, 2>(a, runs, per, s);
            case 52: return launch_stream_t<5, 2>(a, runs, per, s);
            case 62: return launch_stream_t<6, 2>(a, runs, per, s);
            case 72: return launch_stream_t<7, 2>(a, runs, per, s);
            case 82: return launch_stream_t<8, 2>(a, runs, per, s);
        }
    } else if (c.kernel == PwChoice::PW_DIRECT && c.t == 2) {
        const int wc_log = ctiles <= 2 ? 0 : ctiles <= 4 ? 1 : 2;
        switch (c.k) {
#define DN_PWD_CASE2(k) case k: return launch_t<k, 2>(a, wc_log, s);
            DN_PWD_CASE2(0) DN_PWD_CASE2(1) DN_PWD_CASE2(2) DN_PWD_CASE2(3) DN_PWD_CASE2(4) DN_PWD_CASE2(5) DN_PWD_CASE2(6) DN_PWD_CASE2(7) DN_PWD_CASE2(8)
#undef DN_PWD_CASE2
        }
    } else if (c.kernel == PwChoice::PW_DIRECT && c.proj) {
        // the weight-stationary body of the narrow projections: KS1 = k + 1 steps, every channel tile of the layer (one or two) in the wave
        switch ((c.k + 1) * 10 + ctiles) {
#define DN_PWP_CASE(k) case k * 10 + 1: return launch_wstat_proj_t<k, 1>(a, s); case k * 10 + 2: return launch_wstat_proj_t<k, 2>(a, s);
            DN_PWP_CASE(2) DN_PWP_CASE(3) DN_PWP_CASE(4) DN_PWP_CASE(5) DN_PWP_CASE(6) DN_PWP_CASE(7) DN_PWP_CASE(8) DN_PWP_CASE(9)
#undef DN_PWP_CASE
        }
    } else if (c.kernel == PwChoice::PW_DIRECT) {
        const int wc_log = ctiles <= 1 ? 0 : ctiles <= 2 ? 1 : 2;
        switch (c.k) {
#define DN_PWD_CASE(k) case k: return launch_t<k, 1>(a, wc_log, s);
            DN_PWD_CASE(0) DN_PWD_CASE(1) DN_PWD_CASE(2) DN_PWD_CASE(3) DN_PWD_CASE(4) DN_PWD_CASE(5) DN_PWD_CASE(6) DN_PWD_CASE(7) DN_PWD_CASE(8)
            DN_PWD_CASE(9) DN_PWD_CASE(10) DN_PWD_CASE(11) DN_PWD_CASE(12) DN_PWD_CASE(13) DN_PWD_CASE(14) DN_PWD_CASE(15) DN_PWD_CASE(16)
#undef DN_PWD_CASE
        }
    }
    dn_set_error("pointwise (direct): no instantiation %d,%d for cin=%d cout=%d", c.k, c.t, a.cin, a.cout);
    return DN_E_UNSUPPORTED;
}
