// Fused expand + depthwise 3x3 stride 1 + project (+ residual) for the one-chunk block 24 -> 72 -> cout (the 80 x 80 block of MobileNetV3): a wave
// walks DOWN a 32-pixel column strip, expands every input row ONCE on the matrix cores and keeps the last three expanded rows in registers, already in
// the accumulator layout. A third body for the launch that expdw.hip serves (expdw_choose selects it, choice.h: DN_EXPDW_ROWS, default 1); same reference ops
// (mobilenetv3.py:72-95, BN folded).
//
// Why: at stride 1 every expanded value has nine uses, so the per-tap recompute of expdw_direct.hip does not carry over, and expdw_one_kernel pays for
// the sharing with an E tile in LDS (every value rounded, written, read back nine times), a 10 x 18 halo region per 8 x 16 tile, four barrier-separated
// phases per tile and a projection on a fraction of the waves. Here nothing of the block exists in LDS but constants:
//   * a wave owns a strip (lane r = pixel 30 strip - 1 + r of a row: lanes 0 and 31 are halo, computed and not stored) and a band of consecutive output
//     rows of one image; it expands input rows oy0 - 1 .. oy0 + rows one after the other. Per row: the B fragments are 16 contiguous bytes per lane and
//     step straight from memory (raw buffer, a pixel outside the image reads zeros), A = the w1 fragments of channel tiles 0 - 31, 32 - 63 and 64 - 71,
//     K step 0 = channels 0 - 15, the last step = channels 16 - 23 in the low half-wave and the (hi, lo) bias pair against the inside flag in the high
//     half-wave -- the two matrix steps of expdw_one_kernel<..., WIDE>, so a pixel outside the image expands to act1(0) = 0;
//   * the 36 results per lane are activated, rounded as Es was written and packed: 18 registers per row, three rows kept, the loop unrolled by three so
//     that the ring is a renaming;
//   * depthwise: bias first, taps in (ky, kx) order, v_fma_mix_f32; the vertical taps are the ring rows, the horizontal neighbours are the ring row
//     moved by one lane (DPP wave_shr:1 / wave_shl:1); weights / biases of the lane's 36 channels are LDS broadcasts (two addresses per wave);
//   * act2, one rounding, v_permlane32_swap into the projection's B fragments (K step 2 ct + s = the 16 channels Ds held, step 4 = channels 64 - 71 in
//     the low half-wave against zeros), five matrix steps, + b3 in fp32, the residual in fp32 from x, one rounding, the permlane store epilogue.
// One barrier (behind the set-up of the LDS constants), none in the loop. Same operands, same K order, same rounding points, same tap order as
// expdw_kernel<..., ONE> / expdw_one_kernel: outputs are bit-identical (tests/test_gpu_expdw_rows.py).
#include <algorithm>

#include "common.h"

namespace {

constexpr int XR_NW = 4;                // waves per workgroup
constexpr int XR_NT = XR_NW * 64;
constexpr int XR_SW = 30;               // output pixels per strip (32 lanes less the two halo lanes)
constexpr int XR_CIN = 24, XR_CEXP = 72;

typedef unsigned uint2v __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <int ACT>
__device__ __forceinline__ float xr_act(float v) {
    if constexpr (ACT == DN_ACT_RELU) return dn_relu(v);
    else if constexpr (ACT == DN_ACT_RELU6) return dn_relu6(v);
    else if constexpr (ACT == DN_ACT_HSWISH) return v * dn_relu6(v + 3.f) * (1.f / 6.f);
    else return v;
}

// the value of the lane below / above (builtins, not asm: hipcc keeps the wait states between a vector write and a DPP read)
__device__ __forceinline__ unsigned xr_from_left(unsigned v) { return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x138, 0xf, 0xf, true); }     // wave_shr:1
__device__ __forceinline__ unsigned xr_from_right(unsigned v) { return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x130, 0xf, 0xf, true); }    // wave_shl:1

__device__ __forceinline__ void fma_mix_h4(float (&acc)[4], unsigned e0, unsigned e1, const uint2v& w) {
    asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel_hi:[1,1,0]" : "+v"(acc[0]) : "v"(e0), "v"(w[0]));
    asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,1,0]" : "+v"(acc[1]) : "v"(e0), "v"(w[0]));
    asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel_hi:[1,1,0]" : "+v"(acc[2]) : "v"(e1), "v"(w[1]));
    asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,1,0]" : "+v"(acc[3]) : "v"(e1), "v"(w[1]));
}

// ACT1 is a template parameter: the activation follows a matrix instruction, and straight-line code gets its wait states from hipcc's hazard
// recognizer (expdw_direct.hip).
template <int ACT1>
__global__ __launch_bounds__(XR_NT) __attribute__((amdgpu_waves_per_eu(3, 3))) void expdw_rows_kernel(ExpDwArgs a, int per_image, int strips, int bands, int bh) {
    __shared__ __attribute__((aligned(16))) half_t Wl[2 * 9 * 2 * 16];     // [channel tile][tap][hh][16]: the lane's channels 8 g + 4 hh + e at 4 g + e
    __shared__ __attribute__((aligned(16))) uint2v Wl2[9 * 2];             // [tap][hh]: channels 64 + 4 hh + e
    __shared__ __attribute__((aligned(16))) float Bl[2 * 2 * 16];          // [channel tile][hh][16]
    __shared__ __attribute__((aligned(16))) float Bl2[2 * 4];              // [hh][4]
    __shared__ __attribute__((aligned(16))) float B3l[2 * 16];             // [hh][16]
    __shared__ __attribute__((aligned(16))) u32x4 W3l[5 * 64];             // [K step][lane]: the projection's A fragments
    __shared__ __attribute__((aligned(16))) u32x4 W1l[3 * 64];             // [channel tile][lane]: the A fragments of the expand's last step (read per row: 12 registers less)
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int img, idx;
    if (!xcd_image_of(blockIdx.x, per_image, a.xq, a.n, img, idx)) return;      // workgroup-uniform
    const int W = a.W, H = a.H, NC = a.cout;
    // ---- once per workgroup: the LDS constants
    for (int i = tid; i < 2 * 9 * 2 * 16; i += XR_NT) {
        const int j = i & 15, h2 = (i >> 4) & 1, q = i >> 5, ct = q / 9, tp = q - ct * 9;
        Wl[i] = a.wd[tp * XR_CEXP + ct * 32 + 8 * (j >> 2) + 4 * h2 + (j & 3)];
    }
    if (tid < 18) {
        const int tp = tid >> 1, h2 = tid & 1;
        const half4 w = *reinterpret_cast<const half4*>(a.wd + tp * XR_CEXP + 64 + 4 * h2);
        Wl2[tid] = __builtin_bit_cast(uint2v, w);
    }
    if (tid >= 64 && tid < 128) {
        const int i = tid - 64;
        Bl[i] = a.bd[(i >> 5) * 32 + 8 * ((i & 15) >> 2) + 4 * ((i >> 4) & 1) + (i & 3)];
    }
    if (tid >= 128 && tid < 136) Bl2[tid - 128] = a.bd[64 + tid - 128];
    if (tid >= 192 && tid < 224) {
        const int i = tid - 192;
        B3l[i] = a.b3[min(8 * ((i & 15) >> 2) + 4 * (i >> 4) + (i & 3), NC - 1)];
    }
    if (tid < 64) {
#pragma unroll
        for (int ks = 0; ks < 5; ++ks) {
            const u32x4 w = *reinterpret_cast<const u32x4*>(a.w3 + (size_t)min(r, NC - 1) * XR_CEXP + min(ks * 16 + hh * 8, XR_CEXP - 8));
            W3l[ks * 64 + lane] = (r < NC && ks * 16 + hh * 8 < XR_CEXP) ? w : u32x4{0u, 0u, 0u, 0u};
        }
    }
    // ---- the expand's A fragments: channel tiles 0 - 31, 32 - 63 and 64 - 71 (rows beyond channel 71 repeat it; their results are not read)
    const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    half8 wf[3];
#pragma unroll
    for (int ct = 0; ct < 3; ++ct) {
        const int ch = min(ct * 32 + r, XR_CEXP - 1);
        wf[ct] = *reinterpret_cast<const half8*>(a.w1 + (size_t)ch * XR_CIN + hh * 8);
        const half8 wl = *reinterpret_cast<const half8*>(a.w1 + (size_t)ch * XR_CIN + 16);
        const float b = a.b1[ch];
        const half_t hi = (half_t)b;
        const half8 bw = {hi, (half_t)(b - (float)hi), 0, 0, 0, 0, 0, 0};
        if (tid < 64) W1l[ct * 64 + lane] = __builtin_bit_cast(u32x4, hh ? bw : wl);      // (columns 16 .. 23: x; 24, 25: the bias pair; 26 .. 31: zeros)
    }
    __syncthreads();
    const int unit = idx * XR_NW + wave;                     // (band, strip), strips fastest: the waves of a workgroup share their input rows
    if (unit >= strips * bands) return;                      // wave-uniform
    const int band = unit / strips, strip = unit - band * strips;
    const int oy0 = band * bh, rows = min(bh, H - oy0);
    const int px = strip * XR_SW - 1 + r;
    const bool pin = px >= 0 && px < W;
    const __amdgpu_buffer_rsrc_t xrs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(a.x + (size_t)img * H * W * XR_CIN), 0, H * W * (XR_CIN * 2), 0x00020000);
    const unsigned OOB = 0x80000000u;                        // far out of range = zeros
    const unsigned pxo = (unsigned)(px * (XR_CIN * 2));
    // B fragments of input row i of the band (image row oy0 - 1 + i): requested a row ahead
    u32x4 xc0, xc1;
    auto request = [&](int i, u32x4& v0, u32x4& v1) __attribute__((always_inline)) {
        const int iy = oy0 - 1 + i;
        const bool ok = pin && iy >= 0 && iy < H && i < rows + 2;
        const unsigned o = (unsigned)(iy * W) * (unsigned)(XR_CIN * 2) + pxo;
        v0 = __builtin_amdgcn_raw_buffer_load_b128(xrs, ok ? o + (unsigned)hh * 16u : OOB, 0, 0);
        v1 = __builtin_amdgcn_raw_buffer_load_b128(xrs, (ok && !hh) ? o + 32u : OOB, 0, 0);
    };
    request(0, xc0, xc1);
    auto expand = [&](int i, unsigned (&E)[18]) __attribute__((always_inline)) {
        const int iy = oy0 - 1 + i;
        const bool ok = pin && iy >= 0 && iy < H;
        u32x4 n0, n1;
        request(i + 1, n0, n1);
        u32x4 b1 = xc1;
        b1[0] |= (ok && hh) ? 0x3c003c00u : 0u;              // the (1, 1) of the bias step for a pixel inside the image
        const half8 xb0 = __builtin_bit_cast(half8, xc0), xb1 = __builtin_bit_cast(half8, b1);
        floatx16 acc[3];
        half8 wlast[3];
#pragma unroll
        for (int ct = 0; ct < 3; ++ct) wlast[ct] = __builtin_bit_cast(half8, W1l[ct * 64 + lane]);
#pragma unroll
        for (int ct = 0; ct < 3; ++ct) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[ct][e] = 0.f;
            acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[ct], xb0, acc[ct], 0, 0, 0);
            acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wlast[ct], xb1, acc[ct], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            half8 e0, e1;
            if constexpr (ACT1 == DN_ACT_RELU) {
                // ReLU: round first, then v_pk_max_f16 against zero: the same bits as relu-then-round for every finite input (expdw_direct.hip)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    e0[e] = (half_t)acc[ct][e];
                    e1[e] = (half_t)acc[ct][8 + e];
                }
                e0 = __builtin_elementwise_max(e0, zero8);
                e1 = __builtin_elementwise_max(e1, zero8);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    e0[e] = (half_t)xr_act<ACT1>(acc[ct][e]);
                    e1[e] = (half_t)xr_act<ACT1>(acc[ct][8 + e]);
                }
            }
            const u32x4 p0 = __builtin_bit_cast(u32x4, e0), p1 = __builtin_bit_cast(u32x4, e1);
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                E[ct * 8 + d] = p0[d];
                E[ct * 8 + 4 + d] = p1[d];
            }
        }
        {
            half4 e2;
            if constexpr (ACT1 == DN_ACT_RELU) {
                const half4 z4 = {0, 0, 0, 0};
#pragma unroll
                for (int e = 0; e < 4; ++e) e2[e] = (half_t)acc[2][e];
                e2 = __builtin_elementwise_max(e2, z4);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) e2[e] = (half_t)xr_act<ACT1>(acc[2][e]);
            }
            const uint2v p2 = __builtin_bit_cast(uint2v, e2);
            E[16] = p2[0];
            E[17] = p2[1];
        }
        xc0 = n0;
        xc1 = n1;
    };
    const uint4* const wbase = reinterpret_cast<const uint4*>(Wl + hh * 16);
    const bool keep = r >= 1 && r <= XR_SW && px < W;        // not a halo lane, inside the image
    half_t* const obase = a.out + (size_t)img * H * W * NC + hh * 8;
    // output row o of the band from the expanded rows o (Ra), o + 1 (Rb), o + 2 (Rc)
    auto output = [&](int o, const unsigned (&Ra)[18], const unsigned (&Rb)[18], const unsigned (&Rc)[18]) __attribute__((always_inline)) {
        const int oy = oy0 + o;
        const unsigned po = (unsigned)(oy * W) * (unsigned)(XR_CIN * 2) + pxo;
        uint2v res[3] = {{0u, 0u}, {0u, 0u}, {0u, 0u}};
        if (a.has_res) {
#pragma unroll
            for (int g = 0; g < 3; ++g) res[g] = __builtin_amdgcn_raw_buffer_load_b64(xrs, pin ? po + (unsigned)(16 * g + 8 * hh) : OOB, 0, 0);
        }
        half8 xf[5];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            float d0[8], d1[8];
            {
                const float4* bp = reinterpret_cast<const float4*>(Bl + (ct * 2 + hh) * 16);
                const float4 c0 = bp[0], c1 = bp[1], c2 = bp[2], c3 = bp[3];
                d0[0] = c0.x; d0[1] = c0.y; d0[2] = c0.z; d0[3] = c0.w; d0[4] = c1.x; d0[5] = c1.y; d0[6] = c1.z; d0[7] = c1.w;
                d1[0] = c2.x; d1[1] = c2.y; d1[2] = c2.z; d1[3] = c2.w; d1[4] = c3.x; d1[5] = c3.y; d1[6] = c3.z; d1[7] = c3.w;
            }
            auto taps = [&](int ky, const unsigned (&R)[18]) __attribute__((always_inline)) {
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const uint4 w0 = wbase[((ct * 9 + ky * 3 + kx) * 4)], w1 = wbase[((ct * 9 + ky * 3 + kx) * 4) + 1];
                    unsigned v[8];
#pragma unroll
                    for (int d = 0; d < 8; ++d) v[d] = kx == 0 ? xr_from_left(R[ct * 8 + d]) : (kx == 2 ? xr_from_right(R[ct * 8 + d]) : R[ct * 8 + d]);
                    fma_mix_h8(d0, make_uint4(v[0], v[1], v[2], v[3]), w0);
                    fma_mix_h8(d1, make_uint4(v[4], v[5], v[6], v[7]), w1);
                }
            };
            taps(0, Ra);
            taps(1, Rb);
            taps(2, Rc);
            dn_act_n<float[8], 8>(d0, a.act2);
            dn_act_n<float[8], 8>(d1, a.act2);
            uint2v p[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                half4 hv;
#pragma unroll
                for (int e = 0; e < 4; ++e) hv[e] = (half_t)(g < 2 ? d0[4 * g + e] : d1[4 * (g - 2) + e]);
                p[g] = __builtin_bit_cast(uint2v, hv);
            }
            // lanes r / r + 32 hold the two halves of every 8-channel group of pixel r: after the swaps lane (r, hh) holds channels 8 hh .. + 7 of the
            // tile's first / second 16 channels -- the B fragments of K steps 2 ct and 2 ct + 1 (expdw_direct.hip)
            const uint2v s0 = __builtin_amdgcn_permlane32_swap(p[0][0], p[1][0], false, false);
            const uint2v s1 = __builtin_amdgcn_permlane32_swap(p[0][1], p[1][1], false, false);
            const uint2v s2 = __builtin_amdgcn_permlane32_swap(p[2][0], p[3][0], false, false);
            const uint2v s3 = __builtin_amdgcn_permlane32_swap(p[2][1], p[3][1], false, false);
            xf[2 * ct] = __builtin_bit_cast(half8, u32x4{s0[0], s1[0], s0[1], s1[1]});
            xf[2 * ct + 1] = __builtin_bit_cast(half8, u32x4{s2[0], s3[0], s2[1], s3[1]});
        }
        {   // channels 64 + 4 hh + e
            float d2[4];
            const float4 c = *reinterpret_cast<const float4*>(Bl2 + hh * 4);
            d2[0] = c.x; d2[1] = c.y; d2[2] = c.z; d2[3] = c.w;
            auto taps2 = [&](int ky, const unsigned (&R)[18]) __attribute__((always_inline)) {
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const uint2v w = Wl2[(ky * 3 + kx) * 2 + hh];
                    const unsigned v0 = kx == 0 ? xr_from_left(R[16]) : (kx == 2 ? xr_from_right(R[16]) : R[16]);
                    const unsigned v1 = kx == 0 ? xr_from_left(R[17]) : (kx == 2 ? xr_from_right(R[17]) : R[17]);
                    fma_mix_h4(d2, v0, v1, w);
                }
            };
            taps2(0, Ra);
            taps2(1, Rb);
            taps2(2, Rc);
            dn_act_n<float[4], 4>(d2, a.act2);
            half4 hv;
#pragma unroll
            for (int e = 0; e < 4; ++e) hv[e] = (half_t)d2[e];
            const uint2v p = __builtin_bit_cast(uint2v, hv);
            // K step 4: channels 64 .. 71 in the low half-wave, zeros in the high half-wave
            const uint2v s0 = __builtin_amdgcn_permlane32_swap(p[0], 0u, false, false);
            const uint2v s1 = __builtin_amdgcn_permlane32_swap(p[1], 0u, false, false);
            xf[4] = __builtin_bit_cast(half8, u32x4{s0[0], s1[0], s0[1], s1[1]});
        }
        // ---- the projection: lane = pixel r, registers 4 g .. 4 g + 3 = channels 8 g + 4 hh .. + 3
        floatx16 pacc;
#pragma unroll
        for (int e = 0; e < 16; ++e) pacc[e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 5; ++ks) pacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, W3l[ks * 64 + lane]), xf[ks], pacc, 0, 0, 0);
        uint2v pk[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 b = *reinterpret_cast<const float4*>(B3l + hh * 16 + 4 * g);
            float v[4] = {pacc[4 * g + 0] + b.x, pacc[4 * g + 1] + b.y, pacc[4 * g + 2] + b.z, pacc[4 * g + 3] + b.w};
            if (g < 3 && a.has_res) {        // residual (cout == cin): channels 8 g + 4 hh .. + 3 of the block's input at the same pixel
                const half4 rr = __builtin_bit_cast(half4, res[g]);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += (float)rr[e];
            }
            half4 hv;
#pragma unroll
            for (int e = 0; e < 4; ++e) hv[e] = (half_t)v[e];
            pk[g] = __builtin_bit_cast(uint2v, hv);
        }
        const uint2v s0 = __builtin_amdgcn_permlane32_swap(pk[0][0], pk[1][0], false, false);
        const uint2v s1 = __builtin_amdgcn_permlane32_swap(pk[0][1], pk[1][1], false, false);
        const uint2v s2 = __builtin_amdgcn_permlane32_swap(pk[2][0], pk[3][0], false, false);
        const uint2v s3 = __builtin_amdgcn_permlane32_swap(pk[2][1], pk[3][1], false, false);
        const uint4 lo4 = make_uint4(s0[0], s1[0], s0[1], s1[1]), hi4 = make_uint4(s2[0], s3[0], s2[1], s3[1]);
        half_t* orow = obase + ((size_t)oy * W + px) * NC;
        const int c0 = hh * 8;
        if (keep) {
            if (c0 < NC) *reinterpret_cast<uint4*>(orow) = lo4;
            if (c0 + 16 < NC) *reinterpret_cast<uint4*>(orow + 16) = hi4;
        }
    };
    unsigned E0[18], E1[18], E2[18];
    expand(0, E0);
    expand(1, E1);
    for (int o = 0; o < rows; o += 3) {
        expand(o + 2, E2);
        output(o, E0, E1, E2);
        if (o + 1 >= rows) break;
        expand(o + 3, E0);
        output(o + 1, E1, E2, E0);
        if (o + 2 >= rows) break;
        expand(o + 4, E1);
        output(o + 2, E2, E0, E1);
    }
}

template <int ACT1>
int xr_launch(const ExpDwArgs& a, int bh, hipStream_t s) {
    const int strips = dn_cdiv(a.W, XR_SW), bands = dn_cdiv(a.Ho, bh);
    const int per_image = dn_cdiv((long)strips * bands, XR_NW);
    hipLaunchKernelGGL((expdw_rows_kernel<ACT1>), dim3((unsigned)(xcd_image_slots(a.xq, a.n) * per_image)), dim3(XR_NT), 0, s, a, per_image, strips,
                       bands, bh);
    return DN_OK;
}

}  // namespace

// Output rows per band, 0 = the shape is not this body's. DN_EXPDW_ROWS_BAND: rows per band (measured alone on the chip: LAB_NOTEBOOK).
int expdw_rows_band(const ExpDwArgs& a) {
    const bool act_ok = a.act1 >= DN_ACT_NONE && a.act1 <= DN_ACT_HSWISH && a.act2 >= DN_ACT_NONE && a.act2 <= DN_ACT_HSWISH;
    if (!(a.k == 3 && a.stride == 1 && a.pad == 1 && a.w1 && a.w3 && a.cin == XR_CIN && a.cexp == XR_CEXP && a.cout % 8 == 0 && a.cout >= 8 &&
          a.cout <= 32 && (!a.has_res || a.cout == a.cin) && !a.pool && act_ok && a.Ho == a.H && a.Wo == a.W))
        return 0;
    if ((long)a.H * a.W * (XR_CIN * 2) >= (1L << 31)) return 0;                                 // buffer range
    int bh = dn_knob("DN_EXPDW_ROWS_BAND", 5);
    if (bh < 1) bh = 1;
    if (bh > a.Ho) bh = a.Ho;
    if ((long)xcd_image_slots(a.xq, a.n) * dn_cdiv((long)dn_cdiv(a.W, XR_SW) * dn_cdiv(a.Ho, bh), XR_NW) >= (1L << 31)) return 0;      // grid
    return bh;
}

int launch_expdw_rows(const ExpDwArgs& a, int bh, hipStream_t s) {
    switch (a.act1) {
        case DN_ACT_RELU: return xr_launch<DN_ACT_RELU>(a, bh, s);
        case DN_ACT_RELU6: return xr_launch<DN_ACT_RELU6>(a, bh, s);
        case DN_ACT_HSWISH: return xr_launch<DN_ACT_HSWISH>(a, bh, s);
        default: return xr_launch<DN_ACT_NONE>(a, bh, s);
    }
}
