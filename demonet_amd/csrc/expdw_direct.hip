// Fused expand + depthwise 3x3 stride 2 + project for the one-chunk block 16 -> 64 -> cout (the 160 x 160 -> 80 x 80 block of MobileNetV3):
// the expanded value of EACH TAP comes out of the matrix cores in the accumulator position of the output pixel that needs it and goes straight
// into the depthwise sum. A second body for the launch that expdw.hip serves (expdw_choose selects it, choice.h: DN_EXPDW_DIRECT, default 1); same
// reference ops (mobilenetv3.py:72-95, BN folded).
//
// Why: at stride 2 an expanded value is used by 2.25 output pixels on average, and the expand is ONE 16-deep matrix step plus the bias step.
// expdw_one_kernel pays for sharing those 2.25 uses with an E tile in LDS (every value rounded, written, read back: 18 ds_read_b128 for 72
// multiply-adds per thread, nine of them weights), four barrier-separated phases per 8 x 8 tile, an expand that runs 20 units on 8 waves and a
// projection that two of the eight waves run. Here nothing of the block exists in LDS but its input:
//   * a workgroup owns a BAND of whole output rows of one image (XCD grouping: xcd_image_of); the 2 bh + 1 input rows it needs enter LDS once
//     as 32-byte pixels through a per-image raw buffer (rows above / below the image read as zeros), ONE barrier, none after it;
//   * a wave walks the band's 32-pixel output tiles in flattened (y, x) order and carries both 32-channel tiles of the expansion, one after
//     the other. Per tap: one ds_read_b128 at a per-lane address (a tap outside the image reads a zero slot) is the B fragment, A = the w1
//     fragment, then the (hi, lo) bias fragment against a per-lane ones / zero constant picked by the tap's inside flag -- the two matrix steps
//     of expdw_kernel, so a pixel outside the image expands to act(0) = 0. The 16 results per lane are activated and rounded as Es was written
//     and enter the depthwise accumulators (bias first, taps in (ky, kx) order, v_fma_mix_f32); the depthwise weights / biases of the lane's 16
//     channels are LDS broadcasts (two addresses per wave), laid out once per band;
//   * act2, one rounding, v_permlane32_swap: the lane's 4-channel groups become the projection's B fragments -- K step 2 ct + s holds the 16
//     channels Ds held, in its order -- four matrix steps, + b3 in fp32, one rounding, the permlane store epilogue of pw_direct_kernel.
// Swizzle: a tap puts lane r on chunk 4 r + const (16-byte chunks, pixels 64 bytes apart), 16 chunks span the 64 banks: byte address A is
// kept at A ^ (((A >> 8) & 3) << 4), which spreads the four lanes of a 16-lane group that share (4 r) mod 16 over the four chunks of a pixel pair.
// Same operands, same K order, same rounding points as expdw_kernel / expdw_one_kernel: outputs are bit-identical (tests/test_gpu_expdw_direct.py).
#include <algorithm>

#include "common.h"

namespace {

constexpr int XD_NW = 8;                // waves per workgroup (DN_EXPDW_DIRECT_WAVES, 2 .. 8): 128 registers, two workgroups per compute unit
constexpr int XD_NT_MAX = 512;
constexpr int XD_LDS_MAX = 64 * 1024;
constexpr int XD_CONST_BYTES = 64 + 2 * 9 * 2 * 32 + 2 * 2 * 64 + 2 * 64 + 4 * 64 * 16;    // zero / ones slots, depthwise weights, depthwise bias, project bias, project fragments
static inline size_t xd_lds_bytes(int bh, int W) { return (((size_t)(2 * bh + 1) * W * 32 + 63) & ~(size_t)63) + XD_CONST_BYTES; }

typedef unsigned uint2v __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <int ACT>
__device__ __forceinline__ float xd_act(float v) {
    if constexpr (ACT == DN_ACT_RELU) return dn_relu(v);
    else if constexpr (ACT == DN_ACT_RELU6) return dn_relu6(v);
    else if constexpr (ACT == DN_ACT_HSWISH) return v * dn_relu6(v + 3.f) * (1.f / 6.f);
    else return v;
}

// ACT1 is a template parameter: the activation follows a matrix instruction, and straight-line code gets its wait states from hipcc's hazard
// recognizer (a uniform switch there needs explicit ones on every path: pwdirect.hip act16).
template <int ACT1>
__global__ __launch_bounds__(XD_NT_MAX) __attribute__((amdgpu_waves_per_eu(4, 4))) void expdw_direct_kernel(ExpDwArgs a, int bands, int bh, FastDiv fd_wo) {
    extern __shared__ __attribute__((aligned(16))) unsigned char xdl[];
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NT = (int)blockDim.x, NW = NT >> 6;
    int img, bi;
    if (!xcd_image_of(blockIdx.x, bands, a.xq, a.n, img, bi)) return;      // workgroup-uniform
    const int W = a.W, H = a.H, Wo = a.Wo, NC = a.cout;
    const int oy0 = bi * bh, rows = min(bh, a.Ho - oy0);
    const int blen = rows * Wo;                              // output pixels of the band
    const int iy0 = oy0 * 2 - 1;                             // image row of staged row 0 (pad 1)
    const unsigned rowb = (unsigned)W * 32u;
    const unsigned zoff = ((unsigned)(2 * rows + 1) * rowb + 63u) & ~63u;     // the zero slot (behind whole 64-byte swizzle units: W may be odd)
    half_t* Wl = reinterpret_cast<half_t*>(xdl + zoff + 64);       // [channel tile][tap][hh][16]: the lane's channels 8 g + 4 hh + e at 4 g + e
    float* Bl = reinterpret_cast<float*>(Wl + 2 * 9 * 2 * 16);     // [channel tile][hh][16]
    float* B3l = Bl + 2 * 2 * 16;                                  // [hh][16]
    u32x4* W3l = reinterpret_cast<u32x4*>(B3l + 2 * 16);           // [K step][lane]: the projection's A fragments (read per tile: 16 registers less)
    // ---- staging: every 16-byte chunk of the 2 rows + 1 input rows
    {
        const __amdgpu_buffer_rsrc_t xrs =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(a.x + (size_t)img * H * W * 16), 0, H * (int)rowb, 0x00020000);
        const int chunks = (2 * rows + 1) * W * 2;
        const unsigned g0 = (unsigned)(iy0 * (int)rowb);          // "negative" (the pad row above the image) = far out of range = zeros
        for (int c0 = tid; c0 < chunks; c0 += 5 * NT) {
            u32x4 v[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int c = c0 + i * NT;
                v[i] = __builtin_amdgcn_raw_buffer_load_b128(xrs, c < chunks ? g0 + (unsigned)c * 16u : 0x80000000u, 0, 0);
            }
            asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]));      // (pinned: all five requests before the first store)
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const unsigned A = (unsigned)(c0 + i * NT) * 16u;
                if (c0 + i * NT < chunks) *reinterpret_cast<u32x4*>(xdl + (A ^ (((A >> 8) & 3u) << 4))) = v[i];
            }
        }
        if (tid < 4) *reinterpret_cast<u32x4*>(xdl + zoff + tid * 16) = u32x4{tid == 2 ? 0x3c003c00u : 0u, 0u, 0u, 0u};     // zeros; at + 32 the (1, 1) of the bias step
        for (int i = tid; i < 2 * 9 * 2 * 16; i += NT) {
            const int j = i & 15, h2 = (i >> 4) & 1, q = i >> 5, ct = q / 9, tp = q - ct * 9;
            Wl[i] = a.wd[tp * 64 + ct * 32 + 8 * (j >> 2) + 4 * h2 + (j & 3)];
        }
        if (tid < 64) Bl[tid] = a.bd[(tid >> 5) * 32 + 8 * ((tid & 15) >> 2) + 4 * ((tid >> 4) & 1) + (tid & 3)];
        if (tid >= 64 && tid < 96) {
            const int i = tid - 64;
            B3l[i] = a.b3[min(8 * ((i & 15) >> 2) + 4 * (i >> 4) + (i & 3), NC - 1)];
        }
    }
    // ---- once per band: the expand's and the projection's A fragments
    const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    half8 wf[2], wlast[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        wf[ct] = *reinterpret_cast<const half8*>(a.w1 + (size_t)(ct * 32 + r) * 16 + hh * 8);
        const float b = a.b1[ct * 32 + r];
        const half_t hi = (half_t)b;
        const half8 bw = {hi, (half_t)(b - (float)hi), 0, 0, 0, 0, 0, 0};
        wlast[ct] = hh ? zero8 : bw;                         // (columns 16 .. 23 of the last step: the bias pair; 24 .. 31: zeros)
    }
    if (tid < 64) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const u32x4 w = *reinterpret_cast<const u32x4*>(a.w3 + (size_t)min(r, NC - 1) * 64 + ks * 16 + hh * 8);
            W3l[ks * 64 + lane] = r < NC ? w : u32x4{0u, 0u, 0u, 0u};
        }
    }
    __syncthreads();
    half_t* const obase = a.out + ((size_t)img * a.Ho + oy0) * Wo * NC + hh * 8;
    const int ntiles = (blen + 31) >> 5;
    for (int t = wave; t < ntiles; t += NW) {
        const int pl = t * 32 + r, plc = min(pl, blen - 1);               // this lane's pixel of the band (a ragged last tile: clamped, not stored)
        const int oyl = (int)fd_div((unsigned)plc, fd_wo), ox = plc - oyl * Wo;
        // tap (ky, kx): staged row 2 oyl + ky, column 2 ox - 1 + kx. Outside the image: the zero slot, and zeros against the bias pair
        unsigned ad[9], ins = 0;
        {
            const int A0 = ((2 * oyl) * W + 2 * ox - 1) * 32 + hh * 16;
            const int gy = iy0 + 2 * oyl, gx = 2 * ox - 1;
#pragma unroll
            for (int tp = 0; tp < 9; ++tp) {
                const int ky = tp / 3, kx = tp % 3;
                const bool ok = gy + ky >= 0 && gy + ky < H && gx + kx >= 0 && gx + kx < W;
                const unsigned A = (unsigned)(A0 + (ky * W + kx) * 32);
                ad[tp] = ok ? (A ^ (((A >> 8) & 3u) << 4)) : zoff;
                ins |= ok ? (1u << tp) : 0u;
            }
        }
        // Software pipeline over the 18 (channel tile, tap) steps: the matrix steps of step u + 1, the B fragment of step u + 2 and the depthwise weights of
        // step u + 1 are issued in FRONT of the vector work of step u (fences: left alone, hipcc puts every matrix step right in front of its first use,
        // on one accumulator, and the wave then waits for each LDS read and each matrix result in turn).
        half8 xf[4];
        const unsigned ooff = zoff + (hh ? 0u : 32u);          // the ones / zero step: (1, 1, 0 ..) for a tap inside the image (hh = 0; zeros for hh = 1, as X's columns 24 .. 31 were)
        auto mfma2 = [&](int u, const half8& xb) {
            const int ct = u / 9, tp = u - ct * 9;
            const half8 xo = *reinterpret_cast<const half8*>(xdl + ((ins >> tp) & 1u ? ooff : zoff));
            floatx16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[ct], xb, acc, 0, 0, 0);
            return __builtin_amdgcn_mfma_f32_32x32x16_f16(wlast[ct], xo, acc, 0, 0, 0);
        };
        const uint4* const wbase = reinterpret_cast<const uint4*>(Wl + hh * 16);
        half8 xb = *reinterpret_cast<const half8*>(xdl + ad[0]);
        uint4 w0n = wbase[0], w1n = wbase[1];
        floatx16 accn = mfma2(0, xb);
        xb = *reinterpret_cast<const half8*>(xdl + ad[1]);
        float dacc[2][8];
#pragma unroll
        for (int u = 0; u < 18; ++u) {
            const int ct = u / 9, tp = u - ct * 9;
            const floatx16 acc = accn;
            const uint4 w0 = w0n, w1 = w1n;
            float4 c0, c1, c2, c3;
            if (tp == 0) {
                const float4* bp = reinterpret_cast<const float4*>(Bl + (ct * 2 + hh) * 16);
                c0 = bp[0]; c1 = bp[1]; c2 = bp[2]; c3 = bp[3];
            }
            if (u + 1 < 18) {
                accn = mfma2(u + 1, xb);
                if (u + 2 < 18) xb = *reinterpret_cast<const half8*>(xdl + ad[(u + 2) % 9]);
                w0n = wbase[(u + 1) * 4]; w1n = wbase[(u + 1) * 4 + 1];
            }
            __builtin_amdgcn_sched_barrier(0);
            if (tp == 0) {
                dacc[0][0] = c0.x; dacc[0][1] = c0.y; dacc[0][2] = c0.z; dacc[0][3] = c0.w; dacc[0][4] = c1.x; dacc[0][5] = c1.y; dacc[0][6] = c1.z; dacc[0][7] = c1.w;
                dacc[1][0] = c2.x; dacc[1][1] = c2.y; dacc[1][2] = c2.z; dacc[1][3] = c2.w; dacc[1][4] = c3.x; dacc[1][5] = c3.y; dacc[1][6] = c3.z; dacc[1][7] = c3.w;
            }
            half8 e0, e1;
            if constexpr (ACT1 == DN_ACT_RELU) {
                // ReLU: round first, then v_pk_max_f16 against zero -- 8 + 8 instructions instead of 16 + 8. The same bits as relu-then-round for every finite
                // input (rounding is monotonic and keeps the sign; max(-0, +0) = +0); the other activations keep the fp32 form.
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    e0[e] = (half_t)acc[e];
                    e1[e] = (half_t)acc[8 + e];
                }
                const half8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
                e0 = __builtin_elementwise_max(e0, z8);
                e1 = __builtin_elementwise_max(e1, z8);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    e0[e] = (half_t)xd_act<ACT1>(acc[e]);
                    e1[e] = (half_t)xd_act<ACT1>(acc[8 + e]);
                }
            }
            fma_mix_h8(dacc[0], __builtin_bit_cast(uint4, e0), w0);
            fma_mix_h8(dacc[1], __builtin_bit_cast(uint4, e1), w1);
            __builtin_amdgcn_sched_barrier(0);
            if (tp == 8) {
                dn_act_n<float[8], 8>(dacc[0], a.act2);
                dn_act_n<float[8], 8>(dacc[1], a.act2);
                uint2v p[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    half4 hv;
#pragma unroll
                    for (int e = 0; e < 4; ++e) hv[e] = (half_t)dacc[g >> 1][4 * (g & 1) + e];
                    p[g] = __builtin_bit_cast(uint2v, hv);
                }
                // lanes r / r + 32 hold the two halves of every 8-channel group of pixel r: after the swaps lane (r, hh) holds channels 8 hh .. + 7 of the
                // tile's first / second 16 channels -- the B fragments of K steps 2 ct and 2 ct + 1
                const uint2v s0 = __builtin_amdgcn_permlane32_swap(p[0][0], p[1][0], false, false);
                const uint2v s1 = __builtin_amdgcn_permlane32_swap(p[0][1], p[1][1], false, false);
                const uint2v s2 = __builtin_amdgcn_permlane32_swap(p[2][0], p[3][0], false, false);
                const uint2v s3 = __builtin_amdgcn_permlane32_swap(p[2][1], p[3][1], false, false);
                xf[2 * ct] = __builtin_bit_cast(half8, u32x4{s0[0], s1[0], s0[1], s1[1]});
                xf[2 * ct + 1] = __builtin_bit_cast(half8, u32x4{s2[0], s3[0], s2[1], s3[1]});
            }
        }
        // ---- the projection: lane = pixel r, registers 4 g .. 4 g + 3 = channels 8 g + 4 hh .. + 3
        floatx16 pacc;
#pragma unroll
        for (int e = 0; e < 16; ++e) pacc[e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) pacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, W3l[ks * 64 + lane]), xf[ks], pacc, 0, 0, 0);
        uint2v pk[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 b = *reinterpret_cast<const float4*>(B3l + hh * 16 + 4 * g);
            half4 hv;
            hv[0] = (half_t)(pacc[4 * g + 0] + b.x); hv[1] = (half_t)(pacc[4 * g + 1] + b.y);
            hv[2] = (half_t)(pacc[4 * g + 2] + b.z); hv[3] = (half_t)(pacc[4 * g + 3] + b.w);
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

template <int ACT1>
int xd_launch(const ExpDwArgs& a, int bands, int bh, size_t lds, hipStream_t s) {
    const int nw = std::min(std::max(dn_knob("DN_EXPDW_DIRECT_WAVES", XD_NW), 2), XD_NT_MAX / 64);
    hipLaunchKernelGGL((expdw_direct_kernel<ACT1>), dim3((unsigned)(xcd_image_slots(a.xq, a.n) * bands)), dim3(nw * 64), lds, s, a, bands, bh,
                       fastdiv((unsigned)a.Wo));
    return DN_OK;
}

}  // namespace

// Output rows per band, 0 = the shape is not this body's. DN_EXPDW_DIRECT_BAND: 4 by default (2 and 4 measured alone on the chip: LAB_NOTEBOOK),
// halved until the band's input rows fit LDS.
int expdw_direct_band(const ExpDwArgs& a) {
    const bool act_ok = a.act1 >= DN_ACT_NONE && a.act1 <= DN_ACT_HSWISH && a.act2 >= DN_ACT_NONE && a.act2 <= DN_ACT_HSWISH;
    if (!(a.k == 3 && a.stride == 2 && a.pad == 1 && a.w1 && a.w3 && a.cin == 16 && a.cexp == 64 && a.cout % 8 == 0 && a.cout >= 8 && a.cout <= 32 &&
          !a.has_res && !a.pool && act_ok))
        return 0;
    if ((long)a.H * a.W * 32 >= (1L << 31) || (long)xcd_image_slots(a.xq, a.n) * a.Ho >= (1L << 31)) return 0;      // buffer range, grid
    int bh = dn_knob("DN_EXPDW_DIRECT_BAND", 4);
    if (bh < 1) bh = 1;
    if (bh > a.Ho) bh = a.Ho;
    while (bh > 1 && xd_lds_bytes(bh, a.W) > (size_t)XD_LDS_MAX) bh >>= 1;
    if (xd_lds_bytes(bh, a.W) > (size_t)XD_LDS_MAX) return 0;
    if (!fd_ok((unsigned long long)bh * a.Wo, (unsigned)a.Wo)) return 0;
    return bh;
}

int launch_expdw_direct(const ExpDwArgs& a, int bh, hipStream_t s) {
    const int bands = dn_cdiv(a.Ho, bh);
    const size_t lds = xd_lds_bytes(bh, a.W);
    switch (a.act1) {
        case DN_ACT_RELU: return xd_launch<DN_ACT_RELU>(a, bands, bh, lds, s);
        case DN_ACT_RELU6: return xd_launch<DN_ACT_RELU6>(a, bands, bh, lds, s);
        case DN_ACT_HSWISH: return xd_launch<DN_ACT_HSWISH>(a, bands, bh, lds, s);
        default: return xd_launch<DN_ACT_NONE>(a, bands, bh, lds, s);
    }
}
