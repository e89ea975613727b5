// Camera-motion compensation for the trackers: dn_motion_estimate measures, per stream and frame step, the global motion of the image
// (translation + isotropic scale, previous frame -> current frame) from the luma of the surfaces a dn_frame table names, and dn_track_compensate
// applies it to a tracker's state block in front of that frame's dn_track_update. The semantics, sentence by sentence, are in
// include/demonet_hip.h and restated in tests/motion_ref.py; this file must agree with them bit for bit.
//   motion_thumb_kernel   box-filters every frame's luma to a thumbnail (the bandwidth-bound part: every luma byte is read once, by 16-byte
//                         loads where the surface's alignment allows, 4-byte loads otherwise, bytes for packed RGB). Each stream keeps two
//                         thumbnails; a parity word in the state says which one is the previous frame's, so the step's arguments never change
//                         and a captured graph replays.
//   motion_match_kernel   one wave per block of the current thumbnail: the search window of the previous thumbnail sits in LDS as dwords, the
//                         block in registers, and one v_qsad_pk_u16_u8 scores four neighbouring dx candidates against four block pixels; a lane
//                         walks (dy, group of four dx) items. The winner is the minimum of one packed 64-bit key (SAD, dx^2 + dy^2, dy, dx), so
//                         the reduction does not depend on its order.
//   motion_fit_kernel     one workgroup per stream: medians from 33-bin histograms, exact int64 sums through integer LDS atomics, the float64
//                         closed form, the outputs, and the parity flip.
//   track_compensate_kernel   a thread per track slot: read-modify-write of the 15 filter floats the transform touches.
// Compiled with -ffp-contract=off: every operation of the header's text rounds once. No inline asm, no float atomics.
#include "trackcore.h"

namespace {

constexpr int MO_NT = 256;
constexpr int MO_HDR = 16;                 // bytes of the per-stream header: int32 parity, have, height, width
constexpr int MO_MAX_SIDE = 512;           // thumbnail capacity per side
constexpr int MO_MAX_R = 16;
constexpr int MO_MAX_K = 4096;             // box side: k * k * 255 stays below 2^32
constexpr int MO_MAX_D = 512;              // masking rows per stream
constexpr int MO_MAX_STREAMS = 65535;      // grid.y

struct MoArgs {
    int TH, TW, TWp;                       // capacity, and the thumbnails' row pitch (TW rounded up to 16)
    int blk, r, min_texture, min_blocks, max_blocks;
    float mask_thresh;
    int d;
    size_t stride;                         // bytes per stream
};

struct MoGeom { int k, th, tw, nbx, nby; };

__device__ __forceinline__ MoGeom mo_geom(const int W, const int H, const MoArgs& a) {
    MoGeom g;
    const int kw = W / (a.TW + 1), kh = H / (a.TH + 1);
    g.k = (kw > kh ? kw : kh) + 1;         // the smallest k >= 1 with floor(W / k) <= TW and floor(H / k) <= TH
    const bool ok = W >= 1 && H >= 1 && g.k <= MO_MAX_K;
    g.th = ok ? H / g.k : 0;
    g.tw = ok ? W / g.k : 0;
    const int need = a.blk + 2 * a.r;
    const bool fits = g.tw >= need && g.th >= need;
    g.nbx = fits ? (g.tw - 2 * a.r) / a.blk : 0;
    g.nby = fits ? (g.th - 2 * a.r) / a.blk : 0;
    return g;
}

inline size_t mo_up16(size_t v) { return (v + 15) & ~(size_t)15; }
inline int mo_max_blocks(const dn_motion_params& p) { return ((p.max_w - 2 * p.radius) / p.block) * ((p.max_h - 2 * p.radius) / p.block); }
inline size_t mo_stride(const dn_motion_params& p) {
    return MO_HDR + (size_t)16 * mo_max_blocks(p) + 2 * (size_t)p.max_h * mo_up16(p.max_w);
}

__device__ __forceinline__ unsigned char* mo_thumb(unsigned char* sb, const MoArgs& a, const int which) {
    return sb + MO_HDR + (size_t)16 * a.max_blocks + (size_t)which * a.TH * a.TWp;
}

// the 8-bit luma of frame pixel (x, y)
template <int FMT>
__device__ __forceinline__ unsigned mo_luma(const dn_frame& f, const int x, const int y) {
    if (FMT == DN_FRAME_RGB24 || FMT == DN_FRAME_BGR24) {
        const uint8_t* p = f.plane[0] + (size_t)y * f.pitch[0] + (size_t)x * 3;
        const unsigned r = p[FMT == DN_FRAME_RGB24 ? 0 : 2], g = p[1], b = p[FMT == DN_FRAME_RGB24 ? 2 : 0];
        return (77u * r + 150u * g + 29u * b + 128u) >> 8;
    }
    return f.plane[0][(size_t)y * f.pitch[0] + x];
}

// A thread owns four neighbouring thumbnail pixels of one row: 4 k source bytes per source row, k rows.
template <int FMT>
__global__ __launch_bounds__(MO_NT) void motion_thumb_kernel(const dn_frame* __restrict__ frames, unsigned char* __restrict__ state, const MoArgs a) {
    const int b = blockIdx.y;
    const dn_frame f = frames[b];
    const MoGeom g = mo_geom(f.width, f.height, a);
    unsigned char* const sb = state + (size_t)b * a.stride;
    const int parity = reinterpret_cast<const int*>(sb)[0] & 1;
    unsigned char* const dst = mo_thumb(sb, a, parity ^ 1);
    const int ngx = (g.tw + 3) >> 2;
    const int t = blockIdx.x * MO_NT + threadIdx.x;
    if (t >= ngx * g.th) return;
    const int ty = t / ngx, gx = t - ty * ngx;
    const int k = g.k;
    unsigned s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    const bool yuv = FMT == DN_FRAME_NV12 || FMT == DN_FRAME_I420;
    const bool full = 4 * gx + 4 <= g.tw;
    const size_t base_bits = reinterpret_cast<size_t>(f.plane[0]) | (size_t)f.pitch[0];
    if (yuv && full && (k & 3) == 0 && (base_bits & 3) == 0) {
        // every dword of the span belongs to one pixel: kq dwords per pixel and row
        const int kq = k >> 2;
        const uint8_t* row = f.plane[0] + (size_t)(ty * k) * f.pitch[0] + (size_t)(4 * gx) * k;
        const bool wide = (base_bits & 15) == 0;       // (the span starts at a multiple of 4 k = 16 kq bytes)
        for (int r = 0; r < k; ++r, row += f.pitch[0]) {
            int p = 0, c = 0;
            auto add = [&](const unsigned q) {
                const unsigned v = __builtin_amdgcn_sad_u8(q, 0u, 0u);
                s0 += p == 0 ? v : 0u; s1 += p == 1 ? v : 0u; s2 += p == 2 ? v : 0u; s3 += p == 3 ? v : 0u;
                if (++c == kq) { c = 0; ++p; }
            };
            if (wide) {
                const uint4* q4 = reinterpret_cast<const uint4*>(row);
                for (int j = 0; j < kq; ++j) {
                    const uint4 q = q4[j];
                    add(q.x); add(q.y); add(q.z); add(q.w);
                }
            } else {
                const unsigned* q1 = reinterpret_cast<const unsigned*>(row);
                for (int j = 0; j < k; ++j) add(q1[j]);
            }
        }
    } else if (yuv && full && (base_bits & 3) == 0) {
        // 4-byte loads, the bytes dealt to their pixels one by one
        const uint8_t* row = f.plane[0] + (size_t)(ty * k) * f.pitch[0] + (size_t)(4 * gx) * k;
        for (int r = 0; r < k; ++r, row += f.pitch[0]) {
            const unsigned* q1 = reinterpret_cast<const unsigned*>(row);
            int p = 0, c = 0;
            for (int j = 0; j < k; ++j) {
                const unsigned q = q1[j];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned v = (q >> (8 * e)) & 255u;
                    s0 += p == 0 ? v : 0u; s1 += p == 1 ? v : 0u; s2 += p == 2 ? v : 0u; s3 += p == 3 ? v : 0u;
                    if (++c == k) { c = 0; ++p; }
                }
            }
        }
    } else {
        // packed RGB, surfaces that are not 4-byte aligned, and the last group of a row whose width is no multiple of 4
        unsigned s[4] = {0, 0, 0, 0};
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (4 * gx + p >= g.tw) continue;
            const int x0 = (4 * gx + p) * k, y0 = ty * k;
            for (int r = 0; r < k; ++r)
                for (int c = 0; c < k; ++c) s[p] += mo_luma<FMT>(f, x0 + c, y0 + r);
        }
        s0 = s[0]; s1 = s[1]; s2 = s[2]; s3 = s[3];
    }
    const unsigned kk = (unsigned)k * (unsigned)k, half = kk >> 1;
    const unsigned m0 = (s0 + half) / kk, m1 = (s1 + half) / kk, m2 = (s2 + half) / kk, m3 = (s3 + half) / kk;
    // (pixels at or beyond tw in the last group are 0: their sums are)
    const unsigned out = (4 * gx + 0 < g.tw ? m0 : 0u) | (4 * gx + 1 < g.tw ? m1 << 8 : 0u) | (4 * gx + 2 < g.tw ? m2 << 16 : 0u) |
                         (4 * gx + 3 < g.tw ? m3 << 24 : 0u);
    *reinterpret_cast<unsigned*>(dst + (size_t)ty * a.TWp + 4 * gx) = out;
}

__device__ __forceinline__ unsigned mo_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ unsigned long long mo_wave_min(unsigned long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, o), hi = __shfl_xor((unsigned)(v >> 32), o);
        const unsigned long long w = ((unsigned long long)hi << 32) | lo;
        v = w < v ? w : v;
    }
    return v;
}

// One wave per block of the current thumbnail.
template <int BLK>
__global__ __launch_bounds__(64) void motion_match_kernel(const dn_frame* __restrict__ frames, const float4* __restrict__ boxes,
                                                          const float* __restrict__ scores, const int32_t* __restrict__ counts,
                                                          unsigned char* __restrict__ state, const MoArgs a) {
    constexpr int ND = BLK * BLK / 4;                  // dwords of a block
    constexpr int BQ = BLK / 4;                        // dwords of a block row
    constexpr int PW = (2 * MO_MAX_R + 1 + 3) / 4 + BQ;        // window row pitch in dwords: the groups of four dx, and the block's width beyond the last
    constexpr int WR = BLK + 2 * MO_MAX_R;             // window rows at most
    __shared__ unsigned win[WR * PW];
    __shared__ unsigned curb[ND];
    const int b = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x;
    unsigned char* const sb = state + (size_t)b * a.stride;
    const int* const hdr = reinterpret_cast<const int*>(sb);
    int4* const vec = reinterpret_cast<int4*>(sb + MO_HDR) + blk;
    const int W = frames[b].width, H = frames[b].height;
    const MoGeom g = mo_geom(W, H, a);
    const bool seeded = hdr[1] != 0 && hdr[2] == H && hdr[3] == W;
    if (blk >= g.nbx * g.nby || !seeded) {              // (wave-uniform)
        if (lane == 0) *vec = make_int4(0, 0, 0, 0);
        return;
    }
    const int parity = hdr[0] & 1;
    const unsigned char* const prev = mo_thumb(sb, a, parity);
    const unsigned char* const cur = mo_thumb(sb, a, parity ^ 1);
    const int r = a.r;
    const int bj = blk / g.nbx, bi = blk - bj * g.nbx;
    const int wx = bi * BLK, wy = bj * BLK;             // the window's corner; the block's is (wx + r, wy + r)
    const int ww = BLK + 2 * r;                         // window side in pixels
    const int G = (2 * r + 1 + 3) >> 2;                 // groups of four dx
    const int cols = G + BQ;                            // dword columns an item can read
    // the window: 4-byte loads (wx is a multiple of 8, the pitch of 16), bytes at or beyond ww zeroed
    for (int i = lane; i < ww * cols; i += 64) {
        const int row = i / cols, col = i - row * cols;
        const int nv = ww - 4 * col;
        unsigned v = 0;
        if (nv > 0) {
            v = *reinterpret_cast<const unsigned*>(prev + (size_t)(wy + row) * a.TWp + wx + 4 * col);
            if (nv < 4) v &= (1u << (8 * nv)) - 1u;
        }
        win[row * PW + col] = v;
    }
    // the block: byte loads (its corner is aligned only when r is), one dword per lane
    unsigned mine = 0;
    if (lane < ND) {
        const unsigned char* p = cur + (size_t)(wy + r + lane / BQ) * a.TWp + wx + r + 4 * (lane % BQ);
        mine = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
        curb[lane] = mine;
    }
    // texture: sum |p - m| with m the rounded mean
    const unsigned total = mo_wave_sum(lane < ND ? __builtin_amdgcn_sad_u8(mine, 0u, 0u) : 0u);
    const unsigned m = (total + BLK * BLK / 2) / (BLK * BLK);
    const unsigned tex = mo_wave_sum(lane < ND ? __builtin_amdgcn_sad_u8(mine, m * 0x01010101u, 0u) : 0u);
    // masking: is the block's centre inside a detection box of this stream
    bool masked = false;
    if (boxes) {
        const float cx = (float)(g.k * (wx + r + BLK / 2)) - 0.5f, cy = (float)(g.k * (wy + r + BLK / 2)) - 0.5f;
        const int c = counts[b];
        const int n = c < 0 ? 0 : (c > a.d ? a.d : c);
        bool hit = false;
        for (int j = lane; j < n; j += 64) {
            const float sc = scores[(size_t)b * a.d + j];
            const float4 q = boxes[(size_t)b * a.d + j];
            const bool fin = isfinite(q.x) && isfinite(q.y) && isfinite(q.z) && isfinite(q.w);
            hit = hit || (sc >= a.mask_thresh && fin && q.x <= cx && cx < q.z && q.y <= cy && cy < q.w);      // (a NaN score compares false)
        }
        masked = __any(hit);
    }
    __syncthreads();
    unsigned ref[ND];
#pragma unroll
    for (int i = 0; i < ND; ++i) ref[i] = curb[i];
    unsigned long long best = ~0ull;
    const int items = (2 * r + 1) * G;
    for (int it = lane; it < items; it += 64) {
        const int iy = it / G, gq = it - iy * G;
        unsigned long long acc = 0;
        const unsigned* wr = win + iy * PW + gq;
#pragma unroll
        for (int j = 0; j < BLK; ++j, wr += PW) {
            unsigned lo = wr[0];
#pragma unroll
            for (int c = 0; c < BQ; ++c) {
                const unsigned hi = wr[c + 1];
                acc = __builtin_amdgcn_qsad_pk_u16_u8(((unsigned long long)hi << 32) | lo, ref[j * BQ + c], acc);
                lo = hi;
            }
        }
        const int dy = iy - r;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int dxi = 4 * gq + q;
            if (dxi > 2 * r) continue;
            const int dx = dxi - r;
            const unsigned long long sad = (acc >> (16 * q)) & 0xffffull;
            const unsigned long long key = (sad << 22) | ((unsigned long long)(dx * dx + dy * dy) << 12) | ((unsigned long long)iy << 6) | (unsigned)dxi;
            best = key < best ? key : best;
        }
    }
    best = mo_wave_min(best);
    if (lane == 0) {
        const int dx = (int)(best & 63) - r, dy = (int)((best >> 6) & 63) - r;
        *vec = make_int4(dx, dy, (int)(best >> 22), (tex >= (unsigned)a.min_texture && !masked) ? 1 : 0);
    }
}

// One workgroup per stream.
__global__ __launch_bounds__(MO_NT) void motion_fit_kernel(const dn_frame* __restrict__ frames, unsigned char* __restrict__ state, const MoArgs a,
                                                           float4* __restrict__ motion_out, int4* __restrict__ stats_out, int4* __restrict__ vectors_out) {
    __shared__ int hist[2][2 * MO_MAX_R + 1];
    __shared__ int med[2];
    __shared__ unsigned long long sums[7];
    const int b = blockIdx.x, t = threadIdx.x;
    unsigned char* const sb = state + (size_t)b * a.stride;
    int* const hdr = reinterpret_cast<int*>(sb);
    const int4* const vec = reinterpret_cast<const int4*>(sb + MO_HDR);
    const int W = frames[b].width, H = frames[b].height;
    const MoGeom g = mo_geom(W, H, a);
    const int parity = hdr[0] & 1;
    const bool seeded = hdr[1] != 0 && hdr[2] == H && hdr[3] == W;
    const int nb = g.nbx * g.nby;
    const int r = a.r;
    for (int i = t; i < 2 * (2 * MO_MAX_R + 1); i += MO_NT) (&hist[0][0])[i] = 0;
    if (t < 7) sums[t] = 0;
    __syncthreads();
    if (seeded)
        for (int i = t; i < nb; i += MO_NT) {
            const int4 v = vec[i];
            if (v.w) { atomicAdd(&hist[0][v.x + r], 1); atomicAdd(&hist[1][v.y + r], 1); }
        }
    __syncthreads();
    int valid = 0;
    for (int i = 0; i <= 2 * r; ++i) valid += hist[0][i];
    if (t < 2 && valid > 0) {
        // the lower median: the element of rank (valid - 1) / 2 in ascending order
        const int want = (valid - 1) / 2 + 1;
        int cum = 0, i = 0;
        for (; i <= 2 * r; ++i) { cum += hist[t][i]; if (cum >= want) break; }
        med[t] = i - r;
    }
    __syncthreads();
    if (valid > 0) {
        const int mdx = med[0], mdy = med[1];
        long long s[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int i = t; i < nb; i += MO_NT) {
            const int4 v = vec[i];
            const int ex = v.x - mdx, ey = v.y - mdy;
            const int e = max(ex < 0 ? -ex : ex, ey < 0 ? -ey : ey);
            if (!v.w || e > 2) continue;
            const int bj = i / g.nbx, bi = i - bj * g.nbx;
            const long long xc = r + bi * a.blk + a.blk / 2, yc = r + bj * a.blk + a.blk / 2;      // the block's centre u = (x', y')
            const long long x = xc + v.x, y = yc + v.y;
            s[0] += 1; s[1] += x; s[2] += y; s[3] += xc; s[4] += yc; s[5] += x * x + y * y; s[6] += x * xc + y * yc;
        }
        if (s[0])
#pragma unroll
            for (int i = 0; i < 7; ++i) atomicAdd(&sums[i], (unsigned long long)s[i]);
    }
    __syncthreads();
    if (vectors_out) {
        int4* const vo = vectors_out + (size_t)b * a.max_blocks;
        for (int i = t; i < a.max_blocks; i += MO_NT) vo[i] = vec[i];
    }
    __syncthreads();            // (everyone has read the header)
    if (t == 0) {
        const long long n = (long long)sums[0], sx = (long long)sums[1], sy = (long long)sums[2], sxp = (long long)sums[3], syp = (long long)sums[4],
                        sqq = (long long)sums[5], sxx = (long long)sums[6];
        float4 mo = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
        const long long num = n * sxx - sx * sxp - sy * syp, den = n * sqq - sx * sx - sy * sy;
        if (seeded && valid >= a.min_blocks && n * 2 >= valid && den != 0) {
            const double s = (double)num / (double)den;
            if (s >= 0.8 && s <= 1.25) {
                const double dn = (double)n;
                const double tu = ((double)sxp - s * (double)sx) / dn;
                const double tv = ((double)syp - s * (double)sy) / dn;
                const double dk = (double)g.k;
                const double c = ((1.0 - s) * (double)(g.k - 1)) / 2.0;
                mo = make_float4((float)s, (float)(dk * tu + c), (float)(dk * tv + c), 1.0f);
            }
        }
        motion_out[b] = mo;
        stats_out[b] = make_int4(nb, valid, (int)n, g.k);
        hdr[0] = parity ^ 1; hdr[1] = 1; hdr[2] = H; hdr[3] = W;
    }
}

__global__ __launch_bounds__(MO_NT) void motion_reset_kernel(unsigned char* __restrict__ state, const uint8_t* __restrict__ which, size_t stride) {
    const int b = blockIdx.x;
    if (which && which[b] == 0) return;
    uint4* const g = reinterpret_cast<uint4*>(state + (size_t)b * stride);
    for (size_t i = threadIdx.x; i < stride / 16; i += MO_NT) g[i] = make_uint4(0u, 0u, 0u, 0u);
}

// A thread per track slot of a stream whose step is ok.
__global__ __launch_bounds__(64) void track_compensate_kernel(float* __restrict__ state, const float4* __restrict__ motion, int T, int Tp, size_t words) {
    const int b = blockIdx.y, slot = blockIdx.x * 64 + threadIdx.x;
    const float4 mo = motion[b];
    if (!(mo.w != 0.0f) || slot >= T) return;
    float* const g = state + (size_t)b * words;
    if (reinterpret_cast<const int*>(g)[TK_HDR + slot] == TK_FREE) return;
    float* const f = g + TK_HDR + 5 * (size_t)Tp + slot;       // filter row i of this slot: f[i * Tp]
    const float s = mo.x, s2 = s * s;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k == 2) continue;                                   // a = w / h does not change
        float* const c = f + (size_t)(5 * k) * Tp;
        const float x = s * c[0];
        c[0] = k == 0 ? x + mo.y : (k == 1 ? x + mo.z : x);
        c[Tp] = s * c[Tp];
        c[2 * (size_t)Tp] = c[2 * (size_t)Tp] * s2;
        c[3 * (size_t)Tp] = c[3 * (size_t)Tp] * s2;
        c[4 * (size_t)Tp] = c[4 * (size_t)Tp] * s2;
    }
}

// what every entry point checks of the parameters; DN_OK or the error code
inline int mo_check_params(const char* who, const dn_motion_params* params) {
    DN_REQUIRE(params, "%s: null params", who);
    const dn_motion_params& p = *params;
    DN_REQUIRE(p.block == 8 || p.block == 16, "%s: block=%d must be 8 or 16", who, p.block);
    DN_REQUIRE(p.radius >= 1 && p.radius <= MO_MAX_R, "%s: radius=%d must be 1 .. %d", who, p.radius, MO_MAX_R);
    DN_REQUIRE(p.max_h >= 1 && p.max_w >= 1, "%s: bad capacity %d x %d", who, p.max_h, p.max_w);
    DN_REQUIRE(p.min_texture >= 0 && p.min_blocks >= 1, "%s: min_texture=%d must be >= 0, min_blocks=%d >= 1", who, p.min_texture, p.min_blocks);
    DN_REQUIRE(p.mask_thresh == p.mask_thresh, "%s: mask_thresh must be a number", who);
    DN_REQUIRE(p.reserved == 0, "%s: the reserved word must be 0", who);
    const int need = p.block + 2 * p.radius;
    if (p.max_h > MO_MAX_SIDE || p.max_w > MO_MAX_SIDE || p.max_h < need || p.max_w < need) {
        dn_set_error("%s: capacity %d x %d, each side must be block + 2 radius = %d .. %d", who, p.max_h, p.max_w, need, MO_MAX_SIDE);
        return DN_E_UNSUPPORTED;
    }
    return DN_OK;
}

inline MoArgs mo_args(const dn_motion_params& p, int d) {
    MoArgs a;
    a.TH = p.max_h; a.TW = p.max_w; a.TWp = (int)mo_up16(p.max_w);
    a.blk = p.block; a.r = p.radius; a.min_texture = p.min_texture; a.min_blocks = p.min_blocks; a.max_blocks = mo_max_blocks(p);
    a.mask_thresh = p.mask_thresh; a.d = d; a.stride = mo_stride(p);
    return a;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) size_t dn_motion_state_bytes(int streams, const dn_motion_params* params) {
    if (streams < 1 || streams > MO_MAX_STREAMS || mo_check_params("dn_motion_state_bytes", params) != DN_OK) return 0;
    return (size_t)streams * mo_stride(*params);
}

extern "C" __attribute__((visibility("default"))) int dn_motion_reset(void* state, size_t state_bytes, int streams, const dn_motion_params* params,
                                                                     const uint8_t* which, void* stream) {
    DN_REQUIRE(state, "dn_motion_reset: null state");
    DN_REQUIRE(streams >= 1, "dn_motion_reset: bad streams=%d", streams);
    DN_REQUIRE((reinterpret_cast<size_t>(state) & 15) == 0, "dn_motion_reset: the state must be 16-byte aligned");
    const int rc = mo_check_params("dn_motion_reset", params);
    if (rc != DN_OK) return rc;
    if (streams > MO_MAX_STREAMS) {
        dn_set_error("dn_motion_reset: streams=%d, at most %d", streams, MO_MAX_STREAMS);
        return DN_E_UNSUPPORTED;
    }
    const size_t stride = mo_stride(*params);
    if (state_bytes < stride * streams) {
        dn_set_error("dn_motion_reset: state of %zu B, %zu B needed", state_bytes, stride * streams);
        return DN_E_WORKSPACE;
    }
    dn_note_kernel("motion_reset_kernel");
    hipLaunchKernelGGL(motion_reset_kernel, dim3(streams), dim3(MO_NT), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<unsigned char*>(state),
                       which, stride);
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}

extern "C" __attribute__((visibility("default"))) int dn_motion_estimate(const dn_frame* frames, int n, int format, const dn_motion_params* params,
                                                                        const float* boxes, const float* scores, const int32_t* counts, int d,
                                                                        void* state, size_t state_bytes, float* motion_out, int32_t* stats_out,
                                                                        int32_t* vectors_out, void* stream) {
    DN_REQUIRE(frames && state && motion_out && stats_out, "dn_motion_estimate: null argument");
    DN_REQUIRE(n >= 1, "dn_motion_estimate: bad n=%d", n);
    const int rc = mo_check_params("dn_motion_estimate", params);
    if (rc != DN_OK) return rc;
    const bool masking = boxes || scores || counts;
    DN_REQUIRE(!masking || (boxes && scores && counts), "dn_motion_estimate: boxes, scores and counts come together or not at all");
    DN_REQUIRE(!masking || d >= 1, "dn_motion_estimate: bad d=%d", d);
    DN_REQUIRE(((reinterpret_cast<size_t>(state) | reinterpret_cast<size_t>(motion_out) | reinterpret_cast<size_t>(stats_out) |
                 reinterpret_cast<size_t>(vectors_out) | reinterpret_cast<size_t>(boxes)) & 15) == 0 &&
                   ((reinterpret_cast<size_t>(scores) | reinterpret_cast<size_t>(counts)) & 3) == 0 && (reinterpret_cast<size_t>(frames) & 7) == 0,
               "dn_motion_estimate: the state, boxes and the outputs must be 16-byte aligned, the frame table 8-byte, scores and counts 4-byte aligned");
    if (format != DN_FRAME_NV12 && format != DN_FRAME_I420 && format != DN_FRAME_RGB24 && format != DN_FRAME_BGR24) {
        dn_set_error("dn_motion_estimate: unknown format code %d", format);
        return DN_E_UNSUPPORTED;
    }
    if (n > MO_MAX_STREAMS || (masking && d > MO_MAX_D)) {
        dn_set_error("dn_motion_estimate: n=%d at most %d, d=%d at most %d", n, MO_MAX_STREAMS, d, MO_MAX_D);
        return DN_E_UNSUPPORTED;
    }
    const MoArgs a = mo_args(*params, masking ? d : 0);
    if (state_bytes < a.stride * n) {
        dn_set_error("dn_motion_estimate: state of %zu B, %zu B needed", state_bytes, a.stride * n);
        return DN_E_WORKSPACE;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned char* const st = reinterpret_cast<unsigned char*>(state);
    const dim3 tgrid(((a.TWp / 4) * a.TH + MO_NT - 1) / MO_NT, n);
    switch (format) {
        case DN_FRAME_RGB24: hipLaunchKernelGGL(motion_thumb_kernel<DN_FRAME_RGB24>, tgrid, dim3(MO_NT), 0, s, frames, st, a); break;
        case DN_FRAME_BGR24: hipLaunchKernelGGL(motion_thumb_kernel<DN_FRAME_BGR24>, tgrid, dim3(MO_NT), 0, s, frames, st, a); break;
        default: hipLaunchKernelGGL(motion_thumb_kernel<DN_FRAME_NV12>, tgrid, dim3(MO_NT), 0, s, frames, st, a); break;      // (I420's luma plane lies the same)
    }
    DN_HIP_CHECK(hipGetLastError());
    const dim3 mgrid(a.max_blocks, n);
    const float4* const bx = reinterpret_cast<const float4*>(boxes);
    if (a.blk == 16) hipLaunchKernelGGL(motion_match_kernel<16>, mgrid, dim3(64), 0, s, frames, bx, scores, counts, st, a);
    else hipLaunchKernelGGL(motion_match_kernel<8>, mgrid, dim3(64), 0, s, frames, bx, scores, counts, st, a);
    DN_HIP_CHECK(hipGetLastError());
    dn_note_kernel("motion_fit_kernel");
    hipLaunchKernelGGL(motion_fit_kernel, dim3(n), dim3(MO_NT), 0, s, frames, st, a, reinterpret_cast<float4*>(motion_out),
                       reinterpret_cast<int4*>(stats_out), reinterpret_cast<int4*>(vectors_out));
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}

extern "C" __attribute__((visibility("default"))) int dn_track_compensate(void* state, size_t state_bytes, int streams, int max_tracks,
                                                                         const float* motion, void* stream) {
    DN_REQUIRE(state && motion, "dn_track_compensate: null argument");
    DN_REQUIRE(streams >= 1 && max_tracks >= 1, "dn_track_compensate: bad sizes streams=%d max_tracks=%d", streams, max_tracks);
    DN_REQUIRE(((reinterpret_cast<size_t>(state) | reinterpret_cast<size_t>(motion)) & 15) == 0,
               "dn_track_compensate: the state and motion must be 16-byte aligned");
    if (max_tracks > TK_NT || streams > MO_MAX_STREAMS) {
        dn_set_error("dn_track_compensate: max_tracks=%d at most %d, streams=%d at most %d", max_tracks, TK_NT, streams, MO_MAX_STREAMS);
        return DN_E_UNSUPPORTED;
    }
    const size_t words = tk_stream_words(max_tracks);
    if (state_bytes < (size_t)streams * words * 4) {
        dn_set_error("dn_track_compensate: state of %zu B, %zu B needed", state_bytes, (size_t)streams * words * 4);
        return DN_E_WORKSPACE;
    }
    dn_note_kernel("track_compensate_kernel");
    hipLaunchKernelGGL(track_compensate_kernel, dim3((max_tracks + 63) / 64, streams), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<float*>(state), reinterpret_cast<const float4*>(motion), max_tracks, tk_padded(max_tracks), words);
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}
