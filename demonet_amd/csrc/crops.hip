// Object crops from video surfaces behind the tracker: dn_crop_objects turns the boxes of every stream into fixed-size normalised
// patches cut from the frames at native resolution. The rules, step by step, are in include/demonet_hip.h and restated in tests/crops_ref.py;
// this file must agree with them bit for bit.
//   launch 1, crop_plan_kernel: one workgroup of 256 threads per stream. Thread t owns rows 2t and 2t + 1 (d <= 512): box -> margin -> square ->
//   integer rectangle clamped to the frame (steps 1-5). A prefix scan over the workgroup numbers the stream's survivors in row order; the compact
//   list of (row, X0, Y0, width, height) and the survivor count go to the workspace.
//   launch 2, crop_gather_kernel<FMT, HALF>: the host does not know how many rows survive, so the grid is capacity x row bands. Every workgroup
//   scans the at most 1024 stream counts in LDS and finds its slot's stream and rank there; a workgroup whose slot is beyond the kept ones writes
//   the -1 index row (band 0) and leaves. The per-column taps and weights are computed once per workgroup into LDS; a lane owns 4 (fp32) or
//   8 (fp16) adjacent output columns of one row, converts its taps with frame_tap_rgb8 (frametap.h, the network input's own definition; the
//   division by 255 behind it is a table of the same 256 quotients in LDS), blends,
//   normalises and leaves with one 16-byte store per channel plane -- single stores when out_w is no multiple of the vector width.
// Compiled with -ffp-contract=off: every operation of the header's text rounds once; the divisions are correctly rounded. Box values are not
// trusted: the rectangle is clamped against the frame record's own width and height before anything is read through it. No inline asm, no float
// atomics, no host synchronisation.
#include <type_traits>

#include "common.h"
#include "frametap.h"

namespace {

constexpr int CR_NT = 256;
constexpr int CR_WAVES = CR_NT / 64;
constexpr int CR_MAX_STREAMS = 1024, CR_MAX_D = 512, CR_MAX_OUT = 1024, CR_MAX_CAPACITY = 8192;
static_assert(CR_MAX_D == 2 * CR_NT && CR_MAX_STREAMS == 4 * CR_NT, "rows per thread of the plan launch, counts per thread of the gather launch");
static_assert(sizeof(dn_crop_params) == 64, "dn_crop_params: the header pins 64 bytes");

// the workspace: int32 survivors [streams], then [streams][d] entries of two int4: (row, X0, Y0, width), (height, 0, 0, 0)
inline size_t cr_list_offset(int streams) { return a256((size_t)streams * 4); }

struct CropPlanArgs {
    const dn_frame* frames;
    const float4* boxes;
    const int32_t* counts;
    const uint8_t* select;
    int32_t* wcount;
    int4* wlist;
    int d, square, min_w, min_h;
    float margin;
};

struct CropGatherArgs {
    const dn_frame* frames;
    const int32_t* wcount;
    const int4* wlist;
    void* patches;
    int4* index;
    int4* totals;
    int streams, d, capacity, oh, ow, band_rows;
    float mean[3], sd[3];
    FrameColor k;
};

// exclusive prefix sum of v over the workgroup in thread order, and the total. wtot: CR_WAVES ints of LDS.
__device__ __forceinline__ int cr_scan(const int v, int* wtot, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wtot[wave] = x;
    __syncthreads();
    int before = x - v, sum = 0;
#pragma unroll
    for (int w = 0; w < CR_WAVES; ++w) {
        const int c = wtot[w];
        if (w < wave) before += c;
        sum += c;
    }
    total = sum;
    return before;
}

__device__ __forceinline__ bool cr_finite(float v) { return fabsf(v) < INFINITY; }

// steps 1 (the box's own conditions) to 5 of a row; W, H >= 1 are the frame record's
__device__ __forceinline__ bool cr_rect(const float4 box, const int W, const int H, const CropPlanArgs& a, int4& r) {
    const float x1 = box.x, y1 = box.y, x2 = box.z, y2 = box.w;
    if (!(cr_finite(x1) && cr_finite(y1) && cr_finite(x2) && cr_finite(y2))) return false;
    const float w = x2 - x1, h = y2 - y1;
    if (!(w > 0.0f && h > 0.0f)) return false;
    const float mx = w * a.margin, my = h * a.margin;
    float xa = x1 - mx, xb = x2 + mx, ya = y1 - my, yb = y2 + my;
    if (a.square) {
        const float cw = xb - xa, ch = yb - ya;
        const float s = fmaxf(cw, ch), hs = s * 0.5f;
        const float cx = (xa + xb) * 0.5f, cy = (ya + yb) * 0.5f;
        xa = cx - hs; xb = cx + hs; ya = cy - hs; yb = cy + hs;
    }
    if (!(cr_finite(xa) && cr_finite(xb) && cr_finite(ya) && cr_finite(yb))) return false;
    if (!(xb > 0.0f && xa < (float)W && yb > 0.0f && ya < (float)H)) return false;
    // clamped in float, then converted; the integer clamp behind it changes nothing while W - 1 and H - 1 are exact in fp32 (frames below 2^24 pixels
    // a side) and keeps the rectangle inside the record's size beyond that
    int X0 = (int)fminf(fmaxf(floorf(xa), 0.0f), (float)(W - 1));
    X0 = X0 > W - 1 ? W - 1 : X0;
    int X1 = (int)fminf(fmaxf(ceilf(xb), (float)(X0 + 1)), (float)W);
    X1 = X1 > W ? W : (X1 < X0 + 1 ? X0 + 1 : X1);
    int Y0 = (int)fminf(fmaxf(floorf(ya), 0.0f), (float)(H - 1));
    Y0 = Y0 > H - 1 ? H - 1 : Y0;
    int Y1 = (int)fminf(fmaxf(ceilf(yb), (float)(Y0 + 1)), (float)H);
    Y1 = Y1 > H ? H : (Y1 < Y0 + 1 ? Y0 + 1 : Y1);
    const int width = X1 - X0, height = Y1 - Y0;
    if (width < a.min_w || height < a.min_h) return false;
    r = make_int4(X0, Y0, width, height);
    return true;
}

__global__ __launch_bounds__(CR_NT) void crop_plan_kernel(const CropPlanArgs a) {
    __shared__ int wtot[CR_WAVES];
    const int b = blockIdx.x, t = threadIdx.x, d = a.d;
    const int cnt = a.counts[b];
    const int n = cnt < 0 ? 0 : (cnt > d ? d : cnt);
    const int W = a.frames[b].width, H = a.frames[b].height;
    int4 r[2];
    bool ok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int j = 2 * t + i;
        ok[i] = false;
        if (j < n && (!a.select || a.select[(size_t)b * d + j] != 0)) ok[i] = cr_rect(a.boxes[(size_t)b * d + j], W, H, a, r[i]);
    }
    int total;
    int pos = cr_scan((ok[0] ? 1 : 0) + (ok[1] ? 1 : 0), wtot, total);
    int4* const list = a.wlist + (size_t)b * d * 2;
#pragma unroll
    for (int i = 0; i < 2; ++i)
        if (ok[i]) {
            list[2 * pos] = make_int4(2 * t + i, r[i].x, r[i].y, r[i].z);
            list[2 * pos + 1] = make_int4(r[i].w, 0, 0, 0);
            ++pos;
        }
    if (t == 0) a.wcount[b] = total;
}

// one axis of the resize n_in -> n_out at output index o, dn_forward_regions' expressions: first tap, second tap (clamped at the rectangle's edge), weight
__device__ __forceinline__ void cr_axis(const int n_in, const int n_out, const int o, int& i0, int& i1, float& l) {
    const float r = (float)n_in / (float)n_out;
    const float s = fmaxf(r * ((float)o + 0.5f) - 0.5f, 0.f);
    i0 = (int)s;
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    l = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
}

template <int FMT, bool HALF>
__global__ __launch_bounds__(CR_NT) void crop_gather_kernel(const CropGatherArgs a) {
    constexpr int VEC = HALF ? 8 : 4;
    typedef typename std::conditional<HALF, half_t, float>::type out_t;
    __shared__ __attribute__((aligned(16))) int xt0[CR_MAX_OUT];       // frame column of the first and of the second tap, per output column
    __shared__ __attribute__((aligned(16))) int xt1[CR_MAX_OUT];
    __shared__ __attribute__((aligned(16))) float xtl[CR_MAX_OUT];     // the second tap's weight
    __shared__ float unit[256];                                       // v / 255 for the 256 values of a byte (frame_unit)
    __shared__ int wtot[CR_WAVES];
    __shared__ int found[2];

    const int t = threadIdx.x, band = blockIdx.x, s = blockIdx.y;
    // 6. the survivors are numbered stream by stream: which stream holds slot s, and which of its survivors is it
    int c[4], own = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = 4 * t + i;
        c[i] = b < a.streams ? a.wcount[b] : 0;
        own += c[i];
    }
    int total;
    int before = cr_scan(own, wtot, total);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (s >= before && s < before + c[i]) {
            found[0] = 4 * t + i;
            found[1] = s - before;
        }
        before += c[i];
    }
    const int kept = total < a.capacity ? total : a.capacity;
    if (band == 0 && s == 0 && t == 0) a.totals[0] = make_int4(kept, total - kept, 0, 0);
    if (s >= kept) {                    // (the same for every thread of the workgroup)
        if (band == 0 && t == 0) {
            a.index[2 * s] = make_int4(-1, 0, 0, 0);
            a.index[2 * s + 1] = make_int4(0, 0, 0, 0);
        }
        return;
    }
    __syncthreads();
    const int b = found[0];
    const int4* const e = a.wlist + ((size_t)b * a.d + found[1]) * 2;
    const int4 e0 = e[0];
    const int X0 = e0.y, Y0 = e0.z, w = e0.w, h = e[1].x;
    if (band == 0 && t == 0) {
        a.index[2 * s] = make_int4(b, e0.x, X0, Y0);
        a.index[2 * s + 1] = make_int4(w, h, 0, 0);
    }
    const dn_frame f = a.frames[b];
    const int oh = a.oh, ow = a.ow;
    const bool one_tap = h == oh && w == ow;      // weights exactly (1, 0): bilerp would return its first tap unchanged
    const int G = (ow + VEC - 1) / VEC;           // lanes per row
    // the columns' taps, once per workgroup; the columns behind out_w that a ragged last lane still walks repeat the last one, so they stay in the rectangle
    for (int ox = t; ox < G * VEC; ox += CR_NT) {
        int x0, x1;
        float lx;
        cr_axis(w, ow, ox < ow ? ox : ow - 1, x0, x1, lx);
        xt0[ox] = X0 + x0;
        xt1[ox] = X0 + x1;
        xtl[ox] = lx;
    }
    // a tap's three divisions by 255 become three reads of a table that holds the same correctly rounded quotients: twelve divisions per output pixel were
    // most of the kernel's vector instructions
    static_assert(CR_NT == 256, "one table entry per thread");
    unit[t] = frame_unit(t);
    __syncthreads();

    const bool vector = ow % VEC == 0;            // every row of every plane then starts on a 16-byte boundary
    const int rows = min(a.band_rows, oh - band * a.band_rows);
    for (int item = t; item < rows * G; item += CR_NT) {
        const int ry = item / G, g = item - ry * G;
        const int oy = band * a.band_rows + ry, ox = g * VEC;
        int y0, y1;
        float ly;
        cr_axis(h, oh, oy, y0, y1, ly);
        const float hy = 1.f - ly;
        const int Ya = Y0 + y0, Yb = Y0 + y1;
        int xa[VEC], xb[VEC];
        float lx[VEC];
#pragma unroll
        for (int q = 0; q < VEC / 4; ++q) {
            const int4 va = *reinterpret_cast<const int4*>(&xt0[ox + 4 * q]), vb = *reinterpret_cast<const int4*>(&xt1[ox + 4 * q]);
            const float4 vl = *reinterpret_cast<const float4*>(&xtl[ox + 4 * q]);
            xa[4 * q] = va.x; xa[4 * q + 1] = va.y; xa[4 * q + 2] = va.z; xa[4 * q + 3] = va.w;
            xb[4 * q] = vb.x; xb[4 * q + 1] = vb.y; xb[4 * q + 2] = vb.z; xb[4 * q + 3] = vb.w;
            lx[4 * q] = vl.x; lx[4 * q + 1] = vl.y; lx[4 * q + 2] = vl.z; lx[4 * q + 3] = vl.w;
        }
        out_t o[3][VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            float v[3];
            if (one_tap) {
                int p[3];
                frame_tap_rgb8<FMT>(f, xa[i], Ya, a.k, p[0], p[1], p[2]);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) v[ch] = unit[p[ch]];
            } else {
                int p[3], q[3], r[3], u[3];
                frame_tap_rgb8<FMT>(f, xa[i], Ya, a.k, p[0], p[1], p[2]);
                frame_tap_rgb8<FMT>(f, xb[i], Ya, a.k, q[0], q[1], q[2]);
                frame_tap_rgb8<FMT>(f, xa[i], Yb, a.k, r[0], r[1], r[2]);
                frame_tap_rgb8<FMT>(f, xb[i], Yb, a.k, u[0], u[1], u[2]);
                const float hx = 1.f - lx[i];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) v[ch] = bilerp(unit[p[ch]], unit[q[ch]], unit[r[ch]], unit[u[ch]], hx, lx[i], hy, ly);
            }
            // 8. one subtraction, one correctly rounded division; the fp16 conversion rounds to nearest even
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) o[ch][i] = (out_t)((v[ch] - a.mean[ch]) / a.sd[ch]);
        }
        out_t* const dst = reinterpret_cast<out_t*>(a.patches) + (((size_t)s * 3) * oh + oy) * ow + ox;
        const size_t plane = (size_t)oh * ow;
        if (vector) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                uint4 pack;
                __builtin_memcpy(&pack, o[ch], 16);
                *reinterpret_cast<uint4*>(dst + ch * plane) = pack;
            }
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int i = 0; i < VEC; ++i)
                    if (ox + i < ow) dst[ch * plane + i] = o[ch][i];
        }
    }
}

template <int FMT>
void cr_launch_gather(bool half, dim3 grid, hipStream_t s, const CropGatherArgs& a) {
    if (half) hipLaunchKernelGGL((crop_gather_kernel<FMT, true>), grid, dim3(CR_NT), 0, s, a);
    else hipLaunchKernelGGL((crop_gather_kernel<FMT, false>), grid, dim3(CR_NT), 0, s, a);
}

inline bool cr_sizes_supported(int streams, int d) { return streams <= CR_MAX_STREAMS && d <= CR_MAX_D; }

}  // namespace

extern "C" __attribute__((visibility("default"))) size_t dn_crop_workspace_bytes(int streams, int d) {
    if (streams < 1 || d < 1 || !cr_sizes_supported(streams, d)) return 0;
    return cr_list_offset(streams) + (size_t)streams * d * 32;
}

extern "C" __attribute__((visibility("default"))) int dn_crop_objects(const dn_frame* frames, int format, int color, const float* boxes,
                                                                     const int32_t* counts, const uint8_t* select, int streams, int d,
                                                                     const dn_crop_params* params, void* patches_out, int32_t* index_out,
                                                                     int32_t* totals_out, void* workspace, size_t workspace_bytes, void* stream) {
    DN_REQUIRE(frames && boxes && counts && params && patches_out && index_out && totals_out && workspace, "dn_crop_objects: null argument");
    const dn_crop_params p = *params;
    DN_REQUIRE(streams >= 1 && d >= 1 && p.out_h >= 1 && p.out_w >= 1 && p.capacity >= 1,
               "dn_crop_objects: bad sizes streams=%d d=%d out_h=%d out_w=%d capacity=%d", streams, d, p.out_h, p.out_w, p.capacity);
    DN_REQUIRE(p.margin >= 0.0f && p.margin < INFINITY, "dn_crop_objects: margin=%g must be finite and >= 0", (double)p.margin);
    for (int c = 0; c < 3; ++c) {
        DN_REQUIRE(p.std[c] > 0.0f && p.std[c] < INFINITY, "dn_crop_objects: std[%d]=%g must be finite and > 0", c, (double)p.std[c]);
        DN_REQUIRE(fabsf(p.mean[c]) < INFINITY, "dn_crop_objects: mean[%d]=%g must be finite", c, (double)p.mean[c]);
    }
    DN_REQUIRE((p.square == 0 || p.square == 1) && (p.out_fp16 == 0 || p.out_fp16 == 1), "dn_crop_objects: square=%d and out_fp16=%d must be 0 or 1",
               p.square, p.out_fp16);
    DN_REQUIRE(p.min_width >= 1 && p.min_height >= 1, "dn_crop_objects: min_width=%d and min_height=%d must be >= 1", p.min_width, p.min_height);
    DN_REQUIRE(p.reserved[0] == 0 && p.reserved[1] == 0, "dn_crop_objects: the reserved words must be 0");
    DN_REQUIRE(((reinterpret_cast<size_t>(boxes) | reinterpret_cast<size_t>(patches_out) | reinterpret_cast<size_t>(index_out) |
                 reinterpret_cast<size_t>(totals_out) | reinterpret_cast<size_t>(workspace)) & 15) == 0 && (reinterpret_cast<size_t>(counts) & 3) == 0,
               "dn_crop_objects: boxes, patches, index, totals and the workspace must be 16-byte aligned, counts 4-byte aligned");
    FrameColor k;
    if (!dn_frame_codes_known(format, color) || !frame_color(color, &k)) {
        dn_set_error("dn_crop_objects: unknown format %d or colour code 0x%x", format, color);
        return DN_E_UNSUPPORTED;
    }
    if (!cr_sizes_supported(streams, d) || p.capacity > CR_MAX_CAPACITY || p.out_h > CR_MAX_OUT || p.out_w > CR_MAX_OUT) {
        dn_set_error("dn_crop_objects: streams=%d at most %d, d=%d at most %d, capacity=%d at most %d, out_h=%d and out_w=%d at most %d", streams,
                     CR_MAX_STREAMS, d, CR_MAX_D, p.capacity, CR_MAX_CAPACITY, p.out_h, p.out_w, CR_MAX_OUT);
        return DN_E_UNSUPPORTED;
    }
    const size_t need = dn_crop_workspace_bytes(streams, d);
    if (workspace_bytes < need) {
        dn_set_error("dn_crop_objects: workspace of %zu B, %zu B needed", workspace_bytes, need);
        return DN_E_WORKSPACE;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint8_t* const ws = reinterpret_cast<uint8_t*>(workspace);

    CropPlanArgs pa;
    pa.frames = frames;
    pa.boxes = reinterpret_cast<const float4*>(boxes);
    pa.counts = counts;
    pa.select = select;
    pa.wcount = reinterpret_cast<int32_t*>(ws);
    pa.wlist = reinterpret_cast<int4*>(ws + cr_list_offset(streams));
    pa.d = d; pa.square = p.square; pa.min_w = p.min_width; pa.min_h = p.min_height; pa.margin = p.margin;
    hipLaunchKernelGGL(crop_plan_kernel, dim3(streams), dim3(CR_NT), 0, s, pa);
    DN_HIP_CHECK(hipGetLastError());

    CropGatherArgs ga;
    ga.frames = frames;
    ga.wcount = pa.wcount;
    ga.wlist = pa.wlist;
    ga.patches = patches_out;
    ga.index = reinterpret_cast<int4*>(index_out);
    ga.totals = reinterpret_cast<int4*>(totals_out);
    ga.streams = streams; ga.d = d; ga.capacity = p.capacity; ga.oh = p.out_h; ga.ow = p.out_w;
    const int vec = p.out_fp16 ? 8 : 4, lanes_per_row = (p.out_w + vec - 1) / vec;
    ga.band_rows = CR_NT / lanes_per_row > 0 ? CR_NT / lanes_per_row : 1;       // a band is one pass of the workgroup where a row takes at most 256 lanes
    for (int c = 0; c < 3; ++c) { ga.mean[c] = p.mean[c]; ga.sd[c] = p.std[c]; }
    ga.k = k;
    const dim3 grid(dn_cdiv(p.out_h, ga.band_rows), p.capacity);
    dn_note_kernel("crop_gather_kernel<%d,%d>", format, p.out_fp16);
    switch (format) {
        case DN_FRAME_NV12: cr_launch_gather<DN_FRAME_NV12>(p.out_fp16 != 0, grid, s, ga); break;
        case DN_FRAME_I420: cr_launch_gather<DN_FRAME_I420>(p.out_fp16 != 0, grid, s, ga); break;
        case DN_FRAME_RGB24: cr_launch_gather<DN_FRAME_RGB24>(p.out_fp16 != 0, grid, s, ga); break;
        default: cr_launch_gather<DN_FRAME_BGR24>(p.out_fp16 != 0, grid, s, ga); break;
    }
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}
