// Surface composition on the device: dn_compose scales, converts and tiles rectangles of the surfaces of one dn_frame table into
// rectangles of the surfaces of another; dn_surface_fill writes whole surfaces with one colour. The rules are in include/demonet_hip.h and restated
// in tests/compose_ref.py; this file must agree with them bit for bit. Integers only: every sum is an unsigned 32-bit sum that cannot wrap
// (255 sw sh <= 255 * 2^24), the division is the integer division.
//   One launch, a fixed grid of persistent workgroups of 256 threads. The work list is never written: tile t of the call belongs to the item whose
//   tile0 (the exclusive prefix sum of ceil(dw / 32) ceil(dh / 32), made by the caller when the table goes up) is the largest <= t. A workgroup takes
//   one contiguous run of tiles, finds its first item by bisection and walks on from there. Per tile of 32 x 32 destination pixels:
//     the edge positions (j sw) / dw of the tile's 33 column and 33 row edges go to LDS, one division each;
//     the source footprint is walked in bands of 128 (RGB kernels: 32) source rows: a horizontal pass makes, per band row and destination column, the weighted row sum
//     (weights: the overlap lengths of the header) into LDS, a vertical pass adds the band's rows into the accumulators of the thread's pixels;
//     after the last band (sum + D / 2) / D leaves as bytes.
//   The plane-wise kernel runs this three times per tile (Y at 32 x 32, U and V at 16 x 16 from the chroma rectangles), the RGB kernels once with three
//   channels: a source pixel becomes RGB8 by frame_tap_rgb8 as it is read, and thread (qx, qy) owns the 2 x 2 quad of destination pixels with its
//   chroma sample, so that U and V come from registers.
// The tables are trusted (the header says how far): no clamp here replaces the caller's validation.
#include "common.h"
#include "frametap.h"

namespace {

constexpr int CP_NT = 256;
constexpr int CP_TILE = 32;
constexpr int CP_BAND = 128;              // source rows per band of the footprint walk, plane-wise kernel: a 4:1 tile is one band, 16 loads in flight per thread
constexpr int CP_BAND_RGB = 32;           // RGB kernels: three channels of row sums per band row
constexpr int CP_GRID = 4096;             // workgroups: short runs of tiles even for a wall of previews
constexpr int CP_MAX_ITEMS = 65536;
static_assert(sizeof(dn_compose_item) == 48 && sizeof(dn_compose_header) == 16, "the header pins these sizes");

struct CpForward { int y[3], u[3], v[3], yo; };      // round(c * 2^14) of the RGB -> YUV matrix (demonet_amd/osd.py, forward_coeffs), the luma offset

struct CpArgs {
    const dn_frame* src;
    const dn_frame* dst;
    const dn_compose_header* table;
    int capacity;
    FrameColor k;
    CpForward fw;
};

// the forward matrices, as osd.forward_coeffs derives them in float64
inline bool cp_forward(int color, CpForward* f) {
    const bool full = (color & DN_COLOR_FULL_RANGE) != 0;
    switch (color & ~DN_COLOR_FULL_RANGE) {
        case DN_COLOR_BT601:
            *f = full ? CpForward{{4899, 9617, 1868}, {-2765, -5427, 8192}, {8192, -6860, -1332}, 0}
                      : CpForward{{4207, 8260, 1604}, {-2428, -4768, 7196}, {7196, -6026, -1170}, 16};
            return true;
        case DN_COLOR_BT709:
            *f = full ? CpForward{{3483, 11718, 1183}, {-1877, -6315, 8192}, {8192, -7441, -751}, 0}
                      : CpForward{{2991, 10064, 1016}, {-1649, -5547, 7196}, {7196, -6536, -660}, 16};
            return true;
    }
    return false;
}

__device__ __forceinline__ int cp_component(const int* c, int r, int g, int b, int off) {
    return frame_clamp8(((c[0] * r + c[1] * g + c[2] * b + (1 << 13)) >> 14) + off);      // >> of a signed int: arithmetic (floor)
}

// The tiles [t0, t1) of this workgroup and the item of t0; false when it has none. n_items is cut at the capacity the call was given.
struct CpWalk {
    const dn_compose_item* items;
    int n_items, n_tiles, t1, it, next0;
    dn_compose_item cur;
};

__device__ __forceinline__ bool cp_walk_begin(const CpArgs& a, CpWalk& w, int& t0) {
    w.items = reinterpret_cast<const dn_compose_item*>(a.table + 1);
    const int n = a.table->n_items;
    w.n_items = n < 0 ? 0 : (n > a.capacity ? a.capacity : n);
    w.n_tiles = a.table->n_tiles;
    if (w.n_items == 0 || w.n_tiles <= 0) return false;
    const long long per = ((long long)w.n_tiles + gridDim.x - 1) / gridDim.x;
    const long long first = per * blockIdx.x;
    if (first >= w.n_tiles) return false;
    t0 = (int)first;
    w.t1 = (int)(first + per < (long long)w.n_tiles ? first + per : (long long)w.n_tiles);
    int lo = 0, hi = w.n_items - 1;                       // the last item whose tile0 <= t0
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (w.items[mid].tile0 <= t0) lo = mid;
        else hi = mid - 1;
    }
    w.it = lo;
    w.cur = w.items[lo];
    w.next0 = lo + 1 < w.n_items ? w.items[lo + 1].tile0 : w.n_tiles;
    return true;
}

// the item of `tile` (tiles come in ascending order) and the tile's origin inside the item's destination rectangle; false: past the table
__device__ __forceinline__ bool cp_walk_tile(CpWalk& w, int tile, int& jx0, int& jy0) {
    while (tile >= w.next0) {
        if (w.it + 1 >= w.n_items) return false;
        ++w.it;
        w.cur = w.items[w.it];
        w.next0 = w.it + 1 < w.n_items ? w.items[w.it + 1].tile0 : w.n_tiles;
    }
    const int local = tile - w.cur.tile0;
    const int tiles_x = (w.cur.dw + CP_TILE - 1) / CP_TILE;
    const int ty = local / tiles_x, tx = local - ty * tiles_x;
    jx0 = tx * CP_TILE;
    jy0 = ty * CP_TILE;
    return local >= 0 && jy0 < w.cur.dh;
}

// edge positions of a tile: xe[j] = ((jx0 + j) sw) / dw for j = 0 .. tw, ye likewise; one division per edge
__device__ __forceinline__ void cp_edges(int* xe, int* ye, int jx0, int jy0, int tw, int th, unsigned sw, unsigned sh, unsigned dw, unsigned dh) {
    const int t = threadIdx.x;
    if (t <= tw) xe[t] = (int)(((unsigned)(jx0 + t) * sw) / dw);
    if (t >= 64 && t - 64 <= th) ye[t - 64] = (int)(((unsigned)(jy0 + t - 64) * sh) / dh);
}

// One plane sample grid to another. s, d: sample (0, 0) of the planes; ss, ds: bytes between samples of a row (2 inside NV12's UV plane).
struct CpPlane {
    const uint8_t* s;
    uint8_t* d;
    int sp, dp, ss, ds;
};

// The tile of (1 << wshift)^2 destination samples at (jx0, jy0) of the rectangle (dx0, dy0, dw, dh), from the rectangle (sx0, sy0, sw, sh).
__device__ __forceinline__ void cp_plane_tile(const CpPlane& P, int sx0, int sy0, unsigned sw, unsigned sh, int dx0, int dy0, unsigned dw, unsigned dh,
                                              int jx0, int jy0, int wshift, uint32_t* H, int* xe, int* ye) {
    const int t = threadIdx.x;
    const int side = 1 << wshift, mask = side - 1;
    const int tw = min(side, (int)dw - jx0), th = min(side, (int)dh - jy0);
    cp_edges(xe, ye, jx0, jy0, tw, th, sw, sh, dw, dh);
    __syncthreads();
    const int y_first = ye[0];
    const int y_end = (int)(((unsigned)(jy0 + th) * sh + dh - 1) / dh);           // exclusive
    uint32_t acc[4] = {0, 0, 0, 0};
    for (int band0 = y_first; band0 < y_end; band0 += CP_BAND) {
        const int nb = min(CP_BAND, y_end - band0);
        // horizontal: H[r][j] = sum over the source columns of destination column j of weight * sample, for the band's rows
        for (int it = t; it < (nb << wshift); it += CP_NT) {
            const int r = it >> wshift, j = it & mask;
            if (j >= tw) continue;
            const uint8_t* const row = P.s + (size_t)(sy0 + band0 + r) * P.sp + (size_t)sx0 * P.ss;
            const unsigned a = (unsigned)(jx0 + j) * sw, b = a + sw;
            unsigned s = (unsigned)xe[j], pos = s * dw, sum = 0;
            for (;;) {
                const unsigned nxt = pos + dw;
                const unsigned lo = a > pos ? a : pos, hi = b < nxt ? b : nxt;
                sum += (hi - lo) * row[(size_t)s * P.ss];
                if (nxt >= b) break;
                pos = nxt;
                ++s;
            }
            H[r * CP_TILE + j] = sum;
        }
        __syncthreads();
        // vertical: the band's rows into the accumulators of this thread's samples
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = t + q * CP_NT;
            const int i = e >> wshift, j = e & mask;
            if (i >= th || j >= tw) continue;
            const unsigned a = (unsigned)(jy0 + i) * sh, b = a + sh;
            int y = ye[i] > band0 ? ye[i] : band0;
            for (; y < band0 + nb; ++y) {
                const unsigned pos = (unsigned)y * dh, nxt = pos + dh;
                if (pos >= b) break;
                const unsigned lo = a > pos ? a : pos, hi = b < nxt ? b : nxt;
                acc[q] += (hi - lo) * H[(y - band0) * CP_TILE + j];
            }
        }
        __syncthreads();
    }
    const unsigned D = sw * sh;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = t + q * CP_NT;
        const int i = e >> wshift, j = e & mask;
        if (i >= th || j >= tw) continue;
        P.d[(size_t)(dy0 + jy0 + i) * P.dp + (size_t)(dx0 + jx0 + j) * P.ds] = (uint8_t)((acc[q] + D / 2) / D);
    }
}

// channel c (0: Y, 1: U, 2: V) of a 4:2:0 frame as a sample grid
__device__ __forceinline__ void cp_channel(const dn_frame& f, int fmt, int c, const uint8_t*& base, int& pitch, int& step) {
    if (c == 0) { base = f.plane[0]; pitch = f.pitch[0]; step = 1; }
    else if (fmt == DN_FRAME_NV12) { base = f.plane[1] + (c - 1); pitch = f.pitch[1]; step = 2; }
    else { base = c == 1 ? f.plane[1] : f.plane[2]; pitch = c == 1 ? f.pitch[1] : f.pitch[2]; step = 1; }      // (no indexed access: the record stays in registers)
}

// YUV -> YUV of one colour code: every plane on its own
template <int SRC, int DST>
__global__ __launch_bounds__(CP_NT) void compose_planes_kernel(const CpArgs a) {
    __shared__ uint32_t H[CP_BAND * CP_TILE];
    __shared__ int xe[CP_TILE + 1], ye[CP_TILE + 1];
    CpWalk w;
    int t0;
    if (!cp_walk_begin(a, w, t0)) return;
    for (int tile = t0; tile < w.t1; ++tile) {
        int jx0, jy0;
        if (!cp_walk_tile(w, tile, jx0, jy0)) break;
        const dn_compose_item I = w.cur;
        const dn_frame fs = a.src[I.src], fd = a.dst[I.dst];
#pragma unroll 1
        for (int c = 0; c < 3; ++c) {
            CpPlane P;
            const uint8_t* d;
            cp_channel(fs, SRC, c, P.s, P.sp, P.ss);
            cp_channel(fd, DST, c, d, P.dp, P.ds);
            P.d = const_cast<uint8_t*>(d);
            if (c == 0)
                cp_plane_tile(P, I.sx0, I.sy0, I.sw, I.sh, I.dx0, I.dy0, I.dw, I.dh, jx0, jy0, 5, H, xe, ye);
            else
                cp_plane_tile(P, I.sx0 >> 1, I.sy0 >> 1, (I.sw + 1) >> 1, (I.sh + 1) >> 1, I.dx0 >> 1, I.dy0 >> 1, (I.dw + 1) >> 1, (I.dh + 1) >> 1,
                              jx0 >> 1, jy0 >> 1, 4, H, xe, ye);
        }
    }
}

// every other pair: through RGB8 per source pixel, three channels resampled at luma resolution
template <int SRC, int DST>
__global__ __launch_bounds__(CP_NT) void compose_rgb_kernel(const CpArgs a) {
    constexpr bool DST_RGB = DST == DN_FRAME_RGB24 || DST == DN_FRAME_BGR24;
    __shared__ uint32_t H[3][CP_BAND_RGB * CP_TILE];
    __shared__ int xe[CP_TILE + 1], ye[CP_TILE + 1];
    CpWalk w;
    int t0;
    if (!cp_walk_begin(a, w, t0)) return;
    const int t = threadIdx.x, qx = t & 15, qy = t >> 4;
    for (int tile = t0; tile < w.t1; ++tile) {
        int jx0, jy0;
        if (!cp_walk_tile(w, tile, jx0, jy0)) break;
        const dn_compose_item I = w.cur;
        const dn_frame fs = a.src[I.src], fd = a.dst[I.dst];
        const unsigned sw = I.sw, sh = I.sh, dw = I.dw, dh = I.dh;
        const int tw = min(CP_TILE, I.dw - jx0), th = min(CP_TILE, I.dh - jy0);
        cp_edges(xe, ye, jx0, jy0, tw, th, sw, sh, dw, dh);
        __syncthreads();
        const int y_first = ye[0];
        const int y_end = (int)(((unsigned)(jy0 + th) * sh + dh - 1) / dh);
        uint32_t acc[4][3];
        bool in[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            acc[p][0] = acc[p][1] = acc[p][2] = 0;
            in[p] = 2 * qx + (p & 1) < tw && 2 * qy + (p >> 1) < th;
        }
        for (int band0 = y_first; band0 < y_end; band0 += CP_BAND_RGB) {
            const int nb = min(CP_BAND_RGB, y_end - band0);
            for (int it = t; it < nb * CP_TILE; it += CP_NT) {
                const int r = it >> 5, j = it & 31;
                if (j >= tw) continue;
                const int y = I.sy0 + band0 + r;
                const unsigned c0 = (unsigned)(jx0 + j) * sw, c1 = c0 + sw;
                unsigned s = (unsigned)xe[j], pos = s * dw, sr = 0, sg = 0, sb = 0;
                for (;;) {
                    const unsigned nxt = pos + dw;
                    const unsigned lo = c0 > pos ? c0 : pos, hi = c1 < nxt ? c1 : nxt;
                    int r8, g8, b8;
                    frame_tap_rgb8<SRC>(fs, I.sx0 + (int)s, y, a.k, r8, g8, b8);
                    sr += (hi - lo) * (unsigned)r8;
                    sg += (hi - lo) * (unsigned)g8;
                    sb += (hi - lo) * (unsigned)b8;
                    if (nxt >= c1) break;
                    pos = nxt;
                    ++s;
                }
                H[0][r * CP_TILE + j] = sr;
                H[1][r * CP_TILE + j] = sg;
                H[2][r * CP_TILE + j] = sb;
            }
            __syncthreads();
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (!in[p]) continue;
                const int i = 2 * qy + (p >> 1), j = 2 * qx + (p & 1);
                const unsigned r0 = (unsigned)(jy0 + i) * sh, r1 = r0 + sh;
                int y = ye[i] > band0 ? ye[i] : band0;
                for (; y < band0 + nb; ++y) {
                    const unsigned pos = (unsigned)y * dh, nxt = pos + dh;
                    if (pos >= r1) break;
                    const unsigned lo = r0 > pos ? r0 : pos, hi = r1 < nxt ? r1 : nxt;
                    const int at = (y - band0) * CP_TILE + j;
                    acc[p][0] += (hi - lo) * H[0][at];
                    acc[p][1] += (hi - lo) * H[1][at];
                    acc[p][2] += (hi - lo) * H[2][at];
                }
            }
            __syncthreads();
        }
        const unsigned D = sw * sh;
        int rgb[4][3];
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int c = 0; c < 3; ++c) rgb[p][c] = in[p] ? (int)((acc[p][c] + D / 2) / D) : 0;
        const int X = I.dx0 + jx0 + 2 * qx, Y = I.dy0 + jy0 + 2 * qy;      // the quad's first pixel in the destination frame
        uint8_t* const p0 = const_cast<uint8_t*>(fd.plane[0]);
        if (DST_RGB) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (!in[p]) continue;
                uint8_t* const o = p0 + (size_t)(Y + (p >> 1)) * fd.pitch[0] + (size_t)(X + (p & 1)) * 3;
                o[0] = (uint8_t)rgb[p][DST == DN_FRAME_RGB24 ? 0 : 2];
                o[1] = (uint8_t)rgb[p][1];
                o[2] = (uint8_t)rgb[p][DST == DN_FRAME_RGB24 ? 2 : 0];
            }
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (in[p]) p0[(size_t)(Y + (p >> 1)) * fd.pitch[0] + X + (p & 1)] = (uint8_t)cp_component(a.fw.y, rgb[p][0], rgb[p][1], rgb[p][2], a.fw.yo);
            if (in[0]) {
                // the chroma sample of the quad: the mean, rounded half up, of the quad's pixels inside the rectangle (1, 2 or 4), then the matrix
                const int n = 1 + (in[1] ? 1 : 0) + (in[2] ? 1 : 0) + (in[3] ? 1 : 0);
                int m[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) m[c] = (rgb[0][c] + rgb[1][c] + rgb[2][c] + rgb[3][c] + n / 2) / n;
                const uint8_t u = (uint8_t)cp_component(a.fw.u, m[0], m[1], m[2], 128), v = (uint8_t)cp_component(a.fw.v, m[0], m[1], m[2], 128);
                const int cx = X >> 1, cy = Y >> 1;
                if (DST == DN_FRAME_NV12) {
                    uint8_t* const o = const_cast<uint8_t*>(fd.plane[1]) + (size_t)cy * fd.pitch[1] + (size_t)cx * 2;
                    o[0] = u;
                    o[1] = v;
                } else {
                    const_cast<uint8_t*>(fd.plane[1])[(size_t)cy * fd.pitch[1] + cx] = u;
                    const_cast<uint8_t*>(fd.plane[2])[(size_t)cy * fd.pitch[2] + cx] = v;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------- dn_surface_fill
struct CpFillArgs {
    const dn_frame* frames;
    int format;
    int c0, c1, c2;
};

// byte `ph` (0 .. 2) of a pattern held in three registers
__device__ __forceinline__ uint32_t cp_pat(int ph, uint32_t p0, uint32_t p1, uint32_t p2) { return ph == 0 ? p0 : (ph == 1 ? p1 : p2); }

// nb bytes of a row with the period-P pattern (p0, p1, p2): 16-byte stores where a piece is aligned and inside the payload, bytes otherwise
__device__ __forceinline__ void cp_fill_row(uint8_t* p, int nb, int P, uint32_t p0, uint32_t p1, uint32_t p2) {
    const int mis = (int)(reinterpret_cast<size_t>(p) & 15);
    const int pieces = (nb + mis + 15) >> 4;
    for (int k = threadIdx.x; k < pieces; k += CP_NT) {
        const int lo = k * 16 - mis, hi = lo + 16;
        if (lo >= 0 && hi <= nb) {
            uint32_t wd[4];
            int ph = lo % P;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t v = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v |= cp_pat(ph, p0, p1, p2) << (8 * i);
                    ph = ph + 1 == P ? 0 : ph + 1;
                }
                wd[q] = v;
            }
            *reinterpret_cast<uint4*>(p + lo) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
        } else {
            const int i0 = lo < 0 ? 0 : lo, i1 = hi < nb ? hi : nb;
            for (int i = i0; i < i1; ++i) p[i] = (uint8_t)cp_pat(i % P, p0, p1, p2);
        }
    }
}

__global__ __launch_bounds__(CP_NT) void surface_fill_kernel(const CpFillArgs a) {
    const dn_frame f = a.frames[blockIdx.y];
    const int W = f.width, H = f.height, cw = (W + 1) >> 1, ch = (H + 1) >> 1;
    const bool rgb = a.format == DN_FRAME_RGB24 || a.format == DN_FRAME_BGR24;
    const int rows = rgb ? H : (a.format == DN_FRAME_NV12 ? H + ch : H + 2 * ch);
    for (int R = blockIdx.x; R < rows; R += gridDim.x) {
        uint32_t p0 = a.c0, p1 = a.c0, p2 = a.c0;
        int P = 1, r = R, nb = W, pitch = f.pitch[0];
        const uint8_t* base = f.plane[0];
        if (rgb) {
            P = 3;
            nb = 3 * W;
            p0 = a.format == DN_FRAME_RGB24 ? a.c0 : a.c2; p1 = a.c1; p2 = a.format == DN_FRAME_RGB24 ? a.c2 : a.c0;
        } else if (R >= H) {
            if (a.format == DN_FRAME_NV12) {
                base = f.plane[1]; pitch = f.pitch[1]; r = R - H; P = 2; nb = 2 * cw;
                p0 = a.c1; p1 = a.c2;
            } else {
                const bool second = R - H >= ch;
                base = second ? f.plane[2] : f.plane[1]; pitch = second ? f.pitch[2] : f.pitch[1];
                r = R - H - (second ? ch : 0); nb = cw;
                p0 = p1 = p2 = second ? a.c2 : a.c1;
            }
        }
        cp_fill_row(const_cast<uint8_t*>(base) + (size_t)r * pitch, nb, P, p0, p1, p2);
    }
}

inline size_t cp_addr(const void* p) { return reinterpret_cast<size_t>(p); }
inline bool cp_format_ok(int f) { return f == DN_FRAME_NV12 || f == DN_FRAME_I420 || f == DN_FRAME_RGB24 || f == DN_FRAME_BGR24; }
inline bool cp_yuv(int f) { return f == DN_FRAME_NV12 || f == DN_FRAME_I420; }

template <int SRC>
void cp_launch_rgb(int dst_format, hipStream_t s, const CpArgs& a) {
    const dim3 grid(CP_GRID), block(CP_NT);
    switch (dst_format) {
        case DN_FRAME_NV12: hipLaunchKernelGGL((compose_rgb_kernel<SRC, DN_FRAME_NV12>), grid, block, 0, s, a); break;
        case DN_FRAME_I420: hipLaunchKernelGGL((compose_rgb_kernel<SRC, DN_FRAME_I420>), grid, block, 0, s, a); break;
        case DN_FRAME_RGB24: hipLaunchKernelGGL((compose_rgb_kernel<SRC, DN_FRAME_RGB24>), grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL((compose_rgb_kernel<SRC, DN_FRAME_BGR24>), grid, block, 0, s, a); break;
    }
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int dn_compose(const dn_frame* src_frames, int src_format, int src_color, const dn_frame* dst_frames,
                                                                int dst_format, int dst_color, const dn_compose_header* table, int capacity,
                                                                void* stream) {
    DN_REQUIRE(src_frames && dst_frames && table, "dn_compose: null table");
    DN_REQUIRE(((cp_addr(src_frames) | cp_addr(dst_frames)) & 7) == 0 && (cp_addr(table) & 15) == 0,
               "dn_compose: the frame tables must be 8-byte aligned, the item table 16-byte");
    DN_REQUIRE(capacity >= 1, "dn_compose: capacity=%d, it takes 1 .. %d", capacity, CP_MAX_ITEMS);
    DN_REQUIRE(cp_format_ok(src_format) && cp_format_ok(dst_format), "dn_compose: unknown format %d -> %d", src_format, dst_format);
    CpArgs a;
    DN_REQUIRE(frame_color(src_color, &a.k) && cp_forward(dst_color, &a.fw), "dn_compose: unknown colour code %d -> %d", src_color, dst_color);
    if (capacity > CP_MAX_ITEMS) {
        dn_set_error("dn_compose: capacity=%d, at most %d items", capacity, CP_MAX_ITEMS);
        return DN_E_UNSUPPORTED;
    }
    a.src = src_frames;
    a.dst = dst_frames;
    a.table = table;
    a.capacity = capacity;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (cp_yuv(src_format) && cp_yuv(dst_format) && src_color == dst_color) {
        dn_note_kernel("compose_planes_kernel<%d,%d>", src_format, dst_format);
        const dim3 grid(CP_GRID), block(CP_NT);
        if (src_format == DN_FRAME_NV12 && dst_format == DN_FRAME_NV12) hipLaunchKernelGGL((compose_planes_kernel<DN_FRAME_NV12, DN_FRAME_NV12>), grid, block, 0, s, a);
        else if (src_format == DN_FRAME_NV12) hipLaunchKernelGGL((compose_planes_kernel<DN_FRAME_NV12, DN_FRAME_I420>), grid, block, 0, s, a);
        else if (dst_format == DN_FRAME_NV12) hipLaunchKernelGGL((compose_planes_kernel<DN_FRAME_I420, DN_FRAME_NV12>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((compose_planes_kernel<DN_FRAME_I420, DN_FRAME_I420>), grid, block, 0, s, a);
    } else {
        dn_note_kernel("compose_rgb_kernel<%d,%d>", src_format, dst_format);
        switch (src_format) {
            case DN_FRAME_NV12: cp_launch_rgb<DN_FRAME_NV12>(dst_format, s, a); break;
            case DN_FRAME_I420: cp_launch_rgb<DN_FRAME_I420>(dst_format, s, a); break;
            case DN_FRAME_RGB24: cp_launch_rgb<DN_FRAME_RGB24>(dst_format, s, a); break;
            default: cp_launch_rgb<DN_FRAME_BGR24>(dst_format, s, a); break;
        }
    }
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}

extern "C" __attribute__((visibility("default"))) int dn_surface_fill(const dn_frame* frames, int n, int format, int c0, int c1, int c2, void* stream) {
    DN_REQUIRE(frames && (cp_addr(frames) & 7) == 0, "dn_surface_fill: the frame table must be non-null and 8-byte aligned");
    DN_REQUIRE(n >= 1, "dn_surface_fill: n=%d", n);
    DN_REQUIRE(cp_format_ok(format), "dn_surface_fill: unknown format %d", format);
    DN_REQUIRE(c0 >= 0 && c0 <= 255 && c1 >= 0 && c1 <= 255 && c2 >= 0 && c2 <= 255, "dn_surface_fill: the colour bytes take 0 .. 255, got %d %d %d", c0, c1, c2);
    if (n > 65535) {
        dn_set_error("dn_surface_fill: n=%d, at most 65535 surfaces", n);
        return DN_E_UNSUPPORTED;
    }
    CpFillArgs a;
    a.frames = frames;
    a.format = format;
    a.c0 = c0; a.c1 = c1; a.c2 = c2;
    dn_note_kernel("surface_fill_kernel");
    hipLaunchKernelGGL(surface_fill_kernel, dim3(128, n), dim3(CP_NT), 0, reinterpret_cast<hipStream_t>(stream), a);
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}
