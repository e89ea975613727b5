// Surface dewarping on the device: dn_warp fills rectangles of the surfaces of one dn_frame table from the surfaces of another through a
// coordinate mesh and a bilinear filter. The rules are in include/demonet_hip.h and restated in tests/warp_ref.py; this file must agree with them bit
// for bit. Integers only: a position is |P| < 2^27 (chroma: 2^29), a blend 255 * 1024 + 512.
//   One launch, a fixed grid of persistent workgroups of 256 threads, the work list of compose.hip: tile t of the call belongs to the item whose tile0
//   is the largest <= t; a workgroup takes one contiguous run of tiles, finds its first item by bisection and walks on from there. Per tile of 32 x 32
//   destination pixels (4 x 4 mesh cells):
//     the tile's 25 control points go to LDS, once, and their range decides the tile's path: where the source footprint lies inside the frame and fits
//     the staging buffers it is copied to LDS with 16-byte loads and the taps are read from there (see "the staged path" below), else they are gathered;
//     thread (qx, qy) owns the 2 x 2 quad of pixels at (2 qx, 2 qy) with its chroma sample(s) -- the quad lies in one mesh cell --, interpolates its
//     positions and blends its taps. A gathered tap is clamped into its plane before the load and replaced by the border byte behind it where the
//     rule says so; a staged tile needs neither. So no mesh value leads to a read outside a surface;
//     the results go to an LDS copy of the tile whose rows are shifted by the destination row's address & 15, and leave from there in 16-byte stores
//     where a row piece is aligned and inside the rectangle, in bytes elsewhere.
// The tables are trusted (the header says how far): no clamp here replaces the caller's validation of indices, rectangles and mesh0.
#include "common.h"

namespace {

constexpr int WP_NT = 256;
constexpr int WP_TILE = 32;
constexpr int WP_PTS = WP_TILE / DN_WARP_CELL + 1;      // control points per tile side
constexpr int WP_GRID = 4096;                           // workgroups: short runs of tiles, as in compose.hip
constexpr int WP_MAX_ITEMS = 65536;
constexpr int WP_PACKED = 2;                            // the third instantiation: RGB24 and BGR24 are the same bytes
static_assert(sizeof(dn_warp_item) == 48 && sizeof(dn_warp_header) == 16, "the header pins these sizes");
static_assert(DN_WARP_CELL == 8 && WP_PTS == 5, "the shifts below are those of an 8-pixel cell");

struct WpArgs {
    const dn_frame* src;
    const dn_frame* dst;
    const dn_warp_header* table;
    const int2* mesh;
    int capacity;
    int stage;                           // 0: every tile gathers (the knob DN_WARP_STAGE=0: an A/B switch for tests and tools/time_warp.py)
};

// The tiles [t0, t1) of this workgroup and the item of t0; false when it has none. n_items is cut at the capacity the call was given.
struct WpWalk {
    const dn_warp_item* items;
    int n_items, n_tiles, t1, it, next0;
    dn_warp_item cur;
};

__device__ __forceinline__ bool wp_walk_begin(const WpArgs& a, WpWalk& w, int& t0) {
    w.items = reinterpret_cast<const dn_warp_item*>(a.table + 1);
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
__device__ __forceinline__ bool wp_walk_tile(WpWalk& w, int tile, int& jx0, int& jy0) {
    while (tile >= w.next0) {
        if (w.it + 1 >= w.n_items) return false;
        ++w.it;
        w.cur = w.items[w.it];
        w.next0 = w.it + 1 < w.n_items ? w.items[w.it + 1].tile0 : w.n_tiles;
    }
    const int local = tile - w.cur.tile0;
    const int tiles_x = (w.cur.dw + WP_TILE - 1) / WP_TILE;
    const int ty = local / tiles_x, tx = local - ty * tiles_x;
    jx0 = tx * WP_TILE;
    jy0 = ty * WP_TILE;
    return local >= 0 && jy0 < w.cur.dh;
}

// The four taps of a position q = (qx, qy) in 1/32 sample on a plane of W x H samples: coordinates clamped into the plane (every load is inside
// it), the blend weights, and per tap whether the sample counts or the border byte does (replicate: the clamped sample always counts).
struct WpTaps {
    int x0, x1, y0, y1;
    int w00, w01, w10, w11;
    bool in00, in01, in10, in11;
};

__device__ __forceinline__ WpTaps wp_taps(int qx, int qy, int W, int H, bool replicate) {
    WpTaps t;
    const int x0 = qx >> 5, fx = qx & 31, y0 = qy >> 5, fy = qy & 31;      // >> of a signed int: arithmetic (floor)
    const int x1 = x0 + 1, y1 = y0 + 1;
    t.w00 = (32 - fx) * (32 - fy);
    t.w01 = fx * (32 - fy);
    t.w10 = (32 - fx) * fy;
    t.w11 = fx * fy;
    t.x0 = min(max(x0, 0), W - 1);
    t.x1 = min(max(x1, 0), W - 1);
    t.y0 = min(max(y0, 0), H - 1);
    t.y1 = min(max(y1, 0), H - 1);
    const bool ax0 = replicate || t.x0 == x0, ax1 = replicate || t.x1 == x1, ay0 = replicate || t.y0 == y0, ay1 = replicate || t.y1 == y1;
    t.in00 = ax0 && ay0;
    t.in01 = ax1 && ay0;
    t.in10 = ax0 && ay1;
    t.in11 = ax1 && ay1;
    return t;
}

// one byte channel through the taps: `step` bytes between the samples of a row, `off` the channel's byte inside a sample
__device__ __forceinline__ uint8_t wp_blend(const uint8_t* base, int pitch, int step, int off, const WpTaps& t, int border) {
    const uint8_t* const r0 = base + (size_t)t.y0 * pitch + off;
    const uint8_t* const r1 = base + (size_t)t.y1 * pitch + off;
    const int a = r0[(size_t)t.x0 * step], b = r0[(size_t)t.x1 * step], c = r1[(size_t)t.x0 * step], d = r1[(size_t)t.x1 * step];
    const int p00 = t.in00 ? a : border, p01 = t.in01 ? b : border, p10 = t.in10 ? c : border, p11 = t.in11 ? d : border;
    return (uint8_t)((t.w00 * p00 + t.w01 * p01 + t.w10 * p10 + t.w11 * p11 + 512) >> 10);
}

// rows x nb bytes of a tile from its LDS copy to the surface. p0: the address of the tile's first byte; row r of the copy starts at lds + r * 16 *
// PIECES and holds the row's bytes from offset (address of the row & 15) on, so an aligned 16-byte piece of the surface is an aligned one of the copy.
template <int PIECES>
__device__ __forceinline__ void wp_store_rows(uint8_t* p0, int pitch, int rows, int nb, const uint8_t* lds) {
    for (int idx = threadIdx.x; idx < rows * PIECES; idx += WP_NT) {
        const int r = idx / PIECES, k = idx - r * PIECES;
        uint8_t* const p = p0 + (size_t)r * pitch;
        const int mis = (int)(reinterpret_cast<size_t>(p) & 15);
        const int lo = k * 16 - mis, hi = lo + 16;
        if (lo >= nb) continue;
        const uint8_t* const row = lds + r * (16 * PIECES);
        if (lo >= 0 && hi <= nb) {
            *reinterpret_cast<uint4*>(p + lo) = *reinterpret_cast<const uint4*>(row + k * 16);
        } else {
            const int i0 = lo < 0 ? 0 : lo, i1 = hi < nb ? hi : nb;
            for (int i = i0; i < i1; ++i) p[i] = row[mis + i];
        }
    }
}

__device__ __forceinline__ int wp_mis(const uint8_t* p) { return (int)(reinterpret_cast<size_t>(p) & 15); }

// ---- the staged path. The bilinear interpolation of the mesh is a convex combination, so every position of a tile lies inside the bounding box of
// its 25 points [minX, maxX] x [minY, maxY] (1/64 pixel), and with the rounding of q every luma tap inside the samples
//     floor(min / 64) .. floor((max + 1) / 64) + 1,        every chroma tap inside      floor((min - 33) / 128) .. floor((max - 30) / 128) + 1.
// Where those boxes lie INSIDE their planes -- then no tap needs the border rule -- and fit the staging buffers below, the boxes are copied to LDS
// with aligned 16-byte loads (bytes where a piece leaves the row's payload) and the taps are read from there; otherwise (strong minification, a tile
// across the rim of a fisheye or the edge of the frame) the taps are gathered from global memory. Same arithmetic, same bits.
// A staged row r holds the bytes of the plane from the 16-byte boundary at or below the box's first byte of that row, at lds + r * SS: the box's
// byte i of the row is at offset (address & 15) + i.
constexpr int WP_ST_W = 112, WP_ST_H = 112;        // luma / packed box: at most 112 x 112 samples (a 32 x 32 tile at up to 3.4 : 1)
constexpr int WP_ST_CW = 64, WP_ST_CH = 64;        // chroma box: at most 64 x 64 samples (follows from the luma limit; checked all the same)

struct WpBox { int x0, y0, w, h; };

__device__ __forceinline__ bool wp_box(int lo_x, int hi_x, int lo_y, int hi_y, int W, int H, int maxw, int maxh, WpBox& b) {
    b.x0 = lo_x;
    b.y0 = lo_y;
    b.w = hi_x - lo_x + 1;
    b.h = hi_y - lo_y + 1;
    return lo_x >= 0 && lo_y >= 0 && hi_x < W && hi_y < H && b.w <= maxw && b.h <= maxh;
}

// copy the box (x0, y0, w, h samples of `step` bytes) of a plane whose rows hold `payload` bytes to LDS rows of SS bytes
template <int SS>
__device__ __forceinline__ void wp_stage(uint8_t* lds, const uint8_t* plane, int pitch, int payload, int step, const WpBox& b) {
    constexpr int PP = SS / 16;
    const int nb = b.w * step;
    for (int idx = threadIdx.x; idx < b.h * PP; idx += WP_NT) {
        const int r = idx / PP, k = idx - r * PP;
        const uint8_t* const row = plane + (size_t)(b.y0 + r) * pitch;
        const uint8_t* const a = row + (size_t)b.x0 * step;
        const int shift = wp_mis(a);
        const int lo = 16 * k - shift, hi = lo + 16;
        if (lo >= nb || hi <= 0) continue;
        const uint8_t* const g = a + lo;
        if (g >= row && g + 16 <= row + payload) {
            *reinterpret_cast<uint4*>(lds + r * SS + 16 * k) = *reinterpret_cast<const uint4*>(g);
        } else {
            const int i0 = lo < 0 ? 0 : lo, i1 = hi < nb ? hi : nb;      // (inside the box, which is inside the payload)
            for (int i = i0; i < i1; ++i) lds[r * SS + shift + i] = a[i];
        }
    }
}

// one byte channel from a staged box: a0 = the low bits of the address of the plane's byte (box x0, row 0)
template <int SS>
__device__ __forceinline__ uint8_t wp_blend_lds(const uint8_t* lds, unsigned a0, int pitch, const WpBox& b, int step, int off, int qx, int qy) {
    const int x0 = qx >> 5, fx = qx & 31, y0 = qy >> 5, fy = qy & 31;
    const unsigned s0 = (a0 + (unsigned)y0 * (unsigned)pitch) & 15u, s1 = (s0 + (unsigned)pitch) & 15u;
    const int rx = (x0 - b.x0) * step + off;
    const uint8_t* const p = lds + (y0 - b.y0) * SS + s0 + rx;
    const uint8_t* const q = lds + (y0 - b.y0 + 1) * SS + s1 + rx;
    const int p00 = p[0], p01 = p[step], p10 = q[0], p11 = q[step];
    return (uint8_t)(((32 - fx) * (32 - fy) * p00 + fx * (32 - fy) * p01 + (32 - fx) * fy * p10 + fx * fy * p11 + 512) >> 10);
}

__device__ __forceinline__ unsigned wp_low(const uint8_t* p) { return (unsigned)reinterpret_cast<size_t>(p); }

// LDS copy of a tile: packed 32 rows of 96 + 16 bytes; 4:2:0 the luma's 32 rows of 32 + 16 bytes, then NV12's 16 UV rows of 32 + 16 or I420's 16 + 16
// rows of 16 + 16
constexpr int WP_OUT_BYTES = 32 * 112;
constexpr int WP_OUT_CHROMA = 32 * 48, WP_OUT_V = WP_OUT_CHROMA + 16 * 32;
// staging buffers: row strides (box bytes + 16; the luma's + 32 = 144: not a multiple of the 128 bytes of the LDS banks -- measured neutral) and sizes
constexpr int WP_SS_Y = WP_ST_W + 32, WP_SS_UV = 2 * WP_ST_CW + 16, WP_SS_C = WP_ST_CW + 16, WP_SS_RGB = 3 * WP_ST_W + 16;
constexpr int WP_ST_YUV_BYTES = WP_SS_Y * WP_ST_H + WP_SS_UV * WP_ST_CH;          // NV12: the luma box and the UV box
constexpr int WP_ST_I420_BYTES = WP_SS_Y * WP_ST_H + 2 * WP_SS_C * WP_ST_CH;
constexpr int WP_ST_RGB_BYTES = WP_SS_RGB * WP_ST_H;
static_assert(WP_SS_Y % 16 == 0 && WP_SS_UV % 16 == 0 && WP_SS_C % 16 == 0 && WP_SS_RGB % 16 == 0, "staged rows start on 16-byte boundaries");

template <int FMT>
__global__ __launch_bounds__(WP_NT) void warp_kernel(const WpArgs a) {
    constexpr bool PACKED = FMT == WP_PACKED;
    constexpr int BPP = PACKED ? 3 : 1;
    constexpr int ST_BYTES = PACKED ? WP_ST_RGB_BYTES : (FMT == DN_FRAME_NV12 ? WP_ST_YUV_BYTES : WP_ST_I420_BYTES);
    __shared__ int2 cp[WP_PTS * WP_PTS];
    __shared__ int4 range;                                              // minX, maxX, minY, maxY of the tile's points
    __shared__ uint4 out4[WP_OUT_BYTES / 16];
    __shared__ uint4 st4[ST_BYTES / 16];
    uint8_t* const out = reinterpret_cast<uint8_t*>(out4);
    uint8_t* const st = reinterpret_cast<uint8_t*>(st4);
    uint8_t* const st_u = st + (PACKED ? 0 : WP_SS_Y * WP_ST_H);
    uint8_t* const st_v = st_u + WP_SS_C * WP_ST_CH;                    // I420 only
    WpWalk w;
    int t0;
    if (!wp_walk_begin(a, w, t0)) return;
    const int t = threadIdx.x, qx = t & 15, qy = t >> 4;
    const int lx = 2 * qx, ly = 2 * qy;                                  // the quad's first pixel in the tile
    const int cell = (ly >> 3) * WP_PTS + (lx >> 3);
    for (int tile = t0; tile < w.t1; ++tile) {
        int jx0, jy0;
        if (!wp_walk_tile(w, tile, jx0, jy0)) break;
        const dn_warp_item I = w.cur;
        const dn_frame fs = a.src[I.src], fd = a.dst[I.dst];
        const int tw = min(WP_TILE, I.dw - jx0), th = min(WP_TILE, I.dh - jy0);
        if (t < 64) {
            // the first wave loads the points and reduces their range. The points of cells the tile does not reach are not used: their indices are
            // clamped into the item's mesh (lanes 25 .. 63 repeat point 24)
            const int tt = min(t, WP_PTS * WP_PTS - 1);
            const int r = tt / WP_PTS, c = tt - r * WP_PTS;
            const int mesh_h = ((I.dh + DN_WARP_CELL - 1) >> 3) + 1;
            const int mx = min((jx0 >> 3) + c, I.mesh_w - 1), my = min((jy0 >> 3) + r, mesh_h - 1);
            const int2 pt = a.mesh[(size_t)I.mesh0 + (size_t)my * I.mesh_w + mx];
            if (t < WP_PTS * WP_PTS) cp[t] = pt;
            int lo_x = pt.x, hi_x = pt.x, lo_y = pt.y, hi_y = pt.y;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                lo_x = min(lo_x, __shfl_xor(lo_x, m));
                hi_x = max(hi_x, __shfl_xor(hi_x, m));
                lo_y = min(lo_y, __shfl_xor(lo_y, m));
                hi_y = max(hi_y, __shfl_xor(hi_y, m));
            }
            if (t == 0) range = make_int4(lo_x, hi_x, lo_y, hi_y);
        }
        __syncthreads();
        const int4 rg = range;
        WpBox by_, bc_;
        bool staged = wp_box(rg.x >> 6, ((rg.y + 1) >> 6) + 1, rg.z >> 6, ((rg.w + 1) >> 6) + 1, fs.width, fs.height, WP_ST_W, WP_ST_H, by_) && a.stage != 0;
        if (!PACKED)
            staged = wp_box((rg.x - 33) >> 7, ((rg.y - 30) >> 7) + 1, (rg.z - 33) >> 7, ((rg.w - 30) >> 7) + 1, (fs.width + 1) >> 1, (fs.height + 1) >> 1,
                            WP_ST_CW, WP_ST_CH, bc_) && staged;
        if (staged) {
            wp_stage<PACKED ? WP_SS_RGB : WP_SS_Y>(st, fs.plane[0], fs.pitch[0], fs.width * BPP, BPP, by_);
            if (FMT == DN_FRAME_NV12) wp_stage<WP_SS_UV>(st_u, fs.plane[1], fs.pitch[1], 2 * ((fs.width + 1) >> 1), 2, bc_);
            if (FMT == DN_FRAME_I420) {
                wp_stage<WP_SS_C>(st_u, fs.plane[1], fs.pitch[1], (fs.width + 1) >> 1, 1, bc_);
                wp_stage<WP_SS_C>(st_v, fs.plane[2], fs.pitch[2], (fs.width + 1) >> 1, 1, bc_);
            }
            __syncthreads();
        }
        const bool replicate = (I.flags & 1) == DN_WARP_BORDER_REPLICATE;
        const int b0 = I.border & 255, b1 = (I.border >> 8) & 255, b2 = (I.border >> 16) & 255;
        const int2 A = cp[cell], B = cp[cell + 1], C = cp[cell + WP_PTS], D = cp[cell + WP_PTS + 1];
        const int X = I.dx0 + jx0, Y = I.dy0 + jy0;                      // the tile's first pixel in the destination frame
        uint8_t* const d0 = const_cast<uint8_t*>(fd.plane[0]) + (size_t)Y * fd.pitch[0] + (size_t)X * BPP;
        constexpr int S0 = PACKED ? 112 : 48;
        const unsigned ay = wp_low(fs.plane[0]) + (unsigned)(by_.x0 * BPP);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int px = lx + (p & 1), py = ly + (p >> 1);
            if (px >= tw || py >= th) continue;
            const int i = px & 7, j = py & 7;
            const int Px = (8 - j) * ((8 - i) * A.x + i * B.x) + j * ((8 - i) * C.x + i * D.x);
            const int Py = (8 - j) * ((8 - i) * A.y + i * B.y) + j * ((8 - i) * C.y + i * D.y);
            const int qx_ = (Px + 64) >> 7, qy_ = (Py + 64) >> 7;
            uint8_t* const o = out + py * S0 + wp_mis(d0 + (size_t)py * fd.pitch[0]) + px * BPP;
            if (staged) {
                o[0] = wp_blend_lds<PACKED ? WP_SS_RGB : WP_SS_Y>(st, ay, fs.pitch[0], by_, BPP, 0, qx_, qy_);
                if (PACKED) {
                    o[1] = wp_blend_lds<WP_SS_RGB>(st, ay, fs.pitch[0], by_, 3, 1, qx_, qy_);
                    o[2] = wp_blend_lds<WP_SS_RGB>(st, ay, fs.pitch[0], by_, 3, 2, qx_, qy_);
                }
            } else {
                const WpTaps tp = wp_taps(qx_, qy_, fs.width, fs.height, replicate);
                o[0] = wp_blend(fs.plane[0], fs.pitch[0], BPP, 0, tp, b0);
                if (PACKED) {
                    o[1] = wp_blend(fs.plane[0], fs.pitch[0], 3, 1, tp, b1);
                    o[2] = wp_blend(fs.plane[0], fs.pitch[0], 3, 2, tp, b2);
                }
            }
        }
        uint8_t* const du = PACKED ? nullptr : const_cast<uint8_t*>(fd.plane[1]) + (size_t)(Y >> 1) * fd.pitch[1] + (size_t)(X >> 1) * (FMT == DN_FRAME_NV12 ? 2 : 1);
        uint8_t* const dv = FMT == DN_FRAME_I420 ? const_cast<uint8_t*>(fd.plane[2]) + (size_t)(Y >> 1) * fd.pitch[2] + (X >> 1) : nullptr;
        if (!PACKED && lx < tw && ly < th) {
            // the quad's chroma sample, at luma position (lx + 0.5, ly + 0.5) of the tile
            const int i2 = 2 * (lx & 7) + 1, j2 = 2 * (ly & 7) + 1;
            const int Px = (16 - j2) * ((16 - i2) * A.x + i2 * B.x) + j2 * ((16 - i2) * C.x + i2 * D.x);
            const int Py = (16 - j2) * ((16 - i2) * A.y + i2 * B.y) + j2 * ((16 - i2) * C.y + i2 * D.y);
            const int qx_ = ((Px + 512) >> 10) - 8, qy_ = ((Py + 512) >> 10) - 8;
            uint8_t u, v;
            if (staged) {
                if (FMT == DN_FRAME_NV12) {
                    const unsigned au = wp_low(fs.plane[1]) + (unsigned)(bc_.x0 * 2);
                    u = wp_blend_lds<WP_SS_UV>(st_u, au, fs.pitch[1], bc_, 2, 0, qx_, qy_);
                    v = wp_blend_lds<WP_SS_UV>(st_u, au, fs.pitch[1], bc_, 2, 1, qx_, qy_);
                } else {
                    u = wp_blend_lds<WP_SS_C>(st_u, wp_low(fs.plane[1]) + (unsigned)bc_.x0, fs.pitch[1], bc_, 1, 0, qx_, qy_);
                    v = wp_blend_lds<WP_SS_C>(st_v, wp_low(fs.plane[2]) + (unsigned)bc_.x0, fs.pitch[2], bc_, 1, 0, qx_, qy_);
                }
            } else {
                const WpTaps tp = wp_taps(qx_, qy_, (fs.width + 1) >> 1, (fs.height + 1) >> 1, replicate);
                if (FMT == DN_FRAME_NV12) {
                    u = wp_blend(fs.plane[1], fs.pitch[1], 2, 0, tp, b1);
                    v = wp_blend(fs.plane[1], fs.pitch[1], 2, 1, tp, b2);
                } else {
                    u = wp_blend(fs.plane[1], fs.pitch[1], 1, 0, tp, b1);
                    v = wp_blend(fs.plane[2], fs.pitch[2], 1, 0, tp, b2);
                }
            }
            if (FMT == DN_FRAME_NV12) {
                uint8_t* const o = out + WP_OUT_CHROMA + qy * 48 + wp_mis(du + (size_t)qy * fd.pitch[1]) + 2 * qx;
                o[0] = u;
                o[1] = v;
            } else {
                out[WP_OUT_CHROMA + qy * 32 + wp_mis(du + (size_t)qy * fd.pitch[1]) + qx] = u;
                out[WP_OUT_V + qy * 32 + wp_mis(dv + (size_t)qy * fd.pitch[2]) + qx] = v;
            }
        }
        __syncthreads();
        if (PACKED) {
            wp_store_rows<7>(d0, fd.pitch[0], th, 3 * tw, out);
        } else {
            const int cw = (tw + 1) >> 1, ch = (th + 1) >> 1;
            wp_store_rows<3>(d0, fd.pitch[0], th, tw, out);
            if (FMT == DN_FRAME_NV12) {
                wp_store_rows<3>(du, fd.pitch[1], ch, 2 * cw, out + WP_OUT_CHROMA);
            } else {
                wp_store_rows<2>(du, fd.pitch[1], ch, cw, out + WP_OUT_CHROMA);
                wp_store_rows<2>(dv, fd.pitch[2], ch, cw, out + WP_OUT_V);
            }
        }
        __syncthreads();                 // the next tile overwrites the points, the boxes and the copy
    }
}

inline size_t wp_addr(const void* p) { return reinterpret_cast<size_t>(p); }

}  // namespace

extern "C" __attribute__((visibility("default"))) int dn_warp(const dn_frame* src_frames, const dn_frame* dst_frames, int format, const void* table,
                                                             int capacity, const int32_t* mesh, void* stream) {
    DN_REQUIRE(src_frames && dst_frames && table && mesh, "dn_warp: null table");
    DN_REQUIRE(((wp_addr(src_frames) | wp_addr(dst_frames) | wp_addr(mesh)) & 7) == 0 && (wp_addr(table) & 15) == 0,
               "dn_warp: the frame tables and the mesh must be 8-byte aligned, the item table 16-byte");
    DN_REQUIRE(capacity >= 1, "dn_warp: capacity=%d, it takes 1 .. %d", capacity, WP_MAX_ITEMS);
    if (format != DN_FRAME_NV12 && format != DN_FRAME_I420 && format != DN_FRAME_RGB24 && format != DN_FRAME_BGR24) {
        dn_set_error("dn_warp: unknown format %d", format);
        return DN_E_UNSUPPORTED;
    }
    if (capacity > WP_MAX_ITEMS) {
        dn_set_error("dn_warp: capacity=%d, at most %d items", capacity, WP_MAX_ITEMS);
        return DN_E_UNSUPPORTED;
    }
    WpArgs a;
    a.src = src_frames;
    a.dst = dst_frames;
    a.table = static_cast<const dn_warp_header*>(table);
    a.mesh = reinterpret_cast<const int2*>(mesh);
    a.capacity = capacity;
    a.stage = dn_knob("DN_WARP_STAGE", 1);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(WP_GRID), block(WP_NT);
    const int which = format == DN_FRAME_NV12 || format == DN_FRAME_I420 ? format : WP_PACKED;
    dn_note_kernel("warp_kernel<%d>", which);
    if (which == DN_FRAME_NV12) hipLaunchKernelGGL((warp_kernel<DN_FRAME_NV12>), grid, block, 0, s, a);
    else if (which == DN_FRAME_I420) hipLaunchKernelGGL((warp_kernel<DN_FRAME_I420>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((warp_kernel<WP_PACKED>), grid, block, 0, s, a);
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}
