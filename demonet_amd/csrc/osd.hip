// On-screen display on the device: dn_osd_paint paints track boxes, labels, counting lines, zone edges and redaction in place into the
// surfaces of a dn_frame table, in their own colour space. The rules are in include/demonet_hip.h and restated in tests/osd_ref.py; this file must
// agree with them bit for bit.
//   launch 1, osd_plan_kernel: one workgroup of 256 threads per stream. Thread t owns segment candidates 2t, 2t + 1 (16 lines + 16 x 16 zone edges)
//   and rows 2t, 2t + 1 (d <= 512): it validates them, makes the integer rectangles and formats the label bytes. Three prefix scans compact the live
//   primitives into the stream's list in paint order (segments, boxes, labels). The tiles a primitive can touch are marked in an LDS bitmap --
//   rectangles exactly, segments by os_seg_box -- and the marked tiles leave for the global work list behind one atomicAdd per workgroup. The
//   counter is zero on entry: the last workgroup of launch 2 clears it (a memset node in front would be a third graph node per step).
//   launch 2, osd_paint_kernel<FMT>: a fixed grid of persistent workgroups walks the list. Per tile of 32 x 32 luma pixels: the planes' tile rows
//   come into LDS (16-byte pieces where a piece is aligned and inside the tile's payload, bytes otherwise; an LDS row starts at the global row's
//   own misalignment so that aligned pieces are aligned on both sides), thread t takes the 2 x 2 luma quad (t & 15, t >> 4) with its chroma pair
//   into registers, the block sums of the four pixelate sizes are formed from the snapshot, the stream's primitives are culled against the tile
//   256 at a time into LDS in order and applied, the values go back to LDS and leave the way they came.
// Compiled with -ffp-contract=off: every operation of the segment test rounds once; the division is correctly rounded. Boxes, counts, labels, ids,
// the zone config, styles and names are not trusted: every rectangle is clamped against the frame record's own size before a tile is marked, and a
// tile's reads and writes stay inside the tile's payload. No inline asm, no float atomics, no host synchronisation.
#include "common.h"

namespace {

constexpr int OS_NT = 256;
constexpr int OS_WAVES = OS_NT / 64;
constexpr int OS_MAX_D = 512, OS_MAX_STREAMS = 65535;
constexpr int OS_SEGS = 16 + 16 * 16;                 // segment candidates of a dn_zone_config
constexpr int OS_BITS = 65536, OS_WORDS = OS_BITS / 32, OS_WORDS_PER_THREAD = OS_WORDS / OS_NT;      // the tile bitmap of a band of tile rows
constexpr int OS_GRID = 8192;                         // workgroups of launch 2: enough that the tail of the walk is short against the whole
constexpr int OS_TILE = 32;
static_assert(OS_MAX_D == 2 * OS_NT && OS_SEGS <= 2 * OS_NT, "two rows and two segment candidates per thread of the plan launch");
static_assert(sizeof(dn_osd_params) == 64 && sizeof(dn_osd_style) == 8 && sizeof(dn_osd_color) == 8, "the header pins these sizes");

enum { OS_SEG = 0, OS_BOX = 1, OS_LABEL = 2 };
// 32 bytes. OS_SEG: x0 .. y1 the bits of ax, ay, bx, by, col the colour, txt the alpha, extra the bits of r. OS_BOX: the rectangle, col the colour,
// extra = thickness | fill_alpha << 8 | block << 16. OS_LABEL: the label rectangle cut at the frame (x0, y0 are its uncut left and top), col and
// txt the two colours, extra = the row.
struct OsdPrim { int type, x0, y0, x1, y1; uint32_t col, txt, extra; };
static_assert(sizeof(OsdPrim) == 32, "two 16-byte words");

__host__ __device__ inline int os_pmax(int d) { return OS_SEGS + 2 * d; }
// the workspace: 256 bytes (bytes 0 .. 7: the tile counter, 64 bits so that no sum of tiles wraps; word 2: the last call's tiles, saturated;
// word 3: the paint workgroups that have finished), int4 info [streams] (segments, boxes, labels, any pixelate), the primitives
// [streams][os_pmax(d)], the label bytes [streams][d][32], the work list int2 [tile_capacity]
inline size_t os_info_offset() { return 256; }
inline size_t os_prim_offset(int streams) { return os_info_offset() + a256((size_t)streams * 16); }
inline size_t os_text_offset(int streams, int d) { return os_prim_offset(streams) + a256((size_t)streams * os_pmax(d) * sizeof(OsdPrim)); }
inline size_t os_list_offset(int streams, int d) { return os_text_offset(streams, d) + a256((size_t)streams * d * 32); }

struct OsdPlanArgs {
    const dn_frame* frames;
    const float4* boxes;
    const float* scores;
    const int64_t* labels;
    const int64_t* ids;
    const int32_t* counts;
    const dn_osd_style* styles;
    const uint8_t* names;
    const dn_osd_color* palette;
    const dn_zone_config* zones;
    int32_t* counter;
    int4* info;
    OsdPrim* prims;
    uint8_t* text;
    int2* list;
    int4* stats;
    int d, n_labels, n_colors, color_by_id, scale, capacity;
    dn_osd_style def;
    uint32_t line_col, zone_col, zone_alpha;
    float line_r, zone_r;
};

struct OsdPaintArgs {
    const dn_frame* frames;
    int32_t* counter;
    const int4* info;
    const OsdPrim* prims;
    const uint8_t* text;
    const int2* list;
    const uint8_t* font;
    int d, pmax, capacity, scale, label_alpha;
};

// exclusive prefix sum of v over the workgroup in thread order, and the total. wtot: OS_WAVES ints of LDS, free again on return.
__device__ __forceinline__ int os_scan(const int v, int* wtot, int& total) {
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
    for (int w = 0; w < OS_WAVES; ++w) {
        const int c = wtot[w];
        if (w < wave) before += c;
        sum += c;
    }
    total = sum;
    __syncthreads();
    return before;
}

__device__ __forceinline__ bool os_finite(float v) { return fabsf(v) < INFINITY; }
__device__ __forceinline__ int os_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The pixels a live segment can cover, as a rectangle cut at the frame; false for a segment the header skips (L == 0 or not finite) and for one
// that cannot reach the frame. q = a + t * d of the test lies, in fp32, between a and a + d (rounding is monotone), so the box spans a, b and
// a + d; two pixels more than the radius on every side cover the half pixel of the centre and the rounding of the distance.
__device__ __forceinline__ bool os_seg_box(float ax, float ay, float bx, float by, float r, int W, int H, int& x0, int& y0, int& x1, int& y1) {
    const float dx = bx - ax, dy = by - ay;
    const float L = dx * dx + dy * dy;
    if (!(L > 0.f && L < INFINITY)) return false;
    const float cx = ax + dx, cy = ay + dy;
    const float lx = floorf(fminf(fminf(ax, bx), cx) - r) - 2.f, hx = ceilf(fmaxf(fmaxf(ax, bx), cx) + r) + 2.f;
    const float ly = floorf(fminf(fminf(ay, by), cy) - r) - 2.f, hy = ceilf(fmaxf(fmaxf(ay, by), cy) + r) + 2.f;
    if (!(hx > 0.f && lx < (float)W && hy > 0.f && ly < (float)H)) return false;
    x0 = os_clampi((int)fminf(fmaxf(lx, 0.f), (float)W), 0, W);
    x1 = os_clampi((int)fminf(fmaxf(hx, 0.f), (float)W), 0, W);
    y0 = os_clampi((int)fminf(fmaxf(ly, 0.f), (float)H), 0, H);
    y1 = os_clampi((int)fminf(fmaxf(hy, 0.f), (float)H), 0, H);
    return x0 < x1 && y0 < y1;
}

// the label bytes of a row: name, " #" id, " " percent "%"; returns the length (<= 31)
__device__ int os_text(uint8_t* out, const uint8_t* name, bool has_id, int64_t id, bool with_score, float score) {
    int n = 0;
    if (name)
        for (int i = 0; i < 15; ++i) {
            const uint8_t c = name[i];
            if (c == 0) break;
            out[n++] = c;
        }
    if (has_id) {
        out[n++] = ' ';
        out[n++] = '#';
        if (id < 0 || id > 999999999) out[n++] = '?';
        else {
            uint32_t v = (uint32_t)id;
            uint8_t dg[10];
            int k = 0;
            do { dg[k++] = (uint8_t)('0' + v % 10u); v /= 10u; } while (v);
            while (k) out[n++] = dg[--k];
        }
    }
    if (with_score) {
        out[n++] = ' ';
        if (!os_finite(score)) out[n++] = '?';
        else {
            const float v = score * 100.f + 0.5f;
            uint32_t p = v < 0.f ? 0u : (v > 100.f ? 100u : (uint32_t)(int)v);
            if (p > 100u) p = 100u;
            if (p >= 100u) out[n++] = '1';
            if (p >= 10u) out[n++] = (uint8_t)('0' + p / 10u % 10u);
            out[n++] = (uint8_t)('0' + p % 10u);
        }
        out[n++] = '%';
    }
    return n;
}

// bits [lo, hi] of the bitmap
__device__ __forceinline__ void os_mark_span(uint32_t* bits, int lo, int hi) {
    for (int w = lo >> 5; w <= hi >> 5; ++w) {
        const int a = w == lo >> 5 ? lo & 31 : 0, b = w == hi >> 5 ? hi & 31 : 31;
        const uint32_t m = (b == 31 ? 0xffffffffu : (1u << (b + 1)) - 1u) & ~((1u << a) - 1u);
        atomicOr(&bits[w], m);
    }
}

// the tiles of the pixel rectangle r (x0, y0, x1, y1; nothing when empty) inside the band of tile rows [tb0, tb1)
__device__ __forceinline__ void os_mark_rect(uint32_t* bits, const int4 r, int tiles_x, int tb0, int tb1) {
    if (r.x >= r.z || r.y >= r.w) return;
    const int tx0 = r.x >> 5, tx1 = (r.z - 1) >> 5;
    const int ty0 = max(r.y >> 5, tb0), ty1 = min((r.w - 1) >> 5, tb1 - 1);
    for (int ty = ty0; ty <= ty1; ++ty) os_mark_span(bits, (ty - tb0) * tiles_x + tx0, (ty - tb0) * tiles_x + tx1);
}

__global__ __launch_bounds__(OS_NT) void osd_plan_kernel(const OsdPlanArgs a) {
    __shared__ uint32_t bits[OS_WORDS];
    __shared__ int wtot[OS_WAVES];
    __shared__ long long sbase;
    const int b = blockIdx.x, t = threadIdx.x, d = a.d;
    const int cnt = a.counts[b];
    const int n = cnt < 0 ? 0 : (cnt > d ? d : cnt);
    const int W = a.frames[b].width, H = a.frames[b].height;
    const int tiles_x = (W + OS_TILE - 1) / OS_TILE, tiles_y = (H + OS_TILE - 1) / OS_TILE;
    const bool frame_ok = W >= 1 && H >= 1 && tiles_x <= OS_BITS;
    OsdPrim* const prims = a.prims + (size_t)b * os_pmax(d);
    int4 rect[6];                       // what this thread's primitives can touch: 2 segments, 2 boxes, 2 labels
#pragma unroll
    for (int i = 0; i < 6; ++i) rect[i] = make_int4(0, 0, 0, 0);

    // 1. segments: candidate c < 16 is line c, the others edge (c - 16) & 15 of zone (c - 16) >> 4
    OsdPrim sp[2];
    bool sok[2] = {false, false};
    if (a.zones && frame_ok) {
        const dn_zone_config* const z = a.zones + b;
        const int n_lines = os_clampi(z->n_lines, 0, 16), n_zones = os_clampi(z->n_zones, 0, 16);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = 2 * t + i;
            float ax = 0.f, ay = 0.f, bx = 0.f, by = 0.f;
            bool have = false, line = c < 16;
            if (line) {
                if (c < n_lines) { ax = z->lines[c][0]; ay = z->lines[c][1]; bx = z->lines[c][2]; by = z->lines[c][3]; have = true; }
            } else if (c < OS_SEGS) {
                const int zi = (c - 16) >> 4, e = (c - 16) & 15;
                if (zi < n_zones) {
                    const int nv = os_clampi(z->nv[zi], 3, 16);
                    if (e < nv) {
                        const int e1 = e + 1 == nv ? 0 : e + 1;
                        ax = z->verts[zi][e][0]; ay = z->verts[zi][e][1]; bx = z->verts[zi][e1][0]; by = z->verts[zi][e1][1];
                        have = true;
                    }
                }
            }
            const float r = line ? a.line_r : a.zone_r;
            int x0, y0, x1, y1;
            if (have && os_seg_box(ax, ay, bx, by, r, W, H, x0, y0, x1, y1)) {
                sok[i] = true;
                rect[i] = make_int4(x0, y0, x1, y1);
                sp[i].type = OS_SEG;
                sp[i].x0 = __float_as_int(ax); sp[i].y0 = __float_as_int(ay); sp[i].x1 = __float_as_int(bx); sp[i].y1 = __float_as_int(by);
                sp[i].col = line ? a.line_col : a.zone_col;
                sp[i].txt = a.zone_alpha;
                sp[i].extra = __float_as_uint(r);
            }
        }
    }
    int n_seg;
    int pos = os_scan((sok[0] ? 1 : 0) + (sok[1] ? 1 : 0), wtot, n_seg);
#pragma unroll
    for (int i = 0; i < 2; ++i)
        if (sok[i]) prims[pos++] = sp[i];

    // 2. rows
    OsdPrim bp[2], lp[2];
    bool bok[2] = {false, false}, lok[2] = {false, false};
    int pix = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int j = 2 * t + i;
        if (j >= n || !frame_ok) continue;
        const size_t row = (size_t)b * d + j;
        const float4 box = a.boxes[row];
        if (!(os_finite(box.x) && os_finite(box.y) && os_finite(box.z) && os_finite(box.w))) continue;
        const int64_t label = a.labels[row];
        if (label < 0 || label >= (int64_t)a.n_labels) continue;
        dn_osd_style st = a.styles ? a.styles[label] : a.def;
        if (st.flags & DN_OSD_HIDE) continue;
        const int ix0 = os_clampi((int)fminf(fmaxf(floorf(box.x), 0.f), (float)W), 0, W);
        const int iy0 = os_clampi((int)fminf(fmaxf(floorf(box.y), 0.f), (float)H), 0, H);
        const int ix1 = os_clampi((int)fminf(fmaxf(ceilf(box.z), 0.f), (float)W), 0, W);
        const int iy1 = os_clampi((int)fminf(fmaxf(ceilf(box.w), 0.f), (float)H), 0, H);
        if (ix0 >= ix1 || iy0 >= iy1) continue;
        const int thick = st.thickness > 16 ? 16 : st.thickness;
        const int block = (st.pixelate == 4 || st.pixelate == 8 || st.pixelate == 16 || st.pixelate == 32) ? st.pixelate : 0;
        const bool has_id = a.ids != nullptr;
        const int64_t id = has_id ? a.ids[row] : 0;
        const uint32_t key = (has_id && a.color_by_id) ? (uint32_t)(uint64_t)id : (uint32_t)(uint64_t)label;
        const dn_osd_color pc = a.palette[key % (uint32_t)a.n_colors];
        const uint32_t col = pc.color[0] | pc.color[1] << 8 | pc.color[2] << 16, txt = pc.text[0] | pc.text[1] << 8 | pc.text[2] << 16;
        bok[i] = true;
        pix |= block;
        rect[2 + i] = make_int4(ix0, iy0, ix1, iy1);
        bp[i].type = OS_BOX; bp[i].x0 = ix0; bp[i].y0 = iy0; bp[i].x1 = ix1; bp[i].y1 = iy1;
        bp[i].col = col; bp[i].txt = 0; bp[i].extra = (uint32_t)thick | (uint32_t)st.fill_alpha << 8 | (uint32_t)block << 16;
        if (st.flags & DN_OSD_LABEL) {
            uint8_t tb[32];
#pragma unroll
            for (int q = 0; q < 32; ++q) tb[q] = 0;
            const int len = os_text(tb, a.names ? a.names + (size_t)label * 16 : nullptr, has_id, id, (st.flags & DN_OSD_SCORE) != 0, a.scores[row]);
            uint8_t* const dst = a.text + row * 32;
            for (int q = 0; q < 32; ++q) dst[q] = tb[q];
            const int cell = 8 * a.scale;
            const int top = iy0 >= cell ? iy0 - cell : iy0;
            const int right = min(ix0 + cell * len, W), bottom = min(top + cell, H);
            if (len > 0 && ix0 < right && top < bottom) {
                lok[i] = true;
                rect[4 + i] = make_int4(ix0, top, right, bottom);
                lp[i].type = OS_LABEL; lp[i].x0 = ix0; lp[i].y0 = top; lp[i].x1 = right; lp[i].y1 = bottom;
                lp[i].col = col; lp[i].txt = txt; lp[i].extra = (uint32_t)j;
            }
        }
    }
    int n_box, n_lab;
    pos = n_seg + os_scan((bok[0] ? 1 : 0) + (bok[1] ? 1 : 0), wtot, n_box);
#pragma unroll
    for (int i = 0; i < 2; ++i)
        if (bok[i]) prims[pos++] = bp[i];
    pos = n_seg + n_box + os_scan((lok[0] ? 1 : 0) + (lok[1] ? 1 : 0), wtot, n_lab);
#pragma unroll
    for (int i = 0; i < 2; ++i)
        if (lok[i]) prims[pos++] = lp[i];
    const int any_pix = __syncthreads_or(pix);
    if (t == 0) a.info[b] = make_int4(n_seg, n_box, n_lab, any_pix ? 1 : 0);

    // 3. the tiles, a band of tile rows at a time (one band unless the frame has more than 65536 tiles)
    int touched = 0, dropped = 0;
    if (frame_ok) {
        const int band = OS_BITS / tiles_x;
        for (int tb0 = 0; tb0 < tiles_y; tb0 += band) {
            const int tb1 = min(tb0 + band, tiles_y);
            for (int w = t; w < OS_WORDS; w += OS_NT) bits[w] = 0;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 6; ++i) os_mark_rect(bits, rect[i], tiles_x, tb0, tb1);
            __syncthreads();
            uint32_t mine[OS_WORDS_PER_THREAD];
            int have = 0;
#pragma unroll
            for (int q = 0; q < OS_WORDS_PER_THREAD; ++q) {
                mine[q] = bits[t * OS_WORDS_PER_THREAD + q];
                have += __popc(mine[q]);
            }
            int total;
            int at = os_scan(have, wtot, total);
            if (t == 0) sbase = total ? (long long)atomicAdd(reinterpret_cast<unsigned long long*>(a.counter), (unsigned long long)total) : 0;
            __syncthreads();
            const long long base = sbase;
#pragma unroll
            for (int q = 0; q < OS_WORDS_PER_THREAD; ++q) {
                uint32_t m = mine[q];
                while (m) {
                    const int bit = __ffs((int)m) - 1;
                    m &= m - 1;
                    const long long slot = base + at++;
                    if (slot < (long long)a.capacity) a.list[slot] = make_int2(b, tb0 * tiles_x + (t * OS_WORDS_PER_THREAD + q) * 32 + bit);
                }
            }
            const long long left = (long long)a.capacity - base;
            const int room = left <= 0 ? 0 : (left < (long long)total ? (int)left : total);
            touched += total;
            dropped += total - room;
            __syncthreads();
        }
    }
    if (t == 0) a.stats[b] = make_int4(n_box, n - n_box, touched, dropped);
}

// -------------------------------------------------------------------------------------------------------------------------------- launch 2
template <int FMT> struct OsdFmt {
    static constexpr bool RGB = FMT == DN_FRAME_RGB24 || FMT == DN_FRAME_BGR24;
    static constexpr int S0 = RGB ? 112 : 48;                          // LDS row stride of plane 0: 96 or 32 payload bytes + 16 of misalignment
    static constexpr int S1 = FMT == DN_FRAME_NV12 ? 48 : 32;          // of a chroma plane: 32 or 16 payload bytes + 16
    static constexpr int B0 = OS_TILE * S0;
    static constexpr int B1 = RGB ? 0 : (OS_TILE / 2) * S1;
    static constexpr int B2 = FMT == DN_FRAME_I420 ? (OS_TILE / 2) * S1 : 0;
};

// `rows` rows of nb bytes between a plane (row r at g + r * pitch) and LDS (row r at lds + r * stride + the global row's misalignment): 16-byte
// pieces where a piece is aligned and inside the nb bytes, single bytes otherwise
template <bool STORE>
__device__ __forceinline__ void os_copy(uint8_t* g, size_t pitch, int rows, int nb, uint8_t* lds, int stride) {
    const int slots = stride >> 4;
    for (int item = threadIdx.x; item < rows * slots; item += OS_NT) {
        const int r = item / slots, k = item - r * slots;
        uint8_t* const p = g + (size_t)r * pitch;
        const int mis = (int)(reinterpret_cast<size_t>(p) & 15);
        const int lo = k * 16 - mis, hi = lo + 16;
        if (lo >= nb) continue;
        uint8_t* const l = lds + r * stride + k * 16;
        if (lo >= 0 && hi <= nb) {
            if (STORE) *reinterpret_cast<uint4*>(p + lo) = *reinterpret_cast<const uint4*>(l);
            else *reinterpret_cast<uint4*>(l) = *reinterpret_cast<const uint4*>(p + lo);
        } else {
            const int i0 = lo < 0 ? 0 : lo, i1 = hi < nb ? hi : nb;
            for (int i = i0; i < i1; ++i) {
                if (STORE) p[i] = l[i - lo];
                else l[i - lo] = p[i];
            }
        }
    }
}

__device__ __forceinline__ int os_blend(int a, int c, int p) { return (a * c + (255 - a) * p + 127) / 255; }

// entry of the block-sum pyramid: level l (block 4 << l) at in-tile luma position (lx, ly)
__device__ __forceinline__ int os_pyr_index(int l, int lx, int ly) {
    const int bx = lx >> (2 + l), by = ly >> (2 + l);
    return l == 0 ? by * 8 + bx : (l == 1 ? 64 + by * 4 + bx : (l == 2 ? 80 + by * 2 + bx : 84));
}

template <int FMT>
__global__ __launch_bounds__(OS_NT, 3) void osd_paint_kernel(const OsdPaintArgs a) {
    typedef OsdFmt<FMT> F;
    constexpr bool RGB = F::RGB;
    __shared__ __attribute__((aligned(16))) uint8_t buf[F::B0 + F::B1 + F::B2];
    __shared__ __attribute__((aligned(16))) OsdPrim lp[OS_NT];
    __shared__ uint4 ltext[2 * OS_NT];
    __shared__ int pyr[3][85];
    __shared__ uint8_t font[512];
    __shared__ int wtot[OS_WAVES];

    const int t = threadIdx.x;
    for (int i = t; i < 512; i += OS_NT) font[i] = a.font[i];
    const unsigned long long marked = __hip_atomic_load(reinterpret_cast<unsigned long long*>(a.counter), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int n_tiles = marked > (unsigned long long)a.capacity ? a.capacity : (int)marked;
    const int qx = t & 15, qy = t >> 4;

    for (int item = blockIdx.x; item < n_tiles; item += gridDim.x) {
        int2 ent = a.list[item];
        ent = make_int2(__builtin_amdgcn_readfirstlane(ent.x), __builtin_amdgcn_readfirstlane(ent.y));      // (the same in every lane: scalar registers)
        const int b = ent.x;
        const dn_frame f = a.frames[b];
        const int4 info = a.info[b];
        const int W = f.width, H = f.height;
        const int tiles_x = (W + OS_TILE - 1) / OS_TILE;
        const int ty = ent.y / tiles_x, tx = ent.y - ty * tiles_x;
        const int X0 = tx * OS_TILE, Y0 = ty * OS_TILE;
        const int tw = min(OS_TILE, W - X0), th = min(OS_TILE, H - Y0);
        const int cw = (tw + 1) >> 1, chh = (th + 1) >> 1;              // chroma samples and rows of the tile
        const int n_prim = min(info.x + info.y + info.z, a.pmax);
        const OsdPrim* const prims = a.prims + (size_t)b * a.pmax;
        OsdPrim pr_first = {};                                          // the first pass's record travels with the tile's rows
        if (t < n_prim) pr_first = prims[t];

        // the tile's rows of every plane
        uint8_t* const g0 = const_cast<uint8_t*>(f.plane[0]) + (size_t)Y0 * f.pitch[0] + (size_t)X0 * (RGB ? 3 : 1);
        const int nb0 = RGB ? 3 * tw : tw;
        uint8_t* g1 = nullptr;
        uint8_t* g2 = nullptr;
        int nb1 = 0;
        if (!RGB) {
            if (FMT == DN_FRAME_NV12) {
                g1 = const_cast<uint8_t*>(f.plane[1]) + (size_t)(Y0 >> 1) * f.pitch[1] + X0;
                nb1 = 2 * cw;
            } else {
                g1 = const_cast<uint8_t*>(f.plane[1]) + (size_t)(Y0 >> 1) * f.pitch[1] + (X0 >> 1);
                g2 = const_cast<uint8_t*>(f.plane[2]) + (size_t)(Y0 >> 1) * f.pitch[2] + (X0 >> 1);
                nb1 = cw;
            }
        }
        uint8_t* const l0 = buf;
        uint8_t* const l1 = buf + F::B0;
        uint8_t* const l2 = buf + F::B0 + F::B1;
        os_copy<false>(g0, f.pitch[0], th, nb0, l0, F::S0);
        if (!RGB) {
            os_copy<false>(g1, f.pitch[1], chh, nb1, l1, F::S1);
            if (FMT == DN_FRAME_I420) os_copy<false>(g2, f.pitch[2], chh, nb1, l2, F::S1);
        }
        __syncthreads();

        // this thread's quad: luma rows 2 qy, 2 qy + 1, columns 2 qx, 2 qx + 1, chroma sample (qx, qy)
        const int lx = 2 * qx, ly = 2 * qy;
        bool in[4];
        uint8_t* at[4];                   // plane 0 bytes of the four pixels
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int x = lx + (p & 1), y = ly + (p >> 1);
            in[p] = x < tw && y < th;
            const int mis = (int)(reinterpret_cast<size_t>(g0 + (size_t)y * f.pitch[0]) & 15);
            at[p] = l0 + y * F::S0 + mis + x * (RGB ? 3 : 1);
        }
        uint8_t* cu = nullptr;
        uint8_t* cv = nullptr;
        if (!RGB) {
            const int m1 = (int)(reinterpret_cast<size_t>(g1 + (size_t)qy * f.pitch[1]) & 15);
            if (FMT == DN_FRAME_NV12) {
                cu = l1 + qy * F::S1 + m1 + 2 * qx;
                cv = cu + 1;
            } else {
                const int m2 = (int)(reinterpret_cast<size_t>(g2 + (size_t)qy * f.pitch[2]) & 15);
                cu = l1 + qy * F::S1 + m1 + qx;
                cv = l2 + qy * F::S1 + m2 + qx;
            }
        }
        int v[3][4];                      // RGB: [memory byte][pixel]; YUV: [0][pixel] luma, [1][0] U, [2][0] V
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            v[0][p] = v[1][p] = v[2][p] = 0;
            if (in[p]) {
                v[0][p] = at[p][0];
                if (RGB) { v[1][p] = at[p][1]; v[2][p] = at[p][2]; }
            }
        }
        if (!RGB && in[0]) { v[1][0] = *cu; v[2][0] = *cv; }

        bool have_pyr = false;

        // the primitives, 256 at a time: cull against the tile in order, then apply
        for (int first = 0; first < n_prim; first += OS_NT) {
            const int idx = first + t;
            OsdPrim pr;
            bool hit = false;
            if (idx < n_prim) {
                pr = first == 0 ? pr_first : prims[idx];
                int x0 = pr.x0, y0 = pr.y0, x1 = pr.x1, y1 = pr.y1;
                bool live = true;
                if (pr.type == OS_SEG)
                    live = os_seg_box(__int_as_float(pr.x0), __int_as_float(pr.y0), __int_as_float(pr.x1), __int_as_float(pr.y1),
                                      __uint_as_float(pr.extra), W, H, x0, y0, x1, y1);
                hit = live && x0 < X0 + tw && x1 > X0 && y0 < Y0 + th && y1 > Y0;
            }
            int n_hit;
            const int pos = os_scan(hit ? 1 : 0, wtot, n_hit);
            if (hit) {
                lp[pos] = pr;
                if (pr.type == OS_LABEL) {         // the label's bytes come along: the glyph lookup then stays in LDS
                    const uint4* const src = reinterpret_cast<const uint4*>(a.text + ((size_t)b * a.d + (pr.extra < (uint32_t)a.d ? pr.extra : 0u)) * 32);
                    ltext[2 * pos] = src[0];
                    ltext[2 * pos + 1] = src[1];
                }
            }
            const int need_pyr = __syncthreads_or(hit && pr.type == OS_BOX && ((pr.extra >> 16) & 255) != 0);
            // the block sums of the snapshot: 8 x 8 cells of 4 x 4 pixels (2 x 2 chroma samples), then the 4 x 4, 2 x 2 and 1 coarser levels
            if (need_pyr && !have_pyr) {
                if (t < 192) {
                    const int ch = t >> 6, cell = t & 63, cx = cell & 7, cy = cell >> 3;
                    int sum = 0;
                    if (RGB || ch == 0) {
                        for (int y = 4 * cy; y < min(4 * cy + 4, th); ++y) {
                            const int mis = (int)(reinterpret_cast<size_t>(g0 + (size_t)y * f.pitch[0]) & 15);
                            const uint8_t* const r = l0 + y * F::S0 + mis;
                            for (int x = 4 * cx; x < min(4 * cx + 4, tw); ++x) sum += RGB ? r[3 * x + ch] : r[x];
                        }
                    } else {
                        const bool second = FMT == DN_FRAME_I420 && ch == 2;
                        uint8_t* const gp = second ? g2 : g1;
                        const size_t cp = second ? f.pitch[2] : f.pitch[1];
                        for (int y = 2 * cy; y < min(2 * cy + 2, chh); ++y) {
                            const int mis = (int)(reinterpret_cast<size_t>(gp + (size_t)y * cp) & 15);
                            const uint8_t* const r = (second ? l2 : l1) + y * F::S1 + mis;
                            for (int x = 2 * cx; x < min(2 * cx + 2, cw); ++x) sum += FMT == DN_FRAME_NV12 ? r[2 * x + ch - 1] : r[x];
                        }
                    }
                    pyr[ch][cell] = sum;
                }
                __syncthreads();
                // each coarser level from the four entries below it: 16, 4 and 1 entries per channel
                for (int lvl = 1; lvl < 4; ++lvl) {
                    const int side = 8 >> lvl, from = lvl == 1 ? 0 : (lvl == 2 ? 64 : 80), to = lvl == 1 ? 64 : (lvl == 2 ? 80 : 84);
                    if (t < 3 * side * side) {
                        const int ch = t / (side * side), e = t - ch * side * side, bx = e % side, by = e / side;
                        const int* const src = &pyr[ch][from + 2 * by * 2 * side + 2 * bx];
                        pyr[ch][to + e] = src[0] + src[1] + src[2 * side] + src[2 * side + 1];
                    }
                    __syncthreads();
                }
                have_pyr = true;
            }
            for (int i = 0; i < n_hit; ++i) {
                const OsdPrim q = lp[i];
                const int c0 = q.col & 255, c1 = (q.col >> 8) & 255, c2 = (q.col >> 16) & 255;
                if (q.type == OS_SEG) {
                    const float ax = __int_as_float(q.x0), ay = __int_as_float(q.y0), bx = __int_as_float(q.x1), by = __int_as_float(q.y1);
                    const float r = __uint_as_float(q.extra);
                    const float dx = bx - ax, dy = by - ay;
                    const float L = dx * dx + dy * dy;
                    const float rr = r * r;
                    const int al = (int)q.txt;
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const float px = (float)(X0 + lx + (p & 1)) + 0.5f, py = (float)(Y0 + ly + (p >> 1)) + 0.5f;
                        const float ux = px - ax, uy = py - ay;
                        const float m0 = ux * dx, m1 = uy * dy;
                        const float tt = fminf(fmaxf((m0 + m1) / L, 0.f), 1.f);
                        const float sx = tt * dx, sy = tt * dy;
                        const float ex = px - (ax + sx), ey = py - (ay + sy);
                        const float e0 = ex * ex, e1 = ey * ey;
                        if (in[p] && e0 + e1 <= rr) {
                            if (RGB) {
                                v[0][p] = os_blend(al, FMT == DN_FRAME_BGR24 ? c2 : c0, v[0][p]);
                                v[1][p] = os_blend(al, c1, v[1][p]);
                                v[2][p] = os_blend(al, FMT == DN_FRAME_BGR24 ? c0 : c2, v[2][p]);
                            } else {
                                v[0][p] = os_blend(al, c0, v[0][p]);
                                if (p == 0) { v[1][0] = os_blend(al, c1, v[1][0]); v[2][0] = os_blend(al, c2, v[2][0]); }
                            }
                        }
                    }
                } else if (q.type == OS_BOX) {
                    const int thick = q.extra & 255, fa = (q.extra >> 8) & 255, block = (q.extra >> 16) & 255;
                    const int sx0 = q.x0 + thick, sy0 = q.y0 + thick, sx1 = q.x1 - thick, sy1 = q.y1 - thick;
                    const bool whole = sx0 >= sx1 || sy0 >= sy1;
                    const int lvl = block == 4 ? 0 : (block == 8 ? 1 : (block == 16 ? 2 : 3));
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const int px = lx + (p & 1), py = ly + (p >> 1);
                        const int x = X0 + px, y = Y0 + py;
                        if (!(in[p] && x >= q.x0 && x < q.x1 && y >= q.y0 && y < q.y1)) continue;
                        if (block) {
                            const int e = os_pyr_index(lvl, px, py);
                            const int fx = (x >> (2 + lvl)) << (2 + lvl), fy = (y >> (2 + lvl)) << (2 + lvl);
                            const int cnt = min(block, W - fx) * min(block, H - fy);
                            v[0][p] = (pyr[0][e] + cnt / 2) / cnt;
                            if (RGB) {
                                v[1][p] = (pyr[1][e] + cnt / 2) / cnt;
                                v[2][p] = (pyr[2][e] + cnt / 2) / cnt;
                            } else if (p == 0) {
                                const int hb = block >> 1;
                                const int cfx = ((x >> 1) / hb) * hb, cfy = ((y >> 1) / hb) * hb;
                                const int cc = min(hb, ((W + 1) >> 1) - cfx) * min(hb, ((H + 1) >> 1) - cfy);
                                v[1][0] = (pyr[1][e] + cc / 2) / cc;
                                v[2][0] = (pyr[2][e] + cc / 2) / cc;
                            }
                        }
                        if (fa) {
                            if (RGB) {
                                v[0][p] = os_blend(fa, FMT == DN_FRAME_BGR24 ? c2 : c0, v[0][p]);
                                v[1][p] = os_blend(fa, c1, v[1][p]);
                                v[2][p] = os_blend(fa, FMT == DN_FRAME_BGR24 ? c0 : c2, v[2][p]);
                            } else {
                                v[0][p] = os_blend(fa, c0, v[0][p]);
                                if (p == 0) { v[1][0] = os_blend(fa, c1, v[1][0]); v[2][0] = os_blend(fa, c2, v[2][0]); }
                            }
                        }
                        if (thick && (whole || !(x >= sx0 && x < sx1 && y >= sy0 && y < sy1))) {
                            if (RGB) {
                                v[0][p] = FMT == DN_FRAME_BGR24 ? c2 : c0;
                                v[1][p] = c1;
                                v[2][p] = FMT == DN_FRAME_BGR24 ? c0 : c2;
                            } else {
                                v[0][p] = c0;
                                if (p == 0) { v[1][0] = c1; v[2][0] = c2; }
                            }
                        }
                    }
                } else {
                    const int k = a.scale, al = a.label_alpha;
                    const int t0 = q.txt & 255, t1 = (q.txt >> 8) & 255, t2 = (q.txt >> 16) & 255;
                    const uint8_t* const text = reinterpret_cast<const uint8_t*>(&ltext[2 * i]);
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const int x = X0 + lx + (p & 1), y = Y0 + ly + (p >> 1);
                        if (!(in[p] && x >= q.x0 && x < q.x1 && y >= q.y0 && y < q.y1)) continue;
                        const int col = (x - q.x0) / k, row = ((y - q.y0) / k) & 7;
                        int g = text[(col >> 3) & 31];
                        if (g >= 'a' && g <= 'z') g -= 32;
                        if (g < 32 || g > 95) g = '?';
                        const bool on = (font[(g - 32) * 8 + row] >> (7 - (col & 7))) & 1;
                        const int d0 = on ? t0 : c0, d1 = on ? t1 : c1, d2 = on ? t2 : c2;
                        if (RGB) {
                            v[0][p] = os_blend(al, FMT == DN_FRAME_BGR24 ? d2 : d0, v[0][p]);
                            v[1][p] = os_blend(al, d1, v[1][p]);
                            v[2][p] = os_blend(al, FMT == DN_FRAME_BGR24 ? d0 : d2, v[2][p]);
                        } else {
                            v[0][p] = os_blend(al, d0, v[0][p]);
                            if (p == 0) { v[1][0] = os_blend(al, d1, v[1][0]); v[2][0] = os_blend(al, d2, v[2][0]); }
                        }
                    }
                }
            }
            __syncthreads();
        }

        // back through LDS (the pyramid has been read; nobody reads the snapshot any more), and out
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (in[p]) {
                at[p][0] = (uint8_t)v[0][p];
                if (RGB) { at[p][1] = (uint8_t)v[1][p]; at[p][2] = (uint8_t)v[2][p]; }
            }
        if (!RGB && in[0]) { *cu = (uint8_t)v[1][0]; *cv = (uint8_t)v[2][0]; }
        __syncthreads();
        os_copy<true>(g0, f.pitch[0], th, nb0, l0, F::S0);
        if (!RGB) {
            os_copy<true>(g1, f.pitch[1], chh, nb1, l1, F::S1);
            if (FMT == DN_FRAME_I420) os_copy<true>(g2, f.pitch[2], chh, nb1, l2, F::S1);
        }
        __syncthreads();
    }
    // The counter goes back to zero for the next call without a memset node: every workgroup has read it before it arrives here, so the last one
    // to arrive may clear it; word 2 keeps the call's count for the caller.
    if (t == 0) {
        __threadfence();
        if (atomicAdd(a.counter + 3, 1) == (int)gridDim.x - 1) {
            a.counter[2] = marked > 0x7fffffffull ? 0x7fffffff : (int)marked;
            a.counter[3] = 0;
            a.counter[1] = 0;
            a.counter[0] = 0;
        }
    }
}

inline bool os_sizes_supported(int streams, int d) { return streams <= OS_MAX_STREAMS && d <= OS_MAX_D; }
inline bool os_style_ok(const dn_osd_style& s) {
    return s.thickness <= 16 && (s.pixelate == 0 || s.pixelate == 4 || s.pixelate == 8 || s.pixelate == 16 || s.pixelate == 32) &&
           (s.flags & ~(DN_OSD_LABEL | DN_OSD_SCORE | DN_OSD_HIDE)) == 0 && s.reserved[0] == 0 && s.reserved[1] == 0 && s.reserved[2] == 0 &&
           s.reserved[3] == 0;
}
inline size_t os_addr(const void* p) { return reinterpret_cast<size_t>(p); }

}  // namespace

extern "C" __attribute__((visibility("default"))) size_t dn_osd_workspace_bytes(int streams, int d, int tile_capacity) {
    if (streams < 1 || d < 1 || tile_capacity < 0 || !os_sizes_supported(streams, d)) return 0;
    return os_list_offset(streams, d) + (size_t)tile_capacity * 8;
}

extern "C" __attribute__((visibility("default"))) int dn_osd_paint(const dn_frame* frames, int n, int format, const float* boxes, const float* scores,
                                                                  const int64_t* labels, const int64_t* ids, const int32_t* counts, int d,
                                                                  const dn_osd_style* styles, int n_labels, const uint8_t* names,
                                                                  const dn_osd_color* palette, const uint8_t* font, const dn_zone_config* zones,
                                                                  const dn_osd_params* params, void* workspace, size_t workspace_bytes,
                                                                  int32_t* stats, void* stream) {
    DN_REQUIRE(frames && boxes && scores && labels && counts && palette && font && params && workspace && stats, "dn_osd_paint: null argument");
    const dn_osd_params p = *params;
    DN_REQUIRE(names || (!styles && !(p.default_style.flags & DN_OSD_LABEL)), "dn_osd_paint: labels need the name table");
    DN_REQUIRE(n >= 1 && d >= 1 && n_labels >= 1, "dn_osd_paint: bad sizes n=%d d=%d n_labels=%d", n, d, n_labels);
    DN_REQUIRE(format == DN_FRAME_NV12 || format == DN_FRAME_I420 || format == DN_FRAME_RGB24 || format == DN_FRAME_BGR24,
               "dn_osd_paint: unknown format %d", format);
    DN_REQUIRE(p.scale >= 1 && p.scale <= 4, "dn_osd_paint: scale=%d, it takes 1 .. 4", p.scale);
    DN_REQUIRE(p.line_thickness >= 1 && p.line_thickness <= 64 && p.zone_thickness >= 1 && p.zone_thickness <= 64,
               "dn_osd_paint: line_thickness=%d and zone_thickness=%d take 1 .. 64", p.line_thickness, p.zone_thickness);
    DN_REQUIRE(os_style_ok(p.default_style), "dn_osd_paint: the default style: thickness 0 .. 16, block 0, 4, 8, 16 or 32, known flags, reserved bytes 0");
    DN_REQUIRE(p.n_colors >= 1 && p.n_colors <= 256, "dn_osd_paint: n_colors=%d, it takes 1 .. 256", p.n_colors);
    DN_REQUIRE(p.label_alpha >= 0 && p.label_alpha <= 255 && p.zone_alpha >= 0 && p.zone_alpha <= 255 && (p.color_by_id == 0 || p.color_by_id == 1),
               "dn_osd_paint: label_alpha=%d and zone_alpha=%d take 0 .. 255, color_by_id=%d 0 or 1", p.label_alpha, p.zone_alpha, p.color_by_id);
    DN_REQUIRE(p.reserved0 == 0 && p.reserved1 == 0 && p.reserved[0] == 0 && p.reserved[1] == 0 && p.reserved[2] == 0 && p.reserved[3] == 0 &&
               p.reserved[4] == 0, "dn_osd_paint: the reserved words must be 0");
    DN_REQUIRE(((os_addr(boxes) | os_addr(workspace) | os_addr(stats) | os_addr(zones)) & 15) == 0 &&
               ((os_addr(labels) | os_addr(ids) | os_addr(styles) | os_addr(palette) | os_addr(frames)) & 7) == 0 &&
               ((os_addr(scores) | os_addr(counts)) & 3) == 0,
               "dn_osd_paint: boxes, workspace, stats and the zone config must be 16-byte aligned, labels, ids, styles and palette 8-byte, scores and counts "
               "4-byte");
    if (!os_sizes_supported(n, d)) {
        dn_set_error("dn_osd_paint: n=%d at most %d, d=%d at most %d", n, OS_MAX_STREAMS, d, OS_MAX_D);
        return DN_E_UNSUPPORTED;
    }
    const size_t fixed = dn_osd_workspace_bytes(n, d, 0);
    if (workspace_bytes < fixed + 8) {
        dn_set_error("dn_osd_paint: workspace of %zu B, at least %zu B needed", workspace_bytes, fixed + 8);
        return DN_E_WORKSPACE;
    }
    const size_t room = (workspace_bytes - fixed) / 8;
    const int capacity = room > (size_t)0x7fffffff ? 0x7fffffff : (int)room;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint8_t* const ws = reinterpret_cast<uint8_t*>(workspace);

    OsdPlanArgs pa;
    pa.frames = frames;
    pa.boxes = reinterpret_cast<const float4*>(boxes);
    pa.scores = scores; pa.labels = labels; pa.ids = ids; pa.counts = counts;
    pa.styles = styles; pa.names = names; pa.palette = palette; pa.zones = zones;
    pa.counter = reinterpret_cast<int32_t*>(ws);
    pa.info = reinterpret_cast<int4*>(ws + os_info_offset());
    pa.prims = reinterpret_cast<OsdPrim*>(ws + os_prim_offset(n));
    pa.text = ws + os_text_offset(n, d);
    pa.list = reinterpret_cast<int2*>(ws + fixed);
    pa.stats = reinterpret_cast<int4*>(stats);
    pa.d = d; pa.n_labels = n_labels; pa.n_colors = p.n_colors; pa.color_by_id = p.color_by_id; pa.scale = p.scale; pa.capacity = capacity;
    pa.def = p.default_style;
    pa.line_col = p.line_color[0] | p.line_color[1] << 8 | p.line_color[2] << 16;
    pa.zone_col = p.zone_color[0] | p.zone_color[1] << 8 | p.zone_color[2] << 16;
    pa.zone_alpha = (uint32_t)p.zone_alpha;
    pa.line_r = (float)p.line_thickness * 0.5f;
    pa.zone_r = (float)p.zone_thickness * 0.5f;
    hipLaunchKernelGGL(osd_plan_kernel, dim3(n), dim3(OS_NT), 0, s, pa);
    DN_HIP_CHECK(hipGetLastError());

    OsdPaintArgs ga;
    ga.frames = frames;
    ga.counter = pa.counter; ga.info = pa.info; ga.prims = pa.prims; ga.text = pa.text; ga.list = pa.list;
    ga.font = font;
    ga.d = d; ga.pmax = os_pmax(d); ga.capacity = capacity; ga.scale = p.scale; ga.label_alpha = p.label_alpha;
    const dim3 grid(capacity < OS_GRID ? capacity : OS_GRID);
    dn_note_kernel("osd_paint_kernel<%d>", format);
    switch (format) {
        case DN_FRAME_NV12: hipLaunchKernelGGL((osd_paint_kernel<DN_FRAME_NV12>), grid, dim3(OS_NT), 0, s, ga); break;
        case DN_FRAME_I420: hipLaunchKernelGGL((osd_paint_kernel<DN_FRAME_I420>), grid, dim3(OS_NT), 0, s, ga); break;
        case DN_FRAME_RGB24: hipLaunchKernelGGL((osd_paint_kernel<DN_FRAME_RGB24>), grid, dim3(OS_NT), 0, s, ga); break;
        default: hipLaunchKernelGGL((osd_paint_kernel<DN_FRAME_BGR24>), grid, dim3(OS_NT), 0, s, ga); break;
    }
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}
