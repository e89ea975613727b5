// Baseline JPEG encoding of surface rectangles on the device: dn_jpeg_encode turns rectangles of the surfaces of a dn_frame table into
// complete JFIF files in one byte arena, dn_jpeg_items_from_index writes its item table from an object cropper's index table. The rules are in
// include/demonet_hip.h and restated in tests/jpeg_ref.py; this file must agree with them byte for byte. Integers only.
//   Three launches. jpeg_rows_kernel<.., false> codes every MCU row (one restart interval) for its exact stuffed byte length; jpeg_scan_kernel, one
//   workgroup, turns row lengths into row offsets inside each file and file lengths into offsets, results and totals; jpeg_rows_kernel<.., true> codes
//   every row again and stores it at its final place, the first row of a file with the 613 header bytes. Nothing is kept between the two codings
//   but 4 bytes per row, so no buffer is sized by a guessed compression ratio.
//   A row is coded by one wave (a workgroup of 64 threads; persistent workgroups stride over the work list). A lane owns one 8 x 8 BLOCK: ten MCUs of
//   six blocks make a group of 60 lanes in stream order. Per group: gather and level shift (the plane-wise path in 8- and 16-byte loads where the row
//   piece is aligned and inside the plane), the transform in 64 registers, the quantiser by a multiply-high with the row's tables (made from the
//   item's quality in LDS), the quantised block to LDS, the DC predictions by wave shuffles, the block's bit length from a first walk in zigzag order,
//   a wave prefix scan of the lengths, a second walk that ORs every code word into a zeroed LDS window (32-bit integer OR atomics: commutative, hence
//   deterministic), and a byte pass that counts 0xFF bytes by ballot and stores the stuffed bytes, 64 consecutive bytes per step. The bits that do
//   not fill a byte are carried into the next group's window.
// The item table is trusted (the header says how far); the index table of dn_jpeg_items_from_index is not.
#include "common.h"
#include "frametap.h"

namespace {

constexpr int JP_NT = 64;
constexpr int JP_GROUP_MCUS = 10;
constexpr int JP_GROUP_BLOCKS = 6 * JP_GROUP_MCUS;
constexpr int JP_BLOCK_MAX_BITS = (11 + 11) + 63 * (16 + 10);              // the longest DC code + 11 value bits, 63 AC codes of 16 + 10 bits
constexpr int JP_WIN_WORDS = (7 + JP_GROUP_BLOCKS * JP_BLOCK_MAX_BITS + 31) / 32 + 2;
constexpr int JP_GRID = 2048;
constexpr int JP_HEAD = DN_JPEG_HEADER_BYTES;
constexpr int JP_SCAN_NT = 256;
static_assert(sizeof(dn_jpeg_item) == 32 && sizeof(dn_jpeg_header) == 16, "the header pins these sizes");

// ---------------------------------------------------------------------------------------------------------------- T.81 Annex K, at compile time
struct JpTables {
    uint32_t dc[2][16];           // by category: length << 16 | code
    uint32_t ac[2][256];          // by run << 4 | category
    int32_t zz[64];               // natural index of zigzag position k
    int32_t base[2][64];          // the quantisation tables at quality 50, natural order
    uint8_t head[JP_HEAD + 3];    // the bytes in front of the data; the Q values, the sizes and DRI are patched per file
};

constexpr uint8_t JP_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t JP_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t JP_AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr uint8_t JP_ZIGZAG[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57,
                                   50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint8_t JP_Q_LUMA[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t JP_Q_CHROMA_HEAD[32] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99};

// offsets inside the header bytes (tests/jpeg_ref.py, header())
constexpr int JP_AT_QL = 25, JP_AT_QC = 90, JP_AT_SIZE = 159, JP_AT_DRI = 597;

constexpr JpTables jp_make_tables() {
    JpTables t{};
    for (int c = 0; c < 2; ++c) {
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < JP_DC_BITS[c][len - 1]; ++i) t.dc[c][k++] = (uint32_t)len << 16 | code++;      // the DC values are 0 .. 11 in order
            code <<= 1;
        }
        code = 0;
        k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < JP_AC_BITS[c][len - 1]; ++i) t.ac[c][JP_AC_VALS[c][k++]] = (uint32_t)len << 16 | code++;
            code <<= 1;
        }
    }
    for (int k = 0; k < 64; ++k) {
        t.zz[k] = JP_ZIGZAG[k];
        t.base[0][k] = JP_Q_LUMA[k];
        t.base[1][k] = k < 32 ? JP_Q_CHROMA_HEAD[k] : 99;
    }
    int n = 0;
    auto put = [&](int v) { t.head[n++] = (uint8_t)v; };
    put(0xFF); put(0xD8);
    put(0xFF); put(0xE0); put(0); put(16); put('J'); put('F'); put('I'); put('F'); put(0); put(1); put(1); put(0); put(0); put(1); put(0); put(1); put(0); put(0);
    put(0xFF); put(0xDB); put(0); put(2 + 65 * 2);
    put(0); for (int k = 0; k < 64; ++k) put(0);
    put(1); for (int k = 0; k < 64; ++k) put(0);
    put(0xFF); put(0xC0); put(0); put(17); put(8); put(0); put(0); put(0); put(0); put(3); put(1); put(0x22); put(0); put(2); put(0x11); put(1); put(3); put(0x11); put(1);
    put(0xFF); put(0xC4); put((2 + 2 * (17 + 12) + 2 * (17 + 162)) >> 8); put((2 + 2 * (17 + 12) + 2 * (17 + 162)) & 255);
    for (int c = 0; c < 2; ++c) {
        put(0x00 | c); for (int i = 0; i < 16; ++i) put(JP_DC_BITS[c][i]);
        for (int i = 0; i < 12; ++i) put(i);
        put(0x10 | c); for (int i = 0; i < 16; ++i) put(JP_AC_BITS[c][i]);
        for (int i = 0; i < 162; ++i) put(JP_AC_VALS[c][i]);
    }
    put(0xFF); put(0xDD); put(0); put(4); put(0); put(0);
    put(0xFF); put(0xDA); put(0); put(12); put(3); put(1); put(0x00); put(2); put(0x11); put(3); put(0x11); put(0); put(0x3F); put(0);
    t.head[JP_HEAD] = (uint8_t)(n == JP_HEAD);          // (checked below)
    return t;
}
constexpr JpTables JP_HOST_TABLES = jp_make_tables();
static_assert(JP_HOST_TABLES.head[JP_HEAD] == 1 && JP_HOST_TABLES.head[JP_AT_QL - 1] == 0 && JP_HOST_TABLES.head[JP_AT_QC - 1] == 1 &&
              JP_HOST_TABLES.head[JP_AT_SIZE - 1] == 8 && JP_HOST_TABLES.head[JP_AT_DRI - 1] == 4, "the header template");
__constant__ JpTables JP_TABLES = jp_make_tables();

// ---------------------------------------------------------------------------------------------------------------- arguments
struct JpArgs {
    const dn_frame* frames;
    const dn_jpeg_header* table;
    int capacity;
    uint8_t* arena;
    int arena_bytes;
    int32_t* results;
    int32_t* totals;
    long long* file_len;        // workspace: [capacity]; the file length, or the negative status of a slot without a file
    int32_t* row;               // workspace: [segcap]; the stuffed bytes of a row, then (jpeg_scan_kernel) its offset behind the file's header
    int segcap;
    FrameColor k;
};

// the BT.601 full-range forward matrix, round(c 2^14): compose.hip's cp_forward(DN_COLOR_BT601 | DN_COLOR_FULL_RANGE)
__device__ __forceinline__ int jp_y(int r, int g, int b) { return frame_clamp8((4899 * r + 9617 * g + 1868 * b + (1 << 13)) >> 14); }
__device__ __forceinline__ int jp_cb(int r, int g, int b) { return frame_clamp8(((-2765 * r - 5427 * g + 8192 * b + (1 << 13)) >> 14) + 128); }
__device__ __forceinline__ int jp_cr(int r, int g, int b) { return frame_clamp8(((8192 * r - 6860 * g - 1332 * b + (1 << 13)) >> 14) + 128); }

__device__ __forceinline__ int jp_items(const JpArgs& a) {
    const int n = a.table->n_items;
    return n < 0 ? 0 : (n > a.capacity ? a.capacity : n);
}
__device__ __forceinline__ int jp_segments(const JpArgs& a) {
    const int n = a.table->n_segments;
    return n < 0 ? 0 : (n > a.segcap ? a.segcap : n);
}
__device__ __forceinline__ int jp_rows(const dn_jpeg_item& I) { return I.frame >= 0 && I.height >= 1 && I.width >= 1 ? (I.height + 15) >> 4 : 0; }

// the item of work-list row s: the last one whose seg0 <= s; -1 when s is not one of its rows
__device__ __forceinline__ int jp_find(const dn_jpeg_item* items, int n_items, int n_seg, int s, dn_jpeg_item& I, int& r) {
    int lo = 0, hi = n_items - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].seg0 <= s) lo = mid;
        else hi = mid - 1;
    }
    I = items[lo];
    r = s - I.seg0;
    const int rows = jp_rows(I);
    return r >= 0 && r < rows && I.seg0 >= 0 && I.seg0 <= n_seg - rows ? lo : -1;
}

// ---------------------------------------------------------------------------------------------------------------- the transform
constexpr int JP_CONST_BITS = 13, JP_PASS1_BITS = 2;
__device__ __forceinline__ int jp_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }      // >> of a signed int: arithmetic (floor)

// one 1-D pass of the Loeffler-Ligtenberg-Moschytz transform; the constants are round(c 2^13) of tests/jpeg_ref.py's closed forms
template <bool FIRST>
__device__ __forceinline__ void jp_dct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
    const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int N = FIRST ? JP_CONST_BITS - JP_PASS1_BITS : JP_CONST_BITS + JP_PASS1_BITS;
    if (FIRST) {
        d0 = (t10 + t11) * (1 << JP_PASS1_BITS);
        d4 = (t10 - t11) * (1 << JP_PASS1_BITS);
    } else {
        d0 = jp_descale(t10 + t11, JP_PASS1_BITS);
        d4 = jp_descale(t10 - t11, JP_PASS1_BITS);
    }
    int z1 = (t12 + t13) * 4433;
    d2 = jp_descale(z1 + t13 * 6270, N);
    d6 = jp_descale(z1 - t12 * 15137, N);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
    z1 = -z1 * 7373;
    z2 = -z2 * 20995;
    z3 = -z3 * 16069 + z5;
    z4 = -z4 * 3196 + z5;
    d7 = jp_descale(u4 + z1 + z3, N);
    d5 = jp_descale(u5 + z2 + z4, N);
    d3 = jp_descale(u6 + z2 + z3, N);
    d1 = jp_descale(u7 + z1 + z4, N);
}

// ---------------------------------------------------------------------------------------------------------------- the samples of a block
// channel c (0: Y, 1: Cb, 2: Cr) of a 4:2:0 frame as a sample grid
template <int FMT>
__device__ __forceinline__ void jp_channel(const dn_frame& f, int c, const uint8_t*& base, int& pitch, int& step) {
    const uint8_t* const p0 = f.plane[0];                 // (no indexed access and no address of the record: it stays in registers)
    const uint8_t* const p1 = f.plane[1];
    const uint8_t* const p2 = FMT == DN_FRAME_NV12 ? p1 : f.plane[2];
    const int s0 = f.pitch[0], s1 = f.pitch[1], s2 = FMT == DN_FRAME_NV12 ? s1 : f.pitch[2];
    base = c == 0 ? p0 : (FMT == DN_FRAME_NV12 ? p1 + (c - 1) : (c == 1 ? p1 : p2));
    pitch = c == 0 ? s0 : (c == 1 ? s1 : s2);
    step = FMT == DN_FRAME_NV12 && c != 0 ? 2 : 1;
}

// Block b (0 .. 3: Y, 4: Cb, 5: Cr) of MCU (m, r) of the item, level shifted; samples beyond the component plane replicate its last column and row.
// stage: the lane's column of the coefficient array in LDS (element e at stage[e * JP_NT]), free at this point
template <int FMT, bool PLANES>
__device__ __forceinline__ void jp_gather(const dn_frame& f, const dn_jpeg_item& I, const FrameColor& k, int m, int r, int b, int16_t* stage, int (&v)[64]) {
    const bool luma = b < 4;
    const int pw = luma ? I.width : (I.width + 1) >> 1, ph = luma ? I.height : (I.height + 1) >> 1;      // the component plane
    const int px0 = luma ? m * 16 + (b & 1) * 8 : m * 8, py0 = luma ? r * 16 + (b >> 1) * 8 : r * 8;
    if (PLANES) {
        const uint8_t* base;
        int pitch, step;
        jp_channel<FMT>(f, luma ? 0 : b - 3, base, pitch, step);
        const int ox = luma ? I.x0 : I.x0 >> 1, oy = luma ? I.y0 : I.y0 >> 1;
        const bool inside = px0 + 8 <= pw;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int y = min(py0 + j, ph - 1);
            const uint8_t* const row = base + (size_t)(oy + y) * pitch + (size_t)ox * step;
            const uint8_t* const p = row + (size_t)px0 * step;
            if (inside && step == 1 && (reinterpret_cast<size_t>(p) & 7) == 0) {
                const uint2 w = *reinterpret_cast<const uint2*>(p);
#pragma unroll
                for (int i = 0; i < 8; ++i) v[j * 8 + i] = (int)(((i < 4 ? w.x : w.y) >> (8 * (i & 3))) & 255) - 128;
            } else if (inside && step == 2 && (reinterpret_cast<size_t>(p - (b - 4)) & 15) == 0) {
                const uint4 w = *reinterpret_cast<const uint4*>(p - (b - 4));          // eight UV pairs: byte 2 i + (b - 4) is sample i
                const uint32_t q[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (int i = 0; i < 8; ++i) v[j * 8 + i] = (int)((q[i >> 1] >> (16 * (i & 1) + 8 * (b - 4))) & 255) - 128;
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[j * 8 + i] = (int)row[(size_t)min(px0 + i, pw - 1) * step] - 128;
            }
        }
    } else {
        // one sample at a time through the lane's LDS column (a rolled loop: 64 inlined conversions per path would be most of the kernel's code)
#pragma unroll 1
        for (int e = 0; e < 64; ++e) {
            const int j = e >> 3, i = e & 7;
            int val;
            if (luma) {
                int r8, g8, b8;
                frame_tap_rgb8<FMT>(f, I.x0 + min(px0 + i, pw - 1), I.y0 + min(py0 + j, ph - 1), k, r8, g8, b8);
                val = jp_y(r8, g8, b8);
            } else {
                // a chroma sample: the mean, rounded half up, of the pixels of its 2 x 2 block of the rectangle that lie inside the rectangle (1, 2 or 4)
                const int cx = min(px0 + i, pw - 1), cy = min(py0 + j, ph - 1);
                const bool two_x = 2 * cx + 1 < I.width, two_y = 2 * cy + 1 < I.height;
                const int X = I.x0 + 2 * cx, Y = I.y0 + 2 * cy;
                int sr, sg, sb, r8, g8, b8, shift = 0;
                frame_tap_rgb8<FMT>(f, X, Y, k, sr, sg, sb);
                if (two_x) { frame_tap_rgb8<FMT>(f, X + 1, Y, k, r8, g8, b8); sr += r8; sg += g8; sb += b8; ++shift; }
                if (two_y) {
                    frame_tap_rgb8<FMT>(f, X, Y + 1, k, r8, g8, b8); sr += r8; sg += g8; sb += b8; ++shift;
                    if (two_x) { frame_tap_rgb8<FMT>(f, X + 1, Y + 1, k, r8, g8, b8); sr += r8; sg += g8; sb += b8; }
                }
                const int half = shift ? 1 << (shift - 1) : 0;          // n = 1 << shift pixels: (sum + n / 2) / n
                sr = (sr + half) >> shift; sg = (sg + half) >> shift; sb = (sb + half) >> shift;
                val = b == 4 ? jp_cb(sr, sg, sb) : jp_cr(sr, sg, sb);
            }
            stage[e * JP_NT] = (int16_t)(val - 128);
        }
#pragma unroll
        for (int e = 0; e < 64; ++e) v[e] = stage[e * JP_NT];
    }
}

// ---------------------------------------------------------------------------------------------------------------- bits
__device__ __forceinline__ int jp_category(int v) { return 32 - __clz(v < 0 ? -v : v); }
__device__ __forceinline__ uint32_t jp_value_bits(int v, int cat) { return (uint32_t)(v < 0 ? v + (1 << cat) - 1 : v); }

// n <= 27 bits at bit `pos` of the window, MSB first
__device__ __forceinline__ void jp_put(uint32_t* win, int pos, uint32_t bits, int n) {
    if (n <= 0) return;
    const int w = pos >> 5, o = pos & 31;
    if (w + 1 >= JP_WIN_WORDS) return;                      // (cannot happen: the window holds the longest group)
    const unsigned long long x = (unsigned long long)bits << (64 - o - n);
    atomicOr(&win[w], (uint32_t)(x >> 32));
    if ((uint32_t)x) atomicOr(&win[w + 1], (uint32_t)x);
}

template <bool EMIT>
__device__ __forceinline__ int jp_walk_block(const int16_t* coef, const int* zz, const uint32_t* hdc, const uint32_t* hac, int lane, int diff, uint32_t* win, int pos) {
    int len = 0;
    {
        const int cat = jp_category(diff);
        const uint32_t e = hdc[cat & 15];
        const int n = (int)(e >> 16) + cat;
        if (EMIT) jp_put(win, pos, (e & 0xFFFF) << cat | jp_value_bits(diff, cat), n);
        len += n;
    }
    const uint32_t zrl = hac[0xF0], eob = hac[0x00];
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int c = coef[zz[k] * JP_NT + lane];
        if (c == 0) {
            ++run;
            continue;
        }
        for (; run >= 16; run -= 16) {
            if (EMIT) jp_put(win, pos + len, zrl & 0xFFFF, (int)(zrl >> 16));
            len += (int)(zrl >> 16);
        }
        const int cat = jp_category(c);
        const uint32_t e = hac[(run << 4 | cat) & 255];
        const int n = (int)(e >> 16) + cat;
        if (EMIT) jp_put(win, pos + len, (e & 0xFFFF) << cat | jp_value_bits(c, cat), n);
        len += n;
        run = 0;
    }
    if (run > 0) {
        if (EMIT) jp_put(win, pos + len, eob & 0xFFFF, (int)(eob >> 16));
        len += (int)(eob >> 16);
    }
    return len;
}

__device__ __forceinline__ int jp_wave_inclusive(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    return v;
}

// ---------------------------------------------------------------------------------------------------------------- the rows
template <int FMT, bool PLANES, bool WRITE>
__global__ __launch_bounds__(JP_NT) void jpeg_rows_kernel(const JpArgs a) {
    __shared__ int16_t coef[64 * JP_NT];                  // [natural index][lane]
    __shared__ uint32_t win[JP_WIN_WORDS];
    __shared__ uint32_t hdc[2][16], hac[2][256];
    __shared__ int zz[64];
    __shared__ uint32_t qd[2][64], qm[2][64];             // d = 8 Q and ceil(2^32 / d), natural order
    const int lane = threadIdx.x;
    for (int i = lane; i < 32; i += JP_NT) hdc[i >> 4][i & 15] = JP_TABLES.dc[i >> 4][i & 15];
    for (int i = lane; i < 512; i += JP_NT) hac[i >> 8][i & 255] = JP_TABLES.ac[i >> 8][i & 255];
    zz[lane] = JP_TABLES.zz[lane];
    const dn_jpeg_item* const items = reinterpret_cast<const dn_jpeg_item*>(a.table + 1);
    const int n_items = jp_items(a), n_seg = jp_segments(a);
    if (n_items == 0) return;
    const int mcu_l = lane / 6, b = lane - mcu_l * 6, t = b >= 4 ? 1 : 0;
    int have_q = -1;
    for (int s = blockIdx.x; s < n_seg; s += gridDim.x) {
        dn_jpeg_item I;
        int r;
        const int it = jp_find(items, n_items, n_seg, s, I, r);
        if (it < 0) {
            if (!WRITE) a.row[s] = 0;
            continue;
        }
        uint8_t* dst = nullptr;
        long long room = 0;              // bytes of the arena from dst on
        if (WRITE) {
            if (a.results[4 * it + 2] != 0) continue;
            const long long at = (long long)a.results[4 * it] + JP_HEAD + a.row[s];
            dst = a.arena + at;
            room = (long long)a.arena_bytes - at;
        }
        const int q = min(max(I.quality, 1), 100);
        if (q != have_q) {
            __syncthreads();
            const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int Q = min(max((JP_TABLES.base[c][lane] * scale + 50) / 100, 1), 255);
                qd[c][lane] = 8u * Q;
                qm[c][lane] = 0xFFFFFFFFu / (8u * Q) + 1u;
            }
            have_q = q;
        }
        __syncthreads();
        const dn_frame f = a.frames[I.frame];
        const int rows = (I.height + 15) >> 4, mcus = (I.width + 15) >> 4;
        if (WRITE && r == 0) {
            uint8_t* const head = a.arena + a.results[4 * it];
            for (int i = lane; i < JP_HEAD; i += JP_NT) {
                int byte = JP_TABLES.head[i];
                if (i >= JP_AT_QL && i < JP_AT_QL + 64) byte = (int)(qd[0][zz[i - JP_AT_QL]] >> 3);
                else if (i >= JP_AT_QC && i < JP_AT_QC + 64) byte = (int)(qd[1][zz[i - JP_AT_QC]] >> 3);
                else if (i == JP_AT_SIZE) byte = I.height >> 8;
                else if (i == JP_AT_SIZE + 1) byte = I.height & 255;
                else if (i == JP_AT_SIZE + 2) byte = I.width >> 8;
                else if (i == JP_AT_SIZE + 3) byte = I.width & 255;
                else if (i == JP_AT_DRI) byte = mcus >> 8;
                else if (i == JP_AT_DRI + 1) byte = mcus & 255;
                head[i] = (uint8_t)byte;
            }
        }
        int carry_dc0 = 0, carry_dc1 = 0, carry_dc2 = 0, carry_bits = 0, out = 0;
        uint32_t carry_word = 0;
        for (int m0 = 0; m0 < mcus; m0 += JP_GROUP_MCUS) {
            const int m = m0 + mcu_l;
            const bool active = lane < JP_GROUP_BLOCKS && m < mcus;
            const bool last = m0 + JP_GROUP_MCUS >= mcus;
            int qdc = 0;
            if (active) {
                int v[64];
                jp_gather<FMT, PLANES>(f, I, a.k, m, r, b, coef + lane, v);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    jp_dct8<true>(v[j * 8], v[j * 8 + 1], v[j * 8 + 2], v[j * 8 + 3], v[j * 8 + 4], v[j * 8 + 5], v[j * 8 + 6], v[j * 8 + 7]);
#pragma unroll
                for (int i = 0; i < 8; ++i) jp_dct8<false>(v[i], v[8 + i], v[16 + i], v[24 + i], v[32 + i], v[40 + i], v[48 + i], v[56 + i]);
#pragma unroll
                for (int k = 0; k < 64; ++k) {
                    const int c = v[k];
                    const uint32_t d = qd[t][k];
                    const int mag = (int)__umulhi((uint32_t)(c < 0 ? -c : c) + (d >> 1), qm[t][k]);      // (|c| + d / 2) / d: exact, (|c| + d / 2) d < 2^32
                    const int sq = c < 0 ? -mag : mag;
                    coef[k * JP_NT + lane] = (int16_t)sq;
                    if (k == 0) qdc = sq;
                }
            }
            // the DC prediction: the previous block of the same component in stream order
            const int up1 = __shfl_up(qdc, 1), up3 = __shfl_up(qdc, 3), up6 = __shfl_up(qdc, 6);
            const int pred = b == 0 ? (lane >= 6 ? up3 : carry_dc0) : (b < 4 ? up1 : (lane >= 6 ? up6 : (b == 4 ? carry_dc1 : carry_dc2)));
            carry_dc0 = __shfl(qdc, JP_GROUP_BLOCKS - 3);
            carry_dc1 = __shfl(qdc, JP_GROUP_BLOCKS - 2);
            carry_dc2 = __shfl(qdc, JP_GROUP_BLOCKS - 1);
            const int diff = qdc - pred;
            const int len = active ? jp_walk_block<false>(coef, zz, hdc[t], hac[t], lane, diff, nullptr, 0) : 0;
            const int incl = jp_wave_inclusive(len, lane);
            const int total = carry_bits + __shfl(incl, JP_NT - 1);
            const int words = min((total + 31) >> 5, JP_WIN_WORDS - 1) + 1;
            for (int w = lane; w < words; w += JP_NT) win[w] = w == 0 ? carry_word : 0u;
            __syncthreads();
            if (active) jp_walk_block<true>(coef, zz, hdc[t], hac[t], lane, diff, win, carry_bits + incl - len);
            const int rem = total & 7;
            if (last && rem && lane == 0) jp_put(win, total, (1u << (8 - rem)) - 1u, 8 - rem);          // the row's last byte: 1-bits
            __syncthreads();
            const int nbytes = last ? (total + 7) >> 3 : total >> 3;
            for (int base = 0; base < nbytes; base += JP_NT) {
                const int i = base + lane;
                const bool valid = i < nbytes;
                const uint32_t byte = valid ? (win[i >> 2] >> (24 - 8 * (i & 3))) & 255u : 0u;
                const bool ff = valid && byte == 255u;
                const unsigned long long mask = __ballot(ff);
                if (WRITE && valid) {
                    const long long pos = (long long)out + (i - base) + __popcll(mask & ((1ull << lane) - 1ull));
                    if (pos < room) dst[pos] = (uint8_t)byte;
                    if (ff && pos + 1 < room) dst[pos + 1] = 0;
                }
                out += min(JP_NT, nbytes - base) + __popcll(mask);
            }
            carry_word = last ? 0u : ((win[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 255u) << 24;
            carry_bits = last ? 0 : rem;
            __syncthreads();
        }
        if (!WRITE) {
            if (lane == 0) a.row[s] = out;
        } else if (lane < 2) {
            // RSTm behind every row but the last, EOI behind the last
            const int byte = lane == 0 ? 0xFF : (r < rows - 1 ? 0xD0 + (r & 7) : 0xD9);
            if ((long long)out + lane < room) dst[out + lane] = (uint8_t)byte;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- offsets, results, totals
__global__ __launch_bounds__(JP_SCAN_NT) void jpeg_scan_kernel(const JpArgs a) {
    __shared__ long long part[JP_SCAN_NT];
    __shared__ int s_written, s_refused, s_used;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const dn_jpeg_item* const items = reinterpret_cast<const dn_jpeg_item*>(a.table + 1);
    const int n_items = jp_items(a), n_seg = jp_segments(a);
    if (t == 0) s_written = s_refused = s_used = 0;
    // a wave per item: the rows' lengths (+ 2: the marker behind each) become their offsets behind the file's header
    for (int it = wave; it < a.capacity; it += JP_SCAN_NT / 64) {
        long long flen = -1;               // an empty slot
        if (it < n_items) {
            const dn_jpeg_item I = items[it];
            const int rows = jp_rows(I);
            if (I.frame < 0) flen = I.frame >= -3 ? I.frame : -2;
            else if (rows == 0) flen = -2;
            else if (I.seg0 < 0 || I.seg0 > n_seg - rows) flen = -3;            // its rows lie beyond the work list the workspace holds
            else {
                long long run = 0;
                for (int base = 0; base < rows; base += 64) {
                    const int r = base + lane;
                    const int len = r < rows ? a.row[I.seg0 + r] + 2 : 0;
                    const int incl = jp_wave_inclusive(len, lane);
                    if (r < rows) a.row[I.seg0 + r] = (int32_t)(run + incl - len);
                    run += __shfl(incl, 63);
                }
                flen = JP_HEAD + run;
            }
        }
        if (lane == 0) a.file_len[it] = flen;
    }
    __syncthreads();
    // offset_i: the sum of align16(length_j) over every encodable j < i
    const int per = (a.capacity + JP_SCAN_NT - 1) / JP_SCAN_NT;
    const int i0 = min(t * per, a.capacity), i1 = min(i0 + per, a.capacity);
    long long sum = 0;
    for (int i = i0; i < i1; ++i) {
        const long long n = a.file_len[i];
        if (n >= 0) sum += (n + 15) & ~15ll;
    }
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < JP_SCAN_NT; d <<= 1) {
        const long long u = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += u;
        __syncthreads();
    }
    long long off = part[t] - sum;
    int written = 0, refused = 0, used = 0;
    for (int i = i0; i < i1; ++i) {
        const long long n = a.file_len[i];
        int32_t* const res = a.results + 4 * i;
        if (n < 0) {
            res[0] = 0; res[1] = 0; res[2] = (int32_t)-n; res[3] = 0;
            refused += n != -1;
            continue;
        }
        const bool fits = off + n <= (long long)a.arena_bytes;
        res[0] = (int32_t)(off < 0x7FFFFFFFll ? off : 0x7FFFFFFFll);
        res[1] = fits ? (int32_t)n : 0;
        res[2] = fits ? 0 : 3;
        res[3] = 0;
        if (fits) {
            ++written;
            used = (int)(off + n);
        } else {
            ++refused;
        }
        off += (n + 15) & ~15ll;
    }
    atomicAdd(&s_written, written);
    atomicAdd(&s_refused, refused);
    atomicMax(&s_used, used);
    __syncthreads();
    if (t == 0) {
        a.totals[0] = s_written; a.totals[1] = s_refused; a.totals[2] = s_used; a.totals[3] = 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- dn_jpeg_items_from_index
struct JpIndexArgs {
    const dn_frame* frames;
    int n_frames, yuv;
    const int32_t* index;
    int rows;
    const uint8_t* select;
    int quality, max_segments;
    dn_jpeg_header* table;
};

// the slot's status (0: a file) and, for a file, its rectangle
__device__ __forceinline__ int jp_index_row(const JpIndexArgs& a, int s, dn_jpeg_item& I) {
    const int32_t* const row = a.index + 8 * (size_t)s;
    const int f = row[0];
    int x0 = row[2], y0 = row[3], w = row[4], h = row[5];
    I.frame = -1; I.x0 = I.y0 = I.width = I.height = 0; I.quality = a.quality; I.seg0 = 0; I.reserved = 0;
    if (f == -1 || (a.select && a.select[s] == 0)) return 1;
    if (f < 0 || f >= a.n_frames || w < 1 || h < 1 || w > 32768 || h > 32768 || x0 < 0 || y0 < 0) return 2;
    const int W = a.frames[f].width, H = a.frames[f].height;
    if (x0 > W - w || y0 > H - h) return 2;
    if (a.yuv) {
        w += x0 & 1; h += y0 & 1;
        x0 &= ~1; y0 &= ~1;
    }
    I.frame = f; I.x0 = x0; I.y0 = y0; I.width = w; I.height = h;
    return 0;
}

__global__ __launch_bounds__(JP_SCAN_NT) void jpeg_index_kernel(const JpIndexArgs a) {
    __shared__ int part[JP_SCAN_NT];
    __shared__ int s_total;
    const int t = threadIdx.x;
    const int per = (a.rows + JP_SCAN_NT - 1) / JP_SCAN_NT;
    const int i0 = min(t * per, a.rows), i1 = min(i0 + per, a.rows);
    if (t == 0) s_total = 0;
    int sum = 0;
    for (int s = i0; s < i1; ++s) {
        dn_jpeg_item I;
        if (jp_index_row(a, s, I) == 0) sum += (I.height + 15) >> 4;          // (at most 8192 slots of 2048 rows: inside an int)
    }
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < JP_SCAN_NT; d <<= 1) {
        const int u = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += u;
        __syncthreads();
    }
    int cum = part[t] - sum, accepted = 0;
    dn_jpeg_item* const items = reinterpret_cast<dn_jpeg_item*>(a.table + 1);
    for (int s = i0; s < i1; ++s) {
        dn_jpeg_item I;
        int status = jp_index_row(a, s, I);
        I.seg0 = cum;
        if (status == 0) {
            const int rows = (I.height + 15) >> 4;
            if (cum > a.max_segments - rows) status = 3;
            else accepted = cum + rows;
            cum += rows;
        }
        if (status != 0) {
            I.frame = -status;
            I.x0 = I.y0 = I.width = I.height = 0;
        }
        items[s] = I;
    }
    atomicMax(&s_total, accepted);
    __syncthreads();
    if (t == 0) {
        a.table->n_items = a.rows;
        a.table->n_segments = s_total;
        a.table->reserved[0] = a.table->reserved[1] = 0;
    }
}

inline size_t jp_addr(const void* p) { return reinterpret_cast<size_t>(p); }
inline bool jp_format_ok(int f) { return f == DN_FRAME_NV12 || f == DN_FRAME_I420 || f == DN_FRAME_RGB24 || f == DN_FRAME_BGR24; }
inline bool jp_yuv(int f) { return f == DN_FRAME_NV12 || f == DN_FRAME_I420; }
inline size_t jp_items_bytes(int capacity) { return a256((size_t)capacity * sizeof(long long)); }

template <int FMT, bool PLANES>
void jp_launch(const JpArgs& a, bool write, hipStream_t s) {
    if (write) hipLaunchKernelGGL((jpeg_rows_kernel<FMT, PLANES, true>), dim3(JP_GRID), dim3(JP_NT), 0, s, a);
    else hipLaunchKernelGGL((jpeg_rows_kernel<FMT, PLANES, false>), dim3(JP_GRID), dim3(JP_NT), 0, s, a);
}

void jp_launch_rows(int format, bool planes, const JpArgs& a, bool write, hipStream_t s) {
    if (planes) {
        if (format == DN_FRAME_NV12) jp_launch<DN_FRAME_NV12, true>(a, write, s);
        else jp_launch<DN_FRAME_I420, true>(a, write, s);
        return;
    }
    switch (format) {
        case DN_FRAME_NV12: jp_launch<DN_FRAME_NV12, false>(a, write, s); break;
        case DN_FRAME_I420: jp_launch<DN_FRAME_I420, false>(a, write, s); break;
        case DN_FRAME_RGB24: jp_launch<DN_FRAME_RGB24, false>(a, write, s); break;
        default: jp_launch<DN_FRAME_BGR24, false>(a, write, s); break;
    }
}

}  // namespace

extern "C" __attribute__((visibility("default"))) size_t dn_jpeg_workspace_bytes(int capacity_items, int max_segments) {
    if (capacity_items < 1 || capacity_items > DN_JPEG_MAX_ITEMS || max_segments < 1) return 0;
    return jp_items_bytes(capacity_items) + a256((size_t)max_segments * sizeof(int32_t));
}

extern "C" __attribute__((visibility("default"))) int dn_jpeg_encode(const dn_frame* frames, int format, int color, const dn_jpeg_header* table,
                                                                    int capacity_items, uint8_t* arena, int arena_bytes, int32_t* results,
                                                                    int32_t* totals, void* workspace, size_t workspace_bytes, void* stream) {
    DN_REQUIRE(frames && table && arena && results && totals && workspace, "dn_jpeg_encode: null pointer");
    DN_REQUIRE((jp_addr(frames) & 7) == 0 && ((jp_addr(table) | jp_addr(results) | jp_addr(totals) | jp_addr(workspace)) & 15) == 0,
               "dn_jpeg_encode: the frame table must be 8-byte aligned, the item table, results, totals and the workspace 16-byte");
    DN_REQUIRE(capacity_items >= 1, "dn_jpeg_encode: capacity_items=%d, it takes 1 .. %d", capacity_items, DN_JPEG_MAX_ITEMS);
    DN_REQUIRE(arena_bytes >= 0, "dn_jpeg_encode: arena_bytes=%d", arena_bytes);
    DN_REQUIRE(jp_format_ok(format), "dn_jpeg_encode: unknown format %d", format);
    JpArgs a;
    DN_REQUIRE(frame_color(color, &a.k), "dn_jpeg_encode: unknown colour code %d", color);
    if (capacity_items > DN_JPEG_MAX_ITEMS) {
        dn_set_error("dn_jpeg_encode: capacity_items=%d, at most %d items", capacity_items, DN_JPEG_MAX_ITEMS);
        return DN_E_UNSUPPORTED;
    }
    DN_REQUIRE(workspace_bytes >= dn_jpeg_workspace_bytes(capacity_items, 1), "dn_jpeg_encode: workspace of %zu bytes, dn_jpeg_workspace_bytes(%d, 1) is %zu",
               workspace_bytes, capacity_items, dn_jpeg_workspace_bytes(capacity_items, 1));
    a.frames = frames;
    a.table = table;
    a.capacity = capacity_items;
    a.arena = arena;
    a.arena_bytes = arena_bytes;
    a.results = results;
    a.totals = totals;
    a.file_len = static_cast<long long*>(workspace);
    a.row = reinterpret_cast<int32_t*>(static_cast<uint8_t*>(workspace) + jp_items_bytes(capacity_items));
    const size_t segcap = (workspace_bytes - jp_items_bytes(capacity_items)) / sizeof(int32_t);
    a.segcap = (int)(segcap < 0x7FFFFFFFu ? segcap : 0x7FFFFFFFu);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool planes = jp_yuv(format) && color == (DN_COLOR_BT601 | DN_COLOR_FULL_RANGE);
    dn_note_kernel(planes ? "jpeg_planes_kernel<%d>" : "jpeg_rgb_kernel<%d>", format);
    jp_launch_rows(format, planes, a, false, s);
    DN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(JP_SCAN_NT), 0, s, a);
    DN_HIP_CHECK(hipGetLastError());
    jp_launch_rows(format, planes, a, true, s);
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}

extern "C" __attribute__((visibility("default"))) int dn_jpeg_items_from_index(const dn_frame* frames, int n_frames, int format, const int32_t* index,
                                                                              int index_rows, const uint8_t* select, int quality, int max_segments,
                                                                              dn_jpeg_header* table, void* stream) {
    DN_REQUIRE(frames && index && table, "dn_jpeg_items_from_index: null pointer");
    DN_REQUIRE((jp_addr(frames) & 7) == 0 && ((jp_addr(index) | jp_addr(table)) & 15) == 0,
               "dn_jpeg_items_from_index: the frame table must be 8-byte aligned, the index and item tables 16-byte");
    DN_REQUIRE(n_frames >= 1 && index_rows >= 1 && max_segments >= 1, "dn_jpeg_items_from_index: n_frames=%d index_rows=%d max_segments=%d", n_frames, index_rows,
               max_segments);
    DN_REQUIRE(quality >= 1 && quality <= 100, "dn_jpeg_items_from_index: quality=%d, it takes 1 .. 100", quality);
    DN_REQUIRE(jp_format_ok(format), "dn_jpeg_items_from_index: unknown format %d", format);
    if (index_rows > DN_JPEG_MAX_ITEMS) {
        dn_set_error("dn_jpeg_items_from_index: index_rows=%d, at most %d", index_rows, DN_JPEG_MAX_ITEMS);
        return DN_E_UNSUPPORTED;
    }
    JpIndexArgs a;
    a.frames = frames;
    a.n_frames = n_frames;
    a.yuv = jp_yuv(format) ? 1 : 0;
    a.index = index;
    a.rows = index_rows;
    a.select = select;
    a.quality = quality;
    a.max_segments = max_segments;
    a.table = table;
    dn_note_kernel("jpeg_index_kernel");
    hipLaunchKernelGGL(jpeg_index_kernel, dim3(1), dim3(JP_SCAN_NT), 0, reinterpret_cast<hipStream_t>(stream), a);
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}
