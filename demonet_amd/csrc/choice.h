// Which kernel a 1x1 convolution, a dense convolution, a grouped head launch, a depthwise convolution, the squeeze-excitation FCs, a stem, the soft-NMS reduce or a fused inverted-residual block runs on: ONE pure function per family (no HIP call, no label, argument
// untouched; knobs read through dn_knob at the call -- INTEGRATION.md: kernel-choice knobs at every launch). The launchers validate, ask here and switch from
// the answer to the template instantiation; the plan-time predicates ask the same functions about a shape. The order of the rules in a function is their
// precedence, with the measurement that justifies a rule next to it; capability tests (*_shape, *_supported) stand in front of the function that uses them.
#pragma once
#include <algorithm>

#include "common.h"

struct PwChoice {
    enum Kernel {
        NONE,                                               // no kernel of the family takes the problem
        AS_POINTWISE,                                       // conv_choose: a dense 1x1 that the 1x1 family serves -- pw_choose decides, on conv_1x1_as_pw(a)
        PW_WSTAT, PW_STREAM, PW_DIRECT,                     // pwdirect.hip: pw_wstat_kernel<KS1 = k, RT = t, false>, pw_stream_kernel<KSF = k, PX = t>, pw_direct_kernel<KSF = k, TC = t> (or, proj, its weight-stationary body)
        PW_XS, PW_TILE, PW_GROUP,                           // pointwise.hip: pw_xs_kernel<32>, pw_kernel / pw_group_kernel<bp, bc, .., conv, bk, pf, sef, fk>
        CONV_PATCH, CONV_PATCH_RESIDENT, CONV_HALO, CONV_GLDS   // convbig.hip; conv_halo_kernel<3, TP, TC, head> by halo: 1 = 256 px x 256 ch, 2 = 512 x 128, 3 = 256 x 128
    };
    Kernel kernel = NONE;
    int bp = 0, bc = 0, bk = 32, pf = 1;      // workgroup tile (pixels x channels), K per stage, stages requested ahead
    bool conv = false, sef = false, fk = false;   // implicit-GEMM body; squeeze-excitation in the prologue; the bound-test-free K loop
    int k = 0, t = 0, halo = 0;
    bool head = false, pool = false;          // fp32 head form (takes the rider w_b); writes the 2 x 2 max-pooled map (pool_out)
    bool proj = false;                        // PW_DIRECT, t = 1: the weight-stationary body (pw_wstat_kernel<k + 1, .., PROJ>) behind the launch and its label
};

// ---- workgroup thresholds. Tile choice of the staged kernels: these GEMMs are latency/HBM-bound, not MFMA-bound, so what matters is (a) enough
// workgroups to fill 256 CUs several times over and (b) not re-reading x for many channel tiles. Prefer the largest tile that still gives
// >= ~1500 workgroups, else fall back to smaller tiles.
constexpr long PW_FILL_WGS = 1500;
constexpr long PW_64x128_MIN_WGS = 600;
constexpr long CONV_128x128_MIN_WGS = 300;      // min workgroups for the 128x128 tile of the MFMA-bound dense convs (measured on the VGG models)
constexpr long CONV_RING_MAX_WGS = 512;         // below: a small dense conv, latency-bound (conv_choose)
constexpr long CONV_BIG_MIN_WGS = 40;           // 256 x 256 tiles. Measured on both VGG models: 40 < 90 < 200; the sub-batch chains fill the chip together
constexpr long HEAD_512x128_MIN_WGS = 128;      // half the chip in 512-pixel tiles
constexpr long GROUP_RING_MAX_WGS = 256;        // (in 128 x 128 tiles) below: a small-level dense head group, latency-bound (pw_group_choose)
constexpr int PW_DIRECT_TC2_MIN_COUT = 400;
constexpr int CONV_BIG_TILE = 256, CONV_GLDS_K = 64;      // conv_glds_kernel: tile edge and K per stage (convbig.hip asserts its own constants against these)

inline long pw_wgs(const PwArgs& a, int bp, int bc) { return (long)dn_cdiv(a.m, bp) * dn_cdiv(a.cout, bc); }

// pw_kernel on 32-deep double-buffered K staging (measured and dropped: a single exact-K stage for K <= 128 -- no load/compute overlap, slower; 64-deep double
// buffer -- lost to occupancy), or (ring) with the stages requested 4 ahead through a register ring
inline PwChoice pw_tile(const PwArgs& a, bool conv, int bp, int bc, bool ring = false, bool sef = false) {
    PwChoice c;
    c.kernel = PwChoice::PW_TILE; c.bp = bp; c.bc = bc; c.conv = conv; c.pf = ring ? 4 : 1; c.sef = sef;
    // MFMA-bound dense convolutions (VGG): 64-deep stages halve the barriers per MFMA; the tile is register-limited to two
    // workgroups per CU either way, and 2 x 74 KB of LDS fit
    if (conv && !ring && bp == 128 && bc == 128 && a.cv_cin % 64 == 0) c.bk = 64;
    // the bound-test-free K loop (pw_body FK): whole 32-deep stages, no SE-scaled staging, 32-bit byte offsets
    c.fk = ring && !conv && !sef && dn_knob("DN_PW_FASTK", 1) && a.cin % c.bk == 0 && (!a.se || a.hw >= bp) && !(a.act >> 8) && (size_t)a.m * a.cin < (1u << 30) &&
           (size_t)a.cout * a.cin < (1u << 30);
    return c;
}
// the last rules of pw_choose and conv_choose: the wide tiles by fill
inline PwChoice pw_tile_wide(const PwArgs& a, bool conv) {
    if (pw_wgs(a, 128, 128) >= (conv ? CONV_128x128_MIN_WGS : PW_FILL_WGS)) return pw_tile(a, conv, 128, 128);
    if ((pw_wgs(a, 128, 64) >= PW_FILL_WGS || a.cout % 128 > 64 || a.cout % 128 == 0) && pw_wgs(a, 64, 128) >= PW_64x128_MIN_WGS) return pw_tile(a, conv, 64, 128);
    return pw_tile(a, conv, 64, 64);
}

// ================================================================ (a) one 1x1 convolution
// register-direct schedule for short reductions (pwdirect.hip)
inline bool pw_direct_supported(const PwArgs& a) {
    // squeeze-excitation scaled inputs: only where a 32-row tile lies inside one image (the 40 x 40 maps) and the reduction is short
    if (a.se && !(a.hw % 32 == 0 && a.cin <= 128)) return false;
    return dn_knob("DN_PW_DIRECT", 1) != 0 && a.cv_k == 1 && !a.out_fp32 && !a.sef_part && !a.w_b && a.cin % 8 == 0 && a.cin >= 8 &&
           a.cin <= 256 && a.cout % 8 == 0 && a.cout >= 8 && !(a.act >> 8) && a.out_img_stride == 0 && a.out_base == 0;
}
inline bool pw_wstat_supported(const PwArgs& a) {
    return dn_knob("DN_PW_WSTAT", 1) != 0 && a.wfrag && !a.se && !a.residual && a.cin >= 16 && a.cin <= 128 && a.cin % 8 == 0 && a.m >= 3200 &&
           (long)a.m * a.cout * 2 < 0x7fffffffL && a.cout >= 64;
}
// The narrow projections (cout <= 64: one or two channel tiles, every A fragment of the layer in a wave's registers), with or without squeeze-excitation
// scale and residual, on the same weight-stationary schedule (pw_wstat_kernel<.., PROJ = true>). A 32-row tile lies inside one image (hw % 32 == 0): one
// scale row serves it, and its residual rows are 64 cout contiguous bytes. DN_PW_WSTAT_PROJ: 1 (default) = from PW_WSTAT_PROJ_MIN_ROWS rows, 0 = never,
// 2 = wherever the body can run (tests, A/B).
constexpr int PW_WSTAT_PROJ_MIN_ROWS = 51200;
inline bool pw_wstat_proj_supported(const PwArgs& a) {
    const int knob = dn_knob("DN_PW_WSTAT_PROJ", 1);
    return knob != 0 && a.wfrag && a.cin >= 16 && a.cin <= 128 && a.cin % 8 == 0 && a.cout <= 64 && a.hw % 32 == 0 && (knob == 2 || a.m >= PW_WSTAT_PROJ_MIN_ROWS) &&
           (long)a.m * a.cout * 2 < 0x7fffffffL;
}
// the squeeze-excitation of a projection can be computed in the projection kernel's prologue (SEF variant of the 64 x 64 tile)
inline bool pw_sef_supported(const PwArgs& a) {
    return dn_knob("DN_SE_FOLD", 1) != 0 && !a.se && a.cin % 8 == 0 && a.sef_sq <= 32 && a.hw >= 64;
}

inline PwChoice pw_choose(const PwArgs& a) {
    PwChoice c;
    if (pw_direct_supported(a)) {
        // the expansions (short reduction, wide output, no scale, no residual): weight-stationary waves over LDS-DMA'd pixel tiles (round 6)
        if (pw_wstat_supported(a)) {
            c.kernel = PwChoice::PW_WSTAT;
            c.k = a.cin / 16 + 1;
            const int ctiles = dn_cdiv(a.cout, 32);
            // tiles per run: as many as 96 registers of A fragments allow, least padding of the last run first
            int waste = 1 << 30;
            c.t = 2;
            for (int rt = 4; rt >= 2; --rt) {
                if (c.k * rt > 24) continue;
                const int w = dn_cdiv(ctiles, rt) * rt - ctiles;
                if (w < waste) { waste = w; c.t = rt; }
            }
            return c;
        }
        const int ctiles = dn_cdiv(a.cout, 32);
        const int ksf = a.cin >> 4;
        c.k = ksf;
        // wide expansions with enough rows: the streaming variant (pw_stream_kernel) -- channel runs sized so that all waves are resident at once
        if (dn_knob("DN_PW_STREAM", 1) && !a.se && !a.residual && ksf >= 4 && ksf <= 8 && ctiles >= 12 && a.m >= 12800) {
            c.kernel = PwChoice::PW_STREAM;
            c.t = 2;                        // 32-pixel tiles per wave
            return c;
        }
        // One 32-channel tile per wave (TC = 1) on the narrow layers: these launches are latency-bound, and twice the waves with half the
        // registers overlap their single memory round trip better. Wide expansions (cout >= PW_DIRECT_TC2_MIN_COUT, short reductions) take two
        // tiles per wave: every wave re-reads its x rows once per channel tile, and at 21 tiles (112 -> 672) that is most of the traffic
        // (measured: threshold 400 -> batch 64 1.115 -> 1.107 ms, batch 32 0.79 -> 0.77 ms; 200 and 600 in between).
        c.kernel = PwChoice::PW_DIRECT;
        c.t = (ksf <= 8 && a.cout >= PW_DIRECT_TC2_MIN_COUT) ? 2 : 1;
        // the narrow projections with many rows (the SE-scaled 72 / 120 -> 40 of the 40 x 40 maps at batch 32 and more): the weight-stationary body behind
        // this launch. Measured (profiles/pw_wstat_proj_ab.txt; rocprofv3, one forward at a time): 102 400 rows 120 -> 40 13.8 -> 11.2 us, 72 -> 40 9.4 -> 8.1;
        // 51 200 rows 9.8 -> 8.4 and 5.9 -> 5.6; the step at batch 64 0.5693 -> 0.5624 ms, at batch 32 level. Fewer rows: not measured, the register-direct body stays.
        c.proj = c.t == 1 && pw_wstat_proj_supported(a);
        return c;
    }
    if (dn_knob("DN_PW_XS", 1) && !a.sef_part && a.wfrag && a.cin % 16 == 0 && a.cin <= 1024 && a.cout <= 160 && !(a.act >> 8) &&      // (K % 16 == 8: measured slower than the tiled kernel)
        ((a.cin >= 64 && a.m <= 8192) || (a.cin >= 160 && a.m <= 16384))) {
        // measured (tools/tune_pw.py): the strip kernel wins where the tiled kernel cannot fill the chip -- M <= ~8k rows, or
        // M <= ~16k rows when K is long (the tiled kernel pays one exposed round trip per 32-deep K stage)
        c.kernel = PwChoice::PW_XS;
        return c;
    }
    // 1x1 convs with a thin side (cin < 256 or cout < 128) are HBM/latency-bound: tools/tune_pw.py over every layer shape
    // of the model shows the small tiles (most workgroups, fewest registers: 64 VGPRs -> 8 waves/SIMD) winning or tying
    // everywhere, 128x32 when there is a single channel tile. The big tiles only pay off for MFMA-bound shapes.
    if (a.cin < 256 || a.cout < 128) {
        if (a.cin > 32) {
            // the register ring on both measured cases: 2..4 K stages (cin <= 128), all loads up front; long K on a thin layer (cin > 128), loads 4 stages ahead
            if (a.sef_part && a.cin <= 128 && pw_sef_supported(a)) return pw_tile(a, false, 64, 64, true, true);     // squeeze-excitation folded in
            return a.cout <= 32 ? pw_tile(a, false, 128, 32, true) : pw_tile(a, false, 64, 64, true);
        }
        return a.cout <= 32 ? pw_tile(a, false, 128, 32) : pw_tile(a, false, 64, 64);
    }
    // a 1x1 layer with few workgroups and a long K (the first extras layer: 480 -> 256 on 10 x 10) is a chain of exposed round trips with the plain
    // double buffer: stages requested 4 ahead on the bound-test-free loop. Measured (round 3): the launch 18.8 -> 14 us, one forward at a time -5 us,
    // with three forwards in flight 0.2 - 0.3 % slower in three of three pairs: opt-in
    // (cin >= 256 and cout >= 128 here)
    if (dn_knob("DN_PW_LONGK_PF", 0) && a.cin % 32 == 0 && pw_wgs(a, 64, 64) < PW_FILL_WGS) return pw_tile(a, false, 64, 64, true);
    return pw_tile_wide(a, false);
}

// ================================================================ (b) one dense convolution
// the 1x1 problem that a dense 1x1 / stride 1 / pad 0 conv with fp16 output is
inline PwArgs conv_1x1_as_pw(const PwArgs& a) {
    PwArgs b;
    b.x = a.x; b.w = a.w; b.bias = a.bias; b.residual = nullptr; b.se = nullptr; b.out = a.out;
    b.hw = a.hw; b.m = a.m; b.cin = a.cv_cin; b.cout = a.cout; b.act = a.act; b.out_fp32 = 0; b.out_img_stride = 0; b.out_base = 0;
    b.xq = a.xq;
    return b;
}
// the one-image 3 x 3 "same" conv that a plan-time (cin, cout, h, w) question is about
inline PwArgs conv3x3_query(int cin, int cout, int h, int w) {
    static const half_t dummy_zero[8] = {};
    PwArgs a{};
    a.cv_k = 3; a.cv_stride = 1; a.cv_pad = 1; a.cv_dil = 1; a.cv_h = a.cv_ho = h; a.cv_w = a.cv_wo = w; a.cv_cin = cin;
    a.zeros = dummy_zero; a.residual = nullptr; a.se = nullptr; a.out_fp32 = 0;
    a.hw = h * w; a.m = a.hw; a.cin = 9 * cin; a.cout = cout;
    return a;
}

// conv_patch_kernel / conv_patch_resident_kernel: 3 x 3 "same", 64 or 128 input channels
inline bool patch_shape(const PwArgs& a) {
    return a.zeros && !a.out_fp32 && !a.residual && !a.se && a.cv_k == 3 && a.cv_stride == 1 && a.cv_pad == 1 && a.cv_dil == 1 &&
           a.cv_ho == a.cv_h && a.cv_wo == a.cv_w && a.cv_cin % 64 == 0 && a.cv_cin <= 128 && a.cout % 64 == 0 && a.m / a.hw <= 65535;
}
inline bool patch_resident_shape(const PwArgs& a) {
    const long out_bytes = (long)(a.m / a.hw) * (a.pool_out ? (a.cv_h >> 1) * (a.cv_w >> 1) : a.cv_h * a.cv_w) * a.cout * 2;
    return a.cv_cin == 64 && a.act == DN_ACT_RELU && out_bytes < 0xFFFFFFF0L && (long)a.cv_h * a.cv_w * 128 < (1L << 31) && dn_knob("DN_PATCH_RESIDENT", 1) != 0;
}
// conv_halo_kernel: the run-staged tiles
constexpr int halo_run_rows(int tp, int tc) { return tc == 4 ? 704 : tp == 8 ? 832 : 960; }      // rows of a staged run (pixel tile + halo on both sides), upper bound
inline bool halo_shape(const PwArgs& a) {
    const int halo = dn_knob("DN_CONV_HALO", 1);
    return halo && a.zeros && a.cv_k == 3 && a.cv_stride == 1 && a.cv_pad == a.cv_dil && a.cv_ho == a.cv_h && a.cv_wo == a.cv_w &&
           a.cv_cin % 64 == 0 && (long)a.m * a.cv_cin * 2 < (1L << 31) && (long)(a.cout + a.cout_b) * a.cin * 2 < (1L << 32);
}
inline int halo_rows(const PwArgs& a) { return 2 * (a.cv_pad * a.cv_w + a.cv_pad); }
// which tile a fp16-output 3x3 stride-1 conv runs on: 0 none, 1 = 256 x 256, 2 = 512 x 128, 3 = 256 x 128
inline int halo_variant(const PwArgs& a) {
    if (a.out_fp32 || a.residual || a.se || !halo_shape(a)) return 0;
    const int hr = halo_rows(a);
    if (a.cout % 256 == 0 && 256 + hr <= halo_run_rows(4, 4)) return 1;
    if (a.cout % 128 == 0 && a.cv_cin >= 128 && 512 + hr <= halo_run_rows(8, 2)) return 2;
    if (a.cout % 128 == 0 && a.cv_cin >= 128 && 256 + hr <= halo_run_rows(4, 2)) return 3;      // (one 64-channel iteration: measured level with the 128x128 tile)
    // (a 256 x 64 tile for the 64-channel layer conv1_2: 330 vs 388 TFLOP/s for the 128 x 64 tile of pointwise.hip -- four MFMAs per K
    // step cannot cover the fragment masks and reads)
    return 0;
}
// ... with the max-pool epilogue (conv3_3 of ssd512: 256 channels on 128 x 128), asked of ONE image: the tile must be whole row pairs of one
// image (256 % 2W == 0, H W % 256 == 0)
inline bool halo_pool_shape(const PwArgs& one) {
    return !(one.cv_h & 1) && !(one.cv_w & 1) && halo_variant(one) == 1 && 256 % (2 * one.cv_w) == 0 && one.hw % 256 == 0;
}
inline bool conv_glds_shape(const PwArgs& a) {
    return a.zeros && a.cv_cin % CONV_GLDS_K == 0 && a.cout % CONV_BIG_TILE == 0 && !a.out_fp32 && !a.residual && !a.se && a.cv_k * a.cv_k <= 32 && a.cin >= 2 * CONV_GLDS_K &&
           (long)a.m / a.hw * a.cv_h * a.cv_w * a.cv_cin * 2 < (1L << 31) && (long)a.cout * a.cin * 2 < (1L << 32);
}

enum ConvUse {
    CONV_PLAIN,     // launch_conv
    CONV_POOLED,    // launch_conv_pool: MaxPool2d(2, 2) in the epilogue (a.pool_out)
    CONV_HEAD       // launch_conv_head_big: a dense fp32 head on the run-staged tiles, with or without the rider (a.w_b); NONE: the group launch takes it
};

inline PwChoice conv_choose(const PwArgs& a, ConvUse use) {
    PwChoice c;
    c.conv = true;
    if (use == CONV_HEAD) {
        // Dense 3x3 heads with fp32 outputs (SSDHead, generalized_ssd.py:77-92) on the run-staged tiles; channel tiles beyond cout compute on the last
        // weight row and are not stored. The class + box channels of a level (380 / 570 for 91 classes) fill 74 % of two / three 256-channel tiles but
        // 99 % / 89 % of three / five 128-channel tiles, and the 512 x 128 run tile runs level with the 256 x 256 one per FLOP (conv3 .. conv5 of
        // ssd512_vgg16: 1140-1330 vs 1150-1320 TFLOP/s): the idle channels were a quarter of the head launches' time. A level too small for half the
        // chip in 512-pixel tiles (the 16 x 16 level of ssd512 at batch 32: 80 workgroups) takes 256 x 128 tiles -- twice the workgroups at half the
        // work each.
        if (!dn_knob("DN_CONV_HEAD_BIG", 1) || !a.out_fp32 || a.residual || a.se || !halo_shape(a) || (a.cout & 1)) return c;
        c.head = true;
        const int hr = halo_rows(a), nc = a.cout + a.cout_b;
        const int c256 = dn_cdiv(nc, 256), c128 = dn_cdiv(nc, 128);
        const long p256 = dn_cdiv(a.m, 256), p512 = dn_cdiv(a.m, 512);
        if (dn_knob("DN_CONV_HEAD_NARROW", 1) && c128 * 128 < c256 * 256 && a.cv_cin >= 128) {
            if (512 + hr <= halo_run_rows(8, 2) && p512 * c128 >= HEAD_512x128_MIN_WGS) c.halo = 2;
            else if (256 + hr <= halo_run_rows(4, 2) && p256 * c128 >= 2 * CONV_BIG_MIN_WGS) c.halo = 3;      // (40 workgroups of the 8 x 8 level: slower than the group launch)
        }
        const int tiles = dn_cdiv(a.cout, 256);
        if (!c.halo && 256 + hr <= halo_run_rows(4, 4) && a.cout * 10 >= tiles * 256 * 6 && p256 * tiles >= CONV_BIG_MIN_WGS) c.halo = 1;      // at most 40 % of the channel tiles idle
        if (c.halo) c.kernel = PwChoice::CONV_HALO;
        return c;
    }
    const bool patch = patch_shape(a);
    const PwChoice::Kernel patch_kernel = patch_resident_shape(a) ? PwChoice::CONV_PATCH_RESIDENT : PwChoice::CONV_PATCH;
    if (use == CONV_POOLED) {
        // By geometry alone, and of ONE image (the launcher walks a batch beyond the run-staged tile's 2 GB in image ranges). This is the one place where
        // launch and plan deliberately differ: DN_CONV_BIG / DN_CONV_POOL / DN_CONV_HALO_POOL decide at dn_create (conv_patch_pool_ok,
        // conv_halo_pool_ok), the launch only checks the geometry, so a knob flipped between dn_create and dn_forward cannot strand a fused pair.
        // Nor may a.out steer the choice: the patch kernel never writes the full-resolution map (a pair whose map has other readers is only fused
        // when the run-staged tile takes it: plan.hip), and a.out is non-null for EVERY tensor with DN_WS_REUSE=0.
        PwArgs one = a;
        one.m = a.hw;
        c.pool = true;
        // 64 input channels: always the patch kernel
        if (halo_pool_shape(one) && !(patch && a.cv_cin <= 64) && pw_wgs(one, 256, 256) >= CONV_BIG_MIN_WGS) { c.kernel = PwChoice::CONV_HALO; c.halo = 1; }
        else if (patch) c.kernel = patch_kernel;
        return c;
    }
    // the 256 x 256-tile kernels (convbig.hip), where one of them takes the shape and the launch has enough of their workgroups
    const int hv = halo_variant(a);
    const bool big = dn_knob("DN_CONV_BIG", 1) && (hv || patch || conv_glds_shape(a)) && pw_wgs(a, 256, 256) >= CONV_BIG_MIN_WGS;
    // a 1x1 dense conv IS a pointwise conv: unless it is big enough for the 256 x 256-tile kernel, the pointwise path serves it
    // (register-direct kernel up to cin = 256, 4-stage prefetch ring beyond; the implicit-GEMM body walks it one exposed stage at a time)
    if (!big && a.cv_k == 1 && a.cv_stride == 1 && a.cv_pad == 0 && !a.out_fp32) { c.kernel = PwChoice::AS_POINTWISE; return c; }
    if (big) {
        // 64 input channels: always the patch kernel; 128: where the run kernel would need its 256 x 128 tile (maps wider than 159; measured:
        // conv2_2 of ssd512 882 vs 568 TFLOP/s, while the 512 x 128 run tile of the 150-wide map keeps the faster step)
        if (patch && (a.cv_cin <= 64 || hv == 0 || hv == 3)) { c.kernel = patch_kernel; return c; }
        c.kernel = hv ? PwChoice::CONV_HALO : PwChoice::CONV_GLDS;
        c.halo = hv;
        return c;
    }
    if (a.cout <= 32) return pw_wgs(a, 256, 32) >= PW_FILL_WGS ? pw_tile(a, true, 256, 32) : pw_tile(a, true, 128, 32);
    if (a.cout <= 64) return pw_wgs(a, 128, 64) >= PW_FILL_WGS ? pw_tile(a, true, 128, 64) : pw_tile(a, true, 64, 64);
    // small dense convs (the extras of the VGG models: <= 16 x 16 maps, K = 9 cin up to 4608): a few workgroups walking 70 - 140
    // K stages, each an exposed memory round trip with the plain double buffer (60 - 130 us per layer for < 1 us of MFMA work):
    // request the stages 4 ahead through the register ring of the short-K pointwise variant
    if (pw_wgs(a, 64, 64) < CONV_RING_MAX_WGS) return pw_tile(a, true, 64, 64, true);
    return pw_tile_wide(a, true);
}

// ================================================================ (c) a grouped head launch
// All problems are of the same kind (pointwise or implicit-GEMM conv); the tile is chosen for the widest one. Stages requested ahead: head 1x1
// convs have long K (21 stages at level 0), loads run 3 stages ahead; the dense-conv heads of the VGG models are MFMA-bound at 184 VGPRs and keep
// the plain double buffer -- except the small levels.
inline PwChoice pw_group_choose(const PwArgs* arr, int count, bool conv) {
    int maxc = 0;
    long wg128 = 0;
    bool all64 = true;
    for (int i = 0; i < count; ++i) {
        if (arr[i].cout > maxc) maxc = arr[i].cout;
        wg128 += pw_wgs(arr[i], 128, 128);
        all64 &= arr[i].cv_cin % 64 == 0;
    }
    PwChoice c;
    c.kernel = PwChoice::PW_GROUP; c.conv = conv; c.pf = conv ? 1 : 3;
    auto tile = [&](int bp, int bc) { c.bp = bp; c.bc = bc; };
    if (maxc <= 32) { tile(128, 32); if (conv && wg128 < GROUP_RING_MAX_WGS) c.pf = 3; }
    else if (maxc <= 64) tile(64, 64);
    else if (wg128 >= PW_FILL_WGS) {
        tile(128, 128);
        // MFMA-bound dense-conv heads: 64-deep stages as in pw_tile (half the barriers per MFMA)
        if (conv && all64) c.bk = 64;
        if (!conv) {
            // 96-wide channel tiles (a wave = 32 pixels x 96 channels) where they pad less: the 546 class channels of the SSDLite heads are
            // 6 x 96 = 576 columns instead of 5 x 128 = 640 -- the head launch is the longest full-chip launch of a forward (batch 64, three
            // forwards in flight: 0.789 -> 0.775 ms; 128 x 192 tiles 0.808, 64 x 192 level)
            double c96 = 0, c128 = 0;
            for (int i = 0; i < count; ++i) {
                c96 += (double)arr[i].m * dn_cdiv(arr[i].cout, 96) * 96;
                c128 += (double)arr[i].m * dn_cdiv(arr[i].cout, 128) * 128;
            }
            if (c96 <= 0.95 * c128) tile(128, 96);
        }
    } else {
        tile(64, 128);
        // the dense heads of the small levels (a few dozen workgroups, 72 - 144 K stages): latency-bound, stages requested 3 ahead
        if (conv && wg128 < GROUP_RING_MAX_WGS) c.pf = 3;
    }
    if (!conv) {
        // every problem on the bound-test-free K loop (whole 32-deep stages, no SE-scaled staging, 32-bit byte offsets): the instantiation that holds nothing else
        c.fk = dn_knob("DN_PW_FASTK", 1) != 0;
        for (int i = 0; i < count; ++i)
            c.fk &= arr[i].cin % c.bk == 0 && !arr[i].se && !(arr[i].act >> 8) && (size_t)arr[i].m * arr[i].cin < (1u << 30) && (size_t)arr[i].cout * arr[i].cin < (1u << 30);
    }
    return c;
}

// ================================================================ (d) one depthwise convolution (depthwise.hip: dw_kernel / dw_group_kernel<K, S, TW>)
constexpr int dw_tw(int stride) { return stride == 1 ? 4 : 2; }     // output pixels of a row per thread: the window of TW pixels is (TW - 1) S + K input columns
struct DwChoice {
    enum Kernel { NONE, DW };
    enum Pool { NO_POOL, POOLED, POOLED_SE };       // launch class: dw_kernel's POOL = 0, 1 (per-workgroup channel sums), 2 (+ the SE FCs in the image's last workgroup)
    Kernel kernel = NONE;
    int k = 0, stride = 0, tw = 0;
    Pool pool = NO_POOL;
};
inline DwChoice dw_choose(const DwArgs& a) {
    DwChoice c;
    c.k = a.k; c.stride = a.stride;
    if ((a.k != 3 && a.k != 5) || (a.stride != 1 && a.stride != 2)) return c;
    c.kernel = DwChoice::DW; c.tw = dw_tw(a.stride);
    c.pool = a.se_scale ? DwChoice::POOLED_SE : a.pool ? DwChoice::POOLED : DwChoice::NO_POOL;       // (the SE tail without a pooled output: the launcher refuses it)
    return c;
}

// ================================================================ (e) the squeeze-excitation FCs
// the small ones (the 40 x 40 blocks of MobileNetV3): DN_SE_SMALL moves them from the projection's prologue into the tail of the pooling depthwise launch
// (plan.hip, both sites); the device's dw_se_tail_is_small adds what only the launch knows (constexpr: callable from there)
constexpr bool se_is_small(int c, int squeeze) { return c <= 128 && squeeze <= 32; }
struct SeChoice {
    enum Kernel { FC, FC8_14_6, FC8_15_4 };     // se_fc_kernel, se_fc8_kernel<FB, PB>: 16-byte weight rows / partial rows in flight per thread
    Kernel kernel = FC;
    int rs = 0, ks1 = 0, ks2 = 0;               // se_fc8_kernel's slices of the partial rows and of the two reduction axes (they size its LDS)
};
inline SeChoice se_choose(int c, int squeeze, int nblk) {
    SeChoice s;
    if (!depthwise_se_tail_supported(c, squeeze) || !dn_knob("DN_SE_FC8", 1)) return s;      // 16-byte loads need both widths in whole 8s
    s.rs = std::max(1, std::min(1024 / (c >> 2), nblk));
    s.ks1 = std::max(1, std::min(1024 / (squeeze >> 3), c >> 3));
    s.ks2 = std::max(1, std::min(1024 / (c >> 3), squeeze >> 3));
    // the 960 / 240 blocks (29 - 30 rows per slice): two batches of 15 instead of three of 14
    const bool wide = (dn_cdiv(c, s.ks1) > 14 || dn_cdiv(squeeze, s.ks2) > 14) && nblk <= 4 * s.rs;
    s.kernel = wide ? SeChoice::FC8_15_4 : SeChoice::FC8_14_6;
    return s;
}

// ================================================================ (f) the stem (3 x 3, 16 / 32 / 64 output channels)
struct StemChoice {
    enum Kernel { NONE, SPLIT, S2, MFMA64P, MFMA64, PLAIN };    // stem_split_kernel, stem3s2_kernel, stem_mfma64p_kernel, stem_mfma64_kernel, stem_kernel
    Kernel kernel = NONE;
    int tpw = 0, ahead = 0;     // SPLIT: tiles per wave, tiles a request runs ahead
    bool touch = false;         // SPLIT: the wave touches its image lines up front
};
inline StemChoice stem_choose(const StemArgs& a) {
    StemChoice c;
    if (a.k != 3 || (a.cout != 16 && a.cout != 32 && a.cout != 64)) return c;
    // the fp16 matrix cores with split operands: the three stems of the zoo, inside the kernel's 32-bit byte offsets
    const bool split_inst = (a.cout == 64 && a.stride == 1 && a.act == DN_ACT_RELU) || (a.cout == 16 && a.stride == 2 && a.act == DN_ACT_HSWISH) ||
                            (a.cout == 32 && a.stride == 2 && a.act == DN_ACT_RELU6);
    const bool split_geom = a.stride == 1 ? (a.ho == a.h && a.wo == a.w_) : ((a.w_ & 1) == 0 && 2 * a.wo == a.w_ && a.ho == (a.h + 1) / 2);
    if (a.pad == 1 && a.split_ok && dn_knob("DN_STEM_SPLIT", 1) && a.wo >= 32 && (long)3 * a.h * a.w_ < (1L << 28) && (long)a.ho * a.wo * a.cout < (1L << 29) &&
        split_inst && split_geom) {
        c.kernel = StemChoice::SPLIT;
        // requests run 3 tiles ahead and the wave touches its lines up front for the 64-channel stem (1 GB of stores per forward: a first touch of an
        // image line behind that stream outlasts two tiles; 16 images of 512 x 512, same box: 145 us -> 126 with the touch, 128 with 3 tiles
        // ahead, 121 - 126 with both, 123 with 4), 2 tiles ahead and no touch for the narrow ones (17.6 / 36.3 us; with the touch 19.1 / 37.2).
        c.ahead = a.cout >= 64 ? 3 : 2;
        c.touch = a.cout >= 64;
        // tiles per wave: 8 for the 64-channel stem (the weights' split -- 64 values per lane -- once per 8 tiles), 4 for the narrow ones (their
        // launches are small: more, shorter waves; measured 4 / 8 / 16: 17.5 / 19.3 / 19.0 us for 16 channels, 36.2 / 38.0 / 38.4 for 32,
        // 147.5 / 144.8 / 144.6 for 64)
        c.tpw = a.cout >= 64 ? 8 : 4;
        return c;
    }
    // fp32 from here on. 3 x 3 stride 2 on an even-width image: all nine (channel, row) loads up front
    if (a.stride == 2 && a.pad == 1 && (a.w_ & 1) == 0 && 2 * a.wo == a.w_) { c.kernel = StemChoice::S2; return c; }
    // 64 channels, stride 1 on the fp32 matrix cores; pipelined inside the wave where pad 1 / ReLU / "same" let the step run without branches
    if (dn_knob("DN_STEM_MFMA", 1) && a.cout == 64 && a.stride == 1 && (long)3 * a.h * a.w_ < (1L << 30)) {
        const bool pipe = dn_knob("DN_STEM_PIPE", 1) && a.pad == 1 && a.act == DN_ACT_RELU && a.ho == a.h && a.wo == a.w_ && a.wo >= 32 && (long)a.h * a.w_ < (1L << 24);
        c.kernel = pipe ? StemChoice::MFMA64P : StemChoice::MFMA64;
        return c;
    }
    c.kernel = StemChoice::PLAIN;
    return c;
}

// ================================================================ (g) the per-class selection kernels of the post-process (postprocess.hip)
// Candidate capacity in words of 64 candidates: the NW the hard kernels (select_nms_kernel, select_nms_fast_kernel) and the soft reduce
// (select_soft_kernel) are instantiated for; topk_candidates is 1 .. 512 (launch_postprocess validates it).
constexpr int post_nw_bucket(int topk) {
    const int w = (topk + 63) / 64;
    return w <= 2 ? w : w <= 4 ? 4 : w <= 5 ? 5 : 8;
}
// The soft reduce has one form: four waves with an LDS exchange per step (one wave, no exchange, for a capacity of 64 candidates). Measured
// against one wave holding NW candidates per lane (no barrier) at topk 300, batch 64, 90 classes: 1.53 vs 2.05 ms per forward in linear mode,
// 1.42 vs 1.98 ms in Gaussian mode; the one-wave form is gone.

// ================================================================ (h) the fused inverted-residual launch (expdw.hip; its two other bodies in expdw_direct.hip, expdw_rows.hip)
constexpr int EXPDW_NT = 512;           // threads per workgroup: 8 waves (expdw.hip asserts its own constants against these three)
constexpr int EXPDW_EW = 72;            // halfs per row of the expanded tile in LDS: a 64-channel chunk + 8, which a last chunk of exactly 72 channels fills
constexpr int EXPDW_XKS = 8;            // most full 16-deep K steps of the expand (cin <= 128)
constexpr size_t EXPDW_LDS_MAX = 160 * 1024, EXPDW_PERSIST_LDS_MAX = 80 * 1024;     // a workgroup's LDS; the persistent form's (two resident workgroups per CU)
constexpr int EXPDW_MIN_WGS = 1024;     // (without a project stage) split the chunks over grid.y until there are enough workgroups to fill the chip a few times over

struct ExpDwChoice {
    enum Body {
        NONE,               // the tiled bodies cannot take the launch (lds beyond EXPDW_LDS_MAX, or a grid beyond 65535 in y or z) and no other body does
        DIRECT, ROWS,       // expdw_direct_kernel<act1> (expdw_direct.hip), expdw_rows_kernel<act1> (expdw_rows.hip): bands of `band` output rows
        ONE_PERSIST,        // expdw_one_kernel<k, stride, oh, ow, ksm, xw8, wide>: the resident workgroups walk the tiles
        TILED               // expdw_kernel<k, stride, oh, ow, ksm, exp, proj, xw8, wide, one>: one workgroup per tile (and run of chunks)
    };
    Body body = NONE;
    int k = 0, stride = 0, oh = 0, ow = 0;              // kernel size, stride, output tile
    int ksm = 0, xw8 = 0;                               // full K steps of the expand held in registers; X row width in 16-byte pieces where it is a compile-time constant (0: runtime)
    bool exp = false, proj = false, wide = false, one = false;   // expand / project stage; a last chunk of 72 channels taken whole; the chunk loop is one chunk
    bool whole = false;                                 // TILED: the phases walked once over the whole expanded width (expdw_whole_kernel, expdw_whole.hip), not per 64-channel chunk
    int band = 0;                                       // DIRECT, ROWS: output rows per band
    int cpw = 0, zsplit = 1, xw = 0, stage_out = 0;     // chunks per workgroup and their split over grid.y; halfs per X row; the projected tile leaves through LDS
    size_t lds = 0, lds_p = 0;                          // LDS bytes of expdw_kernel / of expdw_one_kernel (+ the tile's own output buffer)
    size_t lds_w = 0;                                   // LDS bytes of expdw_whole_kernel (0: the shape is not its)
    char label[64] = "";                                // the launch's label: ALWAYS the tiled choice's, whichever body runs (plan signatures and bench families do not see DIRECT / ROWS)
};

// the output tile of a map
inline void expdw_tile(int Ho, int Wo, int stride, int proj_cout, int* oh, int* ow) {
    if (Wo <= 5 && Ho <= 5) { *oh = 5; *ow = 5; }
    else if (Wo <= 10) { *oh = 5; *ow = 10; }
    else if (Wo < 32 && Wo % 16 != 0) {                     // 19x19 / 20x20 maps: 10-wide tiles waste nothing
        if (stride == 1) { *oh = 10; *ow = 10; } else { *oh = 5; *ow = 10; }       // (measured again in round 4 on the V2 model at 300 x 300: 5 x 10 tiles there are 2.4 % slower, although the 10 x 10 variants with cin >= 64 spill 36 - 44 B per lane)
        // with a project stage the (pixel tile x channel tile) units must fit the 8 waves: 100 pixels x 80 channels = 12 units, 50 x 80 = 6
        if (proj_cout > 0 && ((*oh * *ow + 31) / 32) * ((proj_cout + 31) / 32) > EXPDW_NT / 64) { *oh = 5; *ow = 10; }
    }
    else { *oh = 8; *ow = (stride == 1) ? 16 : 8; }
}
inline int expdw_tiles_per_image(int Ho, int Wo, int stride) {
    int oh, ow;
    expdw_tile(Ho, Wo, stride, 0, &oh, &ow);
    return dn_cdiv(Ho, oh) * dn_cdiv(Wo, ow);
}
inline bool expdw_supported(int cin, int cexp, int k, int stride) {
    return cin % 8 == 0 && cin <= 16 * EXPDW_XKS && cexp % 8 == 0 && (k == 3 || k == 5) && (stride == 1 || stride == 2);
}
// the project stage keeps one MFMA accumulator per wave: (pixels of the tile / 32) x (cout / 32) units must fit the 8 waves
inline bool expdw_project_supported(int cexp, int cout, int Ho, int Wo, int stride) {
    int oh, ow;
    expdw_tile(Ho, Wo, stride, cout, &oh, &ow);
    return cexp % 8 == 0 && cout % 8 == 0 && ((oh * ow + 31) / 32) * ((cout + 31) / 32) <= EXPDW_NT / 64;
}
// rows of the staged input region of a tile, in whole 32-row MFMA tiles (ExpDwGeom::ROWS)
constexpr int expdw_region_rows(int k, int stride, int oh, int ow) { return (((oh - 1) * stride + k) * ((ow - 1) * stride + k) + 31) / 32 * 32; }
// the persistent single-chunk form (expdw_one_kernel) is instantiated for the block shapes that take it: 3x3 on the 8 x 8 stride-2 / 8 x 16 stride-1 tiles of
// the large maps, cin 16 / 24 / 32. It needs the staged output tile inside the dead E buffer (no barrier between the project stage and its write), a stride of
// whole tiles per step, and no pooled sums or stamps.
inline bool expdw_persist_supported(const ExpDwArgs& a, const ExpDwChoice& c, bool stamped) {
    return c.exp && c.proj && c.ksm <= 2 && (c.xw8 == 3 || c.xw8 == 5) && c.k == 3 && c.oh == 8 && c.ow == (c.stride == 1 ? 16 : 8) && !a.pool && !stamped &&
           a.cout % 8 == 0 && a.cout <= 256 && c.lds_p <= EXPDW_PERSIST_LDS_MAX && fd_ok((unsigned long long)c.oh * c.ow * (a.cout >> 3), (unsigned)(a.cout >> 3));
}

// The whole-width form of the tiled body (expdw_whole_kernel, expdw_whole.hip) is built for the multi-chunk full blocks of the 20 x 20 maps: 3x3 stride 1 on the
// 5 x 10 tile, cin 80 (88-half X rows, five full K steps), any expanded width whose whole E tile fits beside the rest at two workgroups per CU. Its LDS: the
// depthwise output D[64][round16(cexp) + 8] laid over the dead X region [96][88] + 8, E[96][cexp, + 8 where that makes the 16-byte pieces of a row an odd number] (the finished tile is staged over it),
// all nine depthwise weight rows, the depthwise bias, the project bias.
constexpr int EXPDW_WHOLE_CIN = 80, EXPDW_WHOLE_OH = 5, EXPDW_WHOLE_OW = 10, EXPDW_WHOLE_ROWS = 96, EXPDW_WHOLE_DROWS = 64;
constexpr int EXPDW_WHOLE_CEXP_MAX = 224;       // seven 32-channel tiles of the expand on the eight waves, fourteen K steps of the projection in registers
constexpr int expdw_whole_front_halfs(int cexp) {
    const int x = EXPDW_WHOLE_ROWS * (EXPDW_WHOLE_CIN + 8) + 8, d = EXPDW_WHOLE_DROWS * (((cexp + 15) & ~15) + 8);
    return x > d ? x : d;
}
// halfs per E row: an odd number of 16-byte pieces. The expand writes 8-byte pieces down 32 rows: an even count puts them on 4 (cexp 224) or 2 (cexp 128) of the 32
// banks -- measured alone, 128 channels without the pad: 12.3 us against the chunk loop's 10.9
constexpr int expdw_whole_erow(int cexp) { return ((cexp >> 3) & 1) ? cexp : cexp + 8; }
constexpr size_t expdw_whole_lds(int cexp) {
    return ((size_t)expdw_whole_front_halfs(cexp) + (size_t)EXPDW_WHOLE_ROWS * expdw_whole_erow(cexp) + 9 * (size_t)cexp) * sizeof(half_t) + ((size_t)cexp + 256) * sizeof(float);
}
static_assert(expdw_whole_lds(EXPDW_WHOLE_CEXP_MAX) <= EXPDW_PERSIST_LDS_MAX && expdw_whole_lds(EXPDW_WHOLE_CEXP_MAX + 8) > EXPDW_PERSIST_LDS_MAX, "the widest block that keeps two workgroups per CU");
// no pooled sums, no stamps; the staged tile must fit the dead E rows and the (row tile, channel tile) units of the projection the 8 waves; the nine
// weight rows are staged by one 16-byte piece per thread
inline bool expdw_whole_supported(const ExpDwArgs& a, const ExpDwChoice& c, bool stamped) {
    return c.exp && c.proj && c.k == 3 && c.stride == 1 && a.pad == 1 && c.oh == EXPDW_WHOLE_OH && c.ow == EXPDW_WHOLE_OW && a.cin == EXPDW_WHOLE_CIN && !a.pool && !stamped &&
           a.cexp % 8 == 0 && a.cexp >= 8 && a.cexp <= EXPDW_WHOLE_CEXP_MAX && expdw_whole_lds(a.cexp) <= EXPDW_PERSIST_LDS_MAX && 9 * (a.cexp >> 3) <= EXPDW_NT &&
           a.cout % 8 == 0 && a.cout >= 8 && a.cout <= 256 && (EXPDW_WHOLE_DROWS / 32) * dn_cdiv(a.cout, 32) <= EXPDW_NT / 64 && c.stage_out &&
           (size_t)c.oh * c.ow * a.cout <= (size_t)EXPDW_WHOLE_ROWS * a.cexp && c.zsplit == 1;
}

// `a` as launch_expdw has validated it (its DN_REQUIREs; the launcher-filled fields are not read). stamped: a dev build with phase stamps armed
// (dn_debug_expdw_stamps) -- it takes neither the persistent form nor the two other bodies.
inline ExpDwChoice expdw_choose(const ExpDwArgs& a, bool stamped) {
    ExpDwChoice c;
    c.k = a.k; c.stride = a.stride; c.exp = a.w1 != nullptr; c.proj = a.w3 != nullptr;
    c.xw = ((a.cin + 15) / 16) * 16 + 8;                    // round16(cin) + 8
    expdw_tile(a.Ho, a.Wo, a.stride, c.proj ? a.cout : 0, &c.oh, &c.ow);
    // The A fragments of the expand live in registers: 2 full K steps + the tail/bias step cover cin <= 40 (fewer registers -> more waves), then 5 (cin <= 88), 6
    // (cin 96, with a project stage) or all 8. The block shapes of the backbones get compile-time X row widths: cin 8 / 16 (24 halfs; with a project stage),
    // 24 / 32 (40), 40 (56), 80 (88: the 20 x 20 blocks and the squeeze-excitation blocks of the 20 x 20 / 10 x 10 maps), 96 (104; with a project stage).
    // (cin 48 has 56-half rows too and takes that rung, as it always has, although it has three full K steps: no model has that width.)
    if (!c.exp) { c.ksm = 2; c.xw8 = 0; }
    else if (c.xw == 24) { c.ksm = 2; c.xw8 = c.proj ? 3 : 0; }
    else if (c.xw == 40) { c.ksm = 2; c.xw8 = 5; }
    else if (c.xw == 56) { c.ksm = 2; c.xw8 = 7; }
    else if (c.xw == 88) { c.ksm = 5; c.xw8 = 11; }
    else if (c.proj && a.cin <= 88) { c.ksm = 5; c.xw8 = 0; }
    else if (c.proj && c.xw == 104) { c.ksm = 6; c.xw8 = 13; }
    else { c.ksm = EXPDW_XKS; c.xw8 = 0; }
    // LDS of expdw_kernel: X rows (+ 8 zero halfs), the E tile, the chunk's depthwise weights, the depthwise output (project only); depthwise bias, pooled-sum
    // scratch, project bias
    const int rows = expdw_region_rows(a.k, a.stride, c.oh, c.ow), drows = (c.oh * c.ow + 31) / 32 * 32, kk = a.k * a.k;
    c.lds = ((size_t)rows * c.xw + 8 + (c.exp ? (size_t)rows * EXPDW_EW : 0) + kk * EXPDW_EW + (c.proj ? (size_t)drows * EXPDW_EW : 0)) * sizeof(half_t) +
            (EXPDW_EW + EXPDW_NT / 64 * 64 + (c.proj ? 256 : 0)) * sizeof(float);
    c.lds_p = c.lds + (size_t)c.oh * c.ow * a.cout * sizeof(half_t);
    // chunks per workgroup (not split with a project stage: it sums over all chunks inside the workgroup)
    const int tiles_y = dn_cdiv(a.Ho, c.oh), tiles = dn_cdiv(a.Wo, c.ow) * tiles_y, chunks = dn_cdiv(a.cexp, 64);
    c.cpw = chunks;
    while (!c.proj && c.cpw > 1 && (long)tiles * a.n * dn_cdiv(chunks, c.cpw) < EXPDW_MIN_WGS) --c.cpw;
    c.zsplit = dn_cdiv(chunks, c.cpw);
    if (c.proj) {
        // the output tile is staged over the E .. depthwise-output buffers (everything between the X rows and the project bias)
        const size_t avail = ((c.exp ? (size_t)rows * EXPDW_EW : 0) + kk * EXPDW_EW + (size_t)drows * EXPDW_EW) * sizeof(half_t) + (EXPDW_EW + EXPDW_NT / 64 * 64) * sizeof(float);
        c.stage_out = (size_t)c.oh * c.ow * a.cout * sizeof(half_t) <= avail && a.cout % 8 == 0 && fd_ok((unsigned long long)c.oh * c.ow * (a.cout >> 3), (unsigned)(a.cout >> 3));
    }
    // The whole expanded width as ONE chunk (full blocks with at most two K steps): the chunk loop is not a loop. The wide variant (a last chunk of 72 channels
    // taken whole) exists for the one shape that uses it: the whole expanded width IS that chunk (24 -> 72 -> 24). As a tail of a longer chunk run (cexp = 136,
    // 200 ... with cin <= 40) it was never dispatched by the model zoo and every such instantiation spilled 36 - 76 B per lane at the 128-register cap: not
    // instantiated.
    const bool full = c.exp && c.proj && c.ksm <= 2, one_knob = dn_knob("DN_EXPDW_ONE", 1) != 0;
    c.wide = full && a.cexp == EXPDW_EW && one_knob;
    const bool one_chunk = full && (c.wide || a.cexp <= 64);
    // ... walked by the resident workgroups (DN_EXPDW_PERSIST), else by one workgroup per tile (DN_EXPDW_ONE; 0: the chunk loop's general form, 72 channels as 64 + 8)
    const bool persist = one_chunk && expdw_persist_supported(a, c, stamped) && dn_knob("DN_EXPDW_PERSIST", 1);
    c.one = one_chunk && (persist || one_knob);
    const bool fits = c.lds <= EXPDW_LDS_MAX && (long)tiles_y * c.zsplit <= 65535 && a.n <= 65535 && (c.exp || c.proj) &&
                      (!c.proj || (drows / 32) * dn_cdiv(a.cout, 32) <= EXPDW_NT / 64);
    c.body = !fits ? ExpDwChoice::NONE : persist ? ExpDwChoice::ONE_PERSIST : ExpDwChoice::TILED;
    if (persist) snprintf(c.label, sizeof c.label, "expdw_one_kernel<%d,%d,%d,%d,%d>", c.k, c.stride, c.oh, c.ow, c.ksm);
    else snprintf(c.label, sizeof c.label, "expdw_kernel<%d,%d,%d,%d,%d,%s,%s>", c.k, c.stride, c.oh, c.ow, c.ksm, c.exp ? "true" : "false", c.proj ? "true" : "false");
    // The two other bodies replace body and band, never the label. The per-tap body for the one-chunk stride-2 block 16 -> 64 -> cout, then the row-reuse body
    // for the one-chunk stride-1 block 24 -> 72 -> cout; *_band: output rows per band, 0 = not that body's shape.
    if (!stamped && dn_knob("DN_EXPDW_DIRECT", 1)) {
        if (const int bh = expdw_direct_band(a)) { c.body = ExpDwChoice::DIRECT; c.band = bh; return c; }
    }
    if (!stamped && dn_knob("DN_EXPDW_ROWS", 1)) {
        if (const int bh = expdw_rows_band(a)) { c.body = ExpDwChoice::ROWS; c.band = bh; return c; }
    }
    // The whole-width form of the tiled body: a flag like `one` and `wide` -- body, label, band and tile stay. DN_EXPDW_WHOLE: 1 = the shapes measured faster
    // on MI355X, which are the two multi-chunk widths of the 20 x 20 blocks of MobileNetV3, 200 (four passes of the chunk loop, the last for 8 channels) and 184
    // (three); every other width the form can run keeps the chunk loop until someone measures it. 0 = never, 2 = wherever it can run (tests, A/B).
    if (c.body == ExpDwChoice::TILED && !c.one && expdw_whole_supported(a, c, stamped)) {
        c.lds_w = expdw_whole_lds(a.cexp);
        const int knob = dn_knob("DN_EXPDW_WHOLE", 1);
        c.whole = knob >= 2 || (knob == 1 && (a.cexp == 200 || a.cexp == 184));
    }
    return c;
}

// ================================================================ a request that the chosen kernel does not implement is an error, not a launch
inline int pw_check_honoured(const PwArgs& a, const PwChoice& c, const char* who) {
    const char* field = (a.sef_part && !c.sef) ? "sef_part" : (a.w_b && !c.head) ? "w_b" : (a.pool_out && !c.pool) ? "pool_out" : nullptr;
    if (!field) return DN_OK;
    dn_set_error("%s: no kernel implements %s for cin=%d cout=%d on %d rows of %d per image (k=%d)", who, field, a.cv_k > 1 ? a.cv_cin : a.cin, a.cout, a.m, a.hw, a.cv_k);
    return DN_E_UNSUPPORTED;
}

// the kernels of the other two files, behind their part of the switch
int launch_pw_direct(const PwArgs& a, const PwChoice& c, hipStream_t s);      // PW_WSTAT, PW_STREAM, PW_DIRECT (pwdirect.hip)
int launch_conv_big(const PwArgs& a, const PwChoice& c, hipStream_t s);       // CONV_PATCH, CONV_PATCH_RESIDENT, CONV_HALO, CONV_GLDS (convbig.hip)
