// Line-crossing and zone analytics behind the tracker: dn_zone_update accumulates, per stream, directed line counts, zone entries /
// exits / vanishings / occupancy / dwell and a short event list from the tracker's state of the frame; dn_zone_reset clears streams. The semantics,
// rule by rule, are in include/demonet_hip.h and restated in tests/zones_ref.py; this file must agree with them bit for bit.
//   one workgroup of 256 threads per stream. Thread t OWNS slot t of the tracker and of the zone state: it reads the tracker's fields of its slot
//   straight from global memory (the per-slot arrays are contiguous in t), decides what happened to it -- three 16-bit masks: vanished zones, crossed
//   lines with their directions, zones entered or left -- and counts its events. The stream's configuration record and its counters sit in LDS:
//   every thread walks the same lines and vertices (broadcast reads), and the counters meet through LDS integer atomics, whose sums do not depend on
//   the order. A block-wide prefix scan of the per-slot event counts gives every event its row, so the list's order is fixed.
// Compiled with -ffp-contract=off: every operation of the header's text rounds once. No inline asm, no float atomics, no workspace; the tracker's
// state is only read.
#include <stddef.h>

#include "common.h"

namespace {

constexpr int ZN_NT = 256;                 // threads of the workgroup = the largest track table
constexpr int ZN_WAVES = ZN_NT / 64;
constexpr int ZN_MAX_EVENTS = 1024;
constexpr int ZN_HDR = 4;                  // words of the per-stream header
constexpr int ZN_SLOT_WORDS = 22;          // words per slot: id, bin, has_prev, px, py, inside, enter_frame[16]
constexpr int ZN_CNT_WORDS = 1152;         // words of the counters
constexpr int ZN_CFG_WORDS = (int)(sizeof(dn_zone_config) / 4);
// the counters, in words from their start
enum { ZC_LINE = 0, ZC_ENTRIES = 256, ZC_EXITS = 384, ZC_VANISHED = 512, ZC_OCC = 640, ZC_DMAX = 768, ZC_DSUM = 896 };
// the configuration record, in words
enum { ZF_NLINES = 0, ZF_LINES = 1, ZF_NZONES = 65, ZF_NV = 66, ZF_VERTS = 82 };
static_assert(sizeof(dn_zone_config) == 2384 && sizeof(dn_zone_config) % 16 == 0, "dn_zone_config: the header pins 2384 bytes");
static_assert(offsetof(dn_zone_config, n_lines) == 4 * ZF_NLINES && offsetof(dn_zone_config, lines) == 4 * ZF_LINES &&
                  offsetof(dn_zone_config, n_zones) == 4 * ZF_NZONES && offsetof(dn_zone_config, nv) == 4 * ZF_NV &&
                  offsetof(dn_zone_config, verts) == 4 * ZF_VERTS && offsetof(dn_zone_config, reserved) == 2376,
              "dn_zone_config: the header pins these offsets");
static_assert(ZC_DSUM + 2 * 128 == ZN_CNT_WORDS && ZC_OCC % 4 == 0 && ZC_DMAX % 4 == 0 && ZC_DSUM % 2 == 0, "the counters' layout");

// the tracker's layout (include/demonet_hip.h, dn_track_update): 4 header words, then per-slot arrays of Tp entries
constexpr int TK_HDR = 4, TK_SLOT_WORDS = 28;

inline int zn_padded(int max_tracks) { return (max_tracks + 3) & ~3; }
inline size_t zn_stream_words(int max_tracks) { return (size_t)ZN_HDR + (size_t)ZN_SLOT_WORDS * zn_padded(max_tracks) + ZN_CNT_WORDS; }

struct ZoneArgs {
    const int32_t* track;
    const uint4* config;
    const uint8_t* class_bin;
    uint4* zstate;
    int4* events;
    int32_t* counts;
    int T, Tp, n_labels, anchor, max_events;
};

// exclusive prefix sum of v over the workgroup in thread order, and the total. wtot: ZN_WAVES ints of LDS.
__device__ __forceinline__ int zn_scan(const int v, int* wtot, int& total) {
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
    for (int w = 0; w < ZN_WAVES; ++w) {
        const int c = wtot[w];
        if (w < wave) before += c;
        sum += c;
    }
    total = sum;
    return before;
}

__device__ __forceinline__ float zn_side(float ax, float ay, float bx, float by, float px, float py) {
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}

__device__ __forceinline__ bool zn_finite(float v) { return fabsf(v) < INFINITY; }

__device__ __forceinline__ int zn_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(ZN_NT) void zone_update_kernel(const ZoneArgs a) {
    __shared__ uint4 cfg4[ZN_CFG_WORDS / 4];   // the stream's configuration record
    __shared__ uint4 cnt4[ZN_CNT_WORDS / 4];   // the stream's counters, as they lie in memory
    __shared__ int wtot[ZN_WAVES];

    const int b = blockIdx.x, t = threadIdx.x;
    const int T = a.T, Tp = a.Tp;
    const int32_t* const tk = a.track + (size_t)b * (TK_HDR + TK_SLOT_WORDS * Tp);
    const int zwords = ZN_HDR + ZN_SLOT_WORDS * Tp + ZN_CNT_WORDS;
    const int cbase = ZN_HDR + ZN_SLOT_WORDS * Tp;                    // (a multiple of 4: Tp is)
    uint4* const gz4 = a.zstate + (size_t)b * (zwords / 4);
    int* const gzi = reinterpret_cast<int*>(gz4);
    float* const gzf = reinterpret_cast<float*>(gz4);
    const int oId = ZN_HDR, oBin = ZN_HDR + Tp, oHas = ZN_HDR + 2 * Tp, oPx = ZN_HDR + 3 * Tp, oPy = ZN_HDR + 4 * Tp, oIn = ZN_HDR + 5 * Tp,
              oEnter = ZN_HDR + 6 * Tp;

    for (int i = t; i < ZN_CFG_WORDS / 4; i += ZN_NT) cfg4[i] = a.config[(size_t)b * (ZN_CFG_WORDS / 4) + i];
    // 4. the occupancy is rewritten every step: it starts from zero
    for (int i = t; i < ZN_CNT_WORDS / 4; i += ZN_NT)
        cnt4[i] = (i >= ZC_OCC / 4 && i < ZC_DMAX / 4) ? make_uint4(0u, 0u, 0u, 0u) : gz4[cbase / 4 + i];
    __syncthreads();
    const int* const cfgi = reinterpret_cast<const int*>(cfg4);
    const float* const cfgf = reinterpret_cast<const float*>(cfg4);
    int* const cnt = reinterpret_cast<int*>(cnt4);
    unsigned long long* const dsum = reinterpret_cast<unsigned long long*>(cnt + ZC_DSUM);

    const int f = tk[0];                                             // the tracker's frame word
    const int n_lines = zn_clamp(cfgi[ZF_NLINES], 0, 16), n_zones = zn_clamp(cfgi[ZF_NZONES], 0, 16);

    // what happened to the own slot: the zones the old entry vanished from; the lines crossed and their directions; the zone bits before and after
    const bool slot = t < T;
    unsigned vmask = 0u, cmask = 0u, dmask = 0u, inside = 0u, newin = 0u;
    bool observed = false;
    int vid = 0, vbin = 0, tid = 0, lab = 0, bin = 255;
    if (slot) {
        const int tstate = tk[TK_HDR + t];
        tid = tk[TK_HDR + Tp + t];
        const long long label = reinterpret_cast<const long long*>(tk + TK_HDR + 2 * Tp)[t];
        const int last = tk[TK_HDR + 26 * Tp + t];
        lab = (int)label;
        int zid = gzi[oId + t];
        int has_prev = gzi[oHas + t];
        inside = (unsigned)gzi[oIn + t] & 0xFFFFu;
        // 1. a slot that is free or holds another track: the old entry is closed
        if (tstate == 0 || tid != zid) {
            vmask = inside;
            vid = zid;
            vbin = gzi[oBin + t] & 7;
            zid = tstate ? tid : 0;
            has_prev = 0;
            inside = 0u;
            gzi[oId + t] = zid;
            gzi[oHas + t] = 0;
            gzi[oIn + t] = 0;
        }
        // 2. observed?
        if (!a.class_bin) {
            bin = 0;
        } else if (label >= 0 && label < (long long)a.n_labels) {
            const int v = a.class_bin[label];
            bin = v < 8 ? v : 255;
        }
        float px = 0.0f, py = 0.0f;
        if (tstate == 2 && last == f && bin != 255) {
            const float* const flt = reinterpret_cast<const float*>(tk + TK_HDR + 5 * Tp);
            const float cx = flt[0 * Tp + t], cy = flt[5 * Tp + t], ar = flt[10 * Tp + t], h = flt[15 * Tp + t];
            // mean -> box, the tracker's operation order
            const float w = ar * h;
            const float x1 = cx - w * 0.5f, y1 = cy - h * 0.5f;
            const float x2 = x1 + w, y2 = y1 + h;
            px = (x1 + x2) * 0.5f;
            py = a.anchor == 0 ? (y1 + y2) * 0.5f : y2;
            observed = zn_finite(px) && zn_finite(py);
        }
        if (observed) {
            gzi[oBin + t] = bin;
            // 3. lines
            if (has_prev) {
                const float qx = gzf[oPx + t], qy = gzf[oPy + t];
                for (int i = 0; i < n_lines; ++i) {
                    const float ax = cfgf[ZF_LINES + 4 * i], ay = cfgf[ZF_LINES + 4 * i + 1], bx = cfgf[ZF_LINES + 4 * i + 2],
                                by = cfgf[ZF_LINES + 4 * i + 3];
                    const float sa = zn_side(ax, ay, bx, by, qx, qy), sc = zn_side(ax, ay, bx, by, px, py);
                    const float su = zn_side(qx, qy, px, py, ax, ay), sv = zn_side(qx, qy, px, py, bx, by);
                    const bool numbers = sa == sa && sc == sc && su == su && sv == sv;
                    if (numbers && ((sa >= 0.0f) != (sc >= 0.0f)) && ((su >= 0.0f) != (sv >= 0.0f))) {
                        cmask |= 1u << i;
                        if (!(sc >= 0.0f)) dmask |= 1u << i;
                    }
                }
            }
            // 4. zones, even-odd rule
            for (int z = 0; z < n_zones; ++z) {
                const int nv = zn_clamp(cfgi[ZF_NV + z], 3, 16);
                const float* const vz = cfgf + ZF_VERTS + 32 * z;
                bool in = false;
                for (int e = 0; e < nv; ++e) {
                    const int j = e ? e - 1 : nv - 1;
                    const float xi = vz[2 * e], yi = vz[2 * e + 1], xj = vz[2 * j], yj = vz[2 * j + 1];
                    if ((yi > py) != (yj > py)) {
                        const float x = (xj - xi) * (py - yi) / (yj - yi) + xi;
                        if (px < x) in = !in;
                    }
                }
                if (in) newin |= 1u << z;
            }
            // 5.
            gzf[oPx + t] = px;
            gzf[oPy + t] = py;
            gzi[oHas + t] = 1;
            gzi[oIn + t] = (int)newin;
        } else {
            newin = inside;                                          // not observed: the bits stay, nothing changes, nothing is counted
        }
    }
    const unsigned changed = inside ^ newin;

    // 6. every event's row: slot ascending, within the slot VANISH by zone, CROSS by line, EXIT / ENTER by zone
    int total;
    int pos = zn_scan(__popc(vmask) + __popc(cmask) + __popc(changed), wtot, total);
    const int max_events = a.max_events;
    int4* const ev = a.events + (size_t)b * max_events * 2;
    for (unsigned m = vmask; m; m &= m - 1u, ++pos) {
        const int z = __ffs(m) - 1;
        const int dwell = f - gzi[oEnter + z * Tp + t];
        atomicAdd(&cnt[ZC_VANISHED + 8 * z + vbin], 1);
        if (pos < max_events) {
            ev[2 * pos] = make_int4(DN_ZONE_VANISH, z, vid, -1);
            ev[2 * pos + 1] = make_int4(vbin, f, dwell, 0);
        }
    }
    for (unsigned m = cmask; m; m &= m - 1u, ++pos) {
        const int i = __ffs(m) - 1;
        const int dir = (int)((dmask >> i) & 1u);
        atomicAdd(&cnt[ZC_LINE + (2 * i + dir) * 8 + bin], 1);
        if (pos < max_events) {
            ev[2 * pos] = make_int4(DN_ZONE_CROSS, i, tid, lab);
            ev[2 * pos + 1] = make_int4(bin, f, 0, dir);
        }
    }
    for (unsigned m = changed; m; m &= m - 1u, ++pos) {
        const int z = __ffs(m) - 1;
        const bool enter = (newin >> z) & 1u;
        int dwell = 0;
        if (enter) {
            atomicAdd(&cnt[ZC_ENTRIES + 8 * z + bin], 1);
            gzi[oEnter + z * Tp + t] = f;                            // (after the VANISH of the same zone above has read the old value)
        } else {
            dwell = f - gzi[oEnter + z * Tp + t];
            atomicAdd(&cnt[ZC_EXITS + 8 * z + bin], 1);
            atomicAdd(&dsum[8 * z + bin], (unsigned long long)(long long)dwell);
            atomicMax(&cnt[ZC_DMAX + 8 * z + bin], dwell);
        }
        if (pos < max_events) {
            ev[2 * pos] = make_int4(enter ? DN_ZONE_ENTER : DN_ZONE_EXIT, z, tid, lab);
            ev[2 * pos + 1] = make_int4(bin, f, dwell, 0);
        }
    }
    if (observed)
        for (unsigned m = newin; m; m &= m - 1u) atomicAdd(&cnt[ZC_OCC + 8 * (__ffs(m) - 1) + bin], 1);

    // 7. the first max_events are kept, the rows behind them are zero, the excess is counted
    const int kept = total < max_events ? total : max_events;
    for (int r = kept + t; r < max_events; r += ZN_NT) {
        ev[2 * r] = make_int4(0, 0, 0, 0);
        ev[2 * r + 1] = make_int4(0, 0, 0, 0);
    }
    if (t == 0) {
        a.counts[b] = kept;
        gzi[0] = gzi[0] + (total - kept);
    }
    __syncthreads();
    for (int i = t; i < ZN_CNT_WORDS / 4; i += ZN_NT) gz4[cbase / 4 + i] = cnt4[i];
}

// one workgroup per stream: the selected streams become all zero
__global__ __launch_bounds__(ZN_NT) void zone_reset_kernel(uint4* __restrict__ zstate, const uint8_t* __restrict__ which, int words4) {
    const int b = blockIdx.x;
    if (which && which[b] == 0) return;
    uint4* const g = zstate + (size_t)b * words4;
    for (int i = threadIdx.x; i < words4; i += ZN_NT) g[i] = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace

extern "C" __attribute__((visibility("default"))) size_t dn_zone_state_bytes(int streams, int max_tracks) {
    if (streams < 1 || max_tracks < 1 || max_tracks > ZN_NT) return 0;
    return (size_t)streams * zn_stream_words(max_tracks) * 4;
}

extern "C" __attribute__((visibility("default"))) int dn_zone_reset(void* zstate, int streams, int max_tracks, const uint8_t* which, void* stream) {
    DN_REQUIRE(zstate, "dn_zone_reset: null state");
    DN_REQUIRE(streams >= 1 && max_tracks >= 1, "dn_zone_reset: bad sizes streams=%d max_tracks=%d", streams, max_tracks);
    DN_REQUIRE((reinterpret_cast<size_t>(zstate) & 15) == 0, "dn_zone_reset: the state must be 16-byte aligned");
    if (max_tracks > ZN_NT) {
        dn_set_error("dn_zone_reset: max_tracks=%d, at most %d", max_tracks, ZN_NT);
        return DN_E_UNSUPPORTED;
    }
    dn_note_kernel("zone_reset_kernel");
    hipLaunchKernelGGL(zone_reset_kernel, dim3(streams), dim3(ZN_NT), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<uint4*>(zstate), which,
                       (int)(zn_stream_words(max_tracks) / 4));
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}

extern "C" __attribute__((visibility("default"))) int dn_zone_update(const void* track_state, size_t track_state_bytes, int streams, int max_tracks,
                                                                    const dn_zone_config* config, const uint8_t* class_bin, int n_labels, int anchor,
                                                                    void* zstate, size_t zstate_bytes, int32_t* events_out,
                                                                    int32_t* event_counts_out, int max_events, void* stream) {
    DN_REQUIRE(track_state && config && zstate && events_out && event_counts_out, "dn_zone_update: null argument");
    DN_REQUIRE(streams >= 1 && max_tracks >= 1 && max_events >= 1 && (!class_bin || n_labels >= 1),
               "dn_zone_update: bad sizes streams=%d max_tracks=%d max_events=%d n_labels=%d", streams, max_tracks, max_events, n_labels);
    DN_REQUIRE(anchor == 0 || anchor == 1, "dn_zone_update: anchor=%d, 0 (box centre) or 1 (bottom centre)", anchor);
    DN_REQUIRE(((reinterpret_cast<size_t>(track_state) | reinterpret_cast<size_t>(config) | reinterpret_cast<size_t>(zstate) |
                 reinterpret_cast<size_t>(events_out)) & 15) == 0 && (reinterpret_cast<size_t>(event_counts_out) & 3) == 0,
               "dn_zone_update: the tracker's state, the configuration, the zone state and the events must be 16-byte aligned, the counts 4-byte aligned");
    if (max_tracks > ZN_NT || max_events > ZN_MAX_EVENTS) {
        dn_set_error("dn_zone_update: max_tracks=%d at most %d, max_events=%d at most %d", max_tracks, ZN_NT, max_events, ZN_MAX_EVENTS);
        return DN_E_UNSUPPORTED;
    }
    const size_t tneed = dn_track_state_bytes(streams, max_tracks);
    DN_REQUIRE(track_state_bytes >= tneed, "dn_zone_update: a tracker state of %zu B, dn_track_state_bytes gives %zu B", track_state_bytes, tneed);
    const size_t need = dn_zone_state_bytes(streams, max_tracks);
    if (zstate_bytes < need) {
        dn_set_error("dn_zone_update: zone state of %zu B, %zu B needed", zstate_bytes, need);
        return DN_E_WORKSPACE;
    }
    ZoneArgs a;
    a.track = reinterpret_cast<const int32_t*>(track_state);
    a.config = reinterpret_cast<const uint4*>(config);
    a.class_bin = class_bin;
    a.zstate = reinterpret_cast<uint4*>(zstate);
    a.events = reinterpret_cast<int4*>(events_out);
    a.counts = event_counts_out;
    a.T = max_tracks; a.Tp = zn_padded(max_tracks); a.n_labels = n_labels; a.anchor = anchor; a.max_events = max_events;
    dn_note_kernel("zone_update_kernel");
    hipLaunchKernelGGL(zone_update_kernel, dim3(streams), dim3(ZN_NT), 0, reinterpret_cast<hipStream_t>(stream), a);
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}
