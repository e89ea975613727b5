// The frame step of the device tracker: the one definition shared by track.hip (dn_track_update: ByteTrack's BYTETracker.update,
// Zhang et al. 2022, with its constant-velocity Kalman filter, for B independent streams in ONE launch) and trackapp.hip
// (dn_track_update_appearance: the same step with BoT-SORT's appearance term fused into the pair value). The semantics, sentence by sentence, are
// in include/demonet_hip.h and restated in tests/track_ref.py and tests/track_appearance_ref.py; this file must agree with them bit for bit.
// This header has the constants, the argument records, the filter / IoU / scan helpers and the host-side argument checks; trackstep.inc has the
// kernel body, which both kernels include as text (why: see there).
//   one workgroup of 256 threads per stream. Thread t OWNS track slot t: its 20 filter floats and its bookkeeping live in registers for the whole
//   step. The stream's state block comes into LDS by 16-byte loads and leaves by 16-byte stores; the frame's detections (boxes by 16-byte loads)
//   sit in LDS beside it.
//   association (stages 1 - 3) = rounds of locally dominant pairs: every free track scans the free detections of the stage for its best one
//   (IoU descending, row ascending), every detection that got a proposal scans the free tracks for its best one (IoU descending, slot ascending),
//   and the pairs that chose each other are matched. Under the total order (IoU descending, slot ascending, row ascending) those are exactly the
//   pairs the sequential greedy walk takes; the largest pair left is always among them, so the rounds end after at most min(tracks, detections).
//   Both sides evaluate the SAME function of (track box, detection box), so they see the same bits. The T x D matrix is never stored.
//   A stage's first track-side scan also leaves every row its best track (an integer maximum in LDS), so a row scans only after losing it.
//   new tracks = two block-wide prefix scans (ballot + popcount per wave, the wave totals through LDS): the r-th starting detection in row order
//   takes the r-th free slot in slot order.
// Compiled with -ffp-contract=off: every operation of the header's text rounds once. No inline asm, no float atomics (the one atomic is an
// unsigned maximum in LDS), no scratch.
#pragma once
#include "detset.h"

namespace {

constexpr int TK_NT = 256;                 // threads of the workgroup = the largest track table
constexpr int TK_MAX_D = 512;              // detection rows per stream
constexpr int TK_WAVES = TK_NT / 64;
constexpr int TK_SCAN = 8;                 // rows (slots) a thread examines per step of a scan; divides TK_MAX_D and TK_NT
constexpr int TK_HDR = 4;                  // words of the per-stream header
constexpr int TK_SLOT_WORDS = 28;          // words per slot: state, id, label (2), score, 20 filter floats, start, last, det
enum { TK_FREE = 0, TK_TENTATIVE = 1, TK_TRACKED = 2, TK_LOST = 3 };
enum { TK_NONE = 0, TK_HIGH = 1, TK_LOW = 2 };

inline int tk_padded(int max_tracks) { return (max_tracks + 3) & ~3; }
inline size_t tk_stream_words(int max_tracks) { return (size_t)TK_HDR + (size_t)TK_SLOT_WORDS * tk_padded(max_tracks); }

struct TrackArgs {
    const float4* boxes; const float* scores; const int64_t* labels; const int32_t* counts;
    uint4* state;
    float4* boxes_out; float* scores_out; int64_t* labels_out; int64_t* ids_out; int32_t* det_out; int32_t* counts_out; int64_t* det_ids_out;
    int d, T, Tp;
    float track_thresh, low_thresh, new_thresh;
    float gate1, gate2, gate3;             // 1 - match_thresh, 1 - second_thresh, 1 - unconfirmed_thresh: one fp32 subtraction each, on the host
    int track_buffer, class_agnostic;
};

// IoU of a track's box a with a detection's box b: the intersection is dn_merge_detections' own (dn_box_inter, the track as a_i), the rest its
// DN_MERGE_IOU order
__device__ __forceinline__ float tk_iou(const float4 a, const float4 b) {
    const float inter = dn_box_inter(a, b);
    if (!(inter > 0.0f)) return -1.0f;      // u would be 0 or NaN: below every gate (the gates are >= 0), and the division is the costly part
    const float aa = (a.z - a.x) * (a.w - a.y);
    const float ab = (b.z - b.x) * (b.w - b.y);
    return inter / ((aa + ab) - inter);
}

// What the appearance step adds to a frame step (trackapp.hip). map == nullptr: a step without embeddings (no row has one; S, en and epres are
// not read).
struct TrackAppArgs {
    const float* S;                        // [B][Tp][d], written by track_sim_kernel in front of this launch
    const int32_t* map;                    // [B][d]: the embedding slot of the row, -1 none
    const int32_t* epres;                  // [E]: the slot's embedding is present
    const half_t* en;                      // [E][dim]: the normalised rows
    int32_t* fflag;                        // the feature buffer: per stream int32 valid [Tp], then fp32 feature [Tp][dim]
    int dim;
    float alpha, beta;                     // beta = 1 - alpha: one fp32 subtraction, on the host
    float app_thresh, prox_thresh;
};
enum { TK_F_NONE = 0, TK_F_CLEAR = 1, TK_F_INIT = 2, TK_F_EMA = 3 };     // what the step's tail does to a slot's feature

// The fused pair value of stages 1 and 3 for a pair whose track AND row have a feature (include/demonet_hip.h): u is the IoU in full (no
// shortcut for an empty intersection: appearance may admit such a pair), e = max((1 - S) / 2, 0) with a NaN kept, admissible = e <= app_thresh
// and 1 - u <= prox_thresh (a NaN compares false), v = admissible ? max(u, 1 - e) : u. Both sides of the association call this one function.
__device__ __forceinline__ float tk_fused(const float4 a, const float4 b, const float s, const float app_thresh, const float prox_thresh) {
    const float inter = dn_box_inter(a, b);
    const float aa = (a.z - a.x) * (a.w - a.y);
    const float ab = (b.z - b.x) * (b.w - b.y);
    const float u = inter / ((aa + ab) - inter);
    const float h = (1.0f - s) * 0.5f;
    const float e = h < 0.0f ? 0.0f : h;
    const bool adm = e <= app_thresh && (1.0f - u) <= prox_thresh;
    const float w = 1.0f - e;
    return adm ? (u > w ? u : w) : u;
}

constexpr float TK_WP = 0.05f, TK_WV = 0.00625f;      // 1 / 20 and 1 / 160, rounded to fp32

// box -> measurement (cx, cy, a, h)
__device__ __forceinline__ void tk_measure(const float4 b, float (&z)[4]) {
    const float w = b.z - b.x, h = b.w - b.y;
    z[0] = b.x + w * 0.5f;
    z[1] = b.y + h * 0.5f;
    z[2] = w / h;
    z[3] = h;
}

// mean -> box
__device__ __forceinline__ float4 tk_box(const float (&f)[20]) {
    const float h = f[15], w = f[10] * h;
    const float x1 = f[0] - w * 0.5f, y1 = f[5] - h * 0.5f;
    return make_float4(x1, y1, x1 + w, y1 + h);
}

// coordinate k of the filter: f[5 k + (0 x, 1 v, 2 Pxx, 3 Pxv, 4 Pvv)]
__device__ __forceinline__ void tk_init(float (&f)[20], const float4 b) {
    float z[4];
    tk_measure(b, z);
    const float h = z[3];
    const float sp = TK_WP * h, sv = TK_WV * h;
    const float p2 = 2.0f * sp, v10 = 10.0f * sv;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f[5 * k + 0] = z[k];
        f[5 * k + 1] = 0.0f;
        f[5 * k + 2] = k == 2 ? 1e-2f * 1e-2f : p2 * p2;
        f[5 * k + 3] = 0.0f;
        f[5 * k + 4] = k == 2 ? 1e-5f * 1e-5f : v10 * v10;
    }
}

__device__ __forceinline__ void tk_predict(float (&f)[20]) {
    const float h = f[15];
    const float sp = TK_WP * h, sv = TK_WV * h;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float qp = k == 2 ? 1e-2f * 1e-2f : sp * sp;
        const float qv = k == 2 ? 1e-5f * 1e-5f : sv * sv;
        const float pxx = f[5 * k + 2], pxv = f[5 * k + 3], pvv = f[5 * k + 4];
        f[5 * k + 0] = f[5 * k + 0] + f[5 * k + 1];
        f[5 * k + 2] = ((pxx + 2.0f * pxv) + pvv) + qp;
        f[5 * k + 3] = pxv + pvv;
        f[5 * k + 4] = pvv + qv;
    }
}

__device__ __forceinline__ void tk_update(float (&f)[20], const float4 b) {
    float z[4];
    tk_measure(b, z);
    const float h = f[15];
    const float sp = TK_WP * h;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float r = k == 2 ? 1e-1f * 1e-1f : sp * sp;
        const float pxx = f[5 * k + 2], pxv = f[5 * k + 3], pvv = f[5 * k + 4];
        const float S = pxx + r;
        const float kx = pxx / S, kv = pxv / S;
        const float y = z[k] - f[5 * k + 0];
        f[5 * k + 0] = f[5 * k + 0] + kx * y;
        f[5 * k + 1] = f[5 * k + 1] + kv * y;
        const float ks = kx * S, vs = kv * S;
        f[5 * k + 2] = pxx - ks * kx;
        f[5 * k + 3] = pxv - ks * kv;
        f[5 * k + 4] = pvv - vs * kv;
    }
}

// exclusive prefix count of `flag` over the workgroup in thread order, and the total. wtot: TK_WAVES ints of LDS, free for reuse on return.
__device__ __forceinline__ int tk_scan(const bool flag, int* wtot, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) wtot[wave] = __popcll(m);
    __syncthreads();
    int before = __popcll(m & ((1ull << lane) - 1ull));
    int sum = 0;
#pragma unroll
    for (int w = 0; w < TK_WAVES; ++w) {
        const int c = wtot[w];
        if (w < wave) before += c;
        sum += c;
    }
    total = sum;
    __syncthreads();
    return before;
}

inline bool tk_number(float v) { return v >= 0.0f; }      // (a NaN compares false)

// Everything dn_track_update checks before it launches, under the caller's name `who`, and the kernel's arguments; DN_OK or the error code.
inline int tk_check_step(const char* who, const float* boxes, const float* scores, const int64_t* labels, const int32_t* counts, int streams, int d,
                         const dn_track_params* params, void* state, size_t state_bytes, float* boxes_out, float* scores_out, int64_t* labels_out,
                         int64_t* ids_out, int32_t* det_out, int32_t* counts_out, int64_t* det_ids_out, TrackArgs& a) {
    DN_REQUIRE(boxes && scores && labels && counts && params && state && boxes_out && scores_out && labels_out && ids_out && det_out && counts_out &&
                   det_ids_out, "%s: null argument", who);
    const dn_track_params& p = *params;
    DN_REQUIRE(streams >= 1 && d >= 1 && p.max_tracks >= 1, "%s: bad sizes streams=%d d=%d max_tracks=%d", who, streams, d, p.max_tracks);
    DN_REQUIRE(tk_number(p.track_thresh) && tk_number(p.low_thresh) && tk_number(p.new_thresh) && tk_number(p.match_thresh) &&
                   tk_number(p.second_thresh) && tk_number(p.unconfirmed_thresh),
               "%s: the thresholds must be numbers >= 0 (track %g low %g new %g match %g second %g unconfirmed %g)", who, (double)p.track_thresh,
               (double)p.low_thresh, (double)p.new_thresh, (double)p.match_thresh, (double)p.second_thresh, (double)p.unconfirmed_thresh);
    DN_REQUIRE(p.match_thresh <= 1.0f && p.second_thresh <= 1.0f && p.unconfirmed_thresh <= 1.0f,
               "%s: match_thresh=%g, second_thresh=%g and unconfirmed_thresh=%g are costs 1 - IoU: at most 1", who, (double)p.match_thresh,
               (double)p.second_thresh, (double)p.unconfirmed_thresh);
    DN_REQUIRE(p.track_buffer >= 0, "%s: track_buffer=%d must not be negative", who, p.track_buffer);
    DN_REQUIRE(((reinterpret_cast<size_t>(boxes) | reinterpret_cast<size_t>(boxes_out) | reinterpret_cast<size_t>(state)) & 15) == 0 &&
                   ((reinterpret_cast<size_t>(labels) | reinterpret_cast<size_t>(labels_out) | reinterpret_cast<size_t>(ids_out) |
                     reinterpret_cast<size_t>(det_ids_out)) & 7) == 0 &&
                   ((reinterpret_cast<size_t>(scores) | reinterpret_cast<size_t>(counts) | reinterpret_cast<size_t>(scores_out) |
                     reinterpret_cast<size_t>(det_out) | reinterpret_cast<size_t>(counts_out)) & 3) == 0,
               "%s: boxes, boxes_out and the state must be 16-byte aligned, labels, ids and det_ids 8-byte aligned, the others 4-byte aligned", who);
    if (d > TK_MAX_D || p.max_tracks > TK_NT) {
        dn_set_error("%s: d=%d at most %d, max_tracks=%d at most %d", who, d, TK_MAX_D, p.max_tracks, TK_NT);
        return DN_E_UNSUPPORTED;
    }
    const size_t need = (size_t)streams * tk_stream_words(p.max_tracks) * 4;
    if (state_bytes < need) {
        dn_set_error("%s: state of %zu B, %zu B needed", who, state_bytes, need);
        return DN_E_WORKSPACE;
    }
    a.boxes = reinterpret_cast<const float4*>(boxes); a.scores = scores; a.labels = labels; a.counts = counts;
    a.state = reinterpret_cast<uint4*>(state);
    a.boxes_out = reinterpret_cast<float4*>(boxes_out); a.scores_out = scores_out; a.labels_out = labels_out; a.ids_out = ids_out;
    a.det_out = det_out; a.counts_out = counts_out; a.det_ids_out = det_ids_out;
    a.d = d; a.T = p.max_tracks; a.Tp = tk_padded(p.max_tracks);
    a.track_thresh = p.track_thresh; a.low_thresh = p.low_thresh; a.new_thresh = p.new_thresh;
    a.gate1 = 1.0f - p.match_thresh; a.gate2 = 1.0f - p.second_thresh; a.gate3 = 1.0f - p.unconfirmed_thresh;
    a.track_buffer = p.track_buffer; a.class_agnostic = p.class_agnostic;
    return DN_OK;
}

}  // namespace

