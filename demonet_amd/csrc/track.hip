// Multi-object tracking on the device: dn_track_update is ByteTrack's BYTETracker.update (Zhang et al. 2022) with its constant-velocity
// Kalman filter for B independent streams in ONE launch per frame step; dn_track_reset restarts streams. The semantics, sentence by sentence, are
// in include/demonet_hip.h and restated in tests/track_ref.py; this file must agree with them bit for bit.
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

__global__ __launch_bounds__(TK_NT) void track_update_kernel(const TrackArgs a) {
    __shared__ uint4 st4[1 + 7 * TK_NT];       // the stream's state block, as it lies in memory
    __shared__ float4 dbox[TK_MAX_D];
    __shared__ long long dlab[TK_MAX_D];
    __shared__ float dscore[TK_MAX_D];
    __shared__ int dcls[TK_MAX_D];             // TK_NONE / TK_HIGH / TK_LOW; TK_NONE again once a track has taken the row
    __shared__ int did[TK_MAX_D];              // -1: free; otherwise the id of the track that took the row
    __shared__ int dhas[TK_MAX_D];             // this round: some track proposed to the row
    __shared__ int dprop[TK_MAX_D];            // this stage: the row's best track when it was last scanned, -1 nobody, -2 not scanned yet
    __shared__ unsigned long long dkey[TK_MAX_D];   // this stage: the largest (IoU bits, ~slot) over the admissible pairs of the row, 0 none
    __shared__ float4 tbox[TK_NT];
    __shared__ long long tlab[TK_NT];
    __shared__ int tact[TK_NT];                // the slot takes part in the current stage and is still unmatched
    __shared__ int detlist[TK_NT];             // r -> row of the r-th starting detection
    __shared__ int wtot[TK_WAVES];

    const int b = blockIdx.x, t = threadIdx.x;
    const int T = a.T, Tp = a.Tp, d = a.d;
    const int words = TK_HDR + TK_SLOT_WORDS * Tp;
    uint4* const gstate = a.state + (size_t)b * (words / 4);
    int* const sti = reinterpret_cast<int*>(st4);
    float* const stf = reinterpret_cast<float*>(st4);
    const int oState = TK_HDR, oId = TK_HDR + Tp, oLabel = TK_HDR + 2 * Tp, oScore = TK_HDR + 4 * Tp, oFilt = TK_HDR + 5 * Tp,
              oStart = TK_HDR + 25 * Tp, oLast = TK_HDR + 26 * Tp, oDet = TK_HDR + 27 * Tp;

    for (int i = t; i < words / 4; i += TK_NT) st4[i] = gstate[i];
    int n = a.counts[b];
    n = n < 0 ? 0 : (n > d ? d : n);
    for (int j = t; j < TK_MAX_D; j += TK_NT) {
        int cls = TK_NONE;
        if (j < n) {
            const size_t g = (size_t)b * d + j;
            const float4 bx = a.boxes[g];
            const float s = a.scores[g];
            dbox[j] = bx;
            dscore[j] = s;
            dlab[j] = a.labels[g];
            const bool fin = fabsf(bx.x) < INFINITY && fabsf(bx.y) < INFINITY && fabsf(bx.z) < INFINITY && fabsf(bx.w) < INFINITY;
            const bool ok = s == s && fin && (bx.z - bx.x) > 0.0f && (bx.w - bx.y) > 0.0f;
            if (ok) cls = s >= a.track_thresh ? TK_HIGH : ((s > a.low_thresh && s < a.track_thresh) ? TK_LOW : TK_NONE);
        }
        dcls[j] = cls;
        did[j] = -1;
        dhas[j] = 0;
    }
    __syncthreads();

    // 1. the header and the own slot
    const int frame = sti[0] + 1;
    const int next_id = sti[1];
    int dropped = sti[2];
    const bool slot = t < T;
    int state = TK_FREE, id = 0, start = 0, last = 0, det = 0;
    long long label = 0;
    float score = 0.0f;
    float f[20];
#pragma unroll
    for (int i = 0; i < 20; ++i) f[i] = 0.0f;
    if (slot) {
        state = sti[oState + t];
        id = sti[oId + t];
        label = reinterpret_cast<const long long*>(sti + oLabel)[t];
        score = stf[oScore + t];
#pragma unroll
        for (int i = 0; i < 20; ++i) f[i] = stf[oFilt + i * Tp + t];
        start = sti[oStart + t];
        last = sti[oLast + t];
        det = state == TK_FREE ? 0 : -1;
    }

    // 3. predict the tracked and the lost tracks (a lost track's velocity of h is cleared first); tentative tracks stay as they are
    if (state == TK_LOST) f[16] = 0.0f;
    if (state == TK_TRACKED || state == TK_LOST) tk_predict(f);
    tbox[t] = tk_box(f);
    tlab[t] = label;

    const bool agn = a.class_agnostic != 0;
    const int before = state;                  // the state this frame began with
    bool matched = false;
    for (int stage = 1; stage <= 3; ++stage) {
        const int cls = stage == 2 ? TK_LOW : TK_HIGH;
        const float gate = stage == 1 ? a.gate1 : (stage == 2 ? a.gate2 : a.gate3);
        bool active = stage == 1 ? (before == TK_TRACKED || before == TK_LOST)
                                 : (stage == 2 ? (before == TK_TRACKED && !matched) : before == TK_TENTATIVE);
        tact[t] = active ? 1 : 0;
        for (int j = t; j < n; j += TK_NT) {
            dprop[j] = -2;                                            // not looked at yet in this stage
            dkey[j] = 0ull;
        }
        __syncthreads();
        const float4 mybox = tbox[t];
        // Within a stage the free sets only shrink, so a side's best partner stays its best until somebody else takes it: a track scans again
        // only when its detection is gone, a detection only when its track is (and none at all once a scan found nobody).
        // The first scan of a stage sees every admissible pair of the stage, so it also leaves every row its best track: an integer maximum
        // in LDS over (IoU bits, ~slot) -- an admissible IoU is a positive float, whose bits order like its value -- and the order of the
        // atomics does not matter to a maximum. A row scans the slots itself only when that track has been taken.
        int bj = -1;
        bool scanned = false;
        for (;;) {
            if (active && (!scanned || (bj >= 0 && dcls[bj] != cls))) {
                float bu = gate;
                const bool first = !scanned;
                bj = -1;
                scanned = true;
                // TK_SCAN rows per step, their LDS reads in flight together (one dependent read per row made this loop wait for LDS, not compute);
                // a taken row has lost its class. j0 + k <= 511: the arrays are TK_MAX_D long and the rows at or beyond n have no class.
                for (int j0 = 0; j0 < n; j0 += TK_SCAN) {
                    int c[TK_SCAN];
                    bool any = false;
#pragma unroll
                    for (int k = 0; k < TK_SCAN; ++k) {
                        c[k] = dcls[j0 + k];
                        any = any || c[k] == cls;
                    }
                    if (!any) continue;                               // (uniform)
                    long long l[TK_SCAN];
                    float4 bx[TK_SCAN];
#pragma unroll
                    for (int k = 0; k < TK_SCAN; ++k) {
                        l[k] = dlab[j0 + k];
                        bx[k] = dbox[j0 + k];
                    }
#pragma unroll
                    for (int k = 0; k < TK_SCAN; ++k)
                        if (c[k] == cls && (agn || l[k] == label)) {
                            const float u = tk_iou(mybox, bx[k]);
                            if (first && u > gate)
                                atomicMax(&dkey[j0 + k], ((unsigned long long)__float_as_uint(u) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)t));
                            if (u > bu) { bu = u; bj = j0 + k; }
                        }
                }
            }
            const bool propose = active && bj >= 0;
            if (propose) dhas[bj] = 1;
            if (!__syncthreads_or(propose)) break;
            for (int j = t; j < n; j += TK_NT) {
                if (!dhas[j]) continue;
                dhas[j] = 0;
                int bs = dprop[j];
                if (bs == -2) {
                    const unsigned long long key = dkey[j];
                    bs = key ? (int)(0xFFFFFFFFu - (unsigned)key) : -1;
                    dprop[j] = bs;
                }
                if (bs >= 0 && !tact[bs]) {
                    const float4 bx = dbox[j];
                    const long long lb = dlab[j];
                    float du = gate;
                    bs = -1;
                    for (int s0 = 0; s0 < T; s0 += TK_SCAN) {         // (s0 + k <= 255; the slots at or beyond T are never active)
                        int c[TK_SCAN];
                        bool any = false;
#pragma unroll
                        for (int k = 0; k < TK_SCAN; ++k) {
                            c[k] = tact[s0 + k];
                            any = any || c[k] != 0;
                        }
                        if (!any) continue;                           // (uniform)
                        long long l[TK_SCAN];
                        float4 tb[TK_SCAN];
#pragma unroll
                        for (int k = 0; k < TK_SCAN; ++k) {
                            l[k] = tlab[s0 + k];
                            tb[k] = tbox[s0 + k];
                        }
#pragma unroll
                        for (int k = 0; k < TK_SCAN; ++k)
                            if (c[k] != 0 && (agn || l[k] == lb)) {
                                const float u = tk_iou(tb[k], bx);
                                if (u > du) { du = u; bs = s0 + k; }
                            }
                    }
                    dprop[j] = bs;
                }
            }
            __syncthreads();
            if (propose && dprop[bj] == t) {
                // 4. - 6. a match: the filter takes the measurement; a lost or tentative track becomes tracked and keeps its id
                tk_update(f, dbox[bj]);
                score = dscore[bj];
                state = TK_TRACKED;
                last = frame;
                det = bj;
                matched = true;
                active = false;
                tact[t] = 0;
                did[bj] = id;
                dcls[bj] = TK_NONE;
            }
            __syncthreads();
        }
        if (stage == 2 && before == TK_TRACKED && !matched) state = TK_LOST;
        if (stage == 3 && before == TK_TENTATIVE && !matched) state = TK_FREE;
    }

    // 7. new tracks: the r-th remaining high detection with score >= new_thresh, in row order, takes the r-th free slot, in slot order
    int nnew = 0, r0, r1, tot;
    const int j1 = t + TK_NT;
    const bool s0 = t < n && dcls[t] == TK_HIGH && dscore[t] >= a.new_thresh;
    const bool s1 = j1 < n && dcls[j1] == TK_HIGH && dscore[j1] >= a.new_thresh;
    r0 = tk_scan(s0, wtot, tot);
    nnew = tot;
    r1 = nnew + tk_scan(s1, wtot, tot);
    nnew += tot;
    int nfree;
    const int fr = tk_scan(slot && state == TK_FREE, wtot, nfree);
    if (s0 && r0 < TK_NT) detlist[r0] = t;
    if (s1 && r1 < TK_NT) detlist[r1] = j1;
    const bool confirm_now = frame == 1;
    if (s0 && r0 < nfree) did[t] = confirm_now ? next_id + r0 : -1;
    if (s1 && r1 < nfree) did[j1] = confirm_now ? next_id + r1 : -1;
    __syncthreads();
    const int started = nnew < nfree ? nnew : nfree;
    if (slot && state == TK_FREE) {
        if (fr < started) {
            const int j = detlist[fr];
            tk_init(f, dbox[j]);
            state = confirm_now ? TK_TRACKED : TK_TENTATIVE;
            id = next_id + fr;
            label = dlab[j];
            score = dscore[j];
            start = frame;
            last = frame;
            det = j;
        } else {
            id = 0; label = 0; score = 0.0f; start = 0; last = 0; det = 0;
#pragma unroll
            for (int i = 0; i < 20; ++i) f[i] = 0.0f;
        }
    }
    dropped += nnew - started;

    // 8. a lost track that has not been seen for more than track_buffer frames is removed
    if (state == TK_LOST && frame - last > a.track_buffer) {
        state = TK_FREE;
        id = 0; label = 0; score = 0.0f; start = 0; last = 0; det = 0;
#pragma unroll
        for (int i = 0; i < 20; ++i) f[i] = 0.0f;
    }

    // 9. outputs: the confirmed tracks updated in this frame, in slot order
    const bool out = state == TK_TRACKED && last == frame;
    int nout;
    const int orank = tk_scan(out, wtot, nout);
    if (out) {
        const size_t o = (size_t)b * T + orank;
        a.boxes_out[o] = tk_box(f);
        a.scores_out[o] = score;
        a.labels_out[o] = label;
        a.ids_out[o] = id;
        a.det_out[o] = det;
    }
    if (slot && t >= nout) {
        const size_t o = (size_t)b * T + t;
        a.boxes_out[o] = make_float4(0.f, 0.f, 0.f, 0.f);
        a.scores_out[o] = 0.0f;
        a.labels_out[o] = 0;
        a.ids_out[o] = 0;
        a.det_out[o] = -1;
    }
    if (t == 0) a.counts_out[b] = nout;
    for (int j = t; j < d; j += TK_NT) a.det_ids_out[(size_t)b * d + j] = j < n ? (long long)did[j] : -1ll;

    // the state goes back through LDS
    if (slot) {
        sti[oState + t] = state;
        sti[oId + t] = id;
        reinterpret_cast<long long*>(sti + oLabel)[t] = label;
        stf[oScore + t] = score;
#pragma unroll
        for (int i = 0; i < 20; ++i) stf[oFilt + i * Tp + t] = f[i];
        sti[oStart + t] = start;
        sti[oLast + t] = last;
        sti[oDet + t] = det;
    }
    if (t == 0) {
        sti[0] = frame;
        sti[1] = next_id + started;
        sti[2] = dropped;
    }
    __syncthreads();
    for (int i = t; i < words / 4; i += TK_NT) gstate[i] = st4[i];
}

// one workgroup per stream: the selected streams restart at frame 0 with an empty table and next_id = 1
__global__ __launch_bounds__(TK_NT) void track_reset_kernel(uint4* __restrict__ state, const uint8_t* __restrict__ which, int words4) {
    const int b = blockIdx.x;
    if (which && which[b] == 0) return;
    uint4* const g = state + (size_t)b * words4;
    for (int i = threadIdx.x; i < words4; i += TK_NT) g[i] = i == 0 ? make_uint4(0u, 1u, 0u, 0u) : make_uint4(0u, 0u, 0u, 0u);
}

bool tk_number(float v) { return v >= 0.0f; }      // (a NaN compares false)

}  // namespace

extern "C" __attribute__((visibility("default"))) size_t dn_track_state_bytes(int streams, int max_tracks) {
    if (streams < 1 || max_tracks < 1 || max_tracks > TK_NT) return 0;
    return (size_t)streams * tk_stream_words(max_tracks) * 4;
}

extern "C" __attribute__((visibility("default"))) int dn_track_reset(void* state, int streams, int max_tracks, const uint8_t* which, void* stream) {
    DN_REQUIRE(state, "dn_track_reset: null state");
    DN_REQUIRE(streams >= 1 && max_tracks >= 1, "dn_track_reset: bad sizes streams=%d max_tracks=%d", streams, max_tracks);
    DN_REQUIRE((reinterpret_cast<size_t>(state) & 15) == 0, "dn_track_reset: the state must be 16-byte aligned");
    if (max_tracks > TK_NT) {
        dn_set_error("dn_track_reset: max_tracks=%d, at most %d", max_tracks, TK_NT);
        return DN_E_UNSUPPORTED;
    }
    dn_note_kernel("track_reset_kernel");
    hipLaunchKernelGGL(track_reset_kernel, dim3(streams), dim3(TK_NT), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<uint4*>(state), which,
                       (int)(tk_stream_words(max_tracks) / 4));
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}

extern "C" __attribute__((visibility("default"))) int dn_track_update(const float* boxes, const float* scores, const int64_t* labels,
                                                                     const int32_t* counts, int streams, int d, const dn_track_params* params,
                                                                     void* state, size_t state_bytes, float* boxes_out, float* scores_out,
                                                                     int64_t* labels_out, int64_t* ids_out, int32_t* det_out, int32_t* counts_out,
                                                                     int64_t* det_ids_out, void* stream) {
    DN_REQUIRE(boxes && scores && labels && counts && params && state && boxes_out && scores_out && labels_out && ids_out && det_out && counts_out &&
                   det_ids_out, "dn_track_update: null argument");
    const dn_track_params& p = *params;
    DN_REQUIRE(streams >= 1 && d >= 1 && p.max_tracks >= 1, "dn_track_update: bad sizes streams=%d d=%d max_tracks=%d", streams, d, p.max_tracks);
    DN_REQUIRE(tk_number(p.track_thresh) && tk_number(p.low_thresh) && tk_number(p.new_thresh) && tk_number(p.match_thresh) &&
                   tk_number(p.second_thresh) && tk_number(p.unconfirmed_thresh),
               "dn_track_update: the thresholds must be numbers >= 0 (track %g low %g new %g match %g second %g unconfirmed %g)", (double)p.track_thresh,
               (double)p.low_thresh, (double)p.new_thresh, (double)p.match_thresh, (double)p.second_thresh, (double)p.unconfirmed_thresh);
    DN_REQUIRE(p.match_thresh <= 1.0f && p.second_thresh <= 1.0f && p.unconfirmed_thresh <= 1.0f,
               "dn_track_update: match_thresh=%g, second_thresh=%g and unconfirmed_thresh=%g are costs 1 - IoU: at most 1", (double)p.match_thresh,
               (double)p.second_thresh, (double)p.unconfirmed_thresh);
    DN_REQUIRE(p.track_buffer >= 0,"dn_track_update: track_buffer=%d must not be negative", p.track_buffer);
    DN_REQUIRE(((reinterpret_cast<size_t>(boxes) | reinterpret_cast<size_t>(boxes_out) | reinterpret_cast<size_t>(state)) & 15) == 0 &&
                   ((reinterpret_cast<size_t>(labels) | reinterpret_cast<size_t>(labels_out) | reinterpret_cast<size_t>(ids_out) |
                     reinterpret_cast<size_t>(det_ids_out)) & 7) == 0 &&
                   ((reinterpret_cast<size_t>(scores) | reinterpret_cast<size_t>(counts) | reinterpret_cast<size_t>(scores_out) |
                     reinterpret_cast<size_t>(det_out) | reinterpret_cast<size_t>(counts_out)) & 3) == 0,
               "dn_track_update: boxes, boxes_out and the state must be 16-byte aligned, labels, ids and det_ids 8-byte aligned, the others 4-byte aligned");
    if (d > TK_MAX_D || p.max_tracks > TK_NT) {
        dn_set_error("dn_track_update: d=%d at most %d, max_tracks=%d at most %d", d, TK_MAX_D, p.max_tracks, TK_NT);
        return DN_E_UNSUPPORTED;
    }
    const size_t need = dn_track_state_bytes(streams, p.max_tracks);
    if (state_bytes < need) {
        dn_set_error("dn_track_update: state of %zu B, %zu B needed", state_bytes, need);
        return DN_E_WORKSPACE;
    }
    TrackArgs a;
    a.boxes = reinterpret_cast<const float4*>(boxes); a.scores = scores; a.labels = labels; a.counts = counts;
    a.state = reinterpret_cast<uint4*>(state);
    a.boxes_out = reinterpret_cast<float4*>(boxes_out); a.scores_out = scores_out; a.labels_out = labels_out; a.ids_out = ids_out;
    a.det_out = det_out; a.counts_out = counts_out; a.det_ids_out = det_ids_out;
    a.d = d; a.T = p.max_tracks; a.Tp = tk_padded(p.max_tracks);
    a.track_thresh = p.track_thresh; a.low_thresh = p.low_thresh; a.new_thresh = p.new_thresh;
    a.gate1 = 1.0f - p.match_thresh; a.gate2 = 1.0f - p.second_thresh; a.gate3 = 1.0f - p.unconfirmed_thresh;
    a.track_buffer = p.track_buffer; a.class_agnostic = p.class_agnostic;
    dn_note_kernel("track_update_kernel");
    hipLaunchKernelGGL(track_update_kernel, dim3(streams), dim3(TK_NT), 0, reinterpret_cast<hipStream_t>(stream), a);
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}
