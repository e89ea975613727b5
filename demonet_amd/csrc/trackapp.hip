// Appearance association in the device tracker: dn_track_update_appearance is dn_track_update with BoT-SORT's appearance term
// (Aharon et al. 2022) fused into the pair value of stages 1 and 3. The semantics, sentence by sentence, are in include/demonet_hip.h and
// restated in tests/track_appearance_ref.py. A step with embeddings is four graph nodes, none of which waits for the host:
//   1. a fill: the row -> embedding-slot map becomes -1;
//   2. track_emb_prepare_kernel, a wave per embedding slot, lanes over dim: the fp32 norm, the normalised fp16 row `en`, the slot's presence
//      flag, and the slot's entry in the map -- an integer maximum, so of two index rows that name the same (stream, row) the higher slot wins
//      whatever order the waves run in;
//   3. track_sim_kernel: S[b][slot][row] = half(feature[slot]) . en[slot_of(row)] on v_mfma_f32_16x16x32_f16, fp32 accumulation. A wave owns
//      16 slots x 64 rows (four accumulator tiles that share one A fragment); the operands come straight from global memory -- per stream the
//      whole problem is at most 256 x 512 x 512, there is no reuse worth an LDS tile -- the features rounded to fp16 as they are loaded, the
//      en rows gathered through the map. A 16 x 16 tile whose slots or rows have no feature issues no matrix instruction and stores zeros.
//      The 16x16x32 form, not 32x32x16: the track side is padded to 16 and not to 32 slots (max_tracks 1 .. 17 are real configurations), and
//      a tile is skipped at 16-row granularity; the two forms were not timed against each other.
//   4. track_update_app_kernel: the body of track_update_kernel (trackstep.inc) with the fused value v in place of u, S read from global
//      memory (the track side its own row, 8 consecutive floats per scan step; a row's rescan its column), and the features' start / EMA /
//      clear in the same launch's tail, a wave per slot.
// A step without embeddings (E = 0) is launch 4 alone. Compiled with -ffp-contract=off like track.hip. No inline asm, no float atomics.
#include "trackcore.h"

namespace {

constexpr int TA_MAX_E = 8192;             // embedding slots per step (the cropper's capacity)
constexpr int TA_MAX_DIM = 512;
constexpr int TA_ROWS = 64;                // rows (four 16-wide tiles) a wave of track_sim_kernel owns

inline size_t ta_up16(size_t v) { return (v + 15) & ~(size_t)15; }
inline size_t ta_feature_words(int max_tracks, int dim) { return (size_t)tk_padded(max_tracks) * (1 + (size_t)dim); }

// the workspace, every part 16-byte aligned: en [E][dim] fp16, present [E] int32, map [B][d] int32, S [B][Tp][d] fp32
struct TaLayout { size_t en, present, map, S, total; };
inline TaLayout ta_layout(int streams, int max_tracks, int d, int E, int dim) {
    TaLayout l;
    l.en = 0;
    l.present = ta_up16((size_t)E * dim * 2);
    l.map = l.present + ta_up16((size_t)E * 4);
    l.S = l.map + ta_up16((size_t)streams * d * 4);
    l.total = l.S + (size_t)streams * tk_padded(max_tracks) * d * 4;
    return l;
}

inline bool ta_dim_ok(int dim) { return dim >= 32 && dim <= TA_MAX_DIM && dim % 32 == 0; }

// 2. one wave per embedding slot e. Nothing of the index table or of the embeddings is trusted.
template <typename T>
__global__ __launch_bounds__(TK_NT) void track_emb_prepare_kernel(const T* __restrict__ emb, const int32_t* __restrict__ index,
                                                                  const int32_t* __restrict__ counts, int E, int dim, int streams, int d,
                                                                  half_t* __restrict__ en, int32_t* __restrict__ present, int32_t* map) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * TK_WAVES + (threadIdx.x >> 6);
    if (e >= E) return;                                               // (a whole wave)
    const T* const x = emb + (size_t)e * dim;
    float v[8];
    float ss = 0.0f;
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = lane + 64 * i;
        v[i] = 0.0f;
        if (k < dim) {
            v[i] = (float)x[k];
            fin = fin && fabsf(v[i]) < INFINITY;                      // (a NaN compares false)
            ss += v[i] * v[i];
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m);        // a butterfly: every lane ends with the same bits, on every run
    const float nrm = sqrtf(ss);
    const bool ok = __all(fin) && nrm > 0.0f && nrm < INFINITY;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = lane + 64 * i;
        if (k < dim) en[(size_t)e * dim + k] = ok ? (half_t)(v[i] / nrm) : (half_t)0.0f;
    }
    if (lane == 0) {
        present[e] = ok ? 1 : 0;
        const int s = index[(size_t)e * 8], r = index[(size_t)e * 8 + 1];
        if (s >= 0 && s < streams && r >= 0) {
            int n = counts[s];
            n = n < 0 ? 0 : (n > d ? d : n);
            if (r < n) atomicMax(&map[(size_t)s * d + r], e);
        }
    }
}

struct SimArgs {
    const int32_t* fflag;                  // the feature buffer (see TrackAppArgs)
    const half_t* en;
    const int32_t* present;
    const int32_t* map;
    float* S;
    int d, Tp, dim;
};

// 3. grid (stream, 64-row group, 64-slot group), a wave per 16 slots. Operand lane maps of v_mfma_f32_16x16x32_f16 (lane l, r = l & 15,
// q = l >> 4): A[row r][k = 8 q + j], B[k = 8 q + j][column r], j = 0 .. 7; the result D[row 4 q + i][column r] in register i.
// Here A's rows are slots, B's columns are detection rows.
__global__ __launch_bounds__(TK_NT) void track_sim_kernel(const SimArgs a) {
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const int b = blockIdx.x;
    const int n0 = blockIdx.y * TA_ROWS;
    const int m0 = blockIdx.z * 64 + (threadIdx.x >> 6) * 16;
    if (m0 >= a.Tp) return;                                           // (a whole wave; the kernel has no barrier)
    const int32_t* const fl = a.fflag + (size_t)b * a.Tp * (1 + (size_t)a.dim);
    const float* const fv = reinterpret_cast<const float*>(fl + a.Tp);
    const int slot = m0 + r;
    const bool sok = slot < a.Tp && fl[slot] != 0;
    const unsigned long long smask = __ballot(sok);                   // bits 0 .. 15: the tile's slots
    int e[4];
    bool any[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int row = n0 + 16 * c + r;
        e[c] = row < a.d ? a.map[(size_t)b * a.d + row] : -1;
        if (e[c] >= 0 && a.present[e[c]] == 0) e[c] = -1;
        any[c] = __ballot(e[c] >= 0) != 0ull;
    }
    floatx4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
    if ((smask & 0xFFFFull) != 0ull && (any[0] || any[1] || any[2] || any[3])) {
        const float* const arow = fv + (size_t)(sok ? slot : 0) * a.dim + 8 * q;
        for (int k0 = 0; k0 < a.dim; k0 += 32) {
            half8 af;
#pragma unroll
            for (int j = 0; j < 8; ++j) af[j] = (half_t)0.0f;
            if (sok) {
                const float4 lo = *reinterpret_cast<const float4*>(arow + k0), hi = *reinterpret_cast<const float4*>(arow + k0 + 4);
                af[0] = (half_t)lo.x; af[1] = (half_t)lo.y; af[2] = (half_t)lo.z; af[3] = (half_t)lo.w;
                af[4] = (half_t)hi.x; af[5] = (half_t)hi.y; af[6] = (half_t)hi.z; af[7] = (half_t)hi.w;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (!any[c]) continue;                                // (uniform)
                half8 bf;
#pragma unroll
                for (int j = 0; j < 8; ++j) bf[j] = (half_t)0.0f;
                if (e[c] >= 0) bf = *reinterpret_cast<const half8*>(a.en + (size_t)e[c] * a.dim + k0 + 8 * q);
                acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, acc[c], 0, 0, 0);
            }
        }
    }
    // every entry of the stream's [Tp][d] block is written in every step; an entry whose slot or row has no feature is 0
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int row = n0 + 16 * c + r;
        if (row >= a.d) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int trk = m0 + 4 * q + i;
            if (trk < a.Tp) a.S[((size_t)b * a.Tp + trk) * a.d + row] = (((smask >> (4 * q + i)) & 1ull) != 0ull && e[c] >= 0) ? acc[c][i] : 0.0f;
        }
    }
}

// 4. the frame step with the fused pair value and the features' tail
__global__ __launch_bounds__(TK_NT) void track_update_app_kernel(const TrackArgs a, const TrackAppArgs p) {
    constexpr bool APP = true;
    __shared__ unsigned char dfeat[TK_MAX_D];  // the row has an embedding
#include "trackstep.inc"
}

// one workgroup per stream: the selected streams lose every feature (flags and values become 0)
__global__ __launch_bounds__(TK_NT) void track_feature_reset_kernel(uint4* __restrict__ feat, const uint8_t* __restrict__ which, size_t words4) {
    const int b = blockIdx.x;
    if (which && which[b] == 0) return;
    uint4* const g = feat + (size_t)b * words4;
    for (size_t i = threadIdx.x; i < words4; i += TK_NT) g[i] = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace

extern "C" __attribute__((visibility("default"))) size_t dn_track_feature_bytes(int streams, int max_tracks, int dim) {
    if (streams < 1 || max_tracks < 1 || max_tracks > TK_NT || !ta_dim_ok(dim)) return 0;
    return (size_t)streams * ta_feature_words(max_tracks, dim) * 4;
}

extern "C" __attribute__((visibility("default"))) size_t dn_track_appearance_workspace_bytes(int streams, int max_tracks, int d, int E, int dim) {
    if (streams < 1 || max_tracks < 1 || max_tracks > TK_NT || d < 1 || d > TK_MAX_D || E < 1 || E > TA_MAX_E || !ta_dim_ok(dim)) return 0;
    return ta_layout(streams, max_tracks, d, E, dim).total;
}

extern "C" __attribute__((visibility("default"))) int dn_track_feature_reset(void* features, int streams, int max_tracks, int dim,
                                                                            const uint8_t* which, void* stream) {
    DN_REQUIRE(features, "dn_track_feature_reset: null features");
    DN_REQUIRE(streams >= 1 && max_tracks >= 1 && dim >= 1, "dn_track_feature_reset: bad sizes streams=%d max_tracks=%d dim=%d", streams, max_tracks,
               dim);
    DN_REQUIRE((reinterpret_cast<size_t>(features) & 15) == 0, "dn_track_feature_reset: the features must be 16-byte aligned");
    if (max_tracks > TK_NT || !ta_dim_ok(dim)) {
        dn_set_error("dn_track_feature_reset: max_tracks=%d at most %d, dim=%d a multiple of 32 in 32 .. %d", max_tracks, TK_NT, dim, TA_MAX_DIM);
        return DN_E_UNSUPPORTED;
    }
    dn_note_kernel("track_feature_reset_kernel");
    hipLaunchKernelGGL(track_feature_reset_kernel, dim3(streams), dim3(TK_NT), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<uint4*>(features), which, ta_feature_words(max_tracks, dim) / 4);
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}

extern "C" __attribute__((visibility("default"))) int dn_track_update_appearance(
    const float* boxes, const float* scores, const int64_t* labels, const int32_t* counts, int streams, int d, const dn_track_params* params,
    const dn_track_appearance_params* app, const void* emb, const int32_t* emb_index, int E, void* state, size_t state_bytes, void* features,
    size_t feature_bytes, void* workspace, size_t workspace_bytes, float* boxes_out, float* scores_out, int64_t* labels_out, int64_t* ids_out,
    int32_t* det_out, int32_t* counts_out, int64_t* det_ids_out, void* stream) {
    const char* const who = "dn_track_update_appearance";
    TrackArgs a;
    const int rc = tk_check_step(who, boxes, scores, labels, counts, streams, d, params, state, state_bytes, boxes_out, scores_out, labels_out,
                                 ids_out, det_out, counts_out, det_ids_out, a);
    if (rc != DN_OK) return rc;
    DN_REQUIRE(app && features, "%s: null argument", who);
    const dn_track_appearance_params& q = *app;
    DN_REQUIRE(q.dim >= 1 && E >= 0, "%s: bad sizes dim=%d E=%d", who, q.dim, E);
    DN_REQUIRE(q.alpha >= 0.0f && q.alpha <= 1.0f, "%s: alpha=%g must be a number in 0 .. 1", who, (double)q.alpha);
    DN_REQUIRE(tk_number(q.appearance_thresh) && tk_number(q.proximity_thresh), "%s: appearance_thresh=%g and proximity_thresh=%g must be numbers >= 0",
               who, (double)q.appearance_thresh, (double)q.proximity_thresh);
    DN_REQUIRE(q.emb_fp16 == 0 || q.emb_fp16 == 1, "%s: emb_fp16=%d must be 0 or 1", who, q.emb_fp16);
    DN_REQUIRE(q.reserved[0] == 0 && q.reserved[1] == 0 && q.reserved[2] == 0, "%s: the reserved words must be 0", who);
    DN_REQUIRE((reinterpret_cast<size_t>(features) & 15) == 0, "%s: the features must be 16-byte aligned", who);
    if (E == 0) DN_REQUIRE(!emb && !emb_index, "%s: E=0 with an embedding or an index table", who);
    else
        DN_REQUIRE(emb && emb_index && workspace && ((reinterpret_cast<size_t>(emb) | reinterpret_cast<size_t>(emb_index) |
                                                      reinterpret_cast<size_t>(workspace)) & 15) == 0,
                   "%s: E=%d needs embeddings, an index table and a workspace, each 16-byte aligned", who, E);
    if (!ta_dim_ok(q.dim) || E > TA_MAX_E) {
        dn_set_error("%s: dim=%d a multiple of 32 in 32 .. %d, E=%d at most %d", who, q.dim, TA_MAX_DIM, E, TA_MAX_E);
        return DN_E_UNSUPPORTED;
    }
    const size_t fneed = (size_t)streams * ta_feature_words(a.T, q.dim) * 4;
    if (feature_bytes < fneed) {
        dn_set_error("%s: features of %zu B, %zu B needed", who, feature_bytes, fneed);
        return DN_E_WORKSPACE;
    }
    const TaLayout l = ta_layout(streams, a.T, d, E, q.dim);
    if (E > 0 && workspace_bytes < l.total) {
        dn_set_error("%s: workspace of %zu B, %zu B needed", who, workspace_bytes, l.total);
        return DN_E_WORKSPACE;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* const ws = static_cast<char*>(workspace);
    TrackAppArgs p{};
    p.fflag = static_cast<int32_t*>(features);
    p.dim = q.dim;
    p.alpha = q.alpha; p.beta = 1.0f - q.alpha;
    p.app_thresh = q.appearance_thresh; p.prox_thresh = q.proximity_thresh;
    if (E > 0) {
        half_t* const en = reinterpret_cast<half_t*>(ws + l.en);
        int32_t* const present = reinterpret_cast<int32_t*>(ws + l.present);
        int32_t* const map = reinterpret_cast<int32_t*>(ws + l.map);
        float* const S = reinterpret_cast<float*>(ws + l.S);
        DN_HIP_CHECK(hipMemsetAsync(map, 0xFF, (size_t)streams * d * 4, s));
        const dim3 pg((E + TK_WAVES - 1) / TK_WAVES);
        dn_note_kernel("track_emb_prepare_kernel");
        if (q.emb_fp16)
            hipLaunchKernelGGL(track_emb_prepare_kernel<half_t>, pg, dim3(TK_NT), 0, s, static_cast<const half_t*>(emb), emb_index, counts, E, q.dim,
                               streams, d, en, present, map);
        else
            hipLaunchKernelGGL(track_emb_prepare_kernel<float>, pg, dim3(TK_NT), 0, s, static_cast<const float*>(emb), emb_index, counts, E, q.dim,
                               streams, d, en, present, map);
        DN_HIP_CHECK(hipGetLastError());
        SimArgs m;
        m.fflag = p.fflag; m.en = en; m.present = present; m.map = map; m.S = S;
        m.d = d; m.Tp = a.Tp; m.dim = q.dim;
        dn_note_kernel("track_sim_kernel");
        hipLaunchKernelGGL(track_sim_kernel, dim3(streams, (d + TA_ROWS - 1) / TA_ROWS, (a.Tp + 63) / 64), dim3(TK_NT), 0, s, m);
        DN_HIP_CHECK(hipGetLastError());
        p.S = S; p.map = map; p.epres = present; p.en = en;
    }
    dn_note_kernel("track_update_app_kernel");
    hipLaunchKernelGGL(track_update_app_kernel, dim3(streams), dim3(TK_NT), 0, s, a, p);
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}
