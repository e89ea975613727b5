// Weighted boxes fusion: dn_fuse_detections, the reducer for sources that are different opinions about the same objects -- the plain
// and the flipped pass of one image, several checkpoints. Where dn_merge_detections (sliced.hip) keeps the best box of an overlapping set, this
// averages the set with the scores as weights and marks down what only some of the sources saw (Solovyev, Wang, Gabruseva 2019; conf_type 'avg').
//   1      fuse_keys_kernel                       v = score * weight of every candidate as a key
//   2 - 3  detset_rank (detset.hip)               the ranking of the candidates: rank by counting and scatter, the merge's own
//   4      fuse_walk_kernel                       one wave per group walks the ranking and builds the cluster table
//   5      detset_rank once more, no scatter      ranks the clusters by their final score (the table's keys take the place of the candidates')
//   6      fuse_emit_kernel                       cluster of rank r -> output row r; the rows behind the count are cleared
// Compiled with -ffp-contract=off: every operation of the header's text rounds once, as tests/wbf_ref.py restates it. No inline asm, no atomics
// in this file.
#include "detset.h"

namespace {

constexpr int FZ_MAX_D = 512, FZ_MAX_SLOTS = 8192;
constexpr int FZ_NT = 256;                 // threads of the keys and emit workgroups
constexpr int FZ_WAVE = 64;                // the walk's workgroup: one wave
constexpr int FZ_SCAN = 4, FZ_SCAN_WS = 8;  // clusters a lane examines per step of its scan: in LDS, in the workspace
constexpr int FZ_LDS_CLUSTERS = 1024;      // clusters the walk keeps in LDS, 48 bytes each (a multiple of 64 * FZ_SCAN); the others live in the workspace
static_assert(FZ_LDS_CLUSTERS % (FZ_WAVE * FZ_SCAN) == 0, "a scan step must stay inside the LDS table");
constexpr int FZ_NONE = 0x7FFFFFFF;        // no cluster matched

// One entry per slot; cluster c of a group lives at the group's first slot + c (a group has at most as many clusters as candidates).
struct FuseBuffers {
    unsigned* keys;        // [N] launches 1 - 3: v as an unsigned that orders like the float, 0: not a candidate. From the walk on: the same for the
                           //     cluster's final score, 0: no cluster
    unsigned* rank;        // [N] candidates (later: clusters) of the same group that rank higher
    unsigned* order;       // [N] flattened index of the candidate of each rank, per group from the group's first slot; DS_END behind the last
    float4* fbox;          // [N] fused box
    float4* acc;           // [N] A_k = sum of v * coord_k (used by the clusters beyond the walk's LDS table only)
    long long* label;      // [N]
    float* sv;             // [N] Sv = sum of v during the walk, the cluster's score after it
    int32_t* members;      // [N] T
    size_t bytes;
};
FuseBuffers fuse_buffers(void* ws, size_t n_slots) {
    FuseBuffers b;
    unsigned char* p = reinterpret_cast<unsigned char*>(ws);
    b.fbox = reinterpret_cast<float4*>(p); p += a256(n_slots * 16);
    b.acc = reinterpret_cast<float4*>(p); p += a256(n_slots * 16);
    b.label = reinterpret_cast<long long*>(p); p += a256(n_slots * 8);
    b.keys = reinterpret_cast<unsigned*>(p); p += a256(n_slots * 4);
    b.rank = reinterpret_cast<unsigned*>(p); p += a256(n_slots * 4);
    b.order = reinterpret_cast<unsigned*>(p); p += a256(n_slots * 4);
    b.sv = reinterpret_cast<float*>(p); p += a256(n_slots * 4);
    b.members = reinterpret_cast<int32_t*>(p); p += a256(n_slots * 4);
    b.bytes = (size_t)(p - reinterpret_cast<unsigned char*>(ws));
    return b;
}

// Launch 1, one thread per slot (source s, row j; flattened index i = s * d + j): v = score * weight[s]; a candidate (j < counts[s], v not NaN,
// v >= skip_thresh, v > 0) gets v's dn_order_key, every other slot 0. Also clears what the two ranking launches fill.
__global__ __launch_bounds__(FZ_NT) void fuse_keys_kernel(const float* __restrict__ scores, const int32_t* __restrict__ counts,
                                                          const float* __restrict__ weights, float skip_thresh, int n_slots, int d,
                                                          unsigned* __restrict__ keys, unsigned* __restrict__ rank, unsigned* __restrict__ order) {
    const int i = blockIdx.x * FZ_NT + threadIdx.x;
    if (i >= n_slots) return;
    const int s = i / d, j = i - s * d;
    const float v = scores[i] * (weights ? weights[s] : 1.0f);
    keys[i] = (j < counts[s] && v == v && v >= skip_thresh && v > 0.f) ? dn_order_key(v) : 0u;
    rank[i] = 0u;
    order[i] = DS_END;
}

struct FuseArgs {
    const float4* boxes; const float* scores; const int64_t* labels; const float2* offsets; const float* weights;
    FuseBuffers b;
    int d, d_out;
    float thresh;
    float4* boxes_out; float* scores_out; int64_t* labels_out; int32_t* counts_out; int32_t* members_out;
};

// IoU of the cluster's fused box f with the candidate b (area ab): the merge's (DN_MERGE_IOU) by construction, both divide dn_box_inter by the same
// sum. thresh >= 0, so a pair without intersection (overlap 0 or NaN) cannot pass `> thresh`: -1 stands for "no match" there, as it does for a NaN
// overlap at the caller.
__device__ __forceinline__ float fz_iou(const float4 f, const float4 b, const float ab) {
    const float inter = dn_box_inter(f, b);
    if (inter == 0.0f) return -1.0f;
    const float af = (f.z - f.x) * (f.w - f.y);
    return inter / (af + ab - inter);
}

// one step of a lane's scan: the cluster c with fused box f, if it is live (exists and has the candidate's label), against the best so far
__device__ __forceinline__ void fz_consider(float& bu, int& bc, const bool live, const float4 f, const float4 b, const float ab, const float thresh,
                                            const int c) {
    if (live) {
        const float u = fz_iou(f, b, ab);
        if (u > thresh && u > bu) { bu = u; bc = c; }
    }
}

// Launch 4, one wave per group. Lane c % 64 OWNS cluster c: no other lane reads or writes its fused box, label, A, Sv or T before the walk has
// ended, so program order is all the ordering the table needs. The first FZ_LDS_CLUSTERS clusters live in LDS while the walk runs and are written
// to the workspace when it ends; the clusters beyond them live in the workspace from the start.
//   per chunk of 64 ranks: lane t fetches the candidate of rank pos + t (shifted box, v, label) into LDS; the fetch of the next chunk is issued
//   before the walk through this one, so its two dependent global reads (order -> row) run under it;
//   per candidate, in rank order: every lane scans its own clusters of the candidate's label for the largest u > thresh (the earliest on a tie:
//   its clusters come in ascending order and the comparison is strict), FZ_SCAN clusters per step so that their LDS reads are in flight together.
//   No lane with a match: lane (clusters % 64) opens a new cluster. One lane: its cluster wins. Several: a butterfly of __shfl_xor leaves
//   (largest u, lowest cluster index) in every lane. The owner of the winner adds the candidate to it.
// When the ranking is exhausted every owner turns Sv into the cluster's score and writes its key for launch 5.
__global__ __launch_bounds__(FZ_WAVE) void fuse_walk_kernel(FuseArgs a, GroupTab gt) {
    __shared__ float4 lbox[FZ_LDS_CLUSTERS];
    __shared__ float4 lacc[FZ_LDS_CLUSTERS];
    __shared__ long long llabel[FZ_LDS_CLUSTERS];
    __shared__ float lsv[FZ_LDS_CLUSTERS];
    __shared__ int lmem[FZ_LDS_CLUSTERS];
    __shared__ float4 cbox[FZ_WAVE];
    __shared__ long long clabel[FZ_WAVE];
    __shared__ float cval[FZ_WAVE];

    const int g = blockIdx.x, lane = threadIdx.x;
    const int s0 = gt.begin[g], ns = gt.begin[g + 1] - s0;
    const int base = s0 * a.d, n = ns * a.d;
    const int G = gt.first + g;
    const float thresh = a.thresh;
    float4* const fbox = a.b.fbox + base;
    float4* const acc = a.b.acc + base;
    long long* const flabel = a.b.label + base;
    float* const sv = a.b.sv + base;
    int32_t* const members = a.b.members + base;

    float W = (float)ns;      // (NULL weights: ns ones, exact below 2^24)
    if (a.weights) {
        W = 0.f;
        for (int s = 0; s < ns; ++s) W = W + a.weights[s0 + s];
    }

    // the candidate of rank pos + lane: false when the ranking has ended there
    auto fetch = [&](const int pos, float4& b, float& v, long long& lb) -> bool {
        const unsigned idx = pos + lane < n ? a.b.order[base + pos + lane] : DS_END;
        if (idx == DS_END) return false;
        const unsigned s = idx / (unsigned)a.d;
        const float2 o = a.offsets[s];
        b = a.boxes[idx];
        b.x = b.x + o.x; b.y = b.y + o.y; b.z = b.z + o.x; b.w = b.w + o.y;
        v = a.scores[idx] * (a.weights ? a.weights[s] : 1.0f);
        lb = a.labels[idx];
        return true;
    };

    int nc = 0;
    float4 fb = make_float4(0.f, 0.f, 0.f, 0.f);
    float fv = 0.f;
    long long fl = 0;
    bool valid = fetch(0, fb, fv, fl);
    for (int pos = 0; pos < n; pos += FZ_WAVE) {
        if (valid) { cbox[lane] = fb; cval[lane] = fv; clabel[lane] = fl; }
        const int nv = __popcll(__ballot(valid));      // candidates fill the ranks from 0 without a gap
        __syncthreads();
        valid = nv == FZ_WAVE && fetch(pos + FZ_WAVE, fb, fv, fl);
        for (int i = 0; i < nv; ++i) {
            const float4 b = cbox[i];
            const float v = cval[i];
            const long long lb = clabel[i];
            const float ab = (b.z - b.x) * (b.w - b.y);
            float bu = -1.0f;
            int bc = FZ_NONE;
            const int nl = nc < FZ_LDS_CLUSTERS ? nc : FZ_LDS_CLUSTERS;
            for (int c0 = lane; c0 < nl; c0 += FZ_WAVE * FZ_SCAN) {
                // c0 + 64 k < FZ_LDS_CLUSTERS (a multiple of 64 FZ_SCAN) for every k; rows at or beyond nl hold stale values and are not looked at
                long long l[FZ_SCAN];
                float4 f[FZ_SCAN];
#pragma unroll
                for (int k = 0; k < FZ_SCAN; ++k) {
                    l[k] = llabel[c0 + FZ_WAVE * k];
                    f[k] = lbox[c0 + FZ_WAVE * k];
                }
#pragma unroll
                for (int k = 0; k < FZ_SCAN; ++k) fz_consider(bu, bc, c0 + FZ_WAVE * k < nl && l[k] == lb, f[k], b, ab, thresh, c0 + FZ_WAVE * k);
            }
            for (int c0 = FZ_LDS_CLUSTERS + lane; c0 < nc; c0 += FZ_WAVE * FZ_SCAN_WS) {
                // the same from the workspace, more reads in flight per step: the index is clamped into the group's n slots, and a row at or
                // beyond nc (stale, or another lane's) is not looked at
                long long l[FZ_SCAN_WS];
                float4 f[FZ_SCAN_WS];
#pragma unroll
                for (int k = 0; k < FZ_SCAN_WS; ++k) {
                    const int c = c0 + FZ_WAVE * k < n ? c0 + FZ_WAVE * k : n - 1;
                    l[k] = flabel[c];
                    f[k] = fbox[c];
                }
#pragma unroll
                for (int k = 0; k < FZ_SCAN_WS; ++k) fz_consider(bu, bc, c0 + FZ_WAVE * k < nc && l[k] == lb, f[k], b, ab, thresh, c0 + FZ_WAVE * k);
            }
            const unsigned long long hit = __ballot(bc != FZ_NONE);
            if (hit == 0ull) {
                if ((nc & (FZ_WAVE - 1)) == lane) {
                    if (nc < FZ_LDS_CLUSTERS) {
                        lmem[nc] = 1;
                        lsv[nc] = v;
                        lacc[nc] = make_float4(v * b.x, v * b.y, v * b.z, v * b.w);
                        lbox[nc] = b;
                        llabel[nc] = lb;
                    } else {
                        members[nc] = 1;
                        sv[nc] = v;
                        acc[nc] = make_float4(v * b.x, v * b.y, v * b.z, v * b.w);
                        fbox[nc] = b;
                        flabel[nc] = lb;
                    }
                }
                ++nc;
                continue;
            }
            if ((hit & (hit - 1ull)) != 0ull) {
#pragma unroll
                for (int m = 1; m < FZ_WAVE; m <<= 1) {
                    const float ou = __shfl_xor(bu, m, FZ_WAVE);
                    const int oc = __shfl_xor(bc, m, FZ_WAVE);
                    if (ou > bu || (ou == bu && oc < bc)) { bu = ou; bc = oc; }
                }
            }
            // (one lane with a match: only that lane's bc is a cluster, and it is its own)
            if (bc != FZ_NONE && (bc & (FZ_WAVE - 1)) == lane) {
                const int win = bc;
                const bool in_lds = win < FZ_LDS_CLUSTERS;
                const float svn = (in_lds ? lsv[win] : sv[win]) + v;
                float4 A = in_lds ? lacc[win] : acc[win];
                A.x = A.x + v * b.x; A.y = A.y + v * b.y; A.z = A.z + v * b.z; A.w = A.w + v * b.w;
                const float4 f = make_float4(A.x / svn, A.y / svn, A.z / svn, A.w / svn);
                if (in_lds) {
                    lmem[win] = lmem[win] + 1;
                    lsv[win] = svn;
                    lacc[win] = A;
                    lbox[win] = f;
                } else {
                    members[win] = members[win] + 1;
                    sv[win] = svn;
                    acc[win] = A;
                    fbox[win] = f;
                }
            }
        }
        __syncthreads();      // the chunk's LDS rows are rewritten next
        if (nv < FZ_WAVE) break;
    }
    // the owners' last word: their LDS clusters go to the workspace, score = ((Sv / T) * min(T, W)) / W, left to right, takes Sv's place, and
    // every slot of the group gets its key for the cluster ranking
    for (int c = lane; c < n; c += FZ_WAVE) {
        unsigned k = 0u;
        if (c < nc) {
            int T;
            float s;
            if (c < FZ_LDS_CLUSTERS) {
                T = lmem[c];
                s = lsv[c];
                members[c] = T;
                fbox[c] = lbox[c];
                flabel[c] = llabel[c];
            } else {
                T = members[c];
                s = sv[c];
            }
            const float t = (float)T;
            const float sc = ((s / t) * (W < t ? W : t)) / W;
            sv[c] = sc;
            k = dn_order_key(sc);      // (a NaN score ranks behind every number)
        }
        a.b.keys[base + c] = k;
        a.b.rank[base + c] = 0u;
    }
    if (lane == 0) a.counts_out[G] = nc < a.d_out ? nc : a.d_out;
}

// Launch 6: the cluster of rank r < d_out is output row r; rows at or beyond the count are cleared. grid (blocks over max(slots, d_out), groups).
__global__ __launch_bounds__(FZ_NT) void fuse_emit_kernel(FuseArgs a, GroupTab gt) {
    const int g = blockIdx.y;
    const int base = gt.begin[g] * a.d, n = (gt.begin[g + 1] - gt.begin[g]) * a.d;
    const int G = gt.first + g;
    const int i = blockIdx.x * FZ_NT + threadIdx.x;
    if (i < n && a.b.keys[base + i] != 0u) {
        const unsigned r = a.b.rank[base + i];
        if (r < (unsigned)a.d_out) {
            const size_t o = (size_t)G * a.d_out + r;
            a.boxes_out[o] = a.b.fbox[base + i];
            a.scores_out[o] = a.b.sv[base + i];
            a.labels_out[o] = a.b.label[base + i];
            if (a.members_out) a.members_out[o] = a.b.members[base + i];
        }
    }
    if (i < a.d_out && i >= a.counts_out[G]) {
        const size_t o = (size_t)G * a.d_out + i;
        a.boxes_out[o] = make_float4(0.f, 0.f, 0.f, 0.f);
        a.scores_out[o] = 0.f;
        a.labels_out[o] = 0;
        if (a.members_out) a.members_out[o] = 0;
    }
}

bool fuse_supported(int s_total, int d, const int32_t* group_begin, int groups) {
    if (d > FZ_MAX_D || (long long)s_total * d > 0x7FFFFFFFll) return false;
    for (int g = 0; g < groups; ++g)
        if ((long long)(group_begin[g + 1] - group_begin[g]) * d > FZ_MAX_SLOTS) return false;
    return true;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) size_t dn_fuse_detections_workspace_bytes(int s_total, int d, const int32_t* group_begin,
                                                                                           int groups) {
    if (!group_begin || !detset_sizes_ok(s_total, d, groups) || !detset_groups_ok(group_begin, groups, s_total) ||
        !fuse_supported(s_total, d, group_begin, groups))
        return 0;
    return fuse_buffers(nullptr, (size_t)s_total * d).bytes;
}

extern "C" __attribute__((visibility("default"))) int dn_fuse_detections(const float* boxes, const float* scores, const int64_t* labels,
                                                                        const int32_t* counts, const float* offsets, const float* weights,
                                                                        int s_total, int d, const int32_t* group_begin, int groups, float thresh,
                                                                        float skip_thresh, int d_out, float* boxes_out, float* scores_out,
                                                                        int64_t* labels_out, int32_t* counts_out, int32_t* members_out,
                                                                        void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = detset_check("dn_fuse_detections", boxes, scores, labels, counts, offsets, s_total, d, group_begin, groups, d_out, boxes_out,
                                    scores_out, labels_out, counts_out, workspace))
        return rc;
    DN_REQUIRE(thresh >= 0.f && skip_thresh >= 0.f, "dn_fuse_detections: thresh=%g and skip_thresh=%g must be numbers >= 0", (double)thresh,
               (double)skip_thresh);
    if (d_out > FZ_MAX_D || !fuse_supported(s_total, d, group_begin, groups)) {
        dn_set_error("dn_fuse_detections: d=%d and d_out=%d at most %d, at most %d slots (sources * d) per group, s_total * d below 2^31", d, d_out,
                     FZ_MAX_D, FZ_MAX_SLOTS);
        return DN_E_UNSUPPORTED;
    }
    const size_t n_slots = (size_t)s_total * d;
    if (workspace_bytes < fuse_buffers(nullptr, n_slots).bytes) {
        dn_set_error("dn_fuse_detections: workspace of %zu B, %zu B needed", workspace_bytes, fuse_buffers(nullptr, n_slots).bytes);
        return DN_E_WORKSPACE;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    FuseArgs a;
    a.boxes = reinterpret_cast<const float4*>(boxes); a.scores = scores; a.labels = labels; a.offsets = reinterpret_cast<const float2*>(offsets);
    a.weights = weights;
    a.b = fuse_buffers(workspace, n_slots);
    a.d = d; a.d_out = d_out; a.thresh = thresh;
    a.boxes_out = reinterpret_cast<float4*>(boxes_out); a.scores_out = scores_out; a.labels_out = labels_out; a.counts_out = counts_out;
    a.members_out = members_out;
    dn_note_kernel("fuse_keys_kernel");
    hipLaunchKernelGGL(fuse_keys_kernel, dim3(dn_cdiv((long)n_slots, FZ_NT)), dim3(FZ_NT), 0, s, scores, counts, weights, skip_thresh, (int)n_slots, d,
                       a.b.keys, a.b.rank, a.b.order);
    for (int g0 = 0; g0 < groups; g0 += DS_GROUPS) {
        GroupTab gt;
        const int slots = detset_chunk(group_begin, groups, g0, d, gt);
        detset_rank(a.b.keys, a.b.rank, a.b.order, d, gt, slots, s);
        dn_note_kernel("fuse_walk_kernel");
        hipLaunchKernelGGL(fuse_walk_kernel, dim3(gt.count), dim3(FZ_WAVE), 0, s, a, gt);
        detset_rank(a.b.keys, a.b.rank, nullptr, d, gt, slots, s);      // the clusters, by the keys the walk has left
        dn_note_kernel("fuse_emit_kernel");
        hipLaunchKernelGGL(fuse_emit_kernel, dim3(dn_cdiv(slots > d_out ? slots : d_out, FZ_NT), gt.count), dim3(FZ_NT), 0, s, a, gt);
    }
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}
