// Sliced inference: the two device steps around the tile forwards of SSD.detect_sliced.
//   dn_crop_tiles        one gather launch: equal-size tiles of one [3][h][w] image -> [t][3][th][tw], the input of dn_forward
//   dn_merge_detections  hard NMS over detections that already exist: the outputs of dn_forward for several sources (tiles, the whole image,
//                        flipped passes, other models), shifted by one offset per source, merged per output image (group)
// The merge is keys -> ranking (detset.hip, shared with the box fusion) -> walk. Compiled with -ffp-contract=off: the overlap must round like the
// formula of oracle/nms_c.c. No inline asm, no atomics in this file.
#include <vector>

#include "detset.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// crop
// ---------------------------------------------------------------------------------------------------------
constexpr int CROP_NT = 256, CROP_ILP = 4;      // elements (floats, or 16-byte chunks) a thread moves: loads first, then stores

// grid (chunks of a plane, 3 channels, tiles). A tile whose rows start on 16-byte boundaries in both arrays (vec_ok: w % 4 == 0, tw % 4 == 0, both
// bases aligned; and its own x0 % 4 == 0) moves as float4, any other tile as floats: the branch is uniform per workgroup.
__global__ __launch_bounds__(CROP_NT) void crop_tiles_kernel(const float* __restrict__ img, int h, int w, const int32_t* __restrict__ origins, int th,
                                                             int tw, float* __restrict__ out, int vec_ok) {
    const int tile = blockIdx.z, c = blockIdx.y;
    const int x0 = origins[2 * tile], y0 = origins[2 * tile + 1];
    if (x0 < 0 || y0 < 0 || x0 > w - tw || y0 > h - th) return;      // (the host has refused such a call; never read outside the image)
    const float* src = img + ((size_t)c * h + y0) * w + x0;
    float* dst = out + ((size_t)tile * 3 + c) * th * tw;
    const int e0 = blockIdx.x * (CROP_NT * CROP_ILP) + threadIdx.x;
    if (vec_ok && (x0 & 3) == 0) {
        const int rw = tw >> 2, plane = th * rw;
        float4 v[CROP_ILP];
#pragma unroll
        for (int u = 0; u < CROP_ILP; ++u) {      // (an index beyond the plane re-reads the plane's last chunk and stores nothing)
            const int e = min(e0 + u * CROP_NT, plane - 1), r = e / rw, cx = e - r * rw;
            v[u] = *reinterpret_cast<const float4*>(src + (size_t)r * w + 4 * cx);
        }
#pragma unroll
        for (int u = 0; u < CROP_ILP; ++u) {
            const int e = e0 + u * CROP_NT;
            if (e < plane) *reinterpret_cast<float4*>(dst + 4 * (size_t)e) = v[u];      // (rows of tw = 4 rw floats are contiguous in the output)
        }
    } else {
        const int plane = th * tw;
#pragma unroll
        for (int q = 0; q < 4; ++q) {      // the same bytes per workgroup as the 16-byte path
            const int eq = (blockIdx.x * 4 + q) * (CROP_NT * CROP_ILP) + threadIdx.x;
            float v[CROP_ILP];
#pragma unroll
            for (int u = 0; u < CROP_ILP; ++u) {
                const int e = min(eq + u * CROP_NT, plane - 1), r = e / tw, cx = e - r * tw;
                v[u] = src[(size_t)r * w + cx];
            }
#pragma unroll
            for (int u = 0; u < CROP_ILP; ++u) {
                const int e = eq + u * CROP_NT;
                if (e < plane) dst[e] = v[u];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// merge
// ---------------------------------------------------------------------------------------------------------
constexpr int MG_MAX_D = 512, MG_MAX_SOURCES = 1024, MG_MAX_SLOTS = 65536;
constexpr int MG_NT = 256;                 // threads of the keys and walk workgroups; the walk's chunk

struct MergeBuffers {
    unsigned* keys;       // [N] score as an unsigned that orders like the float; 0: not a candidate
    unsigned* rank;       // [N] candidates of the same group that rank higher
    unsigned* order;      // [N] flattened index of the candidate of each rank, per group from the group's first slot; DS_END behind the last
    size_t bytes;
};
MergeBuffers merge_buffers(void* ws, size_t n_slots) {
    MergeBuffers b;
    unsigned char* p = reinterpret_cast<unsigned char*>(ws);
    b.keys = reinterpret_cast<unsigned*>(p); p += a256(n_slots * 4);
    b.rank = reinterpret_cast<unsigned*>(p); p += a256(n_slots * 4);
    b.order = reinterpret_cast<unsigned*>(p); p += a256(n_slots * 4);
    b.bytes = (size_t)(p - reinterpret_cast<unsigned char*>(ws));
    return b;
}

// Launch 1, one thread per slot (source s, row j; flattened index i = s * d + j): the key of a candidate (j < counts[s], score not NaN) is its
// score's dn_order_key, which is never 0; every other slot gets 0. Also clears what the two ranking launches (detset.hip) fill.
__global__ __launch_bounds__(MG_NT) void merge_keys_kernel(const float* __restrict__ scores, const int32_t* __restrict__ counts, int n_slots, int d,
                                                           unsigned* __restrict__ keys, unsigned* __restrict__ rank, unsigned* __restrict__ order) {
    const int i = blockIdx.x * MG_NT + threadIdx.x;
    if (i >= n_slots) return;
    const int s = i / d, j = i - s * d;
    const float sc = scores[i];
    unsigned k = 0u;
    if (j < counts[s] && sc == sc) k = dn_order_key(sc);
    keys[i] = k;
    rank[i] = 0u;
    order[i] = DS_END;
}

struct MergeArgs {
    const float4* boxes; const float* scores; const int64_t* labels; const float2* offsets;
    const unsigned* order;
    int d, metric, class_agnostic, d_out, thresh_nonneg;
    float thresh;
    float4* boxes_out; float* scores_out; int64_t* labels_out; int32_t* counts_out; int32_t* src_out;
};

// Does the kept box a (area aa) suppress the candidate b (area ab)? fp32, the operation order of oracle/nms_c.c. A NaN overlap does not suppress.
// skip0: thresh >= 0, so a pair without intersection (overlap 0 or NaN) cannot pass `> thresh` and the division is not needed.
__device__ __forceinline__ bool mg_suppresses(const float4 a, const float aa, const float4 b, const float ab, const int metric, const float thresh,
                                              const bool skip0) {
    const float inter = dn_box_inter(a, b);
    if (skip0 && inter == 0.0f) return false;
    const float den = metric == DN_MERGE_IOS ? (aa < ab ? aa : ab) : (aa + ab - inter);
    return inter / den > thresh;
}

// a 64-bit value that every lane of the wave holds alike, as scalars: loops over its bits then run on the scalar unit
__device__ __forceinline__ unsigned long long mg_uniform64(const unsigned long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// Launch 4 (2 and 3 are detset_rank), one workgroup per group: the greedy walk down the ranking in chunks of 256 candidates.
//   1. thread t takes the candidate of rank pos + t and tests it against the kept list (LDS, at most d_out <= 512 boxes);
//   2. every survivor builds its row of the chunk's 256 x 256-bit matrix "the surviving candidate j < t of this chunk suppresses me";
//   3. wave 0 resolves the chunk in rank order, 64 candidates at a time: candidates suppressed by the kept ones of the earlier 64s fall away,
//      then the lowest remaining candidate is kept and its column (a ballot) removes what it suppresses, until nothing remains;
//   4. the kept ones append themselves to the kept list and to the outputs at (kept so far + kept ones below them in the chunk).
// The walk ends when d_out are kept or the ranking is exhausted; the rows behind the count are cleared.
__global__ __launch_bounds__(MG_NT) void merge_walk_kernel(MergeArgs a, GroupTab gt) {
    __shared__ float4 kbox[MG_MAX_D];
    __shared__ float karea[MG_MAX_D];
    __shared__ long long klabel[MG_MAX_D];
    __shared__ float4 cbox[MG_NT];
    __shared__ float carea[MG_NT];
    __shared__ long long clabel[MG_NT];
    __shared__ unsigned long long maskw[4][MG_NT];      // [word][candidate]: conflict-free for the writers (step 2) and for wave 0 (step 3)
    __shared__ unsigned long long alive_w[4], kept_w[4];
    __shared__ int last_chunk;

    const int g = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int base = gt.begin[g] * a.d, n = (gt.begin[g + 1] - gt.begin[g]) * a.d;
    const int G = gt.first + g;
    const bool skip0 = a.thresh_nonneg != 0, any_label = a.class_agnostic != 0;
    const int d_out = a.d_out;
    int nk = 0;
    for (int pos = 0; pos < n && nk < d_out; pos += MG_NT) {
        // 1. my candidate
        const unsigned idx = pos + tid < n ? a.order[base + pos + tid] : DS_END;
        const bool valid = idx != DS_END;
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        float sc = 0.f, ar = 0.f;
        long long lb = 0;
        if (valid) {
            const float2 o = a.offsets[idx / (unsigned)a.d];
            b = a.boxes[idx];
            b.x = b.x + o.x; b.y = b.y + o.y; b.z = b.z + o.x; b.w = b.w + o.y;
            sc = a.scores[idx];
            lb = a.labels[idx];
            ar = (b.z - b.x) * (b.w - b.y);
        }
        bool alive = valid;
        for (int k = 0; k < nk; ++k) {
            const float4 kb = kbox[k];
            const float ka = karea[k];
            const long long kl = klabel[k];
            if (alive && (any_label || kl == lb) && mg_suppresses(kb, ka, b, ar, a.metric, a.thresh, skip0)) alive = false;
        }
        cbox[tid] = b; carea[tid] = ar; clabel[tid] = lb;
        const unsigned long long bal = __ballot(alive);
        if (lane == 0) alive_w[wave] = bal;
        if (tid == MG_NT - 1) last_chunk = valid ? 0 : 1;
        __syncthreads();
        // 2. my row of the chunk's matrix: words 0 .. wave (candidates below 64 * (wave + 1))
        unsigned long long m[4] = {0ull, 0ull, 0ull, 0ull};
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w <= wave) {
                const unsigned long long aw = mg_uniform64(alive_w[w]);
                for (unsigned long long rem = aw; rem != 0ull; rem &= rem - 1ull) {      // surviving candidates of this word only (uniform)
                    const int jj = __builtin_ctzll(rem), j = 64 * w + jj;
                    if (alive && j < tid && (any_label || clabel[j] == lb) && mg_suppresses(cbox[j], carea[j], b, ar, a.metric, a.thresh, skip0))
                        m[w] |= 1ull << jj;
                }
            }
            maskw[w][tid] = m[w];
        }
        __syncthreads();
        // 3. wave 0 resolves the chunk
        if (wave == 0) {
            unsigned long long kept[4] = {0ull, 0ull, 0ull, 0ull};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                bool dead = false;
#pragma unroll
                for (int w = 0; w < c; ++w) dead = dead || (maskw[w][64 * c + lane] & kept[w]) != 0ull;
                const unsigned long long mc = maskw[c][64 * c + lane];
                unsigned long long rem = mg_uniform64(alive_w[c]) & ~__ballot(dead);
                unsigned long long kc = 0ull;
                while (rem != 0ull) {
                    const int i = __builtin_ctzll(rem);
                    kc |= 1ull << i;
                    rem &= ~(1ull << i);
                    rem &= ~__ballot(((mc >> i) & 1ull) != 0ull);
                }
                kept[c] = kc;
                if (lane == 0) kept_w[c] = kc;
            }
        }
        __syncthreads();
        // 4. append
        int below = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const unsigned long long kw = kept_w[w];
            total += __popcll(kw);
            if (w < wave) below += __popcll(kw);
            else if (w == wave) below += __popcll(kw & ((1ull << lane) - 1ull));
        }
        const bool kept_me = ((kept_w[wave] >> lane) & 1ull) != 0ull;
        const int at = nk + below;
        if (kept_me && at < d_out) {
            kbox[at] = b; karea[at] = ar; klabel[at] = lb;
            const size_t o = (size_t)G * d_out + at;
            a.boxes_out[o] = b;
            a.scores_out[o] = sc;
            a.labels_out[o] = lb;
            if (a.src_out) a.src_out[o] = (int32_t)idx;
        }
        nk = min(nk + total, d_out);
        const int last = last_chunk;
        __syncthreads();
        if (last) break;
    }
    for (int r = nk + tid; r < d_out; r += MG_NT) {
        const size_t o = (size_t)G * d_out + r;
        a.boxes_out[o] = make_float4(0.f, 0.f, 0.f, 0.f);
        a.scores_out[o] = 0.f;
        a.labels_out[o] = 0;
        if (a.src_out) a.src_out[o] = -1;
    }
    if (tid == 0) a.counts_out[G] = nk;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int dn_crop_tiles(const float* image, int h, int w, const int32_t* origins, int t, int th, int tw,
                                                                   float* out, void* stream) {
    DN_REQUIRE(image && origins && out, "dn_crop_tiles: null argument");
    DN_REQUIRE(h >= 1 && w >= 1 && t >= 1 && th >= 1 && tw >= 1, "dn_crop_tiles: bad sizes h=%d w=%d t=%d th=%d tw=%d", h, w, t, th, tw);
    DN_REQUIRE(th <= h && tw <= w, "dn_crop_tiles: a %d x %d tile does not fit a %d x %d image", th, tw, h, w);
    DN_REQUIRE(t <= 65535 && (long long)th * tw <= 0x7FFFFFFFll / 4, "dn_crop_tiles: t=%d above 65535, or a tile of more than 2^29 pixels", t);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // the origins are device data and a tile outside the image must be refused, not read: they are read back here (8 t bytes; waits for `stream`)
    std::vector<int32_t> o(2 * (size_t)t);
    DN_HIP_CHECK(hipMemcpyAsync(o.data(), origins, o.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    DN_HIP_CHECK(hipStreamSynchronize(s));
    for (int i = 0; i < t; ++i)
        DN_REQUIRE(o[2 * i] >= 0 && o[2 * i + 1] >= 0 && o[2 * i] <= w - tw && o[2 * i + 1] <= h - th,
                   "dn_crop_tiles: tile %d at (x0=%d, y0=%d) of %d x %d leaves the %d x %d image", i, o[2 * i], o[2 * i + 1], th, tw, h, w);
    const int vec_ok = (w % 4 == 0 && tw % 4 == 0 && ((reinterpret_cast<size_t>(image) | reinterpret_cast<size_t>(out)) & 15) == 0) ? 1 : 0;
    const int per_wg = CROP_NT * CROP_ILP * 4;      // floats per workgroup on either path
    dn_note_kernel("crop_tiles_kernel");
    hipLaunchKernelGGL(crop_tiles_kernel, dim3(dn_cdiv((long)th * tw, per_wg), 3, t), dim3(CROP_NT), 0, s, image, h, w, origins, th, tw, out, vec_ok);
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}

extern "C" __attribute__((visibility("default"))) size_t dn_merge_detections_workspace_bytes(int s_total, int d, int groups) {
    if (!detset_sizes_ok(s_total, d, groups) || d > MG_MAX_D || (long long)s_total * d > 0x7FFFFFFFll) return 0;
    return merge_buffers(nullptr, (size_t)s_total * d).bytes;
}

extern "C" __attribute__((visibility("default"))) int dn_merge_detections(const float* boxes, const float* scores, const int64_t* labels,
                                                                         const int32_t* counts, const float* offsets, int s_total, int d,
                                                                         const int32_t* group_begin, int groups, int metric, float thresh,
                                                                         int class_agnostic, int d_out, float* boxes_out, float* scores_out,
                                                                         int64_t* labels_out, int32_t* counts_out, int32_t* src_out, void* workspace,
                                                                         size_t workspace_bytes, void* stream) {
    if (const int rc = detset_check("dn_merge_detections", boxes, scores, labels, counts, offsets, s_total, d, group_begin, groups, d_out, boxes_out,
                                    scores_out, labels_out, counts_out, workspace))
        return rc;
    DN_REQUIRE(metric == DN_MERGE_IOU || metric == DN_MERGE_IOS, "dn_merge_detections: unknown metric %d", metric);
    DN_REQUIRE(class_agnostic == 0 || class_agnostic == 1, "dn_merge_detections: class_agnostic must be 0 or 1, got %d", class_agnostic);
    DN_REQUIRE(thresh == thresh, "dn_merge_detections: thresh is NaN");
    if (d > MG_MAX_D || d_out > MG_MAX_D || (long long)s_total * d > 0x7FFFFFFFll) {
        dn_set_error("dn_merge_detections: d=%d and d_out=%d at most %d, s_total * d below 2^31", d, d_out, MG_MAX_D);
        return DN_E_UNSUPPORTED;
    }
    for (int g = 0; g < groups; ++g) {
        const int ns = group_begin[g + 1] - group_begin[g];
        if (ns > MG_MAX_SOURCES || (long long)ns * d > MG_MAX_SLOTS) {
            dn_set_error("dn_merge_detections: group %d has %d sources of %d rows; at most %d sources and %d slots (sources * d) per group", g, ns, d,
                         MG_MAX_SOURCES, MG_MAX_SLOTS);
            return DN_E_UNSUPPORTED;
        }
    }
    const size_t n_slots = (size_t)s_total * d;
    if (workspace_bytes < merge_buffers(nullptr, n_slots).bytes) {
        dn_set_error("dn_merge_detections: workspace of %zu B, %zu B needed", workspace_bytes, merge_buffers(nullptr, n_slots).bytes);
        return DN_E_WORKSPACE;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const MergeBuffers mb = merge_buffers(workspace, n_slots);
    dn_note_kernel("merge_keys_kernel");
    hipLaunchKernelGGL(merge_keys_kernel, dim3(dn_cdiv((long)n_slots, MG_NT)), dim3(MG_NT), 0, s, scores, counts, (int)n_slots, d, mb.keys, mb.rank,
                       mb.order);
    MergeArgs a;
    a.boxes = reinterpret_cast<const float4*>(boxes); a.scores = scores; a.labels = labels; a.offsets = reinterpret_cast<const float2*>(offsets);
    a.order = mb.order;
    a.d = d; a.metric = metric; a.class_agnostic = class_agnostic; a.d_out = d_out; a.thresh = thresh; a.thresh_nonneg = thresh >= 0.f ? 1 : 0;
    a.boxes_out = reinterpret_cast<float4*>(boxes_out); a.scores_out = scores_out; a.labels_out = labels_out; a.counts_out = counts_out;
    a.src_out = src_out;
    for (int g0 = 0; g0 < groups; g0 += DS_GROUPS) {
        GroupTab gt;
        const int slots = detset_chunk(group_begin, groups, g0, d, gt);
        detset_rank(mb.keys, mb.rank, mb.order, d, gt, slots, s);
        dn_note_kernel("merge_walk_kernel");
        hipLaunchKernelGGL(merge_walk_kernel, dim3(gt.count), dim3(MG_NT), 0, s, a, gt);
    }
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}
