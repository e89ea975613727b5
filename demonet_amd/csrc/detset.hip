// The ranking of a detection set (detset.h): rank by counting and the scatter into rank order, for the keys of up to DS_GROUPS groups per launch,
// and the host pieces around them that dn_merge_detections (sliced.hip) and dn_fuse_detections (fuse.hip) share -- the argument checks and the
// walk over group_begin in tables of DS_GROUPS groups. Compiled with -ffp-contract=off like its users (there is no float arithmetic here). No
// inline asm; the only atomics are unsigned additions of partial counts, whose sum does not depend on their order.
#include "detset.h"

namespace {

constexpr int DS_OTHERS = 2048;            // keys one rank workgroup compares its 256 keys with

// Rank by counting: grid (blocks of 256 own keys, chunks of DS_OTHERS other keys, groups). The rank of a key is the number of keys of its group
// that are larger, or equal with a smaller index. Both ranges are aligned to 256, so a 256-key piece of the chunk lies entirely below the own keys
// (equal counts), entirely above (equal does not count) or is the own block itself. The partial counts of the chunks meet in rank[] by unsigned
// atomic addition: the sum is the same in any order.
__global__ __launch_bounds__(DS_NT) void detset_rank_kernel(const unsigned* __restrict__ keys, unsigned* __restrict__ rank, int d, GroupTab gt) {
    __shared__ unsigned tile[DS_OTHERS];
    const int g = blockIdx.z;
    const int base = gt.begin[g] * d, n = (gt.begin[g + 1] - gt.begin[g]) * d;
    const int i0 = blockIdx.x * DS_NT, j0 = blockIdx.y * DS_OTHERS;
    if (i0 >= n || j0 >= n) return;
    const int tid = threadIdx.x, i = i0 + tid;
    const unsigned mine = i < n ? keys[base + i] : 0u;
    if (!__syncthreads_or(mine != 0u)) return;
#pragma unroll
    for (int u = 0; u < DS_OTHERS / DS_NT; ++u) {
        const int j = j0 + u * DS_NT + tid;
        tile[u * DS_NT + tid] = j < n ? keys[base + j] : 0u;
    }
    __syncthreads();
    unsigned cnt = 0u;
    for (int u = 0; u < DS_OTHERS / DS_NT; ++u) {
        const int js = j0 + u * DS_NT;
        if (js >= n) break;
        const uint4* t4 = reinterpret_cast<const uint4*>(&tile[u * DS_NT]);
        if (js < i0) {
#pragma unroll 8
            for (int q = 0; q < DS_NT / 4; ++q) {
                const uint4 o = t4[q];
                cnt += (o.x >= mine) + (o.y >= mine) + (o.z >= mine) + (o.w >= mine);
            }
        } else if (js > i0) {
#pragma unroll 8
            for (int q = 0; q < DS_NT / 4; ++q) {
                const uint4 o = t4[q];
                cnt += (o.x > mine) + (o.y > mine) + (o.z > mine) + (o.w > mine);
            }
        } else {
#pragma unroll 8
            for (int q = 0; q < DS_NT / 4; ++q) {
                const uint4 o = t4[q];
                const int jq = 4 * q;
                cnt += (o.x > mine || (o.x == mine && jq + 0 < tid)) + (o.y > mine || (o.y == mine && jq + 1 < tid)) +
                       (o.z > mine || (o.z == mine && jq + 2 < tid)) + (o.w > mine || (o.w == mine && jq + 3 < tid));
            }
        }
    }
    if (mine != 0u) atomicAdd(&rank[base + i], cnt);
}

// order[first slot of the group + rank] = flattened index. Ranks of a group's candidates are 0 .. candidates - 1, each once.
__global__ __launch_bounds__(DS_NT) void detset_scatter_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ rank,
                                                               unsigned* __restrict__ order, int d, GroupTab gt) {
    const int g = blockIdx.y;
    const int base = gt.begin[g] * d, n = (gt.begin[g + 1] - gt.begin[g]) * d;
    const int i = blockIdx.x * DS_NT + threadIdx.x;
    if (i >= n || keys[base + i] == 0u) return;
    const unsigned r = rank[base + i];
    if (r < (unsigned)n) order[base + r] = (unsigned)(base + i);
}

}  // namespace

bool detset_sizes_ok(int s_total, int d, int groups) { return s_total >= 1 && d >= 1 && groups >= 1; }

bool detset_groups_ok(const int32_t* group_begin, int groups, int s_total) {
    if (group_begin[0] < 0 || group_begin[groups] > s_total) return false;
    for (int g = 0; g < groups; ++g)
        if (group_begin[g] > group_begin[g + 1]) return false;
    return true;
}

int detset_check(const char* who, const float* boxes, const float* scores, const int64_t* labels, const int32_t* counts, const float* offsets,
                 int s_total, int d, const int32_t* group_begin, int groups, int d_out, const float* boxes_out, const float* scores_out,
                 const int64_t* labels_out, const int32_t* counts_out, const void* workspace) {
    DN_REQUIRE(boxes && scores && labels && counts && offsets && group_begin && boxes_out && scores_out && labels_out && counts_out && workspace,
               "%s: null argument", who);
    DN_REQUIRE(detset_sizes_ok(s_total, d, groups) && d_out >= 1, "%s: bad sizes s_total=%d d=%d groups=%d d_out=%d", who, s_total, d, groups, d_out);
    DN_REQUIRE(((reinterpret_cast<size_t>(boxes) | reinterpret_cast<size_t>(boxes_out) | reinterpret_cast<size_t>(workspace)) & 15) == 0 &&
                   ((reinterpret_cast<size_t>(offsets) | reinterpret_cast<size_t>(labels) | reinterpret_cast<size_t>(labels_out)) & 7) == 0,
               "%s: boxes, boxes_out and the workspace must be 16-byte aligned, offsets and labels 8-byte aligned", who);
    DN_REQUIRE(detset_groups_ok(group_begin, groups, s_total), "%s: group_begin must not decrease and must stay in 0 .. s_total=%d", who, s_total);
    return DN_OK;
}

int detset_chunk(const int32_t* group_begin, int groups, int g0, int d, GroupTab& gt) {
    gt.count = groups - g0 < DS_GROUPS ? groups - g0 : DS_GROUPS;
    gt.first = g0;
    int slots = 0;
    for (int g = 0; g <= DS_GROUPS; ++g) gt.begin[g] = group_begin[g0 + (g < gt.count ? g : gt.count)];
    for (int g = 0; g < gt.count; ++g) slots = (gt.begin[g + 1] - gt.begin[g]) * d > slots ? (gt.begin[g + 1] - gt.begin[g]) * d : slots;
    return slots;
}

void detset_rank(const unsigned* keys, unsigned* rank, unsigned* order, int d, const GroupTab& gt, int slots, hipStream_t s) {
    if (slots <= 0) return;
    dn_note_kernel("detset_rank_kernel");
    hipLaunchKernelGGL(detset_rank_kernel, dim3(dn_cdiv(slots, DS_NT), dn_cdiv(slots, DS_OTHERS), gt.count), dim3(DS_NT), 0, s, keys, rank, d, gt);
    if (!order) return;
    dn_note_kernel("detset_scatter_kernel");
    hipLaunchKernelGGL(detset_scatter_kernel, dim3(dn_cdiv(slots, DS_NT), gt.count), dim3(DS_NT), 0, s, keys, rank, order, d, gt);
}
