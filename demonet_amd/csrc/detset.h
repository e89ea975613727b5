// A set of detections from several sources, grouped per output image: what dn_merge_detections (sliced.hip), dn_fuse_detections (fuse.hip) and
// dn_track_update (track.hip) share. Sources are rows of [s_total][d] arrays; group g of a call is the sources group_begin[g] ..
// group_begin[g + 1] - 1; slot i = s * d + j is row j of source s. A reducer writes one key per slot (0: not a candidate), has the keys of each
// group ranked (detset.hip) and walks down the ranking.
#pragma once
#include "common.h"

constexpr int DS_NT = 256;                 // threads of the ranking workgroups
constexpr int DS_GROUPS = 64;              // groups per launch: their source ranges travel as a kernel argument (no host array is read later)
constexpr unsigned DS_END = 0xFFFFFFFFu;   // order[]: no candidate of this rank

struct GroupTab {
    int count;
    int begin[DS_GROUPS + 1];      // sources begin[g] .. begin[g + 1] - 1 form group g of this launch
    int first;                     // index of group 0 of this launch among the call's groups
};

// a float as an unsigned with the order of the floats (-0 counts as +0: the two compare equal), never 0; a NaN ranks behind every number (-inf
// maps to 0x007FFFFF). Whether a NaN, or any other value, is a candidate at all is the caller's test, made before the call.
__device__ __forceinline__ unsigned dn_order_key(const float f) {
    if (f != f) return 1u;
    const unsigned u = f == 0.f ? 0u : __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Area of the intersection of the boxes a and b (x1, y1, x2, y2): fp32, the operation order of oracle/nms_c.c. Every overlap of the library's
// reducers starts here; the early-out and the denominator are the caller's (they differ on NaN, and must).
__device__ __forceinline__ float dn_box_inter(const float4 a, const float4 b) {
    const float xx1 = a.x > b.x ? a.x : b.x, yy1 = a.y > b.y ? a.y : b.y;
    const float xx2 = a.z < b.z ? a.z : b.z, yy2 = a.w < b.w ? a.w : b.w;
    float w = xx2 - xx1, h = yy2 - yy1;
    if (w < 0.0f) w = 0.0f;
    if (h < 0.0f) h = 0.0f;
    return w * h;
}

// host side (detset.hip)
bool detset_sizes_ok(int s_total, int d, int groups);
bool detset_groups_ok(const int32_t* group_begin, int groups, int s_total);      // does not decrease, stays in 0 .. s_total
// The checks the entry points share, with `who` in front of the message: no NULL among the arrays every call needs, sizes >= 1, boxes / boxes_out /
// workspace 16-byte aligned, offsets / labels / labels_out 8-byte aligned, group_begin as above. DN_OK or DN_E_INVALID. The limits are the caller's.
int detset_check(const char* who, const float* boxes, const float* scores, const int64_t* labels, const int32_t* counts, const float* offsets,
                 int s_total, int d, const int32_t* group_begin, int groups, int d_out, const float* boxes_out, const float* scores_out,
                 const int64_t* labels_out, const int32_t* counts_out, const void* workspace);
// The call's groups g0 .. g0 + DS_GROUPS - 1 (as many as there are) as the table of one launch; returns the slots of the largest of them.
// for (g0 = 0; g0 < groups; g0 += DS_GROUPS) visits every group once.
int detset_chunk(const int32_t* group_begin, int groups, int g0, int d, GroupTab& gt);
// Ranks the keys of every group of the table: rank[i] = keys of the group that are larger than keys[i], or equal with a smaller index (rank[] must be
// 0 where keys[] is not; slots as detset_chunk returned it, nothing is launched for 0). With `order` (DS_END everywhere), also
// order[first slot of the group + rank] = slot: the ranking a walk reads.
void detset_rank(const unsigned* keys, unsigned* rank, unsigned* order, int d, const GroupTab& gt, int slots, hipStream_t s);
