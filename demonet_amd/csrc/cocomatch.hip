// COCO detection matching on the device: dn_coco_match marks the padded detections dn_forward wrote against padded ground truth,
// per image, the way pycocotools' COCOeval.computeIoU + evaluateImg do (semantics: include/demonet_hip.h).
//   one workgroup per image; everything the walk reads is staged in LDS once, SORTED: detections by (label, rank), ground truths by (label, slot),
//   so a category is one contiguous run of each
//   1. positions by counting on LDS keys (c x c and g x g compares); the rank-0 detection of a label enters its category in a table
//   2. one lane per (category, threshold) chain walks the category's detections in rank order; it carries the R area ranges together: one fp64
//      IoU per (detection, ground truth) serves all of them, each range has its own pair of candidates (best not-ignored, best ignored) and its
//      own matched bits. The two passes of evaluateImg (not-ignored ground truths first, ignored ones only if none matched) become one sweep in
//      slot order: the bar only rises on a match, so the ignored pass starts from the untouched bar whenever its result is used.
//   3. matched bits: one bit per (threshold, range, sorted ground truth) in LDS. Chains of different labels share 32-bit words, so the bits are
//      set with LDS atomic OR and read with atomic loads; a bit is only ever written by the one chain that reads it.
// Compiled with -ffp-contract=off: every fp64 operation rounds on its own, as the C of maskApi.c does. No inline asm; the only global atomics are
// 64-bit integer additions into gt_stats, whose sum does not depend on their order.
#include <cmath>

#include "common.h"

namespace {

constexpr int CM_NT = 512;            // threads per workgroup
constexpr int CM_MAX_D = 512, CM_MAX_G = 1024, CM_MAX_T = 16, CM_MAX_R = 4, CM_MAX_N = 65535, CM_MAX_DET = 128;
constexpr int CM_GW = CM_MAX_G / 32;  // words of matched bits per (threshold, range)
constexpr unsigned CM_CROWD = 16u;    // g_ign: bit r = ignored in range r, bit 4 = crowd

struct CocoArgs {
    const float4* boxes; const float* scores; const int64_t* labels; const int32_t* counts;
    const float4* gt_boxes; const int64_t* gt_labels; const int32_t* gt_counts; const uint8_t* gt_crowd; const float* gt_area;
    int d, gmax, num_classes, n_thresh, n_ranges, max_det;
    double bar[CM_MAX_T];             // min(threshold, 1 - 1e-10)
    double lo[CM_MAX_R], hi[CM_MAX_R];
    uint32_t* flags; int32_t* rank; int32_t* match_gt; unsigned long long* gt_stats;
};

struct Category { uint16_t start, size, gstart, gsize; };      // runs in the sorted detections and the sorted ground truths

// LDS at the limits: ground truths 16 + 8 + 2 + 1 KB, detections 8 + 4 + 2 + 1 KB, categories 4 KB, detection flags 8 KB, matched bits 8 KB
// = 62 KB (63 492 B with the counter): two workgroups per CU
__global__ __launch_bounds__(CM_NT) void coco_match_kernel(CocoArgs a) {
    __shared__ float4 g_box[CM_MAX_G];                      // x, y, w, h; sorted by (label, slot)
    __shared__ int64_t g_label[CM_MAX_G];                   // by slot
    __shared__ uint16_t g_slot[CM_MAX_G];                   // sorted position -> slot
    __shared__ uint8_t g_ign[CM_MAX_G];                     // sorted
    __shared__ float4 d_box[CM_MAX_D];                      // x, y, w, h; sorted by (label, rank)
    __shared__ int64_t d_label[CM_MAX_D];                   // by slot
    __shared__ unsigned d_key[CM_MAX_D];                    // by slot: the score as an unsigned that orders like the float; 0 for a NaN score
    __shared__ uint16_t d_slot[CM_MAX_D];                   // sorted position -> slot
    __shared__ Category cat[CM_MAX_D];
    __shared__ unsigned d_flags[CM_MAX_D * CM_MAX_R];       // [sorted position][R]
    __shared__ unsigned matched[CM_MAX_T * CM_MAX_R * CM_GW];
    __shared__ unsigned n_cat;

    const int img = blockIdx.x, tid = threadIdx.x;
    const int d = a.d, gmax = a.gmax, T = a.n_thresh, R = a.n_ranges;
    const int c = min(max(a.counts[img], 0), d);            // (never index beyond the arrays, whatever the counts hold)
    const int g = min(max(a.gt_counts[img], 0), gmax);
    const size_t crow = (size_t)img * d, grow = (size_t)img * gmax;

    for (int k = tid; k < g; k += CM_NT) g_label[k] = a.gt_labels[grow + k];
    for (int j = tid; j < c; j += CM_NT) {
        d_label[j] = a.labels[crow + j];
        const float sc = a.scores[crow + j];
        unsigned key = 0u;
        if (sc == sc) {
            const unsigned u = sc == 0.f ? 0u : __float_as_uint(sc);      // (-0 ranks as +0: the two compare equal)
            key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);           // never 0 for a number
        }
        d_key[j] = key;
    }
    for (int w = tid; w < T * R * CM_GW; w += CM_NT) matched[w] = 0u;
    for (int w = tid; w < c * R; w += CM_NT) d_flags[w] = 0u;
    if (tid == 0) n_cat = 0u;
    __syncthreads();

    // ground truths: sorted position by counting, xywh, the ignore bits, gt_stats
    for (int k = tid; k < g; k += CM_NT) {
        const int64_t lb = g_label[k];
        int at = 0;
        for (int i = 0; i < g; ++i) {
            const int64_t li = g_label[i];
            at += (li < lb || (li == lb && i < k)) ? 1 : 0;
        }
        const float4 b = a.gt_boxes[grow + k];
        const float w = b.z - b.x, h = b.w - b.y;           // fp32, as the records carry them
        const bool crowd = a.gt_crowd ? a.gt_crowd[grow + k] != 0 : false;
        const double area = a.gt_area ? (double)a.gt_area[grow + k] : (double)w * (double)h;
        unsigned ign = crowd ? CM_CROWD : 0u;
        for (int r = 0; r < R; ++r) {
            const bool ig = crowd || area < a.lo[r] || area > a.hi[r];
            ign |= ig ? (1u << r) : 0u;
            if (!ig && a.gt_stats && lb >= 0 && lb < (int64_t)a.num_classes) atomicAdd(&a.gt_stats[lb * R + r], 1ull);
        }
        g_box[at] = make_float4(b.x, b.y, w, h);
        g_slot[at] = (uint16_t)k;
        g_ign[at] = (uint8_t)ign;
    }
    // detections: sorted position and rank by counting; the rank-0 detection of a label describes the category
    for (int j = tid; j < c; j += CM_NT) {
        const int64_t lb = d_label[j];
        const unsigned key = d_key[j];
        int below = 0, before = 0, same = 0;
        for (int i = 0; i < c; ++i) {
            const int64_t li = d_label[i];
            const unsigned ki = d_key[i];
            below += li < lb ? 1 : 0;
            same += li == lb ? 1 : 0;
            before += (li == lb && (ki > key || (ki == key && i < j))) ? 1 : 0;
        }
        const float4 b = a.boxes[crow + j];
        d_box[below + before] = make_float4(b.x, b.y, b.z - b.x, b.w - b.y);
        d_slot[below + before] = (uint16_t)j;
        a.rank[crow + j] = before;
        if (before == 0) {
            int gbelow = 0, gsame = 0;
            for (int i = 0; i < g; ++i) {
                const int64_t li = g_label[i];
                gbelow += li < lb ? 1 : 0;
                gsame += li == lb ? 1 : 0;
            }
            const unsigned ci = atomicAdd(&n_cat, 1u);      // (the order of the table does not reach any output)
            cat[ci] = Category{(uint16_t)below, (uint16_t)same, (uint16_t)gbelow, (uint16_t)gsame};
        }
    }
    __syncthreads();

    // the walk: chain = (category, threshold); neighbouring lanes share a category, so their LDS reads are broadcasts
    const int chains = (int)n_cat * T;
    for (int ch = tid; ch < chains; ch += CM_NT) {
        const Category cg = cat[ch / T];
        const int b = ch % T;
        const double bar0 = a.bar[b];
        const int nd = min((int)cg.size, a.max_det);
        unsigned* const rows = matched + b * R * CM_GW;
        for (int q = 0; q < (int)cg.size; ++q) {
            const int pos = cg.start + q;
            const size_t slot = crow + d_slot[pos];
            if (q >= nd) {                                  // cut by max_det: flags stay 0
                if (a.match_gt)
                    for (int r = 0; r < R; ++r) a.match_gt[(slot * R + r) * T + b] = -1;
                continue;
            }
            const float4 db = d_box[pos];
            const double dx = db.x, dy = db.y, dw = db.z, dh = db.w;
            const double da = dw * dh, dxe = dw + dx, dye = dh + dy;
            double bar1[CM_MAX_R], bar2[CM_MAX_R];          // best not-ignored candidate, best ignored candidate
            int m1[CM_MAX_R], m2[CM_MAX_R];
#pragma unroll
            for (int r = 0; r < CM_MAX_R; ++r) { bar1[r] = bar0; bar2[r] = bar0; m1[r] = -1; m2[r] = -1; }
            for (int gq = 0; gq < (int)cg.gsize; ++gq) {
                const int gp = cg.gstart + gq;
                const float4 gb = g_box[gp];
                const unsigned ign = g_ign[gp];
                const bool crowd = (ign & CM_CROWD) != 0u;
                const double gx = gb.x, gy = gb.y, gw = gb.z, gh = gb.w;
                double iou = 0.0;
                const double iw = fmin(dxe, gw + gx) - fmax(dx, gx);
                if (!(iw <= 0.0)) {
                    const double ih = fmin(dye, gh + gy) - fmax(dy, gy);
                    if (!(ih <= 0.0)) {
                        const double inter = iw * ih;
                        const double uni = crowd ? da : da + gw * gh - inter;
                        iou = inter / uni;
                    }
                }
#pragma unroll
                for (int r = 0; r < CM_MAX_R; ++r) {
                    if (r >= R) continue;
                    const unsigned word = __hip_atomic_load(&rows[r * CM_GW + (gp >> 5)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (((word >> (gp & 31)) & 1u) && !crowd) continue;
                    if ((ign >> r) & 1u) {
                        if (iou < bar2[r]) continue;
                        bar2[r] = iou; m2[r] = gp;
                    } else {
                        if (iou < bar1[r]) continue;
                        bar1[r] = iou; m1[r] = gp;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < CM_MAX_R; ++r) {
                if (r >= R) continue;
                const int m = m1[r] >= 0 ? m1[r] : m2[r];
                unsigned bits = 0u;
                if (m >= 0) {
                    atomicOr(&rows[r * CM_GW + (m >> 5)], 1u << (m & 31));
                    bits = 1u << b;
                    if ((g_ign[m] >> r) & 1u) bits |= 1u << (16 + b);
                } else if (da < a.lo[r] || da > a.hi[r]) {
                    bits = 1u << (16 + b);
                }
                if (bits) atomicOr(&d_flags[pos * R + r], bits);
                if (a.match_gt) a.match_gt[(slot * R + r) * T + b] = m >= 0 ? (int)g_slot[m] : -1;
            }
        }
    }
    __syncthreads();

    for (int w = tid; w < c * R; w += CM_NT) a.flags[(crow + d_slot[w / R]) * R + w % R] = d_flags[w];
    for (int j = c + tid; j < d; j += CM_NT) {              // dead slots
        a.rank[crow + j] = -1;
        for (int r = 0; r < R; ++r) {
            a.flags[(crow + j) * R + r] = 0u;
            if (a.match_gt)
                for (int b = 0; b < T; ++b) a.match_gt[((crow + j) * R + r) * T + b] = -1;
        }
    }
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int dn_coco_match(const float* boxes, const float* scores, const int64_t* labels, const int32_t* counts,
                                                                   const float* gt_boxes, const int64_t* gt_labels, const int32_t* gt_counts,
                                                                   const uint8_t* gt_crowd, const float* gt_area, int n, int d, int gmax, int num_classes,
                                                                   const double* thresholds, int n_thresh, const double* area_ranges, int n_ranges,
                                                                   int max_det, uint32_t* flags, int32_t* rank, int32_t* match_gt, int64_t* gt_stats,
                                                                   void* stream) {
    DN_REQUIRE(boxes && scores && labels && counts && gt_boxes && gt_labels && gt_counts && thresholds && area_ranges && flags && rank,
               "dn_coco_match: null argument");
    DN_REQUIRE(n >= 1 && d >= 1 && gmax >= 1 && n_thresh >= 1 && n_ranges >= 1 && max_det >= 1,
               "dn_coco_match: bad sizes n=%d d=%d gmax=%d n_thresh=%d n_ranges=%d max_det=%d", n, d, gmax, n_thresh, n_ranges, max_det);
    DN_REQUIRE(!gt_stats || num_classes >= 1, "dn_coco_match: num_classes=%d with gt_stats given", num_classes);
    DN_REQUIRE(((reinterpret_cast<size_t>(boxes) | reinterpret_cast<size_t>(gt_boxes)) & 15) == 0 &&
                   ((reinterpret_cast<size_t>(labels) | reinterpret_cast<size_t>(gt_labels) | reinterpret_cast<size_t>(gt_stats)) & 7) == 0 &&
                   ((reinterpret_cast<size_t>(scores) | reinterpret_cast<size_t>(counts) | reinterpret_cast<size_t>(gt_counts) |
                     reinterpret_cast<size_t>(gt_area) | reinterpret_cast<size_t>(flags) | reinterpret_cast<size_t>(rank) |
                     reinterpret_cast<size_t>(match_gt)) & 3) == 0,
               "dn_coco_match: boxes and gt_boxes must be 16-byte aligned, labels, gt_labels and gt_stats 8-byte aligned, the other arrays 4-byte aligned");
    if (d > CM_MAX_D || gmax > CM_MAX_G || n_thresh > CM_MAX_T || n_ranges > CM_MAX_R || n > CM_MAX_N || max_det > CM_MAX_DET) {
        dn_set_error("dn_coco_match: d=%d at most %d, gmax=%d at most %d, n_thresh=%d at most %d, n_ranges=%d at most %d, n=%d at most %d, max_det=%d at most %d",
                     d, CM_MAX_D, gmax, CM_MAX_G, n_thresh, CM_MAX_T, n_ranges, CM_MAX_R, n, CM_MAX_N, max_det, CM_MAX_DET);
        return DN_E_UNSUPPORTED;
    }
    CocoArgs a;
    for (int b = 0; b < CM_MAX_T; ++b) {
        const double t = b < n_thresh ? thresholds[b] : 0.0;
        DN_REQUIRE(t == t, "dn_coco_match: threshold %d is NaN", b);
        a.bar[b] = t < 1.0 - 1e-10 ? t : 1.0 - 1e-10;
    }
    for (int r = 0; r < CM_MAX_R; ++r) {
        a.lo[r] = r < n_ranges ? area_ranges[2 * r] : 0.0;
        a.hi[r] = r < n_ranges ? area_ranges[2 * r + 1] : 0.0;
        DN_REQUIRE(a.lo[r] == a.lo[r] && a.hi[r] == a.hi[r], "dn_coco_match: area range %d holds a NaN", r);
    }
    a.boxes = reinterpret_cast<const float4*>(boxes); a.scores = scores; a.labels = labels; a.counts = counts;
    a.gt_boxes = reinterpret_cast<const float4*>(gt_boxes); a.gt_labels = gt_labels; a.gt_counts = gt_counts; a.gt_crowd = gt_crowd; a.gt_area = gt_area;
    a.d = d; a.gmax = gmax; a.num_classes = num_classes; a.n_thresh = n_thresh; a.n_ranges = n_ranges; a.max_det = max_det;
    a.flags = flags; a.rank = rank; a.match_gt = match_gt; a.gt_stats = reinterpret_cast<unsigned long long*>(gt_stats);
    dn_note_kernel("coco_match_kernel");
    hipLaunchKernelGGL(coco_match_kernel, dim3(n), dim3(CM_NT), 0, reinterpret_cast<hipStream_t>(stream), a);
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}
