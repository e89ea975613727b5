// PASCAL VOC true / false positive marking on the device: dn_match_detections scores the padded detections dn_forward wrote
// against padded ground truth, per image, with the arithmetic of the reference's voc_eval (data/voc_eval.py:116-155; semantics: include/demonet_hip.h).
//   one workgroup per image; ground truths staged in LDS once; every candidate is owned by one thread
//   1. best ground truth per candidate: c x g IoUs in fp64, only for pairs of equal label (the division is skipped for the others)
//   2. rank inside the image by counting, on keys in LDS
//   3. per threshold: one LDS integer min per candidate into a [gmax] table (the best-ranked claimant of each ground truth), one compare
// Compiled with -ffp-contract=off: every fp64 operation rounds on its own, as numpy's float64 does. No inline asm; the only global atomics are
// 64-bit integer additions into gt_stats, whose sum does not depend on their order.
#include <cmath>

#include "common.h"

namespace {

constexpr int EM_NT = 512;            // threads per workgroup: one candidate each at the largest d (the loops cover any d all the same)
constexpr int EM_MAX_D = 512, EM_MAX_G = 1024, EM_MAX_T = 16, EM_MAX_N = 65535;
constexpr unsigned EM_FREE = 0xFFFFFFFFu;

struct MatchArgs {
    const float4* boxes; const float* scores; const int64_t* labels; const int32_t* counts;
    const float4* gt_boxes; const int64_t* gt_labels; const uint8_t* gt_difficult; const int32_t* gt_counts;
    int d, gmax, num_classes, n_thresh;
    double offset;
    double thresholds[EM_MAX_T];
    uint32_t* flags; int32_t* best_gt; double* best_ov; unsigned long long* gt_stats;
};

// numpy's minimum / maximum: a NaN operand gives NaN
__device__ __forceinline__ double np_min(double a, double b) { return (a != a) ? a : ((b != b) ? b : (a < b ? a : b)); }
__device__ __forceinline__ double np_max(double a, double b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }

// LDS at the limits: 16 + 8 + 1 + 4 KB for the ground truths, 2 + 2 + 2 + 4 KB for the candidates = 39 KB
__global__ __launch_bounds__(EM_NT) void match_detections_kernel(MatchArgs a) {
    __shared__ float4 g_box[EM_MAX_G];
    __shared__ int64_t g_label[EM_MAX_G];
    __shared__ double c_ov[EM_MAX_D];
    __shared__ unsigned g_claim[EM_MAX_G];      // per threshold: the lowest rank among the candidates that pass on this ground truth
    __shared__ unsigned c_key[EM_MAX_D];        // the score as an unsigned that orders like the float; 0 for a NaN score
    __shared__ int c_gt[EM_MAX_D];
    __shared__ unsigned c_rank[EM_MAX_D];
    __shared__ uint8_t g_diff[EM_MAX_G];

    const int img = blockIdx.x, tid = threadIdx.x;
    const int d = a.d, gmax = a.gmax;
    const int c = min(max(a.counts[img], 0), d);            // (never index beyond the arrays, whatever the counts hold)
    const int g = min(max(a.gt_counts[img], 0), gmax);
    const size_t crow = (size_t)img * d, grow = (size_t)img * gmax;

    for (int k = tid; k < g; k += EM_NT) {
        g_box[k] = a.gt_boxes[grow + k];
        const int64_t lb = a.gt_labels[grow + k];
        g_label[k] = lb;
        const bool diff = a.gt_difficult ? a.gt_difficult[grow + k] != 0 : false;
        g_diff[k] = diff ? 1 : 0;
        if (a.gt_stats && lb >= 0 && lb < (int64_t)a.num_classes) atomicAdd(&a.gt_stats[2 * lb + (diff ? 1 : 0)], 1ull);
    }
    for (int j = tid; j < c; j += EM_NT) {
        const float sc = a.scores[crow + j];
        unsigned key = 0u;
        if (sc == sc) {
            const unsigned u = sc == 0.f ? 0u : __float_as_uint(sc);      // (-0 ranks as +0: the two compare equal)
            key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);           // never 0 for a number
        }
        c_key[j] = key;
    }
    __syncthreads();

    // best ground truth of every candidate, and its rank
    const double o = a.offset;
    for (int j = tid; j < c; j += EM_NT) {
        const float4 bf = a.boxes[crow + j];
        const int64_t lb = a.labels[crow + j];
        const double x1 = bf.x, y1 = bf.y, x2 = bf.z, y2 = bf.w;
        const double area = (x2 - x1 + o) * (y2 - y1 + o);
        double best = -INFINITY;
        int at = -1;
        bool any_nan = false;
        for (int k = 0; k < g; ++k) {
            if (g_label[k] != lb) continue;
            const float4 gf = g_box[k];
            const double gx1 = gf.x, gy1 = gf.y, gx2 = gf.z, gy2 = gf.w;
            const double iw = np_max(np_min(gx2, x2) - np_max(gx1, x1) + o, 0.0);
            const double ih = np_max(np_min(gy2, y2) - np_max(gy1, y1) + o, 0.0);
            const double inter = iw * ih;
            const double uni = area + (gx2 - gx1 + o) * (gy2 - gy1 + o) - inter;
            const double ov = inter / uni;
            if (ov != ov) any_nan = true;
            if (at < 0 || ov > best) { best = ov; at = k; }      // strict: the lowest k that attains the maximum
        }
        if (any_nan) { best = NAN; at = -1; }
        c_ov[j] = best;
        c_gt[j] = at;
        const unsigned key = c_key[j];
        unsigned r = 0u;
        for (int i = 0; i < c; ++i) {
            const unsigned ki = c_key[i];
            r += (ki > key || (ki == key && i < j)) ? 1u : 0u;
        }
        c_rank[j] = r;
    }

    // marking: for one threshold, the true positive on ground truth k is the best-ranked candidate among those with best_gt == k that pass
    uint32_t fl[(EM_MAX_D + EM_NT - 1) / EM_NT];
#pragma unroll
    for (int u = 0; u < (EM_MAX_D + EM_NT - 1) / EM_NT; ++u) fl[u] = 0u;
    for (int b = 0; b < a.n_thresh; ++b) {
        const double t = a.thresholds[b];
        __syncthreads();                                     // (the previous threshold's reads of g_claim are over)
        for (int k = tid; k < g; k += EM_NT) g_claim[k] = EM_FREE;
        __syncthreads();
        for (int j = tid; j < c; j += EM_NT)
            if (c_ov[j] > t && c_gt[j] >= 0) atomicMin(&g_claim[c_gt[j]], c_rank[j]);
        __syncthreads();
#pragma unroll
        for (int u = 0; u < (EM_MAX_D + EM_NT - 1) / EM_NT; ++u) {
            const int j = tid + u * EM_NT;
            if (j >= c) continue;
            const int at = c_gt[j];
            if (c_ov[j] > t && at >= 0) {
                if (!g_diff[at]) fl[u] |= (g_claim[at] == c_rank[j]) ? (1u << b) : (1u << (16 + b));
            } else {
                fl[u] |= 1u << (16 + b);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < (EM_MAX_D + EM_NT - 1) / EM_NT; ++u) {
        const int j = tid + u * EM_NT;
        if (j >= d) continue;
        const bool live = j < c;
        a.flags[crow + j] = live ? fl[u] : 0u;
        if (a.best_gt) a.best_gt[crow + j] = live ? c_gt[j] : -1;
        if (a.best_ov) a.best_ov[crow + j] = live ? c_ov[j] : 0.0;
    }
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int dn_match_detections(const float* boxes, const float* scores, const int64_t* labels,
                                                                         const int32_t* counts, const float* gt_boxes, const int64_t* gt_labels,
                                                                         const uint8_t* gt_difficult, const int32_t* gt_counts, int n, int d, int gmax,
                                                                         int num_classes, const double* thresholds, int n_thresh, double pixel_offset,
                                                                         uint32_t* flags, int32_t* best_gt, double* best_ov, int64_t* gt_stats,
                                                                         void* stream) {
    DN_REQUIRE(boxes && scores && labels && counts && gt_boxes && gt_labels && gt_counts && thresholds && flags, "dn_match_detections: null argument");
    DN_REQUIRE(n >= 1 && d >= 1 && gmax >= 1 && n_thresh >= 1, "dn_match_detections: bad sizes n=%d d=%d gmax=%d n_thresh=%d", n, d, gmax, n_thresh);
    DN_REQUIRE(!gt_stats || num_classes >= 1, "dn_match_detections: num_classes=%d with gt_stats given", num_classes);
    DN_REQUIRE(std::isfinite(pixel_offset) && pixel_offset >= 0.0, "dn_match_detections: pixel_offset must be finite and not negative, got %g", pixel_offset);
    DN_REQUIRE(((reinterpret_cast<size_t>(boxes) | reinterpret_cast<size_t>(gt_boxes)) & 15) == 0 &&
                   ((reinterpret_cast<size_t>(labels) | reinterpret_cast<size_t>(gt_labels) | reinterpret_cast<size_t>(best_ov) |
                     reinterpret_cast<size_t>(gt_stats)) & 7) == 0,
               "dn_match_detections: boxes and gt_boxes must be 16-byte aligned, labels, gt_labels, best_ov and gt_stats 8-byte aligned");
    if (d > EM_MAX_D || gmax > EM_MAX_G || n_thresh > EM_MAX_T || n > EM_MAX_N) {
        dn_set_error("dn_match_detections: d=%d at most %d, gmax=%d at most %d, n_thresh=%d at most %d, n=%d at most %d", d, EM_MAX_D, gmax, EM_MAX_G,
                     n_thresh, EM_MAX_T, n, EM_MAX_N);
        return DN_E_UNSUPPORTED;
    }
    MatchArgs a;
    for (int b = 0; b < EM_MAX_T; ++b) {
        a.thresholds[b] = b < n_thresh ? thresholds[b] : 0.0;
        DN_REQUIRE(a.thresholds[b] == a.thresholds[b], "dn_match_detections: threshold %d is NaN", b);
    }
    a.boxes = reinterpret_cast<const float4*>(boxes); a.scores = scores; a.labels = labels; a.counts = counts;
    a.gt_boxes = reinterpret_cast<const float4*>(gt_boxes); a.gt_labels = gt_labels; a.gt_difficult = gt_difficult; a.gt_counts = gt_counts;
    a.d = d; a.gmax = gmax; a.num_classes = num_classes; a.n_thresh = n_thresh;
    a.offset = pixel_offset + 0.0;
    a.flags = flags; a.best_gt = best_gt; a.best_ov = best_ov; a.gt_stats = reinterpret_cast<unsigned long long*>(gt_stats);
    dn_note_kernel("match_detections_kernel");
    hipLaunchKernelGGL(match_detections_kernel, dim3(n), dim3(EM_NT), 0, reinterpret_cast<hipStream_t>(stream), a);
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}
