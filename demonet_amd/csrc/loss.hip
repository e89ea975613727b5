// SSD training loss: anchor <-> ground-truth matching, box regression (smooth L1) and classification (cross entropy with hard
// negative mining) -- the value (dn_ssd_loss) and its gradient with respect to both head outputs (dn_ssd_loss_train +
// dn_ssd_loss_backward). SURVEY section 8(f) row 4 -- the step right after the hot path's head outputs when the model is evaluated or
// trained against targets. The backward through the backbone and the heads is not here: the gradients stop at the head outputs.
//
// reference ops replaced:
//   generalized_ssd.py:316-330   per image: box_iou(gt boxes, anchors) -> SSDMatcher
//   _utils.py:264-294,348-362    Matcher with low == high threshold (matches = argmax over gt, -1 below the threshold), then SSDMatcher:
//                                every gt keeps the anchor it overlaps most (matches[argmax over anchors] = gt index, later gts win)
//   torchvision.ops.boxes.box_iou (third-party, published formula): inter / (area1 + area2 - inter), clamp(min=0) on the extents
//   generalized_ssd.py:210-269   compute_loss: encode_boxes (_utils.py:100-133, weights (10, 10, 5, 5)), smooth_l1_loss(sum, beta 1),
//                                cross_entropy(reduction none), hard negative mining = the neg_to_pos_ratio * (#label > 0) largest
//                                losses among the non-foreground anchors of the image, both sums divided by max(1, #matched)
// The reference ranks the negatives with two sorts; only the SUM of the selected losses enters the result, and that sum does not
// depend on how ties at the cut are ordered -- so the selection here is an exact radix select (threshold + quota), not a sort.
// Everything is fp32 in the reference's operation order; sums are taken in a fixed order (deterministic, last-bit different from
// torch.sum's pairwise order: the parity tests use rtol 1e-5).
// The gradient needs the SET of mined negatives, not only their sum: ties at the cut are taken in anchor order (what a stable
// descending sort gives, as for the spill corner), by an ordered count over the tie positions -- see ssd_weight_kernel.
#include <math.h>

#include "common.h"

namespace {

constexpr int GMAX = 256;       // ground-truth boxes per image held in LDS

// torchvision.ops.boxes.box_iou of one (gt, anchor) pair, one rounding per operation as its separate torch ops round: rb - lt, clamp(min=0),
// inter = w * h, union = (area1 + area2) - inter, inter / union (area1 = the gt's, area2 = the anchor's). Contracted to an fma the union
// would see the unrounded product; on boxes that tie -- anchors that share a centre, an IoU of exactly the threshold -- that last bit
// decides the match. The division is the correctly rounded fp32 sequence either way.
__device__ __forceinline__ float match_iou(const float4 b, const float area_b, const float4 ab, const float area_ab) {
#pragma clang fp contract(off)
    const float w = fmaxf(fminf(b.z, ab.z) - fmaxf(b.x, ab.x), 0.f);
    const float h = fmaxf(fminf(b.w, ab.w) - fmaxf(b.y, ab.y), 0.f);
    const float inter = w * h;
    const float both = area_b + area_ab;
    const float uni = both - inter;
    return inter / uni;
}

// ---- matching: one workgroup per image ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ssd_match_kernel(const float4* __restrict__ anchors, const float4* __restrict__ gt_boxes,
                                                       const int* __restrict__ gt_counts, int A, int gmax, float iou_thresh,
                                                       long long* __restrict__ matched) {
    __shared__ float4 gb[GMAX];
    __shared__ float ga[GMAX];
    __shared__ unsigned long long best_for_gt[GMAX];       // (iou bits << 32) | ~anchor: max = highest IoU, lowest anchor index on ties
    const int n = blockIdx.x, tid = threadIdx.x;
    const int G = min(gt_counts[n], gmax);
    long long* mrow = matched + (size_t)n * A;
    if (G <= 0) {           // generalized_ssd.py:318-321: no boxes -> every anchor is background
        for (int a = tid; a < A; a += 256) mrow[a] = -1;
        return;
    }
    for (int g = tid; g < G; g += 256) {
        const float4 b = gt_boxes[(size_t)n * gmax + g];
        gb[g] = b;
        ga[g] = (b.z - b.x) * (b.w - b.y);
        best_for_gt[g] = 0ull;
    }
    __syncthreads();
    for (int a = tid; a < A; a += 256) {
        const float4 ab = anchors[a];
        const float aa = (ab.z - ab.x) * (ab.w - ab.y);
        float best = -1.f;
        int best_g = 0;
        for (int g = 0; g < G; ++g) {
            const float iou = match_iou(gb[g], ga[g], ab, aa);
            if (iou > best) { best = iou; best_g = g; }                 // max over dim 0: first maximum
            // IoU >= 0: its float bits order like the value. NaN (0 / 0 of two degenerate boxes) never wins a comparison.
            if (iou >= 0.f) atomicMax(&best_for_gt[g], ((unsigned long long)__float_as_uint(iou) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)a));
        }
        mrow[a] = best >= iou_thresh ? (long long)best_g : -1ll;       // low == high threshold: BETWEEN_THRESHOLDS cannot occur
    }
    __syncthreads();
    if (tid == 0)
        for (int g = 0; g < G; ++g) {                                   // matches[argmax_a iou(g, a)] = g, in gt order (the last gt wins)
            const unsigned a = 0xFFFFFFFFu - (unsigned)(best_for_gt[g] & 0xFFFFFFFFull);
            if (a < (unsigned)A) mrow[a] = g;
        }
}

// encode_boxes (_utils.py:100-133, weights (10, 10, 5, 5)) of ground-truth box g against anchor ab: one spelling for the value and the
// gradient, so both see the same target bits
__device__ __forceinline__ void encode_target(const float4 ab, const float4 g, float t[4]) {
    const float ew = ab.z - ab.x, eh = ab.w - ab.y, ecx = ab.x + 0.5f * ew, ecy = ab.y + 0.5f * eh;
    const float gw = g.z - g.x, gh = g.w - g.y, gcx = g.x + 0.5f * gw, gcy = g.y + 0.5f * gh;
    t[0] = 10.f * (gcx - ecx) / ew;
    t[1] = 10.f * (gcy - ecy) / eh;
    t[2] = 5.f * logf(gw / ew);
    t[3] = 5.f * logf(gh / eh);
}

// ---- per anchor: cross entropy, foreground flag, smooth-L1 of the encoded target ------------------------------------------------
__global__ __launch_bounds__(256) void ssd_anchor_loss_kernel(const float* __restrict__ logits, const float* __restrict__ reg,
                                                             const float4* __restrict__ anchors, const float4* __restrict__ gt_boxes,
                                                             const long long* __restrict__ gt_labels, const long long* __restrict__ matched,
                                                             int A, int K, int gmax, float* __restrict__ ce, float* __restrict__ bbox_partial,
                                                             int* __restrict__ fg_partial) {
    __shared__ float red[256];
    __shared__ int redi[256];
    const int n = blockIdx.y, a = blockIdx.x * 256 + threadIdx.x;
    float bl = 0.f;
    int matched_cnt = 0;
    if (a < A) {
        const long long m = matched[(size_t)n * A + a];
        const long long target = m >= 0 ? gt_labels[(size_t)n * gmax + m] : 0;
        const float* row = logits + ((size_t)n * A + a) * K;
        float mx = row[0];
        for (int k = 1; k < K; ++k) mx = fmaxf(mx, row[k]);
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += expf(row[k] - mx);
        const float lse = mx + logf(s);
        const float c = lse - row[target];                               // F.cross_entropy(..., reduction='none')
        // foreground for the mining: label > 0 (generalized_ssd.py:255); the loss keeps its value, a flag rides in the sign bit of
        // a separate array
        ce[(size_t)n * A + a] = c;
        if (m >= 0) {
            matched_cnt = 1;
            const float4 ab = anchors[a], g = gt_boxes[(size_t)n * gmax + m];
            const float4 r = reinterpret_cast<const float4*>(reg)[(size_t)n * A + a];
            float t[4];
            encode_target(ab, g, t);
            const float p[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float d = fabsf(p[q] - t[q]);
                bl += d < 1.f ? 0.5f * d * d : d - 0.5f;                  // smooth_l1_loss, beta = 1
            }
        }
    }
    red[threadIdx.x] = bl;
    redi[threadIdx.x] = matched_cnt;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { red[threadIdx.x] += red[threadIdx.x + s]; redi[threadIdx.x] += redi[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        bbox_partial[(size_t)n * gridDim.x + blockIdx.x] = red[0];
        fg_partial[(size_t)n * gridDim.x + blockIdx.x] = redi[0];
    }
}

// ---- per image: hard negative mining (exact top-k sum by radix select), foreground classification sum -----------------------------
__global__ __launch_bounds__(1024) void ssd_mine_kernel(const float* __restrict__ ce, const long long* __restrict__ matched,
                                                       const long long* __restrict__ gt_labels, int A, int gmax, float neg_to_pos_ratio,
                                                       float* __restrict__ cls_partial /*[n][2]: foreground sum, mined background sum*/,
                                                       unsigned* __restrict__ select_out /*optional [n][4]: T, need, want, spill (ssd_weight_kernel)*/) {
    __shared__ unsigned hist[256];
    __shared__ float redf[1024];
    __shared__ unsigned redu[1024];
    __shared__ unsigned sh[4];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* c = ce + (size_t)n * A;
    auto is_fg = [&](int a) {
        const long long m = matched[(size_t)n * A + a];
        return m >= 0 && gt_labels[(size_t)n * gmax + m] > 0;
    };
    auto block_sum_f = [&](float v) {
        redf[tid] = v;
        __syncthreads();
        for (int s = 512; s > 0; s >>= 1) { if (tid < s) redf[tid] += redf[tid + s]; __syncthreads(); }
        const float r = redf[0];
        __syncthreads();
        return r;
    };
    auto block_sum_u = [&](unsigned v) {
        redu[tid] = v;
        __syncthreads();
        for (int s = 512; s > 0; s >>= 1) { if (tid < s) redu[tid] += redu[tid + s]; __syncthreads(); }
        const unsigned r = redu[0];
        __syncthreads();
        return r;
    };
    float fsum = 0.f;
    unsigned nfg = 0;
    for (int a = tid; a < A; a += 1024)
        if (is_fg(a)) { fsum += c[a]; ++nfg; }
    const float fg_sum = block_sum_f(fsum);
    const unsigned num_fg = block_sum_u(nfg);
    const unsigned num_bg_total = (unsigned)A - num_fg;
    // rank < neg_to_pos_ratio * #foreground (a float product in the reference, (1 - 0.25) / 0.25 = 3.0 by default): ceil of it entries
    unsigned long long want64 = (unsigned long long)ceil((double)neg_to_pos_ratio * (double)num_fg);
    unsigned want = want64 > (unsigned long long)A ? (unsigned)A : (unsigned)want64;
    float bg_sum = 0.f;
    unsigned sel_T = 0, sel_need = 0;
    // more negatives wanted than exist: every negative counts, and the ranking runs into the -inf entries of the foreground anchors
    // (generalized_ssd.py:258-262: "positive values that creeped in the sample") -- in a stable descending sort those keep their
    // index order, so the first (want - #negatives) foreground anchors are counted a second time
    unsigned spill = 0;
    if (want > num_bg_total) { spill = want - num_bg_total; want = num_bg_total; }
    if (want > 0) {
        // cross entropy >= 0: float bits order like the values. 4 x 8-bit radix select of the want-th largest negative loss
        unsigned prefix = 0, need = want;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (int a = tid; a < A; a += 1024) {
                if (is_fg(a)) continue;
                const unsigned k = __float_as_uint(fmaxf(c[a], 0.f));
                if (shift == 24 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(k >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned acc = 0;
                int d = 255;
                for (; d > 0; --d) { if (acc + hist[d] >= need) break; acc += hist[d]; }
                sh[0] = (unsigned)d;
                sh[1] = need - acc;
            }
            __syncthreads();
            prefix |= sh[0] << shift;
            need = sh[1];
            __syncthreads();
        }
        const unsigned T = prefix;              // the want-th largest key; `need` of the entries equal to it are taken
        float s = 0.f;
        for (int a = tid; a < A; a += 1024) {
            if (is_fg(a)) continue;
            const float v = fmaxf(c[a], 0.f);
            if (__float_as_uint(v) > T) s += v;
        }
        bg_sum = block_sum_f(s) + (float)need * __uint_as_float(T);
        sel_T = T;
        sel_need = need;
    }
    if (spill > 0) {
        // the first `spill` foreground anchors in index order (rare: more than A / (1 + ratio) foreground anchors)
        float s = 0.f;
        if (tid == 0) {
            unsigned taken = 0;
            for (int a = 0; a < A && taken < spill; ++a)
                if (is_fg(a)) { s += c[a]; ++taken; }
        }
        bg_sum += block_sum_f(s);
    }
    if (tid == 0) {
        cls_partial[2 * n] = fg_sum;
        cls_partial[2 * n + 1] = bg_sum;
        if (select_out) {
            select_out[4 * n] = sel_T;
            select_out[4 * n + 1] = sel_need;
            select_out[4 * n + 2] = want;
            select_out[4 * n + 3] = spill;
        }
    }
}

__global__ void ssd_loss_final_kernel(const float* __restrict__ bbox_partial, const int* __restrict__ fg_partial, const float* __restrict__ cls_partial,
                                      int n, int blocks_per_image, float* __restrict__ losses,
                                      float* __restrict__ normaliser_out /*optional: max(1, #matched), for the backward*/) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float bbox = 0.f, cls = 0.f;
    long long nf = 0;
    for (int i = 0; i < n; ++i) {
        float b = 0.f;
        for (int q = 0; q < blocks_per_image; ++q) { b += bbox_partial[(size_t)i * blocks_per_image + q]; nf += fg_partial[(size_t)i * blocks_per_image + q]; }
        bbox += b;
        cls += cls_partial[2 * i] + cls_partial[2 * i + 1];
    }
    const float N = (float)(nf > 1 ? nf : 1);
    losses[0] = bbox / N;
    losses[1] = cls / N;
    if (normaliser_out) *normaliser_out = N;
}

// ---- per image: the weight of every anchor's cross entropy in the classification sum ----------------------------------------------
// w = (label > 0) + (mined negative), 0 / 1 / 2. The mined set is what a stable descending sort of the negatives gives: every key
// above the threshold T of ssd_mine_kernel, and of the keys equal to T the `need` with the lowest anchor index; in the spill corner
// the first `spill` foreground anchors by index count twice. Ranks among the ties (and among the foreground anchors) are an ordered
// count: ballot + popcount inside a wave, a prefix over the 16 wave totals, a running base across the 1024-anchor chunks.
__global__ __launch_bounds__(1024) void ssd_weight_kernel(const float* __restrict__ ce, const long long* __restrict__ matched,
                                                         const long long* __restrict__ gt_labels, const unsigned* __restrict__ select,
                                                         int A, int gmax, unsigned char* __restrict__ weight) {
    __shared__ unsigned wave_tie[16], wave_fg[16];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned T = select[4 * n], need = select[4 * n + 1], want = select[4 * n + 2], spill = select[4 * n + 3];
    const float* c = ce + (size_t)n * A;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned tie_base = 0, fg_base = 0;
    for (int base = 0; base < A; base += 1024) {
        const int a = base + tid;
        bool fg = false, tie = false, above = false;
        if (a < A) {
            const long long m = matched[(size_t)n * A + a];
            fg = m >= 0 && gt_labels[(size_t)n * gmax + m] > 0;
            if (!fg && want > 0) {
                const unsigned k = __float_as_uint(fmaxf(c[a], 0.f));
                above = k > T;
                tie = k == T;
            }
        }
        const unsigned long long tie_mask = __ballot(tie), fg_mask = __ballot(fg);
        if (lane == 0) { wave_tie[wave] = (unsigned)__popcll(tie_mask); wave_fg[wave] = (unsigned)__popcll(fg_mask); }
        __syncthreads();
        unsigned tie_rank = tie_base + (unsigned)__popcll(tie_mask & below), fg_rank = fg_base + (unsigned)__popcll(fg_mask & below);
        unsigned tie_total = 0, fg_total = 0;
        for (int q = 0; q < 16; ++q) {
            const unsigned t = wave_tie[q], f = wave_fg[q];
            if (q < wave) { tie_rank += t; fg_rank += f; }
            tie_total += t;
            fg_total += f;
        }
        if (a < A) weight[(size_t)n * A + a] = fg ? (fg_rank < spill ? 2 : 1) : (above || (tie && tie_rank < need) ? 1 : 0);
        tie_base += tie_total;
        fg_base += fg_total;
        __syncthreads();
    }
}

// ---- gradient of both losses with respect to the head outputs ---------------------------------------------------------------------
// d cls / d logits[row][k] = g_cls * w[row] * (softmax(row)[k] - [k == target]) / N; d bbox / d reg[row][q] = g_box * clamp(p - t, -1, 1) / N
// for matched anchors. One workgroup per tile of ROWS (64, or 16 for wide rows: more and smaller tiles keep every CU busy to the end)
// consecutive rows, n and A flattened: the tile's slice of the logit gradient is contiguous and 16-byte aligned (ROWS * K floats from
// a multiple of ROWS rows, ROWS a multiple of 4), so it is zero-filled with float4 stores without reading
// a logit; then the few rows with w > 0 (a few per cent at the default 3:1 mining) are overwritten, LANES lanes per row striding it
// (coalesced loads and stores), max and sum by cross-lane reduction, softmax as expf(x - max) / sum like the forward.
template <int LANES, int ROWS>
__global__ __launch_bounds__(256) void ssd_loss_backward_kernel(const float* __restrict__ logits, const float* __restrict__ reg,
                                                               const float4* __restrict__ anchors, const float4* __restrict__ gt_boxes,
                                                               const long long* __restrict__ gt_labels, const long long* __restrict__ matched,
                                                               const unsigned char* __restrict__ weight, const float* __restrict__ normaliser,
                                                               const float* __restrict__ grad_losses, long long rows_total, int A, int K, int gmax,
                                                               float* __restrict__ grad_logits, float4* __restrict__ grad_reg) {
    static_assert(ROWS % 4 == 0 && ROWS <= 64, "a tile is 16-byte aligned and its rows are flagged by one wave");
    __shared__ int sel[ROWS];
    __shared__ int nsel;
    const int tid = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * ROWS;
    const int rows = (int)(rows_total - row0 < ROWS ? rows_total - row0 : ROWS);
    const float N = *normaliser;
    if (grad_reg && tid < rows) {
        const long long row = row0 + tid;
        const long long m = matched[row];
        float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m >= 0) {
            const int img = (int)(row / A), a = (int)(row - (long long)img * A);
            const float4 r = reinterpret_cast<const float4*>(reg)[row];
            float t[4];
            encode_target(anchors[a], gt_boxes[(size_t)img * gmax + m], t);
            const float gs = grad_losses[0] / N;
            out.x = gs * fminf(fmaxf(r.x - t[0], -1.f), 1.f);             // smooth_l1_loss', beta = 1
            out.y = gs * fminf(fmaxf(r.y - t[1], -1.f), 1.f);
            out.z = gs * fminf(fmaxf(r.z - t[2], -1.f), 1.f);
            out.w = gs * fminf(fmaxf(r.w - t[3], -1.f), 1.f);
        }
        grad_reg[row] = out;
    }
    if (!grad_logits) return;
    if (tid < 64) {                                                       // wave 0: the tile's rows with w > 0, in row order
        const int wv = tid < rows ? (int)weight[row0 + tid] : 0;
        const unsigned long long mask = __ballot(wv > 0);
        if (wv > 0) sel[__popcll(mask & ((1ull << tid) - 1ull))] = tid | (wv << 8);
        if (tid == 0) nsel = __popcll(mask);
    }
    float* tile = grad_logits + (size_t)row0 * K;
    const int count = rows * K, vec = count >> 2;
    for (int i = tid; i < vec; i += 256) reinterpret_cast<float4*>(tile)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = (vec << 2) + tid; i < count; i += 256) tile[i] = 0.f;    // the last tile of a buffer whose length is not a multiple of 4
    __syncthreads();                                                      // zeros first: the selected rows are stored over them
    const int lane = tid % LANES;
    const float g_cls = grad_losses[1];
    for (int j = tid / LANES; j < nsel; j += 256 / LANES) {
        const long long row = row0 + (sel[j] & 255);
        const long long m = matched[row];
        const int target = m >= 0 ? (int)gt_labels[(size_t)(row / A) * gmax + m] : 0;
        const float* x = logits + (size_t)row * K;
        float* out = grad_logits + (size_t)row * K;
        float mx = -INFINITY;
        for (int k = lane; k < K; k += LANES) mx = fmaxf(mx, x[k]);
#pragma unroll
        for (int o = LANES / 2; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, LANES));
        float s = 0.f;
        for (int k = lane; k < K; k += LANES) s += expf(x[k] - mx);
#pragma unroll
        for (int o = LANES / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, LANES);
        const float scale = g_cls * (float)(sel[j] >> 8) / N;
        for (int k = lane; k < K; k += LANES) out[k] = scale * (expf(x[k] - mx) / s - (k == target ? 1.f : 0.f));
    }
}

// dn_ssd_loss_train's state, in order: matched [n][A] int64, weight [n][A] uint8, select [n][4] uint32, normaliser fp32
struct LossState {
    long long* matched;
    unsigned char* weight;
    unsigned* select;
    float* normaliser;
};

LossState loss_state(void* state, int n, int A) {
    unsigned char* p = reinterpret_cast<unsigned char*>(state);
    LossState st;
    st.matched = reinterpret_cast<long long*>(p); p += a256((size_t)n * A * 8);
    st.weight = p; p += a256((size_t)n * A);
    st.select = reinterpret_cast<unsigned*>(p); p += a256((size_t)n * 4 * 4);
    st.normaliser = reinterpret_cast<float*>(p);
    return st;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) size_t dn_ssd_loss_workspace_bytes(int n, int num_anchors) {
    const size_t blocks = (size_t)dn_cdiv(num_anchors, 256);
    return a256((size_t)n * num_anchors * 8) + a256((size_t)n * num_anchors * 4) + a256((size_t)n * blocks * 4) * 2 + a256((size_t)n * 2 * 4);
}

namespace {

// the launches of dn_ssd_loss; `st` (dn_ssd_loss_train) additionally keeps the matching, the mining cut and the normaliser
int ssd_loss_launch(const char* who, const float* cls_logits, const float* bbox_regression, const float* anchors, const float* gt_boxes,
                    const int64_t* gt_labels, const int32_t* gt_counts, int n, int num_anchors, int num_classes, int gmax, float iou_thresh,
                    float neg_to_pos_ratio, int64_t* matched_idxs, float* losses, void* workspace, size_t workspace_bytes, const LossState* st,
                    hipStream_t s) {
    DN_REQUIRE(cls_logits && bbox_regression && anchors && gt_boxes && gt_labels && gt_counts && losses && workspace, "%s: null argument", who);
    DN_REQUIRE(n > 0 && num_anchors > 0 && num_classes >= 2 && gmax >= 1 && gmax <= GMAX, "%s: bad sizes n=%d A=%d K=%d gmax=%d (gmax <= %d)", who, n,
               num_anchors, num_classes, gmax, GMAX);
    DN_REQUIRE(n <= 65535 && (long long)n * num_anchors < (1LL << 31), "%s: n=%d above 65535 (the image is on grid.y), or n * num_anchors of 2^31 rows or more (int row indices)", who, n);
    DN_REQUIRE(workspace_bytes >= dn_ssd_loss_workspace_bytes(n, num_anchors), "%s: workspace %zu B too small", who, workspace_bytes);
    DN_REQUIRE((reinterpret_cast<size_t>(anchors) & 15) == 0 && (reinterpret_cast<size_t>(gt_boxes) & 15) == 0 && (reinterpret_cast<size_t>(bbox_regression) & 15) == 0,
               "%s: box arrays must be 16-byte aligned", who);
    const int A = num_anchors, blocks = dn_cdiv(A, 256);
    unsigned char* p = reinterpret_cast<unsigned char*>(workspace);
    long long* matched = reinterpret_cast<long long*>(p); p += a256((size_t)n * A * 8);
    float* ce = reinterpret_cast<float*>(p); p += a256((size_t)n * A * 4);
    float* bbox_partial = reinterpret_cast<float*>(p); p += a256((size_t)n * blocks * 4);
    int* fg_partial = reinterpret_cast<int*>(p); p += a256((size_t)n * blocks * 4);
    float* cls_partial = reinterpret_cast<float*>(p);
    if (st) matched = st->matched;
    else if (matched_idxs) matched = reinterpret_cast<long long*>(matched_idxs);
    hipLaunchKernelGGL(ssd_match_kernel, dim3(n), dim3(256), 0, s, reinterpret_cast<const float4*>(anchors), reinterpret_cast<const float4*>(gt_boxes),
                       gt_counts, A, gmax, iou_thresh, matched);
    hipLaunchKernelGGL(ssd_anchor_loss_kernel, dim3(blocks, n), dim3(256), 0, s, cls_logits, bbox_regression, reinterpret_cast<const float4*>(anchors),
                       reinterpret_cast<const float4*>(gt_boxes), reinterpret_cast<const long long*>(gt_labels), matched, A, num_classes, gmax, ce,
                       bbox_partial, fg_partial);
    hipLaunchKernelGGL(ssd_mine_kernel, dim3(n), dim3(1024), 0, s, ce, matched, reinterpret_cast<const long long*>(gt_labels), A, gmax, neg_to_pos_ratio,
                       cls_partial, st ? st->select : nullptr);
    hipLaunchKernelGGL(ssd_loss_final_kernel, dim3(1), dim3(64), 0, s, bbox_partial, fg_partial, cls_partial, n, blocks, losses,
                       st ? st->normaliser : nullptr);
    if (st) {
        hipLaunchKernelGGL(ssd_weight_kernel, dim3(n), dim3(1024), 0, s, ce, matched, reinterpret_cast<const long long*>(gt_labels), st->select, A, gmax,
                           st->weight);
        if (matched_idxs) DN_HIP_CHECK(hipMemcpyAsync(matched_idxs, matched, (size_t)n * A * 8, hipMemcpyDeviceToDevice, s));
    }
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int dn_ssd_loss(const float* cls_logits, const float* bbox_regression, const float* anchors,
                                                                 const float* gt_boxes, const int64_t* gt_labels, const int32_t* gt_counts,
                                                                 int n, int num_anchors, int num_classes, int gmax, float iou_thresh,
                                                                 float neg_to_pos_ratio, int64_t* matched_idxs, float* losses, void* workspace,
                                                                 size_t workspace_bytes, void* stream) {
    return ssd_loss_launch("dn_ssd_loss", cls_logits, bbox_regression, anchors, gt_boxes, gt_labels, gt_counts, n, num_anchors, num_classes, gmax,
                           iou_thresh, neg_to_pos_ratio, matched_idxs, losses, workspace, workspace_bytes, nullptr, reinterpret_cast<hipStream_t>(stream));
}

extern "C" __attribute__((visibility("default"))) size_t dn_ssd_loss_state_bytes(int n, int num_anchors) {
    return a256((size_t)n * num_anchors * 8) + a256((size_t)n * num_anchors) + a256((size_t)n * 4 * 4) + a256(4);
}

extern "C" __attribute__((visibility("default"))) int dn_ssd_loss_train(const float* cls_logits, const float* bbox_regression, const float* anchors,
                                                                       const float* gt_boxes, const int64_t* gt_labels, const int32_t* gt_counts,
                                                                       int n, int num_anchors, int num_classes, int gmax, float iou_thresh,
                                                                       float neg_to_pos_ratio, int64_t* matched_idxs, float* losses, void* workspace,
                                                                       size_t workspace_bytes, void* state, size_t state_bytes, void* stream) {
    DN_REQUIRE(state && n > 0 && num_anchors > 0 && state_bytes >= dn_ssd_loss_state_bytes(n, num_anchors) && (reinterpret_cast<size_t>(state) & 15) == 0,
               "dn_ssd_loss_train: state null, misaligned or too small (%zu B)", state_bytes);
    const LossState st = loss_state(state, n, num_anchors);
    return ssd_loss_launch("dn_ssd_loss_train", cls_logits, bbox_regression, anchors, gt_boxes, gt_labels, gt_counts, n, num_anchors, num_classes,
                           gmax, iou_thresh, neg_to_pos_ratio, matched_idxs, losses, workspace, workspace_bytes, &st, reinterpret_cast<hipStream_t>(stream));
}

extern "C" __attribute__((visibility("default"))) int dn_ssd_loss_backward(const float* cls_logits, const float* bbox_regression, const float* anchors,
                                                                          const float* gt_boxes, const int64_t* gt_labels, const void* state,
                                                                          size_t state_bytes, const float* grad_losses, int n, int num_anchors,
                                                                          int num_classes, int gmax, float* grad_cls_logits,
                                                                          float* grad_bbox_regression, void* stream) {
    DN_REQUIRE(anchors && gt_boxes && gt_labels && state && grad_losses, "dn_ssd_loss_backward: null argument");
    DN_REQUIRE((!grad_cls_logits || cls_logits) && (!grad_bbox_regression || bbox_regression), "dn_ssd_loss_backward: a gradient is asked for an input that is null");
    DN_REQUIRE(n > 0 && num_anchors > 0 && num_classes >= 2 && gmax >= 1 && gmax <= GMAX, "dn_ssd_loss_backward: bad sizes n=%d A=%d K=%d gmax=%d (gmax <= %d)",
               n, num_anchors, num_classes, gmax, GMAX);
    DN_REQUIRE((long long)n * num_anchors < (1LL << 31), "dn_ssd_loss_backward: n * num_anchors of 2^31 rows or more (int row indices)");
    DN_REQUIRE(state_bytes >= dn_ssd_loss_state_bytes(n, num_anchors) && (reinterpret_cast<size_t>(state) & 15) == 0,
               "dn_ssd_loss_backward: state misaligned or too small (%zu B)", state_bytes);
    DN_REQUIRE(((reinterpret_cast<size_t>(anchors) | reinterpret_cast<size_t>(gt_boxes) | reinterpret_cast<size_t>(bbox_regression) |
                 reinterpret_cast<size_t>(grad_cls_logits) | reinterpret_cast<size_t>(grad_bbox_regression)) & 15) == 0,
               "dn_ssd_loss_backward: box arrays and gradient buffers must be 16-byte aligned");
    if (!grad_cls_logits && !grad_bbox_regression) return DN_OK;
    const LossState st = loss_state(const_cast<void*>(state), n, num_anchors);
    const long long rows = (long long)n * num_anchors;
    const int tile = num_classes <= 256 ? 64 : 16;
    const dim3 grid((unsigned)((rows + tile - 1) / tile));
    auto kernel = num_classes <= 64 ? ssd_loss_backward_kernel<16, 64> : num_classes <= 256 ? ssd_loss_backward_kernel<64, 64> : ssd_loss_backward_kernel<64, 16>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), cls_logits, bbox_regression,
                       reinterpret_cast<const float4*>(anchors), reinterpret_cast<const float4*>(gt_boxes), reinterpret_cast<const long long*>(gt_labels),
                       st.matched, st.weight, st.normaliser, grad_losses, rows, num_anchors, num_classes, gmax, grad_cls_logits,
                       reinterpret_cast<float4*>(grad_bbox_regression));
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}
