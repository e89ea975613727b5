// The optimizer step of head fine-tuning on the device: dn_grad_norm and dn_sgd_step work on a TABLE of tensors in device memory
// (include/demonet_hip.h, dn_sgd_tensor), so one launch covers every parameter of a param group whatever their number and sizes.
//
// The table: T records {p, g, buf, numel} and, behind them, int32 first[T + 1]: first[t] = the chunks of the tensors in front of t, a chunk =
// DN_SGD_CHUNK consecutive elements of one tensor (the last chunk of a tensor may be ragged). A workgroup takes chunk c, finds its tensor by a
// binary search of `first` (T is a few dozen: six steps of uniform loads) and works at element (c - first[t]) * DN_SGD_CHUNK of it: no host loop
// over tensors and no launch per tensor. Both streaming launches cap the grid at SGD_MAX_WG workgroups and stride the chunks beyond.
//
//   grad_sq_kernel      per chunk, the sum of g * g in float64 (an fp32 square is exact there): each thread adds its elements in a fixed order, the
//                       workgroup a fixed-shape tree in LDS; partials[c] gets the chunk's sum. No atomics.
//   grad_norm_kernel    one workgroup: the partials through LDS, thread 0 adds them in index order, takes the square root in float64 and writes
//                       one fp32 value. The same bits on every run.
//   sgd_step_kernel     torch.optim.SGD's update, one rounded fp32 operation per step of (this file is compiled with -ffp-contract=off)
//                           d = g * coef                 clipping on: coef = min(1, max_norm / (norm + 1e-6)), per thread from *norm
//                           d = d + wd * p               wd != 0
//                           b = first ? d : mu * b + (1 - dampening) * d          mu != 0
//                           d = nesterov ? d + mu * b : b
//                           p = p - lr * d
//                       16-byte accesses when p, g and buf are 16-byte aligned (a chunk starts at a multiple of DN_SGD_CHUNK elements), single
//                       floats otherwise; the ragged tail of a tensor is guarded per element. g is only read.
//   The gate: every workgroup reads the (at most 8) gate values and status[0] itself; a non-finite gate value or a set status[0] makes the whole
//   launch write nothing to p or buf. Thread 0 of workgroup 0 then sets status[0] = 1; status[1] receives the step counter of every launch that found
//   status[0] clear, so after a trip it holds the step that tripped. Workgroups do not wait for each other: those that read status[0] while it is
//   being set see 0 or 1 and skip either way, because the gate values that set it are the ones they read themselves.
// No inline asm, no atomics, plain vector stores.
#include <math.h>

#include "common.h"

namespace {

constexpr int SGD_NT = 256;                 // threads per workgroup
constexpr int SGD_MAX_WG = 2048;            // 256 CUs x 8 workgroups: the grid cap of a memory-bound launch
constexpr int NORM_TILE = 2048;             // partials per LDS tile of grad_norm_kernel
static_assert(DN_SGD_CHUNK % (4 * SGD_NT) == 0, "a chunk is a whole number of 16-byte sweeps of the workgroup");
static_assert(sizeof(dn_sgd_tensor) == 32, "dn_sgd_tensor is 32 bytes");

__device__ __forceinline__ const int32_t* table_first(const dn_sgd_tensor* tab, int T) { return reinterpret_cast<const int32_t*>(tab + T); }

// the tensor of chunk c: the last t with first[t] <= c (tensors of no chunks share their successor's first and are never chosen)
__device__ __forceinline__ int tensor_of(const int32_t* first, int T, int c) {
    int lo = 0, hi = T;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }
__device__ __forceinline__ bool non_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(SGD_NT) void grad_sq_kernel(const dn_sgd_tensor* __restrict__ tab, int T, int chunks, double* __restrict__ partials) {
    __shared__ double sh[SGD_NT];
    const int32_t* first = table_first(tab, T);
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int t = tensor_of(first, T, c);
        const dn_sgd_tensor rec = tab[t];
        const int64_t off = (int64_t)(c - first[t]) * DN_SGD_CHUNK;
        const int64_t left = rec.numel - off;
        const int n = left < DN_SGD_CHUNK ? (int)left : DN_SGD_CHUNK;      // (<= 0 only for a table whose `first` disagrees with numel: nothing is read)
        const float* g = rec.g + off;
        double acc = 0.0;
        if (aligned16(rec.g)) {
            for (int i = 4 * tid; i < n; i += 4 * SGD_NT) {
                if (i + 4 <= n) {
                    const float4 v = *reinterpret_cast<const float4*>(g + i);
                    acc += (double)v.x * (double)v.x;
                    acc += (double)v.y * (double)v.y;
                    acc += (double)v.z * (double)v.z;
                    acc += (double)v.w * (double)v.w;
                } else {
                    for (int e = i; e < n; ++e) acc += (double)g[e] * (double)g[e];
                }
            }
        } else {
            for (int i = tid; i < n; i += SGD_NT) acc += (double)g[i] * (double)g[i];
        }
        sh[tid] = acc;
        __syncthreads();
        for (int s = SGD_NT / 2; s > 0; s >>= 1) {
            if (tid < s) sh[tid] += sh[tid + s];
            __syncthreads();
        }
        if (tid == 0) partials[c] = sh[0];
        __syncthreads();
    }
}

__global__ __launch_bounds__(SGD_NT) void grad_norm_kernel(const double* __restrict__ partials, int chunks, float* __restrict__ norm_out) {
    __shared__ double sh[NORM_TILE];
    double acc = 0.0;
    for (int base = 0; base < chunks; base += NORM_TILE) {
        const int m = chunks - base < NORM_TILE ? chunks - base : NORM_TILE;
        for (int i = threadIdx.x; i < m; i += SGD_NT) sh[i] = partials[base + i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < m; ++i) acc += sh[i];
        __syncthreads();
    }
    if (threadIdx.x == 0) *norm_out = (float)sqrt(acc);
}

struct SgdConst {
    float lr, mu, omd, wd, coef;
    bool clip, has_wd, has_mu, nesterov, first;
};

__device__ __forceinline__ void sgd_one(float& p, float g, float& b, const SgdConst& k) {
    float d = g;
    if (k.clip) d = d * k.coef;
    if (k.has_wd) d = d + k.wd * p;
    if (k.has_mu) {
        b = k.first ? d : k.mu * b + k.omd * d;
        d = k.nesterov ? d + k.mu * b : b;
    }
    p = p - k.lr * d;
}

__global__ __launch_bounds__(SGD_NT) void sgd_step_kernel(const dn_sgd_tensor* __restrict__ tab, int T, int chunks, dn_sgd_hyper h,
                                                          const float* __restrict__ gate, int gate_count, const float* __restrict__ norm, float max_norm,
                                                          int32_t* __restrict__ status) {
    bool bad = status[0] != 0;
    for (int i = 0; i < gate_count; ++i) bad |= non_finite(gate[i]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (status[0] == 0) status[1] = h.step;
        if (bad) status[0] = 1;
    }
    if (bad) return;

    SgdConst k;
    k.lr = h.lr; k.mu = h.momentum; k.omd = 1.f - h.dampening; k.wd = h.weight_decay;
    k.clip = max_norm > 0.f;
    k.coef = k.clip ? fminf(1.f, max_norm / (*norm + 1e-6f)) : 1.f;
    k.has_wd = h.weight_decay != 0.f; k.has_mu = h.momentum != 0.f; k.nesterov = h.nesterov != 0; k.first = h.first_step != 0;
    const bool read_b = k.has_mu && !k.first;

    const int32_t* first = table_first(tab, T);
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int t = tensor_of(first, T, c);
        const dn_sgd_tensor rec = tab[t];
        const int64_t off = (int64_t)(c - first[t]) * DN_SGD_CHUNK;
        const int64_t left = rec.numel - off;
        const int n = left < DN_SGD_CHUNK ? (int)left : DN_SGD_CHUNK;
        float* p = rec.p + off;
        const float* g = rec.g + off;
        float* buf = k.has_mu ? rec.buf + off : nullptr;
        if (aligned16(rec.p) && aligned16(rec.g) && (!k.has_mu || aligned16(rec.buf))) {
            for (int i = 4 * tid; i < n; i += 4 * SGD_NT) {
                if (i + 4 <= n) {
                    float4 pv = *reinterpret_cast<const float4*>(p + i);
                    const float4 gv = *reinterpret_cast<const float4*>(g + i);
                    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (read_b) bv = *reinterpret_cast<const float4*>(buf + i);
                    sgd_one(pv.x, gv.x, bv.x, k);
                    sgd_one(pv.y, gv.y, bv.y, k);
                    sgd_one(pv.z, gv.z, bv.z, k);
                    sgd_one(pv.w, gv.w, bv.w, k);
                    *reinterpret_cast<float4*>(p + i) = pv;
                    if (k.has_mu) *reinterpret_cast<float4*>(buf + i) = bv;
                } else {
                    for (int e = i; e < n; ++e) {
                        float pe = p[e], be = read_b ? buf[e] : 0.f;
                        sgd_one(pe, g[e], be, k);
                        p[e] = pe;
                        if (k.has_mu) buf[e] = be;
                    }
                }
            }
        } else {
            for (int i = tid; i < n; i += SGD_NT) {
                float pe = p[i], be = read_b ? buf[i] : 0.f;
                sgd_one(pe, g[i], be, k);
                p[i] = pe;
                if (k.has_mu) buf[i] = be;
            }
        }
    }
}

int check_table(const char* who, const void* table, int T, int chunks) {
    DN_REQUIRE(table, "%s: null table", who);
    DN_REQUIRE(T >= 1 && chunks >= 1, "%s: T=%d chunks=%d", who, T, chunks);
    DN_REQUIRE((reinterpret_cast<size_t>(table) & 7) == 0, "%s: the table is not 8-byte aligned", who);
    if (T > 65535) {
        dn_set_error("%s: T=%d above 65535", who, T);
        return DN_E_UNSUPPORTED;
    }
    return DN_OK;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) size_t dn_sgd_workspace_bytes(int T, int chunks) {
    if (T <= 0 || T > 65535 || chunks <= 0) return 0;
    return ((size_t)chunks * sizeof(double) + 15) & ~(size_t)15;
}

extern "C" __attribute__((visibility("default"))) int dn_grad_norm(const dn_sgd_tensor* table_dev, int T, int chunks, void* partials_ws,
                                                                  size_t workspace_bytes, float* norm_out_dev, void* stream) {
    const int rc = check_table("dn_grad_norm", table_dev, T, chunks);
    if (rc != DN_OK) return rc;
    DN_REQUIRE(partials_ws && norm_out_dev, "dn_grad_norm: null argument");
    DN_REQUIRE((reinterpret_cast<size_t>(partials_ws) & 7) == 0 && (reinterpret_cast<size_t>(norm_out_dev) & 3) == 0,
               "dn_grad_norm: workspace not 8-byte aligned or norm_out not 4-byte aligned");
    if (workspace_bytes < dn_sgd_workspace_bytes(T, chunks)) {
        dn_set_error("dn_grad_norm: workspace of %zu B, %zu B needed", workspace_bytes, dn_sgd_workspace_bytes(T, chunks));
        return DN_E_WORKSPACE;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    double* partials = reinterpret_cast<double*>(partials_ws);
    dn_note_kernel("grad_sq_kernel");
    hipLaunchKernelGGL(grad_sq_kernel, dim3(chunks < SGD_MAX_WG ? chunks : SGD_MAX_WG), dim3(SGD_NT), 0, s, table_dev, T, chunks, partials);
    DN_HIP_CHECK(hipGetLastError());
    dn_note_kernel("grad_norm_kernel");
    hipLaunchKernelGGL(grad_norm_kernel, dim3(1), dim3(SGD_NT), 0, s, partials, chunks, norm_out_dev);
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}

extern "C" __attribute__((visibility("default"))) int dn_sgd_step(const dn_sgd_tensor* table_dev, int T, int chunks, dn_sgd_hyper hyper,
                                                                 const float* gate_dev, int gate_count, const float* norm_dev, float max_norm,
                                                                 int32_t* status_dev, void* stream) {
    const int rc = check_table("dn_sgd_step", table_dev, T, chunks);
    if (rc != DN_OK) return rc;
    DN_REQUIRE(status_dev, "dn_sgd_step: null status");
    DN_REQUIRE(gate_count >= 0 && gate_count <= DN_SGD_MAX_GATE && (gate_count == 0 || gate_dev), "dn_sgd_step: gate_count=%d (0 .. %d) or a null gate",
               gate_count, DN_SGD_MAX_GATE);
    DN_REQUIRE(hyper.lr >= 0.f && hyper.momentum >= 0.f && hyper.weight_decay >= 0.f && std::isfinite(hyper.lr) && std::isfinite(hyper.momentum)
                   && std::isfinite(hyper.weight_decay) && std::isfinite(hyper.dampening) && hyper.step >= 0,
               "dn_sgd_step: negative or non-finite hyper-parameter (lr=%g momentum=%g dampening=%g weight_decay=%g step=%d)", (double)hyper.lr,
               (double)hyper.momentum, (double)hyper.dampening, (double)hyper.weight_decay, hyper.step);
    DN_REQUIRE(!hyper.nesterov || (hyper.momentum > 0.f && hyper.dampening == 0.f), "dn_sgd_step: Nesterov momentum requires a momentum and zero dampening");
    DN_REQUIRE(max_norm >= 0.f && std::isfinite(max_norm), "dn_sgd_step: max_norm=%g (0: no clipping)", (double)max_norm);
    DN_REQUIRE(max_norm == 0.f || norm_dev, "dn_sgd_step: clipping to max_norm=%g needs the norm", (double)max_norm);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dn_note_kernel("sgd_step_kernel");
    hipLaunchKernelGGL(sgd_step_kernel, dim3(chunks < SGD_MAX_WG ? chunks : SGD_MAX_WG), dim3(SGD_NT), 0, s, table_dev, T, chunks, hyper, gate_dev,
                       gate_count, norm_dev, max_norm, status_dev);
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}
