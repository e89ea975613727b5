// C-ABI implementation: plan construction, workspace layout, launch sequence, hipGraph caching, profiling hook.
// Host-side only (no kernels here). See include/demonet_hip.h for the contract.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <atomic>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "choice.h"

// ---------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static thread_local char g_kernel[96] = "";
void dn_note_kernel(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_kernel, sizeof(g_kernel), fmt, ap);
    va_end(ap);
}
const char* dn_last_kernel() { return g_kernel; }

void dn_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* dn_last_error(void) { return g_err; }
extern "C" int dn_abi_version(void) { return DN_ABI_VERSION; }

int dn_knob(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}

hipError_t dn_allow_big_lds(const void* kernel, int bytes) {
    static std::mutex mu;
    static std::set<std::pair<int, const void*>> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    if (done.count({dev, kernel})) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.insert({dev, kernel});
    return e;
}

// XCD grouping policy (common.h). Read per call, never latched: DN_XCD=0 switches it off (A/B runs, tests of the plain mapping).
int xcd_images_per_group(int n) { return dn_knob("DN_XCD", 1) != 0 && n >= 8 ? (n + 7) / 8 : 0; }

struct Layout {
    int n = 0;
    std::vector<size_t> toff;       // per tensor byte offset in workspace (SIZE_MAX: not materialised)
    std::vector<size_t> tbytes;
    size_t resized_off = 0, logits_off = 0, reg_off = 0, scale_off = 0, post_off = 0, post_bytes = 0, total = 0;
    // liveness reuse: every sub-batch chain owns one arena of `arena` bytes (chains run concurrently at different points of the
    // op list, so blocks that different tensors share must not be shared between chains); toff / tbytes then describe chain 0
    // (chain_n images), chain k adds k * arena. arena == 0: one contiguous [n]-image block per tensor.
    size_t arena = 0;
    int chain_n = 0;
    size_t secnt_off = 0;       // [n_se_in_dw][n] unsigned: last-workgroup counters of the squeeze-excitation tails
};

// images of sub-batch chain k of S in a forward of n (batch_split)
static int sub_count(int n, int S, int k) { const int base = n / S, rem = n % S; return base + (k < rem ? 1 : 0); }

// What one forward was asked to do: forward_impl fills it once, everything below takes it whole.
struct Call {
    const void* images; bool u8;    // [n][3][h][w] fp32 planar, or with u8 [n][h][w][3] uint8 (dn_forward_u8)
    int n, h, w;
    float* boxes; float* scores; int64_t* labels; int32_t* counts;      // null with heads_only
    float* packed;                  // optional extra output of the merge kernel: the plan's dn_set_packed_output setting when the call began
    unsigned char* ws; bool heads_only;
    bool features_only = false;     // dn_forward_features: stop in front of the head launches (implies heads_only)
    const dn_frame* frames = nullptr;   // dn_forward_frames: [n] records in DEVICE memory (images is null, h = w = 0: every record has its own size)
    int format = 0, color = 0;          //   DN_FRAME_*, DN_COLOR_*
    const dn_region* regions = nullptr; // dn_forward_regions: [n] records in DEVICE memory, image i = a rectangle of frames[regions[i].frame]
    // the call of sub-batch chain k of S (D = detections_per_img): the one place that knows the per-image strides of its arrays
    Call chain(int S, int k, size_t D) const {
        size_t n0 = 0;
        for (int q = 0; q < k; ++q) n0 += sub_count(n, S, q);
        Call c = *this;
        c.n = sub_count(n, S, k);
        if (regions) c.regions = regions + n0;      // (the regions name their frames by index: every chain reads the same frame table)
        else if (frames) c.frames = frames + n0;
        else c.images = static_cast<const char*>(images) + n0 * 3 * (size_t)h * w * (u8 ? 1 : sizeof(float));
        if (!heads_only) { c.boxes += n0 * D * 4; c.scores += n0 * D; c.labels += n0 * D; c.counts += n0; }     // (all four are set: forward_impl)
        if (packed) c.packed += n0 * (D + 1) * 6;
        return c;
    }
};

struct GraphKey {
    Call c;
    int chain;          // sub-batch chain index (one single-chain graph per sub-batch), -1: the whole forward in one graph
    auto fields() const {
        return std::make_tuple(c.images, c.n, c.h, c.w, c.ws, c.boxes, c.scores, c.labels, c.counts, (c.heads_only ? 1 : 0) | (c.u8 ? 2 : 0) | (c.features_only ? 4 : 0), c.packed, chain,
                               static_cast<const void*>(c.frames), c.format, c.color, static_cast<const void*>(c.regions));
    }
    bool operator<(const GraphKey& o) const { return fields() < o.fields(); }
};

// One kernel launch of the forward over ops [first, first + len). dn_create builds the list once; the workspace layout takes its
// time steps from it and enqueue walks it.
struct Launch {
    enum Kind {
        SINGLE,         // one op (an SE whose FCs run inside another launch has no kernel of its own: se_host)
        EXPDW,          // [expand 1x1 ->] depthwise [-> project 1x1 (+ residual)]: the expanded tensor never leaves LDS (expdw.hip)
        PW_DW,          // depthwise 3x3 computed into the B fragments of its projection (pwdirect.hip pw_dw_direct_kernel)
        CONV_POOL,      // dense 3x3 conv -> MaxPool2d(2, 2) (convbig.hip)
        TAIL,           // a linear run of tiny layers, one workgroup per image (tail.hip)
        HEADS,          // every head op: the fused head launch and / or the grouped launches (run_heads)
    } kind = SINGLE;
    int first = 0, len = 1;
    bool has_expand = false, has_project = false;   // EXPDW
    int se = -1;            // SINGLE PW / DW: the SE op whose FCs run in its prologue (pointwise.hip SEF) / tail (depthwise.hip dw_se_tail)
    int se_slot = -1;       // SINGLE DW with se: its slot of the counter block
    int se_host = -1;       // SINGLE SE: the op whose launch computes it
    bool stem_split = false;    // SINGLE STEM: may run on the split-fp16 matrix kernel (dn_create checks the host copy of the weights)
    int stem_scale_log2 = 0;    //   its power-of-two weight scale
    std::vector<char> materialise;                  // TAIL, per op: its output is read outside the run -> also to HBM
    std::vector<int> head_dw, head_cls, head_reg;   // HEADS: the depthwise ops, class-head and box-head convs
};

struct dn_plan {
    dn_model_desc d;
    std::vector<dn_tensor_desc> tensors;
    std::vector<dn_op_desc> ops;
    std::vector<int> level_off;         // anchor offset per level
    std::vector<int> pool_blocks;       // per DN_T_POOL tensor: partial-sum rows per image (= dw workgroups per image)
    unsigned char* weights_dev = nullptr;
    size_t zeros_off = 0;
    size_t weight_bytes = 0;
    float* anchors_dev = nullptr;
    std::map<int, Layout> layouts;
    // workspaces whose last forward was dn_forward (not dn_forward_heads): their head arrays may be incomplete -- from DN_HEAD_SOFTMAX_MINN images
    // per chain up the fused head launch writes scores / boxes instead of the large levels' logits -- so dn_head_outputs refuses them
    std::map<const void*, bool> heads_partial;
    bool graph_mode = true;
    std::map<GraphKey, hipGraphExec_t> graphs;
    hipStream_t capture_stream = nullptr;   // capture never happens on the caller's stream (may be the null stream)
    int split = 2;                          // sub-batch branches per forward (see batch_split)
    bool ws_reuse = true;                   // DN_WS_REUSE=0: one private block per tensor (every intermediate stays readable after the forward)
    int chain_graphs = -1;                  // DN_CHAIN_GRAPHS: 1 = one single-chain graph per sub-batch on its own stream, 0 = branches of ONE graph, -1 = by batch size
    bool xcd = true;                        // XCD grouping of every kernel's workgroups by image (common.h; DN_XCD, read in dn_create)
    hipStream_t branch_stream[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_branch[3] = {nullptr, nullptr, nullptr};
    std::map<std::pair<int, int>, Layout> sub_layouts;
    int chains_override = 0;                // dn_set_chains: > 0 = that many sub-batch chains per forward whatever the batch size
    int nms_method = DN_NMS_HARD;           // dn_set_nms: the per-class reduce of the next forwards' post-process
    float nms_sigma = 0.5f;
    float* packed_out = nullptr;            // dn_set_packed_output: what the next forwards copy into Call::packed
    std::vector<Launch> launches;           // the forward's kernel launches in order (dn_create), covering every op once
    int n_se_in_dw = 0;                     // depthwise launches computing an SE in their tail; slot q of the counter block belongs to the q-th
    int post_ticket_slot = -1;              // slot of the counter block lent to launch_postprocess (PostArgs::tickets); needs the stem launch that zeroes the block
    // profiling
    bool profiling = false;
    std::vector<hipEvent_t> events;
    std::vector<double> prof_ms;
    std::vector<std::string> prof_kernel;   // label of the launch each op took part in
    std::vector<int> prof_owner;            // op index whose event segment holds that launch's time
    int prof_runs = 0;
    // the graph cache and the stored packed_out setting are per-plan mutable state: a plan serves ONE host thread at a time
    // (several forwards in flight are several STREAMS fed by one thread, pipeline.py). A second thread entering gets DN_E_INVALID.
    std::atomic<int> in_call{0};
};

// Graph executables may still be replaying on other streams (the slots of a ForwardPipeline) when the cache is cleared: drain the
// device first. Clearing is rare (cache bound reached, dn_set_chains, dn_destroy), so the host wait does not matter.
static void drop_graphs(dn_plan* p) {
    if (p->graphs.empty()) return;
    (void)hipDeviceSynchronize();
    for (auto& kv : p->graphs) (void)hipGraphExecDestroy(kv.second);
    p->graphs.clear();
}

// The launch chain is latency-bound (~70 dependent launches, most of them far from filling 256 CUs), so a forward of n images
// is issued as `split` independent sub-batch chains that the hipGraph runs as parallel branches (measured +6 % at n = 64 with
// two branches; more branches lose again, and below 32 images there is nothing to gain). Every workspace tensor is
// image-major, so a sub-batch simply addresses rows [n0, n0 + ns) of the same layout.
static int batch_split(const dn_plan* p, int n) {
    if (p->chains_override > 0) return std::min(p->chains_override, n);
    if (p->split <= 1 || n < 32) return 1;
    return p->split;
}

static int level_of(const dn_plan* p, int t) {
    for (int l = 0; l < p->d.n_levels; ++l) if (p->d.level_tensor[l] == t) return l;
    return -1;
}
static int reads(const dn_op_desc& o, int t) { return (o.in == t) + (o.residual == t) + (o.se == t); }
// readers of tensor t; a pyramid feature counts 100 more (it must be materialised)
static int uses(const dn_plan* p, int t) {
    int u = 0;
    for (const dn_op_desc& o : p->ops) u += reads(o, t);
    for (int l = 0; l < p->d.n_levels; ++l) u += p->d.level_tensor[l] == t ? 100 : 0;
    return u;
}
// t is a pyramid feature or read by an op outside [first, end): a launch of those ops must write it to the workspace
static bool read_outside(const dn_plan* p, int t, int first, int end) {
    if (level_of(p, t) >= 0) return true;
    for (int u = 0; u < (int)p->ops.size(); ++u)
        if ((u < first || u >= end) && reads(p->ops[u], t)) return true;
    return false;
}

static const Layout& get_layout(dn_plan* p, int n) {
    auto it = p->layouts.find(n);
    if (it != p->layouts.end()) return it->second;
    Layout L;
    L.n = n;
    size_t off = 0;
    const size_t T = p->tensors.size();
    L.toff.assign(T, (size_t)-1);
    L.tbytes.assign(T, 0);
    const int S_chains = batch_split(p, n);
    const int nn = p->ws_reuse ? sub_count(n, S_chains, 0) : n;      // images per block: one chain's share with reuse, else all
    L.chain_n = nn;
    for (size_t i = 0; i < T; ++i) {
        const dn_tensor_desc& t = p->tensors[i];
        size_t b = 0;
        if (t.kind == DN_T_ACT) b = (size_t)nn * t.h * t.w * t.c * 2;
        else if (t.kind == DN_T_VEC) b = (size_t)nn * t.c * 4;
        else if (t.kind == DN_T_POOL) b = (size_t)nn * p->pool_blocks[i] * t.c * 4;
        else continue;      // image: caller's buffer (or the resized copy below)
        L.tbytes[i] = b;
    }
    if (!p->ws_reuse) {
        for (size_t i = 0; i < T; ++i)
            if (L.tbytes[i]) { L.toff[i] = off; off += a256(L.tbytes[i]); }
    } else {
        // Liveness reuse: a tensor occupies its block from the launch that writes it to the last launch that reads it (launch
        // time = op index, with the ops of one fused / grouped launch sharing a time step); blocks are placed first-fit at the
        // lowest offset that is free over the whole interval. Tensors that only exist inside a fused launch get no block. The
        // pyramid features live until the head launches. Every block still holds all n images, so the sub-batch chains keep
        // addressing disjoint rows of the same blocks. 2.6 GB -> ~0.4 GB at batch 64: producer -> consumer pairs of the large maps
        // now rewrite lines that are already resident in the Infinity Cache instead of streaming through fresh memory.
        const int NO = (int)p->ops.size();
        std::vector<int> when(NO);                 // launch time step of every op: the index of its launch
        std::vector<char> inner(T, 0);             // tensor produced AND consumed inside one fused launch (never materialised)
        for (size_t t = 0; t < p->launches.size(); ++t) {
            const Launch& l = p->launches[t];
            const int end = l.first + l.len;
            // head launches: the depthwise group, then the 1x1 / dense group(s)
            for (int q = l.first; q < end; ++q) when[q] = (int)t + (l.kind == Launch::HEADS && p->ops[q].type != DN_OP_DW ? 1 : 0);
            if (l.kind != Launch::HEADS)
                for (int q = l.first; q + 1 < end; ++q)
                    if (!read_outside(p, p->ops[q].out, l.first, end)) inner[p->ops[q].out] = 1;
        }
        std::vector<int> born(T, -1), dies(T, -1);
        for (int i = 0; i < NO; ++i) {
            const dn_op_desc& o = p->ops[i];
            auto use = [&](int tid) { if (tid >= 0) dies[tid] = std::max(dies[tid], when[i]); };
            use(o.in); use(o.residual); use(o.se);
            if (born[o.out] < 0) born[o.out] = when[i];
            dies[o.out] = std::max(dies[o.out], when[i]);
            if (o.pool >= 0) { if (born[o.pool] < 0) born[o.pool] = when[i]; dies[o.pool] = std::max(dies[o.pool], when[i]); }
        }
        for (const Launch& l : p->launches) {
            if (l.se < 0) continue;
            const dn_op_desc& so = p->ops[l.se];
            const int t = when[l.first];
            if (p->ops[l.first].type == DN_OP_PW) dies[so.in] = std::max(dies[so.in], t);      // folded SE: the projection reads the pooled partial sums
            else if (born[so.out] >= 0) born[so.out] = std::min(born[so.out], t);                // dw_se_tail: the depthwise launch writes the scale vector
        }
        const int t_end = NO + 2;
        for (int l = 0; l < p->d.n_levels; ++l) dies[p->d.level_tensor[l]] = t_end;      // read back by tests / callers after the forward
        struct Blk { size_t off, bytes; int born, dies; };
        std::vector<Blk> placed;
        std::vector<size_t> order;
        for (size_t i = 0; i < T; ++i)
            if (L.tbytes[i] && !inner[i] && born[i] >= 0) order.push_back(i);
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return born[a] < born[b]; });
        for (size_t i : order) {
            const size_t need = a256(L.tbytes[i]);
            std::vector<std::pair<size_t, size_t>> busy;       // blocks alive at some point of [born, dies]
            for (const Blk& b : placed)
                if (!(b.dies < born[i] || b.born > dies[i])) busy.push_back({b.off, b.off + b.bytes});
            std::sort(busy.begin(), busy.end());
            size_t at = 0;
            for (const auto& iv : busy) {
                if (iv.first >= at + need) break;
                at = std::max(at, iv.second);
            }
            L.toff[i] = at;
            placed.push_back({at, need, born[i], dies[i]});
            off = std::max(off, at + need);
        }
        L.arena = a256(off);
        off = L.arena * (size_t)S_chains;
    }
    L.resized_off = off;
    off += a256((size_t)n * 3 * p->d.image_h * p->d.image_w * 4);
    L.logits_off = off;
    off += a256((size_t)n * p->d.num_anchors * p->d.num_classes * 4);
    L.reg_off = off;
    off += a256((size_t)n * p->d.num_anchors * 4 * 4);
    L.scale_off = off;
    off += a256((size_t)n * 2 * 4);
    L.secnt_off = off;
    off += a256((size_t)n * p->n_se_in_dw * 4 + 4);
    L.post_off = off;
    {
        const int S = batch_split(p, n);          // one private post-process scratch slice per sub-batch branch
        L.post_bytes = (size_t)S * a256(postprocess_ws_bytes(sub_count(n, S, 0), p->d.num_anchors, p->d.num_classes,
                                                                 p->d.topk_candidates, p->d.detections_per_img));
    }
    off += a256(L.post_bytes);
    L.total = off;
    return p->layouts.emplace(n, std::move(L)).first->second;
}

// ---------------------------------------------------------------------------------------------------------
// the launch list: dn_create's grouping passes work on one Launch per op. at[i].len > 0: a launch starts at op i; len == 0: op i
// belongs to an earlier op's launch.
using OpLaunches = std::vector<Launch>;

static bool plain(const OpLaunches& at, int i) { return at[i].kind == Launch::SINGLE && at[i].len == 1; }

static Launch& group(OpLaunches& at, int first, Launch::Kind kind, int len) {
    at[first] = Launch();
    at[first].kind = kind; at[first].first = first; at[first].len = len;
    for (int q = 1; q < len; ++q) at[first + q].len = 0;
    return at[first];
}

static bool plain_pw(const dn_op_desc& o) { return o.type == DN_OP_PW && !o.head && o.se < 0; }
static bool plain_dw(const dn_op_desc& o) { return o.type == DN_OP_DW && !o.head && o.dil == 1; }

// expand (1x1) -> depthwise [-> project] at op i whose expanded tensor has no other reader: the ops of one EXPDW launch, 0: none.
// The project stage (whole inverted-residual block in one launch) goes down to the 20 x 20 maps: one workgroup owns all expanded
// channels of its pixel tile (chunk loop), the expand's A fragments fit the register variants up to cin = 88, and the (pixel tile x
// channel tile) units of the projection must fit the 8 waves (5 x 10 pixel tiles there). Measured: the 160^2 / 80^2 blocks
// -20 % each (round 1); the four blocks without squeeze-excitation on the 20 x 20 maps (40->240->80 stride 2, 80->200->80,
// 2 x 80->184->80: three launches of 5 - 11 us each become one of 11 - 17 us) batch 64 1.10 -> 1.055 ms, batch 32 0.765 -> 0.74
static int expdw_len(const dn_plan* p, int i) {
    const int max_hw = dn_knob("DN_EXPDW_MAXHW", 1 << 30);
    // measured per layer (bench.py --per-op, tools/probe_expdw.py): the fused kernel currently wins on the large maps only
    const int min_hw = dn_knob("DN_EXPDW_MINHW", 6400);
    const int proj_min_hw = dn_knob("DN_EXPDW_PROJ_MINHW", 300);      // (19 x 19 maps of the 300-pixel models included)
    const dn_op_desc& a = p->ops[i];
    const dn_op_desc& d = p->ops[i + 1];
    if (!(plain_pw(a) && a.residual < 0 && uses(p, a.out) == 1 && plain_dw(d) && d.in == a.out && p->tensors[a.in].kind == DN_T_ACT &&
          expdw_supported(a.cin, a.cout, d.k, d.stride)))
        return 0;
    const dn_tensor_desc& to = p->tensors[d.out];
    if (to.h * to.w > max_hw) return 0;
    bool can_proj = i + 2 < (int)p->ops.size() && a.cin <= 96;
    if (can_proj) {
        const dn_op_desc& pj = p->ops[i + 2];
        can_proj = plain_pw(pj) && pj.in == d.out && uses(p, d.out) == 1 && d.pool < 0 && pj.act == DN_ACT_NONE && d.cin <= 640 &&
                   to.h * to.w >= proj_min_hw && expdw_project_supported(d.cin, pj.cout, to.h, to.w, d.stride) &&
                   (pj.residual < 0 || (pj.residual == a.in && d.stride == 1 && pj.cout == p->tensors[a.in].c));
    }
    if (to.h * to.w < min_hw && !can_proj) return 0;      // below the expand+depthwise threshold only whole blocks fuse
    return can_proj ? 3 : 2;
}

// depthwise 3x3 -> project without an expand at op i (first block of the MobileNets, 16 / 32 channels on the largest map): the
// depthwise is computed straight into the projection's B fragments (measured: V3's 16-channel block batch 64 0.782 -> 0.765 ms in
// flight, 1.035 -> 1.02 one at a time; the 32-channel block of the V2 model at 300 x 300 level with the two launches -- two K steps
// of nine taps per lane for a projection that fills half a tile: DN_PW_DW=2 only). (The same pair through the LDS-tiled block
// kernel was correct but slower than the two launches -- 16 channels leave half of the workgroup idle in the depthwise stage -- and
// is not dispatched.)
static bool pw_dw_at(const dn_plan* p, int i, int mode) {
    const dn_op_desc& a = p->ops[i];
    const dn_op_desc& d = p->ops[i + 1];
    const dn_tensor_desc& ti = p->tensors[a.in];
    return mode && plain_dw(a) && a.k == 3 && a.stride == 1 && a.pad == 1 && a.pool < 0 && (a.cin == 16 || (a.cin == 32 && mode == 2)) &&
           ti.kind == DN_T_ACT && plain_pw(d) && d.in == a.out && uses(p, a.out) == 1 && d.cout <= 32 && d.cout % 8 == 0 &&
           (d.residual < 0 || (d.residual == a.in && d.cout == a.cin)) && ti.h * ti.w >= 32 &&
           fd_ok((unsigned long long)ti.h * ti.w, (unsigned)ti.w);      // (the kernel's x = pixel % w)
}

// ---- inverted-residual blocks: EXPDW and PW_DW launches, claimed left to right (the first that matches at an op wins).
//      DN_EXPDW=0 turns both off.
static void group_inverted_residuals(dn_plan* p, OpLaunches& at) {
    if (!dn_knob("DN_EXPDW", 1)) return;
    const int pw_dw = dn_knob("DN_PW_DW", 1);
    for (int i = 0; i + 1 < (int)p->ops.size(); ++i) {
        if (const int len = expdw_len(p, i)) {
            Launch& l = group(at, i, Launch::EXPDW, len);
            l.has_expand = true;
            l.has_project = len == 3;
            i += len - 1;
        } else if (pw_dw_at(p, i, pw_dw)) {
            group(at, i, Launch::PW_DW, 2);
            ++i;
        }
    }
}

// ---- dense 3x3 conv -> MaxPool2d(2, 2) pairs (VGG conv1_2 / conv2_2): one launch (convbig.hip conv_patch_kernel)
static void group_conv_pool(dn_plan* p, OpLaunches& at) {
    for (int i = 0; i + 1 < (int)p->ops.size(); ++i) {
        const dn_op_desc& c = p->ops[i];
        const dn_op_desc& m = p->ops[i + 1];
        const dn_tensor_desc& tc = p->tensors[c.out];
        if (c.type == DN_OP_CONV && !c.head && c.k == 3 && c.stride == 1 && c.pad == 1 && c.dil == 1 && m.type == DN_OP_MAXPOOL && m.in == c.out &&
            m.k == 2 && m.stride == 2 && m.pad == 0 && plain(at, i) && p->tensors[c.in].h == tc.h &&
            ((uses(p, c.out) == 1 && conv_pool_ok(c.cin, c.cout, tc.h, tc.w)) ||
             (!conv_patch_pool_ok(c.cin, c.cout, tc.h, tc.w) && conv_halo_pool_ok(c.cin, c.cout, tc.h, tc.w)))) {      // (the run-staged tile can write both maps)
            group(at, i, Launch::CONV_POOL, 2);
            ++i;
        }
    }
}

// ---- stems: the split-fp16 matrix kernel (depthwise.hip stem_split_kernel) takes weights and bias scaled by a power of two such that the
//      largest magnitude lands in [2^13, 2^15) (the low halves of the split then stay normal fp16 numbers), and a normalised image that fp16 holds
//      (pixels in [0, 1]: |x| <= max(mean, 1 - mean) / std)
static void check_stems(const dn_plan* p, const void* weights, OpLaunches& at) {
    for (int i = 0; i < (int)p->ops.size(); ++i) {
        const dn_op_desc& so = p->ops[i];
        if (so.type != DN_OP_STEM) continue;
        const float* hw = reinterpret_cast<const float*>(static_cast<const unsigned char*>(weights) + so.w_off);
        const float* hb = reinterpret_cast<const float*>(static_cast<const unsigned char*>(weights) + so.b_off);
        bool ok = true;
        float big = 0.f;
        for (int q = 0; q < so.k * so.k * 3 * so.cout; ++q) { ok = ok && std::isfinite(hw[q]); big = std::max(big, std::fabs(hw[q])); }
        for (int q = 0; q < so.cout; ++q) { ok = ok && std::isfinite(hb[q]); big = std::max(big, std::fabs(hb[q])); }
        for (int c = 0; c < 3; ++c) ok = ok && p->d.std[c] > 0.f && std::max(std::fabs(p->d.mean[c]), std::fabs(1.f - p->d.mean[c])) / p->d.std[c] < 3.0e4f;
        int e = 0;
        if (ok && big > 0.f) {
            (void)std::frexp(big, &e);           // big = m 2^e, m in [0.5, 1)
            e = 15 - e;                          // big 2^e in [2^14, 2^15)
            e = std::max(-100, std::min(100, e));
        }
        at[i].stem_split = ok;
        at[i].stem_scale_log2 = e;
    }
}

// ---- small squeeze-excitations (c <= 128, squeeze <= 32: the 40 x 40 blocks of MobileNetV3) are computed in the prologue of the
//      projection that consumes them: one dependent launch (~10 us of pure latency) less per block
static void fold_se_into_projections(const dn_plan* p, OpLaunches& at) {
    const bool se_small = dn_knob("DN_SE_SMALL", 1) != 0;
    for (int i = 0; i + 1 < (int)p->ops.size(); ++i) {
        const dn_op_desc& so = p->ops[i];
        const dn_op_desc& pj = p->ops[i + 1];
        if (so.type != DN_OP_SE || pj.type != DN_OP_PW || pj.se != so.out || pj.head) continue;
        const dn_tensor_desc& ti = p->tensors[pj.in];
        const auto users = std::count_if(p->ops.begin(), p->ops.end(), [&](const dn_op_desc& o) { return o.se == so.out; });
        if (users == 1 && pw_se_fold_supported(pj.cin, pj.cout, so.squeeze, ti.h * ti.w)) {
            // DN_SE_SMALL (default 1, see below): these small FCs go to the tail of the pooling depthwise launch instead and the projection runs
            // on the register-direct kernel with the scale applied to its x fragments
            if (se_small && (ti.h * ti.w) % 32 == 0 && se_is_small(pj.cin, so.squeeze) && depthwise_se_tail_supported(so.cin, so.squeeze)) continue;
            at[i].se_host = i + 1;
            at[i + 1].se = i;
        }
    }
}

// ---- the other squeeze-excitations (opt-in, DN_SE_IN_DW=1): their FCs run in the tail of the depthwise launch that pools for
//      them (the last workgroup of an image to finish; depthwise.hip dw_se_tail) instead of a 32-workgroup launch of their own.
//      Needs the plain depthwise launch (not the fused expand+depthwise or tail runs) and the stem launch, which clears
//      the counters. MEASURED and left off. With a device-scope fence per workgroup the 20 x 20 depthwise launches went from
//      10 to 50 us (a release at agent scope writes back the XCD's L2: batch 64 1.12 -> 1.32 ms). With the fence-free publish
//      (device-scope atomic stores / loads of the partial sums, relaxed ticket) the launch overhead is gone, but the FCs of the
//      large blocks stream 230 - 450 KB of weights into ONE compute unit per image on 256 threads: batch 64 1.063 -> 1.068 ms.
//      DN_SE_SMALL=1 does the same for the small squeeze-excitations only (instead of folding them into the projection's
//      prologue), the projection then runs on the register-direct kernel with the scale applied to its x fragments:
//      1.063 -> 1.054 ms at batch 64, no change at 32 / 16 one forward at a time; with three forwards in flight (pipeline.py)
//      0.840 -> 0.825 ms at batch 64 and 0.463 -> 0.458 ms at 32: on by default.
static void se_in_depthwise_tails(dn_plan* p, OpLaunches& at) {
    const bool all = dn_knob("DN_SE_IN_DW", 0) != 0;
    if ((!all && !dn_knob("DN_SE_SMALL", 1)) || p->ops[0].type != DN_OP_STEM) return;
    for (int i = 1; i < (int)p->ops.size(); ++i) {
        const dn_op_desc& so = p->ops[i];
        if (so.type != DN_OP_SE || at[i].se_host >= 0) continue;
        if (!all && !se_is_small(so.cin, so.squeeze)) continue;      // DN_SE_SMALL alone: the small ones only
        int j = -1;
        for (int q = 0; q < i; ++q) if (p->ops[q].type == DN_OP_DW && p->ops[q].pool == so.in) j = q;
        if (j < 1 || !depthwise_se_tail_supported(so.cin, so.squeeze) || !plain(at, j)) continue;
        at[j].se = i;
        at[j].se_slot = p->n_se_in_dw++;
        at[i].se_host = j;
    }
}

// partial-sum rows of every pooled tensor = workgroups per image of its producing depthwise op
static void size_pool_partials(dn_plan* p, const OpLaunches& at) {
    p->pool_blocks.assign(p->tensors.size(), 0);
    for (int i = 0; i < (int)p->ops.size(); ++i) {
        const dn_op_desc& o = p->ops[i];
        if (o.type != DN_OP_DW || o.pool < 0) continue;
        const dn_tensor_desc& ti = p->tensors[o.in];
        const dn_tensor_desc& to = p->tensors[o.out];
        if (i > 0 && at[i - 1].kind == Launch::EXPDW && at[i - 1].has_expand) {
            p->pool_blocks[o.pool] = expdw_tiles_per_image(to.h, to.w, o.stride);
            continue;
        }
        DwArgs a{};
        a.n = 1; a.h = ti.h; a.w_ = ti.w; a.c = o.cin; a.k = o.k; a.stride = o.stride; a.pad = o.pad; a.ho = to.h; a.wo = to.w;
        p->pool_blocks[o.pool] = depthwise_pool_blocks(a);
    }
}

// ---- heads: once the backbone is done, every remaining op is a head op of the pyramid levels (dw -> 1x1 / dense 3x3 per level,
//      both heads) and they run as one HEADS launch group. Returns its first op (ops.size(): none).
static int group_heads(const dn_plan* p, OpLaunches& at) {
    const int N = (int)p->ops.size();
    // head chain: a head conv, or the op producing its (non-pyramid) input
    auto head_chain = [&](int i) {
        const dn_op_desc& o = p->ops[i];
        if (o.head) return true;
        for (const dn_op_desc& u : p->ops) if (u.head && u.in == o.out && level_of(p, o.out) < 0) return true;
        return false;
    };
    int first = -1, last_main = -1;
    for (int i = 0; i < N; ++i) {
        if (!head_chain(i)) last_main = i;
        else if (first < 0) first = i;
    }
    if (!dn_knob("DN_HEAD_GROUPS", 1) || first < 0 || first < last_main) return N;
    Launch h;
    int kinds = 0;
    for (int i = first; i < N; ++i) {
        const dn_op_desc& o = p->ops[i];
        const dn_op_desc& f = p->ops[first];
        if (o.type == DN_OP_DW) {
            if (o.pool >= 0 || o.k != f.k || o.stride != f.stride || f.type != DN_OP_DW || level_of(p, o.in) < 0) return N;
            h.head_dw.push_back(i);
        } else if ((o.type == DN_OP_PW || o.type == DN_OP_CONV) && o.head) {
            kinds |= (o.type == DN_OP_PW) ? 1 : 2;
            (o.head == 1 ? h.head_cls : h.head_reg).push_back(i);
        } else return N;
    }
    if (kinds == 3 || h.head_dw.size() > 12 || h.head_cls.size() > 8 || h.head_reg.size() > 8 || h.head_cls.empty()) return N;
    Launch& l = group(at, first, Launch::HEADS, N - first);
    l.head_dw.swap(h.head_dw); l.head_cls.swap(h.head_cls); l.head_reg.swap(h.head_reg);
    return first;
}

// ---- tail run: the longest suffix of the backbone (ops [.., end) before the heads) that is a linear chain of tiny layers
static void group_tail(const dn_plan* p, OpLaunches& at, int end) {
    if (!dn_knob("DN_TAIL", 1)) return;
    int first = end;
    while (first > 0) {
        const int i = first - 1;
        const dn_op_desc& o = p->ops[i];
        const dn_tensor_desc& ti = p->tensors[o.in];
        const dn_tensor_desc& to = p->tensors[o.out];
        if (!plain(at, i) || ti.kind != DN_T_ACT || !tail_op_supported(o, ti.h, ti.w, to.h, to.w)) break;
        if (first < end && p->ops[first].in != o.out) break;         // must feed the next op of the run
        --first;
    }
    first = std::max(first, end - TAIL_MAX_OPS);
    if (end - first < 2) return;
    Launch& l = group(at, first, Launch::TAIL, end - first);
    for (int i = first; i < end; ++i) l.materialise.push_back(read_outside(p, p->ops[i].out, first, end) ? 1 : 0);
}

static void plan_launches(dn_plan* p, const void* weights) {
    const int N = (int)p->ops.size();
    OpLaunches at(N);
    for (int i = 0; i < N; ++i) at[i].first = i;
    group_inverted_residuals(p, at);
    group_conv_pool(p, at);
    check_stems(p, weights, at);
    fold_se_into_projections(p, at);
    se_in_depthwise_tails(p, at);
    for (int i = 0; i < N; ++i)
        if (p->ops[i].type == DN_OP_STEM) { p->post_ticket_slot = p->n_se_in_dw++; break; }
    size_pool_partials(p, at);
    group_tail(p, at, group_heads(p, at));
    p->launches.clear();
    for (Launch& l : at) if (l.len > 0) p->launches.push_back(std::move(l));
}

extern "C" int dn_create(const dn_model_desc* desc, const void* weights, size_t weight_bytes, dn_plan** out) {
    DN_REQUIRE(desc && weights && out, "dn_create: null argument");
    DN_REQUIRE(desc->abi_version == DN_ABI_VERSION, "dn_create: ABI version %d != library %d", desc->abi_version, DN_ABI_VERSION);
    DN_REQUIRE(desc->n_tensors > 0 && desc->n_ops > 0 && desc->tensors && desc->ops, "dn_create: empty graph");
    DN_REQUIRE(desc->n_levels >= 1 && desc->n_levels <= 8, "dn_create: n_levels=%d outside [1,8]", desc->n_levels);
    DN_REQUIRE(desc->num_classes >= 2, "dn_create: num_classes must include background (>= 2)");
    if (desc->num_classes > DN_MAX_CLASSES) {
        dn_set_error("dn_create: num_classes=%d above the limit of %d (DN_MAX_CLASSES, background included)", desc->num_classes, DN_MAX_CLASSES);
        return DN_E_UNSUPPORTED;
    }
    DN_REQUIRE(desc->anchors && desc->num_anchors > 0, "dn_create: anchors missing");
    DN_REQUIRE(desc->score_thresh >= 0.f, "dn_create: score_thresh must be >= 0");
    dn_plan* p = new dn_plan();
    p->d = *desc;
    p->tensors.assign(desc->tensors, desc->tensors + desc->n_tensors);
    p->ops.assign(desc->ops, desc->ops + desc->n_ops);
    p->d.tensors = p->tensors.data();
    p->d.ops = p->ops.data();
    // validate ops
    auto fail = [&](int rc) { delete p; return rc; };
    for (int i = 0; i < desc->n_ops; ++i) {
        const dn_op_desc& o = p->ops[i];
        auto ok_t = [&](int t) { return t >= 0 && t < desc->n_tensors; };
        if (!ok_t(o.in) || !ok_t(o.out)) { dn_set_error("dn_create: op %d has bad tensor ids", i); return fail(DN_E_INVALID); }
        if (o.w_off >= 0 && (size_t)o.w_off >= weight_bytes) { dn_set_error("dn_create: op %d weight offset out of range", i); return fail(DN_E_INVALID); }
        if (o.type < DN_OP_STEM || o.type > DN_OP_L2NORM) { dn_set_error("dn_create: op %d unknown type %d", i, o.type); return fail(DN_E_INVALID); }
        if (o.head && (o.level < 0 || o.level >= desc->n_levels)) { dn_set_error("dn_create: head op %d bad level", i); return fail(DN_E_INVALID); }
    }
    plan_launches(p, weights);
    p->graph_mode = dn_knob("DN_GRAPH", 1) != 0;      // DN_GRAPH=0: plain launches (diagnostics)
    p->xcd = dn_knob("DN_XCD", 1) != 0;
    p->chain_graphs = dn_knob("DN_CHAIN_GRAPHS", -1);      // -1: auto (forward_impl)
    p->ws_reuse = dn_knob("DN_WS_REUSE", 1) != 0;
    p->split = std::max(1, std::min(4, dn_knob("DN_SPLIT", 2)));
    // anchor offsets per level
    int acc = 0;
    for (int l = 0; l < desc->n_levels; ++l) {
        const dn_tensor_desc& t = p->tensors[desc->level_tensor[l]];
        p->level_off.push_back(acc);
        acc += t.h * t.w * desc->anchors_per_loc[l];
    }
    if (acc != desc->num_anchors) {
        dn_set_error("dn_create: anchors per level sum to %d, desc says %d", acc, desc->num_anchors);
        return fail(DN_E_INVALID);
    }
    // the arena ends with 256 zero bytes: the source of out-of-image taps in convbig.hip
    p->zeros_off = (weight_bytes + 255) & ~(size_t)255;
    hipError_t e = hipMalloc((void**)&p->weights_dev, p->zeros_off + 256);
    if (e == hipSuccess) e = hipMemset(p->weights_dev + p->zeros_off, 0, 256);
    if (e == hipSuccess) e = hipMemcpy(p->weights_dev, weights, weight_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&p->anchors_dev, (size_t)desc->num_anchors * 16);
    if (e == hipSuccess) e = hipMemcpy(p->anchors_dev, desc->anchors, (size_t)desc->num_anchors * 16, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        dn_set_error("dn_create: device allocation/upload failed: %s", hipGetErrorString(e));
        if (p->weights_dev) (void)hipFree(p->weights_dev);
        if (p->anchors_dev) (void)hipFree(p->anchors_dev);
        return fail(DN_E_HIP);
    }
    for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipStreamCreateWithFlags(&p->branch_stream[i], hipStreamNonBlocking);
    for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&p->ev_branch[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming);
    if (e != hipSuccess) {
        dn_set_error("dn_create: stream/event creation failed: %s", hipGetErrorString(e));
        return fail(DN_E_HIP);
    }
    p->weight_bytes = weight_bytes;
    p->d.anchors = nullptr;
    *out = p;
    return DN_OK;
}

extern "C" void dn_destroy(dn_plan* p) {
    if (!p) return;
    (void)hipDeviceSynchronize();       // forwards of this plan may still be in flight on the caller's streams: the weights go away below
    drop_graphs(p);
    if (p->capture_stream) (void)hipStreamDestroy(p->capture_stream);
    for (int i = 0; i < 3; ++i) if (p->branch_stream[i]) (void)hipStreamDestroy(p->branch_stream[i]);
    for (int i = 0; i < 3; ++i) if (p->ev_branch[i]) (void)hipEventDestroy(p->ev_branch[i]);
    if (p->ev_fork) (void)hipEventDestroy(p->ev_fork);
    for (auto ev : p->events) (void)hipEventDestroy(ev);
    if (p->weights_dev) (void)hipFree(p->weights_dev);
    if (p->anchors_dev) (void)hipFree(p->anchors_dev);
    delete p;
}

extern "C" size_t dn_workspace_bytes(const dn_plan* p, int n) {
    if (!p || n <= 0) return 0;
    return get_layout(const_cast<dn_plan*>(p), n).total;
}

// The in-forward split trades launch-bound kernels for two half-size chains that run in lockstep. A caller that keeps several
// FORWARDS in flight (one stream, workspace and output set each; demonet_amd/pipeline.py) overlaps chains that sit in different
// phases instead, and is better served by one whole-batch chain per forward: batch 64, three in flight: 0.84 ms per forward
// against 1.06 ms for one forward at a time as two chains (tools/pipeline_probe.py).
extern "C" int dn_set_chains(dn_plan* p, int chains) {
    DN_REQUIRE(p, "null plan");
    DN_REQUIRE(chains >= 0 && chains <= 4, "dn_set_chains: %d outside [0, 4] (0 = automatic)", chains);
    if (chains == p->chains_override) return DN_OK;
    p->chains_override = chains;
    // layouts, workspace sizes and captured graphs all depend on the split
    drop_graphs(p);
    p->layouts.clear();
    p->sub_layouts.clear();
    return DN_OK;
}

extern "C" int dn_set_nms(dn_plan* p, int method, float sigma) {
    DN_REQUIRE(p, "null plan");
    DN_REQUIRE(method == DN_NMS_HARD || method == DN_NMS_SOFT_LINEAR || method == DN_NMS_SOFT_GAUSSIAN, "dn_set_nms: unknown method %d", method);
    DN_REQUIRE(method != DN_NMS_SOFT_GAUSSIAN || (std::isfinite(sigma) && sigma > 0.f), "dn_set_nms: Gaussian soft-NMS needs a finite sigma > 0");
    DN_REQUIRE(p->in_call.load() == 0, "dn_set_nms: the plan is inside a forward of another host thread");
    if (method == p->nms_method && sigma == p->nms_sigma) return DN_OK;
    p->nms_method = method;
    p->nms_sigma = sigma;
    drop_graphs(p);      // the captured launch sequences hold the other method's kernels
    return DN_OK;
}

// dev hook: forget the captured graphs (tools that install debug hooks after the first forward)
extern "C" __attribute__((visibility("default"))) int dn_debug_clear_graphs(dn_plan* p) {
    DN_REQUIRE(p, "null plan");
    drop_graphs(p);
    return DN_OK;
}

extern "C" int dn_set_graph_mode(dn_plan* p, int enabled) {
    DN_REQUIRE(p, "null plan");
    p->graph_mode = enabled != 0;
    return DN_OK;
}

// view of rows [n0, n0 + ns) of the n-image layout, as a layout of its own (branch k of S)
static const Layout& get_sub_layout(dn_plan* p, int n, int S, int k) {
    auto key = std::make_pair(n, k);
    auto it = p->sub_layouts.find(key);
    if (it != p->sub_layouts.end()) return it->second;
    const Layout& L = get_layout(p, n);
    int n0 = 0;
    for (int q = 0; q < k; ++q) n0 += sub_count(n, S, q);
    const int ns = sub_count(n, S, k);
    Layout V;
    V.n = ns;
    V.toff = L.toff;
    V.tbytes = L.tbytes;
    for (size_t t = 0; t < L.toff.size(); ++t) {
        if (L.toff[t] == (size_t)-1) continue;
        const size_t per = L.tbytes[t] / (size_t)L.chain_n;
        V.toff[t] = L.arena ? L.toff[t] + (size_t)k * L.arena : L.toff[t] + (size_t)n0 * per;
        V.tbytes[t] = (size_t)ns * per;
    }
    V.resized_off = L.resized_off + (size_t)n0 * 3 * p->d.image_h * p->d.image_w * 4;
    V.logits_off = L.logits_off + (size_t)n0 * p->d.num_anchors * p->d.num_classes * 4;
    V.reg_off = L.reg_off + (size_t)n0 * p->d.num_anchors * 16;
    V.scale_off = L.scale_off + (size_t)n0 * 8;
    V.secnt_off = L.secnt_off + (size_t)n0 * p->n_se_in_dw * 4;
    const size_t slice = L.post_bytes / (size_t)S;
    V.post_off = L.post_off + (size_t)k * slice;
    V.post_bytes = slice;
    V.total = L.total;
    return p->sub_layouts.emplace(key, std::move(V)).first->second;
}

// ---------------------------------------------------------------------------------------------------------
// the launch sequence
// ---------------------------------------------------------------------------------------------------------
// what the launches of one chain address: its workspace view, its images and the weights arena
struct Ctx {
    const dn_plan* p;
    const Layout& L;
    unsigned char* ws;
    int n, xq;              // images of this (sub-)batch; images per XCD group, 0: plain mapping
    template <class T> T* t(int tid) const { return reinterpret_cast<T*>(ws + L.toff[tid]); }
    template <class T> const T* w(long off) const { return reinterpret_cast<const T*>(p->weights_dev + off); }
};

// Profiling event segments of one chain: segment i (events[ev0 + i] -> [ev0 + i + 1]) belongs to op i. A launch over ops
// [first, first + len) opens segment `first`, closes one segment after each of its kernel launches and pads up to first + len, so
// that it records exactly len events; prof_kernel / prof_owner map each op to the kernel it took part in and the segment holding it.
struct Segments {
    dn_plan* p;
    hipStream_t s;
    int ev0;
    bool rec;
    int seg = 0, end = 0;
    void record(int q) const { if (rec) (void)hipEventRecord(p->events[ev0 + q], s); }
    void begin(const Launch& l) { seg = l.first; end = l.first + l.len; record(seg); }
    // after a kernel launch: note() each of its ops (it took the last noted kernel), then close() the segment
    void note(int q) const { if (rec) { p->prof_kernel[q] = dn_last_kernel(); p->prof_owner[q] = seg; } }
    void close() { if (++seg < end) record(seg); }
    template <class Ops> void launched(const Ops& ops) { for (int q : ops) note(q); close(); }
    void finish() const { for (int q = seg + 1; q < end; ++q) record(q); }
};

// what the fused head launch leaves to the post-process when it ran softmax + decode in its epilogue (headfuse.hip, SM)
struct HeadEpilogue {
    bool scores_ready = false;
    HistRows rows;
    int small_first = -1;
};

// a head conv writes fp32 into the logits / regression array at its level's anchor offset, every other conv its fp16 tensor
template <class A> static void set_output(const Ctx& c, const dn_op_desc& o, A& a) {
    if (o.head) {
        const int cols = (o.head == 1) ? c.p->d.num_classes : 4;
        a.out = c.ws + (o.head == 1 ? c.L.logits_off : c.L.reg_off);
        a.out_fp32 = 1;
        a.out_img_stride = (long)c.p->d.num_anchors * cols;
        a.out_base = (long)c.p->level_off[o.level] * cols;
    } else {
        a.out = c.t<void>(o.out);
        a.out_fp32 = 0; a.out_img_stride = 0; a.out_base = 0;
    }
}

static PwArgs make_pw(const Ctx& c, const dn_op_desc& o) {
    const dn_tensor_desc& ti = c.p->tensors[o.in];
    PwArgs a;
    a.x = c.t<const half_t>(o.in);
    a.w = c.w<half_t>(o.w_off);
    a.wfrag = (o.type == DN_OP_PW && o.w2_off >= 0) ? c.w<half_t>(o.w2_off) : nullptr;
    a.bias = c.w<float>(o.b_off);
    a.residual = o.residual >= 0 ? c.t<const half_t>(o.residual) : nullptr;
    a.se = o.se >= 0 ? c.t<const float>(o.se) : nullptr;
    a.hw = ti.h * ti.w;
    a.m = c.n * a.hw;
    a.cin = o.cin; a.cout = o.cout; a.act = o.act;
    a.xq = c.xq;
    set_output(c, o, a);
    return a;
}

static DwArgs make_dw(const Ctx& c, const dn_op_desc& o) {
    const dn_tensor_desc& ti = c.p->tensors[o.in];
    const dn_tensor_desc& to = c.p->tensors[o.out];
    DwArgs a;
    a.x = c.t<const half_t>(o.in);
    a.w = c.w<half_t>(o.w_off);
    a.bias = c.w<float>(o.b_off);
    a.out = c.t<half_t>(o.out);
    a.n = c.n; a.h = ti.h; a.w_ = ti.w; a.c = o.cin; a.k = o.k; a.stride = o.stride; a.pad = o.pad; a.act = o.act;
    a.ho = to.h; a.wo = to.w;
    a.pool = o.pool >= 0 ? c.t<float>(o.pool) : nullptr;
    a.xq = c.xq;
    return a;
}

static ConvArgs make_conv(const Ctx& c, const dn_op_desc& o) {
    const dn_tensor_desc& ti = c.p->tensors[o.in];
    const dn_tensor_desc& to = c.p->tensors[o.out];
    ConvArgs a;
    a.x = c.t<const half_t>(o.in);
    a.w = c.w<half_t>(o.w_off);
    a.bias = c.w<float>(o.b_off);
    a.zeros = c.w<half_t>((long)c.p->zeros_off);
    a.n = c.n; a.h = ti.h; a.w_ = ti.w; a.cin = o.cin; a.cout = o.cout; a.k = o.k; a.stride = o.stride;
    a.pad = o.pad; a.dil = o.dil; a.act = o.act; a.ho = to.h; a.wo = to.w;
    a.xq = c.xq;
    set_output(c, o, a);
    return a;
}

static int run_single(const Ctx& c, const Launch& l, const float* net_in, hipStream_t s) {
    const dn_plan* p = c.p;
    const dn_op_desc& o = p->ops[l.first];
    const dn_tensor_desc& ti = p->tensors[o.in];
    const dn_tensor_desc& to = p->tensors[o.out];
    switch (o.type) {
        case DN_OP_STEM: {
            StemArgs a;
            a.img = net_in;
            a.w = c.w<float>(o.w_off);
            a.bias = c.w<float>(o.b_off);
            a.out = c.t<half_t>(o.out);
            a.n = c.n; a.h = ti.h; a.w_ = ti.w; a.cout = o.cout; a.k = o.k; a.stride = o.stride; a.pad = o.pad; a.act = o.act;
            a.ho = to.h; a.wo = to.w;
            for (int q = 0; q < 3; ++q) { a.mean[q] = p->d.mean[q]; a.inv_std[q] = 1.0f / p->d.std[q]; }
            a.xq = c.xq;
            a.split_ok = l.stem_split ? 1 : 0;
            a.w_scale = std::ldexp(1.0f, l.stem_scale_log2);
            a.w_unscale = std::ldexp(1.0f, -l.stem_scale_log2);
            if (p->n_se_in_dw > 0) { a.zero_u32 = reinterpret_cast<unsigned*>(c.ws + c.L.secnt_off); a.zero_count = p->n_se_in_dw * c.n; }
            return launch_stem(a, s);
        }
        case DN_OP_PW: {
            PwArgs a = make_pw(c, o);
            if (l.se >= 0) {
                // the squeeze-excitation FCs run in this projection's prologue: hand over the pooled partial sums and the FC weights
                const dn_op_desc& so = p->ops[l.se];
                a.se = nullptr;
                a.sef_part = c.t<const float>(so.in);
                a.sef_nblk = p->pool_blocks[so.in];
                a.sef_sq = so.squeeze;
                a.sef_inv = 1.0f / (float)so.pool_pixels;
                a.sef_w1t = c.w<half_t>(so.w_off); a.sef_b1 = c.w<float>(so.b_off);
                a.sef_w2t = c.w<half_t>(so.w2_off); a.sef_b2 = c.w<float>(so.b2_off);
            }
            return launch_pointwise(a, s);
        }
        case DN_OP_DW: {
            DwArgs a = make_dw(c, o);
            if (l.se >= 0) {
                const dn_op_desc& so = p->ops[l.se];
                a.se_w1t = c.w<half_t>(so.w_off); a.se_b1 = c.w<float>(so.b_off);
                a.se_w2t = c.w<half_t>(so.w2_off); a.se_b2 = c.w<float>(so.b2_off);
                a.se_scale = c.t<float>(so.out);
                a.se_counter = reinterpret_cast<unsigned*>(c.ws + c.L.secnt_off) + (size_t)l.se_slot * c.n;
                a.se_sq = so.squeeze;
                a.se_inv = 1.0f / (float)so.pool_pixels;
            }
            return launch_depthwise(a, s);
        }
        case DN_OP_SE:
            if (l.se_host >= 0) {
                dn_note_kernel(p->ops[l.se_host].type == DN_OP_PW ? "(se folded into the projection)" : "(se in the tail of the depthwise launch)");
                return DN_OK;
            }
            return launch_se_fc(c.t<const float>(o.in), p->pool_blocks[o.in], c.w<unsigned char>(o.w_off), c.w<float>(o.b_off),
                                c.w<unsigned char>(o.w2_off), c.w<float>(o.b2_off), c.t<float>(o.out), c.n, o.cin, o.squeeze,
                                o.pool_pixels, s, c.xq);
        case DN_OP_CONV:
            return launch_conv(make_conv(c, o), s);
        case DN_OP_MAXPOOL:
            return launch_maxpool(c.t<const half_t>(o.in), c.t<half_t>(o.out), c.n, ti.h, ti.w, ti.c, o.k, o.stride, o.pad, to.h, to.w, s);
        case DN_OP_L2NORM:
            return launch_l2norm(c.t<const half_t>(o.in), c.w<float>(o.w_off), c.t<half_t>(o.out), (long)c.n * ti.h * ti.w, ti.c, s);
    }
    return DN_OK;
}

static int run_expdw(const Ctx& c, const Launch& l, hipStream_t s) {
    const dn_plan* p = c.p;
    const dn_op_desc* e = l.has_expand ? &p->ops[l.first] : nullptr;
    const dn_op_desc& dwo = p->ops[l.first + (l.has_expand ? 1 : 0)];
    const dn_op_desc* pj = l.has_project ? &p->ops[l.first + l.len - 1] : nullptr;
    const dn_tensor_desc& tin = p->tensors[p->ops[l.first].in];
    const dn_tensor_desc& tdo = p->tensors[dwo.out];
    ExpDwArgs a{};
    a.x = c.t<const half_t>(p->ops[l.first].in);
    a.out = c.t<half_t>(pj ? pj->out : dwo.out);
    a.pool = dwo.pool >= 0 ? c.t<float>(dwo.pool) : nullptr;
    if (e) { a.w1 = c.w<half_t>(e->w_off); a.b1 = c.w<float>(e->b_off); a.act1 = e->act; }
    a.wd = c.w<half_t>(dwo.w_off); a.bd = c.w<float>(dwo.b_off); a.act2 = dwo.act;
    if (pj) { a.w3 = c.w<half_t>(pj->w_off); a.b3 = c.w<float>(pj->b_off); }
    a.n = c.n; a.H = tin.h; a.W = tin.w; a.Ho = tdo.h; a.Wo = tdo.w;
    a.cin = tin.c; a.cexp = dwo.cin; a.cout = pj ? pj->cout : dwo.cin;
    a.k = dwo.k; a.stride = dwo.stride; a.pad = dwo.pad;
    a.has_res = (pj && pj->residual >= 0) ? 1 : 0;
    a.xq = c.xq;
    return launch_expdw(a, s);
}

static int run_pw_dw(const Ctx& c, const Launch& l, hipStream_t s) {
    PwArgs pa = make_pw(c, c.p->ops[l.first + 1]);
    const DwArgs da = make_dw(c, c.p->ops[l.first]);
    pa.x = da.x;                                    // (the depthwise output is not materialised)
    if (pa.residual) pa.residual = da.x;
    return launch_pw_dw_direct(pa, da, s);
}

static int run_conv_pool(const Ctx& c, const Launch& l, hipStream_t s) {
    const dn_op_desc& o = c.p->ops[l.first];
    PwArgs pa = conv_to_pw(make_conv(c, o));
    if (c.L.toff[o.out] == (size_t)-1) pa.out = nullptr;      // (materialised only when something else reads the full-resolution map)
    pa.pool_out = c.t<half_t>(c.p->ops[l.first + 1].out);
    return launch_conv_pool(pa, s);
}

static int run_tail(const Ctx& c, const Launch& l, hipStream_t s) {
    const dn_plan* p = c.p;
    TailArgs ta{};
    ta.count = l.len;
    ta.weights = c.w<half_t>(0);
    const dn_op_desc& o0 = p->ops[l.first];
    ta.in0 = c.t<const half_t>(o0.in);
    ta.in0_stride = (long)(c.L.tbytes[o0.in] / (size_t)c.L.n / 2);
    ta.xq = c.xq;
    for (int q = 0; q < ta.count; ++q) {
        const dn_op_desc& oq = p->ops[l.first + q];
        const dn_tensor_desc& tq = p->tensors[oq.in];
        const dn_tensor_desc& uq = p->tensors[oq.out];
        TailOp& t = ta.op[q];
        t.type = oq.type; t.cin = oq.cin; t.cout = oq.type == DN_OP_DW ? oq.cin : oq.cout; t.k = oq.k; t.stride = oq.stride; t.pad = oq.pad;
        t.hin = tq.h; t.win = tq.w; t.hout = uq.h; t.wout = uq.w; t.act = oq.act;
        t.w_off = (long)((oq.type == DN_OP_PW ? oq.w2_off : oq.w_off) / 2); t.b_off = (long)oq.b_off;
        t.out = l.materialise[q] ? c.t<half_t>(oq.out) : nullptr;
        t.out_stride = (long)(c.L.tbytes[oq.out] / (size_t)c.L.n / 2);
    }
    return launch_tail(ta, c.n, s);
}

// SSDLite heads (depthwise 3x3 -> 1x1, class and box head per level): the levels whose class and box head are both (depthwise 3x3
// stride 1 -> 1x1) chains on the level's feature map, as HeadFuseLevels of ONE launch (headfuse.hip) -- no depthwise output in HBM,
// no second launch. members: the four ops (class dw, box dw, class conv, box conv) of every level that joins.
static int fused_head_levels(const Ctx& c, const Launch& l, HeadFuseLevel* fl, std::vector<int>& members) {
    const dn_plan* p = c.p;
    int nl = 0;
    for (size_t q = 0; q < l.head_cls.size() && nl < 8; ++q) {
        const dn_op_desc& oc = p->ops[l.head_cls[q]];
        int qr = -1;
        for (int u : l.head_reg) if (p->ops[u].level == oc.level) qr = u;
        if (qr < 0 || oc.type != DN_OP_PW || p->ops[qr].type != DN_OP_PW) continue;
        const dn_op_desc& orr = p->ops[qr];
        int dc = -1, dr = -1;
        for (int u : l.head_dw) { if (p->ops[u].out == oc.in) dc = u; if (p->ops[u].out == orr.in) dr = u; }
        if (dc < 0 || dr < 0) continue;
        const dn_op_desc &odc = p->ops[dc], &odr = p->ops[dr];
        if (odc.in != odr.in || odc.k != 3 || odr.k != 3 || odc.stride != 1 || odr.stride != 1 || odc.pad != 1 || odr.pad != 1 || odc.dil != 1 ||
            odr.dil != 1 || odc.act != odr.act || odc.cin != odr.cin || oc.cin != odc.cin || orr.cin != odc.cin || oc.act != DN_ACT_NONE ||
            orr.act != DN_ACT_NONE || oc.se >= 0 || orr.se >= 0 || oc.residual >= 0 || orr.residual >= 0 || oc.w2_off < 0 || orr.w2_off < 0 ||
            odc.pool >= 0 || odr.pool >= 0) continue;
        const dn_tensor_desc& ti = p->tensors[odc.in];
        HeadFuseLevel& f = fl[nl];
        f.x = c.t<const half_t>(odc.in);
        const dn_op_desc* op[2] = {&oc, &orr};
        for (int hsel = 0; hsel < 2; ++hsel) {
            const PwArgs pa = make_pw(c, *op[hsel]);
            f.wf[hsel] = pa.wfrag; f.bias[hsel] = pa.bias;
            f.out[hsel] = reinterpret_cast<float*>(pa.out); f.out_img_stride[hsel] = pa.out_img_stride; f.out_base[hsel] = pa.out_base;
            f.nc[hsel] = pa.cout;
        }
        f.wdg = odc.w2_off >= 0 ? c.w<half_t>(odc.w2_off) : nullptr;
        f.wslot = odc.b2_off >= 0 ? c.w<unsigned char>(odc.b2_off) : nullptr;
        f.n = c.n; f.H = ti.h; f.W = ti.w; f.C = odc.cin; f.act = odc.act;
        if (!head_fused_level_supported(f)) continue;
        // DN_HEAD_FUSE_MINHW: levels with fewer pixels per image stay on the grouped launches. The fused workgroups take 512 residency
        // slots (2 per CU); at batch 64 levels 0 - 1 are 504 of them, every further workgroup starts a second round of the whole launch
        if (ti.h * ti.w < dn_knob("DN_HEAD_FUSE_MINHW", 0)) continue;
        if (nl > 0 && (dn_cdiv(f.nc[0], 32) + 4) / 4 != (dn_cdiv(fl[0].nc[0], 32) + 4) / 4) continue;      // (one instantiation per launch: channel tiles per wave)
        ++nl;
        members.push_back(dc); members.push_back(dr); members.push_back(l.head_cls[q]); members.push_back(qr);
    }
    return nl;
}

// softmax + decode + histogram rows in the epilogue of the fused head launch (DN_HEAD_SOFTMAX, default 1) when EVERY level's heads
// are in it and the post-process follows (dn_forward_heads wants the logits themselves). False: the launch writes logits only.
static bool head_softmax_epilogue(const Ctx& c, HeadFuseLevel* fl, int nl, const std::vector<int>& members, HeadPost& hp, HeadEpilogue& ep) {
    const dn_plan* p = c.p;
    const dn_model_desc& d = p->d;
    // From 32 images per chain up (DN_HEAD_SOFTMAX_MINN): below that the launch is far from filling the chip and the epilogue is pure
    // latency on the chain (batch 32 as two chains of 16: 0.630 -> 0.648 ms one forward at a time; from 32 per chain up it gains).
    if (dn_knob("DN_HEAD_SOFTMAX", 1) == 0 || c.n < dn_knob("DN_HEAD_SOFTMAX_MINN", 32)) return false;
    const PostBuffers pb = post_buffers(c.ws + c.L.post_off, c.n, d.num_anchors, d.num_classes, d.topk_candidates);
    int clamped = 0;
    post_hist_range(d.score_thresh, &hp.hb0, &hp.nb, &clamped);
    hp.scoresT = pb.scoresT; hp.boxes = pb.boxes; hp.hrows = pb.phist; hp.anchors = p->anchors_dev;
    hp.A = d.num_anchors; hp.K = d.num_classes;
    hp.img_w = (float)d.image_w; hp.img_h = (float)d.image_h; hp.score_thr = d.score_thresh;
    // the levels with >= 32 pixels per image take the epilogue; they must be a prefix of the anchor axis (the rest -- anchors
    // [small_first, A) -- gets its softmax in the cut-off launch, from the logits this launch writes for them)
    HistRows hr;
    int rows = 0, nsm = 0;
    bool prefix = true;
    for (int q = 0; q < nl; ++q) {
        const int level = p->ops[members[4 * q + 2]].level;
        fl[q].aoff = p->level_off[level];
        fl[q].aloc = fl[q].nc[0] / d.num_classes;
        fl[q].sm = fl[q].H * fl[q].W >= std::max(32, dn_knob("DN_HEAD_SM_MINHW", 32)) ? 1 : 0;
        if (fl[q].sm) {
            prefix = prefix && nsm == q && (q == 0 ? fl[q].aoff == 0 : fl[q].aoff == fl[q - 1].aoff + fl[q - 1].H * fl[q - 1].W * fl[q - 1].aloc);
            fl[q].sbase = rows;
            hr.hw[nsm] = fl[q].H * fl[q].W; hr.sbase[nsm] = rows; hr.grouped[nsm] = head_fused_grouped(c.xq, hr.hw[nsm]) ? 1 : 0;
            rows += hist_rows_slots(hr.hw[nsm]);
            ++nsm;
        }
    }
    hr.levels = nsm;
    hr.rows_per_image = rows;
    // the epilogue levels must be pyramid levels 0 .. nsm - 1: everything behind them -- small levels of this launch and levels that did
    // not join it (the V2 model's last level is a plain 1x1 conv on the grouped launches) -- stays in logit form
    for (int q = 0; q < nsm; ++q) prefix = prefix && p->ops[members[4 * q + 2]].level == q;
    // (the softmax tiles of those levels put their histogram rows behind these: the row stride of an image covers both)
    const int sfirst = nsm < d.n_levels ? p->level_off[nsm] : d.num_anchors;
    hp.rows_per_image = rows + dn_cdiv(d.num_anchors - sfirst, 64);
    if (!(prefix && nsm > 0 && hp.rows_per_image <= pb.tiles && head_fused_post_supported(fl, nl, hp))) return false;
    ep = HeadEpilogue{true, hr, sfirst};
    return true;
}

// the grouped head launches: the depthwise group, then the 1x1 / dense group(s)
static int run_head_groups(const Ctx& c, const std::vector<int>& h_dw, const std::vector<int>& h_cls, const std::vector<int>& h_reg,
                           hipStream_t s, Segments& sg) {
    const dn_plan* p = c.p;
    int rc = DN_OK;
    if (!h_dw.empty()) {
        DwArgs arr[12];
        for (size_t q = 0; q < h_dw.size(); ++q) arr[q] = make_dw(c, p->ops[h_dw[q]]);
        rc = launch_depthwise_group(arr, (int)h_dw.size(), s);
        if (rc != DN_OK) return rc;
        sg.launched(h_dw);
    }
    // box and class heads of all levels in ONE launch when they fit (a dependent launch costs ~4.5 us even when empty, and
    // the narrow box heads then share the class heads' tile instead of running as a launch of their own)
    const bool merge_heads = dn_knob("DN_HEAD_MERGE", 1) != 0;
    // (dense-conv heads leave in a narrow and a wide launch of at most 12 problems each, so 7 levels x 2 heads still go together --
    // the box heads of the large levels must meet their class heads to ride in their tiles: 0.45 ms per 16 images on ssd512)
    const bool conv_heads = !h_reg.empty() && p->ops[h_reg[0]].type == DN_OP_CONV;
    const bool one = merge_heads && !h_reg.empty() && !h_cls.empty() && p->ops[h_reg[0]].type == p->ops[h_cls[0]].type &&
                     (h_reg.size() + h_cls.size() <= 12 || (conv_heads && h_reg.size() <= 12 && h_cls.size() <= 12));
    for (int kind = 0; kind < 2; ++kind) {
        std::vector<int> lst = kind ? h_cls : h_reg;
        if (one) {
            if (kind == 1) break;
            lst.insert(lst.end(), h_cls.begin(), h_cls.end());
        }
        if (lst.empty()) continue;
        std::vector<PwArgs> arr(lst.size());
        const bool conv = p->ops[lst[0]].type == DN_OP_CONV;
        int cnt = 0;
        std::vector<int> grouped;
        std::set<int> taken;
        // wide heads first, so that a box head that rides along is known before the groups are formed
        std::stable_sort(lst.begin(), lst.end(), [&](int x, int y) { return p->ops[x].cout > p->ops[y].cout; });
        for (size_t q = 0; q < lst.size(); ++q) {
            PwArgs pa = conv ? conv_to_pw(make_conv(c, p->ops[lst[q]])) : make_pw(c, p->ops[lst[q]]);
            if (conv && taken.count(lst[q])) continue;          // rides in another head's launch
            if (conv && conv_head_big_supported(pa)) {
                // the wide dense heads of the large levels: MFMA-bound, each on the run-staged 256x256 tile. The box head of the
                // same level (same input, 16 / 24 channels) fits in the idle part of its last channel tile.
                int rider = -1;
                for (size_t u = 0; u < lst.size() && rider < 0; ++u) {
                    const dn_op_desc &ou = p->ops[lst[u]], &oq = p->ops[lst[q]];
                    if (u != q && !taken.count(lst[u]) && ou.in == oq.in && ou.type == oq.type && ou.k == oq.k && ou.stride == oq.stride &&
                        ou.pad == oq.pad && ou.dil == oq.dil && ou.act == oq.act && ou.cout < oq.cout &&
                        dn_cdiv(oq.cout + ou.cout, 256) == dn_cdiv(oq.cout, 256))
                        rider = (int)u;
                }
                if (rider >= 0) {
                    // the tile is chosen from cout + cout_b: the rider joins only if the launch still has a tile WITH it (21 classes x 6 anchors =
                    // 126 + 24 channels cross a 128-channel tile boundary and fail the narrow-tile test the class head passed alone)
                    const PwArgs pb = conv_to_pw(make_conv(c, p->ops[lst[rider]]));
                    PwArgs with = pa;
                    with.w_b = pb.w; with.bias_b = pb.bias; with.out_b = pb.out; with.cout_b = pb.cout;
                    with.out_b_img_stride = pb.out_img_stride; with.out_b_base = pb.out_base;
                    if (conv_head_big_supported(with)) { pa = with; taken.insert(lst[rider]); }
                    else rider = -1;
                }
                rc = launch_conv_head_big(pa, s);
                if (rc != DN_OK) return rc;
                sg.note(lst[q]);
                if (rider >= 0) sg.note(lst[rider]);
                sg.close();
                continue;
            }
            arr[cnt++] = pa;
            grouped.push_back(lst[q]);
        }
        if (cnt == 0) continue;
        // once the wide heads have left, the narrow box heads (16 / 24 channels) would pay the wide tile of the remaining
        // class heads: dense-conv groups are split into a narrow and a wide launch
        const bool split_narrow = conv && (cnt < (int)lst.size() || cnt > 12);
        for (int pass = 0; pass < (split_narrow ? 2 : 1); ++pass) {
            PwArgs sub[12];
            std::vector<int> ids;
            int nsub = 0;
            for (int q = 0; q < cnt; ++q) {
                const bool narrow = arr[q].cout <= 32;
                if (split_narrow && narrow != (pass == 0)) continue;
                DN_REQUIRE(nsub < 12, "head group: more than 12 problems in one launch");
                sub[nsub++] = arr[q];
                ids.push_back(grouped[q]);
            }
            if (nsub == 0) continue;
            rc = launch_pointwise_group(sub, nsub, conv, s);
            if (rc != DN_OK) return rc;
            sg.launched(ids);
        }
    }
    return DN_OK;
}

// the HEADS launch group: the fused head launch (DN_HEAD_FUSE=0 keeps the grouped launches: the reference path of the bit-identity
// test), then the grouped launches for what did not join it (the V2 model's last level is a plain 1x1 conv). Decided per enqueue:
// the choice depends on the chain's batch size and on knobs read at every launch.
static int run_heads(const Ctx& c, const Launch& l, bool heads_only, hipStream_t s, Segments& sg, HeadEpilogue& ep) {
    std::vector<int> h_dw = l.head_dw, h_cls = l.head_cls, h_reg = l.head_reg;
    if (dn_knob("DN_HEAD_FUSE", 1) != 0 && !h_dw.empty() && !h_cls.empty() && !h_reg.empty()) {
        HeadFuseLevel fl[8];
        std::vector<int> members;
        const int nl = fused_head_levels(c, l, fl, members);
        if (nl > 0) {
            HeadPost hp;
            const bool with_post = !heads_only && head_softmax_epilogue(c, fl, nl, members, hp, ep);
            const int rc = launch_head_fused(fl, nl, c.xq, s, with_post ? &hp : nullptr);
            if (rc != DN_OK) return rc;
            sg.launched(members);
            auto joined = [&](int q) { return std::find(members.begin(), members.end(), q) != members.end(); };
            for (std::vector<int>* v : {&h_dw, &h_cls, &h_reg}) v->erase(std::remove_if(v->begin(), v->end(), joined), v->end());
        }
    }
    return run_head_groups(c, h_dw, h_cls, h_reg, s, sg);
}

static int enqueue(dn_plan* p, const Call& call, const Layout& L, hipStream_t s, bool record, int ev0 = 0) {
    const dn_model_desc& d = p->d;
    const int n = call.n, h = call.h, w = call.w;
    unsigned char* const ws = call.ws;
    const float* net_in = static_cast<const float*>(call.images);
    const bool resize = (h != d.image_h || w != d.image_w);
    float* scale_xy = nullptr;
    if (call.regions) {
        // regions of video surfaces: frames_kernel's pass in region coordinates, one record per network image (the ratio block always)
        float* rz = reinterpret_cast<float*>(ws + L.resized_off);
        scale_xy = reinterpret_cast<float*>(ws + L.scale_off);
        int rc = launch_regions_to_planar(call.frames, call.regions, call.format, call.color, rz, scale_xy, n, d.image_h, d.image_w, s);
        if (rc) return rc;
        net_in = rz;
    } else if (call.frames) {
        // video surfaces: colour conversion of the four taps, /255, bilinear resize and the planar layout in one pass; the ratio block is written
        // always (every record has its own size; a ratio of exactly 1 leaves the boxes as they are)
        float* rz = reinterpret_cast<float*>(ws + L.resized_off);
        scale_xy = reinterpret_cast<float*>(ws + L.scale_off);
        int rc = launch_frames_to_planar(call.frames, call.format, call.color, rz, scale_xy, n, d.image_h, d.image_w, s);
        if (rc) return rc;
        net_in = rz;
    } else if (call.u8) {
        // uint8 HWC decoder output: /255, bilinear resize and HWC -> planar in one pass (the stem then normalises on load)
        float* rz = reinterpret_cast<float*>(ws + L.resized_off);
        if (resize) scale_xy = reinterpret_cast<float*>(ws + L.scale_off);
        int rc = launch_u8hwc_to_planar(static_cast<const unsigned char*>(call.images), rz, scale_xy, n, h, w, d.image_h, d.image_w, s);
        if (rc) return rc;
        net_in = rz;
    } else if (resize) {
        // normalisation commutes with bilinear interpolation (affine per channel), so resizing the raw image first and
        // normalising on load in the stem equals transform.py:113-114 (normalize then resize) up to fp32 rounding.
        float* rz = reinterpret_cast<float*>(ws + L.resized_off);
        scale_xy = reinterpret_cast<float*>(ws + L.scale_off);
        int rc = launch_resize_bilinear(net_in, rz, scale_xy, n, h, w, d.image_h, d.image_w, s);
        if (rc) return rc;
        net_in = rz;
    }
    const Ctx c{p, L, ws, n, (p->xcd && n >= 8) ? (n + 7) / 8 : 0};
    Segments sg{p, s, ev0, record};
    HeadEpilogue ep;
    // DN_POISON=1 (correctness tooling): a launch that fills every LDS byte and vector register with NaN patterns in front of every launch of
    // the forward -- results must not change (no kernel may read LDS or registers it has not written)
    const bool poison = !record && dn_knob("DN_POISON", 0) != 0;
    for (const Launch& l : p->launches) {
        if (call.features_only && l.kind == Launch::HEADS) continue;      // the level tensors are complete in front of the head launches
        if (poison) { int prc = launch_poison(s); if (prc != DN_OK) return prc; }
        sg.begin(l);
        int rc = DN_OK;
        switch (l.kind) {
            case Launch::SINGLE: rc = run_single(c, l, net_in, s); break;
            case Launch::EXPDW: rc = run_expdw(c, l, s); break;
            case Launch::PW_DW: rc = run_pw_dw(c, l, s); break;
            case Launch::CONV_POOL: rc = run_conv_pool(c, l, s); break;
            case Launch::TAIL: rc = run_tail(c, l, s); break;
            case Launch::HEADS: rc = run_heads(c, l, call.heads_only, s, sg, ep); break;
        }
        if (rc != DN_OK) return rc;
        if (l.kind != Launch::HEADS) {      // one kernel for all its ops
            for (int q = l.first; q < l.first + l.len; ++q) sg.note(q);
            sg.close();
        }
        sg.finish();
    }
    if (!call.heads_only) {
        PostArgs a;
        a.logits = reinterpret_cast<float*>(ws + L.logits_off); a.reg = reinterpret_cast<float*>(ws + L.reg_off); a.anchors = p->anchors_dev;
        a.n = n; a.A = d.num_anchors; a.K = d.num_classes;
        a.img_h = (float)d.image_h; a.img_w = (float)d.image_w;
        a.scale_xy = scale_xy;      // with a resize: ratio = original / network size in fp32 (transform.py:280-285), written by the resize kernel
        a.score_thresh = d.score_thresh; a.nms_thresh = d.nms_thresh; a.topk = d.topk_candidates; a.dets = d.detections_per_img;
        a.boxes = call.boxes; a.scores = call.scores; a.labels = call.labels; a.counts = call.counts; a.kept_anchor = nullptr;
        a.packed = call.packed;
        a.nms_method = p->nms_method; a.nms_sigma = p->nms_sigma;
        a.ws = ws + L.post_off; a.ws_bytes = L.post_bytes;
        a.xq = c.xq;
        a.scores_ready = ep.scores_ready; a.hrows = ep.rows; a.small_first = ep.small_first;
        if (ep.scores_ready && p->post_ticket_slot >= 0) a.tickets = reinterpret_cast<unsigned*>(ws + L.secnt_off) + (size_t)p->post_ticket_slot * n;
        int rc = launch_postprocess(a, s, record ? &p->events[ev0 + p->ops.size()] : nullptr);
        if (rc) return rc;
    } else {
        sg.record((int)p->ops.size());
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        dn_set_error("kernel launch failed: %s", hipGetErrorString(e));
        return DN_E_HIP;
    }
    return DN_OK;
}

// chain k of S on stream s (no fork / join): what one per-chain graph captures; record: its own block of profiling events
static int enqueue_chain(dn_plan* p, const Call& call, hipStream_t s, int S, int k, bool record = false) {
    const int ev0 = record ? k * ((int)p->ops.size() + 6) : 0;
    return enqueue(p, call.chain(S, k, (size_t)p->d.detections_per_img), get_sub_layout(p, call.n, S, k), s, record, ev0);
}

// the whole forward: one chain, or batch_split() sub-batch chains forked onto branch streams (parallel graph branches when
// captured). record = profiling: the sub-batches run back to back on `s`, each with its own block of events.
static int enqueue_all(dn_plan* p, const Call& call, hipStream_t s, bool record) {
    const int S = batch_split(p, call.n);
    if (S == 1) return enqueue(p, call, get_layout(p, call.n), s, record);
    if (!record) DN_HIP_CHECK(hipEventRecord(p->ev_fork, s));
    for (int k = 0; k < S; ++k) {
        hipStream_t bs = s;
        if (!record && k > 0) {
            bs = p->branch_stream[k - 1];
            DN_HIP_CHECK(hipStreamWaitEvent(bs, p->ev_fork, 0));
        }
        int rc = enqueue_chain(p, call, bs, S, k, record);
        if (rc) return rc;
        if (!record && k > 0) DN_HIP_CHECK(hipEventRecord(p->ev_branch[k - 1], bs));
    }
    if (!record)
        for (int k = 1; k < S; ++k) DN_HIP_CHECK(hipStreamWaitEvent(s, p->ev_branch[k - 1], 0));
    return DN_OK;
}

// one graph executable of `call` on the plan's capture stream: chain `chain` of S alone, or with chain < 0 the whole forward
static int capture(dn_plan* p, const Call& call, int S, int chain, hipGraphExec_t* out) {
    hipGraph_t g = nullptr;
    if (!p->capture_stream) DN_HIP_CHECK(hipStreamCreateWithFlags(&p->capture_stream, hipStreamNonBlocking));
    DN_HIP_CHECK(hipStreamBeginCapture(p->capture_stream, hipStreamCaptureModeThreadLocal));
    const int rc = chain < 0 ? enqueue_all(p, call, p->capture_stream, false) : enqueue_chain(p, call, p->capture_stream, S, chain);
    hipError_t e = hipStreamEndCapture(p->capture_stream, &g);
    if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (e != hipSuccess) { dn_set_error("hipStreamEndCapture: %s", hipGetErrorString(e)); return DN_E_HIP; }
    e = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) { dn_set_error("hipGraphInstantiate: %s", hipGetErrorString(e)); return DN_E_HIP; }
    return DN_OK;
}

static int forward_impl(dn_plan* p, const void* images, int n, int h, int w, float* boxes, float* scores, int64_t* labels,
                        int32_t* counts, void* workspace, size_t ws_bytes, void* stream, bool heads_only, bool u8 = false, bool features_only = false,
                        const dn_frame* frames = nullptr, int format = 0, int color = 0, const dn_region* regions = nullptr) {
    DN_REQUIRE(p && (images || frames) && workspace, "dn_forward: null argument");
    DN_REQUIRE(n > 0 && (frames || (h > 0 && w > 0)), "dn_forward: bad shape n=%d h=%d w=%d", n, h, w);
    struct Busy {
        std::atomic<int>& f; bool ok;
        explicit Busy(std::atomic<int>& x) : f(x), ok(x.exchange(1) == 0) {}
        ~Busy() { if (ok) f.store(0); }
    } busy(p->in_call);
    DN_REQUIRE(busy.ok, "dn_forward: the plan is in use by another host thread (one plan serves one thread at a time; use one plan per thread)");
    DN_REQUIRE(heads_only || (boxes && scores && labels && counts), "dn_forward: null output buffer");
    {   // the launchers count the rows of a chain's tensors (images x pixels) in an int, the XCD grouping rounds the chain up to 8 groups of images
        const int S0 = batch_split(p, n);
        const long per_chain = (n + S0 - 1) / S0;
        for (const dn_tensor_desc& t : p->tensors)
            DN_REQUIRE((t.kind != DN_T_ACT && t.kind != DN_T_IMAGE) || dn_rows_fit(per_chain, (long)t.h * t.w),
                       "dn_forward: %ld images per chain of %d x %d pixels are 2^31 rows or more", per_chain, t.h, t.w);
    }
    const Layout& L = get_layout(p, n);
    if (ws_bytes < L.total) {
        dn_set_error("dn_forward: workspace %zu B < required %zu B for n=%d", ws_bytes, L.total, n);
        return DN_E_WORKSPACE;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // (inside the guard: dn_set_packed_output refuses to change the stored setting while a call is in progress)
    DN_REQUIRE(!features_only || !p->profiling, "dn_forward_features: not available between dn_profile_begin and dn_profile_end");
    const Call call{images, u8, n, h, w, boxes, scores, labels, counts, p->packed_out, reinterpret_cast<unsigned char*>(workspace), heads_only, features_only, frames, format, color, regions};
    p->heads_partial[workspace] = !heads_only || features_only;      // true: the head arrays of this workspace are not (all) written
    const int S = batch_split(p, n);
    if (p->profiling) {
        const size_t stride = p->ops.size() + 6;
        const size_t need = stride * S;
        while (p->events.size() < need) {
            hipEvent_t e;
            DN_HIP_CHECK(hipEventCreate(&e));
            p->events.push_back(e);
        }
        p->prof_kernel.assign(p->ops.size(), "");
        p->prof_owner.assign(p->ops.size(), -1);
        int rc = enqueue_all(p, call, s, true);
        if (rc) return rc;
        DN_HIP_CHECK(hipStreamSynchronize(s));
        const size_t nseg = heads_only ? p->ops.size() : p->ops.size() + 4;      // + softmax/decode | cut-off + selection | merge | fallback
        if (p->prof_ms.size() < p->ops.size() + 4) p->prof_ms.assign(p->ops.size() + 4, 0.0);
        for (int k = 0; k < S; ++k)
            for (size_t i = 0; i < nseg; ++i) {
                float ms = 0.f;
                (void)hipEventElapsedTime(&ms, p->events[k * stride + i], p->events[k * stride + i + 1]);
                p->prof_ms[i] += ms;        // per op: summed over the sub-batch launches of one forward
            }
        p->prof_runs++;
        return DN_OK;
    }
    if (!p->graph_mode) return enqueue_all(p, call, s, false);

    // Default: the sub-batch chains are parallel branches of ONE graph. DN_CHAIN_GRAPHS=1: one single-chain hipGraph per
    // sub-batch, each replayed on a stream of its own (the caller's and the plan's branch streams, forked / joined with events
    // around the launches). In isolation (tools/queue_probe.hip) single-chain graphs on different streams overlap completely and
    // each queue pays its own 1.7 us per dependent launch, while the branches of one graph pay ~2.9 us per launch one after
    // another; on the real chain the two forms measure the same at two chains (1.25 vs 1.24 ms) and per-chain graphs lose
    // badly at three or four (1.9 ms): kept as an opt-in for that measurement only.
    // Measured (batch 32 = 2 x 16, 12 runs each): per-chain graphs 0.78 ms every time, one graph with two branches 0.785 ms in
    // two runs of three and 0.82 - 0.85 ms in the third (the placement of the branches differs from process to process); at batch
    // 64 one graph is 0.7 % faster (1.127 vs 1.135 ms). Default: per-chain graphs below 64 images.
    const bool want_chains = p->chain_graphs < 0 ? n < 64 : p->chain_graphs != 0;
    const bool per_chain = S > 1 && want_chains;
    const int G = per_chain ? S : 1;        // graphs of this call: one per chain, or one for the whole forward
    auto it = p->graphs.find(GraphKey{call, per_chain ? 0 : -1});
    if (it == p->graphs.end()) {
        // first call with this signature: run once eagerly (sets function attributes, validates), then capture
        int rc = enqueue_all(p, call, s, false);
        if (rc) return rc;
        if (p->graphs.size() + G > 64)      // bound the cache (a pipeline of forwards holds one entry per slot and output set)
            drop_graphs(p);                 // (drains the device first: other slots may be replaying these executables)
        for (int k = 0; k < G; ++k) {
            const int chain = per_chain ? k : -1;
            hipGraphExec_t ge = nullptr;
            rc = capture(p, call, S, chain, &ge);
            if (rc) return rc;
            p->graphs.emplace(GraphKey{call, chain}, ge);
        }
        return DN_OK;       // the eager run above already produced this call's results
    }
    if (G > 1) DN_HIP_CHECK(hipEventRecord(p->ev_fork, s));
    for (int k = 1; k < G; ++k) {
        auto itk = p->graphs.find(GraphKey{call, k});
        DN_REQUIRE(itk != p->graphs.end(), "dn_forward: chain graph %d missing", k);
        hipStream_t bs = p->branch_stream[k - 1];
        DN_HIP_CHECK(hipStreamWaitEvent(bs, p->ev_fork, 0));
        DN_HIP_CHECK(hipGraphLaunch(itk->second, bs));
        DN_HIP_CHECK(hipEventRecord(p->ev_branch[k - 1], bs));
    }
    DN_HIP_CHECK(hipGraphLaunch(it->second, s));
    for (int k = 1; k < G; ++k) DN_HIP_CHECK(hipStreamWaitEvent(s, p->ev_branch[k - 1], 0));
    return DN_OK;
}

extern "C" int dn_forward(dn_plan* plan, const float* images_dev, int n, int h, int w, float* boxes_dev, float* scores_dev,
                          int64_t* labels_dev, int32_t* counts_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    return forward_impl(plan, images_dev, n, h, w, boxes_dev, scores_dev, labels_dev, counts_dev, workspace_dev,
                        workspace_bytes, stream, false);
}

extern "C" int dn_forward_u8(dn_plan* plan, const uint8_t* images_dev, int n, int h, int w, float* boxes_dev, float* scores_dev,
                             int64_t* labels_dev, int32_t* counts_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    DN_REQUIRE(plan, "dn_forward_u8: null plan");
    return forward_impl(plan, images_dev, n, h, w, boxes_dev, scores_dev, labels_dev, counts_dev,
                        workspace_dev, workspace_bytes, stream, false, true);
}

extern "C" int dn_forward_frames(dn_plan* plan, const dn_frame* frames_dev, int n, int format, int color, float* boxes_dev, float* scores_dev,
                                 int64_t* labels_dev, int32_t* counts_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    DN_REQUIRE(plan, "dn_forward_frames: null plan");
    DN_REQUIRE(frames_dev, "dn_forward_frames: null record table");
    DN_REQUIRE(n > 0, "dn_forward_frames: n=%d", n);
    if (!dn_frame_codes_known(format, color)) {
        dn_set_error("dn_forward_frames: unknown format %d or colour code 0x%x", format, color);
        return DN_E_UNSUPPORTED;
    }
    return forward_impl(plan, nullptr, n, 0, 0, boxes_dev, scores_dev, labels_dev, counts_dev, workspace_dev, workspace_bytes, stream,
                        false, false, false, frames_dev, format, color);
}

extern "C" int dn_forward_regions(dn_plan* plan, const dn_frame* frames_dev, const dn_region* regions_dev, int n, int format, int color,
                                  float* boxes_dev, float* scores_dev, int64_t* labels_dev, int32_t* counts_dev, void* workspace_dev, size_t workspace_bytes,
                                  void* stream) {
    DN_REQUIRE(plan, "dn_forward_regions: null plan");
    DN_REQUIRE(frames_dev && regions_dev, "dn_forward_regions: null record table");
    DN_REQUIRE(n > 0, "dn_forward_regions: n=%d", n);
    if (!dn_frame_codes_known(format, color)) {
        dn_set_error("dn_forward_regions: unknown format %d or colour code 0x%x", format, color);
        return DN_E_UNSUPPORTED;
    }
    return forward_impl(plan, nullptr, n, 0, 0, boxes_dev, scores_dev, labels_dev, counts_dev, workspace_dev, workspace_bytes, stream,
                        false, false, false, frames_dev, format, color, regions_dev);
}

extern "C" int dn_forward_heads(dn_plan* plan, const float* images_dev, int n, int h, int w, void* workspace_dev,
                                size_t workspace_bytes, void* stream) {
    return forward_impl(plan, images_dev, n, h, w, nullptr, nullptr, nullptr, nullptr, workspace_dev, workspace_bytes, stream,
                        true);
}

extern "C" int dn_forward_features(dn_plan* plan, const float* images_dev, int n, int h, int w, void* workspace_dev,
                                   size_t workspace_bytes, void* stream) {
    return forward_impl(plan, images_dev, n, h, w, nullptr, nullptr, nullptr, nullptr, workspace_dev, workspace_bytes, stream,
                        true, false, true);
}

extern "C" int dn_level_features(const dn_plan* p, void* workspace, int n, int level, int chain, void** ptr, int* first_image, int* images) {
    DN_REQUIRE(p && workspace && n > 0 && ptr, "dn_level_features: bad argument");
    DN_REQUIRE(level >= 0 && level < p->d.n_levels, "dn_level_features: level %d out of range (%d levels)", level, p->d.n_levels);
    const int S = batch_split(p, n);
    DN_REQUIRE(chain >= 0 && chain < S, "dn_level_features: chain %d out of range (a forward of %d images runs as %d)", chain, n, S);
    const int t = p->d.level_tensor[level];
    const Layout& L = S == 1 ? get_layout(const_cast<dn_plan*>(p), n) : get_sub_layout(const_cast<dn_plan*>(p), n, S, chain);
    DN_REQUIRE(L.toff[t] != (size_t)-1, "dn_level_features: level %d is not materialised in the workspace", level);
    int n0 = 0;
    for (int q = 0; q < chain; ++q) n0 += sub_count(n, S, q);
    *ptr = reinterpret_cast<unsigned char*>(workspace) + L.toff[t];
    if (first_image) *first_image = n0;
    if (images) *images = S == 1 ? n : sub_count(n, S, chain);
    return DN_OK;
}

extern "C" int dn_head_outputs(const dn_plan* p, void* workspace, int n, float** logits, float** reg) {
    DN_REQUIRE(p && workspace && n > 0, "dn_head_outputs: bad argument");
    {
        const auto it = p->heads_partial.find(workspace);
        DN_REQUIRE(it == p->heads_partial.end() || !it->second, "dn_head_outputs: the last forward on this workspace was dn_forward, which may compute softmax / box "
                   "decode inside the head launch and never writes the large levels' logits: run dn_forward_heads first");
    }
    const Layout& L = get_layout(const_cast<dn_plan*>(p), n);
    if (logits) *logits = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(workspace) + L.logits_off);
    if (reg) *reg = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(workspace) + L.reg_off);
    return DN_OK;
}

extern "C" int dn_tensor_ptr(const dn_plan* p, void* workspace, int n, int tensor_id, void** ptr, size_t* bytes) {
    DN_REQUIRE(p && workspace && n > 0 && ptr, "dn_tensor_ptr: bad argument");
    DN_REQUIRE(tensor_id >= 0 && tensor_id < (int)p->tensors.size(), "dn_tensor_ptr: tensor id %d out of range", tensor_id);
    const Layout& L = get_layout(const_cast<dn_plan*>(p), n);
    DN_REQUIRE(L.toff[tensor_id] != (size_t)-1, "dn_tensor_ptr: tensor %d is not materialised in the workspace", tensor_id);
    DN_REQUIRE(L.chain_n == n, "dn_tensor_ptr: with workspace reuse the rows of a tensor are not contiguous across the sub-batch chains of a "
               "%d-image forward (DN_WS_REUSE=0 keeps one block per tensor)", n);
    *ptr = reinterpret_cast<unsigned char*>(workspace) + L.toff[tensor_id];
    if (bytes) *bytes = L.tbytes[tensor_id];
    return DN_OK;
}

// test support (include/demonet_hip_debug.h): what the stem of an n-image forward reads after a resize or a uint8 conversion -- the
// [n][3][image_h][image_w] fp32 block and the [n][2] (w, h) ratios, both contiguous over the sub-batch chains (get_sub_layout)
extern "C" __attribute__((visibility("default"))) int dn_debug_network_input(const dn_plan* p, void* workspace, int n, float** resized, float** scale_xy) {
    DN_REQUIRE(p && workspace && n > 0, "dn_debug_network_input: bad argument");
    const Layout& L = get_layout(const_cast<dn_plan*>(p), n);
    if (resized) *resized = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(workspace) + L.resized_off);
    if (scale_xy) *scale_xy = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(workspace) + L.scale_off);
    return DN_OK;
}

extern "C" int dn_batch_split(const dn_plan* p, int n) {
    DN_REQUIRE(p && n > 0, "dn_batch_split: bad argument");
    return batch_split(p, n);
}

extern "C" int dn_set_packed_output(dn_plan* p, float* packed_dev) {
    DN_REQUIRE(p, "null plan");
    DN_REQUIRE(p->in_call.load() == 0, "dn_set_packed_output: the plan is inside a forward of another host thread");
    p->packed_out = packed_dev;
    return DN_OK;
}

extern "C" int dn_profile_begin(dn_plan* p) {
    DN_REQUIRE(p, "null plan");
    p->profiling = true;
    p->prof_ms.assign(p->ops.size() + 4, 0.0);
    p->prof_runs = 0;
    return DN_OK;
}

extern "C" int dn_profile_op_info(const dn_plan* p, int op_index, char* kernel, int capacity, int32_t* owner) {
    DN_REQUIRE(p && kernel && owner && capacity > 0, "dn_profile_op_info: null argument");
    DN_REQUIRE(op_index >= 0 && (size_t)op_index < p->prof_kernel.size(), "dn_profile_op_info: op %d not profiled", op_index);
    snprintf(kernel, (size_t)capacity, "%s", p->prof_kernel[op_index].c_str());
    *owner = p->prof_owner[op_index];
    return DN_OK;
}

extern "C" int dn_profile_end(dn_plan* p, float* ms_per_op, int capacity) {
    DN_REQUIRE(p && ms_per_op, "null argument");
    p->profiling = false;
    const int nseg = (int)p->ops.size() + 4;
    DN_REQUIRE(capacity >= nseg, "dn_profile_end: capacity %d < %d", capacity, nseg);
    for (int i = 0; i < nseg; ++i) ms_per_op[i] = p->prof_runs ? (float)(p->prof_ms[i] / p->prof_runs) : 0.f;
    return p->prof_runs;
}

// ---------------------------------------------------------------------------------------------------------
// stand-alone entry points
// ---------------------------------------------------------------------------------------------------------
extern "C" size_t dn_postprocess_workspace_bytes(int n, int num_anchors, int num_classes, int topk, int dets) {
    return postprocess_ws_bytes(n, num_anchors, num_classes, topk, dets);
}

extern "C" int dn_postprocess_soft(const float* logits, const float* reg, const float* anchors, int n, int A, int K, float image_h,
                                   float image_w, const float* scale_xy, float score_thresh, float nms_thresh, int nms_method, float nms_sigma,
                                   int topk, int dets, float* boxes, float* scores, int64_t* labels, int32_t* counts, int32_t* kept_anchor,
                                   void* ws, size_t ws_bytes, void* stream) {
    DN_REQUIRE(logits && reg && anchors && boxes && scores && labels && counts && ws, "dn_postprocess: null argument");
    DN_REQUIRE(score_thresh >= 0.f, "dn_postprocess: score_thresh must be >= 0");
    if (K > DN_MAX_CLASSES) {
        dn_set_error("dn_postprocess: num_classes=%d above the limit of %d (DN_MAX_CLASSES, background included)", K, DN_MAX_CLASSES);
        return DN_E_UNSUPPORTED;
    }
    PostArgs a;
    a.logits = logits; a.reg = reg; a.anchors = anchors; a.n = n; a.A = A; a.K = K;
    a.img_h = image_h; a.img_w = image_w; a.scale_xy = scale_xy;
    a.score_thresh = score_thresh; a.nms_thresh = nms_thresh; a.topk = topk; a.dets = dets;
    a.nms_method = nms_method; a.nms_sigma = nms_sigma;
    a.boxes = boxes; a.scores = scores; a.labels = labels; a.counts = counts; a.kept_anchor = kept_anchor;
    a.ws = ws; a.ws_bytes = ws_bytes;
    a.xq = xcd_images_per_group(n);
    return launch_postprocess(a, reinterpret_cast<hipStream_t>(stream), nullptr);
}

extern "C" int dn_postprocess(const float* logits, const float* reg, const float* anchors, int n, int A, int K, float image_h,
                              float image_w, const float* scale_xy, float score_thresh, float nms_thresh, int topk, int dets,
                              float* boxes, float* scores, int64_t* labels, int32_t* counts, int32_t* kept_anchor, void* ws,
                              size_t ws_bytes, void* stream) {
    return dn_postprocess_soft(logits, reg, anchors, n, A, K, image_h, image_w, scale_xy, score_thresh, nms_thresh, DN_NMS_HARD, 0.f, topk, dets,
                               boxes, scores, labels, counts, kept_anchor, ws, ws_bytes, stream);
}

extern "C" int dn_pointwise_conv(const void* x, const void* w, const void* w_frag, const float* bias, const void* residual,
                                 const float* se, void* out, int m, int cin, int cout, int hw, int act, int out_fp32,
                                 int64_t out_img_stride, void* stream) {
    DN_REQUIRE(x && w && bias && out, "dn_pointwise_conv: null argument");
    PwArgs a;
    a.x = reinterpret_cast<const half_t*>(x); a.w = reinterpret_cast<const half_t*>(w); a.bias = bias;
    a.wfrag = reinterpret_cast<const half_t*>(w_frag);
    a.residual = reinterpret_cast<const half_t*>(residual); a.se = se; a.out = out;
    a.m = m; a.cin = cin; a.cout = cout; a.hw = hw; a.act = act; a.out_fp32 = out_fp32;
    a.out_img_stride = out_fp32 ? (long)out_img_stride : 0; a.out_base = 0;
    a.xq = (hw > 0 && m % hw == 0) ? xcd_images_per_group(m / hw) : 0;
    int rc = launch_pointwise(a, reinterpret_cast<hipStream_t>(stream));
    if (rc) return rc;
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}

extern "C" int dn_expand_depthwise(const void* x, const void* w1, const float* b1, const void* wd, const float* bd, const void* w3,
                                   const float* b3, void* out, float* pool_partial, int n, int h, int w, int cin, int cexp, int cout,
                                   int k, int stride, int act1, int act2, int has_res, void* stream) {
    DN_REQUIRE(x && wd && bd && out, "dn_expand_depthwise: null argument");
    DN_REQUIRE((w1 == nullptr) == (b1 == nullptr) && (w3 == nullptr) == (b3 == nullptr), "dn_expand_depthwise: weight without bias");
    ExpDwArgs a{};
    a.x = reinterpret_cast<const half_t*>(x); a.out = reinterpret_cast<half_t*>(out); a.pool = pool_partial;
    a.w1 = reinterpret_cast<const half_t*>(w1); a.b1 = b1; a.wd = reinterpret_cast<const half_t*>(wd); a.bd = bd;
    a.w3 = reinterpret_cast<const half_t*>(w3); a.b3 = b3;
    a.n = n; a.H = h; a.W = w; a.k = k; a.stride = stride; a.pad = (k - 1) / 2;
    a.Ho = (h + 2 * a.pad - k) / stride + 1; a.Wo = (w + 2 * a.pad - k) / stride + 1;
    a.cin = cin; a.cexp = cexp; a.cout = w3 ? cout : cexp; a.act1 = act1; a.act2 = act2; a.has_res = has_res;
    a.xq = xcd_images_per_group(n);
    int rc = launch_expdw(a, reinterpret_cast<hipStream_t>(stream));
    if (rc) return rc;
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}

extern "C" int dn_expand_depthwise_tiles(int ho, int wo, int stride) { return expdw_tiles_per_image(ho, wo, stride); }

extern "C" int dn_depthwise_pointwise(const void* x, const void* wd, const float* bd, const void* w, const float* b, void* out, int n, int h,
                                      int wdt, int c, int cout, int act_dw, int act, int has_res, void* stream) {
    DN_REQUIRE(x && wd && bd && w && b && out, "dn_depthwise_pointwise: null argument");
    DN_REQUIRE(n > 0 && h > 0 && wdt > 0 && c > 0 && cout > 0, "dn_depthwise_pointwise: bad geometry");
    if (!dn_rows_fit(n, (long)h * wdt)) {
        dn_set_error("dn_depthwise_pointwise: n=%d images of %d x %d pixels do not fit 32-bit row indices", n, h, wdt);
        return DN_E_UNSUPPORTED;
    }
    DwArgs d{};
    d.x = reinterpret_cast<const half_t*>(x); d.w = reinterpret_cast<const half_t*>(wd); d.bias = bd;
    d.n = n; d.h = h; d.w_ = wdt; d.c = c; d.k = 3; d.stride = 1; d.pad = 1; d.act = act_dw; d.ho = h; d.wo = wdt;
    PwArgs a{};
    a.x = d.x; a.w = reinterpret_cast<const half_t*>(w); a.bias = b; a.residual = has_res ? d.x : nullptr; a.se = nullptr; a.out = out;
    a.m = n * h * wdt; a.cin = c; a.cout = cout; a.hw = h * wdt; a.act = act; a.out_fp32 = 0; a.out_img_stride = 0; a.out_base = 0;
    a.xq = d.xq = xcd_images_per_group(n);
    if (!pw_dw_direct_supported(a, d)) {
        dn_set_error("dn_depthwise_pointwise: unsupported n=%d h=%d w=%d c=%d cout=%d has_res=%d", n, h, wdt, c, cout, has_res);
        return DN_E_UNSUPPORTED;
    }
    int rc = launch_pw_dw_direct(a, d, reinterpret_cast<hipStream_t>(stream));
    if (rc) return rc;
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}

extern "C" int dn_dense_conv(const void* x, const void* w, const float* bias, const void* zeros, void* out, int n, int h, int wd,
                             int cin, int cout, int k, int stride, int pad, int dil, int act, void* stream) {
    DN_REQUIRE(x && w && bias && out, "dn_dense_conv: null argument");
    DN_REQUIRE(n > 0 && h > 0 && wd > 0 && k >= 1 && stride >= 1 && dil >= 1 && pad >= 0, "dn_dense_conv: bad geometry");
    ConvArgs a;
    a.x = reinterpret_cast<const half_t*>(x); a.w = reinterpret_cast<const half_t*>(w); a.bias = bias; a.out = out;
    a.zeros = reinterpret_cast<const half_t*>(zeros);
    a.n = n; a.h = h; a.w_ = wd; a.cin = cin; a.cout = cout; a.k = k; a.stride = stride; a.pad = pad; a.dil = dil; a.act = act;
    a.ho = (h + 2 * pad - dil * (k - 1) - 1) / stride + 1;
    a.wo = (wd + 2 * pad - dil * (k - 1) - 1) / stride + 1;
    DN_REQUIRE(a.ho > 0 && a.wo > 0, "dn_dense_conv: empty output");
    a.out_fp32 = 0; a.out_img_stride = 0; a.out_base = 0;
    a.xq = xcd_images_per_group(n);
    int rc = launch_conv(a, reinterpret_cast<hipStream_t>(stream));
    if (rc) return rc;
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}

extern "C" int dn_depthwise_conv(const void* x, const void* w, const float* bias, void* out, int n, int h, int wd, int c, int k,
                                 int stride, int pad, int act, void* stream) {
    DN_REQUIRE(x && w && bias && out, "dn_depthwise_conv: null argument");
    DwArgs a;
    a.x = reinterpret_cast<const half_t*>(x); a.w = reinterpret_cast<const half_t*>(w); a.bias = bias;
    a.out = reinterpret_cast<half_t*>(out);
    a.n = n; a.h = h; a.w_ = wd; a.c = c; a.k = k; a.stride = stride; a.pad = pad; a.act = act;
    a.ho = (h + 2 * pad - k) / stride + 1;
    a.wo = (wd + 2 * pad - k) / stride + 1;
    a.xq = xcd_images_per_group(n);
    int rc = launch_depthwise(a, reinterpret_cast<hipStream_t>(stream));
    if (rc) return rc;
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}

extern "C" int dn_depthwise_pool_blocks(int h, int wd, int c, int k, int stride, int pad) {
    DwArgs a{};
    a.n = 1; a.h = h; a.w_ = wd; a.c = c; a.k = k; a.stride = stride; a.pad = pad;
    a.ho = (h + 2 * pad - k) / stride + 1;
    a.wo = (wd + 2 * pad - k) / stride + 1;
    return depthwise_pool_blocks(a);
}

extern "C" int dn_depthwise_conv_pool(const void* x, const void* w, const float* bias, void* out, int n, int h, int wd, int c, int k,
                                      int stride, int pad, int act, float* pool, const void* se_w1t, const float* se_b1, const void* se_w2t,
                                      const float* se_b2, float* se_scale, unsigned* se_counter, int squeeze, void* stream) {
    DN_REQUIRE(x && w && bias && out && pool, "dn_depthwise_conv_pool: null argument");
    DN_REQUIRE(!se_scale || (se_w1t && se_b1 && se_w2t && se_b2 && se_counter), "dn_depthwise_conv_pool: the squeeze-excitation tail needs both FCs and the counters");
    DwArgs a;
    a.x = reinterpret_cast<const half_t*>(x); a.w = reinterpret_cast<const half_t*>(w); a.bias = bias;
    a.out = reinterpret_cast<half_t*>(out);
    a.n = n; a.h = h; a.w_ = wd; a.c = c; a.k = k; a.stride = stride; a.pad = pad; a.act = act;
    a.ho = (h + 2 * pad - k) / stride + 1;
    a.wo = (wd + 2 * pad - k) / stride + 1;
    a.xq = xcd_images_per_group(n);
    a.pool = pool;
    if (se_scale) {
        a.se_w1t = reinterpret_cast<const half_t*>(se_w1t); a.se_b1 = se_b1;
        a.se_w2t = reinterpret_cast<const half_t*>(se_w2t); a.se_b2 = se_b2;
        a.se_scale = se_scale; a.se_counter = se_counter; a.se_sq = squeeze;
        a.se_inv = 1.0f / (float)(a.ho * a.wo);
    }
    int rc = launch_depthwise(a, reinterpret_cast<hipStream_t>(stream));
    if (rc) return rc;
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}

// ---- test support (include/demonet_hip_debug.h): which kernel a stand-alone call took, the image-range loop of launch_conv_pool without a
// model around it, and the choice functions of choice.h asked about a shape on a machine without a GPU
extern "C" __attribute__((visibility("default"))) int dn_debug_last_kernel(char* buf, int capacity) {
    DN_REQUIRE(buf && capacity > 0, "dn_debug_last_kernel: no buffer");
    snprintf(buf, (size_t)capacity, "%s", dn_last_kernel());
    return DN_OK;
}

extern "C" __attribute__((visibility("default"))) int dn_debug_conv_pool(const void* x, const void* w, const float* bias, const void* zeros, void* pool_out,
                                                                        void* out, int n, int h, int wd, int cin, int cout, int act, void* stream) {
    DN_REQUIRE(x && w && bias && pool_out, "dn_debug_conv_pool: null argument");
    DN_REQUIRE(n > 0 && h > 0 && wd > 0 && dn_rows_fit(n, (long)h * wd), "dn_debug_conv_pool: bad geometry, or 2^31 rows or more");
    DN_REQUIRE(cin % 32 == 0 && cout % 4 == 0, "dn_debug_conv_pool: cin=%d must be a multiple of 32, cout=%d of 4", cin, cout);
    ConvArgs c;
    c.x = reinterpret_cast<const half_t*>(x); c.w = reinterpret_cast<const half_t*>(w); c.bias = bias; c.out = out;
    c.zeros = reinterpret_cast<const half_t*>(zeros);
    c.n = n; c.h = h; c.w_ = wd; c.cin = cin; c.cout = cout; c.k = 3; c.stride = 1; c.pad = 1; c.dil = 1; c.act = act;
    c.ho = h; c.wo = wd;
    c.out_fp32 = 0; c.out_img_stride = 0; c.out_base = 0;
    c.xq = xcd_images_per_group(n);
    PwArgs a = conv_to_pw(c);
    a.pool_out = reinterpret_cast<half_t*>(pool_out);
    int rc = launch_conv_pool(a, reinterpret_cast<hipStream_t>(stream));
    if (rc) return rc;
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}

// launch_stem on its own: image [n][3][h][w] fp32 in [0, 1], w [27][cout] fp32 (tap (c 3 + ky) 3 + kx), 3 x 3, out [n][ho][wo][cout] fp16. split_ok and
// scale_log2 are what dn_create derives from the host copy of the weights (check_stems): finite values, the largest magnitude times 2^scale_log2 in [2^14, 2^15)
extern "C" __attribute__((visibility("default"))) int dn_debug_stem(const float* img, const float* w, const float* bias, void* out, int n, int h, int wd, int cout,
                                                                   int stride, int pad, int act, const float* mean3, const float* std3, int split_ok, int scale_log2,
                                                                   void* stream) {
    DN_REQUIRE(img && w && bias && out && mean3 && std3, "dn_debug_stem: null argument");
    DN_REQUIRE(n > 0 && h > 0 && wd > 0 && stride >= 1 && pad >= 0 && dn_rows_fit(n, (long)h * wd), "dn_debug_stem: bad geometry, or 2^31 rows or more");
    StemArgs a{};
    a.img = img; a.w = w; a.bias = bias; a.out = reinterpret_cast<half_t*>(out);
    a.n = n; a.h = h; a.w_ = wd; a.cout = cout; a.k = 3; a.stride = stride; a.pad = pad; a.act = act;
    a.ho = (h + 2 * pad - 3) / stride + 1; a.wo = (wd + 2 * pad - 3) / stride + 1;
    DN_REQUIRE(a.ho > 0 && a.wo > 0, "dn_debug_stem: empty output");
    for (int q = 0; q < 3; ++q) { DN_REQUIRE(std3[q] > 0.f, "dn_debug_stem: std must be positive"); a.mean[q] = mean3[q]; a.inv_std[q] = 1.0f / std3[q]; }
    a.xq = xcd_images_per_group(n);
    a.split_ok = split_ok ? 1 : 0;
    a.w_scale = std::ldexp(1.0f, scale_log2);
    a.w_unscale = std::ldexp(1.0f, -scale_log2);
    int rc = launch_stem(a, reinterpret_cast<hipStream_t>(stream));
    if (rc) return rc;
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}

static const char* pw_choice_name(PwChoice::Kernel k) {
    switch (k) {
        case PwChoice::NONE: return "none";
        case PwChoice::AS_POINTWISE: return "as_pointwise";
        case PwChoice::PW_WSTAT: return "pw_wstat_kernel";
        case PwChoice::PW_STREAM: return "pw_stream_kernel";
        case PwChoice::PW_DIRECT: return "pw_direct_kernel";
        case PwChoice::PW_XS: return "pw_xs_kernel";
        case PwChoice::PW_TILE: return "pw_kernel";
        case PwChoice::PW_GROUP: return "pw_group_kernel";
        case PwChoice::CONV_PATCH: return "conv_patch_kernel";
        case PwChoice::CONV_PATCH_RESIDENT: return "conv_patch_resident_kernel";
        case PwChoice::CONV_HALO: return "conv_halo_kernel";
        case PwChoice::CONV_GLDS: return "conv_glds_kernel";
    }
    return "?";
}
static int pw_choice_text(const PwChoice& c, char* buf, int capacity) {
    snprintf(buf, (size_t)capacity, "kernel=%s tile=%dx%d bk=%d pf=%d conv=%d sef=%d fk=%d k=%d t=%d halo=%d head=%d pool=%d proj=%d", pw_choice_name(c.kernel), c.bp, c.bc,
             c.bk, c.pf, (int)c.conv, (int)c.sef, (int)c.fk, c.k, c.t, c.halo, (int)c.head, (int)c.pool, (int)c.proj);
    return DN_OK;
}

void depthwise_debug_limits(const DwArgs& a, int tw, bool* in_range, size_t* wlds_bytes);       // depthwise.hip

// family and dims (every entry an int64; pointers are asked for as 0 / 1 flags and stand in as dummies: no function called here reads through one):
//   "pw"        m cin cout hw act out_fp32 se residual wfrag                    -> pw_choose
//   "pw_group"  conv count, then count x (m cin cout hw)                        -> pw_group_choose (problems without scale or activation)
//   "conv"      n h w cin cout k stride pad dil act zeros use[0 plain, 1 pooled, 2 head] cout_b   -> conv_choose; a 1x1 that the pointwise family serves: pw_choose's answer
//   "dw"        n h w c k stride pad                                            -> dw_choose, dw_fill (range=), dw_wlds_bytes (wlds=)
//   "stem"      n h w cout stride pad act split_ok                              -> stem_choose
//   "headfuse"  n H W C nc0 nc1 stride0 stride1                                 -> head_fused_level_supported (supported=)
//   "headpost"  n H W aloc K A                                                  -> head_fused_post_supported of one level with the epilogue (supported=)
//   "patch_blocks" n h w                                                        -> conv_patch_resident_blocks (blocks=, launched=: below the launcher's 2^30)
//   "expdw"     n h w cin cexp cout k stride act1 act2 has_res pool             -> expdw_choose (body=direct / rows / tiled / none, band=, label=, tile=<oh>x<ow>); cout 0: no project stage, act1 -1: no expand stage
//   "expdw_whole" the same twelve numbers                                       -> expdw_choose's flag of the tiled body (whole=, lds= the whole-width form's LDS bytes, 0 without it)
extern "C" __attribute__((visibility("default"))) int dn_debug_choice(const char* family, const int64_t* d, int nd, char* buf, int capacity) {
    DN_REQUIRE(family && d && buf && capacity > 0, "dn_debug_choice: null argument");
    static const half_t dummy_h[8] = {};
    static const float dummy_f[4] = {};
    static float dummy_out[4];
    auto fits = [](int64_t v) { return v >= 0 && v < (1LL << 31); };
    const std::string f(family);
    if (f == "pw") {
        DN_REQUIRE(nd == 9 && fits(d[0]) && d[3] > 0, "dn_debug_choice: pw takes m cin cout hw act out_fp32 se residual wfrag, m below 2^31");
        PwArgs a{};
        a.x = a.w = dummy_h; a.bias = dummy_f; a.out = dummy_out;
        a.m = (int)d[0]; a.cin = (int)d[1]; a.cout = (int)d[2]; a.hw = (int)d[3]; a.act = (int)d[4]; a.out_fp32 = (int)d[5];
        a.se = d[6] ? dummy_f : nullptr; a.residual = d[7] ? dummy_h : nullptr; a.wfrag = d[8] ? dummy_h : nullptr;
        return pw_choice_text(pw_choose(a), buf, capacity);
    }
    if (f == "pw_group") {
        DN_REQUIRE(nd >= 2 && d[1] >= 1 && d[1] <= 12 && nd == 2 + 4 * d[1], "dn_debug_choice: pw_group takes conv count and count x (m cin cout hw)");
        PwArgs arr[12];
        for (int i = 0; i < (int)d[1]; ++i) {
            const int64_t* q = d + 2 + 4 * i;
            DN_REQUIRE(fits(q[0]) && q[3] > 0, "dn_debug_choice: pw_group problem %d: m must lie below 2^31", i);
            PwArgs a{};
            a.x = a.w = dummy_h; a.bias = dummy_f; a.out = dummy_out;
            a.m = (int)q[0]; a.cin = (int)q[1]; a.cout = (int)q[2]; a.hw = (int)q[3]; a.out_fp32 = 1;
            if (d[0]) { a.cv_k = 3; a.cv_cin = a.cin; a.cin = 9 * a.cv_cin; }
            arr[i] = a;
        }
        return pw_choice_text(pw_group_choose(arr, (int)d[1], d[0] != 0), buf, capacity);
    }
    if (f == "conv") {
        DN_REQUIRE(nd == 13 && d[0] > 0 && d[1] > 0 && d[2] > 0 && d[5] >= 1 && d[6] >= 1 && d[8] >= 1, "dn_debug_choice: conv takes n h w cin cout k stride pad dil act zeros use cout_b");
        ConvArgs c;
        c.x = c.w = dummy_h; c.bias = dummy_f; c.out = dummy_out; c.zeros = d[10] ? dummy_h : nullptr;
        c.n = (int)d[0]; c.h = (int)d[1]; c.w_ = (int)d[2]; c.cin = (int)d[3]; c.cout = (int)d[4]; c.k = (int)d[5]; c.stride = (int)d[6]; c.pad = (int)d[7];
        c.dil = (int)d[8]; c.act = (int)d[9];
        c.ho = (c.h + 2 * c.pad - c.dil * (c.k - 1) - 1) / c.stride + 1;
        c.wo = (c.w_ + 2 * c.pad - c.dil * (c.k - 1) - 1) / c.stride + 1;
        DN_REQUIRE(c.ho > 0 && c.wo > 0 && dn_rows_fit(d[0], (long)c.ho * c.wo), "dn_debug_choice: conv with an empty output, or 2^31 rows or more");
        const int use = (int)d[11];
        c.out_fp32 = use == 2; c.out_img_stride = use == 2 ? (long)c.ho * c.wo * (c.cout + d[12]) : 0; c.out_base = 0; c.xq = 0;
        PwArgs a = conv_to_pw(c);
        if (use == 1) a.pool_out = const_cast<half_t*>(dummy_h);
        if (use == 2 && d[12] > 0) { a.w_b = dummy_h; a.bias_b = dummy_f; a.out_b = dummy_out; a.cout_b = (int)d[12]; }
        PwChoice ch = conv_choose(a, use == 1 ? CONV_POOLED : use == 2 ? CONV_HEAD : CONV_PLAIN);
        if (ch.kernel == PwChoice::AS_POINTWISE) ch = pw_choose(conv_1x1_as_pw(a));
        return pw_choice_text(ch, buf, capacity);
    }
    if (f == "dw") {
        DN_REQUIRE(nd == 7 && d[0] > 0 && d[1] > 0 && d[2] > 0 && d[5] >= 1, "dn_debug_choice: dw takes n h w c k stride pad");
        DwArgs a{};
        a.x = a.w = dummy_h; a.bias = dummy_f;
        a.n = (int)d[0]; a.h = (int)d[1]; a.w_ = (int)d[2]; a.c = (int)d[3]; a.k = (int)d[4]; a.stride = (int)d[5]; a.pad = (int)d[6];
        a.ho = (a.h + 2 * a.pad - a.k) / a.stride + 1; a.wo = (a.w_ + 2 * a.pad - a.k) / a.stride + 1;
        const DwChoice c = dw_choose(a);
        if (c.kernel == DwChoice::NONE) { snprintf(buf, (size_t)capacity, "kernel=none"); return DN_OK; }
        bool in_range = false;
        size_t wlds = 0;
        depthwise_debug_limits(a, c.tw, &in_range, &wlds);
        snprintf(buf, (size_t)capacity, "kernel=dw_kernel<%d,%d,%d> range=%d wlds=%zu", c.k, c.stride, c.tw, (int)in_range, wlds);
        return DN_OK;
    }
    if (f == "stem") {
        DN_REQUIRE(nd == 8 && d[0] > 0 && d[1] > 0 && d[2] > 0 && d[4] >= 1, "dn_debug_choice: stem takes n h w cout stride pad act split_ok");
        StemArgs a{};
        a.n = (int)d[0]; a.h = (int)d[1]; a.w_ = (int)d[2]; a.cout = (int)d[3]; a.k = 3; a.stride = (int)d[4]; a.pad = (int)d[5]; a.act = (int)d[6]; a.split_ok = (int)d[7];
        a.ho = (a.h + 2 * a.pad - 3) / a.stride + 1; a.wo = (a.w_ + 2 * a.pad - 3) / a.stride + 1;
        const StemChoice c = stem_choose(a);
        static const char* const names[] = {"none", "stem_split_kernel", "stem3s2_kernel", "stem_mfma64p_kernel", "stem_mfma64_kernel", "stem_kernel"};
        snprintf(buf, (size_t)capacity, "kernel=%s tpw=%d ahead=%d touch=%d", names[c.kernel], c.tpw, c.ahead, (int)c.touch);
        return DN_OK;
    }
    if (f == "headfuse") {
        DN_REQUIRE(nd == 8 && d[0] > 0, "dn_debug_choice: headfuse takes n H W C nc0 nc1 stride0 stride1");
        HeadFuseLevel l{};
        l.x = l.wdg = dummy_h; l.wslot = reinterpret_cast<const unsigned char*>(dummy_h);
        for (int h = 0; h < 2; ++h) { l.wf[h] = dummy_h; l.bias[h] = dummy_f; l.out[h] = nullptr; l.out_img_stride[h] = (long)d[6 + h]; l.out_base[h] = 0; l.nc[h] = (int)d[4 + h]; }
        l.n = (int)d[0]; l.H = (int)d[1]; l.W = (int)d[2]; l.C = (int)d[3]; l.act = DN_ACT_RELU6;
        snprintf(buf, (size_t)capacity, "supported=%d", (int)head_fused_level_supported(l));
        return DN_OK;
    }
    if (f == "headpost") {
        DN_REQUIRE(nd == 6 && d[0] > 0, "dn_debug_choice: headpost takes n H W aloc K A");
        HeadFuseLevel l{};
        l.n = (int)d[0]; l.H = (int)d[1]; l.W = (int)d[2]; l.aloc = (int)d[3]; l.nc[0] = (int)(d[3] * d[4]); l.nc[1] = (int)(4 * d[3]); l.sm = 1; l.sbase = 0;
        HeadPost post;
        post.scoresT = dummy_out; post.boxes = reinterpret_cast<float4*>(dummy_out); post.hrows = reinterpret_cast<unsigned*>(dummy_out); post.anchors = dummy_f;
        post.K = (int)d[4]; post.A = (int)d[5]; post.nb = 1; post.rows_per_image = hist_rows_slots(l.H * l.W);
        snprintf(buf, (size_t)capacity, "supported=%d", (int)head_fused_post_supported(&l, 1, post));
        return DN_OK;
    }
    if (f == "patch_blocks") {
        DN_REQUIRE(nd == 3 && d[0] > 0 && d[1] > 0 && d[2] > 0, "dn_debug_choice: patch_blocks takes n h w");
        const long blocks = conv_patch_resident_blocks((int)d[0], (int)d[1], (int)d[2]);
        snprintf(buf, (size_t)capacity, "blocks=%ld launched=%d", blocks, (int)(blocks < (1L << 30)));
        return DN_OK;
    }
    if (f == "expdw" || f == "expdw_whole") {
        DN_REQUIRE(nd == 12 && d[0] > 0 && d[1] > 0 && d[2] > 0 && d[6] >= 1 && d[7] >= 1, "dn_debug_choice: expdw takes n h w cin cexp cout k stride act1 act2 has_res pool");
        ExpDwArgs a{};
        a.x = a.wd = dummy_h; a.bd = dummy_f; a.pool = d[11] ? dummy_out : nullptr;
        if (d[8] >= 0) { a.w1 = dummy_h; a.b1 = dummy_f; }
        if (d[5] > 0) { a.w3 = dummy_h; a.b3 = dummy_f; }
        a.n = (int)d[0]; a.H = (int)d[1]; a.W = (int)d[2]; a.cin = (int)d[3]; a.cexp = (int)d[4]; a.cout = a.w3 ? (int)d[5] : a.cexp; a.k = (int)d[6]; a.stride = (int)d[7];
        a.pad = (a.k - 1) / 2; a.Ho = (a.H + 2 * a.pad - a.k) / a.stride + 1; a.Wo = (a.W + 2 * a.pad - a.k) / a.stride + 1;
        a.act1 = a.w1 ? (int)d[8] : 0; a.act2 = (int)d[9]; a.has_res = (int)d[10]; a.xq = xcd_images_per_group(a.n);
        DN_REQUIRE(a.Ho > 0 && a.Wo > 0, "dn_debug_choice: expdw with an empty output");
        const ExpDwChoice c = expdw_choose(a, false);
        if (f == "expdw_whole") { snprintf(buf, (size_t)capacity, "whole=%d lds=%zu", (int)c.whole, c.whole ? c.lds_w : (size_t)0); return DN_OK; }
        static const char* const bodies[] = {"none", "direct", "rows", "tiled", "tiled"};       // NONE, DIRECT, ROWS, ONE_PERSIST, TILED
        snprintf(buf, (size_t)capacity, "body=%s band=%d label=%s tile=%dx%d", bodies[c.body], c.band, c.label, c.oh, c.ow);
        return DN_OK;
    }
    dn_set_error("dn_debug_choice: unknown family '%s'", family);
    return DN_E_INVALID;
}
