// The frame step of one stream: the BODY of track_update_kernel (track.hip) and of track_update_app_kernel (trackapp.hip), included as text
// between the braces of each. It is text and not a function because the device code of track_update_kernel must stay, instruction for
// instruction, what it was when this body stood in track.hip: as an inlined function template the same statements compile to a different
// LDS layout and another schedule. The including kernel provides, in front of the #include:
//     constexpr bool APP         false: dn_track_update's step; true: the appearance step (every such statement is behind `if constexpr (APP)`)
//     const TrackArgs a          the kernel's argument
//     const TrackAppArgs p       what the appearance step adds (APP = false: never read)
//     unsigned char* dfeat       TK_MAX_D bytes of LDS: the row has an embedding (APP = false: never read)
// trackcore.h (included at file scope) has the constants, the argument records and the helpers, and describes how the step works.
    __shared__ uint4 st4[1 + 7 * TK_NT];       // the stream's state block, as it lies in memory
    __shared__ float4 dbox[TK_MAX_D];
    __shared__ long long dlab[TK_MAX_D];
    __shared__ float dscore[TK_MAX_D];
    __shared__ int dcls[TK_MAX_D];             // TK_NONE / TK_HIGH / TK_LOW; TK_NONE again once a track has taken the row
    __shared__ int did[TK_MAX_D];              // -1: free; otherwise the id of the track that took the row
    __shared__ int dhas[TK_MAX_D];             // this round: some track proposed to the row
    __shared__ int dprop[TK_MAX_D];            // this stage: the row's best track when it was last scanned, -1 nobody, -2 not scanned yet
    __shared__ unsigned long long dkey[TK_MAX_D];   // this stage: the largest (IoU bits, ~slot) over the admissible pairs of the row, 0 none
    __shared__ float4 tbox[TK_NT];
    __shared__ long long tlab[TK_NT];
    __shared__ int tact[TK_NT];                // the slot takes part in the current stage and is still unmatched
    __shared__ int detlist[TK_NT];             // r -> row of the r-th starting detection
    __shared__ int wtot[TK_WAVES];

    const int b = blockIdx.x, t = threadIdx.x;
    const int T = a.T, Tp = a.Tp, d = a.d;
    const int words = TK_HDR + TK_SLOT_WORDS * Tp;
    uint4* const gstate = a.state + (size_t)b * (words / 4);
    int* const sti = reinterpret_cast<int*>(st4);
    float* const stf = reinterpret_cast<float*>(st4);
    const int oState = TK_HDR, oId = TK_HDR + Tp, oLabel = TK_HDR + 2 * Tp, oScore = TK_HDR + 4 * Tp, oFilt = TK_HDR + 5 * Tp,
              oStart = TK_HDR + 25 * Tp, oLast = TK_HDR + 26 * Tp, oDet = TK_HDR + 27 * Tp;

    for (int i = t; i < words / 4; i += TK_NT) st4[i] = gstate[i];
    int n = a.counts[b];
    n = n < 0 ? 0 : (n > d ? d : n);
    for (int j = t; j < TK_MAX_D; j += TK_NT) {
        int cls = TK_NONE;
        if (j < n) {
            const size_t g = (size_t)b * d + j;
            const float4 bx = a.boxes[g];
            const float s = a.scores[g];
            dbox[j] = bx;
            dscore[j] = s;
            dlab[j] = a.labels[g];
            const bool fin = fabsf(bx.x) < INFINITY && fabsf(bx.y) < INFINITY && fabsf(bx.z) < INFINITY && fabsf(bx.w) < INFINITY;
            const bool ok = s == s && fin && (bx.z - bx.x) > 0.0f && (bx.w - bx.y) > 0.0f;
            if (ok) cls = s >= a.track_thresh ? TK_HIGH : ((s > a.low_thresh && s < a.track_thresh) ? TK_LOW : TK_NONE);
        }
        dcls[j] = cls;
        did[j] = -1;
        dhas[j] = 0;
        if constexpr (APP) {
            // the row has an embedding: the index table named it (the highest slot that did) and that slot's embedding is present
            bool has = false;
            if (j < n && p.map) {
                const int e = p.map[(size_t)b * d + j];
                has = e >= 0 && p.epres[e] != 0;
            }
            dfeat[j] = has ? 1 : 0;
        }
    }
    __syncthreads();

    // 1. the header and the own slot
    const int frame = sti[0] + 1;
    const int next_id = sti[1];
    int dropped = sti[2];
    const bool slot = t < T;
    int state = TK_FREE, id = 0, start = 0, last = 0, det = 0;
    long long label = 0;
    float score = 0.0f;
    float f[20];
#pragma unroll
    for (int i = 0; i < 20; ++i) f[i] = 0.0f;
    if (slot) {
        state = sti[oState + t];
        id = sti[oId + t];
        label = reinterpret_cast<const long long*>(sti + oLabel)[t];
        score = stf[oScore + t];
#pragma unroll
        for (int i = 0; i < 20; ++i) f[i] = stf[oFilt + i * Tp + t];
        start = sti[oStart + t];
        last = sti[oLast + t];
        det = state == TK_FREE ? 0 : -1;
    }
    // the own slot's feature: its flag, its row of S, and what the tail will do to it
    [[maybe_unused]] bool fvalid = false;
    [[maybe_unused]] int fop = TK_F_NONE;
    [[maybe_unused]] const float* srow = nullptr;
    if constexpr (APP) {
        if (slot) {
            fvalid = state != TK_FREE && p.fflag[(size_t)b * (Tp + (size_t)Tp * p.dim) + t] != 0;
            srow = p.S + ((size_t)b * Tp + t) * d;
        }
    }

    // 3. predict the tracked and the lost tracks (a lost track's velocity of h is cleared first); tentative tracks stay as they are
    if (state == TK_LOST) f[16] = 0.0f;
    if (state == TK_TRACKED || state == TK_LOST) tk_predict(f);
    tbox[t] = tk_box(f);
    tlab[t] = label;

    const bool agn = a.class_agnostic != 0;
    const int before = state;                  // the state this frame began with
    bool matched = false;
    for (int stage = 1; stage <= 3; ++stage) {
        const int cls = stage == 2 ? TK_LOW : TK_HIGH;
        const float gate = stage == 1 ? a.gate1 : (stage == 2 ? a.gate2 : a.gate3);
        bool active = stage == 1 ? (before == TK_TRACKED || before == TK_LOST)
                                 : (stage == 2 ? (before == TK_TRACKED && !matched) : before == TK_TENTATIVE);
        if constexpr (APP) tact[t] = active ? (fvalid ? 3 : 1) : 0;      // (bit 1: the track has a feature, for the rows' scans)
        else tact[t] = active ? 1 : 0;
        // stage 2 is IoU alone, as published; a track without a feature never reads S
        [[maybe_unused]] const bool fuse = APP && stage != 2 && fvalid;
        for (int j = t; j < n; j += TK_NT) {
            dprop[j] = -2;                                            // not looked at yet in this stage
            dkey[j] = 0ull;
        }
        __syncthreads();
        const float4 mybox = tbox[t];
        // Within a stage the free sets only shrink, so a side's best partner stays its best until somebody else takes it: a track scans again
        // only when its detection is gone, a detection only when its track is (and none at all once a scan found nobody).
        // The first scan of a stage sees every admissible pair of the stage, so it also leaves every row its best track: an integer maximum
        // in LDS over (IoU bits, ~slot) -- an admissible IoU is a positive float, whose bits order like its value -- and the order of the
        // atomics does not matter to a maximum. A row scans the slots itself only when that track has been taken.
        int bj = -1;
        bool scanned = false;
        for (;;) {
            if (active && (!scanned || (bj >= 0 && dcls[bj] != cls))) {
                float bu = gate;
                const bool first = !scanned;
                bj = -1;
                scanned = true;
                // TK_SCAN rows per step, their LDS reads in flight together (one dependent read per row made this loop wait for LDS, not compute);
                // a taken row has lost its class. j0 + k <= 511: the arrays are TK_MAX_D long and the rows at or beyond n have no class.
                for (int j0 = 0; j0 < n; j0 += TK_SCAN) {
                    int c[TK_SCAN];
                    bool any = false;
#pragma unroll
                    for (int k = 0; k < TK_SCAN; ++k) {
                        c[k] = dcls[j0 + k];
                        any = any || c[k] == cls;
                    }
                    if (!any) continue;                               // (uniform)
                    long long l[TK_SCAN];
                    float4 bx[TK_SCAN];
#pragma unroll
                    for (int k = 0; k < TK_SCAN; ++k) {
                        l[k] = dlab[j0 + k];
                        bx[k] = dbox[j0 + k];
                    }
                    // the track's own row of S, 8 consecutive floats, requested together with the LDS reads (the index is clamped: the row
                    // holds d entries); only a track with a feature reads them, and only for the rows that have one
                    [[maybe_unused]] float sv[TK_SCAN];
                    [[maybe_unused]] bool fe[TK_SCAN];
                    if constexpr (APP) {
#pragma unroll
                        for (int k = 0; k < TK_SCAN; ++k) {
                            fe[k] = fuse && dfeat[j0 + k] != 0;
                            sv[k] = 0.0f;
                        }
                        if (fuse) {
#pragma unroll
                            for (int k = 0; k < TK_SCAN; ++k) sv[k] = srow[j0 + k < d ? j0 + k : d - 1];
                        }
                    }
#pragma unroll
                    for (int k = 0; k < TK_SCAN; ++k)
                        if (c[k] == cls && (agn || l[k] == label)) {
                            float u;
                            if constexpr (APP) u = fe[k] ? tk_fused(mybox, bx[k], sv[k], p.app_thresh, p.prox_thresh) : tk_iou(mybox, bx[k]);
                            else u = tk_iou(mybox, bx[k]);
                            if (first && u > gate)
                                atomicMax(&dkey[j0 + k], ((unsigned long long)__float_as_uint(u) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)t));
                            if (u > bu) { bu = u; bj = j0 + k; }
                        }
                }
            }
            const bool propose = active && bj >= 0;
            if (propose) dhas[bj] = 1;
            if (!__syncthreads_or(propose)) break;
            for (int j = t; j < n; j += TK_NT) {
                if (!dhas[j]) continue;
                dhas[j] = 0;
                int bs = dprop[j];
                if (bs == -2) {
                    const unsigned long long key = dkey[j];
                    bs = key ? (int)(0xFFFFFFFFu - (unsigned)key) : -1;
                    dprop[j] = bs;
                }
                if (bs >= 0 && !tact[bs]) {
                    const float4 bx = dbox[j];
                    const long long lb = dlab[j];
                    float du = gate;
                    bs = -1;
                    for (int s0 = 0; s0 < T; s0 += TK_SCAN) {         // (s0 + k <= 255; the slots at or beyond T are never active)
                        int c[TK_SCAN];
                        bool any = false;
#pragma unroll
                        for (int k = 0; k < TK_SCAN; ++k) {
                            c[k] = tact[s0 + k];
                            any = any || c[k] != 0;
                        }
                        if (!any) continue;                           // (uniform)
                        long long l[TK_SCAN];
                        float4 tb[TK_SCAN];
#pragma unroll
                        for (int k = 0; k < TK_SCAN; ++k) {
                            l[k] = tlab[s0 + k];
                            tb[k] = tbox[s0 + k];
                        }
                        // the row's column of S: one float per slot, d floats apart (a row scans only after losing its best track)
                        [[maybe_unused]] float sv[TK_SCAN];
                        [[maybe_unused]] bool fe[TK_SCAN];
                        if constexpr (APP) {
                            const bool rfuse = stage != 2 && dfeat[j] != 0;
#pragma unroll
                            for (int k = 0; k < TK_SCAN; ++k) {
                                fe[k] = rfuse && (c[k] & 2) != 0;
                                sv[k] = fe[k] ? p.S[((size_t)b * Tp + (s0 + k)) * d + j] : 0.0f;      // (an active slot is < T <= Tp)
                            }
                        }
#pragma unroll
                        for (int k = 0; k < TK_SCAN; ++k)
                            if (c[k] != 0 && (agn || l[k] == lb)) {
                                float u;
                                if constexpr (APP) u = fe[k] ? tk_fused(tb[k], bx, sv[k], p.app_thresh, p.prox_thresh) : tk_iou(tb[k], bx);
                                else u = tk_iou(tb[k], bx);
                                if (u > du) { du = u; bs = s0 + k; }
                            }
                    }
                    dprop[j] = bs;
                }
            }
            __syncthreads();
            if (propose && dprop[bj] == t) {
                // 4. - 6. a match: the filter takes the measurement; a lost or tentative track becomes tracked and keeps its id
                tk_update(f, dbox[bj]);
                score = dscore[bj];
                state = TK_TRACKED;
                last = frame;
                det = bj;
                matched = true;
                active = false;
                tact[t] = 0;
                did[bj] = id;
                dcls[bj] = TK_NONE;
                if constexpr (APP) fop = dfeat[bj] ? (TK_F_EMA | (bj << 2)) : TK_F_NONE;
            }
            __syncthreads();
        }
        if (stage == 2 && before == TK_TRACKED && !matched) state = TK_LOST;
        if (stage == 3 && before == TK_TENTATIVE && !matched) {
            state = TK_FREE;
            if constexpr (APP) fop = TK_F_CLEAR;
        }
    }

    // 7. new tracks: the r-th remaining high detection with score >= new_thresh, in row order, takes the r-th free slot, in slot order
    int nnew = 0, r0, r1, tot;
    const int j1 = t + TK_NT;
    const bool s0 = t < n && dcls[t] == TK_HIGH && dscore[t] >= a.new_thresh;
    const bool s1 = j1 < n && dcls[j1] == TK_HIGH && dscore[j1] >= a.new_thresh;
    r0 = tk_scan(s0, wtot, tot);
    nnew = tot;
    r1 = nnew + tk_scan(s1, wtot, tot);
    nnew += tot;
    int nfree;
    const int fr = tk_scan(slot && state == TK_FREE, wtot, nfree);
    if (s0 && r0 < TK_NT) detlist[r0] = t;
    if (s1 && r1 < TK_NT) detlist[r1] = j1;
    const bool confirm_now = frame == 1;
    if (s0 && r0 < nfree) did[t] = confirm_now ? next_id + r0 : -1;
    if (s1 && r1 < nfree) did[j1] = confirm_now ? next_id + r1 : -1;
    __syncthreads();
    const int started = nnew < nfree ? nnew : nfree;
    if (slot && state == TK_FREE) {
        if (fr < started) {
            const int j = detlist[fr];
            tk_init(f, dbox[j]);
            state = confirm_now ? TK_TRACKED : TK_TENTATIVE;
            id = next_id + fr;
            label = dlab[j];
            score = dscore[j];
            start = frame;
            last = frame;
            det = j;
            if constexpr (APP) fop = dfeat[j] ? (TK_F_INIT | (j << 2)) : TK_F_CLEAR;
        } else {
            id = 0; label = 0; score = 0.0f; start = 0; last = 0; det = 0;
#pragma unroll
            for (int i = 0; i < 20; ++i) f[i] = 0.0f;
        }
    }
    dropped += nnew - started;

    // 8. a lost track that has not been seen for more than track_buffer frames is removed
    if (state == TK_LOST && frame - last > a.track_buffer) {
        state = TK_FREE;
        if constexpr (APP) fop = TK_F_CLEAR;
        id = 0; label = 0; score = 0.0f; start = 0; last = 0; det = 0;
#pragma unroll
        for (int i = 0; i < 20; ++i) f[i] = 0.0f;
    }

    // 9. outputs: the confirmed tracks updated in this frame, in slot order
    const bool out = state == TK_TRACKED && last == frame;
    int nout;
    const int orank = tk_scan(out, wtot, nout);
    if (out) {
        const size_t o = (size_t)b * T + orank;
        a.boxes_out[o] = tk_box(f);
        a.scores_out[o] = score;
        a.labels_out[o] = label;
        a.ids_out[o] = id;
        a.det_out[o] = det;
    }
    if (slot && t >= nout) {
        const size_t o = (size_t)b * T + t;
        a.boxes_out[o] = make_float4(0.f, 0.f, 0.f, 0.f);
        a.scores_out[o] = 0.0f;
        a.labels_out[o] = 0;
        a.ids_out[o] = 0;
        a.det_out[o] = -1;
    }
    if (t == 0) a.counts_out[b] = nout;
    for (int j = t; j < d; j += TK_NT) a.det_ids_out[(size_t)b * d + j] = j < n ? (long long)did[j] : -1ll;
    if constexpr (APP) detlist[t] = fop;       // (detlist was last read in step 7; the scan of step 9 has barriers behind that)

    // the state goes back through LDS
    if (slot) {
        sti[oState + t] = state;
        sti[oId + t] = id;
        reinterpret_cast<long long*>(sti + oLabel)[t] = label;
        stf[oScore + t] = score;
#pragma unroll
        for (int i = 0; i < 20; ++i) stf[oFilt + i * Tp + t] = f[i];
        sti[oStart + t] = start;
        sti[oLast + t] = last;
        sti[oDet + t] = det;
    }
    if (t == 0) {
        sti[0] = frame;
        sti[1] = next_id + started;
        sti[2] = dropped;
    }
    __syncthreads();
    for (int i = t; i < words / 4; i += TK_NT) gstate[i] = st4[i];

    // the features: a wave per slot, lanes over dim (at most 8 values a lane). A start takes float(en[row]); a match with a row that has an
    // embedding takes s = alpha s + (1 - alpha) float(en[row]), s /= |s| (a plain start if the slot had no feature); a freed slot loses its flag.
    // The sum of squares is a lane's values in ascending k, then a butterfly over the wave: the same bits on every run, no atomics.
    if constexpr (APP) {
        const int lane = t & 63, wave = t >> 6;
        int32_t* const fl = p.fflag + (size_t)b * (Tp + (size_t)Tp * p.dim);
        float* const fv = reinterpret_cast<float*>(fl + Tp);
        for (int s = wave; s < T; s += TK_WAVES) {
            const int op = detlist[s], kind = op & 3;                   // (uniform over the wave)
            if (kind == TK_F_NONE) continue;
            if (kind == TK_F_CLEAR) {
                if (lane == 0) fl[s] = 0;
                continue;
            }
            const half_t* const x = p.en + (size_t)p.map[(size_t)b * d + (op >> 2)] * p.dim;      // (the row has an embedding: its slot is >= 0)
            float* const fs = fv + (size_t)s * p.dim;
            const bool ema = kind == TK_F_EMA && fl[s] != 0;
            float v[8];
            float ss = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int k = lane + 64 * i;
                v[i] = 0.0f;
                if (k < p.dim) {
                    const float xf = (float)x[k];
                    v[i] = ema ? p.alpha * fs[k] + p.beta * xf : xf;
                    ss += v[i] * v[i];
                }
            }
            bool ok = true;
            if (ema) {
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m);
                const float nrm = sqrtf(ss);
                ok = nrm > 0.0f && nrm < INFINITY;                      // (a NaN compares false)
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = v[i] / nrm;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int k = lane + 64 * i;
                if (k < p.dim) fs[k] = v[i];
            }
            if (lane == 0) fl[s] = ok ? 1 : 0;
        }
    }
