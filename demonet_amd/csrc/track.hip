// Multi-object tracking on the device: dn_track_update is ByteTrack's BYTETracker.update (Zhang et al. 2022) with its constant-velocity
// Kalman filter for B independent streams in ONE launch per frame step; dn_track_reset restarts streams. The semantics, sentence by sentence, are
// in include/demonet_hip.h and restated in tests/track_ref.py; this file must agree with them bit for bit.
// The frame step itself lives in trackstep.inc and its helpers in trackcore.h, which trackapp.hip shares; how the kernel works is described there.
// Compiled with -ffp-contract=off: every operation of the header's text rounds once.
#include "trackcore.h"

namespace {

__global__ __launch_bounds__(TK_NT) void track_update_kernel(const TrackArgs a) {
    constexpr bool APP = false;
    const TrackAppArgs p{};                    // (never read: trackstep.inc)
    unsigned char* const dfeat = nullptr;
#include "trackstep.inc"
}

// one workgroup per stream: the selected streams restart at frame 0 with an empty table and next_id = 1
__global__ __launch_bounds__(TK_NT) void track_reset_kernel(uint4* __restrict__ state, const uint8_t* __restrict__ which, int words4) {
    const int b = blockIdx.x;
    if (which && which[b] == 0) return;
    uint4* const g = state + (size_t)b * words4;
    for (int i = threadIdx.x; i < words4; i += TK_NT) g[i] = i == 0 ? make_uint4(0u, 1u, 0u, 0u) : make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace

extern "C" __attribute__((visibility("default"))) size_t dn_track_state_bytes(int streams, int max_tracks) {
    if (streams < 1 || max_tracks < 1 || max_tracks > TK_NT) return 0;
    return (size_t)streams * tk_stream_words(max_tracks) * 4;
}

extern "C" __attribute__((visibility("default"))) int dn_track_reset(void* state, int streams, int max_tracks, const uint8_t* which, void* stream) {
    DN_REQUIRE(state, "dn_track_reset: null state");
    DN_REQUIRE(streams >= 1 && max_tracks >= 1, "dn_track_reset: bad sizes streams=%d max_tracks=%d", streams, max_tracks);
    DN_REQUIRE((reinterpret_cast<size_t>(state) & 15) == 0, "dn_track_reset: the state must be 16-byte aligned");
    if (max_tracks > TK_NT) {
        dn_set_error("dn_track_reset: max_tracks=%d, at most %d", max_tracks, TK_NT);
        return DN_E_UNSUPPORTED;
    }
    dn_note_kernel("track_reset_kernel");
    hipLaunchKernelGGL(track_reset_kernel, dim3(streams), dim3(TK_NT), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<uint4*>(state), which,
                       (int)(tk_stream_words(max_tracks) / 4));
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}

extern "C" __attribute__((visibility("default"))) int dn_track_update(const float* boxes, const float* scores, const int64_t* labels,
                                                                     const int32_t* counts, int streams, int d, const dn_track_params* params,
                                                                     void* state, size_t state_bytes, float* boxes_out, float* scores_out,
                                                                     int64_t* labels_out, int64_t* ids_out, int32_t* det_out, int32_t* counts_out,
                                                                     int64_t* det_ids_out, void* stream) {
    TrackArgs a;
    const int rc = tk_check_step("dn_track_update", boxes, scores, labels, counts, streams, d, params, state, state_bytes, boxes_out, scores_out,
                                 labels_out, ids_out, det_out, counts_out, det_ids_out, a);
    if (rc != DN_OK) return rc;
    dn_note_kernel("track_update_kernel");
    hipLaunchKernelGGL(track_update_kernel, dim3(streams), dim3(TK_NT), 0, reinterpret_cast<hipStream_t>(stream), a);
    DN_HIP_CHECK(hipGetLastError());
    return DN_OK;
}
