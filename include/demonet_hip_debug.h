/* Test-support entry points of libdemonet_hip.so that are NOT part of the drop-in boundary (include/demonet_hip.h).
 * The product library exports exactly these eight beside the boundary; everything else named dn_debug_* (phase stamps,
 * tile forcing) exists only in the dev build (python -m demonet_amd.build --stamps, -DDN_DEV_STAMPS).               */
#ifndef DEMONET_HIP_DEBUG_H
#define DEMONET_HIP_DEBUG_H

#include "demonet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Number of head_fused_kernel launches issued by this process so far (tests assert that the fused path was taken). */
DN_API int dn_debug_head_fused_launches(void);

/* ... and how many of them carried the softmax / decode epilogue (scores, boxes and histogram rows instead of logits). */
DN_API int dn_debug_head_softmax_launches(void);

/* Drops the plan's cached hipGraph executables (tests re-capture with other DN_* knobs in one process). 0 on success. */
DN_API int dn_debug_clear_graphs(dn_plan* plan);

/* Where the forwards of an n-image layout leave the network's input after a resize or a uint8 conversion: the [n][3][image_h][image_w]
 * fp32 block and the [n][2] (w ratio, h ratio) block that maps boxes back to the caller's image size. Both are contiguous over the
 * sub-batch chains of the forward. Valid for the workspace of the last forward of n images. 0 on success. */
DN_API int dn_debug_network_input(const dn_plan* plan, void* workspace_dev, int n, float** resized_dev, float** scale_xy_dev);

/* Label of the kernel that the last launcher call on this thread enqueued (the names of dn_profile_op_info), copied into buf. A stand-alone
 * entry point (dn_pointwise_conv, dn_dense_conv, ...) can so be asked which kernel it took. 0 on success. */
DN_API int dn_debug_last_kernel(char* buf, int capacity);

/* 3 x 3 "same" convolution + MaxPool2d(2, 2) in one launch, as the plan issues it for a fused conv / pool pair: x [n][h][w][cin] fp16,
 * w [cout][3][3][cin] fp16, pool_out [n][h/2][w/2][cout] fp16; out (optional) also receives the full-resolution map [n][h][w][cout].
 * A batch beyond the run-staged tile's 2 GB of input goes out in image ranges, one launch each. 0 on success. */
DN_API int dn_debug_conv_pool(const void* x_dev, const void* w_dev, const float* bias_dev, const void* zeros_dev, void* pool_out_dev, void* out_dev,
                              int n, int h, int w, int cin, int cout, int act, void* stream);

/* launch_stem on its own (3 x 3): image [n][3][h][w] fp32 in [0, 1], w [27][cout] fp32 with tap index (c 3 + ky) 3 + kx, out [n][ho][wo][cout] fp16,
 * mean3 / std3 on the host. split_ok / scale_log2: what dn_create derives from the weights -- all finite, and the largest magnitude of weights and
 * bias times 2^scale_log2 lies in [2^14, 2^15); split_ok = 0 keeps the split-operand kernel out. 0 on success. */
DN_API int dn_debug_stem(const float* img_dev, const float* w_dev, const float* bias_dev, void* out_dev, int n, int h, int w, int cout, int stride, int pad, int act,
                         const float* mean3, const float* std3, int split_ok, int scale_log2, void* stream);

/* Host only (no GPU needed): what the kernel-choice functions answer for a shape, as text ("kernel=... tile=.. fk=.. halo=.. ...").
 * family and the int64 entries of dims:
 *   "pw"        m cin cout hw act out_fp32 se residual wfrag (the last three: 0 / 1, is the array given)
 *   "pw_group"  conv count, then count x (m cin cout hw)
 *   "conv"      n h w cin cout k stride pad dil act zeros use cout_b     (use: 0 plain, 1 with the max-pool, 2 fp32 head; a 1x1 that the
 *               pointwise family serves is answered by that family)
 *   "dw"        n h w c k stride pad        (range=: inside the kernel's index range; wlds=: LDS bytes of the weight image, 0 = per-thread loads)
 *   "stem"      n h w cout stride pad act split_ok
 *   "headfuse"  n H W C nc0 nc1 out_img_stride0 out_img_stride1     (supported=: the level may join the fused head launch)
 *   "headpost"  n H W anchors_per_location K A                      (supported=: the level's workgroups may run the softmax / decode epilogue)
 *   "patch_blocks" n h w        (blocks=: 16 x 16 blocks of a conv_patch_resident_kernel launch; launched=: below the launcher's limit)
 *   "expdw"     n h w cin cexp cout k stride act1 act2 has_res pool     (expdw_choose's answer, the function launch_expdw asks. cout 0: no project
 *               stage; act1 -1: no expand stage. body=direct: the per-tap body of expdw_direct.hip takes the launch, band= its output rows per
 *               workgroup; body=rows: the row-reuse body of expdw_rows.hip, band= its output rows per wave; body=tiled: the bodies of expdw.hip;
 *               body=none: no body takes it; label= what the launch notes, whichever body runs; tile= the output tile <oh>x<ow> of the tiled
 *               bodies; reads DN_EXPDW_DIRECT / DN_EXPDW_DIRECT_BAND / DN_EXPDW_ROWS / DN_EXPDW_ROWS_BAND / DN_EXPDW_PERSIST / DN_EXPDW_ONE)
 *   "expdw_whole" the same twelve numbers      (a flag of body=tiled that "expdw" does not show: whole= the phases are walked once over the whole
 *               expanded width, expdw_whole.hip; lds= that form's LDS bytes, 0 without it; reads DN_EXPDW_WHOLE beside the knobs above)
 * 0 on success. */
DN_API int dn_debug_choice(const char* family, const int64_t* dims, int ndims, char* buf, int capacity);

#ifdef __cplusplus
}
#endif
#endif
