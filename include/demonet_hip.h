/* demonet_hip.h -- C ABI of the MI355X (gfx950) SSD inference library.
 *
 * The reference (zhiqwang/demonet) has no FFI/operator layer: its seam is the Python factory ->
 * nn.Module.forward contract (demonet/models/generalized_ssd.py:271-349). This header is the native
 * boundary a maintainer binds instead of calling `SSD.forward` (see INTEGRATION.md for the ctypes stub):
 * plain pointers and sizes only, no torch types. All `*_dev` pointers are device (HBM) pointers owned by
 * the caller; the library owns the plan and its weight arena. No entry point below allocates device
 * memory or synchronises the device except dn_create / dn_destroy.
 *
 * Every function returns 0 on success, a negative DN_E_* code on failure; dn_last_error() gives the text.
 */
#ifndef DEMONET_HIP_H
#define DEMONET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DN_ABI_VERSION 1
/* Largest num_classes (background included) dn_create, dn_forward* and dn_postprocess accept: LVIS v1 (1 204), OpenImages (601) and
 * Objects365 (366) fit. Above it they return DN_E_UNSUPPORTED. */
#define DN_MAX_CLASSES 2048
#define DN_API __attribute__((visibility("default")))

enum { DN_OK = 0, DN_E_INVALID = -1, DN_E_HIP = -2, DN_E_WORKSPACE = -3, DN_E_UNSUPPORTED = -4 };

/* activation fused behind a convolution (reference: mobilenetv3.py:72, ssd_mobilenetv3.py:31,41) */
enum { DN_ACT_NONE = 0, DN_ACT_RELU = 1, DN_ACT_RELU6 = 2, DN_ACT_HSWISH = 3 };

/* op kinds of the lowered graph (demonet_amd/spec.py IR) */
enum { DN_OP_STEM = 1, DN_OP_PW = 2, DN_OP_DW = 3, DN_OP_SE = 4, DN_OP_CONV = 5, DN_OP_MAXPOOL = 6, DN_OP_L2NORM = 7 };

/* tensor kinds: NHWC fp16 activation | NCHW fp32 image | per-image fp32 vector [c] | fp32 pooled partial sums [blocks][c] */
enum { DN_T_ACT = 0, DN_T_IMAGE = 1, DN_T_VEC = 2, DN_T_POOL = 3 };

typedef struct dn_tensor_desc {
    int32_t c, h, w, kind;
} dn_tensor_desc;

typedef struct dn_op_desc {
    int32_t type;                       /* DN_OP_* */
    int32_t in, out;                    /* tensor ids */
    int32_t residual;                   /* PW: tensor added after BN (mobilenetv3.py:97-98); -1 none */
    int32_t se;                         /* PW: DN_T_VEC tensor scaling the input channels per image; -1 none */
    int32_t pool;                       /* DW: DN_T_POOL tensor receiving per-(image,channel) sums; -1 none */
    int32_t cin, cout, k, stride, pad, dil, act;
    int32_t head;                       /* 0 none, 1 class logits, 2 box regression: write fp32 into the head arrays */
    int32_t level;                      /* pyramid level of a head op */
    int32_t squeeze;                    /* SE: squeeze width; pooled pixel count is taken from the producer */
    int32_t ceil_mode;                  /* MAXPOOL */
    int32_t pool_pixels;                /* SE: H*W of the pooled map (mean divisor) */
    int32_t reserved[2];
    int64_t w_off, b_off, w2_off, b2_off;   /* byte offsets into the weight blob; -1 none.
                                               PW/CONV: w = fp16 [cout][k*k*cin] (tap-major, channel-minor), b = fp32 [cout]
                                               PW (optional): w2 = the same weights in MFMA-fragment order
                                                 [ceil(cout/32)][ceil(cin/16)][2 k-halves][32 channels][8] fp16, zero beyond cout / cin; -1: none
                                               DW/STEM: w = fp16 [k*k][c] / fp32 [k*k*3][cout], b = fp32 [c]
                                               SE: w = fp16 fc1 weight TRANSPOSED [c][squeeze], b = fp32 fc1 bias, w2 = fp16 fc2 weight TRANSPOSED [squeeze][c], b2 = fp32 fc2 bias (c, squeeze even)
                                               L2NORM: w = fp32 scale [c] */
} dn_op_desc;

typedef struct dn_model_desc {
    int32_t abi_version;                /* DN_ABI_VERSION */
    int32_t n_tensors, n_ops;
    const dn_tensor_desc* tensors;
    const dn_op_desc* ops;
    int32_t input_tensor;
    int32_t image_h, image_w;           /* fixed network input size (generalized_ssd.py:190-191) */
    float mean[3], std[3];              /* transform.py:129-138 */
    int32_t num_classes;                /* including background class 0; 2 .. DN_MAX_CLASSES (dn_create returns DN_E_UNSUPPORTED above) */
    int32_t n_levels;
    int32_t level_tensor[8];            /* feature-map tensor id per pyramid level */
    int32_t anchors_per_loc[8];
    int32_t num_anchors;
    const float* anchors;               /* host, [num_anchors][4] xyxy pixels (anchor_utils.py:111-126) */
    float score_thresh, nms_thresh;     /* generalized_ssd.py:158-162 */
    int32_t detections_per_img, topk_candidates;
} dn_model_desc;

typedef struct dn_plan dn_plan;

/* Build a plan: validates the graph, uploads `weights` (host blob addressed by the op offsets) and anchors. */
DN_API int dn_create(const dn_model_desc* desc, const void* weights, size_t weight_bytes, dn_plan** out);
DN_API void dn_destroy(dn_plan* plan);

/* Bytes of caller-provided device scratch needed for a batch of n images. */
DN_API size_t dn_workspace_bytes(const dn_plan* plan, int n);

/* The whole hot path, replacing SSD.forward (eval):  images_dev = [n][3][h][w] fp32 in [0,1], NCHW, contiguous
 * (the stacked form of the reference's List[Tensor[3,H,W]]); (h, w) may differ from the network size, in which
 * case the bilinear resize of transform.py:27-53 runs first and boxes are mapped back (transform.py:278-292).
 * Outputs (device): boxes [n][D][4] fp32 xyxy, scores [n][D] fp32, labels [n][D] int64, counts [n] int32, with
 * D = detections_per_img; rows >= counts[i] are zero. Asynchronous on `stream` (a hipStream_t). */
DN_API int dn_forward(dn_plan* plan, const float* images_dev, int n, int h, int w,
               float* boxes_dev, float* scores_dev, int64_t* labels_dev, int32_t* counts_dev,
               void* workspace_dev, size_t workspace_bytes, void* stream);

/* The same with the decoder's output as input -- the step just before the path: images_dev = [n][h][w][3] uint8, HWC,
 * RGB. x/255 (ToTensor), the bilinear resize of transform.py:27-53 and the HWC -> planar conversion run as one pass ahead of the
 * stem (which normalises on load); results are identical to dn_forward on float(images)/255 in NCHW.
 * Like dn_forward, one plan serves one host thread at a time (the plan's graph cache and its stored dn_set_packed_output setting). */
DN_API int dn_forward_u8(dn_plan* plan, const uint8_t* images_dev, int n, int h, int w,
                  float* boxes_dev, float* scores_dev, int64_t* labels_dev, int32_t* counts_dev,
                  void* workspace_dev, size_t workspace_bytes, void* stream);

/* The same with video surfaces as input, as decoders hand them out: one record per image, every image with its own allocation(s), row
 * pitches and SIZE (720p and 1080p cameras mix in one batch). Each bilinear tap of the resize is converted to 8-bit RGB as it is read, in
 * integer arithmetic fixed here; from there on the arithmetic is dn_forward_u8's, so the network input equals, bit for bit, what dn_forward_u8
 * computes from the frame converted by these formulas. With y = Y - yo, u = U - 128, v = V - 128:
 *     R = clamp((cy y + crv v + 2^13) >> 14),  G = clamp((cy y - cgu u - cgv v + 2^13) >> 14),  B = clamp((cy y + cbu u + 2^13) >> 14)
 * (>> arithmetic, i.e. floor; clamp to 0 .. 255), every coefficient round(c 2^14) of cy = 255/219, crv = 2(1 - Kr) cs, cbu = 2(1 - Kb) cs,
 * cgu = 2 Kb (1 - Kb) / Kg cs, cgv = 2 Kr (1 - Kr) / Kg cs, with cs = 255/224 and yo = 16 for limited range (16..235 / 16..240) and
 * cy = cs = 1, yo = 0 for full range; BT.601: Kr, Kb = 0.299, 0.114, BT.709: 0.2126, 0.0722 (Kg = 1 - Kr - Kb).
 * Chroma is NOT interpolated: the chroma sample of pixel (x, y) is (x >> 1, y >> 1), nearest replication as the common fast converters do.
 * DN_FRAME_RGB24 / DN_FRAME_BGR24 skip the conversion (`color` is still checked). */
enum { DN_FRAME_NV12 = 0, DN_FRAME_I420 = 1, DN_FRAME_RGB24 = 2, DN_FRAME_BGR24 = 3 };
enum { DN_COLOR_BT601 = 0, DN_COLOR_BT709 = 1, DN_COLOR_FULL_RANGE = 0x10 };      /* matrix | DN_COLOR_FULL_RANGE: full range; otherwise limited */
typedef struct dn_frame {                                  /* 48 bytes, one per image, in DEVICE memory */
    const uint8_t* plane[3];   /* NV12: Y, interleaved UV, unused; I420: Y, U, V; RGB24/BGR24: packed pixels, unused, unused */
    int32_t pitch[3];          /* bytes per row of each plane (>= the row's payload) */
    int32_t width, height;     /* of THIS frame; chroma planes are ceil(height/2) rows of ceil(width/2) samples */
    int32_t reserved;
} dn_frame;
/* frames_dev = [n] records in device memory, read by the first kernel of the forward WHEN IT RUNS: a captured graph is keyed on the table's
 * address (with n, format, color and the output pointers) and replays on whatever surfaces the table names at that moment -- putting a new
 * frame into the table (an ordinary copy on `stream` ahead of the call) needs no recapture. Outputs and asynchrony are dn_forward's; boxes
 * come back in each frame's own pixel coordinates.
 * TRUST BOUNDARY: the library cannot inspect a device table. It trusts every record: plane pointers valid for pitch * rows bytes, pitches
 * and sizes positive; a wrong record is an out-of-bounds device read. Validate on the host before the records go up (Python: FrameBatch.set).
 * DN_E_INVALID for a null table or n <= 0, DN_E_UNSUPPORTED for an unknown format or colour code. */
DN_API int dn_forward_frames(dn_plan* plan, const dn_frame* frames_dev, int n, int format, int color,
                      float* boxes_dev, float* scores_dev, int64_t* labels_dev, int32_t* counts_dev,
                      void* workspace_dev, size_t workspace_bytes, void* stream);

/* The same with REGIONS of video surfaces as input: network image i is a rectangle of one of the frames, optionally mirrored -- the tiles of
 * sliced inference and the two passes of flip test-time augmentation straight from the surfaces, tiles and whole-frame passes of several
 * cameras in one forward. frames_dev is a dn_frame table as above (any number of records); regions_dev = [n] records, one per network image.
 * Arithmetic: with r = regions[i], f = frames[r.frame], h = r.height, w = r.width, the quantities rh, rw, sy, sx, y0, x0, y1, x1, ly, lx are
 * dn_forward_u8's, expression for expression, IN REGION COORDINATES: the second tap clamps at the region's last row and column
 * (x0 < w - 1), not the frame's. A tap at region pixel (xr, yr) reads frame pixel X = r.x0 + (HFLIP ? w - 1 - xr : xr), Y = r.y0 + yr, converted
 * as above -- so its chroma sample is (X >> 1, Y >> 1) in FRAME coordinates -- then /255 and the bilinear weights without contraction. The
 * ratio of image i is (w / ow, h / oh) of the region. Consequence: the network input of image i equals, bit for bit, what dn_forward_u8
 * computes from the rectangle cut out of the converted frame (mirrored left-right when flagged); a region (f, 0, 0, W, H, 0) reproduces
 * dn_forward_frames. A region of exactly the network size has weights (1, 0): the kernel then reads one tap, with the same bits.
 * Boxes come back in the region's own coordinates; for a mirrored region these are the MIRRORED region's, the caller maps x1' = w - x2,
 * x2' = w - x1. */
enum { DN_REGION_HFLIP = 1 };
typedef struct dn_region {      /* 32 bytes, one per network image, in DEVICE memory */
    int32_t frame;              /* index into the dn_frame table */
    int32_t x0, y0, width, height;   /* the rectangle, in that frame's pixels; wholly inside the frame */
    int32_t flags;              /* 0 or DN_REGION_HFLIP */
    int32_t reserved[2];        /* 0 */
} dn_region;
/* Both tables are read by the first kernel of the forward WHEN IT RUNS: a captured graph is keyed on both addresses (with n, format, color
 * and the output pointers) and replays on whatever surfaces and rectangles they name at that moment. A forward that runs as several
 * sub-batch chains advances the REGION table by the chain's first image; every chain indexes the same frame table.
 * TRUST BOUNDARY: AS FOR dn_frame, THE LIBRARY CANNOT INSPECT A DEVICE TABLE AND TRUSTS BOTH: every region's frame index inside the frame
 * table, width, height >= 1, x0, y0 >= 0, x0 + width <= that frame's width, y0 + height <= its height; a wrong record is an out-of-bounds
 * device read. Validate on the host before the records go up (Python: frames.RegionTable.set, SSD.forward_regions).
 * DN_E_INVALID for a null table or n <= 0, DN_E_UNSUPPORTED for an unknown format or colour code, both before anything is launched. */
DN_API int dn_forward_regions(dn_plan* plan, const dn_frame* frames_dev, const dn_region* regions_dev, int n, int format, int color,
                       float* boxes_dev, float* scores_dev, int64_t* labels_dev, int32_t* counts_dev,
                       void* workspace_dev, size_t workspace_bytes, void* stream);

/* Backbone + heads only (no post-process). The head outputs live inside the workspace; query them with
 * dn_head_outputs:  cls_logits [n][A][K] fp32, bbox_regression [n][A][4] fp32 (generalized_ssd.py:60-74). Valid after
 * dn_forward_heads only: dn_forward may compute softmax / box decode inside the head launch and then never writes the logits
 * of the large pyramid levels -- dn_head_outputs returns DN_E_INVALID for a workspace whose last forward was dn_forward. */
DN_API int dn_forward_heads(dn_plan* plan, const float* images_dev, int n, int h, int w,
                     void* workspace_dev, size_t workspace_bytes, void* stream);
DN_API int dn_head_outputs(const dn_plan* plan, void* workspace_dev, int n, float** cls_logits_dev, float** bbox_regression_dev);
/* Device address/size of an intermediate tensor inside the workspace (parity tests on feature maps). */
DN_API int dn_tensor_ptr(const dn_plan* plan, void* workspace_dev, int n, int tensor_id, void** ptr, size_t* bytes);

/* The level feature maps of the last forward on this workspace, for callers that continue from them (the head backward below).
 * A forward of n images runs as dn_batch_split(plan, n) sub-batch chains, each with an arena of its own, so a level tensor is one
 * contiguous [images][h][w][c] fp16 NHWC piece PER CHAIN: *ptr = the piece of chain `chain` (0 .. dn_batch_split - 1), *first_image =
 * index of its first image in the batch, *images = its image count (either may be NULL). The pieces stay valid until the next forward
 * on the workspace. dn_tensor_ptr serves the single-chain case only. */
DN_API int dn_level_features(const dn_plan* plan, void* workspace_dev, int n, int level, int chain, void** ptr, int* first_image, int* images);
/* Backbone only: dn_forward_heads without its head launches -- the same launch list, stopped in front of them; ends with the level
 * tensors (dn_level_features) complete. The head arrays of the workspace are not written (dn_head_outputs refuses). For a training
 * step that computes the heads from its own, current weights. Not available while profiling. */
DN_API int dn_forward_features(dn_plan* plan, const float* images_dev, int n, int h, int w,
                               void* workspace_dev, size_t workspace_bytes, void* stream);

/* Post-process only, replacing SSD.postprocess_detections (generalized_ssd.py:351-397) + transform.postprocess:
 * softmax -> decode (BoxCoder weights 10,10,5,5) -> clip -> per-class score>thr & top-k -> hard NMS (IoU > thr)
 * -> global top-D by score.  kept_anchor_dev (optional, may be NULL): [n][D] int32 anchor index per detection.
 * num_classes (background included) 2 .. DN_MAX_CLASSES: DN_E_UNSUPPORTED above; topk_candidates and detections_per_img 1 .. 512.
 * score_thresh >= 0: dn_postprocess and dn_postprocess_soft return DN_E_INVALID for a negative threshold, and dn_create refuses a plan with
 * one. The reference keeps a score that underflowed to exactly 0.0 under a negative threshold; here a zero score never is a candidate (its
 * key, 0, means "not passing"), and a threshold of 0 already keeps every positive score. */
DN_API size_t dn_postprocess_workspace_bytes(int n, int num_anchors, int num_classes, int topk_candidates, int detections_per_img);
DN_API int dn_postprocess(const float* cls_logits_dev, const float* bbox_regression_dev, const float* anchors_dev,
                   int n, int num_anchors, int num_classes,
                   float image_h, float image_w, const float* scale_xy_dev /* [n][2] (w,h) ratios or NULL */,
                   float score_thresh, float nms_thresh, int topk_candidates, int detections_per_img,
                   float* boxes_dev, float* scores_dev, int64_t* labels_dev, int32_t* counts_dev,
                   int32_t* kept_anchor_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Soft-NMS (Bodla et al., 2017) as the per-class reduce, instead of hard NMS. Per image and class, on the same candidates (score > score_thresh,
 * the topk_candidates best): repeatedly emit the remaining candidate with the largest CURRENT score (ties: lower anchor index) and multiply the
 * score of every other remaining candidate by f(u), u = its fp32 IoU with the emitted box:
 *   DN_NMS_SOFT_LINEAR   f = u > nms_thresh ? 1 - u : 1
 *   DN_NMS_SOFT_GAUSSIAN f = expf(-(u * u) / sigma)      (nms_thresh unused)
 * a candidate whose score falls to score_thresh or below is dropped. The global top-D then ranks the decayed scores, which are the scores reported.
 * Deterministic. The soft modes run every class of every image (the cut-off of the hard path does not hold under decay). */
enum { DN_NMS_HARD = 0, DN_NMS_SOFT_LINEAR = 1, DN_NMS_SOFT_GAUSSIAN = 2 };
/* The NMS method of the plan's later dn_forward / dn_forward_u8 (default DN_NMS_HARD; sigma is read by DN_NMS_SOFT_GAUSSIAN only and must then be
 * finite and > 0). DN_E_INVALID for an unknown method or such a sigma. Like dn_set_chains it drops the cached graphs: call it with no forward of
 * this plan in flight. dn_workspace_bytes does not change. */
DN_API int dn_set_nms(dn_plan* plan, int method, float sigma);
/* dn_postprocess with the method as an argument; DN_NMS_HARD is dn_postprocess bit for bit. Same workspace (dn_postprocess_workspace_bytes). */
DN_API int dn_postprocess_soft(const float* cls_logits_dev, const float* bbox_regression_dev, const float* anchors_dev,
                   int n, int num_anchors, int num_classes,
                   float image_h, float image_w, const float* scale_xy_dev /* [n][2] (w,h) ratios or NULL */,
                   float score_thresh, float nms_thresh, int nms_method, float nms_sigma, int topk_candidates, int detections_per_img,
                   float* boxes_dev, float* scores_dev, int64_t* labels_dev, int32_t* counts_dev,
                   int32_t* kept_anchor_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Single-kernel entry points (unit parity tests, micro-benchmarks, roofline measurement).
 * x: [m][cin] fp16 (NHWC rows), w: [cout][cin] fp16, bias fp32 [cout], residual [m][cout] fp16 or NULL,
 * w_frag (optional): the same weights in MFMA-fragment order (dn_op_desc PW w2) -- enables the strip kernel,
 * se_scale fp32 [m/hw][cin] or NULL, out fp16 [m][cout] (out_fp32 != 0: fp32, addressed
 * (row/hw)*out_img_stride + (row%hw)*cout + c). */
DN_API int dn_pointwise_conv(const void* x_dev, const void* w_dev, const void* w_frag_dev, const float* bias_dev,
                      const void* residual_dev, const float* se_scale_dev, void* out_dev, int m, int cin, int cout, int hw,
                      int act, int out_fp32, int64_t out_img_stride, void* stream);
/* Dense kxk convolution + bias + activation (the VGG path: vgg16 "D" convs, fc6 dilated 3x3, fc7 1x1, extras, ssd_vgg16.py:30-109).
 * x: [n][h][w][cin] fp16, w: [cout][k][k][cin] fp16, bias fp32 [cout], out [n][ho][wo][cout] fp16; cin % 32 == 0, cout % 4 == 0.
 * zeros (optional): >= 16 zero bytes on the device; with it, layers with cin % 64 == 0 and cout % 256 == 0 run on the
 * 256x256-tile kernel (taps outside the image are read from there). */
DN_API int dn_dense_conv(const void* x_dev, const void* w_dev, const float* bias_dev, const void* zeros_dev, void* out_dev,
                  int n, int h, int w, int cin, int cout, int k, int stride, int pad, int dil, int act, void* stream);
/* x: [n][h][w][c] fp16, w: [k*k][c] fp16, bias fp32 [c], out [n][ho][wo][c] fp16 */
DN_API int dn_depthwise_conv(const void* x_dev, const void* w_dev, const float* bias_dev, void* out_dev,
                      int n, int h, int w, int c, int k, int stride, int pad, int act, void* stream);
/* The same launch with the squeeze-excitation pooling: pool_dev [n][blocks][c] fp32 receives the per-workgroup channel sums of the
 * outputs, blocks = dn_depthwise_pool_blocks(...). With se_scale_dev non-NULL the last workgroup of each image also runs the FCs
 * (w1t [c][squeeze], w2t [squeeze][c] fp16, transposed; biases fp32) and writes scale [n][c] fp32; se_counter_dev: n zeroed
 * unsigneds, left at zero. */
DN_API int dn_depthwise_pool_blocks(int h, int w, int c, int k, int stride, int pad);
DN_API int dn_depthwise_conv_pool(const void* x_dev, const void* w_dev, const float* bias_dev, void* out_dev,
                      int n, int h, int w, int c, int k, int stride, int pad, int act, float* pool_dev,
                      const void* se_w1t_dev, const float* se_b1_dev, const void* se_w2t_dev, const float* se_b2_dev,
                      float* se_scale_dev, unsigned* se_counter_dev, int squeeze, void* stream);

/* Fused inverted-residual stages (expdw.hip): [1x1 expand w1/b1 + act1] -> depthwise kxk wd/bd + act2 -> [1x1 project w3/b3
 * (+ residual = x)], BN folded, padding (k-1)/2; replaces the ConvBNActivation chain of InvertedResidual.forward
 * (mobilenetv3.py:72-99) / _extra_block (ssd_mobilenetv3.py:39-54). The expanded / depthwise activations stay on chip.
 * w1 may be NULL (no expand: cexp == cin), w3 may be NULL (stop after the depthwise stage: out is [n][ho][wo][cexp] and
 * pool_partial (optional) receives [n][tiles][cexp] fp32 channel sums, tiles = dn_expand_depthwise_tiles(ho, wo, stride));
 * not both. x: [n][h][w][cin] fp16, w1 [cexp][cin], wd [k*k][cexp], w3 [cout][cexp] fp16. cin <= 128, k in {3,5}, stride in
 * {1,2}; with w3: (tile pixels / 32) * (cout / 32) <= 8 and no pooling. */
DN_API int dn_expand_depthwise(const void* x_dev, const void* w1_dev, const float* b1_dev, const void* wd_dev, const float* bd_dev,
                        const void* w3_dev, const float* b3_dev, void* out_dev, float* pool_partial_dev,
                        int n, int h, int w, int cin, int cexp, int cout, int k, int stride, int act1, int act2, int has_res,
                        void* stream);
DN_API int dn_expand_depthwise_tiles(int ho, int wo, int stride);

/* First inverted-residual block without an expansion (pwdirect.hip): depthwise 3x3 (stride 1, padding 1) wd/bd + act_dw -> 1x1 projection
 * w/b + act (+ residual = x), BN folded; mobilenetv3.py:61-99 with expanded == input channels, mobilenetv2.py:57-84 with expand_ratio 1.
 * The depthwise output stays in registers; the result equals dn_depthwise_conv followed by dn_pointwise_conv bit for bit.
 * x: [n][h][w][c] fp16, wd [9][c] fp16, bd fp32 [c], w [cout][c] fp16, b fp32 [cout], out [n][h][w][cout] fp16. c in {16, 32},
 * cout <= 32 and a multiple of 8, h * w >= 32, has_res only with cout == c; anything else returns DN_E_UNSUPPORTED.
 * The input is staged through LDS in bands of DN_PW_DW_BAND pixels of one image (environment DN_PW_DW_LDS=0: nine global taps per pixel
 * instead; also taken where a band and its two halos of w + 1 pixels do not fit 64 KB of LDS). */
#define DN_PW_DW_BAND 640
DN_API int dn_depthwise_pointwise(const void* x_dev, const void* wd_dev, const float* bd_dev, const void* w_dev, const float* b_dev,
                           void* out_dev, int n, int h, int w, int c, int cout, int act_dw, int act, int has_res, void* stream);

/* 1 = replay the launch sequence from a cached hipGraph keyed by (n, pointers) [default], 0 = eager launches */
DN_API int dn_set_graph_mode(dn_plan* plan, int enabled);

/* Timing hook for bench.py: average device time in ms of the op at `op_index` over the forwards recorded since
 * dn_profile_begin (HIP events on the forward stream, eager mode). */
DN_API int dn_profile_begin(dn_plan* plan);
DN_API int dn_profile_end(dn_plan* plan, float* ms_per_op /* [n_ops + 4] : ops..., softmax/decode (0 when the fused head launch does it), cut-off + select/NMS, merge, fallback select + merge */, int capacity);
/* After a profiled forward: the label of the kernel launch op `op_index` took part in (same spelling as rocprofv3's kernel
 * names, e.g. "pw_kernel<128,64,4,1,false,32>") and the op whose ms_per_op slot holds that launch's time (grouped launches
 * serve several ops; their members report the same owner). */
DN_API int dn_profile_op_info(const dn_plan* plan, int op_index, char* kernel, int capacity, int32_t* owner);

/* Optional extra output of dn_forward for the multi-GPU gather: when non-NULL, the final merge kernel also writes
 * packed_dev [n][D+1][6] fp32 -- rows (x1,y1,x2,y2,score,label), row D = (count,0,0,0,0,0) -- i.e. the fixed-shape payload of
 * the detections all-gather (the analogue of util/misc.py:75-115 all_gather of pickled results). NULL disables it. */
DN_API int dn_set_packed_output(dn_plan* plan, float* packed_dev);

/* Number of independent sub-batch launch chains a forward of n images is issued as (parallel hipGraph branches; 1 = a single
 * chain). Every kernel then runs once per sub-batch on ~n/split images; results are identical to the unsplit forward. */
DN_API int dn_batch_split(const dn_plan* plan, int n);
/* Overrides that choice: chains > 0 = every forward is issued as min(chains, n) sub-batch chains, 0 = back to the automatic
 * choice. For callers that keep several forwards in flight on streams of their own (one workspace and output set per forward):
 * whole-batch chains of different forwards overlap better than the half-size chains of one. Changes dn_workspace_bytes and drops
 * the cached graphs: call it before sizing workspaces, with no forward of this plan in flight. */
DN_API int dn_set_chains(dn_plan* plan, int chains);

/* SSD training loss, the value (with its gradient: dn_ssd_loss_train below). Replaces, per batch: the matching of
 * generalized_ssd.py:316-330 (torchvision box_iou -> SSDMatcher, _utils.py:264-294,348-362) and SSD.compute_loss
 * (generalized_ssd.py:210-269: encode_boxes _utils.py:100-133, smooth_l1_loss(sum), cross_entropy(none), hard negative mining with
 * neg_to_pos_ratio * (#label > 0) negatives per image, both sums / max(1, #matched anchors)).
 * cls_logits [n][A][K] fp32, bbox_regression [n][A][4] fp32, anchors [A][4] fp32 xyxy (the same for every image, as
 * DefaultBoxGenerator produces them), gt_boxes [n][gmax][4] fp32 xyxy / gt_labels [n][gmax] int64 padded, gt_counts [n] int32
 * (0 = an image without boxes: all background). matched_idxs_dev (optional, [n][A] int64) receives the matched gt index or -1;
 * losses_dev [2] = {bbox_regression, classification}. All pointers are device pointers; asynchronous on `stream`. */
DN_API size_t dn_ssd_loss_workspace_bytes(int n, int num_anchors);
DN_API int dn_ssd_loss(const float* cls_logits_dev, const float* bbox_regression_dev, const float* anchors_dev,
                       const float* gt_boxes_dev, const int64_t* gt_labels_dev, const int32_t* gt_counts_dev,
                       int n, int num_anchors, int num_classes, int gmax, float iou_thresh, float neg_to_pos_ratio,
                       int64_t* matched_idxs_dev, float* losses_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The same loss with its gradient for both head outputs (dn_lite_head_backward continues to the SSDLite head parameters; no backward through the backbone).
 * dn_ssd_loss_train = dn_ssd_loss (the same launches: losses_dev and matched_idxs_dev are bit-identical to it) that also keeps, in
 * state_dev (dn_ssd_loss_state_bytes(n, A) bytes, 16-byte aligned, the caller's until the backward has run), what the backward needs:
 * the matched index, the weight w in {0, 1, 2} of every anchor's cross entropy = (label > 0) + (mined negative), and
 * N = max(1, #matched). The mined negatives are those of a stable descending sort (ties at the cut in anchor order), as the oracle's.
 * dn_ssd_loss_backward, given the same inputs, that state and grad_losses_dev [2] = the upstream gradients of
 * {bbox_regression, classification}, writes every element of
 *   grad_cls_logits_dev [n][A][K]      = g_cls * w * (softmax(row) - onehot(target)) / N   (exactly 0 where w = 0)
 *   grad_bbox_regression_dev [n][A][4] = g_box * clamp(p - encoded target, -1, 1) / N for matched anchors, 0 elsewhere.
 * Either gradient pointer may be NULL (that gradient is not computed, and its input may then be NULL too); both 16-byte aligned.
 * grad_losses_dev and N are read on the device: neither call synchronises with the host, both can be captured. Deterministic. */
DN_API size_t dn_ssd_loss_state_bytes(int n, int num_anchors);
DN_API int dn_ssd_loss_train(const float* cls_logits_dev, const float* bbox_regression_dev, const float* anchors_dev,
                             const float* gt_boxes_dev, const int64_t* gt_labels_dev, const int32_t* gt_counts_dev,
                             int n, int num_anchors, int num_classes, int gmax, float iou_thresh, float neg_to_pos_ratio,
                             int64_t* matched_idxs_dev, float* losses_dev, void* workspace_dev, size_t workspace_bytes,
                             void* state_dev, size_t state_bytes, void* stream);
DN_API int dn_ssd_loss_backward(const float* cls_logits_dev, const float* bbox_regression_dev, const float* anchors_dev,
                                const float* gt_boxes_dev, const int64_t* gt_labels_dev, const void* state_dev, size_t state_bytes,
                                const float* grad_losses_dev, int n, int num_anchors, int num_classes, int gmax,
                                float* grad_cls_logits_dev, float* grad_bbox_regression_dev, void* stream);

/* Backward through one SSDLite head of one pyramid level (csrc/headgrad.hip): the gradients of the FOLDED head parameters, given the
 * gradient of the head output. Differentiates  depthwise 3x3 + BN + ReLU6 -> 1x1 conv with bias  (ssd_mobilenetv3.py:27-36; the V2
 * hub model's MultiBoxLiteHead, box_head.py:24-56, whose last level is a bare 1x1: wd == NULL, h = x, only g_w1 and g_b1 are
 * written and bd, g_wd, g_bd may be NULL).
 * x [n][h][w][c] fp16 NHWC (the level's feature map, e.g. dn_tensor_ptr), wd [9][c] fp16, bd [c] fp32, w1 [cout][c] fp16: the
 * folded weights the forward used. dy: fp32 gradient of the head output, read in place from the [n][A][K] / [n][A][4] gradient
 * tensor: the row of pixel p of image i is dy + i * dy_img_stride + p * cout (pass the tensor's address plus the level's anchor
 * offset times K or 4, and A * K or A * 4 as the stride), exactly as dn_pointwise_conv(out_fp32 = 1) addresses the forward's output.
 *   z = wd (*) x + bd (recomputed, fp32),  h = fp16(min(max(z, 0), 6)),
 *   g_b1[o] = sum_p dy[p][o],  g_w1[o][c] = sum_p dy[p][o] h[p][c],  dz = (dy w1) where 0 < z < 6,
 *   g_bd[c] = sum_p dz[p][c],  g_wd[t][c] = sum_p dz[p][c] x[p + t][c]  (nine taps, zero padding).
 * All four outputs fp32, every element written. The two contractions run on the fp16 matrix cores with dy scaled by a power of
 * two chosen on the device from max|dy| (no host synchronisation; gradients far below fp16's range keep their bits). Deterministic:
 * partial sums meet in a fixed order. Asynchronous on `stream`. x, wd, w1 and the workspace 16-byte aligned.
 * Invalid sizes or pointers: DN_E_INVALID; c % 8 != 0 or cout > 6 * DN_MAX_CLASSES: DN_E_UNSUPPORTED; workspace too small: DN_E_WORKSPACE.
 * dn_lite_head_backward_workspace_bytes: `depthwise` = 0 for a level without a depthwise stage; 0 for sizes the call rejects. */
DN_API size_t dn_lite_head_backward_workspace_bytes(int n, int h, int w, int c, int cout, int depthwise);
DN_API int dn_lite_head_backward(const void* x_dev, const void* wd_dev, const float* bd_dev, const void* w1_dev, const float* dy_dev,
                                 int64_t dy_img_stride, int n, int h, int w, int c, int cout, float* g_wd_dev, float* g_bd_dev,
                                 float* g_w1_dev, float* g_b1_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Sliced inference (csrc/sliced.hip): detection on images much larger than the network size by overlapping tiles at native resolution. A caller
 * crops the tiles (dn_crop_tiles), runs them as one dn_forward batch -- and, optionally, the whole image as one more forward -- and merges the
 * per-tile results into image coordinates (dn_merge_detections). demonet_amd/sliced.py and SSD.detect_sliced are that caller.
 *
 * dn_crop_tiles: image_dev [3][h][w] fp32, origins_dev [t][2] int32 (x0, y0) ON THE DEVICE, out_dev [t][3][th][tw] fp32 contiguous = the images_dev
 * of dn_forward with (n, h, w) = (t, th, tw). One gather launch, bit for bit; tiles whose rows start on 16-byte boundaries in both arrays (w, tw
 * and x0 multiples of 4, aligned bases) move in 16-byte accesses, others as single floats. DN_E_INVALID for a null pointer, a non-positive size,
 * t > 65535 and for a tile that leaves the image: to refuse that one, THIS CALL READS THE ORIGINS BACK (8 t bytes) AND WAITS FOR `stream` before it
 * enqueues the launch -- the exception to this header's rule; it cannot be captured into a graph. */
DN_API int dn_crop_tiles(const float* image_dev, int h, int w, const int32_t* origins_dev, int t, int th, int tw, float* out_dev, void* stream);

/* Hard NMS over detections that already exist: s_total sources, each one image's worth of dn_forward output (boxes [S][d][4] fp32, scores [S][d]
 * fp32, labels [S][d] int64, counts [S] int32), offsets_dev [S][2] fp32 (ox, oy) = where the source's origin lies in its output image, and the HOST
 * array group_begin [groups + 1] int32: sources group_begin[g] .. group_begin[g + 1] - 1 form output image g (0 <= group_begin[0], non-decreasing,
 * group_begin[groups] <= s_total; sources outside every group are ignored). Per group:
 *   1. candidates: the rows j < counts[s] of its sources, without those whose score is NaN; the row order inside a source is not assumed;
 *   2. a candidate's box is (x1 + ox, y1 + oy, x2 + ox, y2 + oy), one fp32 addition each; score and label unchanged;
 *   3. rank: score descending, ties by ascending flattened index s * d + j;
 *   4. in rank order, a candidate is kept unless a kept candidate of higher rank with the same label (any label when class_agnostic = 1) has
 *      m > thresh with it (strict), m in fp32 in the operation order of the per-class NMS: area = (x2 - x1) * (y2 - y1),
 *      inter = max(0, min x2 - max x1) * max(0, min y2 - max y1), DN_MERGE_IOU: m = inter / (a_i + a_j - inter), DN_MERGE_IOS (intersection over
 *      the smaller box, which also removes a box nested in a large one): m = inter / min(a_i, a_j); a NaN m does not suppress;
 *   5. the first d_out kept candidates, in rank order, are the output.
 * Outputs: boxes_out [groups][d_out][4], scores_out [groups][d_out], labels_out [groups][d_out] int64, counts_out [groups] int32 and, optional
 * (may be NULL), src_out [groups][d_out] int32 = the flattened index s * d + j the detection came from; rows at or beyond the count are zero (src -1).
 * Limits: d and d_out 1 .. 512, at most 1 024 sources and 65 536 slots (sources * d) per group, s_total * d < 2^31: DN_E_UNSUPPORTED beyond them.
 * DN_E_WORKSPACE below dn_merge_detections_workspace_bytes (which is 0 for sizes the call refuses; `groups` does not enter today). DN_E_INVALID for
 * null pointers, non-positive sizes, an unknown metric, a NaN thresh, a group_begin that decreases or leaves 0 .. s_total, boxes / boxes_out /
 * workspace not 16-byte aligned, offsets / labels not 8-byte aligned. group_begin is read during the call only. Asynchronous on `stream`, no host
 * synchronisation, can be captured; deterministic (the same bits on every run). */
enum { DN_MERGE_IOU = 0, DN_MERGE_IOS = 1 };
DN_API size_t dn_merge_detections_workspace_bytes(int s_total, int d, int groups);
DN_API int dn_merge_detections(const float* boxes_dev, const float* scores_dev, const int64_t* labels_dev, const int32_t* counts_dev,
                               const float* offsets_dev, int s_total, int d, const int32_t* group_begin, int groups, int metric, float thresh,
                               int class_agnostic, int d_out, float* boxes_out_dev, float* scores_out_dev, int64_t* labels_out_dev,
                               int32_t* counts_out_dev, int32_t* src_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Weighted boxes fusion over detections that already exist (csrc/fuse.hip): the reducer for sources that are different opinions about
 * the same objects -- the plain and the flipped pass of an image, several checkpoints -- where dn_merge_detections' hard NMS would keep one box and
 * drop what the other sources knew (Solovyev, Wang, Gabruseva 2019; conf_type 'avg' of the ensemble_boxes package). demonet_amd/fusion.py
 * (fuse_detections, detect_tta, ensemble_detect) is the caller. Inputs as for dn_merge_detections (boxes [S][d][4] fp32, scores [S][d] fp32, labels
 * [S][d] int64, counts [S] int32, offsets_dev [S][2] fp32, the HOST array group_begin [groups + 1]; sources outside every group are ignored), plus
 * weights_dev [S] fp32, one weight per source (NULL: every weight is 1). All arithmetic is fp32 with one rounding per operation. Per group:
 *   1. W = the weights of the group's sources, added in source order starting from 0;
 *   2. candidates: the rows j < counts[s] of its sources with v = score * weight[s] (one multiplication) not NaN, v >= skip_thresh and v > 0; a
 *      candidate's box is (x1 + ox, y1 + oy, x2 + ox, y2 + oy), one addition each;
 *   3. rank: v descending, ties by ascending flattened index s * d + j;
 *   4. in rank order, a candidate of label l is compared with the clusters of label l in creation order: u = IoU(cluster's fused box, candidate's
 *      box) in the operation order of dn_merge_detections (DN_MERGE_IOU, the fused box as a_i). It joins the cluster with the largest u > thresh
 *      (strict; the earliest-created one on a tie; a NaN u never matches);
 *   5. no such cluster: it opens a new one with T = 1, Sv = v, A_k = v * coord_k, and the fused box is the candidate's box exactly (not A / Sv);
 *   6. otherwise T += 1, Sv += v, A_k += v * coord_k (multiply, then add), fused coord_k = A_k / Sv;
 *   7. at the end a cluster's score is ((Sv / float(T)) * min(float(T), W)) / W, evaluated left to right, min(t, W) = W < t ? W : t;
 *   8. output: the clusters by that score descending (a NaN score, which only weights that are not positive numbers can produce, behind every
 *      number), ties by creation order; the first d_out of them.
 * Outputs: boxes_out [groups][d_out][4] (the fused boxes), scores_out [groups][d_out], labels_out [groups][d_out] int64, counts_out [groups] int32
 * and, optional (may be NULL), members_out [groups][d_out] int32 = T; rows at or beyond the count are zero.
 * Limits: d and d_out 1 .. 512, at most 8 192 slots (sources * d) per group -- the walk is quadratic when every box is a cluster of its own, which
 * is why this is narrower than the merge's 65 536 --, s_total * d < 2^31: DN_E_UNSUPPORTED beyond them. DN_E_WORKSPACE below
 * dn_fuse_detections_workspace_bytes, which takes group_begin as well and is 0 for everything the call refuses on its sizes or its group_begin.
 * DN_E_INVALID for null pointers (weights_dev and members_out_dev excepted), non-positive sizes, a thresh or skip_thresh that is NaN or negative, a
 * group_begin that decreases or leaves 0 .. s_total, boxes / boxes_out / workspace not 16-byte aligned, offsets / labels not 8-byte aligned.
 * group_begin is read during the call only. Six launches per 64 groups, asynchronous on `stream`, no host synchronisation, can be captured;
 * deterministic (no float atomics: the same bits on every run). */
DN_API size_t dn_fuse_detections_workspace_bytes(int s_total, int d, const int32_t* group_begin, int groups);
DN_API int dn_fuse_detections(const float* boxes_dev, const float* scores_dev, const int64_t* labels_dev, const int32_t* counts_dev,
                              const float* offsets_dev, const float* weights_dev, int s_total, int d, const int32_t* group_begin, int groups,
                              float thresh, float skip_thresh, int d_out, float* boxes_out_dev, float* scores_out_dev, int64_t* labels_out_dev,
                              int32_t* counts_out_dev, int32_t* members_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* PASCAL VOC true / false positive marking on the device (csrc/evalmatch.hip): the per-image part of the reference's voc_eval
 * (data/voc_eval.py:116-155) on the arrays dn_forward wrote, for several overlap thresholds in one launch. demonet_amd/voceval.py accumulates the
 * flags and finishes precision / recall / AP; engine.evaluate_voc is the loop around it.
 * Inputs: boxes [n][d][4] fp32 xyxy, scores [n][d] fp32, labels [n][d] int64, counts [n] int32 (dn_forward's outputs); gt_boxes [n][gmax][4] fp32,
 * gt_labels [n][gmax] int64, gt_difficult [n][gmax] uint8 (may be NULL: none difficult), gt_counts [n] int32, padded as dn_ssd_loss takes them.
 * thresholds is a HOST array [n_thresh], read during the call only. Per image i, with c = counts[i] and g = gt_counts[i] (each clamped to its
 * array), all arithmetic in double on the fp32 inputs converted to double, one rounding per operation, in exactly this order (= numpy's float64):
 *   1. candidates: the rows j < c; the row order is not assumed;
 *   2. best ground truth of a candidate (x1, y1, x2, y2) with label L, over the ground truths k < g with gt_labels[k] == L, o = pixel_offset:
 *        iw = max(min(gx2, x2) - max(gx1, x1) + o, 0), ih likewise (min / max as numpy's: a NaN operand gives NaN), inter = iw * ih,
 *        union = (x2 - x1 + o) * (y2 - y1 + o) + (gx2 - gx1 + o) * (gy2 - gy1 + o) - inter, ov = inter / union;
 *      best_ov = the maximum, best_gt = the lowest k that attains it (numpy's argmax); no ground truth of that label: best_ov = -inf, best_gt = -1;
 *      any of these ov NaN: best_ov = NaN, best_gt = -1 and the candidate is a false positive at every threshold (NaN > t is false).
 *      Ground-truth boxes must be finite: the caller's contract;
 *   3. rank inside the image: score descending, NaN scores last, ties by ascending slot j;
 *   4. for each threshold t (index b), in rank order with a fresh "claimed" bit per ground truth: best_ov > t (strict, double against double) and
 *      the ground truth difficult: neither flag; best_ov > t, not difficult, unclaimed: TP (bit b) and the ground truth is claimed; best_ov > t,
 *      not difficult, claimed: FP (bit 16 + b); best_ov > t false: FP. Rows j >= c: flags 0, best_gt -1, best_ov 0;
 *   5. for every k < g with 0 <= gt_labels[k] < num_classes: gt_stats[label][difficult ? 1 : 0] += 1 (integer atomics; other labels are not counted).
 * Outputs: flags [n][d] uint32, best_gt [n][d] int32 (may be NULL), best_ov [n][d] double (may be NULL), gt_stats [num_classes][2] int64 (may be
 * NULL; ADDED to: the caller zeroes it). One launch, one workgroup per image, no workspace.
 * Limits: d 1 .. 512, gmax 1 .. 1 024, n_thresh 1 .. 16, n 1 .. 65 535: DN_E_UNSUPPORTED beyond them. DN_E_INVALID for null required pointers,
 * non-positive sizes, num_classes < 1 with gt_stats given, a NaN threshold, a pixel_offset that is not finite or negative, boxes / gt_boxes not
 * 16-byte aligned, labels / gt_labels / best_ov / gt_stats not 8-byte aligned. Every argument is checked before the launch. Asynchronous on
 * `stream`, no host synchronisation, can be captured; deterministic. */
DN_API int dn_match_detections(const float* boxes_dev, const float* scores_dev, const int64_t* labels_dev, const int32_t* counts_dev,
                               const float* gt_boxes_dev, const int64_t* gt_labels_dev, const uint8_t* gt_difficult_dev,
                               const int32_t* gt_counts_dev, int n, int d, int gmax, int num_classes, const double* thresholds, int n_thresh,
                               double pixel_offset, uint32_t* flags_dev, int32_t* best_gt_dev, double* best_ov_dev, int64_t* gt_stats_dev,
                               void* stream);

/* COCO detection matching on the device (csrc/cocomatch.hip): the per-image part of pycocotools' COCOeval (computeIoU + evaluateImg for
 * bounding boxes, useCats = 1) on the arrays dn_forward wrote, for several IoU thresholds and area ranges in one launch. demonet_amd/cocoeval.py
 * accumulates the flags and finishes precision / recall / the twelve COCO numbers (accumulate + summarize); engine.evaluate_coco is the loop.
 * Inputs: boxes [n][d][4] fp32 xyxy, scores [n][d] fp32, labels [n][d] int64, counts [n] int32 (dn_forward's outputs); gt_boxes [n][gmax][4] fp32
 * xyxy, gt_labels [n][gmax] int64, gt_counts [n] int32, gt_crowd [n][gmax] uint8 (may be NULL: none; nonzero = the annotation's iscrowd or ignore),
 * gt_area [n][gmax] fp32 (may be NULL: w * h of the box; COCO's area is the segmentation's). thresholds [n_thresh] and area_ranges [n_ranges][2]
 * (lo, hi) are HOST arrays, read during the call only. Per image i, with c = counts[i] and g = gt_counts[i] (each clamped to its array); a
 * category = the rows of one label; all arithmetic in double, one rounding per operation, in exactly this order:
 *   1. boxes become (x, y, w, h) with w = fp32(x2 - x1), h = fp32(y2 - y1), detections and ground truths alike, then double;
 *   2. rank of a detection inside (image, category): score descending, NaN scores last, ties by ascending slot. Only ranks < max_det take part;
 *   3. IoU of detection (dx, dy, dw, dh) and ground truth (gx, gy, gw, gh): iw = fmin(dw + dx, gw + gx) - fmax(dx, gx); iw <= 0: IoU = 0;
 *      ih likewise on y; i = iw * ih; u = crowd ? dw * dh : dw * dh + gw * gh - i; IoU = i / u. No pixel offset;
 *   4. for range r = (lo, hi) a ground truth is ignored if it is crowd or area < lo or area > hi (both ends inclusive), area = gt_area or
 *      double(gw) * double(gh);
 *   5. the walk, for each threshold t (index b) and range r, over the category's detections in rank order: bar = min(t, 1 - 1e-10), match = none;
 *      pass 1 over the category's not-ignored ground truths in slot order, pass 2 over its ignored ones in slot order, pass 2 skipped when pass 1
 *      found a match; a ground truth already matched at (t, r) is skipped unless it is crowd; one with IoU < bar is skipped; any other becomes
 *      the match and bar = its IoU (a later equal IoU replaces it). A match marks the ground truth matched at (t, r), sets bit b of the
 *      detection's flags word for r and, if the ground truth is ignored in r, bit 16 + b. No match: bit 16 + b if dw * dh < lo or dw * dh > hi;
 *   6. for every k < g with 0 <= gt_labels[k] < num_classes and every r in which k is not ignored: gt_stats[label][r] += 1 (integer atomics).
 * Outputs: flags [n][d][n_ranges] uint32 (0 for rows >= c and for ranks >= max_det), rank [n][d] int32 (-1 for rows >= c; not cut at max_det),
 * match_gt [n][d][n_ranges][n_thresh] int32 (may be NULL) = the matched ground truth's slot or -1, gt_stats [num_classes][n_ranges] int64 (may be
 * NULL; ADDED to: the caller zeroes it). Every element of every output given is written. One launch, one workgroup per image, no workspace.
 * Limits: d 1 .. 512, gmax 1 .. 1 024, n_thresh 1 .. 16, n_ranges 1 .. 4, max_det 1 .. 128, n 1 .. 65 535: DN_E_UNSUPPORTED above them.
 * DN_E_INVALID for null required pointers, non-positive sizes or max_det, num_classes < 1 with gt_stats given, a NaN threshold or range end,
 * boxes / gt_boxes not 16-byte aligned, labels / gt_labels / gt_stats not 8-byte aligned, the other arrays not 4-byte aligned. Every argument is
 * checked before the launch. Asynchronous on `stream`, no host synchronisation, can be captured; deterministic. */
DN_API int dn_coco_match(const float* boxes_dev, const float* scores_dev, const int64_t* labels_dev, const int32_t* counts_dev,
                         const float* gt_boxes_dev, const int64_t* gt_labels_dev, const int32_t* gt_counts_dev, const uint8_t* gt_crowd_dev,
                         const float* gt_area_dev, int n, int d, int gmax, int num_classes, const double* thresholds, int n_thresh,
                         const double* area_ranges, int n_ranges, int max_det, uint32_t* flags_dev, int32_t* rank_dev, int32_t* match_gt_dev,
                         int64_t* gt_stats_dev, void* stream);

/* SSD training augmentation on the device (csrc/augment.hip): per batch, the reference's DetectionPresetTrain('ssd') (data/presets.py;
 * data/transforms.py:190-239 RandomPhotometricDistort, :132-187 RandomZoomOut, :54-129 RandomIoUCrop, :30-44 RandomHorizontalFlip, :47-51 ToTensor) and
 * the image half of the model transform's resize (transform.py:27-53, 150-173), from the decoder's output straight to the input of dn_forward /
 * SSD.loss with no intermediate image. The random draws and the boxes (transforms.py:121-126, 184-185, 37; transform.py:278-292) are the caller's:
 * demonet_amd/augment.py samples them; this call applies one parameter record per image.
 * images: HOST array of n DEVICE pointers, image i = [h_i][w_i][3] uint8, HWC, RGB, contiguous; sizes: HOST int32 [n][2] = (h_i, w_i); params: HOST
 * [n][DN_AUG_WORDS] 4-byte words (int32 or fp32 bits) as indexed below; out_dev [n][3][out_h][out_w] fp32 in [0, 1], NOT mean / std normalised (the
 * plan's stem does that). Per image, with x = u8 / 255 in fp32, gray = 0.2989 r + 0.587 g + 0.114 b and blend(a, b, f) = clamp(f a + (1 - f) b, 0, 1)
 * (torchvision's tensor formulas), each photometric step only when its flag is set, in this order:
 *   brightness blend(x, 0, f) | contrast blend(x, mean of gray over the whole image as it stands at that point, f) if DN_AUG_F_CONTRAST_BEFORE |
 *   saturation blend(x, gray(x), f) | hue: _rgb2hsv, h = (h + f) mod 1, _hsv2rgb | contrast otherwise | channels out[c] = in[perm[c]];
 *   a canvas CANVAS_H x CANVAS_W with that image at (LEFT, TOP) and FILL[c] elsewhere (the fill is neither distorted nor permuted); the crop
 *   (CROP_L, CROP_T, CROP_W, CROP_H) of the canvas; its horizontal flip if DN_AUG_F_FLIP; the bilinear resize (align_corners = False) of the crop
 *   to out_h x out_w, the arithmetic of dn_forward's input resize.
 * Launches: the contrast means (double sums of fixed chunks, fixed-shape tree, no float atomics; then one thread per image adds the partials in
 * index order) and the output (gather, photometric chain per tap, blend); the output launch alone when no record has contrast on. Deterministic: the same bits on every run. DN_E_INVALID, with nothing launched, for a null pointer (an image's included), n, out_h,
 * out_w or a size <= 0, unknown flag bits, an image placed outside its canvas (LEFT, TOP < 0 or LEFT + w > CANVAS_W or TOP + h > CANVAS_H), a crop
 * that is empty or leaves the canvas, perm not a permutation of 0 1 2, a non-finite factor or fill, a workspace that is not 16-byte aligned or
 * smaller than dn_augment_workspace_bytes(n) (0 for an n the call refuses); DN_E_UNSUPPORTED for n > 65 535, an image above 2^29 pixels or an output
 * of 2^31. Whatever the record says, no byte outside an image's h_i x w_i x 3 is read. The three host arrays are read during the call only: the
 * table goes into the workspace by ONE copy on `stream`, the launches are enqueued behind it, and THE CALL THEN WAITS FOR THAT COPY (the table is
 * the call's own host memory; the launches go on behind it): like dn_crop_tiles an exception to this header's rule, and not capturable. */
enum { DN_AUG_FLAGS = 0,                /* int32: DN_AUG_F_* bits */
       DN_AUG_BRIGHTNESS = 1, DN_AUG_CONTRAST = 2, DN_AUG_SATURATION = 3, DN_AUG_HUE = 4,   /* fp32 factors (read only when the flag is set; always finite) */
       DN_AUG_PERM = 5,                 /* int32 [3] */
       DN_AUG_CANVAS_H = 8, DN_AUG_CANVAS_W = 9, DN_AUG_LEFT = 10, DN_AUG_TOP = 11,         /* int32 */
       DN_AUG_FILL = 12,                /* fp32 [3], in [0, 1] units (the reference's default: (123, 117, 104) / 255) */
       DN_AUG_CROP_L = 15, DN_AUG_CROP_T = 16, DN_AUG_CROP_W = 17, DN_AUG_CROP_H = 18,      /* int32, canvas coordinates */
       DN_AUG_WORDS = 20 };             /* word 19: reserved, 0 */
enum { DN_AUG_F_BRIGHTNESS = 1, DN_AUG_F_CONTRAST = 2, DN_AUG_F_SATURATION = 4, DN_AUG_F_HUE = 8, DN_AUG_F_CONTRAST_BEFORE = 16, DN_AUG_F_FLIP = 32,
       DN_AUG_F_ALL = 63 };
DN_API size_t dn_augment_workspace_bytes(int n);
DN_API int dn_augment_batch(const uint8_t* const* images, const int32_t* sizes, const int32_t* params, int n, int out_h, int out_w,
                            float* out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The optimizer step of head fine-tuning on the device (csrc/optim.hip): torch.optim.SGD's update and clip_grad_norm_'s norm for ALL
 * tensors of a param group in one launch each, and the reference loop's `math.isfinite(loss)` (engine.py:39-44) as a gate inside the update launch,
 * so that a training loop needs no host synchronisation per step. fp32 tensors only.
 * table_dev: DEVICE memory, T records dn_sgd_tensor and, right behind them, int32 first[T + 1]: first[t] = the number of chunks of the tensors in
 * front of t, a chunk = DN_SGD_CHUNK consecutive elements of one tensor (ceil(numel / DN_SGD_CHUNK) per tensor), first[T] = chunks. p, g and buf
 * hold numel contiguous floats each; buf (the momentum buffer) is read and written only when momentum != 0 and may be null otherwise. The caller
 * keeps the table true to its tensors: the library cannot see it from the host and reads numel elements at every pointer.
 * dn_grad_norm: *norm_out_dev = sqrt(sum of g * g over every tensor of the table), fp32. Two launches: per-chunk sums in float64 (an fp32 square is
 * exact there; fixed order per thread, fixed-shape tree per workgroup) into partials_ws[chunk], then ONE workgroup adds the partials in index order,
 * takes the square root in float64 and rounds once. No atomics: the same bits on every run. partials_ws: 8-byte aligned, at least
 * dn_sgd_workspace_bytes(T, chunks) (0 for sizes the calls refuse).
 * dn_sgd_step: one launch, per element, every operation one rounded fp32 operation (no contraction) in torch.optim.SGD's order:
 *   d = g * coef                       only when max_norm > 0: coef = min(1, max_norm / (*norm_dev + 1e-6)), clip_grad_norm_'s coefficient
 *   d = d + weight_decay * p           only when weight_decay != 0
 *   b = first_step ? d : momentum * b + (1 - dampening) * d       only when momentum != 0
 *   d = nesterov ? d + momentum * b : b                           only when momentum != 0
 *   p = p - lr * d
 * g is NOT modified (clip_grad_norm_ scales .grad in place; here the coefficient is applied on the way). 16-byte accesses where p, g and buf are
 * 16-byte aligned, 4-byte accesses otherwise; no element at or beyond numel is touched.
 * The gate: gate_dev = gate_count (0 .. DN_SGD_MAX_GATE) fp32 DEVICE values, typically the loss terms and the norm. If any of them is not finite, or
 * status_dev[0] != 0, the launch writes nothing to any p or buf and sets status_dev[0] = 1: the gate is sticky, every later call is skipped until
 * the caller clears status_dev[0]. status_dev: int32 [2] on the device; [1] receives hyper.step from every call that found [0] clear, so after a
 * trip it holds the step that tripped.
 * Both calls only enqueue on `stream`. DN_E_INVALID for a null table, status, workspace, norm_out or (with gate_count > 0) gate pointer, T or chunks
 * < 1, gate_count outside 0 .. DN_SGD_MAX_GATE, a negative or non-finite lr, momentum, weight_decay or max_norm, a non-finite dampening, a negative
 * step, nesterov without momentum or with dampening, max_norm > 0 without norm_dev; DN_E_UNSUPPORTED for T > 65 535; DN_E_WORKSPACE for a
 * workspace below dn_sgd_workspace_bytes. */
#define DN_SGD_CHUNK 2048
#define DN_SGD_MAX_GATE 8
typedef struct dn_sgd_tensor {
    float* p;
    const float* g;
    float* buf;
    int64_t numel;
} dn_sgd_tensor;
typedef struct dn_sgd_hyper {
    float lr, momentum, dampening, weight_decay;
    int32_t nesterov, first_step;       /* first_step: the buffers of this table's tensors do not exist yet: b = d, without dampening */
    int32_t step;                       /* the caller's step counter, for status_dev[1] */
    int32_t reserved;
} dn_sgd_hyper;
DN_API size_t dn_sgd_workspace_bytes(int T, int chunks);
DN_API int dn_grad_norm(const dn_sgd_tensor* table_dev, int T, int chunks, void* partials_ws, size_t workspace_bytes, float* norm_out_dev, void* stream);
DN_API int dn_sgd_step(const dn_sgd_tensor* table_dev, int T, int chunks, dn_sgd_hyper hyper, const float* gate_dev, int gate_count,
                       const float* norm_dev, float max_norm, int32_t* status_dev, void* stream);

/* Multi-object tracking on the device (csrc/track.hip): ByteTrack (Zhang et al. 2022, BYTETracker.update with its constant-velocity
 * Kalman filter) for `streams` independent video streams, ONE launch per frame step, all tracker state on the device. demonet_amd/track.py
 * (ByteTracker, SSD.track) is the caller. The frame counter and the id counter live in the state, so a step's arguments do not change from frame to
 * frame and the call can be captured. Two deviations from the published tracker:
 *   A. association is GREEDY, not lapjv: pairs above the gate are taken in the total order (IoU descending, track slot ascending, detection row
 *      ascending), a pair being taken when neither side is taken yet. (An optimal assignment is not unique under ties and cannot be held bit for
 *      bit; greedy equals it whenever objects do not compete.) The kernel reaches the same matching by rounds of mutually-best pairs;
 *   B. ids come from a per-stream counter: they start at 1 and are handed out in detection-row order within a frame, so streams are independent
 *      and the result is deterministic. fuse_score (the MOT20 option) is left out.
 * The filter. ByteTrack's 8 x 8 filter is four independent two-state filters: the initial covariance, Q and R are diagonal and F couples each
 * coordinate only with its own velocity, so the covariance stays block-diagonal. Per track and per coordinate k of (cx, cy, a = w / h, h) the state
 * keeps five floats x, v, Pxx, Pxv, Pvv. All arithmetic is fp32, one rounding per operation, in exactly this order; wp = 0.05f, wv = 0.00625f (1 / 20
 * and 1 / 160 rounded to fp32), H = the track's x of coordinate h at the moment named:
 *   box -> measurement: w = x2 - x1, h = y2 - y1, z = (x1 + w * 0.5, y1 + h * 0.5, w / h, h);
 *   mean -> box: h = x_h, w = x_a * h, x1 = x_cx - w * 0.5, y1 = x_cy - h * 0.5, box = (x1, y1, x1 + w, y1 + h);
 *   init from z (H = z_h): x = z, v = 0, Pxv = 0, sp = wp * H, sv = wv * H, Pxx = (2 * sp) * (2 * sp), Pvv = (10 * sv) * (10 * sv); for a:
 *     Pxx = 1e-2f * 1e-2f, Pvv = 1e-5f * 1e-5f;
 *   predict (H before the step): sp = wp * H, sv = wv * H, qp = sp * sp, qv = sv * sv (for a: 1e-2f * 1e-2f and 1e-5f * 1e-5f); per coordinate, from the
 *     old values: x = x + v, Pxx = ((Pxx + 2 * Pxv) + Pvv) + qp, Pxv = Pxv + Pvv, Pvv = Pvv + qv;
 *   update with z (H = the track's current, i.e. predicted, h): sp = wp * H, r = sp * sp (for a: 1e-1f * 1e-1f); per coordinate, from the old values:
 *     S = Pxx + r, kx = Pxx / S, kv = Pxv / S, y = z - x, x = x + kx * y, v = v + kv * y, Pxx = Pxx - (kx * S) * kx, Pxv = Pxv - (kx * S) * kv,
 *     Pvv = Pvv - (kv * S) * kv.
 * A frame step, per stream (slot states: 0 free, 1 tentative, 2 tracked, 3 lost):
 *   1. frame += 1;
 *   2. candidates: the rows j < min(max(counts[b], 0), d) whose score is not NaN, whose four coordinates are finite and whose w = x2 - x1 and
 *      h = y2 - y1 are > 0. HIGH: score >= track_thresh. LOW: low_thresh < score < track_thresh;
 *   3. every tracked and lost track is predicted, a lost one with the v of h set to 0 first; tentative tracks are not predicted. A track's box in
 *      the stages below is mean -> box of what it holds then;
 *   4. stage 1: tracked and lost tracks against the HIGH candidates. A pair is admissible when u > 1 - match_thresh (one fp32 subtraction; strict;
 *      a NaN u never matches) and the labels are equal (any labels with class_agnostic != 0), u = IoU in the operation order of
 *      dn_merge_detections (DN_MERGE_IOU, the track's box as a_i): inter = max(0, min x2 - max x1) * max(0, min y2 - max y1),
 *      u = inter / ((a_i + a_j) - inter). Greedy as in A. A match updates the filter with the row's measurement, sets score = the row's score,
 *      last_frame = frame, det = the row, state = tracked (a lost track is tracked again and keeps its id);
 *   5. stage 2: the tracks that were tracked when the frame began and are still unmatched (not the lost ones) against the LOW candidates, gate
 *      u > 1 - second_thresh, same rules. Those still unmatched become lost;
 *   6. stage 3: tentative tracks against the HIGH candidates no track has taken, gate u > 1 - unconfirmed_thresh. A match confirms the track
 *      (state tracked). An unmatched tentative track is removed;
 *   7. every HIGH candidate still untaken with score >= new_thresh starts a track, in row order, in the lowest free slot (slots freed in step 6
 *      included, those of step 8 not): id = next_id, next_id += 1, label and score the row's, start_frame = last_frame = frame, det = the row,
 *      state tentative -- tracked at once when frame == 1. With no free slot the row starts nothing and `dropped` goes up by one;
 *   8. a lost track with frame - last_frame > track_buffer is removed;
 *   9. outputs: the tracked tracks with last_frame == frame, in ascending slot order: boxes_out [streams][max_tracks][4] (mean -> box), scores_out,
 *      labels_out int64, ids_out int64, det_out int32 (the row that updated or started the track), counts_out [streams] int32; rows at or beyond
 *      the count are zero, det -1. det_ids_out [streams][d] int64, aligned with the input rows: the id of the track output in this frame that the
 *      row updated or started, or -1.
 * The state, dn_track_state_bytes(streams, max_tracks) bytes, 16-byte aligned: per stream W = 4 + 28 Tp 4-byte words, Tp = max_tracks rounded up to
 * a multiple of 4, streams back to back. Words 0 .. 3: int32 frame, next_id, dropped, reserved (0). Then per-slot arrays of Tp entries each, in
 * this order: int32 state, int32 id, int64 label, fp32 score, fp32 filter [20][Tp] (row 5 k + (0 x, 1 v, 2 Pxx, 3 Pxv, 4 Pvv) for coordinate k of cx, cy,
 * a, h), int32 start_frame, int32 last_frame, int32 det (the row that updated the slot in the last step, -1 if none did). Every field of a free slot
 * and of the slots max_tracks .. Tp - 1 is 0. dn_track_reset is one launch: the streams b with which_dev[b] != 0 (which_dev: [streams] uint8 on
 * the device; NULL: all) restart with frame 0, next_id 1, dropped 0 and an empty table; a new state must be reset before its first step.
 * params is HOST memory, read during the call only.
 * Limits: d 1 .. 512, max_tracks 1 .. 256, streams >= 1: DN_E_UNSUPPORTED above them (dn_track_state_bytes then returns 0). DN_E_WORKSPACE for
 * state_bytes below dn_track_state_bytes. DN_E_INVALID for null pointers (which_dev excepted), non-positive sizes, a threshold that is NaN or
 * negative, match_thresh / second_thresh / unconfirmed_thresh above 1, a negative track_buffer, boxes / boxes_out / state not 16-byte aligned,
 * labels / labels_out / ids_out / det_ids_out not 8-byte aligned, the other arrays not 4-byte aligned. One workgroup per stream, no workspace, no
 * float atomics; asynchronous on `stream`, no host synchronisation, can be captured; deterministic (the same bits on every run). */
typedef struct dn_track_params {
    float track_thresh, low_thresh, new_thresh;                 /* ByteTrack: 0.5, 0.1, track_thresh + 0.1 */
    float match_thresh, second_thresh, unconfirmed_thresh;      /* costs 1 - IoU, as in ByteTrack: 0.8, 0.5, 0.7 */
    int32_t track_buffer;                                       /* frames a lost track is kept: 30 */
    int32_t class_agnostic;
    int32_t max_tracks;                                         /* slots per stream, 1 .. 256 */
    int32_t reserved;                                           /* 0 */
} dn_track_params;
DN_API size_t dn_track_state_bytes(int streams, int max_tracks);
DN_API int dn_track_reset(void* state_dev, int streams, int max_tracks, const uint8_t* which_dev, void* stream);
DN_API int dn_track_update(const float* boxes_dev, const float* scores_dev, const int64_t* labels_dev, const int32_t* counts_dev, int streams, int d,
                           const dn_track_params* params, void* state_dev, size_t state_bytes, float* boxes_out_dev, float* scores_out_dev,
                           int64_t* labels_out_dev, int64_t* ids_out_dev, int32_t* det_out_dev, int32_t* counts_out_dev, int64_t* det_ids_out_dev,
                           void* stream);

/* Appearance association in the tracker (csrc/trackapp.hip): dn_track_update_appearance is dn_track_update with the appearance term of
 * BoT-SORT (Aharon et al. 2022) -- cosine distance / 2, an appearance threshold, a proximity mask, min(d_iou, d_emb), an exponentially smoothed
 * unit-norm feature per track -- fused into the pair value. demonet_amd/track.py (AppearanceTracker, SSD.track_frames_appearance) is the caller;
 * tests/track_appearance_ref.py restates these sentences. Every argument of dn_track_update keeps its meaning, and the tracker's state block keeps
 * its layout: dn_zone_update and the cropper read it as before.
 * Inputs beside dn_track_update's, in DEVICE memory: emb_dev [E][dim], fp32 or (params->emb_fp16) fp16, and emb_index_dev [E][8] int32 -- the
 * cropper's index table as it lies: word 0 the stream or -1, word 1 the row; the other words are not read. NONE OF THEM IS TRUSTED: an index row
 * whose stream is outside 0 .. streams - 1 or whose row is outside 0 .. n - 1 (n = min(max(counts[stream], 0), d)) is ignored; if several index
 * rows name the same (stream, row), the highest slot e wins (an integer maximum, so the order in which the device visits them does not
 * matter), whether or not that slot's embedding is present. An embedding is ABSENT when an element is not finite or when its norm -- sqrt of
 * the fp32 sum of the fp32 squares -- is 0 or not finite. A row HAS AN EMBEDDING when a winning slot names it and that slot's embedding is present.
 * Normalised rows: en[e][k] = fp16(x[e][k] / norm_e), the fp32 quotient rounded to nearest even; the rows of absent embeddings are 0. (The order
 * of the norm's sum is the implementation's and fixed: the same bits on every run.)
 * Track features, features_dev, dn_track_feature_bytes(streams, max_tracks, dim) bytes, 16-byte aligned: per stream Tp (1 + dim) 4-byte words,
 * streams back to back: int32 valid [Tp], then fp32 feature [Tp][dim]. The values of a slot whose flag is 0 mean nothing. dn_track_feature_reset
 * zeroes the streams b with which_dev[b] != 0 (NULL: all); a new buffer must be reset before its first step, and a stream restarted with
 * dn_track_reset must be reset here too. A slot that is free has valid = 0.
 * Similarity: S[b][slot][row] = sum_k fp16(feature[slot][k]) * en[e(row)][k], fp16 operands (the feature rounded to nearest even), fp32
 * accumulation on the matrix cores, from the features as the step found them. S is [streams][Tp][d] fp32; all of it is written in every step with
 * embeddings, an entry whose slot has valid = 0 or whose row has no embedding as 0 (such an entry is never used).
 * The pair value v of stages 1 and 3, fp32, one rounding per operation: u = the IoU of dn_track_update. If the track's slot has valid != 0 and the
 * row has an embedding: h = (1 - S) * 0.5, e = h < 0 ? 0 : h (a NaN stays); appearance is ADMISSIBLE when e <= appearance_thresh and
 * 1 - u <= proximity_thresh (a NaN never is); v = admissible ? (u > 1 - e ? u : 1 - e) : u. Otherwise, and always in stage 2 (the LOW rows:
 * IoU alone, as published), v = u. Everything else is dn_track_update's text with v in place of u: the strict gates v > 1 - thresh, the labels,
 * the total order (v descending, slot ascending, row ascending), greedy, new tracks, ids, removal, outputs. With proximity_thresh = 1 a pair with
 * an empty intersection (u = 0) can match by appearance alone: a lost track is found again without overlap.
 * The features after the step: a track that STARTS from a row with an embedding takes feature = float(en[e]) and valid = 1, from a row without
 * one valid = 0. A MATCH (any stage) with a row that has an embedding: with valid != 0, s[k] = alpha * s[k] + (1 - alpha) * float(en[e][k])
 * (1 - alpha: one fp32 subtraction), then s /= |s| (the fp32 norm as above; a norm that is 0 or not finite clears valid); with valid = 0 a plain
 * start. A match with a row without an embedding leaves the feature alone. A slot that is freed (steps 6 and 8) gets valid = 0.
 * With no row that has an embedding -- or with E = 0, emb_dev = emb_index_dev = NULL, when the workspace is not touched and may be NULL -- the
 * step's outputs and state equal dn_track_update's bit for bit.
 * The workspace, dn_track_appearance_workspace_bytes(streams, max_tracks, d, E, dim) bytes, 16-byte aligned; its parts in this order, each rounded
 * up to a multiple of 16 bytes: en [E][dim] fp16, present [E] int32, map [streams][d] int32 (the winning slot of the row or -1),
 * S [streams][Tp][d] fp32. en, S, present and map are outputs a caller may read after the step.
 * params and app are HOST memory, read during the call only. Limits: dn_track_update's, E 0 .. 8192, dim a multiple of 32 in 32 .. 512:
 * DN_E_UNSUPPORTED beyond them (the two size functions then return 0; dn_track_appearance_workspace_bytes also for E = 0). DN_E_INVALID for what
 * dn_track_update refuses, a null app or features, dim < 1, E < 0, alpha not a number in 0 .. 1, a threshold that is NaN or negative, emb_fp16 not 0
 * or 1, non-zero reserved words, E = 0 with a non-null emb or emb_index, E > 0 with a null emb, emb_index or workspace, features / emb / emb_index /
 * workspace not 16-byte aligned. DN_E_WORKSPACE for state_bytes, feature_bytes or (E > 0) workspace_bytes below their size functions. Every error
 * is raised before anything is enqueued. A step with embeddings enqueues four graph nodes (a fill of the map, the norms, the similarity, the
 * step), one without embeddings the step alone; no device memory is allocated, no host synchronisation, can be captured; no float atomics;
 * deterministic (the same bits on every run, S included). */
typedef struct dn_track_appearance_params {   /* 32 bytes, HOST memory */
    int32_t dim;                              /* a multiple of 32 in 32 .. 512 */
    float   alpha;                            /* the feature's smoothing, 0 .. 1: 0.9 */
    float   appearance_thresh;                /* on e = (1 - cosine) / 2: 0.25 */
    float   proximity_thresh;                 /* on 1 - IoU: 0.5; 1 lets appearance match without overlap */
    int32_t emb_fp16;                         /* 0: emb_dev is fp32, 1: fp16 */
    int32_t reserved[3];                      /* 0 */
} dn_track_appearance_params;
#if defined(__cplusplus)
static_assert(sizeof(dn_track_appearance_params) == 32, "dn_track_appearance_params is 32 bytes");
#else
_Static_assert(sizeof(dn_track_appearance_params) == 32, "dn_track_appearance_params is 32 bytes");
#endif
DN_API size_t dn_track_feature_bytes(int streams, int max_tracks, int dim);
DN_API size_t dn_track_appearance_workspace_bytes(int streams, int max_tracks, int d, int E, int dim);
DN_API int dn_track_feature_reset(void* features_dev, int streams, int max_tracks, int dim, const uint8_t* which_dev, void* stream);
DN_API int dn_track_update_appearance(const float* boxes_dev, const float* scores_dev, const int64_t* labels_dev, const int32_t* counts_dev,
                                      int streams, int d, const dn_track_params* params, const dn_track_appearance_params* app,
                                      const void* emb_dev, const int32_t* emb_index_dev, int E, void* state_dev, size_t state_bytes,
                                      void* features_dev, size_t feature_bytes, void* workspace_dev, size_t workspace_bytes,
                                      float* boxes_out_dev, float* scores_out_dev, int64_t* labels_out_dev, int64_t* ids_out_dev,
                                      int32_t* det_out_dev, int32_t* counts_out_dev, int64_t* det_ids_out_dev, void* stream);

/* Line-crossing and zone analytics behind the tracker (csrc/zones.hip): per stream up to 16 directed lines and 16 polygon zones;
 * counters and a short event list accumulate on the device, ONE more small launch per frame step. demonet_amd/zones.py (ZoneAnalytics) is the
 * caller. dn_zone_update runs after dn_track_update on the same stream and READS the tracker's state as documented above (the header words and the
 * per-slot arrays state, id, label, filter, last_frame of Tp entries); it never writes it. The configuration and the class map lie in device
 * memory, so a captured step follows edits made between replays.
 * config_dev: [streams] dn_zone_config, coordinates in frame pixels (the coordinates of the tracker's boxes). n_lines, n_zones and nv come from
 * device memory, so the kernel clamps them: n_lines and n_zones to 0 .. 16, every nv to 3 .. 16 (the caller validates them before upload).
 * class_bin_dev: [n_labels] uint8. A track of label l counts in bin class_bin[l], 0 .. 7; the value 255 (and any value above 7), or l outside
 * [0, n_labels), means the track is ignored. NULL: every label goes to bin 0.
 * anchor: 0 the box centre ((x1 + x2) * 0.5f, (y1 + y2) * 0.5f), 1 the bottom centre ((x1 + x2) * 0.5f, y2); (x1, y1, x2, y2) is the tracker's
 * mean -> box of the slot's filter, in its operation order. All arithmetic is fp32 with one rounding per operation, the divide correctly rounded.
 * A step, per stream. f is the tracker's frame word, T the tracker's fields of slot s, Z the zone state's:
 *   1. per slot s < max_tracks: if T.state == 0 or T.id != Z.id[s], the old entry is closed: for every zone bit z set in Z.inside,
 *      vanished[z][Z.bin] goes up by one and a VANISH event is emitted with dwell f - enter_frame[z] (label -1: the state keeps no label; Z.bin is
 *      taken modulo 8). The entry then becomes (id = T.state ? T.id : 0, has_prev = 0, inside = 0); its other fields stay;
 *   2. the slot is OBSERVED iff T.state == 2, T.last_frame == f, its bin is not 255, and both anchor coordinates are finite. A slot that is not
 *      observed does nothing further and counts in no occupancy. When the slot is observed, Z.bin is set;
 *   3. lines apply only with has_prev. side(A, B, P) = (bx - ax) * (py - ay) - (by - ay) * (px - ax). For line i < n_lines, prev the stored anchor
 *      and p this frame's: a = side(A, B, prev), c = side(A, B, p), u = side(prev, p, A), v = side(prev, p, B). If any of the four is NaN there is
 *      no crossing; otherwise there is one iff (a >= 0) != (c >= 0) and (u >= 0) != (v >= 0). The direction is 0 when c >= 0, else 1.
 *      line_count[i][dir][bin] += 1, and a CROSS event is emitted;
 *   4. zones, even-odd rule: for zone z < n_zones and its edge e with i = e, j = e ? e - 1 : nv - 1: if (yi > py) != (yj > py) and
 *      px < (xj - xi) * (py - yi) / (yj - yi) + xi, toggle. The zones at or beyond n_zones hold nobody. For every z < 16, bit 0 -> 1:
 *      entries[z][bin] += 1, enter_frame[z] = f, an ENTER event (the first observation of a track counts as such); bit 1 -> 0: exits[z][bin] += 1,
 *      dwell = f - enter_frame[z], dwell_sum[z][bin] += dwell, dwell_max[z][bin] = max(dwell_max[z][bin], dwell), an EXIT event.
 *      occupancy[z][bin] is rewritten every step as the number of observed tracks inside;
 *   5. prev = p, has_prev = 1;
 *   6. events are rows of eight int32 (kind, index, id, label, bin, frame, dwell, direction): kind DN_ZONE_CROSS / ENTER / EXIT / VANISH, index the
 *      line or the zone, label the low 32 bits of T.label, dwell 0 for CROSS and ENTER, direction 0 except for CROSS. Their order is slot ascending,
 *      and within a slot VANISH by zone, then CROSS by line, then EXIT / ENTER by zone;
 *   7. the first max_events of a step are kept (events_out_dev [streams][max_events][8]); event_counts_out_dev [streams] is the kept number, the
 *      excess is added to events_dropped, and the rows at or beyond the count are zero.
 * The zone state, dn_zone_state_bytes(streams, max_tracks) bytes, 16-byte aligned: per stream W = 1156 + 22 Tp 4-byte words, Tp = max_tracks rounded
 * up to a multiple of 4 as in the tracker, streams back to back. Words 0 .. 3: int32 events_dropped, three reserved (0). Then per-slot arrays of Tp
 * entries each, in this order: int32 id, int32 bin, int32 has_prev, fp32 px, fp32 py, uint32 inside (bit z: zone z), int32 enter_frame [16][Tp].
 * Then the counters: int32 line_count [16][2][8] (line, direction, bin); int32 entries, exits, vanished, occupancy, dwell_max [16][8] each (zone,
 * bin); int64 dwell_sum [16][8]. dn_zone_reset is one launch: the streams b with which_dev[b] != 0 (NULL: all) become all zero; a new state must be
 * reset before its first step.
 * Limits: max_tracks 1 .. 256, max_events 1 .. 1024: DN_E_UNSUPPORTED above them (dn_zone_state_bytes then returns 0). DN_E_INVALID for null pointers
 * (class_bin_dev and which_dev excepted), non-positive sizes (n_labels only with a class map), anchor not 0 or 1, track state / config / zone state /
 * events not 16-byte aligned, event_counts not 4-byte aligned, or track_state_bytes below dn_track_state_bytes. DN_E_WORKSPACE for zstate_bytes below
 * dn_zone_state_bytes. One workgroup per stream, one thread per slot, no workspace; integer counters meet through LDS integer atomics (an integer sum
 * does not depend on the order), no float atomics; event positions come from a prefix scan inside the workgroup, so their order is fixed.
 * Asynchronous on `stream`, no host synchronisation, can be captured; deterministic (the same bits on every run). */
enum { DN_ZONE_CROSS = 1, DN_ZONE_ENTER = 2, DN_ZONE_EXIT = 3, DN_ZONE_VANISH = 4 };
typedef struct dn_zone_config {     /* 2384 bytes; offsets: n_lines 0, lines 4, n_zones 260, nv 264, verts 328, reserved 2376 */
    int32_t n_lines;                /* 0 .. 16 */
    float lines[16][4];             /* (ax, ay, bx, by) */
    int32_t n_zones;                /* 0 .. 16 */
    int32_t nv[16];                 /* vertices per zone, 3 .. 16 */
    float verts[16][16][2];         /* (x, y) */
    int32_t reserved[2];            /* 0: keeps the records of an array 16-byte aligned */
} dn_zone_config;
DN_API size_t dn_zone_state_bytes(int streams, int max_tracks);
DN_API int dn_zone_reset(void* zstate_dev, int streams, int max_tracks, const uint8_t* which_dev, void* stream);
DN_API int dn_zone_update(const void* track_state_dev, size_t track_state_bytes, int streams, int max_tracks, const dn_zone_config* config_dev,
                          const uint8_t* class_bin_dev, int n_labels, int anchor, void* zstate_dev, size_t zstate_bytes, int32_t* events_out_dev,
                          int32_t* event_counts_out_dev, int max_events, void* stream);

/* Object crops from video surfaces behind the tracker (csrc/crops.hip): the boxes of every stream become fixed-size normalised patches
 * cut out of the frames at native resolution -- the input of a second model (a re-identification embedder, an attribute or plate classifier) --
 * without the boxes visiting the host and without a converted frame. demonet_amd/crops.py (ObjectCropper) is the caller.
 * frames_dev: [streams] dn_frame records as for dn_forward_frames (format, color: its codes); stream b reads frame b. boxes_dev: [streams][d][4] fp32
 * (x1, y1, x2, y2) in that frame's pixels -- the tracker's boxes_out, or a forward's boxes. counts_dev: [streams] int32. select_dev: [streams][d]
 * uint8 or NULL; a row whose byte is 0 is skipped (caller policies such as "every k-th frame of a track's life", computed on the device).
 * params: HOST memory, read during the call only. All arithmetic is fp32 with one rounding per operation and no contraction, divisions correctly
 * rounded.
 * A step. For stream b, with W, H the size in the frame's record, the rows j < min(max(counts[b], 0), d) in ascending order:
 *   1. (x1, y1, x2, y2) = boxes[b][j]. The row is a candidate iff select is NULL or select[b][j] != 0, all four coordinates are finite,
 *      w = x2 - x1 > 0 and h = y2 - y1 > 0;
 *   2. the margin: mx = w * margin, my = h * margin, xa = x1 - mx, xb = x2 + mx, ya = y1 - my, yb = y2 + my;
 *   3. with `square`: cw = xb - xa, ch = yb - ya, s = fmaxf(cw, ch), hs = s * 0.5f, cx = (xa + xb) * 0.5f, cy = (ya + yb) * 0.5f,
 *      xa = cx - hs, xb = cx + hs, ya = cy - hs, yb = cy + hs;
 *   4. the row is dropped if any of xa, xb, ya, yb is not finite, or if the rectangle does not meet the frame: it must satisfy
 *      xb > 0 && xa < (float)W && yb > 0 && ya < (float)H;
 *   5. the integer rectangle, clamped in float first and then converted: X0 = (int)fminf(fmaxf(floorf(xa), 0), W - 1),
 *      X1 = (int)fminf(fmaxf(ceilf(xb), X0 + 1), W), Y0 and Y1 likewise with ya, yb, H; width = X1 - X0, height = Y1 - Y0. The row is skipped if
 *      width < min_width or height < min_height. (Frame 260 x 200, margin 0: the box (10.2, 20.7, 30.1, 40.0) gives (X0, Y0, width, height) =
 *      (10, 20, 21, 20).) For a frame side above 2^24, where W - 1 is not exact in fp32, the integers are clamped once more to the same bounds;
 *   6. the surviving rows are numbered s = 0, 1, ... in the order (stream ascending, row ascending). Rows with s < capacity are kept.
 *      totals_out_dev = (kept, dropped, 0, 0) int32; dropped counts the survivors at or beyond capacity;
 *   7. index_out_dev [capacity][8] int32: for every kept s the row (b, j, X0, Y0, width, height, 0, 0); the rows at or beyond kept are
 *      (-1, 0, 0, 0, 0, 0, 0, 0);
 *   8. patches_out_dev [capacity][3][out_h][out_w], NCHW, channels R, G, B, fp32 or fp16: for every kept s the value v at (c, oy, ox) is exactly
 *      what dn_forward_regions computes for the region (b, X0, Y0, width, height, 0) at the output size out_h x out_w: the tap conversion of
 *      dn_forward_frames, /255, the bilinear resize in REGION coordinates with the second tap clamped at the rectangle's edge, chroma sampled
 *      in frame coordinates, and one tap with the same bits where the rectangle has exactly the patch size. The stored value is
 *      o = (v - mean[c]) / std[c]: one subtraction, then one correctly rounded division (torchvision Normalize's order; no reciprocal, no fused
 *      scale and bias). fp16 output is the round-to-nearest-even conversion of o.
 *      PATCHES AT OR BEYOND kept ARE NOT WRITTEN: they keep whatever the memory held (zeroing 8192 unused slots would cost more than the work).
 * Consequence: with mean = 0, std = 1 and fp32 output, patch s equals, bit for bit, what dn_forward_u8 computes as its network input from the
 * rectangle cut out of the converted frame.
 * TRUST BOUNDARY: the frame table is trusted as for dn_forward_frames. Box values are NOT: whatever bits boxes_dev, counts_dev and select_dev hold,
 * no read leaves the frame, because step 5 clamps the rectangle against the record's own width and height and counts is clamped to 0 .. d.
 * Limits: streams 1 .. 1024, d 1 .. 512, capacity 1 .. 8192, out_h and out_w 1 .. 1024, a known format and colour code (dn_forward_frames'):
 * DN_E_UNSUPPORTED beyond them (dn_crop_workspace_bytes then returns 0). DN_E_INVALID for null pointers (select_dev excepted), non-positive sizes,
 * a margin that is NaN, negative or infinite, a std that is not finite and positive, a mean that is not finite, square or out_fp16 not 0 or 1,
 * min_width or min_height below 1, non-zero reserved words, boxes, patches, index, totals or the workspace not 16-byte aligned, counts not 4-byte
 * aligned. DN_E_WORKSPACE for workspace_bytes below dn_crop_workspace_bytes(streams, d). Every error is raised before anything is launched.
 * Two launches: one workgroup per stream runs steps 1-5 and numbers the stream's survivors with a prefix scan; capacity x row-band workgroups then
 * find their slot's stream from the per-stream counts and write index, totals and patches. Asynchronous on `stream`, no host synchronisation, can
 * be captured (all tables are read when the kernels run); no float atomics; deterministic (the same bits on every run). */
typedef struct dn_crop_params {      /* 64 bytes, HOST memory, read during the call only */
    float   margin;                  /* >= 0, finite: the box grows by margin * its width / height on each side */
    int32_t square;                  /* 0 | 1: after the margin, grow the shorter side to the longer one about the centre */
    int32_t min_width, min_height;   /* >= 1: rectangles smaller than this (after clamping to the frame) are skipped */
    float   mean[3], std[3];         /* per channel R, G, B; std finite and > 0 */
    int32_t out_h, out_w;            /* the patch size, 1 .. 1024 each */
    int32_t out_fp16;                /* 0: fp32 patches, 1: fp16 (round to nearest even of the fp32 value) */
    int32_t capacity;                /* patch slots, 1 .. 8192 */
    int32_t reserved[2];             /* 0 */
} dn_crop_params;
DN_API size_t dn_crop_workspace_bytes(int streams, int d);
DN_API int dn_crop_objects(const dn_frame* frames_dev, int format, int color,
                           const float* boxes_dev, const int32_t* counts_dev, const uint8_t* select_dev, int streams, int d,
                           const dn_crop_params* params, void* patches_out_dev, int32_t* index_out_dev, int32_t* totals_out_dev,
                           void* workspace_dev, size_t workspace_bytes, void* stream);

/* Camera-motion compensation for the trackers (csrc/motion.hip): the third part of BoT-SORT (Aharon et al. 2022). The trackers' filter
 * is constant-velocity in image coordinates, which is right for a fixed camera only; dn_motion_estimate measures the global motion of the image
 * between a stream's previous and current frame from the luma of the surfaces, and dn_track_compensate applies it to the tracker's state in front
 * of that frame's dn_track_update. demonet_amd/motion.py (MotionCompensator) and ByteTracker.compensate are the callers; tests/motion_ref.py
 * restates these sentences in numpy.
 * The model, per stream and frame step, previous frame -> current frame: x' = s x + tx, y' = s y + ty -- translation and isotropic scale. Rotation
 * is deliberately left out: the filter is kept as four independent 2 x 2 blocks (dn_track_update), and only a transform that does not mix cx with cy
 * preserves that structure.
 * a. The luma thumbnail of a frame of W x H pixels, with (TH, TW) = (max_h, max_w) the capacity: k = the smallest integer >= 1 with
 *    floor(W / k) <= TW and floor(H / k) <= TH; the thumbnail is th x tw = floor(H / k) x floor(W / k); pixel (i, j) is the rounded integer mean
 *    (sum + floor(k k / 2)) / (k k) (integer division) of the 8-bit luma of the frame pixels x = k i .. k i + k - 1, y = k j .. k j + k - 1. The
 *    remainder columns and rows at the right and the bottom are ignored. Luma: NV12 / I420 the Y byte as it lies (no range expansion); RGB24 /
 *    BGR24 (77 R + 150 G + 29 B + 128) >> 8. k is at most 4096 (k k 255 < 2^32: the sum is a uint32); a frame beyond that has no blocks.
 * b. Block vectors. With B = block, r = radius: if tw < B + 2 r or th < B + 2 r the frame has no blocks; otherwise nbx = floor((tw - 2 r) / B) by
 *    nby = floor((th - 2 r) / B) blocks, block n = nbx * by_index + bx_index at the corner (bx, by) = (r + B bx_index, r + B by_index) of the CURRENT
 *    thumbnail. It is searched in the PREVIOUS thumbnail over all (dx, dy) in [-r, r]^2: SAD(dx, dy) = the sum over the block's pixels (i, j) of
 *    |cur(bx + i, by + j) - prev(bx + dx + i, by + dy + j)|. The winner is the minimum of the total order (SAD, dx dx + dy dy, dy, dx). A block is
 *    invalid if (1) its texture sum |p - m| over its pixels p, m = (sum p + B B / 2) / (B B), is below min_texture, or (2) its centre lies inside a
 *    masking detection box: with cx = (float)(k (bx + B / 2)) - 0.5f and cy likewise, a row j < min(max(counts[b], 0), d) with score >= mask_thresh
 *    (a NaN score masks nothing), four finite coordinates and x1 <= cx < x2 and y1 <= cy < y2. boxes, scores, counts all NULL: no masking.
 * c. The fit. mdx, mdy = the lower medians (rank floor((valid - 1) / 2) in ascending order) of the valid blocks' dx and dy; the inliers are the
 *    valid blocks with max(|dx - mdx|, |dy - mdy|) <= 2. A block centre u = (bx + B / 2, by + B / 2) of the current thumbnail corresponds to u + d in
 *    the previous one: the fitted pairs are (x, y) = u + d -> (x', y') = u. Over the inliers, exact int64 sums n, Sx, Sy, Sx', Sy', Sqq = sum (x x +
 *    y y), Sxx = sum (x x' + y y'); num = n Sxx - Sx Sx' - Sy Sy', den = n Sqq - Sx Sx - Sy Sy, each converted to float64 once; s = num / den;
 *    tu = (Sx' - s Sx) / n, tv = (Sy' - s Sy) / n in float64 in that order; to frame coordinates tx = k tu + ((1 - s) (k - 1)) / 2, ty likewise,
 *    float64; s, tx, ty are then rounded to fp32 once.
 *    The step is NOT ok, and the motion is the identity (1, 0, 0), when: it is the stream's first frame since the reset; the frame's size differs
 *    from the stored thumbnail's frame; valid < min_blocks; 2 inliers < valid; den = 0; s < 0.8 or s > 1.25 (the float64 s). In the first two cases
 *    no block is searched: every vector row is 0 and valid = inliers = 0. The new thumbnail replaces the stored one in every case.
 * Outputs: motion_out [n][4] fp32 (s, tx, ty, ok = 1 | 0); stats_out [n][4] int32 (blocks, valid, inliers, k); vectors_out [n][max_blocks][4] int32
 * (dx, dy, sad, valid) or NULL, max_blocks = floor((TW - 2 r) / B) floor((TH - 2 r) / B), rows at or beyond the frame's blocks 0.
 * The state, dn_motion_state_bytes(streams, params) bytes, 16-byte aligned, per stream 16 + 16 max_blocks + 2 TH TWp bytes, TWp = TW rounded up to
 * a multiple of 16, streams back to back: int32 parity, have, height, width (of the stored thumbnail's frame); the step's vectors [max_blocks][4]
 * int32; two thumbnails of TH rows of TWp bytes. Thumbnail `parity` is the stored (previous) one; a step writes the other and flips the word last,
 * which is why the step's arguments never change and a captured graph replays. Only th x tw bytes of a thumbnail mean anything. dn_motion_reset
 * zeroes the streams b with which_dev[b] != 0 (NULL: all); a new state must be reset before its first step.
 * d. dn_track_compensate: for every stream b with motion[b].ok != 0 and every slot whose state is not free (dn_track_update's state block; its
 *    layout does not change), fp32, one rounding per operation, no contraction, s2 = s * s: cx: x = s * x + tx (one multiply, then one add);
 *    cy: the same with ty; h: x = s * x; a: untouched; for cx, cy and h: v = s * v, Pxx = Pxx * s2, Pxv = Pxv * s2, Pvv = Pvv * s2. A stream whose
 *    step is not ok is not written at all. It runs BEFORE that frame's dn_track_update: F commutes with the transform, so warp-then-predict equals
 *    BoT-SORT's predict-then-warp in exact arithmetic (Q is then computed from the already scaled h: a rounding-level difference). Zone geometry
 *    (dn_zone_update) is in image coordinates and is not warped.
 * TRUST BOUNDARY: the frame table is trusted as for dn_forward_frames; box values are not (they are only compared).
 * Limits: block 8 | 16, radius 1 .. 16, capacity sides block + 2 radius .. 512, n and streams 1 .. 65535, d 1 .. 512 with masking, max_tracks
 * 1 .. 256: DN_E_UNSUPPORTED beyond the capacity, stream, d and max_tracks limits and for an unknown format (dn_motion_state_bytes then returns 0).
 * DN_E_INVALID for null pointers (the optional ones excepted), some but not all of boxes / scores / counts, non-positive sizes, a bad block or
 * radius, min_texture < 0, min_blocks < 1, a NaN mask_thresh, a non-zero reserved word, the state, boxes, motion, stats or vectors not 16-byte
 * aligned. DN_E_WORKSPACE for state_bytes below the state's size. Every error is raised before anything is launched. dn_motion_estimate is three
 * launches (thumbnails, block match, fit), dn_track_compensate one; asynchronous on `stream`, no host synchronisation, can be captured (the frame
 * table is read when the kernels run); no float atomics; deterministic (the same bits on every run). params is HOST memory, read during the call. */
typedef struct dn_motion_params {    /* 32 bytes, HOST memory */
    int32_t max_h, max_w;            /* the thumbnail capacity (TH, TW): 144, 256 */
    int32_t block;                   /* 8 | 16 */
    int32_t radius;                  /* 1 .. 16 */
    int32_t min_texture;             /* >= 0: 2 * block * block */
    int32_t min_blocks;              /* >= 1: 8 */
    float   mask_thresh;             /* 0.5 */
    int32_t reserved;                /* 0 */
} dn_motion_params;
#ifdef __cplusplus
static_assert(sizeof(dn_motion_params) == 32, "dn_motion_params is 32 bytes");
#else
_Static_assert(sizeof(dn_motion_params) == 32, "dn_motion_params is 32 bytes");
#endif
DN_API size_t dn_motion_state_bytes(int streams, const dn_motion_params* params);
DN_API int dn_motion_reset(void* state_dev, size_t state_bytes, int streams, const dn_motion_params* params, const uint8_t* which_dev, void* stream);
DN_API int dn_motion_estimate(const dn_frame* frames_dev, int n, int format, const dn_motion_params* params, const float* boxes_dev,
                              const float* scores_dev, const int32_t* counts_dev, int d, void* state_dev, size_t state_bytes, float* motion_out_dev,
                              int32_t* stats_out_dev, int32_t* vectors_out_dev, void* stream);
DN_API int dn_track_compensate(void* track_state_dev, size_t track_state_bytes, int streams, int max_tracks, const float* motion_dev, void* stream);

/* On-screen display on the device (csrc/osd.hip): track boxes, class / id / score labels, counting lines, zone edges and redaction
 * (pixelation, opaque fill) painted IN PLACE into the surfaces a dn_frame table names, in the surfaces' own colour space, without a box or an id
 * visiting the host. demonet_amd/osd.py (Overlay) is the caller; tests/osd_ref.py restates these sentences in numpy.
 * Surfaces. frames_dev: [n] dn_frame records (format: dn_forward_frames' codes); stream b paints frame b; width, height, planes and pitches come from
 * the records in device memory. Colours are bytes in the surface's own space in logical order: (Y, U, V) for NV12 / I420, (R, G, B) for RGB24 /
 * BGR24 -- the kernel swaps R and B for BGR24. The device never converts a colour; the caller does, once per palette (Python: Y = ((yr R + yg G +
 * yb B + 2^13) >> 14) + yo, U = ((ur R + ug G + ub B + 2^13) >> 14) + 128, V likewise, >> arithmetic, clamped to 0 .. 255, every coefficient
 * round(c 2^14) of the BT.601 / BT.709 forward matrix in limited (219/255, 224/255, yo = 16) or full range).
 * One pixel, one owner. A pixel's value starts as the frame's value before the call; the primitives that cover the pixel are applied in the fixed
 * order below, later ones over earlier ones. A blend is per component with an exact integer division: out = (a c + (255 - a) p + 127) / 255, a the
 * alpha, c the colour, p the current value. In the 4:2:0 formats chroma sample (cx, cy) is governed by luma pixel (2 cx, 2 cy) (dn_forward_frames'
 * (x >> 1, y >> 1)): U and V receive exactly the primitives that cover that pixel, in the same order with the same alpha. Odd frame sizes are
 * legal. The bytes of uncovered pixels, every byte of a pitch gap and everything of a frame no primitive touches keep their value; a workgroup may
 * store back the value it read for an uncovered payload byte of a 32 x 32 tile it owns, nowhere else.
 * Order, per stream: 1. the lines and zone edges of the stream's dn_zone_config: lines ascending, then zones ascending with edges ascending;
 * 2. the boxes, rows ascending, within a row pixelate, then fill, then outline; 3. the labels, rows ascending.
 * Rows. boxes_dev [n][d][4] fp32, scores_dev [n][d] fp32, labels_dev [n][d] int64, ids_dev [n][d] int64 or NULL, counts_dev [n] int32: a tracker's
 * outputs or raw detections. Row j is used iff j < min(max(counts[b], 0), d), its four coordinates are finite, its label lies in [0, n_labels) and its
 * style has no DN_OSD_HIDE. Its rectangle: ix0 = floor(x1), iy0 = floor(y1), ix1 = ceil(x2), iy1 = ceil(y2), each clamped AS A FLOAT to [0, W]
 * or [0, H] before the conversion to int; a row whose rectangle is empty (ix0 >= ix1 or iy0 >= iy1) is skipped. Its style is styles_dev[label], an
 * 8-byte dn_osd_style (NULL table: params->default_style for every row); a thickness above 16 counts as 16, a pixelate block that is not 4, 8, 16
 * or 32 as 0. Its colour is palette_dev[key % n_colors], key = the low 32 bits, unsigned, of the id when ids are given and params->color_by_id,
 * else of the label; the palette holds n_colors (1 .. 256) dn_osd_color records.
 *   outline, thickness t > 0: the rectangle minus the rectangle shrunk by t on every side; when the shrunk rectangle is empty the whole rectangle.
 *     Opaque (the colour replaces the value).
 *   fill: the rectangle, blended with the style's fill_alpha.
 *   pixelate, block s: blocks are anchored at the frame origin. A covered pixel takes (sum + cnt / 2) / cnt (integer division) over its block
 *     intersected with the frame, per plane (per channel for RGB); in 4:2:0 a governed chroma sample takes the mean of its (s/2) x (s/2) chroma
 *     block intersected with the ceil-sized chroma plane. The sum is ALWAYS over the frame as it was before the call, never over painted values.
 * Labels. A row whose style has DN_OSD_LABEL gets a text, built on the device: the class name names_dev[label] (16 bytes, NUL-padded, at most 15
 * characters; a NULL table: no name); with ids, " #" and the id's decimal digits, or "?" for an id outside 0 .. 999 999 999; with DN_OSD_SCORE,
 * " " p "%", p = (int) of v = score * 100.f + 0.5f clamped as a float to 0 .. 100, or "?" for a non-finite score. At most 31 characters. font_dev:
 * [64][8] uint8, the glyphs of ASCII 32 .. 95, bit 7 - c of row byte r is column c; a lowercase letter takes the uppercase glyph, every other byte
 * outside 32 .. 95 takes '?'. At scale k (1 .. 4) the label rectangle is 8 k len wide and 8 k high at left = ix0, top = iy0 - 8 k when iy0 >= 8 k,
 * else iy0, cut at the frame's edges. Pixel (x, y) of it: column (x - left) / k, row (y - top) / k, character = column >> 3; a set glyph bit takes
 * the palette entry's text colour, a clear one its colour, both blended with label_alpha.
 * Segments. zone_config_dev: ZoneAnalytics' own [n] dn_zone_config, read where it lies, or NULL; n_lines, n_zones and nv are clamped as in
 * dn_zone_update. Line i is A = (ax, ay) -> B = (bx, by); edge e of a zone is A = verts[e] -> B = verts[(e + 1) % nv]. A segment covers the pixel
 * with centre p = (x + 0.5, y + 0.5) by this test in fp32, one rounding per operation, in this order: dx = bx - ax, dy = by - ay, L = dx*dx + dy*dy
 * (L == 0 or not finite: the segment is skipped); t = ((px - ax)*dx + (py - ay)*dy) / L clamped to [0, 1]; qx = ax + t*dx, qy = ay + t*dy;
 * ex = px - qx, ey = py - qy; covered iff ex*ex + ey*ey <= r*r, r = (float)thickness * 0.5f. Lines take line_color, zone edges zone_color, both
 * blended with zone_alpha.
 * Two launches. Launch 1, one workgroup per stream: validates the rows, makes the rectangles, formats the label
 * bytes, compacts the live primitives in paint order, marks the 32 x 32 tiles (anchored at the origin) each primitive can touch -- rectangles
 * exactly, segments by a bounding box grown by the radius -- and appends the marked tiles to one work list through one integer atomic per
 * workgroup. Every tile is independent, so the list's order may vary without changing a byte. Launch 2, a fixed grid of persistent workgroups,
 * walks the list: per tile it snapshots the planes into LDS before it writes anything (every pixelate block lies inside one tile: in place is
 * race-free), paints each 2 x 2 luma quad with its chroma pair in one thread, and stores. Traffic is proportional to the tiles touched.
 * The workspace, dn_osd_workspace_bytes(n, d, tile_capacity) bytes, 16-byte aligned. ITS FIRST 16 BYTES MUST BE ZERO BEFORE THE FIRST CALL: bytes
 * 0 .. 7 are the tile counter (64 bits: no sum of tiles over the streams wraps), word 3 counts the finished workgroups of launch 2, whose last one
 * clears both again and leaves word 2 int32 = the tiles the call marked (kept and dropped, saturated at 2^31 - 1). RECOVERY: when a call returns
 * DN_E_HIP (a launch could not be enqueued), when a graph holding the call is abandoned half way, or when the memory is reused for anything else,
 * zero the first 16 bytes again before the next call (an ordinary fill on the same stream); until then later calls would append behind stale
 * entries and drop tiles. A frame is taken to have fewer than 2^31 tiles (the per-stream figures of stats_dev are int32).
 * The work list, [tile_capacity] pairs of int32 (stream, ty * ceil(W / 32) + tx), starts at byte dn_osd_workspace_bytes(n, d, 0).
 * tile_capacity of a call = (workspace_bytes - dn_osd_workspace_bytes(n, d, 0)) / 8; tiles beyond it are dropped, counted and never written.
 * stats_dev [n][4] int32: rows painted, rows skipped (of the j < min(max(count, 0), d)), tiles touched, tiles dropped.
 * TRUST BOUNDARY: the frame table is trusted as for dn_forward_frames (a frame wider than 2^21 pixels is not painted). Boxes, scores, labels, ids,
 * counts, the zone config, the style bytes and the name bytes are NOT: whatever they hold, no access leaves the frames or the tables' sizes.
 * DN_E_INVALID for null pointers (ids_dev, styles_dev, zone_config_dev excepted, and names_dev when styles_dev is given or the default style has no
 * DN_OSD_LABEL), n, d or n_labels < 1, boxes / workspace / stats / zone config not 16-byte aligned, labels / ids / styles / palette not 8-byte,
 * scores / counts not 4-byte aligned, scale outside 1 .. 4, line or zone thickness outside 1 .. 64, a default thickness above 16 or block not 0, 4,
 * 8, 16, 32, n_colors outside 1 .. 256, an alpha outside 0 .. 255, non-zero reserved words, an unknown format. DN_E_UNSUPPORTED for d > 512 or
 * n > 65535 (dn_osd_workspace_bytes then returns 0). DN_E_WORKSPACE for workspace_bytes below dn_osd_workspace_bytes(n, d, 1). Every error is raised
 * before anything is enqueued. Asynchronous on `stream`, no host synchronisation, can be captured (every table is read when the kernels run); no
 * float atomics; deterministic (the same bits on every run). params is HOST memory, read during the call. */
enum { DN_OSD_LABEL = 1, DN_OSD_SCORE = 2, DN_OSD_HIDE = 4 };
typedef struct dn_osd_style {        /* 8 bytes, DEVICE memory (styles_dev[n_labels]) and inside dn_osd_params */
    uint8_t thickness;               /* outline, 0 .. 16 pixels; 0: none */
    uint8_t fill_alpha;              /* 0: no fill .. 255: opaque */
    uint8_t pixelate;                /* block: 0 (off), 4, 8, 16 or 32 */
    uint8_t flags;                   /* DN_OSD_LABEL | DN_OSD_SCORE | DN_OSD_HIDE */
    uint8_t reserved[4];
} dn_osd_style;
typedef struct dn_osd_color {        /* 8 bytes, DEVICE memory (palette_dev[n_colors]) */
    uint8_t color[3];                /* surface space, logical order */
    uint8_t text[3];                 /* the text's colour on it */
    uint8_t reserved[2];
} dn_osd_color;
typedef struct dn_osd_params {       /* 64 bytes, HOST memory */
    dn_osd_style default_style;      /* the style of every row when styles_dev is NULL */
    int32_t n_colors;                /* 1 .. 256 */
    int32_t color_by_id;             /* 0 | 1 */
    int32_t scale;                   /* 1 .. 4: a character cell is 8 scale x 8 scale */
    int32_t label_alpha;             /* 0 .. 255 */
    int32_t line_thickness;          /* 1 .. 64 */
    int32_t zone_thickness;          /* 1 .. 64 */
    int32_t zone_alpha;              /* 0 .. 255, lines and zone edges */
    uint8_t line_color[3], reserved0;
    uint8_t zone_color[3], reserved1;
    int32_t reserved[5];             /* 0 */
} dn_osd_params;
#ifdef __cplusplus
static_assert(sizeof(dn_osd_params) == 64 && sizeof(dn_osd_style) == 8 && sizeof(dn_osd_color) == 8, "dn_osd_params is 64 bytes, its records 8");
#else
_Static_assert(sizeof(dn_osd_params) == 64 && sizeof(dn_osd_style) == 8 && sizeof(dn_osd_color) == 8, "dn_osd_params is 64 bytes, its records 8");
#endif
DN_API size_t dn_osd_workspace_bytes(int streams, int d, int tile_capacity);
DN_API int dn_osd_paint(const dn_frame* frames_dev, int n, int format, const float* boxes_dev, const float* scores_dev, const int64_t* labels_dev,
                        const int64_t* ids_dev, const int32_t* counts_dev, int d, const dn_osd_style* styles_dev, int n_labels,
                        const uint8_t* names_dev, const dn_osd_color* palette_dev, const uint8_t* font_dev, const dn_zone_config* zone_config_dev,
                        const dn_osd_params* params, void* workspace_dev, size_t workspace_bytes, int32_t* stats_dev, void* stream);

/* Surface composition on the device (csrc/compose.hip): rectangles of the surfaces of one dn_frame table are scaled, converted and
 * written into rectangles of the surfaces of another -- 64 painted streams into one wall surface, a preview per camera, NV12 to RGB for a snapshot,
 * pitched BGR to NV12 for an encoder. demonet_amd/compose.py (Compositor) is the caller; tests/compose_ref.py restates these sentences in numpy.
 * Tables. src_frames_dev / dst_frames_dev: dn_frame tables (formats and colour codes: dn_forward_frames'), every record of a table in the table's
 * format; the destination surfaces are written. table_dev: a 16-byte dn_compose_header followed by `capacity` 48-byte dn_compose_item records, in
 * DEVICE memory, read WHEN THE KERNEL RUNS: the call's arguments are addresses and the capacity only, so a captured graph follows new surfaces, new
 * items and a new item count without a recapture. Item i copies the rectangle (sx0, sy0, sw, sh) of frame `src` of the source table to the rectangle
 * (dx0, dy0, dw, dh) of frame `dst` of the destination table. tile0 is the item's first tile in the call's work list: tile0[0] = 0, tile0[i + 1] =
 * tile0[i] + ceil(dw_i / 32) ceil(dh_i / 32), and header.n_tiles is the total; the caller computes them when it writes the table.
 * Resampling is an exact area (box) filter per plane sample, in integers. Along x, for destination column j of dw over a source extent of sw, the weight
 * of source column s is the length of [j sw, (j + 1) sw) intersected with [s dw, (s + 1) dw); the weights of a column sum to sw. Along y likewise with
 * sh, dh. out = (sum over y, x of wy wx p + D / 2) / D with D = sw sh, integer division: the mean rounded half up. sw sh <= 2^24, so the unsigned
 * 32-bit sum is exact. A 1:1 item is a byte copy; an upscale is nearest with blended seams.
 * Plane-wise path: source and destination both NV12 / I420 (in any combination) AND src_color == dst_color. The Y plane is resampled from the source
 * rectangle to the destination rectangle; U and V with the same filter from the chroma rectangle (sx0 / 2, sy0 / 2, ceil(sw / 2), ceil(sh / 2)) to
 * (dx0 / 2, dy0 / 2, ceil(dw / 2), ceil(dh / 2)). No colour arithmetic; 1.5 bytes per source pixel are read.
 * RGB path: every other pair (RGB / BGR <-> RGB / BGR, YUV -> RGB, RGB -> YUV, YUV -> YUV across matrix or range). Each source pixel becomes RGB8 by
 * dn_forward_frames' integer formulas with src_color, its chroma sample (x >> 1, y >> 1) in FRAME coordinates; R, G and B are area-resampled per
 * channel to one RGB8 per destination pixel. An RGB24 / BGR24 destination stores that RGB8. A YUV destination computes Y per pixel from its RGB8, and
 * U, V per chroma sample from the per-channel mean, rounded half up ((sum + n / 2) / n), of the destination RGB8 pixels that lie in both its 2 x 2
 * block and the rectangle (n = 1, 2 or 4). Y = clamp(((yr R + yg G + yb B + 2^13) >> 14) + yo), U = clamp(((ur R + ug G + ub B + 2^13) >> 14) + 128),
 * V likewise (>> arithmetic, clamp to 0 .. 255), every coefficient round(c 2^14) of the BT.601 / BT.709 forward matrix of dst_color in limited
 * (219/255, 224/255, yo = 16) or full range: dn_osd_paint's colour formula.
 * One byte, one owner. For a YUV source sx0 and sy0 are even, for a YUV destination dx0 and dy0; rectangles lie wholly inside their frames; the
 * destination rectangles of one destination surface do not overlap, their chroma footprints (dx0 / 2, dy0 / 2, ceil(dw / 2), ceil(dh / 2)) neither.
 * Hence the result does not depend on the order of the work and is the same on every run. The bytes of a pitch gap and every payload byte of a
 * destination no item covers keep every bit. Source and destination surfaces must not share memory.
 * TRUST BOUNDARY: THE LIBRARY CANNOT INSPECT A DEVICE TABLE AND TRUSTS ALL THREE, THE ITEM TABLE EXACTLY LIKE dn_region: 0 <= n_items <= capacity,
 * every index inside its frame table, every rectangle inside its frame with sides 1 .. 32768, sw sh <= 2^24, the parity and overlap rules above,
 * tile0 and n_tiles (< 2^31) as defined, reserved words 0; a wrong record is an out-of-bounds device read or WRITE. Validate on the host before the
 * records go up (Python: compose.Compositor.set, which also remembers both tables' sizes and refuses a call after they changed).
 * One launch of persistent workgroups, asynchronous on `stream`, no host wait, no atomics; can be captured. DN_E_INVALID for a null table, frame tables
 * not 8-byte or an item table not 16-byte aligned, capacity < 1, an unknown format or colour code; DN_E_UNSUPPORTED for capacity > 65536. Every error
 * is raised before anything is enqueued.
 * dn_surface_fill writes the PAYLOAD of the n whole surfaces of a table, not the gaps, with one colour: c0, c1, c2 are bytes (0 .. 255) in the
 * surfaces' own space in logical order, (Y, U, V) or (R, G, B) as for dn_osd_paint; the caller converts. One launch, asynchronous, can be captured.
 * DN_E_INVALID for a null or misaligned table, n < 1, an unknown format, a byte outside 0 .. 255; DN_E_UNSUPPORTED for n > 65535. */
typedef struct dn_compose_item {     /* 48 bytes, DEVICE memory */
    int32_t src;                     /* index into the source dn_frame table */
    int32_t sx0, sy0, sw, sh;        /* the source rectangle, in that frame's pixels */
    int32_t dst;                     /* index into the destination dn_frame table */
    int32_t dx0, dy0, dw, dh;        /* the destination rectangle */
    int32_t tile0;                   /* the item's first 32 x 32 tile in the work list (see above) */
    int32_t reserved;                /* 0 */
} dn_compose_item;
typedef struct dn_compose_header {   /* 16 bytes, DEVICE memory, directly in front of the items */
    int32_t n_items;                 /* 0 .. capacity */
    int32_t n_tiles;                 /* the sum of the items' tiles */
    int32_t reserved[2];             /* 0 */
} dn_compose_header;
#ifdef __cplusplus
static_assert(sizeof(dn_compose_item) == 48 && sizeof(dn_compose_header) == 16, "dn_compose_item is 48 bytes, dn_compose_header 16");
#else
_Static_assert(sizeof(dn_compose_item) == 48 && sizeof(dn_compose_header) == 16, "dn_compose_item is 48 bytes, dn_compose_header 16");
#endif
DN_API int dn_compose(const dn_frame* src_frames_dev, int src_format, int src_color, const dn_frame* dst_frames_dev, int dst_format, int dst_color,
                      const dn_compose_header* table_dev, int capacity, void* stream);
DN_API int dn_surface_fill(const dn_frame* frames_dev, int n, int format, int c0, int c1, int c2, void* stream);

/* Surface dewarping on the device (csrc/warp.hip): rectangles of the surfaces of one dn_frame table are filled from the surfaces of
 * another through a coordinate mesh, with a bilinear filter -- virtual PTZ views and panoramas of a fisheye, lens undistortion, homographies, quarter
 * turns, mirrors, bilinear scaling. demonet_amd/warp.py (Warper, and the host-side mesh builders) is the caller; tests/warp_ref.py restates these
 * sentences in numpy integers, and the device matches them bit for bit. Both tables have the SAME format (`format`: dn_forward_frames' codes) and the
 * same colour space: the remap works plane by plane on the stored bytes, colour conversion is dn_compose's job.
 * Tables. table_dev: a 16-byte dn_warp_header followed by `capacity` 48-byte dn_warp_item records, in DEVICE memory, read WHEN THE KERNEL RUNS, like
 * the frame tables and the meshes: a captured graph follows new surfaces, new items, new meshes and a new item count. Item i fills the rectangle
 * (dx0, dy0, dw, dh) of frame `dst` of the destination table from frame `src` of the source table. tile0 and header.n_tiles are dn_compose's:
 * tile0[0] = 0, tile0[i + 1] = tile0[i] + ceil(dw_i / 32) ceil(dh_i / 32).
 * Mesh. mesh_dev: int32 [M][2], every mesh of the call; header.n_points = M. The mesh of an item is the mw x mh points, row-major, from point mesh0
 * on, mw = mesh_w = ceil(dw / DN_WARP_CELL) + 1, mh = ceil(dh / DN_WARP_CELL) + 1; items may share a mesh. Point (cx, cy) = (X, Y) is the source
 * position of rectangle pixel (8 cx, 8 cy) in units of 1/64 source pixel; coordinates are pixel indices, an integer is a pixel centre;
 * |X|, |Y| <= 2^21 - 1. The points past the rectangle's end are part of the mesh.
 * Luma and packed RGB / BGR pixel (x, y) of the rectangle: cx = x >> 3, i = x & 7, cy = y >> 3, j = y & 7; A, B, C, D the points (cx, cy),
 * (cx + 1, cy), (cx, cy + 1), (cx + 1, cy + 1); per coordinate
 *     P = (8 - j) ((8 - i) A + i B) + j ((8 - i) C + i D)          in 1/4096 pixel, |P| < 2^27
 *     q = (P + 64) >> 7                                            in 1/32 pixel; >> of a signed value: arithmetic (floor)
 *     x0 = qx >> 5, fx = qx & 31, y0 = qy >> 5, fy = qy & 31; taps p00 = (x0, y0), p01 = (x0 + 1, y0), p10 = (x0, y0 + 1), p11 = (x0 + 1, y0 + 1)
 *     out = ((32 - fx) (32 - fy) p00 + fx (32 - fy) p01 + (32 - fx) fy p10 + fx fy p11 + 512) >> 10        per byte channel
 * Chroma sample (cxs, cys) of a 4:2:0 rectangle; the chroma rectangle is (dx0 / 2, dy0 / 2, ceil(dw / 2), ceil(dh / 2)) as for dn_compose, the siting
 * centred: the sample sits at luma position (2 cxs + 0.5, 2 cys + 0.5). With x = 2 cxs, y = 2 cys: cx = x >> 3, i2 = 2 (x & 7) + 1, cy = y >> 3,
 * j2 = 2 (y & 7) + 1,
 *     P2 = (16 - j2) ((16 - i2) A + i2 B) + j2 ((16 - i2) C + i2 D)    in 1/16384 luma pixel, |P2| < 2^29
 *     qc = ((P2 + 512) >> 10) - 8                                      in 1/32 chroma sample
 * taps and blend as above on the chroma plane(s) of ceil(W / 2) x ceil(H / 2) samples; NV12 reads U and V at the same taps.
 * Hence an identity mesh is a byte copy of every plane, and quarter turns and mirrors are exact permutations of every plane for even-sized 4:2:0
 * frames and for RGB of any size. There is no anti-aliasing filter: minify strongly with dn_compose's area filter behind the warp.
 * Border. Every tap is tested on its own against its plane, 0 <= x < W, 0 <= y < H. flags = DN_WARP_BORDER_CONSTANT: a tap outside takes the item's
 * border byte of that plane or channel, border = c0 | c1 << 8 | c2 << 16 with (c0, c1, c2) = (Y, U, V) for NV12 / I420 and the three bytes of a
 * packed pixel IN MEMORY ORDER for RGB24 / BGR24 (one kernel serves both); DN_WARP_BORDER_REPLICATE: the tap's coordinates are clamped to the plane.
 * Because of these tests NO MESH VALUE CAN MAKE THE KERNEL READ OUTSIDE A SURFACE.
 * One byte, one owner. Destination rectangles lie inside their frames, sides 1 .. 32768; dx0 and dy0 are even on NV12 / I420; the rectangles of one
 * destination surface do not overlap, their chroma footprints neither; source and destination surfaces share no memory. Hence the result does not
 * depend on the order of the work, and the bytes of a pitch gap and every payload byte no item covers keep every bit.
 * TRUST BOUNDARY: THE LIBRARY CANNOT INSPECT A DEVICE TABLE AND TRUSTS THE ITEM TABLE EXACTLY LIKE dn_region: 0 <= n_items <= capacity, every index
 * inside its frame table, the rectangle rules above, mesh0 >= 0 and mesh0 + mw mh <= M with mesh_w = mw, tile0 and n_tiles (< 2^31) as defined,
 * flags 0 or 1, reserved words 0; a wrong record is an out-of-bounds device read or WRITE. Validate on the host before the records go up (Python:
 * warp.Warper.set, which also remembers both tables' sizes and refuses a call after they changed).
 * One launch of persistent workgroups, asynchronous on `stream`, no host wait, no atomics, no workspace; can be captured. DN_E_INVALID for a null
 * pointer, frame tables or a mesh not 8-byte or an item table not 16-byte aligned, capacity <= 0; DN_E_UNSUPPORTED for an unknown format or
 * capacity > 65536. Every error is raised before anything is enqueued. */
#define DN_WARP_CELL 8
enum { DN_WARP_BORDER_CONSTANT = 0, DN_WARP_BORDER_REPLICATE = 1 };
typedef struct dn_warp_item {        /* 48 bytes, DEVICE memory */
    int32_t src;                     /* index into the source dn_frame table */
    int32_t dst;                     /* index into the destination dn_frame table */
    int32_t dx0, dy0, dw, dh;        /* the destination rectangle */
    int32_t mesh0;                   /* the first point of the item's mesh in mesh_dev */
    int32_t mesh_w;                  /* points per mesh row: ceil(dw / 8) + 1 */
    int32_t flags;                   /* DN_WARP_BORDER_* */
    int32_t border;                  /* c0 | c1 << 8 | c2 << 16 (see above) */
    int32_t tile0;                   /* the item's first 32 x 32 tile in the work list */
    int32_t reserved;                /* 0 */
} dn_warp_item;
typedef struct dn_warp_header {      /* 16 bytes, DEVICE memory, directly in front of the items */
    int32_t n_items;                 /* 0 .. capacity */
    int32_t n_tiles;                 /* the sum of the items' tiles */
    int32_t n_points;                /* M, the points of mesh_dev */
    int32_t reserved;                /* 0 */
} dn_warp_header;
#ifdef __cplusplus
static_assert(sizeof(dn_warp_item) == 48 && sizeof(dn_warp_header) == 16, "dn_warp_item is 48 bytes, dn_warp_header 16");
#else
_Static_assert(sizeof(dn_warp_item) == 48 && sizeof(dn_warp_header) == 16, "dn_warp_item is 48 bytes, dn_warp_header 16");
#endif
DN_API int dn_warp(const dn_frame* src_frames_dev, const dn_frame* dst_frames_dev, int format, const void* table_dev, int capacity,
                   const int32_t* mesh_dev, void* stream);

/* Baseline JPEG encoding of surface rectangles on the device (csrc/jpeg.hip): rectangles of the surfaces of a dn_frame table become
 * complete .jpg files (ITU-T T.81 baseline sequential, JFIF 1.01) in one device byte arena -- the snapshot of an event, the thumbnail of a tracked
 * object, a redacted evidence frame. demonet_amd/jpeg.py (JpegEncoder) is the caller; tests/jpeg_ref.py restates these sentences in numpy and
 * integers, with a decoder of its own, and the device matches it byte for byte.
 * Tables. frames_dev: a dn_frame table (format, color: dn_forward_frames' codes). table_dev: a 16-byte dn_jpeg_header followed by `capacity_items`
 * 32-byte dn_jpeg_item records, in DEVICE memory, read WHEN THE KERNELS RUN: the call's arguments are addresses and capacities only, so a captured
 * graph follows new surfaces, new items and a new item count without a recapture. Item i is the rectangle (x0, y0, width, height) of frame `frame`
 * at quality 1 .. 100, or a slot without a file: frame = -1 an empty slot (status 1), -2 a refused rectangle (2), -3 no space in the work list (3),
 * all three with width = height = 0; slots at or beyond n_items are empty. seg0 is the item's first MCU row in the call's work list: seg0[0] = 0,
 * seg0[i + 1] = seg0[i] + ceil(height_i / 16) (a slot without a file has no rows), header.n_segments the total.
 * Components. Three, YCbCr as JFIF defines it (BT.601, full range), 4:2:0: the MCU is 16 x 16, four Y blocks, then Cb, then Cr.
 * Plane-wise path: format NV12 / I420 AND color == DN_COLOR_BT601 | DN_COLOR_FULL_RANGE. The component planes are the stored bytes: Y the rectangle,
 * Cb and Cr the chroma rectangle (x0 / 2, y0 / 2, ceil(width / 2), ceil(height / 2)) -- dn_compose's plane-wise rule, no colour arithmetic.
 * RGB path: every other table. Each pixel becomes RGB8 by dn_forward_frames' integer formulas (chroma sample (X >> 1, Y >> 1) in FRAME coordinates);
 * Y per pixel, Cb and Cr per chroma sample from the rounded-half-up mean of the RGB8 pixels that lie in both its 2 x 2 block of the rectangle and
 * the rectangle, by dn_compose's forward formula with the BT.601 full-range coefficients: the planes a 1:1 dn_compose item into an I420 BT.601
 * full-range surface of width x height would hold. For NV12 / I420 x0 and y0 are even.
 * Edge. Samples of a partial MCU beyond a component plane replicate that plane's last column and last row.
 * Transform. Level shift by -128, then the 8 x 8 forward DCT in integers: the Loeffler-Ligtenberg-Moschytz form, rows then columns, constants
 * round(c 2^13), the row pass scaled up by 2^2, descales rounded half up with an arithmetic shift; the output is 8 times the orthonormal DCT
 * (tests/jpeg_ref.py, fdct, is the statement).
 * Quantisation. The Annex K luminance and chrominance tables scaled by the IJG quality rule in integers: s = q < 50 ? 5000 / q : 200 - 2 q,
 * Q = clamp((base s + 50) / 100, 1, 255); coefficient = sign(c) ((|c| + d / 2) / d) with d = 8 Q. The kernels derive the tables from `quality`.
 * Entropy coding. Zigzag order, the four Annex K "typical" Huffman tables, written into every file; one DC predictor per component; ZRL and EOB as in
 * T.81; bits MSB first, a 0x00 behind every 0xFF data byte. One MCU row is one restart interval: DRI = ceil(width / 16), RSTm with m = row mod 8
 * behind every row but the last, the predictors reset at every row, the last byte of a row padded with 1-bits.
 * File: SOI, APP0 (JFIF 1.01, density 1:1, no thumbnail), one DQT (both 8-bit tables), SOF0, one DHT (DC0, AC0, DC1, AC1), DRI, SOS, data, EOI;
 * the segments in front of the data are 613 bytes.
 * Results. results_dev: [capacity_items][4] int32 rows (offset, length, status, 0); totals_dev: [4] int32 (written, refused, bytes_used, 0) with
 * refused the slots of status 2 or 3 and bytes_used the end of the last written file. Status 0 written, 1 empty slot, 2 rectangle refused, 3 no
 * space. Placement is a pure prefix sum: offset_i is the sum of (length_j + 15) & ~15 over every encodable j < i whether or not j fitted; item i is
 * written iff offset_i + length_i <= arena_bytes, otherwise status 3, length 0, and no byte of the arena is written on its behalf. The bytes of the
 * alignment gaps and everything beyond bytes_used keep their contents. Two calls on equal inputs give equal bytes: no float, no order dependence.
 * Three launches, asynchronous on `stream`, no host wait, can be captured: every MCU row is coded once for its exact stuffed length, one workgroup
 * scans row and file lengths into offsets, results and totals, and every row is coded again at its final place (nothing is sized by a guessed
 * compression ratio). workspace_dev: dn_jpeg_workspace_bytes(capacity_items, max_segments) bytes, 16-byte aligned, for a work list of at most max_segments
 * MCU rows (4 bytes per row and per item); the kernels cut a table whose n_segments exceeds what workspace_bytes holds at that many rows, so that
 * no table makes them write outside the workspace (the rows beyond are not coded: the caller's validation keeps this from happening).
 * TRUST BOUNDARY: THE LIBRARY CANNOT INSPECT A DEVICE TABLE AND TRUSTS THE ITEM TABLE OF dn_jpeg_encode EXACTLY LIKE dn_compose's: 0 <= n_items <=
 * capacity_items, every frame index inside the frame table, every rectangle inside its frame with sides 1 .. 32768, even origins on NV12 / I420,
 * quality 1 .. 100, seg0 and n_segments as defined, reserved words 0; a wrong record is an out-of-bounds device read. Validate on the host before
 * the records go up (Python: jpeg.JpegEncoder.set) -- or let dn_jpeg_items_from_index write the table.
 * DN_E_INVALID for a null table, arena, result or workspace pointer, frame tables not 8-byte or an item table, results, totals or workspace not
 * 16-byte aligned, capacity_items < 1, arena_bytes < 0, an unknown format or colour code, a workspace below
 * dn_jpeg_workspace_bytes(capacity_items, 1); DN_E_UNSUPPORTED for capacity_items > 8192 (dn_jpeg_workspace_bytes then returns 0). Every error is raised before
 * anything is enqueued.
 * dn_jpeg_items_from_index writes such a table from an object cropper's index table (dn_crop_objects): index_dev = [index_rows][8] int32 rows
 * (stream, row, x0, y0, width, height, 0, 0), stream -1 an unused slot; item s is index row s, header.n_items = index_rows, and table_dev holds at
 * least index_rows item records behind its header. THE ROWS ARE NOT
 * TRUSTED: a stream outside [0, n_frames), a side below 1 or above 32768 or a rectangle not wholly inside that frame's record gives status 2. For
 * NV12 / I420 an odd x0 or y0 moves down to the even pixel and that side grows by one. select_dev (may be null): [index_rows] bytes, 0 deselects the
 * slot; unused and deselected slots give status 1. A slot whose rows would push the segment total past max_segments gives status 3 (the total
 * counts every valid slot in front of it, so every valid slot behind it has status 3 too). seg0 comes from a block scan in slot order. One small
 * launch, can be captured. DN_E_INVALID for a null pointer (select_dev excepted), a frame table not 8-byte or an index or item table not 16-byte
 * aligned, n_frames < 1, index_rows < 1, max_segments < 1, quality outside 1 .. 100, an unknown format; DN_E_UNSUPPORTED for index_rows > 8192. */
#define DN_JPEG_MAX_ITEMS 8192
#define DN_JPEG_HEADER_BYTES 613
typedef struct dn_jpeg_item {        /* 32 bytes, DEVICE memory */
    int32_t frame;                   /* index into the dn_frame table; -1, -2, -3: a slot without a file (status 1, 2, 3) */
    int32_t x0, y0, width, height;   /* the rectangle, in that frame's pixels */
    int32_t quality;                 /* 1 .. 100 */
    int32_t seg0;                    /* the item's first MCU row in the work list (see above) */
    int32_t reserved;                /* 0 */
} dn_jpeg_item;
typedef struct dn_jpeg_header {      /* 16 bytes, DEVICE memory, directly in front of the items */
    int32_t n_items;                 /* 0 .. capacity_items */
    int32_t n_segments;              /* the sum of the items' MCU rows, < 2^31 */
    int32_t reserved[2];             /* 0 */
} dn_jpeg_header;
#ifdef __cplusplus
static_assert(sizeof(dn_jpeg_item) == 32 && sizeof(dn_jpeg_header) == 16, "dn_jpeg_item is 32 bytes, dn_jpeg_header 16");
#else
_Static_assert(sizeof(dn_jpeg_item) == 32 && sizeof(dn_jpeg_header) == 16, "dn_jpeg_item is 32 bytes, dn_jpeg_header 16");
#endif
DN_API size_t dn_jpeg_workspace_bytes(int capacity_items, int max_segments);
DN_API int dn_jpeg_encode(const dn_frame* frames_dev, int format, int color, const dn_jpeg_header* table_dev, int capacity_items,
                          uint8_t* arena_dev, int arena_bytes, int32_t* results_dev, int32_t* totals_dev, void* workspace_dev, size_t workspace_bytes,
                          void* stream);
DN_API int dn_jpeg_items_from_index(const dn_frame* frames_dev, int n_frames, int format, const int32_t* index_dev, int index_rows,
                                    const uint8_t* select_dev, int quality, int max_segments, dn_jpeg_header* table_dev, void* stream);

DN_API const char* dn_last_error(void);
DN_API int dn_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DEMONET_HIP_H */
