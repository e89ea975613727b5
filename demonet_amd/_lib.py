"""ctypes binding of include/demonet_hip.h. Fails loudly when the HIP library is missing: there is no CPU fallback."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DEMONET_HIP_LIB") or os.path.join(_HERE, "lib", "libdemonet_hip.so")      # (DEMONET_HIP_LIB: a dev build of the SAME C ABI, e.g. `python -m demonet_amd.build --stamps`)
DN_ABI_VERSION = 1

DN_OP = dict(stem=1, pw=2, dw=3, se=4, conv=5, maxpool=6, l2norm=7)
DN_T = dict(act=0, image=1, vec=2, pool=3)
DN_NMS = dict(hard=0, linear=1, gaussian=2)
DN_MERGE = dict(iou=0, ios=1)
DN_FRAME = dict(nv12=0, i420=1, rgb24=2, bgr24=3)
DN_COLOR = dict(bt601=0, bt709=1)
DN_COLOR_FULL_RANGE = 0x10
DN_REGION_HFLIP = 1
DN_SGD_CHUNK = 2048
DN_SGD_MAX_GATE = 8
DN_ZONE = dict(cross=1, enter=2, exit=3, vanish=4)
DN_OSD_LABEL, DN_OSD_SCORE, DN_OSD_HIDE = 1, 2, 4
DN_WARP_CELL = 8
DN_WARP_BORDER = dict(constant=0, replicate=1)


DN_JPEG_MAX_ITEMS = 8192
DN_JPEG_HEADER_BYTES = 613


class TensorDesc(C.Structure):
    _fields_ = [("c", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("kind", C.c_int32)]


class OpDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("inp", C.c_int32), ("out", C.c_int32), ("residual", C.c_int32),
                ("se", C.c_int32), ("pool", C.c_int32),
                ("cin", C.c_int32), ("cout", C.c_int32), ("k", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32),
                ("dil", C.c_int32), ("act", C.c_int32),
                ("head", C.c_int32), ("level", C.c_int32), ("squeeze", C.c_int32), ("ceil_mode", C.c_int32),
                ("pool_pixels", C.c_int32), ("reserved", C.c_int32 * 2),
                ("w_off", C.c_int64), ("b_off", C.c_int64), ("w2_off", C.c_int64), ("b2_off", C.c_int64)]


class SgdTensor(C.Structure):
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("buf", C.c_void_p), ("numel", C.c_int64)]


class SgdHyper(C.Structure):
    _fields_ = [("lr", C.c_float), ("momentum", C.c_float), ("dampening", C.c_float), ("weight_decay", C.c_float),
                ("nesterov", C.c_int32), ("first_step", C.c_int32), ("step", C.c_int32), ("reserved", C.c_int32)]


class Frame(C.Structure):
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_int32 * 3), ("width", C.c_int32), ("height", C.c_int32), ("reserved", C.c_int32)]


class Region(C.Structure):
    _fields_ = [("frame", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class TrackParams(C.Structure):
    _fields_ = [("track_thresh", C.c_float), ("low_thresh", C.c_float), ("new_thresh", C.c_float),
                ("match_thresh", C.c_float), ("second_thresh", C.c_float), ("unconfirmed_thresh", C.c_float),
                ("track_buffer", C.c_int32), ("class_agnostic", C.c_int32), ("max_tracks", C.c_int32), ("reserved", C.c_int32)]


class TrackAppearanceParams(C.Structure):
    _fields_ = [("dim", C.c_int32), ("alpha", C.c_float), ("appearance_thresh", C.c_float), ("proximity_thresh", C.c_float),
                ("emb_fp16", C.c_int32), ("reserved", C.c_int32 * 3)]


class ZoneConfig(C.Structure):
    _fields_ = [("n_lines", C.c_int32), ("lines", C.c_float * 4 * 16), ("n_zones", C.c_int32), ("nv", C.c_int32 * 16),
                ("verts", C.c_float * 2 * 16 * 16), ("reserved", C.c_int32 * 2)]


class CropParams(C.Structure):
    _fields_ = [("margin", C.c_float), ("square", C.c_int32), ("min_width", C.c_int32), ("min_height", C.c_int32),
                ("mean", C.c_float * 3), ("std", C.c_float * 3), ("out_h", C.c_int32), ("out_w", C.c_int32), ("out_fp16", C.c_int32),
                ("capacity", C.c_int32), ("reserved", C.c_int32 * 2)]


class MotionParams(C.Structure):
    _fields_ = [("max_h", C.c_int32), ("max_w", C.c_int32), ("block", C.c_int32), ("radius", C.c_int32), ("min_texture", C.c_int32),
                ("min_blocks", C.c_int32), ("mask_thresh", C.c_float), ("reserved", C.c_int32)]


class OsdStyle(C.Structure):
    _fields_ = [("thickness", C.c_uint8), ("fill_alpha", C.c_uint8), ("pixelate", C.c_uint8), ("flags", C.c_uint8), ("reserved", C.c_uint8 * 4)]


class OsdColor(C.Structure):
    _fields_ = [("color", C.c_uint8 * 3), ("text", C.c_uint8 * 3), ("reserved", C.c_uint8 * 2)]


class OsdParams(C.Structure):
    _fields_ = [("default_style", OsdStyle), ("n_colors", C.c_int32), ("color_by_id", C.c_int32), ("scale", C.c_int32), ("label_alpha", C.c_int32),
                ("line_thickness", C.c_int32), ("zone_thickness", C.c_int32), ("zone_alpha", C.c_int32), ("line_color", C.c_uint8 * 3),
                ("reserved0", C.c_uint8), ("zone_color", C.c_uint8 * 3), ("reserved1", C.c_uint8), ("reserved", C.c_int32 * 5)]


class ComposeItem(C.Structure):
    _fields_ = [("src", C.c_int32), ("sx0", C.c_int32), ("sy0", C.c_int32), ("sw", C.c_int32), ("sh", C.c_int32), ("dst", C.c_int32),
                ("dx0", C.c_int32), ("dy0", C.c_int32), ("dw", C.c_int32), ("dh", C.c_int32), ("tile0", C.c_int32), ("reserved", C.c_int32)]


class ComposeHeader(C.Structure):
    _fields_ = [("n_items", C.c_int32), ("n_tiles", C.c_int32), ("reserved", C.c_int32 * 2)]


class JpegItem(C.Structure):
    _fields_ = [("frame", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("quality", C.c_int32),
                ("seg0", C.c_int32), ("reserved", C.c_int32)]


class JpegHeader(C.Structure):
    _fields_ = [("n_items", C.c_int32), ("n_segments", C.c_int32), ("reserved", C.c_int32 * 2)]


class WarpItem(C.Structure):
    _fields_ = [("src", C.c_int32), ("dst", C.c_int32), ("dx0", C.c_int32), ("dy0", C.c_int32), ("dw", C.c_int32), ("dh", C.c_int32),
                ("mesh0", C.c_int32), ("mesh_w", C.c_int32), ("flags", C.c_int32), ("border", C.c_int32), ("tile0", C.c_int32), ("reserved", C.c_int32)]


class WarpHeader(C.Structure):
    _fields_ = [("n_items", C.c_int32), ("n_tiles", C.c_int32), ("n_points", C.c_int32), ("reserved", C.c_int32)]


class ModelDesc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("n_tensors", C.c_int32), ("n_ops", C.c_int32),
                ("tensors", C.POINTER(TensorDesc)), ("ops", C.POINTER(OpDesc)),
                ("input_tensor", C.c_int32), ("image_h", C.c_int32), ("image_w", C.c_int32),
                ("mean", C.c_float * 3), ("std", C.c_float * 3),
                ("num_classes", C.c_int32), ("n_levels", C.c_int32),
                ("level_tensor", C.c_int32 * 8), ("anchors_per_loc", C.c_int32 * 8),
                ("num_anchors", C.c_int32), ("anchors", C.POINTER(C.c_float)),
                ("score_thresh", C.c_float), ("nms_thresh", C.c_float),
                ("detections_per_img", C.c_int32), ("topk_candidates", C.c_int32)]


_SIGNATURES = {
    "dn_abi_version": (C.c_int, []),
    "dn_last_error": (C.c_char_p, []),
    "dn_create": (C.c_int, [C.POINTER(ModelDesc), C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "dn_destroy": (None, [C.c_void_p]),
    "dn_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "dn_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dn_forward_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dn_forward_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dn_forward_regions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dn_forward_heads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dn_head_outputs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "dn_tensor_ptr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "dn_postprocess_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "dn_postprocess": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                 C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dn_postprocess_soft": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                      C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dn_set_nms": (C.c_int, [C.c_void_p, C.c_int, C.c_float]),
    "dn_pointwise_conv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p]),
    "dn_depthwise_conv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "dn_depthwise_pool_blocks": (C.c_int, [C.c_int] * 6),
    "dn_depthwise_conv_pool": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 8 + [C.c_void_p] * 7 + [C.c_int, C.c_void_p]),
    "dn_dense_conv": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 10 + [C.c_void_p]),
    "dn_expand_depthwise": (C.c_int, [C.c_void_p] * 9 + [C.c_int] * 11 + [C.c_void_p]),
    "dn_expand_depthwise_tiles": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "dn_depthwise_pointwise": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 8 + [C.c_void_p]),
    "dn_ssd_loss_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "dn_ssd_loss": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 4 + [C.c_float, C.c_float] + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dn_ssd_loss_state_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "dn_ssd_loss_train": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 4 + [C.c_float, C.c_float] + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                    C.c_void_p]),
    "dn_ssd_loss_backward": (C.c_int, [C.c_void_p] * 6 + [C.c_size_t, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 3),
    "dn_set_graph_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "dn_set_packed_output": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dn_profile_begin": (C.c_int, [C.c_void_p]),
    "dn_profile_end": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int]),
    "dn_batch_split": (C.c_int, [C.c_void_p, C.c_int]),
    "dn_set_chains": (C.c_int, [C.c_void_p, C.c_int]),
    "dn_profile_op_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int32)]),
    "dn_level_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dn_forward_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dn_lite_head_backward_workspace_bytes": (C.c_size_t, [C.c_int] * 6),
    "dn_lite_head_backward": (C.c_int, [C.c_void_p] * 5 + [C.c_int64] + [C.c_int] * 5 + [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p]),
    "dn_crop_tiles": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dn_merge_detections_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "dn_merge_detections": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_float, C.c_int, C.c_int] + [C.c_void_p] * 6
                            + [C.c_size_t, C.c_void_p]),
    "dn_fuse_detections_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int]),
    "dn_fuse_detections": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_float, C.c_float, C.c_int] + [C.c_void_p] * 6
                           + [C.c_size_t, C.c_void_p]),
    "dn_match_detections": (C.c_int, [C.c_void_p] * 8 + [C.c_int] * 4 + [C.POINTER(C.c_double), C.c_int, C.c_double] + [C.c_void_p] * 5),
    "dn_coco_match": (C.c_int, [C.c_void_p] * 9 + [C.c_int] * 4 + [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int] + [C.c_void_p] * 5),
    "dn_augment_workspace_bytes": (C.c_size_t, [C.c_int]),
    "dn_augment_batch": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dn_sgd_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "dn_grad_norm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "dn_sgd_step": (C.c_int, [C.c_void_p, C.c_int, C.c_int, SgdHyper, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "dn_track_state_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "dn_track_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dn_track_update": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.POINTER(TrackParams), C.c_void_p, C.c_size_t] + [C.c_void_p] * 8),
    "dn_track_feature_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "dn_track_appearance_workspace_bytes": (C.c_size_t, [C.c_int] * 5),
    "dn_track_feature_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dn_track_update_appearance": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.POINTER(TrackParams), C.POINTER(TrackAppearanceParams),
                                             C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                             C.c_size_t] + [C.c_void_p] * 8),
    "dn_zone_state_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "dn_zone_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dn_zone_update": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                 C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "dn_crop_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "dn_crop_objects": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(CropParams),
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dn_motion_state_bytes": (C.c_size_t, [C.c_int, C.POINTER(MotionParams)]),
    "dn_motion_reset": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(MotionParams), C.c_void_p, C.c_void_p]),
    "dn_motion_estimate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(MotionParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dn_track_compensate": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dn_osd_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "dn_osd_paint": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 4
                     + [C.POINTER(OsdParams), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "dn_compose": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "dn_surface_fill": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "dn_warp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "dn_jpeg_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "dn_jpeg_encode": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dn_jpeg_items_from_index": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
}
EXPORTS = tuple(_SIGNATURES)
# include/demonet_hip_debug.h: test support beside the boundary (not part of EXPORTS, which mirrors demonet_hip.h)
_DEBUG_SIGNATURES = {
    "dn_debug_last_kernel": (C.c_int, [C.c_char_p, C.c_int]),
    "dn_debug_conv_pool": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 6 + [C.c_void_p]),
    "dn_debug_stem": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 7 + [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p]),
    "dn_debug_choice": (C.c_int, [C.c_char_p, C.POINTER(C.c_int64), C.c_int, C.c_char_p, C.c_int]),
}

_lib = None


class HipLibraryMissing(RuntimeError):
    pass


def lib():
    """Loads libdemonet_hip.so (built in-tree by `python -m demonet_amd.build`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryMissing(
            f"{LIB_PATH} not found: build it with `python -m demonet_amd.build` (hipcc, gfx950). "
            "demonet_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in list(_SIGNATURES.items()) + list(_DEBUG_SIGNATURES.items()):
        fn = getattr(L, name)          # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if L.dn_abi_version() != DN_ABI_VERSION:
        raise HipLibraryMissing(f"ABI mismatch: library {L.dn_abi_version()} vs binding {DN_ABI_VERSION}; rebuild")
    _lib = L
    return L


def check(rc: int, what: str = ""):
    if rc < 0:
        msg = lib().dn_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"demonet_hip {what} failed ({rc}): {msg}")
    return rc


def debug_last_kernel() -> str:
    """Label of the kernel the last launcher call on this thread enqueued (dn_debug_last_kernel)."""
    buf = C.create_string_buffer(128)
    check(lib().dn_debug_last_kernel(buf, len(buf)), "dn_debug_last_kernel")
    return buf.value.decode()


def debug_choice(family: str, *dims) -> dict:
    """What the kernel-choice functions answer for a shape (dn_debug_choice; host only): the "key=value" text as a dict, integers as int."""
    arr = (C.c_int64 * len(dims))(*[int(v) for v in dims])
    buf = C.create_string_buffer(256)
    check(lib().dn_debug_choice(family.encode(), arr, len(dims), buf, len(buf)), "dn_debug_choice")
    out = {}
    for item in buf.value.decode().split():
        k, v = item.split("=", 1)
        out[k] = int(v) if v.lstrip("-").isdigit() else v
    return out
