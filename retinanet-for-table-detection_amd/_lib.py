"""ctypes binding of librtn.so (the C-ABI declared in include/rtn.h).

There is no CPU fallback: if the shared library is missing or a symbol is absent the import
raises, and every call checks its return code and raises RtnError with rtn_last_error().
"""
import ctypes as C
import os

# PyTorch must load ITS HIP runtime before librtn.so is opened: torch bundles libamdhip64.so (SONAME libamdhip64.so.7) and
# librtn.so needs libamdhip64.so.7, so opened second it binds to the copy already in the process.  Opened first, the loader
# takes /opt/rocm/lib/libamdhip64.so.7 and torch then brings a second runtime in: two HIP runtimes in one process hand each
# other streams and pointers, and device discovery in the second one fails intermittently ("no ROCm-capable device").
import torch  # noqa: F401  (load order, see above)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RTN_LIB_PATH") or os.path.join(_HERE, "librtn.so")      # RTN_LIB_PATH: A/B two builds on one box

RTN_BF16, RTN_F32, RTN_U8, RTN_FP8, RTN_I32 = 0, 1, 2, 3, 4
RTN_DET_CLASS_AGNOSTIC, RTN_DET_NO_NMS = 1, 2
RTN_MAX_GROUPS, RTN_MAX_GT, RTN_MAX_DET = 5, 64, 300
RTN_HEADER_MAX_K, RTN_HEADER_WIDTH, RTN_HEADER_MAX_POINTS = 9, 500, 1 << 21
RTN_EFFECT_RAW_HSV, RTN_EFFECT_FORCE_CONTRAST, RTN_EFFECT_FORCE_BRIGHTNESS, RTN_EFFECT_FORCE_HUE, RTN_EFFECT_FORCE_SATURATION = 1, 16, 32, 64, 128

CONV_RELU, CONV_SIGMOID, CONV_RES_SAME, CONV_RES_UPSAMPLE, CONV_OUT_F32, CONV_RELU_MASK, CONV_MASK_PRE = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40

ERRNAMES = {0: "RTN_OK", -1: "RTN_EINVAL", -2: "RTN_EHIP", -3: "RTN_ENOMEM", -4: "RTN_EBOUNDS"}


class RtnError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("%s (%d): %s" % (ERRNAMES.get(code, "RTN_E?"), code, text))
        self.code = code


class ConvGroup(C.Structure):
    _fields_ = [
        ("in_", C.c_void_p), ("out", C.c_void_p), ("res", C.c_void_p),
        ("in_elems", C.c_int64), ("out_elems", C.c_int64), ("res_elems", C.c_int64),
        ("in_img_stride", C.c_int64), ("out_img_stride", C.c_int64), ("out_off", C.c_int64),
        ("res_img_stride", C.c_int64),
        ("in_row_stride", C.c_int32), ("Hin", C.c_int32), ("Win", C.c_int32),
        ("Hout", C.c_int32), ("Wout", C.c_int32), ("Hres", C.c_int32), ("Wres", C.c_int32),
        ("res_ld", C.c_int32),
        ("mask", C.c_void_p), ("mask_elems", C.c_int64), ("mask_img_stride", C.c_int64),
        ("mask_ld", C.c_int32), ("out_step", C.c_int32), ("out_pix_w", C.c_int32), ("reserved_", C.c_int32),
    ]


class ConvDesc(C.Structure):
    _fields_ = [
        ("g", ConvGroup * RTN_MAX_GROUPS),
        ("ngroups", C.c_int32), ("batch", C.c_int32), ("dtype", C.c_int32),
        ("w", C.c_void_p), ("bias", C.c_void_p),
        ("w_rows", C.c_int32), ("N", C.c_int32), ("KH", C.c_int32), ("KW", C.c_int32),
        ("Crun", C.c_int32), ("pix_stride", C.c_int32), ("sy", C.c_int32), ("sx", C.c_int32),
        ("pad_t", C.c_int32), ("pad_l", C.c_int32), ("out_ld", C.c_int32), ("flags", C.c_int32),
        ("reserved_", C.c_int32), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
    ]


class ConvSrc2(C.Structure):
    _fields_ = [
        ("in_", C.c_void_p), ("in_elems", C.c_int64), ("in_img_stride", C.c_int64),
        ("in_row_stride", C.c_int32), ("pix_stride", C.c_int32), ("Hin", C.c_int32), ("Win", C.c_int32),
        ("C", C.c_int32), ("step", C.c_int32),
    ]


class AnchorCfg(C.Structure):
    _fields_ = [
        ("nlevels", C.c_int32), ("A", C.c_int32),
        ("H", C.c_int32 * RTN_MAX_GROUPS), ("W", C.c_int32 * RTN_MAX_GROUPS),
        ("stride", C.c_int32 * RTN_MAX_GROUPS),
        ("anchor_off", C.c_int32 * (RTN_MAX_GROUPS + 1)),
        ("base", ((C.c_double * 4) * 16) * RTN_MAX_GROUPS),
    ]


class BottleneckDesc(C.Structure):
    _fields_ = [
        ("a_in", C.c_void_p), ("a_in_elems", C.c_int64), ("x_in", C.c_void_p), ("x_in_elems", C.c_int64),
        ("x_out", C.c_void_p), ("x_out_elems", C.c_int64), ("a_out", C.c_void_p), ("a_out_elems", C.c_int64),
        ("w2b", C.c_void_p), ("b2b", C.c_void_p), ("w2c", C.c_void_p), ("b2c", C.c_void_p), ("w2a", C.c_void_p), ("b2a", C.c_void_p),
        ("batch", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("mid", C.c_int32), ("dtype", C.c_int32), ("w2c_ld", C.c_int32),
        ("p_in", C.c_void_p), ("p_in_elems", C.c_int64), ("wproj", C.c_void_p),
        ("h1_out", C.c_void_p), ("h1_out_elems", C.c_int64),
        ("x_out_step", C.c_int32), ("x_in_step", C.c_int32),
    ]


class ChainDesc(C.Structure):
    _fields_ = [
        ("h_in", C.c_void_p), ("h_in_elems", C.c_int64), ("x_in", C.c_void_p), ("x_in_elems", C.c_int64),
        ("x_out", C.c_void_p), ("x_out_elems", C.c_int64), ("a_out", C.c_void_p), ("a_out_elems", C.c_int64),
        ("w2c", C.c_void_p), ("b2c", C.c_void_p), ("w2a", C.c_void_p), ("b2a", C.c_void_p),
        ("pixels", C.c_int64), ("mid", C.c_int32), ("out", C.c_int32), ("next", C.c_int32), ("dtype", C.c_int32),
    ]


class JpegInfo(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("components", C.c_int32), ("h_samp", C.c_int32), ("v_samp", C.c_int32),
        ("restart_interval", C.c_int32), ("huffman_tables", C.c_int32), ("quant_tables", C.c_int32),
        ("blob_bytes", C.c_int64), ("workspace_bytes", C.c_int64), ("scan_bytes", C.c_int64),
    ]


class PngInfo(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("components", C.c_int32), ("chunks", C.c_int32),
        ("blob_bytes", C.c_int64), ("workspace_bytes", C.c_int64), ("payload_bytes", C.c_int64),
    ]


class TiffInfo(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("components", C.c_int32), ("strips", C.c_int32),
        ("compression", C.c_int32), ("bits", C.c_int32), ("photometric", C.c_int32), ("predictor", C.c_int32),
        ("blob_bytes", C.c_int64), ("workspace_bytes", C.c_int64), ("payload_bytes", C.c_int64),
    ]


RTN_TIFF_ALLOW_G4_ONE_STRIP = 1


class ComposeItem(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("h", C.c_int32), ("w", C.c_int32), ("orientation", C.c_int32), ("invert", C.c_int32),
        ("page", C.c_int32), ("x", C.c_int32), ("y", C.c_int32),
        ("crop_x", C.c_int32), ("crop_y", C.c_int32), ("crop_w", C.c_int32), ("crop_h", C.c_int32), ("reserved_", C.c_int32),
    ]


def png_blob_bound(file_bytes):
    """RTN_PNG_BLOB_BOUND of include/rtn.h: the most bytes rtn_png_inspect writes for a file of that size."""
    return 128 + 2 * int(file_bytes)


def jpeg_blob_bound(file_bytes):
    """RTN_JPEG_BLOB_BOUND of include/rtn.h: the most bytes rtn_jpeg_inspect writes for a file of that size."""
    return 16384 + 4 * int(file_bytes)


class ConvFp8(C.Structure):
    _fields_ = [("acc_scale", C.c_float), ("out_scale", C.c_float), ("out_dtype", C.c_int32)]


# every symbol include/rtn.h declares: (restype, argtypes)
_P, _I, _I64, _F, _D, _SZ = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_size_t
SIGNATURES = {
    "rtn_create": (_I, [C.POINTER(_P), _I]),
    "rtn_destroy": (_I, [_P]),
    "rtn_create_error": (C.c_char_p, []),
    "rtn_set_stream": (_I, [_P, _P]),
    "rtn_last_error": (C.c_char_p, [_P]),
    "rtn_version": (C.c_char_p, []),
    "rtn_conv2d_workspace_bytes": (_SZ, [_P, C.POINTER(ConvDesc)]),
    "rtn_debug_last_conv_impl": (_I, [_P]),
    "rtn_debug_last_wgrad_impl": (_I, [_P]),
    "rtn_conv2d_fwd": (_I, [_P, C.POINTER(ConvDesc)]),
    "rtn_conv1x1_dual_fwd": (_I, [_P, C.POINTER(ConvDesc), C.POINTER(ConvSrc2)]),
    "rtn_conv1x1_dual_workspace_bytes": (_SZ, [_P, C.POINTER(ConvDesc), C.POINTER(ConvSrc2)]),
    "rtn_conv_workspace_init": (_I, [_P, _P, _SZ]),
    "rtn_debug_last_conv_streamk": (_I, [_P]),
    "rtn_debug_last_conv_tile": (_I, [_P]),
    "rtn_debug_conv_sync_timeouts": (_I, [_P, _P, C.POINTER(C.c_uint32)]),
    "rtn_bottleneck64_fwd": (_I, [_P, C.POINTER(BottleneckDesc)]),
    "rtn_chain1x1_fwd": (_I, [_P, C.POINTER(ChainDesc)]),
    "rtn_chain1x1_supported": (_I, [_I, _I, _I]),
    "rtn_conv2d_dgrad": (_I, [_P, C.POINTER(ConvDesc)]),
    "rtn_pack_dgrad_weights": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I]),
    "rtn_pack_dgrad_weights_multi": (_I, [_P, _P, _I, _I64, _I]),
    "rtn_conv2d_wgrad_workspace_bytes": (_SZ, [C.POINTER(ConvDesc)]),
    "rtn_conv2d_wgrad": (_I, [_P, C.POINTER(ConvDesc), _P, _P, _SZ]),
    "rtn_conv2d_wgrad_bias": (_I, [_P, C.POINTER(ConvDesc), _P, _P, _I, _P, _SZ]),
    "rtn_conv2d_wgrad_rowinfo": (_I, [_P, C.POINTER(ConvDesc), _P, _SZ]),
    "rtn_conv2d_wgrad_prepared": (_I, [_P, C.POINTER(ConvDesc), _P, _P, _I, _P, _SZ]),
    "rtn_bias_grad": (_I, [_P, _P, _I, _I64, _I, _I64, _P]),
    "rtn_pad_cast_rows": (_I, [_P, _P, _P, _I, _I64, _I, _I]),
    "rtn_zero_insert2": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I]),
    "rtn_upsample_add_bwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I]),
    "rtn_maxpool3x3s2_tfsame_bwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I]),
    "rtn_maxpool3x3s2_tfsame_fwd_idx": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I]),
    "rtn_maxpool3x3s2_tfsame_bwd_idx": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I]),
    "rtn_sumsq_workspace_bytes": (_SZ, []),
    "rtn_sumsq_ranges": (_I, [_P, _P, _P, _I64, _P, _I, _I64, _P, _P, _P, _SZ]),
    "rtn_adam_clipnorm_step_ranges": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I64, _P, _I, _I64, _I64, _F, _F, _F, _F, _P, _F, _F]),
    "rtn_adam_clipnorm_step_ranges_pertensor": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I64, _P, _I, _I64, _I64, _F, _F, _F, _F, _P, _F, _F]),
    "rtn_stem_pack": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _I, _I]),
    "rtn_stem_conv_pool": (_I, [_P, _P, _I, _I, _P, _I, _P, _P, _I, _I, _I]),
    "rtn_stem_conv_pool_branch2a": (_I, [_P, _P, _I, _I, _P, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P]),
    "rtn_maxpool3x3s2_tfsame_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I]),
    "rtn_relu": (_I, [_P, _P, _P, _I, _I64]),
    "rtn_generate_anchors": (_I, [_D, C.POINTER(_D), _I, C.POINTER(_D), _I, C.POINTER(_D)]),
    "rtn_anchors_f64": (_I, [_P, C.POINTER(AnchorCfg), _P]),
    "rtn_anchors_f32": (_I, [_P, C.POINTER(AnchorCfg), _P]),
    "rtn_anchor_targets": (_I, [_P, C.POINTER(AnchorCfg), _I, _I, _P, _P, _P, _P, _D, _D, _P, _P]),
    "rtn_anchor_targets_explicit": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _D, _D, _P, _P]),
    "rtn_compute_overlap": (_I, [_P, _P, _P, _I, _I, _P]),
    "rtn_gt_annotations": (_I, [_P, _P, _I, _I, _D, _D, _P, _P, _P]),
    "rtn_bbox_transform": (_I, [_P, _P, _P, _I, C.POINTER(_D), C.POINTER(_D), _P]),
    "rtn_filter_detections": (_I, [_P, _I, _I64, _I, _P, _P, _F, _F, _I, _P, _P, _P, _P, _SZ]),
    "rtn_regress_boxes": (_I, [_P, _P, _P, _I64, C.POINTER(_F), C.POINTER(_F), _P]),
    "rtn_clip_boxes": (_I, [_P, _P, _I64, _F, _F, _P]),
    "rtn_upsample_nearest": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I]),
    "rtn_preprocess_image": (_I, [_P, _P, _I, _P, _I64, _I, _F, _F]),
    "rtn_preprocess_dt3_workspace_bytes": (_SZ, [_I, _I, _I]),
    "rtn_preprocess_dt3": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _SZ]),
    "rtn_distance_transform3": (_I, [_P, _P, _I, _I, _I, _P, _P, _SZ]),
    "rtn_resize_cubic": (_I, [_P, _P, _I, _I, _I, _I, _D, _P, _I, _I, _I, _I64]),
    "rtn_conv2d_fp8_fwd": (_I, [_P, C.POINTER(ConvDesc), C.POINTER(ConvFp8)]),
    "rtn_quantize_fp8": (_I, [_P, _P, _I, _P, _I64, _F]),
    "rtn_conv2d_fwd_fp8out": (_I, [_P, C.POINTER(ConvDesc), _F]),
    "rtn_warp_affine_u8": (_I, [_P, _P, _I, _I, _I, _P, _I, _I, _P, _P]),
    "rtn_retina_loss_fwd": (_I, [_P, _I64, _I, _P, _P, _P, _P, _F, _F, _F, _P, _P, _SZ]),
    "rtn_retina_loss_workspace_bytes": (_SZ, [_I64]),
    "rtn_retina_loss_boxes_workspace_bytes": (_SZ, [_I, _I64]),
    "rtn_retina_loss_boxes_fwd": (_I, [_P, C.POINTER(AnchorCfg), _I, _I, _P, _P, _P, _P, _D, _D, _P, _P, _F, _F, _F, _P, _P, _SZ]),
    "rtn_retina_loss_bwd": (_I, [_P, _I64, _I, _P, _P, _P, _P, _F, _F, _F, _F, _F, _I, _P, _P]),
    "rtn_retina_loss_bwd_dev": (_I, [_P, _I64, _I, _P, _P, _P, _P, _F, _F, _F, _P, _I, _P, _P]),
    "rtn_detect_workspace_bytes": (_SZ, [_I, _I64, _I]),
    "rtn_decode_filter_nms": (_I, [_P, C.POINTER(AnchorCfg), _I, _I, _P, _P, _I, _I, _F, _F, _I, _P, _P, _P, _P, _SZ]),
    "rtn_detect_workspace_bytes_ex": (_SZ, [_I, _I64, _I, _I]),
    "rtn_decode_filter_nms_ex": (_I, [_P, C.POINTER(AnchorCfg), _I, _I, _P, _P, _I, _I, _F, _F, _I, _P, _P, _P, _P, _SZ, _I, _P]),
    "rtn_filter_detections_ex": (_I, [_P, _I, _I64, _I, _P, _P, _F, _F, _I, _P, _P, _P, _P, _SZ, _I, _P]),
    "rtn_gather_detections": (_I, [_P, _I, _I64, _I, _I64, _I, _P, _P, _P]),
    "rtn_eval_workspace_bytes": (_SZ, [_I64, _I, _I]),
    "rtn_eval_match": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, C.POINTER(_D), _D, _I, _P, _P]),
    "rtn_eval_finalize": (_I, [_P, _I64, _I, _P, _P, _I, _I, _D, _P, _P, _SZ]),
    "rtn_jpeg_inspect": (_I, [_P, _P, _SZ, C.POINTER(JpegInfo), _P, _SZ]),
    "rtn_jpeg_workspace_bytes": (_SZ, [_I, _P, _P]),
    "rtn_jpeg_decode": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _SZ]),
    "rtn_jpeg_decode_host": (_I, [_P, _I, _P, _SZ, C.POINTER(C.c_int32)]),
    "rtn_jpeg_decode_host_counters": (None, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rtn_jpeg_encode_header": (_I, [_I, _I, _I, _I, _I, _P, _SZ, C.POINTER(_SZ)]),
    "rtn_jpeg_encode_bound": (_SZ, [_I, _I, _I, _I]),
    "rtn_jpeg_encode_workspace_bytes": (_SZ, [_I, _P, _P, _P, _P]),
    "rtn_jpeg_encode": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ]),
    "rtn_png_encode_bound": (_SZ, [_I, _I, _I]),
    "rtn_png_encode_workspace_bytes": (_SZ, [_I, _P, _P, _P]),
    "rtn_png_encode": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ]),
    "rtn_png_inspect": (_I, [_P, _P, _SZ, C.POINTER(PngInfo), _P, _SZ]),
    "rtn_png_decode_workspace_bytes": (_SZ, [_I, _P, _P]),
    "rtn_png_decode": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _SZ]),
    "rtn_png_inflate_chunk_host": (_I, [_P, _SZ, _P, _SZ, C.POINTER(C.c_int32)]),
    "rtn_png_stream_blob_bound": (_SZ, [_SZ]),
    "rtn_png_stream_inspect": (_I, [_P, _P, _SZ, C.POINTER(PngInfo), _P, _SZ]),
    "rtn_png_stream_decode_workspace_bytes": (_SZ, [_I, _P, _P]),
    "rtn_png_stream_decode": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _SZ]),
    "rtn_png_stream_inflate_host": (_I, [_P, _SZ, _P, _SZ, C.POINTER(C.c_int32)]),
    "rtn_png_layout_blob_bound": (_SZ, [_SZ]),
    "rtn_png_layout_inspect": (_I, [_P, _P, _SZ, C.POINTER(PngInfo), _P, _SZ]),
    "rtn_png_layout_decode_workspace_bytes": (_SZ, [_I, _P, _P]),
    "rtn_png_layout_decode": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _SZ]),
    "rtn_png_layout_pixels_host": (_I, [_P, _P, _SZ, _P, C.POINTER(C.c_int32)]),
    "rtn_tiff_blob_bound": (_SZ, [_SZ]),
    "rtn_tiff_inspect": (_I, [_P, _P, _SZ, C.POINTER(TiffInfo), _P, _SZ]),
    "rtn_tiff_inspect_flags": (_I, [_P, _P, _SZ, _I, C.POINTER(TiffInfo), _P, _SZ]),
    "rtn_tiff_decode_workspace_bytes": (_SZ, [_I, _P, _P]),
    "rtn_tiff_decode": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _SZ]),
    "rtn_tiff_decode_host": (_I, [_P, _P, _SZ, C.POINTER(C.c_int32)]),
    "rtn_tiff_encode_bound": (_SZ, [_I, _I, _I]),
    "rtn_tiff_encode_workspace_bytes": (_SZ, [_I, _P, _P, _P, _P]),
    "rtn_tiff_encode": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ]),
    "rtn_tiff_encode_host": (_I, [_I, _I, _I, _P, _I, _I, _I, _P, _SZ, C.POINTER(_SZ)]),
    "rtn_render_workspace_bytes": (_SZ, [_I, _I, _I]),
    "rtn_render_pages": (_I, [_P, _I, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _SZ, _I, _P, _P, _P, _P, _P, _I, _P, _SZ, _P, _SZ]),
    "rtn_render_host": (_I, [_I, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _SZ, _I, _P, _P, _P, _P, _P, _I, _P, _SZ]),
    "rtn_render_tiles_host": (_I, [_I, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _SZ, _I, _P, _P, _P, _P, _P, _I, _P, _SZ]),
    "rtn_header_workspace_bytes": (_SZ, [_I, _I]),
    "rtn_header_sample": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _SZ, _P, _SZ]),
    "rtn_header_cluster": (_I, [_P, _I, _P, _P, _P, _SZ, _I, _P, _P, _P, _P, _P, _SZ, _P, _SZ]),
    "rtn_header_stats": (_I, [_P, _I, _P, _P, _P, _P, _SZ, _P, _SZ, _P, _P, _SZ]),
    "rtn_header_patches": (_I, [_P, _I, _P, _P, _P, _SZ, _I, _P, _P, _P, _P, _P, _SZ, _P, _SZ]),
    "rtn_header_sample_host": (_I, [_I, _P, _P, _P, _P, _P, _P, _SZ]),
    "rtn_header_cluster_host": (_I, [_I, _P, _P, _P, _SZ, _I, _P, _P, _P, _P, _P, _SZ]),
    "rtn_header_stats_host": (_I, [_I, _P, _P, _P, _P, _SZ, _P, _SZ, _P]),
    "rtn_header_patches_host": (_I, [_I, _P, _P, _P, _SZ, _I, _P, _P, _P, _P, _P, _SZ]),
    "rtn_cca_workspace_bytes": (_SZ, [_I, _P, _P, _I]),
    "rtn_cca_lines_mask": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _SZ, _P, _SZ]),
    "rtn_cca_text_mask": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _SZ, _P, _SZ]),
    "rtn_cca_label": (_I, [_P, _I, _P, _P, _P, _I, _P, _P, _P, _P, _SZ, _P, _SZ]),
    "rtn_cca_paint": (_I, [_P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _P, _SZ]),
    "rtn_cca_lines_mask_host": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "rtn_cca_text_mask_host": (_I, [_I, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "rtn_cca_label_host": (_I, [_I, _P, _P, _P, _I, _P, _P, _P, _P, _SZ]),
    "rtn_cca_paint_host": (_I, [_I, _P, _P, _P, _P, _I, _P, _P, _I]),
    "rtn_visual_effect_workspace_bytes": (_SZ, [_I, _P, _P]),
    "rtn_visual_effect_u8": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _SZ]),
    "rtn_visual_effect_host": (_I, [_I, _P, _P, _P, _P, _P, _P]),
    "rtn_resize_u8_workspace_bytes": (_SZ, [_I]),
    "rtn_resize_u8": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ]),
    "rtn_resize_u8_host": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "rtn_resize_u8_path": (_I, [_D]),
    "rtn_resize_u8_tile": (_I, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rtn_skew_workspace_bytes": (_SZ, [_I, _P, _P, _I, _I]),
    "rtn_skew_counts_layout": (_I, [_I, _P, _P, _I, _I, _P]),
    "rtn_skew_estimate": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _SZ]),
    "rtn_skew_estimate_host": (_I, [_I, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
    "rtn_lattice_workspace_bytes": (_SZ, [_I, _P, C.c_int64]),
    "rtn_lattice_masks": (_I, [_P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _SZ, _P, _SZ]),
    "rtn_lattice_profiles": (_I, [_P, _I, _P, _P, _P, _P, _P, _SZ, _P, _P, _SZ, _P, _SZ]),
    "rtn_lattice_edges": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _SZ, _I, _I, _P, _P, _P, _SZ, _P, _SZ, _P, _SZ]),
    "rtn_lattice_cells": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _SZ, _P, _P, _SZ, _P, _P, _SZ, _P, _SZ]),
    "rtn_lattice_separators_host": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "rtn_lattice_masks_host": (_I, [_I, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _SZ]),
    "rtn_lattice_profiles_host": (_I, [_I, _P, _P, _P, _P, _P, _SZ, _P, _P, _SZ]),
    "rtn_lattice_edges_host": (_I, [_I, _P, _P, _P, _P, _P, _P, _SZ, _I, _I, _P, _P, _P, _SZ, _P, _SZ]),
    "rtn_lattice_cells_host": (_I, [_I, _P, _P, _P, _P, _P, _P, _SZ, _P, _P, _SZ, _P, _P, _SZ]),
    "rtn_page_compose_workspace_bytes": (_SZ, [_I, _I]),
    "rtn_page_compose": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _SZ]),
    "rtn_page_compose_host": (_I, [_I, _P, _I, _P, _P, _P]),
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "librtn.so not found at %s — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C retinanet-for-table-detection_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing: fail loudly
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


class Handle:
    """Owns one rtn_handle_t bound to a device; check() turns error codes into RtnError."""

    def __init__(self, device=0):
        self._h = _P()
        rc = lib.rtn_create(C.byref(self._h), int(device))
        if rc != 0:
            raise RtnError(rc, "rtn_create(device=%d) failed: %s" % (device, lib.rtn_create_error().decode() or "no usable GPU?"))
        self.device = device

    @property
    def raw(self):
        return self._h

    def check(self, rc):
        if rc != 0:
            raise RtnError(rc, lib.rtn_last_error(self._h).decode("utf-8", "replace"))

    def set_stream(self, stream_ptr):
        self.check(lib.rtn_set_stream(self._h, _P(stream_ptr)))

    def close(self):
        if self._h:
            lib.rtn_destroy(self._h)
            self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def attach_conv_workspace(handle, d, s2=None):
    """Give a conv descriptor the scratch rtn_conv2d_workspace_bytes() (with `s2`: rtn_conv1x1_dual_workspace_bytes()) asks for on
    this device: a uint8 device tensor kept alive by the descriptor (the library never allocates; the K-split paths are skipped
    without it).  One buffer per descriptor, so launches on different streams never share scratch.  Its sync block (the first
    RTN_CONV_SYNC_BYTES) is zeroed here, once, on the handle's stream (rtn_conv_workspace_init).  Returns the tensor or None."""
    if s2 is None:
        n = int(lib.rtn_conv2d_workspace_bytes(handle.raw, C.byref(d)))
    else:
        n = int(lib.rtn_conv1x1_dual_workspace_bytes(handle.raw, C.byref(d), C.byref(s2)))
    if n <= 0:
        d.workspace, d.workspace_bytes, d._ws = None, 0, None
        return None
    t = torch.empty(n, dtype=torch.uint8, device=torch.device("cuda", handle.device))
    handle.check(lib.rtn_conv_workspace_init(handle.raw, t.data_ptr(), n))
    d.workspace, d.workspace_bytes, d._ws = t.data_ptr(), n, t
    return t


def generate_anchors_f64(base_size, ratios, scales):
    """Host-side generate_anchors (model/anchors.py:243-278) through the C-ABI."""
    import numpy as np
    r = np.ascontiguousarray(ratios, dtype=np.float64)
    s = np.ascontiguousarray(scales, dtype=np.float64)
    out = np.zeros((len(r) * len(s), 4), dtype=np.float64)
    rc = lib.rtn_generate_anchors(float(base_size), r.ctypes.data_as(C.POINTER(_D)), len(r),
                                  s.ctypes.data_as(C.POINTER(_D)), len(s), out.ctypes.data_as(C.POINTER(_D)))
    if rc != 0:
        raise RtnError(rc, "rtn_generate_anchors")
    return out


def ranges_table(ranges, device=None):
    """[(begin, end)] flat element ranges (in increasing order, non-overlapping) -> (int64 table [nr][3] of (begin, end, vbegin),
    nr, span) for rtn_sumsq_ranges / rtn_adam_clipnorm_step_ranges*: each range starts in the launch's index space at the next
    position congruent to its `begin` modulo 4, so every quad inside a range is one 16-byte access.  device=None: a CPU tensor."""
    rows, v = [], 0
    for b, e in ranges:
        b, e = int(b), int(e)
        if e < b or b < 0:
            raise ValueError("bad range [%d, %d)" % (b, e))
        v += (b - v) % 4
        rows.append((b, e, v))
        v += e - b
    t = torch.tensor(rows, dtype=torch.int64).reshape(-1, 3)
    if device is not None:
        t = t.to(device)
    return t, len(rows), v
