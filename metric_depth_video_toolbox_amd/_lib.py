"""ctypes binding of libmdvt_hip.so (the C ABI declared in include/mdvt.h).

There is no CPU fallback: if the shared library is missing or no gfx950 device is present, the
render entry points raise.  ``load()`` only dlopen()s the library (possible without a GPU);
``Context`` needs a device.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libmdvt_hip.so")

MDVT_OK = 0
MODE_POINTS = 0
MODE_MESH = 1

STATUS_NAMES = {0: "MDVT_OK", -1: "MDVT_ERR_INVALID_ARG", -2: "MDVT_ERR_HIP", -3: "MDVT_ERR_UNSUPPORTED",
                -4: "MDVT_ERR_NO_DEVICE", -5: "MDVT_ERR_OOM"}

# every symbol include/mdvt.h declares
SYMBOLS = ("mdvt_version", "mdvt_create", "mdvt_destroy", "mdvt_last_error", "mdvt_set_config",
           "mdvt_render_stereo", "mdvt_render_stereo_batch", "mdvt_decode_depth", "mdvt_encode_depth",
           "mdvt_edge_filter", "mdvt_infill_using_normals", "mdvt_mark_lower_side", "mdvt_touchly_depth",
           "mdvt_equirect_tables", "mdvt_equirect_remap", "mdvt_masked_blur", "mdvt_finish_infill_mask",
           "mdvt_finish_infill_mask_stereo", "mdvt_swap_rb", "mdvt_selftest", "mdvt_normal_infill", "mdvt_infill_using_mask_normals",
           "mdvt_edge_point_pixels", "mdvt_workspace_bytes", "mdvt_release_cached_memory", "mdvt_cached_memory", "mdvt_set_cached_memory_limit",
           "mdvt_debug_read", "mdvt_finish_infill_mask_heap", "mdvt_finish_infill_mask_heap_stereo",
           "mdvt_encode_video_frames", "mdvt_set_near_clip")

# the entry points include/mdvt_ffv1_decode.h declares (the device FFV1 decoder): bound like the others, listed apart from mdvt.h's
DECODE_SYMBOLS = ("mdvt_decode_video_frames", "mdvt_ffv1_decode_supported")

# the entry points include/mdvt_ffv1_stream_decode.h declares (inter-coded and Golomb-Rice FFV1 streams), listed apart in the same way
STREAM_DECODE_SYMBOLS = ("mdvt_decode_video_stream", "mdvt_ffv1_stream_decode_supported", "mdvt_ffv1_packet_is_key")

# the entry point include/mdvt_convergence.h declares (per-frame convergence depths), listed apart from mdvt.h's in the same way
CONVERGENCE_SYMBOLS = ("mdvt_convergence_depths",)

# the entry points include/mdvt_metric_align.h declares (relative depth to metric depth codes), listed apart in the same way
METRIC_ALIGN_SYMBOLS = ("mdvt_scale_shift_fit", "mdvt_metric_depth_codes")

# the entry point include/mdvt_depth_sink.h declares (metric depth planes to a depth video's codes), listed apart in the same way.  Its
# wrapper is step_device.depth_video_codes
DEPTH_SINK_SYMBOLS = ("mdvt_depth_video_codes",)

# the entry points include/mdvt_depth_engines.h declares (frames into a model, PromptDA's prompt, UniK3D's focal estimate), likewise.
# Their wrappers are step_device.model_frames, depth_prompt and focal_from_points
DEPTH_ENGINE_SYMBOLS = ("mdvt_model_frames", "mdvt_depth_prompt", "mdvt_focal_from_points")

# the entry points include/mdvt_infill_adapter.h declares (the frames around an in-painting model), listed apart in the same way
INFILL_ADAPTER_SYMBOLS = ("mdvt_adapter_prepare_eye", "mdvt_lhm_moments", "mdvt_lhm_apply", "mdvt_adapter_composite_eye")

# the entry points include/mdvt_infill_engines.h declares (the m2svid and stereo_dissoclusion_net steps around their models), likewise
INFILL_ENGINE_SYMBOLS = ("mdvt_m2svid_prepare_eye", "mdvt_model_infill_finish")

# the entry point include/mdvt_view.h declares (the free-camera viewer's vertex centres), likewise
VIEW_SYMBOLS = ("mdvt_view_centers", "mdvt_render_view_batch")

# the entry points include/mdvt_geometry.h declares (per-frame vertex and triangle lists, grey depth), likewise.  Their wrappers are
# geometry_device.enqueue_export (export_batch reads its lists back) and grey_batch
GEOMETRY_SYMBOLS = ("mdvt_export_geometry_batch", "mdvt_depth_grey_batch")

# the entry points include/mdvt_video_mask.h declares (Pillow's Lanczos resize, the mask network's input, the mask from its prediction),
# likewise.  Their wrappers are step_device.lanczos_resize, mask_model_input and mask_from_prediction
VIDEO_MASK_SYMBOLS = ("mdvt_lanczos_resize_u8", "mdvt_mask_model_input", "mdvt_mask_from_prediction")
LANCZOS_AUTO, LANCZOS_FUSED, LANCZOS_TWO_LAUNCH = 0, 1, 2

# the entry points include/mdvt_mvsa.h declares (torch's bilinear resize into the multi-view model, two nearest resizes to depth codes,
# the masked median ratio), likewise.  Their wrappers are step_device.bilinear_model_frames, nearest_depth_codes and ratio_median
MVSA_SYMBOLS = ("mdvt_bilinear_model_frames", "mdvt_nearest_depth_codes", "mdvt_ratio_median")

# the entry points include/mdvt_scene.h declares (the frame difference sums behind scene detection), likewise.  The wrapper is
# step_device.frame_sums
SCENE_SYMBOLS = ("mdvt_scene_frame_sums", "mdvt_scene_vector_path")

# the entry points include/mdvt_megasam.h declares (cv2's area resize, torch's nearest-exact and bilinear resizes into the camera
# tracker, its planes out to video frames), likewise.  Their wrappers are megasam_device.py's
MEGASAM_SYMBOLS = ("mdvt_area_model_frames", "mdvt_megasam_vector_path", "mdvt_tracker_depth", "mdvt_tracker_mask", "mdvt_tracker_outputs")
TRACKER_DEPTH_VIDEO, TRACKER_GREY_VIDEO = 0, 1

# the entry points include/mdvt_inspatio.h declares (the InSpatio-World infill step's masked alignment), likewise.  Their wrappers are
# inspatio_device.py's
INSPATIO_SYMBOLS = ("mdvt_masked_shift_grid", "mdvt_masked_shift_path", "mdvt_flow_warp", "mdvt_inspatio_prepare_eye",
                    "mdvt_inspatio_model_frames", "mdvt_inspatio_composite_eye")
SHIFT_PATH_AUTO, SHIFT_PATH_DIRECT, SHIFT_PATH_TRANSFORM = 0, 1, 2


class MdvtError(RuntimeError):
    def __init__(self, code: int, text: str):
        super().__init__(f"{STATUS_NAMES.get(code, code)}: {text}")
        self.code = code


class MdvtConfig(C.Structure):
    _fields_ = [("mode", C.c_int32), ("remove_edges", C.c_int32), ("edge_points", C.c_int32), ("cull", C.c_int32),
                ("ipd_m", C.c_double), ("max_depth", C.c_double), ("key_rgb", C.c_uint8 * 4), ("workspace_mib", C.c_uint32),
                ("subpixel_bits", C.c_int32),
                # multisampling (took over reserved2 of ABI 0.14; all zero = single sample): samples 0/1 or 4, pattern 0/1, resolve 0/1
                ("samples", C.c_int16), ("sample_pattern", C.c_uint8), ("sample_resolve", C.c_uint8)]


class MdvtFrameParams(C.Structure):
    _fields_ = [("K", C.c_double * 9), ("Krender", C.c_double * 9), ("depth_scale", C.c_double),
                ("convergence_angle", C.c_double), ("T", C.c_double * 16), ("has_T", C.c_int32), ("reserved", C.c_int32)]


class MdvtViewIO(C.Structure):
    _fields_ = [("depth_rgb", C.c_void_p), ("depth_pitch", C.c_size_t), ("depth_stride", C.c_size_t),
                ("color_rgb", C.c_void_p), ("color_pitch", C.c_size_t), ("color_stride", C.c_size_t),
                ("rgb", C.c_void_p), ("rgb_pitch", C.c_size_t), ("rgb_stride", C.c_size_t),
                ("mask", C.c_void_p), ("mask_pitch", C.c_size_t), ("mask_stride", C.c_size_t),
                ("depth", C.c_void_p), ("zout_pitch", C.c_size_t), ("zout_stride", C.c_size_t),
                ("hole_counts", C.c_void_p)]


class MdvtGeometryOpts(C.Structure):
    _fields_ = [("decode", C.c_int32), ("remove_edges", C.c_int32), ("reserved", C.c_int32 * 2), ("max_depth", C.c_double)]


class MdvtGeometryIO(C.Structure):
    _fields_ = [("depth_rgb", C.c_void_p), ("depth_pitch", C.c_size_t), ("depth_stride", C.c_size_t),
                ("color_rgb", C.c_void_p), ("color_pitch", C.c_size_t), ("color_stride", C.c_size_t),
                ("vertices", C.c_void_p), ("vertices_stride", C.c_size_t), ("triangles", C.c_void_p), ("triangles_stride", C.c_size_t),
                ("used_index", C.c_void_p), ("used_stride", C.c_size_t), ("points", C.c_void_p), ("points_stride", C.c_size_t),
                ("point_rgb", C.c_void_p), ("point_rgb_stride", C.c_size_t), ("counts", C.c_void_p)]


class MdvtIO(C.Structure):
    _fields_ = [("depth_rgb", C.c_void_p), ("depth_pitch", C.c_size_t), ("depth_stride", C.c_size_t),
                ("color_rgb", C.c_void_p), ("color_pitch", C.c_size_t), ("color_stride", C.c_size_t),
                ("left_rgb", C.c_void_p), ("right_rgb", C.c_void_p), ("rgb_pitch", C.c_size_t), ("rgb_stride", C.c_size_t),
                ("left_mask", C.c_void_p), ("right_mask", C.c_void_p), ("mask_pitch", C.c_size_t), ("mask_stride", C.c_size_t),
                ("left_depth", C.c_void_p), ("right_depth", C.c_void_p), ("zout_pitch", C.c_size_t), ("zout_stride", C.c_size_t),
                ("left_maskbits", C.c_void_p), ("right_maskbits", C.c_void_p), ("maskbits_pitch", C.c_size_t),
                ("maskbits_stride", C.c_size_t), ("hole_counts", C.c_void_p),
                ("left_seed", C.c_void_p), ("right_seed", C.c_void_p), ("seed_pitch", C.c_size_t), ("seed_stride", C.c_size_t)]


_libs = {}


def lib_path(variant: str = "") -> str:
    return LIB_PATH if not variant else os.path.join(_PKG, f"libmdvt_hip_{variant}.so")


def load():
    """dlopen libmdvt_hip.so and declare prototypes.  Raises if the library has not been built.

    The product library has no tuning / ablation hooks.  With MDVT_LIB_VARIANT=tuning in the environment (read at every
    call, so a test can set it for its own duration) the MDVT_TUNING build of the same objects is loaded instead --
    libmdvt_hip_tuning.so, whose launchers re-read the MDVT_* hooks of csrc/mdvt_internal.h: tools/ and hook-driven tests only."""
    variant = os.environ.get("MDVT_LIB_VARIANT", "")
    if variant in _libs:
        return _libs[variant]
    path = lib_path(variant)
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: the HIP extension has not been built and there is no CPU fallback. "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C metric_depth_video_toolbox_amd/csrc`).")
    L = C.CDLL(path)
    vp = C.c_void_p
    L.mdvt_version.restype = C.c_int
    L.mdvt_version.argtypes = []
    L.mdvt_create.restype = C.c_int
    L.mdvt_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_uint32]
    L.mdvt_destroy.restype = C.c_int
    L.mdvt_destroy.argtypes = [vp]
    L.mdvt_last_error.restype = C.c_char_p
    L.mdvt_last_error.argtypes = [vp]
    L.mdvt_set_config.restype = C.c_int
    L.mdvt_set_config.argtypes = [vp, C.POINTER(MdvtConfig)]
    L.mdvt_set_near_clip.restype = C.c_int
    L.mdvt_set_near_clip.argtypes = [vp, C.c_int32]
    L.mdvt_selftest.restype = C.c_int
    L.mdvt_selftest.argtypes = [vp, C.c_int, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mdvt_render_stereo.restype = C.c_int
    L.mdvt_render_stereo.argtypes = [vp, C.POINTER(MdvtFrameParams), C.POINTER(MdvtIO), vp]
    L.mdvt_render_stereo_batch.restype = C.c_int
    L.mdvt_render_stereo_batch.argtypes = [vp, C.c_int, C.POINTER(MdvtFrameParams), C.POINTER(MdvtIO), vp]
    L.mdvt_decode_depth.restype = C.c_int
    L.mdvt_decode_depth.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_double, C.c_double, vp]
    L.mdvt_encode_depth.restype = C.c_int
    L.mdvt_encode_depth.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_double, C.c_int, vp]
    L.mdvt_edge_filter.restype = C.c_int
    L.mdvt_edge_filter.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_double), C.c_double, C.c_int, vp, vp, vp]
    L.mdvt_infill_using_normals.restype = C.c_int
    L.mdvt_infill_using_normals.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.c_int, vp]
    L.mdvt_mark_lower_side.restype = C.c_int
    L.mdvt_mark_lower_side.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int, vp]
    L.mdvt_touchly_depth.restype = C.c_int
    L.mdvt_touchly_depth.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_double, C.c_double, C.c_int, vp]
    L.mdvt_equirect_tables.restype = C.c_int
    L.mdvt_equirect_tables.argtypes = [C.c_int, C.c_int, C.c_double, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.mdvt_equirect_remap.restype = C.c_int
    L.mdvt_equirect_remap.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_int, vp, vp, vp]
    L.mdvt_masked_blur.restype = C.c_int
    L.mdvt_masked_blur.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp]
    L.mdvt_finish_infill_mask.restype = C.c_int
    L.mdvt_finish_infill_mask.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, vp, vp]
    L.mdvt_finish_infill_mask_stereo.restype = C.c_int
    L.mdvt_finish_infill_mask_stereo.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, vp, vp]
    L.mdvt_finish_infill_mask_heap.restype = C.c_int
    L.mdvt_finish_infill_mask_heap.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_int, vp, vp]
    L.mdvt_finish_infill_mask_heap_stereo.restype = C.c_int
    L.mdvt_finish_infill_mask_heap_stereo.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp, vp, C.c_size_t, C.c_size_t, C.c_int, vp, vp]
    L.mdvt_encode_video_frames.restype = C.c_int
    L.mdvt_encode_video_frames.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                          C.c_uint64, vp, C.c_uint64, vp, vp, vp]
    L.mdvt_swap_rb.restype = C.c_int
    L.mdvt_swap_rb.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_int, vp]
    L.mdvt_normal_infill.restype = C.c_int
    L.mdvt_normal_infill.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_int, vp]
    L.mdvt_infill_using_mask_normals.restype = C.c_int
    L.mdvt_infill_using_mask_normals.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t,
                                                 C.c_int, C.c_int, vp]
    L.mdvt_edge_point_pixels.restype = C.c_int
    L.mdvt_edge_point_pixels.argtypes = [vp, C.POINTER(MdvtFrameParams), vp, C.c_size_t, C.c_int, vp, vp]
    L.mdvt_workspace_bytes.restype = C.c_int
    L.mdvt_workspace_bytes.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.mdvt_release_cached_memory.restype = C.c_int
    L.mdvt_release_cached_memory.argtypes = [C.c_int]
    L.mdvt_cached_memory.restype = C.c_int
    L.mdvt_cached_memory.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mdvt_set_cached_memory_limit.restype = C.c_int
    L.mdvt_set_cached_memory_limit.argtypes = [C.c_uint64]
    L.mdvt_debug_read.restype = C.c_int
    L.mdvt_debug_read.argtypes = [vp, C.c_int, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mdvt_decode_video_frames.restype = C.c_int
    L.mdvt_decode_video_frames.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, C.c_size_t, vp, C.c_uint64, vp, vp, C.c_int, vp, C.c_size_t,
                                          C.c_size_t, C.c_int, vp, vp]
    L.mdvt_ffv1_decode_supported.restype = C.c_char_p
    L.mdvt_ffv1_decode_supported.argtypes = [C.c_char_p, C.c_size_t]
    L.mdvt_decode_video_stream.restype = C.c_int
    L.mdvt_decode_video_stream.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, C.c_size_t, vp, C.c_uint64, vp, vp, C.c_int, C.c_int, vp,
                                          C.c_size_t, C.c_size_t, C.c_int, vp, vp]
    L.mdvt_ffv1_stream_decode_supported.restype = C.c_char_p
    L.mdvt_ffv1_stream_decode_supported.argtypes = [C.c_char_p, C.c_size_t]
    L.mdvt_ffv1_packet_is_key.restype = C.c_int
    L.mdvt_ffv1_packet_is_key.argtypes = [C.c_char_p, C.c_size_t]
    L.mdvt_convergence_depths.restype = C.c_int
    L.mdvt_convergence_depths.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t, C.c_size_t, C.c_int, vp, C.c_size_t, C.c_size_t, C.c_int,
                                         C.c_int, C.c_int, C.c_double, vp, vp, vp]
    L.mdvt_scale_shift_fit.restype = C.c_int
    L.mdvt_scale_shift_fit.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_int,
                                       vp, C.c_size_t, C.c_size_t, vp, vp]
    L.mdvt_metric_depth_codes.restype = C.c_int
    L.mdvt_metric_depth_codes.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, C.c_size_t, vp, C.c_int, C.c_double, C.c_int, C.c_int,
                                          vp, C.c_size_t, C.c_size_t, C.c_int, vp, C.c_size_t, C.c_size_t, vp]
    L.mdvt_depth_video_codes.restype = C.c_int
    L.mdvt_depth_video_codes.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, C.c_size_t, vp, C.c_int, C.c_double, C.c_int, C.c_int,
                                         vp, C.c_size_t, C.c_size_t, C.c_int, vp, C.c_size_t, C.c_size_t, vp]
    st = C.c_size_t
    L.mdvt_model_frames.restype = C.c_int
    L.mdvt_model_frames.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, st, st, C.c_int, C.c_int, C.c_int, C.c_int, vp, st, st, st, vp]
    L.mdvt_depth_prompt.restype = C.c_int
    L.mdvt_depth_prompt.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, st, st, C.c_int, C.c_double, C.c_int, C.c_int, vp, st, st, vp]
    L.mdvt_focal_from_points.restype = C.c_int
    L.mdvt_focal_from_points.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, st, st, st, vp, vp, vp]
    L.mdvt_lanczos_resize_u8.restype = C.c_int
    L.mdvt_lanczos_resize_u8.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, st, st, C.c_int, C.c_int, vp, st, st, C.c_int, vp, vp]
    L.mdvt_mask_model_input.restype = C.c_int
    L.mdvt_mask_model_input.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, st, st, C.c_int, C.c_int, C.c_int, vp, vp, vp, st, st, st, vp]
    L.mdvt_mask_from_prediction.restype = C.c_int
    L.mdvt_mask_from_prediction.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, st, st, C.c_int, C.c_int, C.c_int, vp, st, st, vp]
    L.mdvt_bilinear_model_frames.restype = C.c_int
    L.mdvt_bilinear_model_frames.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, st, st, C.c_int, C.c_int, C.c_int, vp, st, st, st, vp]
    L.mdvt_nearest_depth_codes.restype = C.c_int
    L.mdvt_nearest_depth_codes.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, st, st, C.c_int, C.c_int, vp, st, C.c_double, C.c_int, C.c_int,
                                           vp, st, st, C.c_int, vp, st, st, vp]
    L.mdvt_ratio_median.restype = C.c_int
    L.mdvt_ratio_median.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, st, st, C.c_int, C.c_int, vp, st, st, C.c_int, C.c_int, vp, st, st,
                                    vp, vp, vp]
    L.mdvt_scene_frame_sums.restype = C.c_int
    L.mdvt_scene_frame_sums.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, st, st, C.c_int, vp, st, C.c_int, vp, vp]
    L.mdvt_scene_vector_path.restype = C.c_int
    L.mdvt_scene_vector_path.argtypes = [C.c_int, vp, st, st, vp, st, C.c_int]
    L.mdvt_area_model_frames.restype = C.c_int
    L.mdvt_area_model_frames.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, st, st, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, st, st, st, vp]
    L.mdvt_megasam_vector_path.restype = C.c_int
    L.mdvt_megasam_vector_path.argtypes = [C.c_int, C.c_int, vp, st, st]
    L.mdvt_tracker_depth.restype = C.c_int
    L.mdvt_tracker_depth.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, st, st, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, vp, st, st, vp]
    L.mdvt_tracker_mask.restype = C.c_int
    L.mdvt_tracker_mask.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, st, st, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, st, st, vp]
    L.mdvt_tracker_outputs.restype = C.c_int
    L.mdvt_tracker_outputs.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, st, st, C.c_double, C.c_int, C.c_int, vp, st, st, C.c_int, vp]
    L.mdvt_masked_shift_grid.restype = C.c_int
    L.mdvt_masked_shift_grid.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, st, st, vp, st, st, vp, st, st, C.c_int, vp, vp, vp, vp]
    L.mdvt_inspatio_prepare_eye.restype = C.c_int
    L.mdvt_inspatio_prepare_eye.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, st, st, vp, st, st, C.c_int, C.c_int, vp, st, st, vp, st, st,
                                            vp, st, st, vp, st, st, vp, vp]
    L.mdvt_inspatio_composite_eye.restype = C.c_int
    L.mdvt_inspatio_composite_eye.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, st, st, vp, st, st, vp, st, st, vp, st, st, vp, st, st, vp]
    L.mdvt_inspatio_model_frames.restype = C.c_int
    L.mdvt_inspatio_model_frames.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, st, st, C.c_int, C.c_int, vp, st, st, vp]
    L.mdvt_flow_warp.restype = C.c_int
    L.mdvt_flow_warp.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, st, st, vp, st, st, vp]
    L.mdvt_masked_shift_path.restype = C.c_int
    L.mdvt_masked_shift_path.argtypes = [C.c_int, C.c_int]
    L.mdvt_adapter_prepare_eye.restype = C.c_int
    L.mdvt_adapter_prepare_eye.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, st, st, vp, st, st, C.c_int, C.c_int, vp, st, st, vp, st, st, vp, vp]
    L.mdvt_lhm_moments.restype = C.c_int
    L.mdvt_lhm_moments.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, st, st, vp, st, st, vp, vp]
    L.mdvt_lhm_apply.restype = C.c_int
    L.mdvt_lhm_apply.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, st, st, vp, vp, st, st, vp]
    L.mdvt_adapter_composite_eye.restype = C.c_int
    L.mdvt_adapter_composite_eye.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, st, st, vp, st, st, vp, st, st,
                                             vp, st, st, vp, st, st, vp]
    L.mdvt_m2svid_prepare_eye.restype = C.c_int
    L.mdvt_m2svid_prepare_eye.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, st, st, vp, st, st, vp, C.c_int, C.c_int, st, st,
                                          C.c_int, C.c_int, C.c_int, C.c_int, vp, st, st, vp, st, st, vp, st, st, vp, vp]
    L.mdvt_model_infill_finish.restype = C.c_int
    L.mdvt_model_infill_finish.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, st, st, vp, st, st, vp, st, st, vp, st, st, vp]
    L.mdvt_view_centers.restype = C.c_int
    L.mdvt_view_centers.argtypes = [vp, C.c_int, C.POINTER(MdvtFrameParams), vp, st, st, vp, vp]
    L.mdvt_render_view_batch.restype = C.c_int
    L.mdvt_render_view_batch.argtypes = [vp, C.c_int, C.POINTER(MdvtFrameParams), C.POINTER(MdvtViewIO), vp]
    L.mdvt_export_geometry_batch.restype = C.c_int
    L.mdvt_export_geometry_batch.argtypes = [vp, C.c_int, C.POINTER(MdvtFrameParams), C.POINTER(MdvtGeometryOpts), C.POINTER(MdvtGeometryIO), vp]
    L.mdvt_depth_grey_batch.restype = C.c_int
    L.mdvt_depth_grey_batch.argtypes = [vp, C.c_int, vp, st, st, C.c_double, C.c_int, vp, st, st, vp]
    # the HIP calls SharedContext orders its streams with, reached through the library's own link to the HIP runtime (dlsym
    # searches a library's dependencies), so the events belong to the runtime the kernels are launched by
    L.hipEventCreateWithFlags.restype = C.c_int
    L.hipEventCreateWithFlags.argtypes = [C.POINTER(vp), C.c_uint]
    L.hipEventRecord.restype = C.c_int
    L.hipEventRecord.argtypes = [vp, vp]
    L.hipStreamWaitEvent.restype = C.c_int
    L.hipStreamWaitEvent.argtypes = [vp, vp, C.c_uint]
    L.hipEventDestroy.restype = C.c_int
    L.hipEventDestroy.argtypes = [vp]
    L.hipGetDevice.restype = C.c_int
    L.hipGetDevice.argtypes = [C.POINTER(C.c_int)]
    L.hipSetDevice.restype = C.c_int
    L.hipSetDevice.argtypes = [C.c_int]
    _libs[variant] = L
    return L


def cached_memory(device: int = -1):
    """(idle bytes, idle blocks) of the process-wide workspace pool for GPU `device` (-1: all): mdvt_cached_memory."""
    L = load()
    b, n = C.c_uint64(), C.c_uint64()
    L.mdvt_cached_memory(int(device), C.byref(b), C.byref(n))
    return int(b.value), int(n.value)


def release_cached_memory(device: int = -1) -> None:
    """Return the pool's idle workspace blocks to the driver (mdvt_release_cached_memory)."""
    load().mdvt_release_cached_memory(int(device))


def set_cached_memory_limit(bytes_per_gpu: int) -> None:
    """Idle workspace bytes the process keeps per GPU for the next context (mdvt_set_cached_memory_limit; default 4 GiB)."""
    load().mdvt_set_cached_memory_limit(int(bytes_per_gpu))


def retry_after_release(alloc):
    """Run `alloc()` (a torch allocation); on torch's out-of-memory error hand the library's idle workspace blocks back to the
    driver (torch's allocator cannot see them) and try once more."""
    import torch
    try:
        return alloc()
    except torch.cuda.OutOfMemoryError:
        release_cached_memory(-1)
        torch.cuda.empty_cache()
        return alloc()


def device_index(dev) -> int:
    """The GPU that `dev` (a torch.device, or an int already) names: `cuda` without an index is the current device, not GPU 0."""
    if isinstance(dev, int):
        return dev
    import torch
    return torch.cuda.current_device() if dev.index is None else dev.index


def stream_arg(dev, stream=None):
    """The void* of `stream`, or of the current stream of `dev`, as the library's entry points take it."""
    import torch
    return C.c_void_p((torch.cuda.current_stream(dev) if stream is None else stream).cuda_stream)


def check_tensor(name: str, t, dtype, shape=None, *, ndim=None, device=None, packed: int = 0, contiguous: bool = False,
                 output: bool = False, disjoint: bool = False):
    """The refusal every wrapper makes before a tensor's address reaches the library; returns `t`.  TypeError unless `t` is a torch
    tensor of `dtype` (one dtype or several), ValueError -- naming the argument -- unless it
      is on a GPU, and on `device` (a torch.device, a tensor's, or an index) where one is given;
      has one of `ndim` dimensions and the sizes of `shape` (None = any size; matched against the trailing dimensions);
      packed = k: has its last k dimensions dense (stride 1, then the size of the last: packed pixels; rows and frames at any pitch);
      contiguous: is contiguous (the wrapper passes no pitch of the tensor's own);
      output: has no two elements at one address -- rows at least a row apart, frames at least a frame apart (the library writes
      rows of whole pixels and owns every byte of them: an expanded or folded view would be written twice);
      disjoint: the same for an input of an entry point that takes no pitch below a row and no stride below a frame.
    These raise (an `assert` is stripped by python -O); nothing here runs per launch of a PreparedRender."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    dtypes = dtype if isinstance(dtype, (tuple, list)) else (dtype,)
    if t.dtype not in dtypes:
        raise TypeError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{name} must be on a GPU, it is on {t.device}")
    if device is not None:
        want = device_index(device.device if isinstance(device, torch.Tensor) else device)
        if t.device.index != want:
            raise ValueError(f"{name} is on {t.device}, cuda:{want} is wanted")
    if ndim is not None and t.dim() not in (ndim if isinstance(ndim, (tuple, list)) else (ndim,)):
        raise ValueError(f"{name} must have {ndim} dimensions, got shape {tuple(t.shape)}")
    if shape is not None:
        shape = tuple(shape)
        got = tuple(int(v) for v in t.shape)
        if len(got) < len(shape) or (ndim is None and len(got) != len(shape)) \
                or any(w is not None and int(w) != g for w, g in zip(shape, got[len(got) - len(shape):])):
            raise ValueError(f"{name} must be {tuple('any' if w is None else int(w) for w in shape)}, got {got}")
    dense = 1
    for k in range(1, packed + 1):
        if t.shape[-k] > 1 and t.stride(-k) != dense:
            raise ValueError(f"{name} must have packed pixels (its last {packed} dimension(s) dense; rows and frames may be strided), "
                             f"got strides {tuple(t.stride())}")
        dense *= int(t.shape[-k])
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous, got strides {tuple(t.stride())} for shape {tuple(t.shape)}")
    if output or disjoint:
        need = 1
        for k in range(1, t.dim() + 1):
            if t.shape[-k] > 1 and t.stride(-k) < need:
                raise ValueError(f"{name}{' is written:' if output else ':'} its rows and frames must not overlap, got strides {tuple(t.stride())} "
                                 f"for shape {tuple(t.shape)}")
            if t.shape[-k] > 1:
                need = t.stride(-k) * int(t.shape[-k])
    return t


class _ThreadContexts:
    """The shared contexts of one host thread, by key.  They are closed when the store goes away, which is when its thread ends."""

    def __init__(self):
        self.by_key = {}

    def __del__(self):
        for ctx in self.by_key.values():
            try:
                ctx.close()
            except Exception:
                pass


_shared = threading.local()


def shared_context(device, W: int = 16, H: int = 16) -> "SharedContext":
    """The calling thread's context of a GPU (a torch.device or an index) and render size, for the entry points that keep no state
    in it (for most of them the size is irrelevant: 16 x 16).  A context belongs to the library that made it, so MDVT_LIB_VARIANT
    is part of the key.  A ctx is not thread-safe (include/mdvt.h) and ctypes releases the GIL, so every host thread gets contexts
    of its own; they are closed when the thread ends.  Within a thread the context orders its calls across streams (SharedContext)."""
    key = (device_index(device), int(W), int(H), os.environ.get("MDVT_LIB_VARIANT", ""))
    store = getattr(_shared, "store", None)
    if store is None:
        store = _shared.store = _ThreadContexts()
    ctx = store.by_key.get(key)
    if ctx is None:
        ctx = store.by_key[key] = SharedContext(*key[:3])
    return ctx


def exported_symbols():
    """Names from SYMBOLS that the loaded library actually exports (used by the CPU-only tests)."""
    L = load()
    return [s for s in SYMBOLS if hasattr(L, s)]


class Context:
    """Owns one mdvt_ctx.  ``check`` turns a negative status into MdvtError with the library's text."""

    def __init__(self, device: int, width: int, height: int):
        self._L = load()
        self._h = C.c_void_p()
        rc = self._L.mdvt_create(C.byref(self._h), int(device), int(width), int(height), 0)
        if rc != MDVT_OK:
            raise MdvtError(rc, (self._L.mdvt_last_error(None) or b"").decode())
        self.device, self.W, self.H = int(device), int(width), int(height)

    @property
    def handle(self):
        return self._h

    def check(self, rc: int):
        if rc != MDVT_OK:
            raise MdvtError(rc, (self._L.mdvt_last_error(self._h) or b"").decode())

    def call(self, name: str, *args):
        """`name`(this context, *args) of the library that made the context; a negative status raises MdvtError."""
        self.check(getattr(self._L, name)(self._h, *args))

    def workspace_bytes(self) -> int:
        """Device memory the context owns right now (mdvt_workspace_bytes)."""
        n = C.c_uint64()
        self.call("mdvt_workspace_bytes", C.byref(n))
        return int(n.value)

    def debug_read_queue_block(self):
        """(bytes of the general mesh path's queue block as a uint32 array, info[8]) -- tuning library only (mdvt_debug_read)."""
        import numpy as np
        info = (C.c_uint64 * 8)()
        self.call("mdvt_debug_read", 0, None, 0, info)
        buf = np.zeros(int(info[0]) // 4, dtype=np.uint32)
        if buf.size:
            self.call("mdvt_debug_read", 0, buf.ctypes.data_as(C.c_void_p), buf.nbytes, info)
        return buf, [int(v) for v in info]

    def debug_coherence(self):
        """mdvt_debug_read(what = 1): the cross-XCD coherence test on the queue block (tuning library; overwrites the block).
        -> uint32[80]: [8 w + r] wrong pattern words by writer / reader XCD, [64 + r] wrong atomic sums, [72] total, [73..75] first."""
        import numpy as np
        info = (C.c_uint64 * 8)()
        out = np.zeros(80, dtype=np.uint32)
        self.call("mdvt_debug_read", 1, out.ctypes.data_as(C.c_void_p), out.nbytes, info)
        return out

    def debug_pools(self):
        """mdvt_debug_read(what = 2), tuning library: idle blocks of the two process-wide pools as this context's GPU sees them ->
        dict(param_mine, param_other, ws_mine, ws_other, tag)."""
        info = (C.c_uint64 * 8)()
        self.call("mdvt_debug_read", 2, None, 0, info)
        return dict(param_mine=int(info[0]), param_other=int(info[1]), ws_mine=int(info[2]), ws_other=int(info[3]), tag=int(info[4]))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.mdvt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# the entry points that take a ctx and no stream (every other one takes `void* stream` as its last argument;
# tests/test_shared_context_cpu.py holds the list to the headers)
NO_STREAM = ("mdvt_set_config", "mdvt_set_near_clip", "mdvt_selftest", "mdvt_workspace_bytes", "mdvt_debug_read")

HIP_EVENT_DISABLE_TIMING = 2


class SharedContext(Context):
    """The context shared_context hands out.  Its callers do not see it and still choose a stream, so include/mdvt.h's "ONE stream
    per ctx at a time" is kept here: the context remembers the stream of its latest call and records an event behind that call; a
    call that arrives on another stream first makes that stream wait for the event.  Calls on one stream add the event record
    and nothing else.  Context itself (the renderer's, the benchmark's) records and waits on nothing."""

    def __init__(self, device: int, width: int, height: int):
        super().__init__(device, width, height)
        self._event = None                    # the hipEvent_t, made at the first call
        self._last_stream = None              # the stream (an integer) of the latest call ...
        self._last_event = None               # ... and the event recorded behind it

    def _hip(self, rc: int, what: str):
        if rc != 0:
            raise MdvtError(-2, f"{what} failed with HIP error {rc} while ordering a shared context's streams")

    def _record_event(self, stream: int):
        """Records the context's event on `stream` and returns it (one event serves: a wait takes the record that precedes it)."""
        if self._event is None:
            ev, cur = C.c_void_p(), C.c_int(-1)
            self._hip(self._L.hipGetDevice(C.byref(cur)), "hipGetDevice")
            self._hip(self._L.hipSetDevice(self.device), "hipSetDevice")
            try:
                self._hip(self._L.hipEventCreateWithFlags(C.byref(ev), HIP_EVENT_DISABLE_TIMING), "hipEventCreateWithFlags")
            finally:
                self._L.hipSetDevice(cur.value)
            self._event = ev
        self._hip(self._L.hipEventRecord(self._event, C.c_void_p(stream)), "hipEventRecord")
        return self._event

    def _wait_event(self, stream: int, event):
        """Makes `stream` wait for `event`."""
        self._hip(self._L.hipStreamWaitEvent(C.c_void_p(stream), event, 0), "hipStreamWaitEvent")

    def call(self, name: str, *args):
        if name in NO_STREAM:
            return super().call(name, *args)
        argtypes = getattr(getattr(self._L, name), "argtypes", None)
        if argtypes is not None and argtypes[-1] is not C.c_void_p:
            raise TypeError(f"{name} does not end in `void* stream`: list it in _lib.NO_STREAM, or say here where its stream is")
        stream = args[-1]
        stream = int(getattr(stream, "value", stream) or 0)
        if self._last_event is not None and stream != self._last_stream:
            self._wait_event(stream, self._last_event)
        try:
            super().call(name, *args)
        finally:                              # a call that failed may have enqueued part of its work
            self._last_stream, self._last_event = stream, self._record_event(stream)

    def close(self):
        if getattr(self, "_event", None) is not None:
            self._L.hipEventDestroy(self._event)
            self._event = self._last_event = None
        super().close()
