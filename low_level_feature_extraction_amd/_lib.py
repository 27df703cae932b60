"""ctypes binding of libllfe.so (the C ABI declared in include/llfe.h).

This is the same binding a non-Python caller would write.  Importing
it never falls back to a CPU implementation: if the shared library is missing or cannot
be loaded, ``lib()`` raises.

One HIP runtime per process.  PyTorch-ROCm ships its own ``libamdhip64.so`` (SONAME
``libamdhip64.so.7``, the name libllfe's DT_NEEDED asks for).  When torch is importable
it is imported *before* libllfe is loaded, so the dynamic linker binds libllfe to the
runtime torch already mapped: torch's device pointers and ``cuda_stream`` handles are
then objects of libllfe's own runtime.  ``lib()`` verifies that exactly one
libamdhip64 is mapped and raises otherwise.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libllfe.so")

LLFE_OK = 0
LLFE_ERR_INVALID = -1
LLFE_ERR_HIP = -2
LLFE_ERR_CAPACITY = -3
LLFE_ERR_OOM = -4
LLFE_ERR_UNSUPPORTED = -5

FEATURE_COLORS = 1
FEATURE_SHAPES = 2
FEATURE_SHADOWS = 4
FEATURE_FONTS = 8
LAST_CALL = -1  # LLFE_LAST_CALL (llfe_font_records)

SHAPE_TYPES = {0: "unknown", 1: "triangle", 2: "rectangle", 3: "circle", 4: "polygon"}


MAX_COLORS = 32  # LLFE_MAX_COLORS (include/llfe.h)


class LlfeBatch(C.Structure):
    _fields_ = [
        ("data", C.c_void_p),
        ("n", C.c_int32),
        ("height", C.c_int32),
        ("width", C.c_int32),
        ("on_device", C.c_int32),
        ("noise", C.c_void_p),
        ("noise_on_device", C.c_int32),
        ("n_colors", C.c_int32),
        ("index_base", C.c_int64),
        ("indices", C.c_void_p),
    ]


class LlfeImageResult(C.Structure):
    _fields_ = [
        ("n_colors", C.c_int32),
        ("counts", C.c_int32 * MAX_COLORS),
        ("centers_rgb", (C.c_uint8 * 3) * MAX_COLORS),
        ("pad_", C.c_uint8 * 4),
        ("n_unique", C.c_int64),
        ("compactness", C.c_double),
        ("shadow_sum", C.c_uint64),
        ("shadow_count", C.c_uint64),
        ("shape_offset", C.c_int64),
        ("n_shapes", C.c_int32),
        ("n_contours", C.c_int32),
        ("primary", C.c_char * 8),
        ("background", C.c_char * 8),
        ("accent", (C.c_char * 8) * 3),
        ("shadow_level", C.c_int32),
        ("pad2_", C.c_int32),
    ]


class LlfeImageDesc(C.Structure):
    _fields_ = [
        ("data", C.c_void_p),
        ("height", C.c_int32),
        ("width", C.c_int32),
        ("row_stride", C.c_int64),
        ("on_device", C.c_int32),
        ("noise_on_device", C.c_int32),
        ("noise", C.c_void_p),
    ]


class LlfeThumbOut(C.Structure):
    _fields_ = [
        ("offset", C.c_int64),
        ("height", C.c_int32),
        ("width", C.c_int32),
        ("resized", C.c_int32),
        ("pad_", C.c_int32),
    ]


class LlfeResizeOut(C.Structure):
    _fields_ = [
        ("offset", C.c_int64),
        ("height", C.c_int32),
        ("width", C.c_int32),
        ("interpolation", C.c_int32),
        ("resized", C.c_int32),
    ]


class LlfeColorImage(C.Structure):
    _fields_ = [
        ("pixels", C.c_int64),
        ("field_pixels", C.c_int64),
        ("stage_offset", C.c_int64),
        ("height", C.c_int32),
        ("width", C.c_int32),
        ("steps", C.c_int32),
        ("pass_", C.c_int32),  # `pass` in the header
        ("resized", C.c_int32),
        ("pad_", C.c_int32),
    ]


class LlfeColorWork(C.Structure):
    _fields_ = [
        ("image", C.c_int32),
        ("first_step", C.c_int32),
        ("steps", C.c_int32),
    ]


class LlfeColorPass(C.Structure):
    _fields_ = [
        ("first", C.c_int32),
        ("count", C.c_int32),
        ("work_first", C.c_int32),
        ("work_count", C.c_int32),
        ("tab_steps", C.c_int32),
        ("pad_", C.c_int32),
        ("max_pixels", C.c_int64),
        ("key_stride", C.c_int64),
        ("cube_stride", C.c_int64),
        ("cell_stride", C.c_int64),
        ("stage_bytes", C.c_int64),
    ]


IMAGES_COLORS_ONE_PASS = 1  # LLFE_IMAGES_COLORS_ONE_PASS


class LlfeShapeImage(C.Structure):
    _fields_ = [
        ("pixels", C.c_int64),
        ("class_offset", C.c_int64),
        ("word_offset", C.c_int64),
        ("stage_offset", C.c_int64),
        ("height", C.c_int32),
        ("width", C.c_int32),
        ("strips", C.c_int32),
        ("segs", C.c_int32),
        ("seg_rows", C.c_int32),
        ("tiles_x", C.c_int32),
        ("tiles_y", C.c_int32),
        ("first_tile", C.c_int32),
        ("first_part", C.c_int32),
        ("pass_", C.c_int32),  # `pass` in the header
        ("resized", C.c_int32),
        ("pad_", C.c_int32),
    ]


class LlfeShapeWork(C.Structure):
    _fields_ = [
        ("image", C.c_int32),
        ("strip", C.c_int32),
        ("seg", C.c_int32),
    ]


class LlfeShapePass(C.Structure):
    _fields_ = [
        ("first", C.c_int32),
        ("count", C.c_int32),
        ("work_first", C.c_int32),
        ("work_count", C.c_int32),
        ("tiles", C.c_int32),
        ("pad_", C.c_int32),
        ("class_bytes", C.c_int64),
        ("words", C.c_int64),
        ("first_word", C.c_int64),
        ("stage_bytes", C.c_int64),
        ("workspace_bytes", C.c_int64),
    ]


IMAGES_SHAPES_ONE_PASS = 1  # LLFE_IMAGES_SHAPES_ONE_PASS


class LlfeShape(C.Structure):
    _fields_ = [
        ("type", C.c_int32),
        ("x", C.c_int32),
        ("y", C.c_int32),
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("pad_", C.c_int32),
        ("border_radius", C.c_double),
        ("area", C.c_double),
    ]


class LlfeKernelStat(C.Structure):
    _fields_ = [
        ("name", C.c_char * 32),
        ("launches", C.c_int64),
        ("total_ms", C.c_double),
        ("bytes", C.c_double),
    ]


class LlfeKmeansAttempt(C.Structure):
    _fields_ = [
        ("pp_centers", (C.c_float * 3) * 5),
        ("centers", (C.c_float * 3) * 5),
        ("counts", C.c_int32 * 5),
        ("iters", C.c_int32),
        ("compactness", C.c_double),
    ]


class LlfeFontResult(C.Structure):
    _fields_ = [
        ("n_contours", C.c_int32),
        ("n_regions", C.c_int32),
        ("x", C.c_int32),
        ("y", C.c_int32),
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("region_offset", C.c_int64),
        ("gray_sum", C.c_uint64),
    ]


class LlfeJpegComp(C.Structure):
    _fields_ = [
        ("blocks_w", C.c_int32),
        ("blocks_h", C.c_int32),
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("coef_offset", C.c_int64),
        ("quant_offset", C.c_int64),
    ]


class LlfeJpegDesc(C.Structure):
    _fields_ = [
        ("n_comp", C.c_int32),
        ("sampling", C.c_int32),
        ("comp", LlfeJpegComp * 3),
    ]


class LlfeJpegImage(C.Structure):
    _fields_ = [
        ("slot_offset", C.c_int64),
        ("slot_bytes", C.c_int64),
        ("out_offset", C.c_int64),
        ("height", C.c_int32),
        ("width", C.c_int32),
    ]


class LlfeJpegScan(C.Structure):
    _fields_ = [
        ("record_offset", C.c_int64),
        ("quant_offset", C.c_int32),
        ("table_offset", C.c_int32),
        ("scan_offset", C.c_int32),
        ("scan_bytes", C.c_int32),
        ("mcus_w", C.c_int32),
        ("mcus_h", C.c_int32),
        ("blocks_in_mcu", C.c_int32),
        ("blk_comp", C.c_uint8 * 8),
        ("blk_x", C.c_uint8 * 8),
        ("blk_y", C.c_uint8 * 8),
        ("blk_dc", C.c_uint8 * 8),
        ("blk_ac", C.c_uint8 * 8),
        ("comp_hs", C.c_uint8 * 4),
        ("comp_vs", C.c_uint8 * 4),
        ("restart_interval", C.c_int32),
    ]


class LlfePngDesc(C.Structure):
    _fields_ = [
        ("record_offset", C.c_int64),
        ("raw_bytes", C.c_int64),
        ("deflate_bytes", C.c_int32),
        ("bpp", C.c_int32),
        ("row_bytes", C.c_int32),
        ("adler", C.c_uint32),
    ]


JPEG_GRAY, JPEG_444, JPEG_422, JPEG_420 = 1, 2, 3, 4  # LLFE_JPEG_*
JPEG_HUFF_TABLE_BYTES, JPEG_RECORD_HEADER = 400, 2048  # LLFE_JPEG_HUFF_TABLE_BYTES, LLFE_JPEG_RECORD_HEADER
JPEG_SUBSEQUENCE_BYTES = 128  # csrc/jpeg_huff_core.h kSub
JPEG_PARSE_RESTARTS = 1  # LLFE_JPEG_PARSE_RESTARTS
JPEG_ORIENT = 4  # LLFE_JPEG_ORIENT

# every symbol declared in include/llfe.h, with its ctypes signature
_vp, _i32, _i64, _u32, _u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64
SIGNATURES = {
    "llfe_init": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "llfe_destroy": (C.c_int, [_vp]),
    "llfe_last_error": (C.c_char_p, [_vp]),
    "llfe_abi_version": (C.c_int, []),
    "llfe_hip_runtime": (C.c_char_p, []),
    "llfe_default_host_threads": (C.c_int, []),
    "llfe_set_profiling": (C.c_int, [_vp, C.c_int]),
    "llfe_set_concurrency": (C.c_int, [_vp, C.c_int]),
    "llfe_set_contour_mode": (C.c_int, [_vp, C.c_int]),
    "llfe_get_contour_mode": (C.c_int, [_vp]),
    "llfe_set_inflight": (C.c_int, [_vp, _i32]),
    "llfe_get_inflight": (C.c_int, [_vp]),
    "llfe_submit_batch": (C.c_int, [_vp, C.POINTER(LlfeBatch), _u32, _u64, _vp, C.POINTER(C.c_int64)]),
    "llfe_collect_batch": (C.c_int, [_vp, C.c_int64, _vp, _vp, C.c_int64, C.POINTER(C.c_int64)]),
    "llfe_submit_images": (C.c_int, [_vp, _vp, _i32, _u32, _i32, _u64, _vp, _vp, C.POINTER(C.c_int64)]),
    "llfe_batch_capacity": (C.c_int, [_i32, _i32]),
    "llfe_kernel_stats": (C.c_int, [_vp, C.POINTER(LlfeKernelStat), _i32]),
    "llfe_host_contour_stats": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32), _i32]),
    "llfe_process_batch": (C.c_int, [_vp, C.POINTER(LlfeBatch), _u32, _u64, _vp, _vp, _i64, C.POINTER(C.c_int64), _vp]),
    "llfe_process_images": (C.c_int, [_vp, _vp, _i32, _u32, _i32, _i32, _u64, _i64, _vp, _vp, _i64,
                                      C.POINTER(C.c_int64), _vp]),
    "llfe_process_images_flags": (C.c_int, [_vp, _vp, _i32, _u32, _i32, _i32, _u64, _i64, _vp, _vp, _i64,
                                            C.POINTER(C.c_int64), _vp, _u32]),
    "llfe_colors_images_layout": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _i64, C.POINTER(C.c_int64), _vp, _i32,
                                            C.POINTER(C.c_int32)]),
    "llfe_process_images_routes": (C.c_int, [_vp, _vp, _i32, _u32, _i32, _i32, _u64, _i64, _vp, _vp, _i64,
                                             C.POINTER(C.c_int64), _vp, _u32, _u32]),
    "llfe_shapes_images_layout": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _i64, C.POINTER(C.c_int64), _vp, _i32,
                                            C.POINTER(C.c_int32)]),
    "llfe_shape_bits_images": (C.c_int, [_vp, _vp, _i32, _vp, _i64, _vp]),
    "llfe_shadow_stats_images": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "llfe_hysteresis_images": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _i64]),
    "llfe_color_unique_images": (C.c_int, [_vp, _vp, _i32, _u64, _i64, _vp, _i64, _vp, _vp]),
    "llfe_gray_blur5": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "llfe_shape_mask": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "llfe_edge_classes": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "llfe_canny": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "llfe_hysteresis": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "llfe_dilate3": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "llfe_font_binary": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "llfe_font_detect": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _i64, C.POINTER(C.c_int64), _vp]),
    "llfe_font_bits": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "llfe_font_bits_images": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "llfe_font_bits_tiling": (C.c_int, [_i32, _i32, C.POINTER(_i32), C.POINTER(_i32)]),
    "llfe_font_records": (C.c_int, [_vp, _i64, _vp, _i32]),
    "llfe_text_binary": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, C.POINTER(_i32), _vp]),
    "llfe_text_size": (C.c_int, [_i32, _i32, C.POINTER(_i32), C.POINTER(_i32)]),
    "llfe_shadow_stats": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "llfe_color_unique": (C.c_int, [_vp, C.POINTER(LlfeBatch), _u64, _vp, _vp, _vp]),
    "llfe_kmeans": (C.c_int, [_vp, _vp, _i64, _vp, _i32, _i32, _u64, _i64, _vp, _vp]),
    "llfe_kmeans_attempts": (C.c_int, [_vp, _i32, _vp]),
    "llfe_kmeans_attempts_k": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "llfe_palette_rules": (C.c_int, [_vp, _vp, _i32, _vp]),
    "llfe_resize_lanczos_pil": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _vp]),
    "llfe_reduce_pil": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "llfe_thumbnail_size": (C.c_int, [_i32, _i32, _i32, _i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "llfe_resize_cv": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _vp]),
    "llfe_preprocess_size": (C.c_int, [_i32, _i32, _i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32)]),
    "llfe_thumbnail_pil": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int32), _vp]),
    "llfe_thumbnail_pil_batch": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i64,
                                           C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp]),
    "llfe_thumbnail_images_layout": (C.c_int, [_vp, _i32, _i32, _i32, _vp, C.POINTER(C.c_int64)]),
    "llfe_thumbnail_pil_images": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _i64, _vp, _vp]),
    "llfe_thumbnail_images_tiling": (C.c_int, [C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "llfe_preprocess_images_layout": (C.c_int, [_vp, _i32, _i32, _vp, C.POINTER(C.c_int64)]),
    "llfe_preprocess_images": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i64, _vp, _vp]),
    "llfe_resize_cv_images": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _i64, _vp, _vp]),
    "llfe_resize_cv_images_tiling": (C.c_int, [C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "llfe_find_contours":(C.c_int, [_vp, _i32, _i32, _vp, _i64, _vp, _i32, C.POINTER(C.c_int64)]),
    "llfe_border_radius": (C.c_double, [_vp, _i32, C.c_double]),
    "llfe_classify_contour": (C.c_int, [_vp, _i32, C.POINTER(LlfeShape)]),
    "llfe_shapes_from_mask": (C.c_int, [_vp, _i32, _i32, _vp, _i32, C.POINTER(C.c_int32)]),
    "llfe_find_contours_gpu": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i64, _vp, _i32, C.POINTER(C.c_int64)]),
    "llfe_shapes_from_masks_gpu": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _i64, _vp, _vp,
                                             C.POINTER(C.c_int64)]),
    "llfe_png_info": (C.c_int, [_vp, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "llfe_decode_png_batch": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32]),
    "llfe_image_info": (C.c_int, [_vp, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "llfe_decode_batch": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32]),
    "llfe_decoder_info": (C.c_int, [C.c_char_p, _i32]),
    "llfe_jpeg_coef_slot_bytes": (C.c_int64, [_i32, _i32]),
    "llfe_jpeg_read_coefs_batch": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _i64, C.POINTER(LlfeJpegDesc), _vp, _i32]),
    "llfe_jpeg_reconstruct": (C.c_int, [_vp, _vp, _i64, C.POINTER(LlfeJpegDesc), _i32, _i32, _i32, _vp, _vp]),
    "llfe_jpeg_images_layout": (C.c_int, [_vp, _vp, _i32, C.POINTER(LlfeJpegImage), C.POINTER(_i64), _vp, _i32]),
    "llfe_jpeg_read_coefs_images": (C.c_int, [_vp, _vp, _i32, C.POINTER(LlfeJpegImage), _vp, _i64,
                                              C.POINTER(LlfeJpegDesc), _vp, _i32]),
    "llfe_jpeg_reconstruct_images": (C.c_int, [_vp, _vp, _i64, C.POINTER(LlfeJpegImage), C.POINTER(LlfeJpegDesc), _i32,
                                               _vp, _i64, _vp]),
    "llfe_jpeg_images_layout_flags": (C.c_int, [_vp, _vp, _i32, C.POINTER(LlfeJpegImage), C.POINTER(_i64), _vp, _i32,
                                                _vp, _u32]),
    "llfe_jpeg_orient_reference": (C.c_int, [_vp, _i32, _i32, _i32, _vp]),
    "llfe_jpeg_read_coefs_images_flags": (C.c_int, [_vp, _vp, _i32, C.POINTER(LlfeJpegImage), _vp, _i64,
                                                    C.POINTER(LlfeJpegDesc), _vp, _i32, _u32]),
    "llfe_jpeg_reconstruct_images_oriented": (C.c_int, [_vp, _vp, _i64, C.POINTER(LlfeJpegImage),
                                                        C.POINTER(LlfeJpegDesc), _vp, _i32, _vp, _i64, _vp]),
    "llfe_jpeg_images_tiling": (C.c_int, [_i32, C.POINTER(_i32), C.POINTER(_i32)]),
    "llfe_jpeg_parse_batch": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _i64, _i64, C.POINTER(LlfeJpegDesc),
                                        C.POINTER(LlfeJpegScan), _vp, _i32]),
    "llfe_jpeg_parse_batch_flags": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _i64, _i64, C.POINTER(LlfeJpegDesc),
                                              C.POINTER(LlfeJpegScan), _vp, _i32, _u32]),
    "llfe_jpeg_entropy_reference": (C.c_int, [_vp, _i64, C.POINTER(LlfeJpegScan), C.POINTER(LlfeJpegDesc), _i32, _i32,
                                              _i32, _vp, _i64, _vp, _i32]),
    "llfe_jpeg_entropy_decode": (C.c_int, [_vp, _vp, _i64, C.POINTER(LlfeJpegScan), C.POINTER(LlfeJpegDesc), _i32, _i32,
                                           _i32, _vp, _i64, _vp, _vp]),
    "llfe_jpeg_records_layout": (C.c_int, [_vp, C.POINTER(LlfeJpegImage), _i32, _vp, C.POINTER(_i64)]),
    "llfe_jpeg_parse_images": (C.c_int, [_vp, _vp, _i32, C.POINTER(LlfeJpegImage), _vp, _vp, _i64,
                                         C.POINTER(LlfeJpegDesc), C.POINTER(LlfeJpegScan), _vp, _i32, _u32]),
    "llfe_jpeg_entropy_reference_images": (C.c_int, [_vp, _i64, C.POINTER(LlfeJpegScan), C.POINTER(LlfeJpegDesc),
                                                     C.POINTER(LlfeJpegImage), _i32, _vp, _i64, _vp, _i32]),
    "llfe_jpeg_entropy_decode_images": (C.c_int, [_vp, _vp, _i64, C.POINTER(LlfeJpegScan), C.POINTER(LlfeJpegDesc),
                                                  C.POINTER(LlfeJpegImage), _i32, _vp, _i64, _vp, _vp]),
    "llfe_png_parse_batch": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _i64, C.POINTER(LlfePngDesc), _vp, _i32]),
    "llfe_png_decode_reference": (C.c_int, [_vp, _i64, C.POINTER(LlfePngDesc), _i32, _i32, _i32, _vp, _i64, _vp, _vp]),
    "llfe_png_decode_device": (C.c_int, [_vp, _vp, _i64, C.POINTER(LlfePngDesc), _i32, _i32, _i32, _vp, _i64, _vp, _vp,
                                         _vp]),
}

_lib = None
_lock = threading.Lock()


class LlfeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"llfe error {code}: {msg}")
        self.code = code


def hip_runtimes_mapped() -> list:
    """Distinct libamdhip64 files mapped into this process (from /proc/self/maps)."""
    paths = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                p = line.split()[-1] if line.strip() else ""
                if "libamdhip64" in os.path.basename(p):
                    paths.add(os.path.realpath(p))
    except OSError:  # pragma: no cover - non-Linux
        pass
    return sorted(paths)


def lib():
    """Load libllfe.so (building it from source if it is absent or stale), bound to the
    same HIP runtime as PyTorch when torch is importable."""
    global _lib
    with _lock:
        if _lib is None:
            from . import _build

            try:  # torch first: its libamdhip64 becomes the one libllfe binds to
                import torch  # noqa: F401
            except ImportError:  # pragma: no cover - C-only deployments
                pass
            if _build._stale():
                try:
                    _build.build()
                except Exception as e:  # pragma: no cover - surfaced to caller
                    if not os.path.exists(LIB_PATH):
                        raise RuntimeError(f"libllfe.so is missing and could not be built: {e}") from e
            L = C.CDLL(os.environ.get("LLFE_LIB_PATH", LIB_PATH))
            # (tools/debug/identity.sh runs older builds, which lack later entry points)
            old_ok = os.environ.get("LLFE_LIB_PATH") is not None
            for name, (res, args) in SIGNATURES.items():
                if old_ok and not hasattr(L, name):
                    continue
                f = getattr(L, name)
                f.restype = res
                f.argtypes = args
            rts = hip_runtimes_mapped()
            if len(rts) > 1:
                raise RuntimeError("two HIP runtimes are mapped into this process (%s); libllfe is bound to %s. "
                                   "Import torch before loading libllfe so both share one runtime."
                                   % (", ".join(rts), L.llfe_hip_runtime().decode()))
            _lib = L
    return _lib


def check(ctx, rc):
    if rc < 0:
        msg = lib().llfe_last_error(ctx)
        raise LlfeError(rc, msg.decode() if msg else "")
    return rc
