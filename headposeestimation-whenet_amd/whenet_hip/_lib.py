"""ctypes binding of libwhenet_hip.so (include/whenet_hip.h).  Thin: argument marshalling
and error-code -> exception mapping only.  There is no Python/NumPy implementation of the
path behind it -- if the library or a gfx950 device is missing, callers get an exception.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

ABI_VERSION = 6
F32, F16, F32S = 0, 1, 2          # include/whenet_hip.h WHENET_F32 / WHENET_F16 / WHENET_F32S
OK, ENOENT, EIO, ENOMEM, ENODEV, EINVAL, EFORMAT, EHIP = 0, -2, -5, -12, -19, -22, -74, -1000
EOVERFLOW = -75                   # WHENET_EOVERFLOW: the result does not fit the caller's capacity
MAX_INFLIGHT = 4

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "..", "lib", "libwhenet_hip.so")


class Info(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("dtype", C.c_int32), ("device_id", C.c_int32),
                ("compute_units", C.c_int32), ("params_backbone", C.c_int64),
                ("params_heads", C.c_int64), ("n_tensors", C.c_int32),
                ("n_kernels_per_forward", C.c_int32), ("macs_per_crop", C.c_int64),
                ("arena_bytes", C.c_int64), ("capacity", C.c_int32), ("graph_enabled", C.c_int32),
                ("device_name", C.c_char * 64), ("arch", C.c_char * 32)]


class LaunchStat(C.Structure):
    _fields_ = [("layer", C.c_char * 32), ("kind", C.c_char * 16), ("kernel", C.c_char * 64),
                ("avg_us", C.c_double), ("alg_bytes", C.c_double), ("alg_flops", C.c_double),
                ("crops", C.c_int32), ("chains", C.c_int32)]


_P = C.c_void_p


class YuvFrameC(C.Structure):
    """whenet_yuv_frame_t: the planes of one 4:2:0 frame as a decoder hands them out."""
    _fields_ = [("plane", _P * 3), ("pitch", C.c_int * 3), ("format", C.c_int), ("matrix", C.c_int), ("h", C.c_int), ("w", C.c_int)]


class YuvxFrameC(C.Structure):
    """whenet_yuvx_frame_t (include/whenet_hip_yuv_ext.h): a frame as a layout times a sample container (8 or 16 bit, with a shift)."""
    _fields_ = [("plane", _P * 3), ("pitch", C.c_int * 3), ("layout", C.c_int), ("container", C.c_int), ("shift", C.c_int),
                ("matrix", C.c_int), ("h", C.c_int), ("w", C.c_int)]


class SurfaceC(C.Structure):
    """whenet_surface_t: a destination of the pose overlay (packed pixels, NV12 or I420; host or device memory)."""
    _fields_ = [("plane", _P * 3), ("pitch", C.c_int * 3), ("format", C.c_int), ("matrix", C.c_int), ("on_device", C.c_int)]


class JpegInfoC(C.Structure):
    """whenet_jpeg_info_t: the header SOI..SOS of a baseline JPEG stream, self-contained."""
    _fields_ = [("h", C.c_int32), ("w", C.c_int32), ("components", C.c_int32), ("hs", C.c_int32), ("vs", C.c_int32),
                ("qt", C.c_int32 * 3), ("dc", C.c_int32 * 3), ("ac", C.c_int32 * 3), ("restart_interval", C.c_int32),
                ("intervals", C.c_int32), ("data_offset", C.c_int64), ("q", (C.c_uint8 * 64) * 4), ("q_present", C.c_uint8 * 4),
                ("huff_counts", (C.c_uint8 * 16) * 4), ("huff_values", (C.c_uint8 * 256) * 4), ("huff_present", C.c_uint8 * 4)]


class JpegScanC(C.Structure):
    """whenet_jpeg_scan_t: one scan of a (progressive) JPEG stream."""
    _fields_ = [("ns", C.c_int32), ("comp", C.c_int32 * 3), ("ss", C.c_int32), ("se", C.c_int32), ("ah", C.c_int32), ("al", C.c_int32),
                ("dc", C.c_int32 * 3), ("ac", C.c_int32 * 3), ("tables", C.c_int32), ("ri", C.c_int32), ("intervals", C.c_int32),
                ("level", C.c_int32), ("first_item", C.c_int32), ("progressive", C.c_int32), ("data_offset", C.c_int64),
                ("data_bytes", C.c_int64)]


JPEG_PROG_MAX_SCANS = 128
JPEG_PROG_COUNTERS = ("scans", "items", "levels", "max_eobrun", "refine_zrl", "correction_bits", "corrections")

_PROTOS = {
    "whenet_create": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.POINTER(_P)]),
    "whenet_create_from_memory": (C.c_int, [_P, C.c_size_t, C.c_int, C.c_int, C.POINTER(_P)]),
    "whenet_create_postproc": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "whenet_destroy": (None, [_P]),
    "whenet_last_error": (C.c_char_p, [_P]),
    "whenet_get_info": (C.c_int, [_P, C.POINTER(Info)]),
    "whenet_set_option": (C.c_int, [_P, C.c_char_p, C.c_long]),
    "whenet_forward_u8": (C.c_int, [_P, _P, C.c_int, _P, _P, _P]),
    "whenet_forward_f32": (C.c_int, [_P, _P, C.c_int, _P, _P, _P]),
    "whenet_forward_u8_device": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P]),
    "whenet_sync": (C.c_int, [_P]),
    "whenet_submit_u8": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int)]),
    "whenet_collect": (C.c_int, [_P, C.c_int, _P, _P, _P]),
    "whenet_frame_rects": (C.c_int, [C.c_int, C.c_int, _P, C.c_int, _P]),
    "whenet_normalise_table": (C.c_int, [_P]),
    "whenet_submit_frame": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.POINTER(C.c_int)]),
    "whenet_op_crop_resize": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P]),
    "whenet_letterbox_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32 * 4), C.c_int, _P, _P, C.c_int,
                                        C.POINTER(C.c_int)]),
    "whenet_op_letterbox": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "whenet_frame_begin": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "whenet_frame_letterbox": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "whenet_frame_heads": (C.c_int, [_P, C.c_int, _P, C.c_int]),
    "whenet_yolo_eval": (C.c_int, [_P, C.POINTER(_P), _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_float, C.c_float,
                                   C.c_float, C.c_float, C.c_int, _P, _P, _P, _P, C.POINTER(C.c_int), _P, _P]),
    "whenet_detector_load": (C.c_int, [_P, C.c_char_p]),
    "whenet_detector_load_from_memory": (C.c_int, [_P, _P, C.c_size_t]),
    "whenet_detector_spec": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32 * 12), C.POINTER(C.c_int)]),
    "whenet_op_dconv": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int,
                                  _P, C.c_int, _P]),
    "whenet_op_dpool": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "whenet_detector_forward": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "whenet_op_detect": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_float, C.c_float, C.c_int,
                                   _P, _P, _P, C.POINTER(C.c_int)]),
    "whenet_frame_detect": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_float, C.c_float, C.c_int, _P, _P, _P,
                                      C.POINTER(C.c_int)]),
    "whenet_frame_detect_heads": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_float, C.c_float, C.c_int]),
    "whenet_collect_detect": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int), _P, _P, _P, _P, _P, _P, _P, _P]),
    "whenet_op_head_plan": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P]),
    "whenet_crop_plan": (C.c_int, [_P, _P]),
    "whenet_clip_begin": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "whenet_clip_detect_heads": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int,
                                           C.POINTER(C.c_int)]),
    "whenet_collect_clip": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                      C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "whenet_op_letterbox_batch": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "whenet_yolo_eval_batch": (C.c_int, [_P, C.POINTER(_P), C.c_int, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_float, C.c_float,
                                         C.c_float, C.c_float, C.c_int, _P, _P, _P, _P, _P]),
    "whenet_clip_begin_mixed": (C.c_int, [_P, C.POINTER(_P), C.c_int, _P, _P, C.c_int, C.POINTER(C.c_int)]),
    "whenet_op_letterbox_mixed": (C.c_int, [_P, C.POINTER(_P), C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "whenet_yolo_eval_mixed": (C.c_int, [_P, C.POINTER(_P), C.c_int, _P, _P, C.c_int, _P, C.c_int, C.c_int, _P, C.c_float, C.c_float,
                                         C.c_int, _P, _P, _P, _P, _P]),
    "whenet_letterbox_cache_stats": (C.c_int, [_P, C.POINTER(C.c_int32 * 4)]),
    "whenet_op_head_compact": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "whenet_yuv_to_bgr_host": (C.c_int, [C.POINTER(YuvFrameC), _P]),
    "whenet_op_yuv_to_bgr": (C.c_int, [_P, C.POINTER(YuvFrameC), C.c_int, C.POINTER(_P)]),
    "whenet_frame_begin_yuv": (C.c_int, [_P, C.POINTER(YuvFrameC), C.POINTER(C.c_int)]),
    "whenet_clip_begin_yuv": (C.c_int, [_P, C.POINTER(YuvFrameC), C.c_int, C.POINTER(C.c_int)]),
    "whenet_frame_begin_device": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.POINTER(C.c_int)]),
    "whenet_clip_begin_device": (C.c_int, [_P, C.POINTER(_P), _P, C.c_int, _P, _P, C.c_int, _P, C.POINTER(C.c_int)]),
    "whenet_frame_begin_yuv_device": (C.c_int, [_P, C.POINTER(YuvFrameC), _P, C.POINTER(C.c_int)]),
    "whenet_clip_begin_yuv_device": (C.c_int, [_P, C.POINTER(YuvFrameC), C.c_int, _P, C.POINTER(C.c_int)]),
    "whenet_op_pack_device": (C.c_int, [_P, C.POINTER(_P), _P, C.c_int, _P, _P, _P, C.POINTER(_P)]),
    "whenet_op_yuv_to_bgr_device": (C.c_int, [_P, C.POINTER(YuvFrameC), C.c_int, _P, C.POINTER(_P)]),
    "whenet_overlay_segments": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, _P, C.POINTER(C.c_int32)]),
    "whenet_annotate_host": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.POINTER(SurfaceC)]),
    "whenet_op_annotate": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.POINTER(SurfaceC)]),
    "whenet_frame_annotate": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(SurfaceC), _P]),
    "whenet_overlay_labels": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, _P, _P, C.POINTER(C.c_int32)]),
    "whenet_overlay_glyph": (C.c_int, [C.c_int, _P]),
    "whenet_annotate_host_ex": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.POINTER(SurfaceC), C.c_int]),
    "whenet_op_annotate_ex": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.POINTER(SurfaceC), C.c_int]),
    "whenet_frame_annotate_ex": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(SurfaceC), _P, C.c_int]),
    "whenet_jpeg_header": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.c_int, _P]),
    "whenet_jpeg_bound": (C.c_int64, [C.c_int, C.c_int]),
    "whenet_jpeg_encode_host": (C.c_int, [C.POINTER(SurfaceC), C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "whenet_op_jpeg_encode": (C.c_int, [_P, C.POINTER(SurfaceC), C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "whenet_jpeg_encode_device": (C.c_int, [_P, C.POINTER(SurfaceC), C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P, _P]),
    "whenet_frame_annotate_jpeg": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P, _P]),
    "whenet_jpeg_optimal_table": (C.c_int, [_P, _P, _P, C.POINTER(C.c_int)]),
    "whenet_jpeg_header_ex": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P]),
    "whenet_jpeg_bound_ex": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "whenet_jpeg_encode_host_ex": (C.c_int, [C.POINTER(SurfaceC), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64,
                                             C.POINTER(C.c_int64), _P]),
    "whenet_op_jpeg_encode_ex": (C.c_int, [_P, C.POINTER(SurfaceC), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64,
                                           C.POINTER(C.c_int64), _P]),
    "whenet_jpeg_encode_device_ex": (C.c_int, [_P, C.POINTER(SurfaceC), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64,
                                               _P, _P]),
    "whenet_frame_annotate_jpeg_ex": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P, _P]),
    "whenet_jpeg_parse": (C.c_int, [_P, C.c_int64, C.POINTER(JpegInfoC)]),
    "whenet_jpeg_decode_host": (C.c_int, [_P, C.c_int64, C.POINTER(SurfaceC), C.c_int, _P]),
    "whenet_jpeg_decode_planes_host": (C.c_int, [_P, C.c_int64, C.POINTER(_P), _P, _P]),
    "whenet_op_jpeg_decode": (C.c_int, [_P, _P, C.c_int64, C.POINTER(SurfaceC), C.c_int, _P]),
    "whenet_jpeg_decode_device": (C.c_int, [_P, C.POINTER(JpegInfoC), _P, C.c_int64, C.POINTER(SurfaceC), C.c_int, _P, _P]),
    "whenet_jpeg_decode_segmented_host": (C.c_int, [_P, C.c_int64, C.POINTER(SurfaceC), C.c_int, C.c_int, C.c_int, _P, _P]),
    "whenet_jpeg_decode_segmented_planes_host": (C.c_int, [_P, C.c_int64, C.POINTER(_P), _P, C.c_int, C.c_int, _P, _P]),
    "whenet_op_jpeg_decode_ex": (C.c_int, [_P, _P, C.c_int64, C.POINTER(SurfaceC), C.c_int, C.c_int, C.c_int, _P, _P]),
    "whenet_jpeg_decode_counters": (C.c_int, [_P, C.POINTER(C.c_int64 * 4)]),
    "whenet_jpeg_seg_dc_scan_host": (C.c_int, [_P, C.c_int64, C.c_int, _P]),
    "whenet_frame_begin_jpeg": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.POINTER(C.c_int), _P]),
    "whenet_clip_begin_jpeg": (C.c_int, [_P, C.POINTER(_P), _P, C.c_int, C.c_int, C.POINTER(C.c_int), _P]),
    "whenet_op_jpeg_decode_clip": (C.c_int, [_P, C.POINTER(_P), _P, C.c_int, C.POINTER(SurfaceC), C.c_int, _P, C.c_int, C.c_int]),
    "whenet_jpeg_clip_plan": (C.c_int, [C.POINTER(JpegInfoC), _P, C.c_int, C.c_int, C.c_int, _P]),
    "whenet_jpeg_clip_counters": (C.c_int, [_P, C.POINTER(C.c_int64 * 4)]),
    "whenet_jpeg_decode_rule_host": (C.c_int, [_P, C.c_int64, C.POINTER(SurfaceC), C.c_int, C.c_int, _P]),
    "whenet_jpeg_decode_segmented_rule_host": (C.c_int, [_P, C.c_int64, C.POINTER(SurfaceC), C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "whenet_op_jpeg_decode_rule": (C.c_int, [_P, _P, C.c_int64, C.POINTER(SurfaceC), C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "whenet_op_jpeg_decode_clip_rule": (C.c_int, [_P, C.POINTER(_P), _P, C.c_int, C.POINTER(SurfaceC), C.c_int, _P, C.c_int, C.c_int, C.c_int]),
    "whenet_frame_begin_jpeg_rule": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int), _P]),
    "whenet_clip_begin_jpeg_rule": (C.c_int, [_P, C.POINTER(_P), _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), _P]),
    "whenet_jpeg_parse_scans": (C.c_int, [_P, C.c_int64, C.POINTER(JpegInfoC), C.POINTER(JpegScanC), C.c_int, C.POINTER(C.c_int)]),
    "whenet_jpeg_decode_progressive_host": (C.c_int, [_P, C.c_int64, C.POINTER(SurfaceC), C.c_int, C.c_int, _P]),
    "whenet_jpeg_decode_progressive_planes_host": (C.c_int, [_P, C.c_int64, C.POINTER(_P), _P, C.c_int, _P]),
    "whenet_jpeg_progressive_coefficients_host": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int64, _P, _P]),
    "whenet_op_jpeg_decode_progressive": (C.c_int, [_P, _P, C.c_int64, C.POINTER(SurfaceC), C.c_int, C.c_int, _P, _P]),
    "whenet_frame_begin_jpeg_progressive": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int), _P]),
    "whenet_jpeg_progressive_counters": (C.c_int, [_P, C.POINTER(C.c_int64 * 4)]),
    "whenet_op_jpeg_decode_clip_progressive": (C.c_int, [_P, C.POINTER(_P), _P, C.c_int, C.POINTER(SurfaceC), C.c_int, _P, C.c_int, C.c_int,
                                                         C.c_int]),
    "whenet_clip_begin_jpeg_progressive": (C.c_int, [_P, C.POINTER(_P), _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), _P]),
    "whenet_jpeg_clip_plan_progressive": (C.c_int, [C.POINTER(_P), _P, C.c_int, C.c_int, C.c_int, _P]),
    "whenet_jpeg_orientation": (C.c_int, [_P, C.c_int64]),
    "whenet_jpeg_add_default_tables": (C.c_int, [_P, C.c_int64, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "whenet_jpeg_decode_oriented_host": (C.c_int, [_P, C.c_int64, C.POINTER(SurfaceC), C.c_int, C.c_int, C.c_int, _P]),
    "whenet_op_jpeg_decode_oriented": (C.c_int, [_P, _P, C.c_int64, C.POINTER(SurfaceC), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P,
                                                 _P, _P]),
    "whenet_op_jpeg_decode_clip_oriented": (C.c_int, [_P, C.POINTER(_P), _P, C.c_int, C.POINTER(SurfaceC), C.c_int, _P, C.c_int, C.c_int, C.c_int,
                                                      C.c_int, C.c_int, _P]),
    "whenet_frame_begin_jpeg_oriented": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), _P, _P]),
    "whenet_clip_begin_jpeg_oriented": (C.c_int, [_P, C.POINTER(_P), _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), _P, _P]),
    "whenet_profile": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(LaunchStat), C.c_int, C.POINTER(C.c_int)]),
    "whenet_op_stem": (C.c_int, [_P, _P, C.c_int, _P]),
    "whenet_op_block": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, _P, _P]),
    "whenet_op_block_range": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, _P]),
    "whenet_op_head": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P]),
    "whenet_op_decode": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "whenet_block_spec": (C.c_int, [C.c_int, C.POINTER(C.c_int32 * 8)]),
    "whenet_dw_plan": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int32 * 12)]),
    "whenet_front_plan": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int32 * 12)]),
    "whenet_front2_static_check": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "whenet_pw_static_check": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "whenet_front_static_check": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "whenet_device_alloc": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "whenet_device_free": (C.c_int, [_P, _P]),
    "whenet_memcpy_h2d": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "whenet_memcpy_d2h": (C.c_int, [_P, _P, _P, C.c_size_t]),
}
EXPORTS = tuple(_PROTOS)
# the entry points of include/whenet_hip_jpeg_accept.h (JPEG DECODER, LAYOUTS): a header and a table of their own, bound with the rest
_PROTOS_ACCEPT = {
    "whenet_jpeg_parse_scans_accept": (C.c_int, [_P, C.c_int64, C.c_int, C.POINTER(JpegInfoC), C.POINTER(JpegScanC), C.c_int, C.POINTER(C.c_int)]),
    "whenet_jpeg_decode_accept_host": (C.c_int, [_P, C.c_int64, C.POINTER(SurfaceC), C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "whenet_jpeg_decode_accept_planes_host": (C.c_int, [_P, C.c_int64, C.POINTER(_P), _P, C.c_int, C.c_int, _P]),
    "whenet_jpeg_decode_segmented_accept_host": (C.c_int, [_P, C.c_int64, C.POINTER(SurfaceC), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "whenet_jpeg_decode_segmented_accept_planes_host": (C.c_int, [_P, C.c_int64, C.POINTER(_P), _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "whenet_op_jpeg_decode_accept": (C.c_int, [_P, _P, C.c_int64, C.POINTER(SurfaceC), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P,
                                               _P, _P]),
    "whenet_op_jpeg_decode_clip_accept": (C.c_int, [_P, C.POINTER(_P), _P, C.c_int, C.POINTER(SurfaceC), C.c_int, _P, C.c_int, C.c_int, C.c_int,
                                                    C.c_int, C.c_int, _P]),
    "whenet_frame_begin_jpeg_accept": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), _P, _P]),
    "whenet_clip_begin_jpeg_accept": (C.c_int, [_P, C.POINTER(_P), _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), _P, _P]),
    "whenet_jpeg_clip_plan_accept": (C.c_int, [C.POINTER(_P), _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
}
EXPORTS_ACCEPT = tuple(_PROTOS_ACCEPT)
# the entry points of include/whenet_hip_yuv_ext.h (16-bit containers, planar 4:4:4, BT.2020): the twins of the seven YUV calls above
_PROTOS_YUVX = {
    "whenet_yuvx_to_bgr_host": (C.c_int, [C.POINTER(YuvxFrameC), _P]),
    "whenet_op_yuvx_to_bgr": (C.c_int, [_P, C.POINTER(YuvxFrameC), C.c_int, C.POINTER(_P)]),
    "whenet_frame_begin_yuvx": (C.c_int, [_P, C.POINTER(YuvxFrameC), C.POINTER(C.c_int)]),
    "whenet_clip_begin_yuvx": (C.c_int, [_P, C.POINTER(YuvxFrameC), C.c_int, C.POINTER(C.c_int)]),
    "whenet_frame_begin_yuvx_device": (C.c_int, [_P, C.POINTER(YuvxFrameC), _P, C.POINTER(C.c_int)]),
    "whenet_clip_begin_yuvx_device": (C.c_int, [_P, C.POINTER(YuvxFrameC), C.c_int, _P, C.POINTER(C.c_int)]),
    "whenet_op_yuvx_to_bgr_device": (C.c_int, [_P, C.POINTER(YuvxFrameC), C.c_int, _P, C.POINTER(_P)]),
}
EXPORTS_YUVX = tuple(_PROTOS_YUVX)

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """dlopen the library and bind every symbol the header declares (works without a GPU)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("WHENET_HIP_LIB", LIB_PATH)
    if not os.path.exists(path):
        raise OSError(f"{path} not found: build it with `python __graft_entry__.py` "
                      "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, args) in list(_PROTOS.items()) + list(_PROTOS_ACCEPT.items()) + list(_PROTOS_YUVX.items()):
        fn = getattr(lib, name)          # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


RGB, BGR = 0, 1
MAX_CLIP_FRAMES = 16      # the detector's batch limit
MAX_CLIP_SLOTS = 1024     # frames x classes x max_boxes of a clip
MAX_CLIP_HEADS = 256      # rows of a clip's forward


def clip_u8(frames) -> np.ndarray:
    """The frames of a clip as ONE contiguous uint8 [F,H,W,3] block: an array of that shape, or a list of uint8 [H,W,3] frames of
    one shape (stacked here).  ValueError for frames of different shapes or dtypes, and for F outside 1..16."""
    if isinstance(frames, np.ndarray):
        a = frames
    else:
        items = [np.asarray(f) for f in frames]
        if not 1 <= len(items) <= MAX_CLIP_FRAMES:
            raise ValueError(f"a clip holds 1..{MAX_CLIP_FRAMES} frames, got {len(items)}")
        for f in items:
            if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
                raise ValueError(f"frame must be uint8 [H,W,3], got {f.dtype} {f.shape}")
            if f.shape != items[0].shape:
                raise ValueError(f"the frames of a clip have one size: got {items[0].shape} and {f.shape}")
        a = np.stack(items)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3 or a.shape[1] < 1 or a.shape[2] < 1:
        raise ValueError(f"a clip must be uint8 [F,H,W,3], got {a.dtype} {a.shape}")
    if not 1 <= a.shape[0] <= MAX_CLIP_FRAMES:
        raise ValueError(f"a clip holds 1..{MAX_CLIP_FRAMES} frames, got {a.shape[0]}")
    return np.ascontiguousarray(a)


MAX_FRAME_SIDE = 8192     # LETTERBOX_MAX_FRAME_SIDE: a frame row is staged in LDS


def mixed_u8(frames) -> list:
    """The frames of a MIXED clip as a list of contiguous uint8 [H_i,W_i,3] arrays, each of its own size: 1..16 frames, sides
    1..8192.  ValueError otherwise (a single frame, a wrong dtype or rank, an empty or oversized frame)."""
    if isinstance(frames, np.ndarray):
        if frames.ndim != 4:
            raise ValueError(f"a mixed clip is a list of uint8 [H,W,3] frames, got an array of shape {frames.shape}")
        frames = list(frames)
    try:
        items = [np.asarray(f) for f in frames]
    except TypeError:
        raise ValueError(f"a mixed clip is a list of uint8 [H,W,3] frames, got {type(frames).__name__}") from None
    if not 1 <= len(items) <= MAX_CLIP_FRAMES:
        raise ValueError(f"a clip holds 1..{MAX_CLIP_FRAMES} frames, got {len(items)}")
    for i, f in enumerate(items):
        if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
            raise ValueError(f"frame {i} must be uint8 [H,W,3], got {f.dtype} {f.shape}")
        if not (1 <= f.shape[0] <= MAX_FRAME_SIDE and 1 <= f.shape[1] <= MAX_FRAME_SIDE):
            raise ValueError(f"frame {i} is {f.shape[0]} x {f.shape[1]}: sides must be 1..{MAX_FRAME_SIDE}")
    return [np.ascontiguousarray(f) for f in items]


def _mixed_args(frames):
    """(pointer array, heights, widths) of mixed_u8's list, as the three array arguments of the mixed entry points."""
    ptrs = (_P * len(frames))(*[f.ctypes.data for f in frames])
    return ptrs, np.array([f.shape[0] for f in frames], np.int32), np.array([f.shape[1] for f in frames], np.int32)


# ---- device arrays: anything that exposes __cuda_array_interface__ (torch-ROCm tensors, CuPy arrays); no torch import here ----
class DeviceView:
    """A strided view of uint8 device memory: `ptr` (an integer address), `shape`, byte `strides`, and `owner`, the object whose
    memory it is (kept alive with the view).  It exposes `__cuda_array_interface__` itself, so it is a device array too."""

    def __init__(self, ptr: int, shape, strides, owner=None):
        self.ptr, self.shape, self.strides, self.owner = int(ptr), tuple(int(v) for v in shape), tuple(int(v) for v in strides), owner

    @property
    def __cuda_array_interface__(self):
        return dict(shape=self.shape, typestr="|u1", data=(self.ptr, True), strides=self.strides, version=3)


def is_device_array(a) -> bool:
    return hasattr(a, "__cuda_array_interface__")


def device_view(a, what: str = "device array") -> DeviceView:
    """The `__cuda_array_interface__` of `a` as a DeviceView: uint8 only, a non-NULL pointer, non-negative strides (None: C
    order).  The read-only flag is accepted: the library only reads.  ValueError otherwise; nothing is ever copied."""
    cai = a.__cuda_array_interface__
    if not isinstance(cai, dict) or "shape" not in cai or "typestr" not in cai or "data" not in cai:
        raise ValueError(f"{what}: malformed __cuda_array_interface__")
    if cai["typestr"] not in ("|u1", "<u1", ">u1", "=u1"):
        raise ValueError(f"{what} must be uint8, got typestr {cai['typestr']!r}")
    shape = tuple(int(v) for v in cai["shape"])
    strides = cai.get("strides")
    if strides is None:
        strides, acc = [], 1
        for n in reversed(shape):
            strides.append(acc)
            acc *= n
        strides = tuple(reversed(strides))
    strides = tuple(int(v) for v in strides)
    if len(strides) != len(shape) or any(v < 0 for v in strides):
        raise ValueError(f"{what}: strides {strides} do not fit shape {shape} (negative strides are not supported)")
    ptr = cai["data"][0]
    if not ptr and all(shape):
        raise ValueError(f"{what}: NULL device pointer")
    return DeviceView(int(ptr or 0), shape, strides, a)


class DeviceFrame:
    """One packed 3-byte-pixel frame in device memory as the device entry points take it: `ptr`, byte `pitch`, `h`, `w`
    (`owner`: what keeps the memory alive)."""

    def __init__(self, ptr: int, pitch: int, h: int, w: int, owner=None):
        self.ptr, self.pitch, self.h, self.w, self.owner = int(ptr), int(pitch), int(h), int(w), owner

    def __repr__(self):
        return f"DeviceFrame(ptr=0x{self.ptr:x}, pitch={self.pitch}, h={self.h}, w={self.w})"


def _device_frame_of_view(v: DeviceView, what: str) -> DeviceFrame:
    if len(v.shape) != 3 or v.shape[2] != 3:
        raise ValueError(f"{what} must be uint8 [H,W,3], got shape {v.shape}")
    h, w = v.shape[0], v.shape[1]
    if not (1 <= h <= MAX_FRAME_SIDE and 1 <= w <= MAX_FRAME_SIDE):
        raise ValueError(f"{what} is {h} x {w}: sides must be 1..{MAX_FRAME_SIDE}")
    if v.strides[2] != 1 or (w > 1 and v.strides[1] != 3):
        raise ValueError(f"{what}: the pixels of a row must be packed (inner strides (3, 1), got {v.strides[1:]}); "
                         "a device frame is never copied: make it contiguous on the device first")
    pitch = v.strides[0] if h > 1 else 3 * w           # (a frame of one row has no row stride of its own)
    if pitch < 3 * w:
        raise ValueError(f"{what}: row stride {pitch} is below its row of {3 * w} bytes")
    return DeviceFrame(v.ptr, pitch, h, w, v.owner)


def device_frame(a, what: str = "frame") -> DeviceFrame:
    """A uint8 [H,W,3] device array -> DeviceFrame: the inner strides must be (3, 1), the row stride is the pitch (a DeviceFrame
    is returned as it is).  ValueError for anything else; nothing is copied."""
    if isinstance(a, DeviceFrame):
        return a
    return _device_frame_of_view(device_view(a, what), what)


def device_frames(frames, one_size: bool = False) -> list:
    """The frames of a clip in device memory -> a list of 1..16 DeviceFrames: a list of uint8 [H,W,3] device arrays (or
    DeviceFrames), or ONE uint8 [F,H,W,3] device array.  one_size: all frames must have one size.  A list that mixes host and
    device frames is a ValueError."""
    if is_device_array(frames):
        v = device_view(frames, "clip")
        if len(v.shape) != 4:
            raise ValueError(f"a device clip must be uint8 [F,H,W,3] or a list of uint8 [H,W,3] device arrays, got shape {v.shape}")
        items = [_device_frame_of_view(DeviceView(v.ptr + f * v.strides[0], v.shape[1:], v.strides[1:], v.owner), f"frame {f}")
                 for f in range(v.shape[0])]
    else:
        frames = list(frames)
        on_device = [isinstance(f, DeviceFrame) or is_device_array(f) for f in frames]
        if any(on_device) and not all(on_device):
            raise ValueError("a clip's frames are all in device memory or all in host memory, not mixed: frames " +
                             str([i for i, d in enumerate(on_device) if not d]) + " are host arrays")
        items = [device_frame(f, f"frame {i}") for i, f in enumerate(frames)]
    if not 1 <= len(items) <= MAX_CLIP_FRAMES:
        raise ValueError(f"a clip holds 1..{MAX_CLIP_FRAMES} frames, got {len(items)}")
    if one_size:
        for f in items:
            if (f.h, f.w) != (items[0].h, items[0].w):
                raise ValueError(f"the frames of a clip have one size: got {(items[0].h, items[0].w)} and {(f.h, f.w)}")
    return items


def any_on_device(frames) -> bool:
    """Whether a clip argument (an array or a list of frames) holds device memory anywhere."""
    if isinstance(frames, np.ndarray):
        return False
    if is_device_array(frames) or isinstance(frames, DeviceFrame):
        return True
    try:
        return any(isinstance(f, DeviceFrame) or is_device_array(f) for f in frames)
    except TypeError:
        return False


def _device_args(frames):
    """(pointer array, pitches, heights, widths) of a list of DeviceFrames, as the array arguments of the device entry points."""
    ptrs = (_P * max(len(frames), 1))(*[f.ptr for f in frames])
    return (ptrs,) + tuple(np.array([getattr(f, k) for f in frames], np.int32) for k in ("pitch", "h", "w"))


def _stream(stream):
    """A stream argument -> void*: None (the default stream) or an integer stream handle (torch: `s.cuda_stream`)."""
    if stream is None or stream == 0:
        return None
    if not isinstance(stream, int):
        raise ValueError(f"stream must be None or an integer stream handle (torch.cuda.current_stream().cuda_stream), got {type(stream).__name__}")
    return _P(stream)


def check_max_heads(max_heads) -> None:
    if max_heads is not None and not 1 <= int(max_heads) <= MAX_CLIP_HEADS:
        raise ValueError(f"max_heads must be 1..{MAX_CLIP_HEADS}, got {max_heads}")


def as_uint8_crops(img) -> np.ndarray:
    """Validate like Keras would at Model.predict (ValueError on wrong rank/shape) and return a
    contiguous uint8 array.  The reference divides by 255 whatever the dtype
    (/root/reference/whenet.py:25); integer-valued arrays in [0,255] of any dtype are therefore
    accepted here.  (Real-valued crops take WHENet.get_angle's float path instead.)"""
    a = np.asarray(img)
    if a.ndim != 4 or tuple(a.shape[1:]) != (224, 224, 3):
        raise ValueError(f"Error when checking input: expected input to have shape "
                         f"(None, 224, 224, 3) but got array with shape {a.shape}")
    if a.dtype != np.uint8:
        if a.dtype == object or not np.issubdtype(a.dtype, np.number):
            raise ValueError(f"crops must be numeric, got dtype {a.dtype}")
        if a.size and (a.min() < 0 or a.max() > 255 or not np.all(a == np.rint(a))):
            raise ValueError("not 8-bit RGB crops (integer values 0..255), as produced by cv2.resize on an "
                             "image (demo.py:11)")
        a = a.astype(np.uint8)
    return np.ascontiguousarray(a)


def _frame_u8(frame) -> np.ndarray:
    frame = np.asarray(frame)
    if frame.ndim != 3 or frame.shape[2] != 3 or frame.dtype != np.uint8:
        raise ValueError(f"frame must be uint8 [H,W,3], got {frame.dtype} {frame.shape}")
    return np.ascontiguousarray(frame)


def frame_rects(frame_h: int, frame_w: int, bboxes) -> np.ndarray:
    """demo_video.py:13-21 for k YOLO boxes (y_min, x_min, y_max, x_max) -> int32 [k,4] windows
    (y0, x0, y1, x1).  Pure host arithmetic inside the library (no GPU needed)."""
    b = np.ascontiguousarray(bboxes, np.float32).reshape(-1, 4)
    out = np.empty((b.shape[0], 4), np.int32)
    code = load().whenet_frame_rects(int(frame_h), int(frame_w), _ptr(b), b.shape[0], _ptr(out))
    raise_for(code, "whenet_frame_rects: bad arguments")
    return out


CROP_PLAN_INTS = 8 + 6 * 224      # WHENET_CROP_PLAN_INTS


def crop_plan(rect) -> np.ndarray:
    """The crop plan of one window (y0, x0, y1, x1) as the library computes it for `frame_heads`: int32 [CROP_PLAN_INTS] =
    {y0, x0, h, w, 2x-shrink flag, xmax, 0, 0} + xofs | a0 | a1 | yofs | b0 | b1 (224 each).  Pure host arithmetic inside the
    library (no GPU needed); an empty window raises ValueError."""
    r = np.ascontiguousarray(rect, np.int32).reshape(4)
    out = np.empty(CROP_PLAN_INTS, np.int32)
    raise_for(load().whenet_crop_plan(_ptr(r), _ptr(out)), f"whenet_crop_plan: empty crop window {r.tolist()}")
    return out


YUV_NV12, YUV_I420 = 0, 1                      # WHENET_YUV_NV12 / WHENET_YUV_I420
YUV_YUYV, YUV_UYVY = 3, 4                      # WHENET_YUV_YUYV / WHENET_YUV_UYVY: packed 4:2:2, one plane (2 is SURF_PACKED)
YUV_BT601, YUV_BT709, YUV_JFIF = 0, 1, 2       # WHENET_YUV_BT601 / _BT709 / _JFIF


def _yuv_descs(frames):
    """The whenet_yuv_frame_t array of a list of frames (`whenet_hip.yuv.YUVFrame`s, or YuvFrameC descriptors as they are)."""
    descs = [f if isinstance(f, YuvFrameC) else f.descriptor() for f in frames]
    for i, d in enumerate(descs):
        if not isinstance(d, YuvFrameC):
            raise ValueError(f"frame {i} needs the extended calls (a 16-bit container, 4:4:4 or BT.2020): op_yuvx_to_bgr / frame_begin_yuvx / "
                             "clip_begin_yuvx and their device twins take it")
    return (YuvFrameC * max(len(descs), 1))(*descs), descs


def yuv_to_bgr_host(desc: YuvFrameC) -> np.ndarray:
    """The YUV -> BGR conversion of include/whenet_hip.h on one frame descriptor -> uint8 [h,w,3] (B, G, R).  Pure host arithmetic
    inside the library (no GPU needed); a descriptor the library refuses raises ValueError with its text."""
    lib = load()
    out = np.empty((max(int(desc.h), 0), max(int(desc.w), 0), 3), np.uint8)
    rc = lib.whenet_yuv_to_bgr_host(C.byref(desc), _ptr(out) if out.size else None)
    if rc != OK:
        raise_for(rc, (lib.whenet_last_error(None) or b"").decode(errors="replace") if out.size else "yuv_to_bgr_host: frame 0 is empty")
    return out


# ---- include/whenet_hip_yuv_ext.h ----
YUVX_I444 = 16                                 # WHENET_YUVX_I444: the layout beside YUV_NV12 / _I420 / _YUYV / _UYVY
YUVX_U8, YUVX_U16 = 8, 16                      # WHENET_YUVX_U8 / _U16: the container, bits per stored sample
YUV_BT2020 = 3                                 # WHENET_YUV_BT2020: the fourth row of WHENET_YUVX_COEFFS


def yuvx_desc(f) -> YuvxFrameC:
    """The whenet_yuvx_frame_t of a frame: a YuvxFrameC as it is, a YuvFrameC (an old format: 8-bit container, shift 0), or a
    `whenet_hip.yuv.YUVFrame` (its `descriptor_ext()`)."""
    if isinstance(f, YuvxFrameC):
        return f
    if isinstance(f, YuvFrameC):
        d = YuvxFrameC()
        for i in range(3):
            d.plane[i], d.pitch[i] = f.plane[i], f.pitch[i]
        d.layout, d.container, d.shift, d.matrix, d.h, d.w = f.format, YUVX_U8, 0, f.matrix, f.h, f.w
        return d
    return f.descriptor_ext()


def _yuvx_descs(frames):
    descs = [yuvx_desc(f) for f in frames]
    return (YuvxFrameC * max(len(descs), 1))(*descs), descs


def yuvx_to_bgr_host(desc: YuvxFrameC) -> np.ndarray:
    """`yuv_to_bgr_host` for a whenet_yuvx_frame_t: the host statement of include/whenet_hip_yuv_ext.h, inside the library."""
    lib = load()
    out = np.empty((max(int(desc.h), 0), max(int(desc.w), 0), 3), np.uint8)
    rc = lib.whenet_yuvx_to_bgr_host(C.byref(desc), _ptr(out) if out.size else None)
    if rc != OK:
        raise_for(rc, (lib.whenet_last_error(None) or b"").decode(errors="replace") if out.size else "yuvx_to_bgr_host: frame 0 is empty")
    return out


SURF_PACKED = 2                                # WHENET_SURF_PACKED, beside YUV_NV12 / YUV_I420
MAX_OVERLAY_HEADS = 256
DISPLAY_SIMPLE, DISPLAY_FULL = 0, 1            # WHENET_DISPLAY_SIMPLE / _FULL: demo_video.py's --display
OVERLAY_GLYPHS = "0123456789achiloprtwy: -."   # WHENET_OVERLAY_GLYPHS: the characters of the labels' font


def display_code(display) -> int:
    """'simple' | 'full' -> WHENET_DISPLAY_SIMPLE | WHENET_DISPLAY_FULL; anything else is a ValueError."""
    if display == "simple":
        return DISPLAY_SIMPLE
    if display == "full":
        return DISPLAY_FULL
    raise ValueError(f"display must be 'simple' or 'full', got {display!r}")


def overlay_labels(rect, yaw: float, pitch: float, roll: float):
    """The labels of one head (include/whenet_hip.h, LABELS): window (y0, x0, y1, x1) and float32 angles in degrees ->
    (the three texts 'yaw: 10.0', 'pitch: -5.0', 'roll: 2.0', their baseline-left origins int32 [3,2] as (x, y), flags: 1 rectangle |
    2 axes | 4 labels).  Without the 4 the texts are empty.  Pure host arithmetic inside the library (no GPU needed)."""
    lib = load()
    r = np.ascontiguousarray(rect, np.int32).reshape(4)
    text = C.create_string_buffer(48)
    origin = np.zeros((3, 2), np.int32)
    flags = C.c_int32(0)
    rc = lib.whenet_overlay_labels(_ptr(r), float(np.float32(yaw)), float(np.float32(pitch)), float(np.float32(roll)), text, _ptr(origin),
                                   C.byref(flags))
    if rc != OK:
        raise_for(rc, (lib.whenet_last_error(None) or b"").decode(errors="replace"))
    raw = text.raw
    return [raw[16 * i:16 * i + 16].split(b"\0", 1)[0].decode() for i in range(3)], origin, int(flags.value)


def overlay_glyph(ch: str) -> np.ndarray:
    """The strokes of one character of the labels' font: int32 [n,4] rows of x0, y0, x1, y1 relative to the character's origin
    (y grows downward, the baseline is 0), n = 0..8.  ValueError for a character the font does not have."""
    lib = load()
    if not isinstance(ch, str) or len(ch) != 1:
        raise ValueError(f"glyph: one character, got {ch!r}")
    segs = np.zeros((8, 4), np.int32)
    n = lib.whenet_overlay_glyph(ord(ch), _ptr(segs))
    if n < 0:
        raise ValueError(f"glyph: {ch!r} is not one of {OVERLAY_GLYPHS!r}")
    return segs[:n].copy()


def overlay_segments(rect, yaw: float, pitch: float, roll: float):
    """The segments of one head (include/whenet_hip.h, POSE OVERLAY): window (y0, x0, y1, x1) and float32 angles in degrees ->
    (int32 [16] = x0, y0, x1, y1 of the rectangle, then P and Q of the X, Y and Z axis as (x, y) pairs, flags: 1 rectangle | 2 axes).
    Pure host arithmetic inside the library (no GPU needed)."""
    lib = load()
    r = np.ascontiguousarray(rect, np.int32).reshape(4)
    seg = np.empty(16, np.int32)
    flags = C.c_int32(0)
    rc = lib.whenet_overlay_segments(_ptr(r), float(np.float32(yaw)), float(np.float32(pitch)), float(np.float32(roll)), _ptr(seg), C.byref(flags))
    if rc != OK:
        raise_for(rc, (lib.whenet_last_error(None) or b"").decode(errors="replace"))
    return seg, int(flags.value)


def overlay_heads(rects, valid, ypr):
    """The head arrays of an annotate call: rects int32 [k,4], valid int32 [k] or None, ypr float32 [k,3], k = 0..256."""
    rects = np.ascontiguousarray(rects, np.int32).reshape(-1, 4)
    ypr = np.ascontiguousarray(ypr, np.float32).reshape(-1, 3)
    if valid is not None:
        valid = np.ascontiguousarray(valid, np.int32).reshape(-1)
    k = rects.shape[0]
    if ypr.shape[0] != k or (valid is not None and valid.shape[0] != k):
        raise ValueError(f"annotate: {k} windows, {ypr.shape[0]} angle rows" + ("" if valid is None else f", {valid.shape[0]} valid flags"))
    if k > MAX_OVERLAY_HEADS:
        raise ValueError(f"annotate: {k} heads, the overlay takes at most {MAX_OVERLAY_HEADS}")
    return rects, valid, ypr


def annotate_host(frame: np.ndarray, rects, valid, ypr, surface: SurfaceC, bgr: bool = True, display: int = DISPLAY_SIMPLE) -> None:
    """`whenet_annotate_host_ex`: the overlay as pure host arithmetic inside the library (no GPU needed), written into a host surface."""
    lib = load()
    frame = np.ascontiguousarray(frame, np.uint8)
    if frame.ndim != 3 or frame.shape[2] != 3:
        raise ValueError(f"frame must be uint8 [H,W,3], got {frame.shape}")
    rects, valid, ypr = overlay_heads(rects, valid, ypr)
    rc = lib.whenet_annotate_host_ex(_ptr(frame), frame.shape[0], frame.shape[1], BGR if bgr else RGB, _ptr(rects), _ptr(valid), _ptr(ypr),
                                     rects.shape[0], C.byref(surface), int(display))
    if rc != OK:
        raise_for(rc, (lib.whenet_last_error(None) or b"").decode(errors="replace"))


JPEG_HEADER_BYTES = 629           # WHENET_JPEG_HEADER_BYTES
JPEG_DEFAULT_QUALITY = 95


class CapacityError(RuntimeError):
    """WHENET_EOVERFLOW: a result that does not fit the capacity it was given; `needed` is the size it has."""

    def __init__(self, needed: int, msg: str):
        super().__init__(msg)
        self.needed = int(needed)


JPEG_SAMPLING = {"4:2:0": 0, "4:2:2": 1, "4:4:4": 2}      # WHENET_JPEG_420 / 422 / 444


def jpeg_sampling_code(sampling) -> int:
    if sampling not in JPEG_SAMPLING:
        raise ValueError(f"sampling must be '4:2:0', '4:2:2' or '4:4:4', got {sampling!r}")
    return JPEG_SAMPLING[sampling]


def jpeg_header(h: int, w: int, quality: int = JPEG_DEFAULT_QUALITY, sampling: str = "4:2:0"):
    """`whenet_jpeg_header_ex`: (the 629 header bytes SOI..SOS of an h x w stream with the standard tables, the two scaled quantiser
    tables int32 [2,64] in natural order).  Pure host arithmetic inside the library (no GPU needed)."""
    lib = load()
    out = np.empty(JPEG_HEADER_BYTES, np.uint8)
    q = np.empty((2, 64), np.int32)
    n = lib.whenet_jpeg_header_ex(int(h), int(w), int(quality), jpeg_sampling_code(sampling), _ptr(out), out.size, _ptr(q))
    if n < 0:
        raise_for(n, (lib.whenet_last_error(None) or b"").decode(errors="replace"))
    return out[:n].tobytes(), q


def jpeg_bound(h: int, w: int, sampling: str = "4:2:0") -> int:
    """`whenet_jpeg_bound_ex`: a capacity no stream of an h x w frame exceeds."""
    lib = load()
    n = int(lib.whenet_jpeg_bound_ex(int(h), int(w), jpeg_sampling_code(sampling)))
    if n < 0:
        raise_for(n, (lib.whenet_last_error(None) or b"").decode(errors="replace"))
    return n


def jpeg_optimal_table(freq):
    """`whenet_jpeg_optimal_table`: the frequencies uint32 [256] of a table's symbols -> (bits uint8 [16], the number of codes of each
    length 1..16; vals uint8 [count], the symbols in code order).  Pure host arithmetic inside the library."""
    lib = load()
    freq = np.ascontiguousarray(freq, np.uint32)
    if freq.shape != (256,):
        raise ValueError(f"freq must be uint32 [256], got {freq.shape}")
    bits, vals, count = np.zeros(16, np.uint8), np.zeros(256, np.uint8), C.c_int(0)
    rc = lib.whenet_jpeg_optimal_table(_ptr(freq), _ptr(bits), _ptr(vals), C.byref(count))
    if rc != OK:
        raise_for(rc, (lib.whenet_last_error(None) or b"").decode(errors="replace"))
    return bits, vals[:count.value].copy()


def jpeg_encode_host(surface: SurfaceC, h: int, w: int, bgr: bool, quality: int, out: np.ndarray, sampling: str = "4:2:0",
                     optimize: bool = False, hist=None):
    """`whenet_jpeg_encode_host_ex` into the uint8 array `out` (its size is the capacity): (return code, the stream's full length).
    The code is OK or EOVERFLOW; anything else raises.  `hist`: None or a uint32 [4,256] array for the histograms of optimize=True."""
    lib = load()
    size = C.c_int64(0)
    rc = lib.whenet_jpeg_encode_host_ex(C.byref(surface), int(h), int(w), BGR if bgr else RGB, int(quality), jpeg_sampling_code(sampling),
                                        int(bool(optimize)), _ptr(out) if out.size else None, int(out.size), C.byref(size),
                                        None if hist is None else _ptr(_hist_array(hist)))
    if rc not in (OK, EOVERFLOW):
        raise_for(rc, (lib.whenet_last_error(None) or b"").decode(errors="replace"))
    return rc, int(size.value)


def _hist_array(hist) -> np.ndarray:
    if not isinstance(hist, np.ndarray) or hist.dtype != np.uint32 or hist.shape != (4, 256) or not hist.flags.c_contiguous:
        raise ValueError("hist must be a C-contiguous uint32 [4,256] array")
    return hist


def _stream_array(data) -> np.ndarray:
    """The bytes of a JPEG stream as a contiguous uint8 array (bytes, bytearray, memoryview or a uint8 array; never reinterpreted)."""
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8 or data.ndim != 1:
            raise ValueError(f"a JPEG stream must be bytes or a 1-D uint8 array, got {data.dtype} {data.shape}")
        return np.ascontiguousarray(data)
    return np.frombuffer(bytes(data), np.uint8)


def jpeg_parse(data) -> JpegInfoC:
    """`whenet_jpeg_parse`: the header SOI..SOS of a stream.  ValueError with the reason for anything but a baseline stream the
    decoder accepts.  Pure host arithmetic inside the library (no GPU needed)."""
    lib = load()
    a = _stream_array(data)
    info = JpegInfoC()
    rc = lib.whenet_jpeg_parse(_ptr(a) if a.size else None, int(a.size), C.byref(info))
    if rc != OK:
        raise_for(rc, (lib.whenet_last_error(None) or b"").decode(errors="replace"))
    return info


def _host_rc(lib, rc):
    if rc != OK:
        raise_for(rc, (lib.whenet_last_error(None) or b"").decode(errors="replace"))


def jpeg_parse_scans(data):
    """`whenet_jpeg_parse_scans`: (the header, the list of `JpegScanC` records) of a baseline OR progressive stream.  ValueError with
    the reason for a stream neither decoder accepts.  Pure host arithmetic inside the library."""
    lib = load()
    a = _stream_array(data)
    info, scans, n = JpegInfoC(), (JpegScanC * JPEG_PROG_MAX_SCANS)(), C.c_int(0)
    _host_rc(lib, lib.whenet_jpeg_parse_scans(_ptr(a) if a.size else None, int(a.size), C.byref(info), scans, JPEG_PROG_MAX_SCANS, C.byref(n)))
    return info, [scans[i] for i in range(n.value)]


def jpeg_decode_progressive_host(data, surface: SurfaceC, bgr: bool, rule: str = "own") -> np.ndarray:
    """`whenet_jpeg_decode_progressive_host` into a host surface: the two status words (OK or EFORMAT, the first bad item or -1)."""
    lib = load()
    a = _stream_array(data)
    status = np.zeros(2, np.int32)
    _host_rc(lib, lib.whenet_jpeg_decode_progressive_host(_ptr(a) if a.size else None, int(a.size), C.byref(surface), BGR if bgr else RGB,
                                                          jpeg_rule_code(rule), _ptr(status)))
    return status


def jpeg_decode_progressive_planes_host(data, planes, rule: str = "own") -> np.ndarray:
    """`whenet_jpeg_decode_progressive_planes_host` into uint8 2-D arrays (contiguous rows): the two status words."""
    lib = load()
    a = _stream_array(data)
    status = np.zeros(2, np.int32)
    ptrs = (_P * 3)(*[p.ctypes.data for p in planes])
    pitch = np.array([p.strides[0] for p in planes] + [0] * (3 - len(planes)), np.int32)
    _host_rc(lib, lib.whenet_jpeg_decode_progressive_planes_host(_ptr(a) if a.size else None, int(a.size), ptrs, _ptr(pitch),
                                                                 jpeg_rule_code(rule), _ptr(status)))
    return status


def jpeg_progressive_coefficients_host(data, blocks: int):
    """`whenet_jpeg_progressive_coefficients_host`: (finished records int16 [blocks,64] in natural order, raw records int16 [blocks,64]
    in zigzag order, the counters as a dict, the two status words) of a SOF2 stream of `blocks` blocks."""
    lib = load()
    a = _stream_array(data)
    coef, raw = np.zeros((blocks, 64), np.int16), np.zeros((blocks, 64), np.int16)
    cnt, status = np.zeros(8, np.int64), np.zeros(2, np.int32)
    _host_rc(lib, lib.whenet_jpeg_progressive_coefficients_host(_ptr(a) if a.size else None, int(a.size), _ptr(coef), _ptr(raw), int(blocks),
                                                                _ptr(cnt), _ptr(status)))
    return coef, raw, {k: int(cnt[i]) for i, k in enumerate(JPEG_PROG_COUNTERS)}, status


def jpeg_decode_host(data, surface: SurfaceC, bgr: bool) -> np.ndarray:
    """`whenet_jpeg_decode_host` into a host surface: the two status words int32 [2] (OK or EFORMAT, the first bad interval or -1)."""
    lib = load()
    a = _stream_array(data)
    status = np.zeros(2, np.int32)
    rc = lib.whenet_jpeg_decode_host(_ptr(a) if a.size else None, int(a.size), C.byref(surface), BGR if bgr else RGB, _ptr(status))
    if rc != OK:
        raise_for(rc, (lib.whenet_last_error(None) or b"").decode(errors="replace"))
    return status


def jpeg_decode_planes_host(data, planes: list) -> np.ndarray:
    """`whenet_jpeg_decode_planes_host` into the uint8 [rows, width] arrays `planes` (one per component, rows contiguous): the two
    status words."""
    lib = load()
    a = _stream_array(data)
    status = np.zeros(2, np.int32)
    ptrs = (_P * 3)(*[p.ctypes.data for p in planes] + [None] * (3 - len(planes)))
    pitch = np.array([int(p.strides[0]) if p.shape[0] > 1 else int(p.shape[1]) for p in planes] + [0] * (3 - len(planes)), np.int32)
    rc = lib.whenet_jpeg_decode_planes_host(_ptr(a) if a.size else None, int(a.size), ptrs, _ptr(pitch), _ptr(status))
    if rc != OK:
        raise_for(rc, (lib.whenet_last_error(None) or b"").decode(errors="replace"))
    return status


JPEG_SEG_WINDOW = 256          # WHENET_JPEG_SEG_WINDOW: the segments of one sync window (one workgroup)
JPEG_SEG_AUTO_BYTES = 4096     # option jpeg_entropy = 2 takes the segmented form from this many bytes per restart interval on
JPEG_ENTROPY = {"interval": 0, "segmented": 1, "auto": 2}


def jpeg_decode_segmented_host(data, surface: SurfaceC, bgr: bool, seg_bytes: int, window: int):
    """`whenet_jpeg_decode_segmented_host` into a host surface: (the two status words int32 [2], the statistics int64 [8])."""
    lib = load()
    a = _stream_array(data)
    status, stats = np.zeros(2, np.int32), np.zeros(8, np.int64)
    rc = lib.whenet_jpeg_decode_segmented_host(_ptr(a) if a.size else None, int(a.size), C.byref(surface), BGR if bgr else RGB, int(seg_bytes),
                                               int(window), _ptr(status), _ptr(stats))
    if rc != OK:
        raise_for(rc, (lib.whenet_last_error(None) or b"").decode(errors="replace"))
    return status, stats


def jpeg_decode_segmented_planes_host(data, planes: list, seg_bytes: int, window: int):
    """`whenet_jpeg_decode_segmented_planes_host` into the uint8 [rows, width] arrays `planes`: (status int32 [2], statistics int64 [8])."""
    lib = load()
    a = _stream_array(data)
    status, stats = np.zeros(2, np.int32), np.zeros(8, np.int64)
    ptrs = (_P * 3)(*[p.ctypes.data for p in planes] + [None] * (3 - len(planes)))
    pitch = np.array([int(p.strides[0]) if p.shape[0] > 1 else int(p.shape[1]) for p in planes] + [0] * (3 - len(planes)), np.int32)
    rc = lib.whenet_jpeg_decode_segmented_planes_host(_ptr(a) if a.size else None, int(a.size), ptrs, _ptr(pitch), int(seg_bytes), int(window),
                                                      _ptr(status), _ptr(stats))
    if rc != OK:
        raise_for(rc, (lib.whenet_last_error(None) or b"").decode(errors="replace"))
    return status, stats


JPEG_RULE = {"own": 0, "libjpeg": 1}      # the decode rule: the project's own (default), or libjpeg's bytes (option "jpeg_rule")


def jpeg_rule_code(rule) -> int:
    """"own" -> 0, "libjpeg" -> 1, None -> -1 (the handle's option "jpeg_rule")."""
    if rule is None:
        return -1
    if rule not in JPEG_RULE:
        raise ValueError("rule must be 'own' or 'libjpeg'")
    return JPEG_RULE[rule]


def jpeg_decode_rule_host(data, surface: SurfaceC, bgr: bool, rule: str = "own") -> np.ndarray:
    """`whenet_jpeg_decode_rule_host` into a packed host surface: `jpeg_decode_host` by the rule "own" or "libjpeg"; the two status
    words."""
    lib = load()
    a = _stream_array(data)
    status = np.zeros(2, np.int32)
    rc = lib.whenet_jpeg_decode_rule_host(_ptr(a) if a.size else None, int(a.size), C.byref(surface), BGR if bgr else RGB,
                                          jpeg_rule_code(rule), _ptr(status))
    if rc != OK:
        raise_for(rc, (lib.whenet_last_error(None) or b"").decode(errors="replace"))
    return status


def jpeg_orientation(data) -> int:
    """`whenet_jpeg_orientation`: the EXIF orientation (tag 0x0112 in IFD0 of the first Exif APP1) of a stream, 1..8; 1 for a stream
    without one and for any broken EXIF structure.  Pure host arithmetic inside the library."""
    lib = load()
    a = _stream_array(data)
    return int(lib.whenet_jpeg_orientation(_ptr(a) if a.size else None, int(a.size)))


JPEG_DEFAULT_TABLES_MAX = 420      # bytes `whenet_jpeg_add_default_tables` adds at most (one DHT segment of the four Annex K tables)


def jpeg_add_default_tables(data) -> bytes:
    """`whenet_jpeg_add_default_tables`: the stream with the Annex K Huffman tables (what libjpeg installs) for every slot DC 0, AC 0,
    DC 1, AC 1 that no DHT before the first SOS defines, in one DHT segment directly in front of that SOS.  A complete stream and a
    header that cannot be followed come back byte for byte.  Pure host arithmetic inside the library."""
    lib = load()
    a = _stream_array(data)
    out = np.empty(int(a.size) + JPEG_DEFAULT_TABLES_MAX, np.uint8)
    n = C.c_int64(0)
    rc = lib.whenet_jpeg_add_default_tables(_ptr(a) if a.size else _ptr(out), int(a.size), _ptr(out), int(out.size), C.byref(n))
    if rc != 0:
        raise_for(rc, (lib.whenet_last_error(None) or b"").decode(errors="replace"))
    return out[:n.value].tobytes()


def jpeg_tristate(v) -> int:
    """None -> -1 (the handle's option), else 0 / 1."""
    return -1 if v is None else int(bool(v))


def jpeg_decode_oriented_host(data, surface: SurfaceC, bgr: bool, rule: str = "own", progressive: bool = False) -> np.ndarray:
    """`whenet_jpeg_decode_oriented_host` into a packed host surface of the ORIENTED size: the two status words."""
    lib = load()
    a = _stream_array(data)
    status = np.zeros(2, np.int32)
    _host_rc(lib, lib.whenet_jpeg_decode_oriented_host(_ptr(a) if a.size else None, int(a.size), C.byref(surface), BGR if bgr else RGB,
                                                       jpeg_rule_code(rule), int(bool(progressive)), _ptr(status)))
    return status


def jpeg_decode_segmented_rule_host(data, surface: SurfaceC, bgr: bool, seg_bytes: int, window: int, rule: str = "own"):
    """`whenet_jpeg_decode_segmented_rule_host`: `jpeg_decode_segmented_host` by the rule "own" or "libjpeg": (status, statistics)."""
    lib = load()
    a = _stream_array(data)
    status, stats = np.zeros(2, np.int32), np.zeros(8, np.int64)
    rc = lib.whenet_jpeg_decode_segmented_rule_host(_ptr(a) if a.size else None, int(a.size), C.byref(surface), BGR if bgr else RGB,
                                                    int(seg_bytes), int(window), jpeg_rule_code(rule),
                                                    _ptr(status), _ptr(stats))
    if rc != OK:
        raise_for(rc, (lib.whenet_last_error(None) or b"").decode(errors="replace"))
    return status, stats


# ---- the accept bits (include/whenet_hip.h, JPEG DECODER, LAYOUTS): the calls named ..._accept ----
JPEG_ACCEPT_PROGRESSIVE, JPEG_ACCEPT_LAYOUTS = 1, 2


def jpeg_accept_bits(progressive=False, layouts=False) -> int:
    """The `accept` argument of the ..._accept calls from the two flags."""
    return (JPEG_ACCEPT_PROGRESSIVE if progressive else 0) | (JPEG_ACCEPT_LAYOUTS if layouts else 0)


def jpeg_parse_scans_accept(data, accept: int):
    """`whenet_jpeg_parse_scans_accept`: `jpeg_parse_scans` with the accept bits (without the PROGRESSIVE bit a SOF2 stream is refused)."""
    lib = load()
    a = _stream_array(data)
    info, scans, n = JpegInfoC(), (JpegScanC * JPEG_PROG_MAX_SCANS)(), C.c_int(0)
    _host_rc(lib, lib.whenet_jpeg_parse_scans_accept(_ptr(a) if a.size else None, int(a.size), int(accept), C.byref(info), scans,
                                                     JPEG_PROG_MAX_SCANS, C.byref(n)))
    return info, [scans[i] for i in range(n.value)]


def jpeg_decode_accept_host(data, surface: SurfaceC, bgr: bool, rule: str = "own", accept: int = 0, orient: bool = False):
    """`whenet_jpeg_decode_accept_host` into a packed host surface (of the ORIENTED size where orient): (the two status words, the
    orientation applied)."""
    lib = load()
    a = _stream_array(data)
    status, applied = np.zeros(2, np.int32), np.ones(1, np.int32)
    _host_rc(lib, lib.whenet_jpeg_decode_accept_host(_ptr(a) if a.size else None, int(a.size), C.byref(surface), BGR if bgr else RGB,
                                                     jpeg_rule_code(rule), int(accept), int(bool(orient)), _ptr(status), _ptr(applied)))
    return status, int(applied[0])


def _plane_args(planes):
    ptrs = (_P * 3)(*[p.ctypes.data for p in planes] + [None] * (3 - len(planes)))
    pitch = np.array([int(p.strides[0]) if p.shape[0] > 1 else int(p.shape[1]) for p in planes] + [0] * (3 - len(planes)), np.int32)
    return ptrs, pitch


def jpeg_decode_accept_planes_host(data, planes, rule: str = "own", accept: int = 0) -> np.ndarray:
    """`whenet_jpeg_decode_accept_planes_host` into uint8 2-D arrays (contiguous rows): the two status words."""
    lib = load()
    a = _stream_array(data)
    status = np.zeros(2, np.int32)
    ptrs, pitch = _plane_args(planes)
    _host_rc(lib, lib.whenet_jpeg_decode_accept_planes_host(_ptr(a) if a.size else None, int(a.size), ptrs, _ptr(pitch), jpeg_rule_code(rule),
                                                            int(accept), _ptr(status)))
    return status


def jpeg_decode_segmented_accept_host(data, surface: SurfaceC, bgr: bool, seg_bytes: int, window: int, rule: str = "own", accept: int = 0):
    """`whenet_jpeg_decode_segmented_accept_host`: (status, statistics)."""
    lib = load()
    a = _stream_array(data)
    status, stats = np.zeros(2, np.int32), np.zeros(8, np.int64)
    _host_rc(lib, lib.whenet_jpeg_decode_segmented_accept_host(_ptr(a) if a.size else None, int(a.size), C.byref(surface), BGR if bgr else RGB,
                                                               int(seg_bytes), int(window), jpeg_rule_code(rule), int(accept), _ptr(status),
                                                               _ptr(stats)))
    return status, stats


def jpeg_decode_segmented_accept_planes_host(data, planes, seg_bytes: int, window: int, rule: str = "own", accept: int = 0):
    """`whenet_jpeg_decode_segmented_accept_planes_host`: (status, statistics)."""
    lib = load()
    a = _stream_array(data)
    status, stats = np.zeros(2, np.int32), np.zeros(8, np.int64)
    ptrs, pitch = _plane_args(planes)
    _host_rc(lib, lib.whenet_jpeg_decode_segmented_accept_planes_host(_ptr(a) if a.size else None, int(a.size), ptrs, _ptr(pitch),
                                                                      int(seg_bytes), int(window), jpeg_rule_code(rule), int(accept),
                                                                      _ptr(status), _ptr(stats)))
    return status, stats


JPEG_CLIP_PLAN_FRAME_WORDS, JPEG_CLIP_PLAN_TOTAL_WORDS = 32, 8
JPEG_CLIP_REGIONS = ("tables", "data", "start", "meta", "seg_stats", "coef", "plane0", "plane1", "plane2", "first_seg", "seg_exit",
                     "seg_count", "seg_blk")


def jpeg_clip_plan(infos, nbytes, entropy: int = 2, seg_bytes: int = 128) -> dict:
    """`whenet_jpeg_clip_plan` (pure host): the layout a clip of JPEG streams gets.  infos: `JpegInfoC` per frame, nbytes: the length
    of each frame's entropy data; entropy 0, 1 or 2 (auto).  {"frames": [{"form", "seg_bytes", "seg_cap", region: (offset, length)
    for region in JPEG_CLIP_REGIONS}], "records": (offset, length), "upload_bytes", "zero": (offset, length), "bytes", "forms":
    (frames of form 0, of form 1)}."""
    n = len(infos)
    arr = (JpegInfoC * max(n, 1))(*infos)
    nb = np.ascontiguousarray(nbytes, np.int64)
    if nb.size != n:
        raise ValueError("one nbytes per info is needed")
    out = np.zeros(max(n, 0) * JPEG_CLIP_PLAN_FRAME_WORDS + JPEG_CLIP_PLAN_TOTAL_WORDS, np.int64)
    lib = load()
    rc = lib.whenet_jpeg_clip_plan(arr, _ptr(nb if nb.size else np.zeros(1, np.int64)), n, int(entropy), int(seg_bytes), _ptr(out))
    if rc != OK:
        raise ValueError(lib.whenet_last_error(None).decode())
    frames = []
    for f in range(n):
        o = out[f * JPEG_CLIP_PLAN_FRAME_WORDS:(f + 1) * JPEG_CLIP_PLAN_FRAME_WORDS]
        d = {"form": int(o[0]), "seg_bytes": int(o[1]), "seg_cap": int(o[2])}
        for k, name in enumerate(JPEG_CLIP_REGIONS):
            d[name] = (int(o[4 + 2 * k]), int(o[5 + 2 * k]))
        frames.append(d)
    t = out[n * JPEG_CLIP_PLAN_FRAME_WORDS:]
    return {"frames": frames, "records": (int(t[0]), int(t[1])), "upload_bytes": int(t[2]), "zero": (int(t[3]), int(t[4])),
            "bytes": int(t[5]), "forms": (int(t[6]), int(t[7]))}


def _clip_streams(datas):
    """The streams of a clip as (arrays kept alive, void* [F], int64 [F])."""
    arrs = [_stream_array(d) for d in datas]
    ptrs = (_P * max(len(arrs), 1))(*[_ptr(a) if a.size else None for a in arrs])
    sizes = np.array([a.size for a in arrs], np.int64)
    return arrs, ptrs, sizes


JPEG_CLIP_PROG_PLAN_FRAME_WORDS, JPEG_CLIP_PROG_PLAN_TOTAL_WORDS = 48, 16
JPEG_CLIP_FORM_PROGRESSIVE = 2
JPEG_CLIP_PROG_REGIONS = ("scans", "huff", "qz", "items", "raw")


def jpeg_clip_plan_progressive(datas, entropy: int = 2, seg_bytes: int = 128) -> dict:
    """`whenet_jpeg_clip_plan_progressive` (pure host): the layout a clip gets that may hold progressive streams, from the streams
    themselves.  The dict of `jpeg_clip_plan`; a frame of form 2 is progressive, and every frame also has (offset, length) for the
    regions of JPEG_CLIP_PROG_REGIONS (empty for a baseline frame) and the counts "nscans", "levels" and "list" (the entries of its
    item list); the totals add "progressive" (frames), "scan_launches", "record_stride" and "prog_record_offset".  ValueError that
    names the frame for a stream the scan parser refuses."""
    return _clip_plan_progressive(datas, entropy, seg_bytes, None)


def jpeg_clip_plan_accept(datas, entropy: int = 2, seg_bytes: int = 128, accept: int = 0) -> dict:
    """`whenet_jpeg_clip_plan_accept` (pure host): `jpeg_clip_plan_progressive` with the accept bits."""
    return _clip_plan_progressive(datas, entropy, seg_bytes, int(accept))


def _clip_plan_progressive(datas, entropy, seg_bytes, accept):
    arrs, ptrs, sizes = _clip_streams(datas)
    n = len(arrs)
    out = np.zeros(max(n, 0) * JPEG_CLIP_PROG_PLAN_FRAME_WORDS + JPEG_CLIP_PROG_PLAN_TOTAL_WORDS, np.int64)
    lib = load()
    if accept is None:
        rc = lib.whenet_jpeg_clip_plan_progressive(ptrs, _ptr(sizes) if sizes.size else None, n, int(entropy), int(seg_bytes), _ptr(out))
    else:
        rc = lib.whenet_jpeg_clip_plan_accept(ptrs, _ptr(sizes) if sizes.size else None, n, int(entropy), int(seg_bytes), accept, _ptr(out))
    if rc != OK:
        raise ValueError(lib.whenet_last_error(None).decode())
    frames = []
    for f in range(n):
        o = out[f * JPEG_CLIP_PROG_PLAN_FRAME_WORDS:(f + 1) * JPEG_CLIP_PROG_PLAN_FRAME_WORDS]
        d = {"form": int(o[0]), "seg_bytes": int(o[1]), "seg_cap": int(o[2])}
        for k, name in enumerate(JPEG_CLIP_REGIONS + JPEG_CLIP_PROG_REGIONS):
            at = 4 + 2 * k if k < len(JPEG_CLIP_REGIONS) else 6 + 2 * k
            d[name] = (int(o[at]), int(o[at + 1]))
        d["nscans"], d["levels"], d["list"] = int(o[42]), int(o[43]), int(o[44])
        frames.append(d)
    t = out[n * JPEG_CLIP_PROG_PLAN_FRAME_WORDS:]
    return {"frames": frames, "records": (int(t[0]), int(t[1])), "upload_bytes": int(t[2]), "zero": (int(t[3]), int(t[4])),
            "bytes": int(t[5]), "forms": (int(t[6]), int(t[7])), "progressive": int(t[8]), "scan_launches": int(t[9]),
            "record_stride": int(t[10]), "prog_record_offset": int(t[11])}


def jpeg_seg_dc_scan_host(diff, chunk: int) -> np.ndarray:
    """`whenet_jpeg_seg_dc_scan_host`: the DC predictor behind every difference of int32 [n] `diff` (from 0, kept inside
    -32768..32767 after every step), computed as the segmented decoder does: saturating maps composed over chunks of `chunk`."""
    d = np.ascontiguousarray(diff, np.int32)
    out = np.zeros(d.size, np.int32)
    rc = load().whenet_jpeg_seg_dc_scan_host(_ptr(d) if d.size else None, int(d.size), int(chunk), _ptr(out) if d.size else None)
    if rc != OK:
        raise_for(rc, (load().whenet_last_error(None) or b"").decode(errors="replace"))
    return out


def normalise_lut() -> np.ndarray:
    """[3,256] float32: whenet.py:23-26 + Keras' float32 cast for every byte value, as the stem kernels apply it.
    Pure host arithmetic inside the library (no GPU needed)."""
    out = np.empty((3, 256), np.float32)
    raise_for(load().whenet_normalise_table(_ptr(out)), "whenet_normalise_table: bad arguments")
    return out


def letterbox_plan(frame_h: int, frame_w: int, out_h: int, out_w: int):
    """The letterbox geometry and resample tables as the kernels use them (yolo_v3/utils.py:25-33 + Pillow's
    precompute_coeffs / normalize_coeffs_8bpc): ((nw, nh, x0, y0), [(ksize, bounds int32 [n,2], coeffs int32 [n,ksize]) for the
    horizontal and the vertical axis]).  Pure host arithmetic inside the library (no GPU needed)."""
    lib = load()
    geom = (C.c_int32 * 4)()
    axes = []
    for axis in (0, 1):
        ks = C.c_int(0)
        args = (int(frame_h), int(frame_w), int(out_h), int(out_w), C.byref(geom), axis)
        raise_for(lib.whenet_letterbox_plan(*args, None, None, 0, C.byref(ks)),
                  f"whenet_letterbox_plan({frame_h}x{frame_w} -> {out_h}x{out_w}): frame sides 1..8192, output sides 1..4096, "
                  "and the resized image needs at least one pixel per side")
        n = geom[0] if axis == 0 else geom[1]
        bounds = np.empty((n, 2), np.int32)
        coeffs = np.empty((n, ks.value), np.int32)
        raise_for(lib.whenet_letterbox_plan(*args, _ptr(bounds), _ptr(coeffs), coeffs.size, C.byref(ks)),
                  "whenet_letterbox_plan: bad arguments")
        axes.append((ks.value, bounds, coeffs))
    return tuple(geom), axes


class WhenetError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libwhenet_hip error {code}: {msg}")
        self.code = code


def raise_for(code: int, msg: str):
    """Map ABI codes onto what the reference's Keras path raises:
    missing/unreadable snapshot -> OSError; bad shape/argument/format -> ValueError."""
    if code == OK:
        return
    if code in (ENOENT, EIO):
        raise OSError(msg)
    if code in (EINVAL, EFORMAT):
        raise ValueError(msg)
    if code == ENOMEM:
        raise MemoryError(msg)
    raise WhenetError(code, msg)


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(_P)


DETECTOR_DTYPES = {"f16": 0, "f32": 1}        # option "detector_dtype" (include/whenet_hip.h)


class Handle:
    """Owns one whenet_t*."""
    _detector_dtype = 0                        # what option "detector_dtype" was last set to on this handle

    def __init__(self, snapshot, device: int = 0, dtype: int = F32):
        lib = load()
        h = _P()
        if isinstance(snapshot, (bytes, bytearray, memoryview)):
            buf = (C.c_char * len(snapshot)).from_buffer_copy(bytes(snapshot))
            rc = lib.whenet_create_from_memory(C.cast(buf, _P), len(snapshot), device, dtype, C.byref(h))
        else:
            rc = lib.whenet_create(os.fsencode(snapshot), device, dtype, C.byref(h))
        if rc != OK:
            raise_for(rc, (lib.whenet_last_error(None) or b"").decode(errors="replace"))
        self._h = h
        self._lib = lib
        self.dtype = dtype
        self.device = device

    @classmethod
    def postproc(cls, device: int = 0) -> "Handle":
        """A handle WITHOUT a network (whenet_create_postproc): device, stream and scratch for the frame / detector
        stages (yolo_eval, op_crop_resize); forwards raise."""
        lib = load()
        h = _P()
        rc = lib.whenet_create_postproc(device, C.byref(h))
        if rc != OK:
            raise_for(rc, (lib.whenet_last_error(None) or b"").decode(errors="replace"))
        self = cls.__new__(cls)
        self._h = h
        self._lib = lib
        self.dtype = F32
        self.device = device
        return self

    def _check(self, rc: int):
        if rc != OK:
            raise_for(rc, (self._lib.whenet_last_error(self._h) or b"").decode(errors="replace"))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.whenet_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- hot path ---------------------------------------------------------------------
    def forward(self, crops: np.ndarray, want_logits: bool = True):
        # the C side reads n*150,528 bytes from this pointer: never hand it anything else
        if not (isinstance(crops, np.ndarray) and crops.dtype == np.uint8 and crops.ndim == 4
                and crops.shape[1:] == (224, 224, 3) and crops.flags.c_contiguous):
            raise ValueError("Handle.forward needs a C-contiguous uint8 array [n,224,224,3] "
                             f"(got {getattr(crops, 'dtype', type(crops))} {getattr(crops, 'shape', '')}); "
                             "use whenet_hip._lib.as_uint8_crops()")
        n = crops.shape[0]
        if n == 0:
            return (np.empty((0, 3), np.float32), np.empty((0, 3), np.int32),
                    np.empty((0, 252), np.float32) if want_logits else None)
        ypr = np.empty((n, 3), np.float32)
        am = np.empty((n, 3), np.int32)
        lg = np.empty((n, 252), np.float32) if want_logits else None
        self._check(self._lib.whenet_forward_u8(self._h, _ptr(crops), n, _ptr(ypr), _ptr(am), _ptr(lg)))
        return ypr, am, lg

    def forward_f32(self, x: np.ndarray, want_logits: bool = True):
        """x: the NORMALISED float32 image [n,224,224,3] (what whenet.py:27 feeds Model.predict)."""
        if not (isinstance(x, np.ndarray) and x.dtype == np.float32 and x.ndim == 4
                and x.shape[1:] == (224, 224, 3) and x.flags.c_contiguous and x.shape[0] >= 1):
            raise ValueError("Handle.forward_f32 needs a C-contiguous float32 array [n>=1,224,224,3]")
        n = x.shape[0]
        ypr = np.empty((n, 3), np.float32)
        am = np.empty((n, 3), np.int32)
        lg = np.empty((n, 252), np.float32) if want_logits else None
        self._check(self._lib.whenet_forward_f32(self._h, _ptr(x), n, _ptr(ypr), _ptr(am), _ptr(lg)))
        return ypr, am, lg

    def forward_device(self, d_crops: int, n: int, d_ypr: int, d_argmax: int = 0, d_logits: int = 0, stream: int = 0):
        self._check(self._lib.whenet_forward_u8_device(self._h, d_crops, n, d_ypr, d_argmax or None,
                                                       d_logits or None, stream or None))

    def sync(self):
        self._check(self._lib.whenet_sync(self._h))

    def submit(self, crops: np.ndarray) -> int:
        if not (isinstance(crops, np.ndarray) and crops.dtype == np.uint8 and crops.ndim == 4
                and crops.shape[1:] == (224, 224, 3) and crops.flags.c_contiguous and crops.shape[0] >= 1):
            raise ValueError("Handle.submit needs a C-contiguous uint8 array [n>=1,224,224,3]")
        t = C.c_int(-1)
        self._check(self._lib.whenet_submit_u8(self._h, _ptr(crops), crops.shape[0], C.byref(t)))
        return t.value

    def submit_frame(self, frame: np.ndarray, rects: np.ndarray, bgr: bool = True) -> int:
        """frame uint8 [H,W,3]; rects int32 [k,4] (y0,x0,y1,x1) -> ticket (collect with n=k)."""
        frame = _frame_u8(frame)
        rects = np.ascontiguousarray(rects, np.int32).reshape(-1, 4)
        t = C.c_int(-1)
        self._check(self._lib.whenet_submit_frame(self._h, _ptr(frame), frame.shape[0], frame.shape[1],
                                                  BGR if bgr else RGB, _ptr(rects), rects.shape[0], C.byref(t)))
        return t.value

    def op_crop_resize(self, frame: np.ndarray, rects: np.ndarray, bgr: bool = True) -> np.ndarray:
        frame = _frame_u8(frame)
        rects = np.ascontiguousarray(rects, np.int32).reshape(-1, 4)
        out = np.empty((rects.shape[0], 224, 224, 3), np.uint8)
        self._check(self._lib.whenet_op_crop_resize(self._h, _ptr(frame), frame.shape[0], frame.shape[1],
                                                    BGR if bgr else RGB, _ptr(rects), rects.shape[0], _ptr(out)))
        return out

    @staticmethod
    def _letterbox_outputs(size, want_u8: bool, want_f32: bool):
        oh, ow = int(size[0]), int(size[1])
        if oh < 1 or ow < 1:
            raise ValueError(f"letterbox: size must be (h, w) >= 1, got {size}")
        u8 = np.empty((oh, ow, 3), np.uint8) if want_u8 else None
        f32 = np.empty((oh, ow, 3), np.float32) if want_f32 else None
        return oh, ow, u8, f32

    def op_letterbox(self, frame: np.ndarray, size=(416, 416), bgr: bool = True, want_u8: bool = True, want_f32: bool = True):
        """yolo_v3/utils.py:23-34 + yolo_postprocess.py:191-195 on the device: frame uint8 [H,W,3] -> (canvas uint8 [h,w,3],
        image float32 [h,w,3] = canvas / 255); `size` = (h, w) as the reference's model_image_size.  An output not wanted is None."""
        frame = _frame_u8(frame)
        oh, ow, u8, f32 = self._letterbox_outputs(size, want_u8, want_f32)
        self._check(self._lib.whenet_op_letterbox(self._h, _ptr(frame), frame.shape[0], frame.shape[1], BGR if bgr else RGB,
                                                  oh, ow, _ptr(u8), _ptr(f32)))
        return u8, f32

    def frame_begin(self, frame: np.ndarray, bgr: bool = True) -> int:
        """Upload the frame once; the ticket is carried through frame_letterbox / frame_heads to collect."""
        frame = _frame_u8(frame)
        t = C.c_int(-1)
        self._check(self._lib.whenet_frame_begin(self._h, _ptr(frame), frame.shape[0], frame.shape[1], BGR if bgr else RGB,
                                                 C.byref(t)))
        return t.value

    def frame_letterbox(self, ticket: int, size=(416, 416), want_u8: bool = True, want_f32: bool = True):
        oh, ow, u8, f32 = self._letterbox_outputs(size, want_u8, want_f32)
        self._check(self._lib.whenet_frame_letterbox(self._h, int(ticket), oh, ow, _ptr(u8), _ptr(f32)))
        return u8, f32

    def frame_heads(self, ticket: int, rects: np.ndarray) -> None:
        rects = np.ascontiguousarray(rects, np.int32).reshape(-1, 4)
        self._check(self._lib.whenet_frame_heads(self._h, int(ticket), _ptr(rects), rects.shape[0]))

    def yolo_eval(self, yolo_outputs, anchors, num_classes: int, image_shape, max_boxes: int = 20,
                  score_threshold: float = .6, iou_threshold: float = .5, debug: bool = False):
        """yolo_v3/model.py:193-232 on numpy feature maps [gh, gw, 3*(5+C)] (or with a leading batch axis of 1).
        Returns boxes [k,4] (y_min, x_min, y_max, x_max), scores [k], classes [k]; with debug also the box
        indices and every decoded box / score."""
        maps = []
        for m in yolo_outputs:
            m = np.asarray(m)
            if m.ndim == 4:
                if m.shape[0] != 1:
                    raise ValueError("yolo_eval: batch of one, as YOLO.detect feeds it")
                m = m[0]
            if m.ndim != 3 or m.shape[2] != 3 * (5 + num_classes):
                raise ValueError(f"yolo_eval: feature map of shape {m.shape}, expected [gh, gw, {3 * (5 + num_classes)}]")
            maps.append(np.ascontiguousarray(m, np.float32))
        anchors = np.ascontiguousarray(anchors, np.float32).reshape(-1, 2)
        L = len(maps)
        ptrs = (_P * L)(*[_ptr(m) for m in maps])
        gh = np.array([m.shape[0] for m in maps], np.int32)
        gw = np.array([m.shape[1] for m in maps], np.int32)
        n_all = int(sum(m.shape[0] * m.shape[1] * 3 for m in maps))
        if max_boxes < 1:
            raise ValueError("yolo_eval: max_boxes must be >= 1")
        cap = num_classes * min(int(max_boxes), n_all)          # (no more selections per class than boxes)
        boxes = np.empty((cap, 4), np.float32)
        scores = np.empty(cap, np.float32)
        classes = np.empty(cap, np.int32)
        index = np.empty(cap, np.int32)
        all_boxes = np.empty((n_all, 4), np.float32) if debug else None
        all_scores = np.empty((n_all, num_classes), np.float32) if debug else None
        count = C.c_int(0)
        self._check(self._lib.whenet_yolo_eval(self._h, ptrs, _ptr(gh), _ptr(gw), L, _ptr(anchors), anchors.shape[0],
                                               num_classes, float(image_shape[0]), float(image_shape[1]),
                                               float(score_threshold), float(iou_threshold), int(max_boxes), _ptr(boxes),
                                               _ptr(scores), _ptr(classes), _ptr(index), C.byref(count), _ptr(all_boxes),
                                               _ptr(all_scores)))
        k = count.value
        res = (boxes[:k].copy(), scores[:k].copy(), classes[:k].copy())
        return res + (index[:k].copy(), all_boxes, all_scores) if debug else res

    # ---- the detector body (csrc/detector.cpp) --------------------------------------------------
    def detector_load(self, snapshot, dtype: str = "f16") -> None:
        """Attach a detector: packed snapshot bytes or a path (whenet_hip/detector_weights.py).  `dtype`: "f16" (binary16 storage,
        the default) or "f32" (float32 storage, the parity-grade body): option "detector_dtype" of the handle, set before the
        weights are packed.  A handle that holds a detector keeps its dtype (the library says so)."""
        if dtype not in DETECTOR_DTYPES:
            raise ValueError(f"detector dtype must be one of {sorted(DETECTOR_DTYPES)}, got {dtype!r}")
        if DETECTOR_DTYPES[dtype] != self._detector_dtype:
            self.set_option("detector_dtype", DETECTOR_DTYPES[dtype])
        if isinstance(snapshot, (bytes, bytearray, memoryview)):
            buf = (C.c_char * len(snapshot)).from_buffer_copy(bytes(snapshot))
            self._check(self._lib.whenet_detector_load_from_memory(self._h, C.cast(buf, _P), len(snapshot)))
        else:
            self._check(self._lib.whenet_detector_load(self._h, os.fsencode(snapshot)))

    def detector_forward(self, image: np.ndarray, kind: int, out_filters: int):
        """yolo_model.predict(image_data): image float32 [n,H,W,3] -> list of maps [n,gh,gw,out_filters], coarsest first."""
        x = np.ascontiguousarray(image, np.float32)
        if x.ndim != 4 or x.shape[3] != 3:
            raise ValueError(f"detector_forward: image must be float32 [n,H,W,3], got {x.shape}")
        n, H, W, _ = x.shape
        if H % 32 or W % 32 or H < 32 or W < 32:
            raise ValueError(f"Multiples of 32 required, got image size {(H, W)}")
        maps = [np.empty((n, (H // 32) << l, (W // 32) << l, out_filters), np.float32) for l in range(2 if kind == 1 else 3)]
        ptrs = (_P * len(maps))(*[_ptr(m) for m in maps])
        self._check(self._lib.whenet_detector_forward(self._h, _ptr(x), n, H, W, ptrs))
        return maps

    @staticmethod
    def _detect_outputs(anchors, num_classes: int, max_boxes: int):
        anchors = np.ascontiguousarray(anchors, np.float32).reshape(-1, 2)
        if max_boxes < 1:
            raise ValueError("detect: max_boxes must be >= 1")
        cap = int(num_classes) * int(max_boxes)
        return anchors, np.empty((cap, 4), np.float32), np.empty(cap, np.float32), np.empty(cap, np.int32), C.c_int(0)

    def op_detect(self, frame: np.ndarray, anchors, num_classes: int, size=(416, 416), score: float = .3, iou: float = .45,
                  max_boxes: int = 20, bgr: bool = True):
        """YOLO.detect (yolo_postprocess.py:180-205) of one host frame on the device: (boxes [k,4], scores [k], classes [k])."""
        frame = _frame_u8(frame)
        anchors, boxes, scores, classes, count = self._detect_outputs(anchors, num_classes, max_boxes)
        self._check(self._lib.whenet_op_detect(self._h, _ptr(frame), frame.shape[0], frame.shape[1], BGR if bgr else RGB, int(size[0]),
                                               int(size[1]), _ptr(anchors), anchors.shape[0], float(score), float(iou), int(max_boxes),
                                               _ptr(boxes), _ptr(scores), _ptr(classes), C.byref(count)))
        k = count.value
        return boxes[:k].copy(), scores[:k].copy(), classes[:k].copy()

    def frame_detect(self, ticket: int, anchors, num_classes: int, size=(416, 416), score: float = .3, iou: float = .45,
                     max_boxes: int = 20):
        """The same on the resident frame of `ticket` (frame_begin), before its heads."""
        anchors, boxes, scores, classes, count = self._detect_outputs(anchors, num_classes, max_boxes)
        self._check(self._lib.whenet_frame_detect(self._h, int(ticket), int(size[0]), int(size[1]), _ptr(anchors), anchors.shape[0],
                                                  float(score), float(iou), int(max_boxes), _ptr(boxes), _ptr(scores), _ptr(classes),
                                                  C.byref(count)))
        k = count.value
        return boxes[:k].copy(), scores[:k].copy(), classes[:k].copy()

    def frame_detect_heads(self, ticket: int, anchors, num_classes: int, size=(416, 416), score: float = .3, iou: float = .45,
                           max_boxes: int = 20) -> int:
        """frame_detect + frame_heads of the resident frame of `ticket` as ONE enqueue-only submission: returns at once with the
        capacity (rows) that `collect_detect` needs."""
        anchors = np.ascontiguousarray(anchors, np.float32).reshape(-1, 2)
        self._check(self._lib.whenet_frame_detect_heads(self._h, int(ticket), int(size[0]), int(size[1]), _ptr(anchors), anchors.shape[0],
                                                        float(score), float(iou), int(max_boxes)))
        return int(num_classes) * int(max_boxes)

    def collect_detect(self, ticket: int, capacity: int, want_logits: bool = False):
        """A `frame_detect_heads` ticket -> (boxes [k,4], scores [k], classes [k], rects [k,4], valid [k], ypr [k,3], argmax [k,3],
        logits [k,252] or None) over all k detections; rows of heads without a window inside the frame: valid 0, NaN / -1 / NaN."""
        cap = int(capacity)
        boxes, scores, classes = np.empty((cap, 4), np.float32), np.empty(cap, np.float32), np.empty(cap, np.int32)
        rects, valid = np.empty((cap, 4), np.int32), np.empty(cap, np.int32)
        ypr, am = np.empty((cap, 3), np.float32), np.empty((cap, 3), np.int32)
        lg = np.empty((cap, 252), np.float32) if want_logits else None
        count = C.c_int(0)
        self._check(self._lib.whenet_collect_detect(self._h, int(ticket), cap, C.byref(count), _ptr(boxes), _ptr(scores), _ptr(classes),
                                                    _ptr(rects), _ptr(valid), _ptr(ypr), _ptr(am), _ptr(lg)))
        k = count.value
        return tuple(None if a is None else a[:k].copy() for a in (boxes, scores, classes, rects, valid, ypr, am, lg))

    # ---- clips: F frames per submission ----------------------------------------------------------
    def clip_begin(self, frames: np.ndarray, bgr: bool = True) -> int:
        """Upload the F frames of a clip (uint8 [F,H,W,3], one size) once; the ticket goes to clip_detect_heads / collect_clip."""
        frames = clip_u8(frames)
        t = C.c_int(-1)
        self._check(self._lib.whenet_clip_begin(self._h, _ptr(frames), frames.shape[0], frames.shape[1], frames.shape[2],
                                                BGR if bgr else RGB, C.byref(t)))
        return t.value

    def clip_detect_heads(self, ticket: int, anchors, num_classes: int, size=(416, 416), score: float = .3, iou: float = .45,
                          max_boxes: int = 20, max_heads=None) -> int:
        """frame_detect_heads over the frames of the clip of `ticket` as ONE enqueue-only submission whose forward runs over
        `max_heads` rows (None: min(F * K, 256)); returns K, the detection slots per frame."""
        check_max_heads(max_heads)
        anchors = np.ascontiguousarray(anchors, np.float32).reshape(-1, 2)
        k = C.c_int(0)
        self._check(self._lib.whenet_clip_detect_heads(self._h, int(ticket), int(size[0]), int(size[1]), _ptr(anchors), anchors.shape[0],
                                                       float(score), float(iou), int(max_boxes), 0 if max_heads is None else int(max_heads),
                                                       C.byref(k)))
        return k.value

    def collect_clip(self, ticket: int, frames: int, slots_per_frame: int, want_logits: bool = False):
        """A `clip_detect_heads` ticket -> (counts [F], boxes [F,K,4], scores [F,K], classes [F,K], rects [F,K,4], valid [F,K],
        row [F,K], ypr [F,K,3], argmax [F,K,3], logits [F,K,252] or None, rows_used, overflow): slot (f, i) is detection i of frame
        f; row -1 (no window, beyond counts[f], or over max_heads): NaN / -1 / NaN."""
        F, K = int(frames), int(slots_per_frame)
        S = F * K
        counts = np.zeros(16, np.int32)
        boxes, scores, classes = np.empty((S, 4), np.float32), np.empty(S, np.float32), np.empty(S, np.int32)
        rects, valid, row = np.empty((S, 4), np.int32), np.empty(S, np.int32), np.empty(S, np.int32)
        ypr, am = np.empty((S, 3), np.float32), np.empty((S, 3), np.int32)
        lg = np.empty((S, 252), np.float32) if want_logits else None
        nf, used, over = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self._lib.whenet_collect_clip(self._h, int(ticket), S, C.byref(nf), _ptr(counts), _ptr(boxes), _ptr(scores),
                                                  _ptr(classes), _ptr(rects), _ptr(valid), _ptr(row), _ptr(ypr), _ptr(am), _ptr(lg),
                                                  C.byref(used), C.byref(over)))
        if nf.value != F:
            raise ValueError(f"collect_clip: the clip holds {nf.value} frames, not {F}")
        shaped = tuple(None if a is None else a.reshape((F, K) + a.shape[1:]) for a in (boxes, scores, classes, rects, valid, row, ypr, am, lg))
        return (counts[:F].copy(),) + shaped + (used.value, over.value)

    def op_letterbox_batch(self, frames: np.ndarray, size=(416, 416), bgr: bool = True, want_u8: bool = True, want_f32: bool = True):
        """`op_letterbox` of the F frames of a clip (uint8 [F,H,W,3]) in one call: (canvas uint8 [F,h,w,3], image float32 [F,h,w,3])."""
        frames = clip_u8(frames)
        F = frames.shape[0]
        oh, ow, _, _ = self._letterbox_outputs(size, False, False)
        u8 = np.empty((F, oh, ow, 3), np.uint8) if want_u8 else None
        f32 = np.empty((F, oh, ow, 3), np.float32) if want_f32 else None
        self._check(self._lib.whenet_op_letterbox_batch(self._h, _ptr(frames), F, frames.shape[1], frames.shape[2], BGR if bgr else RGB,
                                                        oh, ow, _ptr(u8), _ptr(f32)))
        return u8, f32

    def yolo_eval_batch(self, yolo_outputs, anchors, num_classes: int, image_shape, max_boxes: int = 20,
                        score_threshold: float = .6, iou_threshold: float = .5):
        """`yolo_eval` of F images that share a shape: maps [F, gh, gw, 3*(5+C)] per layer -> a list of F tuples
        (boxes [k,4], scores [k], classes [k], index [k]), each what `yolo_eval(..., debug=True)[:4]` returns for that image alone."""
        maps = [np.ascontiguousarray(m, np.float32) for m in yolo_outputs]
        F = maps[0].shape[0] if maps and maps[0].ndim == 4 else 0
        for m in maps:
            if m.ndim != 4 or m.shape[0] != F or m.shape[3] != 3 * (5 + num_classes):
                raise ValueError(f"yolo_eval_batch: feature map of shape {m.shape}, expected [{F}, gh, gw, {3 * (5 + num_classes)}]")
        if not 1 <= F <= MAX_CLIP_FRAMES:
            raise ValueError(f"yolo_eval_batch: {F} images, expected 1..{MAX_CLIP_FRAMES}")
        if max_boxes < 1:
            raise ValueError("yolo_eval_batch: max_boxes must be >= 1")
        anchors = np.ascontiguousarray(anchors, np.float32).reshape(-1, 2)
        L = len(maps)
        ptrs = (_P * L)(*[_ptr(m) for m in maps])
        gh = np.array([m.shape[1] for m in maps], np.int32)
        gw = np.array([m.shape[2] for m in maps], np.int32)
        n_all = int(sum(m.shape[1] * m.shape[2] * 3 for m in maps))
        cap = num_classes * min(int(max_boxes), n_all)
        boxes, scores = np.empty((F, cap, 4), np.float32), np.empty((F, cap), np.float32)
        classes, index, counts = np.empty((F, cap), np.int32), np.empty((F, cap), np.int32), np.zeros(F, np.int32)
        self._check(self._lib.whenet_yolo_eval_batch(self._h, ptrs, F, _ptr(gh), _ptr(gw), L, _ptr(anchors), anchors.shape[0], num_classes,
                                                     float(image_shape[0]), float(image_shape[1]), float(score_threshold),
                                                     float(iou_threshold), int(max_boxes), _ptr(boxes), _ptr(scores), _ptr(classes),
                                                     _ptr(index), _ptr(counts)))
        return [tuple(a[f, :counts[f]].copy() for a in (boxes, scores, classes, index)) for f in range(F)]

    # ---- mixed clips: frames of different sizes per submission; the letterbox geometry cache ---------
    def clip_begin_mixed(self, frames: list, bgr: bool = True) -> int:
        """Upload the frames of a mixed clip (a list of uint8 [H_i,W_i,3] arrays, each of its own size) once, packed back to back; the
        ticket goes to clip_detect_heads / collect_clip like `clip_begin`'s."""
        frames = mixed_u8(frames)
        ptrs, fh, fw = _mixed_args(frames)
        t = C.c_int(-1)
        self._check(self._lib.whenet_clip_begin_mixed(self._h, ptrs, len(frames), _ptr(fh), _ptr(fw), BGR if bgr else RGB, C.byref(t)))
        return t.value

    # ---- YUV 4:2:0 ingest: a decoder's planes in, the resident BGR frame built on the device ---------
    def op_yuv_to_bgr(self, frames: list) -> list:
        """The conversion kernel alone on 1..16 frames (`whenet_hip.yuv.YUVFrame`) of their own sizes, formats and matrices, packed
        back to back on the device as a mixed clip packs them -> a list of uint8 [H_i,W_i,3] arrays (B, G, R)."""
        arr, descs = _yuv_descs(frames)
        outs = [np.empty((max(int(d.h), 0), max(int(d.w), 0), 3), np.uint8) for d in descs]
        ptrs = (_P * max(len(outs), 1))(*[o.ctypes.data if o.size else None for o in outs])
        self._check(self._lib.whenet_op_yuv_to_bgr(self._h, arr, len(descs), ptrs))
        return outs

    def frame_begin_yuv(self, frame) -> int:
        """`frame_begin` from a decoder's planes: they are uploaded as they are and converted on the device; the ticket is
        `frame_begin(frame.to_bgr(), bgr=True)`'s in everything that follows."""
        arr, _ = _yuv_descs([frame])
        t = C.c_int(-1)
        self._check(self._lib.whenet_frame_begin_yuv(self._h, arr, C.byref(t)))
        return t.value

    def clip_begin_yuv(self, frames: list) -> int:
        """`clip_begin` (frames of one size) or `clip_begin_mixed` (otherwise) from the planes of 1..16 frames, each with its own
        format and matrix; the ticket goes to clip_detect_heads / collect_clip."""
        arr, descs = _yuv_descs(frames)
        t = C.c_int(-1)
        self._check(self._lib.whenet_clip_begin_yuv(self._h, arr, len(descs), C.byref(t)))
        return t.value

    # ---- ingest from device memory: the frame (or its planes) is already in HBM ------------------------
    def frame_begin_device(self, frame, bgr: bool = True, stream=None) -> int:
        """`frame_begin` of a uint8 [H,W,3] device array (or a DeviceFrame): no host copy, no PCIe; ordered on `stream` (None: the
        default stream; torch: `torch.cuda.current_stream().cuda_stream`)."""
        f = device_frame(frame)
        t = C.c_int(-1)
        self._check(self._lib.whenet_frame_begin_device(self._h, f.ptr, f.pitch, f.h, f.w, BGR if bgr else RGB, _stream(stream), C.byref(t)))
        return t.value

    def clip_begin_device(self, frames, bgr: bool = True, stream=None) -> int:
        """`clip_begin` (frames of one size) or `clip_begin_mixed` (otherwise) of frames in device memory: a list of uint8 [H,W,3]
        device arrays or one [F,H,W,3] device array."""
        items = device_frames(frames)
        ptrs, pitch, fh, fw = _device_args(items)
        t = C.c_int(-1)
        self._check(self._lib.whenet_clip_begin_device(self._h, ptrs, _ptr(pitch), len(items), _ptr(fh), _ptr(fw), BGR if bgr else RGB,
                                                       _stream(stream), C.byref(t)))
        return t.value

    def frame_begin_yuv_device(self, frame, stream=None) -> int:
        """`frame_begin_yuv` of a frame whose planes are in device memory (a `YUVFrame` with `on_device`, or a YuvFrameC)."""
        arr, _ = _yuv_descs([frame])
        t = C.c_int(-1)
        self._check(self._lib.whenet_frame_begin_yuv_device(self._h, arr, _stream(stream), C.byref(t)))
        return t.value

    def clip_begin_yuv_device(self, frames: list, stream=None) -> int:
        """`clip_begin_yuv` of frames whose planes are in device memory."""
        arr, descs = _yuv_descs(frames)
        t = C.c_int(-1)
        self._check(self._lib.whenet_clip_begin_yuv_device(self._h, arr, len(descs), _stream(stream), C.byref(t)))
        return t.value

    def op_pack_device(self, frames, stream=None) -> list:
        """The packing kernel alone on 1..16 frames in device memory (uint8 [H_i,W_i,3] device arrays or DeviceFrames), packed back
        to back on the device as a mixed clip packs them -> a list of tight uint8 [H_i,W_i,3] host arrays."""
        items = device_frames(frames) if len(frames) else []
        ptrs, pitch, fh, fw = _device_args(items)
        outs = [np.empty((max(f.h, 0), max(f.w, 0), 3), np.uint8) for f in items]
        optrs = (_P * max(len(outs), 1))(*[o.ctypes.data if o.size else None for o in outs])
        self._check(self._lib.whenet_op_pack_device(self._h, ptrs, _ptr(pitch), len(items), _ptr(fh), _ptr(fw), _stream(stream), optrs))
        return outs

    def op_yuv_to_bgr_device(self, frames: list, stream=None) -> list:
        """The plane kernel alone on 1..16 frames whose planes are in device memory, with their pitches -> a list of uint8
        [H_i,W_i,3] host arrays (B, G, R): the device twin of `op_yuv_to_bgr`."""
        arr, descs = _yuv_descs(frames)
        outs = [np.empty((max(int(d.h), 0), max(int(d.w), 0), 3), np.uint8) for d in descs]
        ptrs = (_P * max(len(outs), 1))(*[o.ctypes.data if o.size else None for o in outs])
        self._check(self._lib.whenet_op_yuv_to_bgr_device(self._h, arr, len(descs), _stream(stream), ptrs))
        return outs

    # ---- extended YUV ingest (include/whenet_hip_yuv_ext.h): the same seven calls for whenet_yuvx_frame_t ---------------
    def _op_yuvx(self, fn, frames, *stream):
        arr, descs = _yuvx_descs(frames)
        outs = [np.empty((max(int(d.h), 0), max(int(d.w), 0), 3), np.uint8) for d in descs]
        ptrs = (_P * max(len(outs), 1))(*[o.ctypes.data if o.size else None for o in outs])
        self._check(fn(self._h, arr, len(descs), *stream, ptrs))
        return outs

    def op_yuvx_to_bgr(self, frames: list) -> list:
        """`op_yuv_to_bgr` through the extended call: frames of any layout, container and matrix (`YUVFrame`s, old formats included)."""
        return self._op_yuvx(self._lib.whenet_op_yuvx_to_bgr, frames)

    def op_yuvx_to_bgr_device(self, frames: list, stream=None) -> list:
        """`op_yuv_to_bgr_device` through the extended call."""
        return self._op_yuvx(self._lib.whenet_op_yuvx_to_bgr_device, frames, _stream(stream))

    def frame_begin_yuvx(self, frame) -> int:
        """`frame_begin_yuv` through the extended call."""
        arr, _ = _yuvx_descs([frame])
        t = C.c_int(-1)
        self._check(self._lib.whenet_frame_begin_yuvx(self._h, arr, C.byref(t)))
        return t.value

    def clip_begin_yuvx(self, frames: list) -> int:
        """`clip_begin_yuv` through the extended call: a clip may mix old and new formats."""
        arr, descs = _yuvx_descs(frames)
        t = C.c_int(-1)
        self._check(self._lib.whenet_clip_begin_yuvx(self._h, arr, len(descs), C.byref(t)))
        return t.value

    def frame_begin_yuvx_device(self, frame, stream=None) -> int:
        """`frame_begin_yuv_device` through the extended call."""
        arr, _ = _yuvx_descs([frame])
        t = C.c_int(-1)
        self._check(self._lib.whenet_frame_begin_yuvx_device(self._h, arr, _stream(stream), C.byref(t)))
        return t.value

    def clip_begin_yuvx_device(self, frames: list, stream=None) -> int:
        """`clip_begin_yuv_device` through the extended call."""
        arr, descs = _yuvx_descs(frames)
        t = C.c_int(-1)
        self._check(self._lib.whenet_clip_begin_yuvx_device(self._h, arr, len(descs), _stream(stream), C.byref(t)))
        return t.value

    def op_letterbox_mixed(self, frames: list, size=(416, 416), bgr: bool = True, want_u8: bool = True, want_f32: bool = True):
        """`op_letterbox` of F frames of their own sizes in one call: (canvas uint8 [F,h,w,3], image float32 [F,h,w,3])."""
        frames = mixed_u8(frames)
        F = len(frames)
        oh, ow, _, _ = self._letterbox_outputs(size, False, False)
        u8 = np.empty((F, oh, ow, 3), np.uint8) if want_u8 else None
        f32 = np.empty((F, oh, ow, 3), np.float32) if want_f32 else None
        ptrs, fh, fw = _mixed_args(frames)
        self._check(self._lib.whenet_op_letterbox_mixed(self._h, ptrs, F, _ptr(fh), _ptr(fw), BGR if bgr else RGB, oh, ow, _ptr(u8),
                                                        _ptr(f32)))
        return u8, f32

    def yolo_eval_mixed(self, yolo_outputs, anchors, num_classes: int, image_shapes, max_boxes: int = 20,
                        score_threshold: float = .6, iou_threshold: float = .5):
        """`yolo_eval_batch` of F images that each have their own shape: image_shapes [F,2] = (h, w) per image -> a list of F tuples
        (boxes [k,4], scores [k], classes [k], index [k]), each what `yolo_eval(..., debug=True)[:4]` returns for that image alone."""
        maps = [np.ascontiguousarray(m, np.float32) for m in yolo_outputs]
        F = maps[0].shape[0] if maps and maps[0].ndim == 4 else 0
        for m in maps:
            if m.ndim != 4 or m.shape[0] != F or m.shape[3] != 3 * (5 + num_classes):
                raise ValueError(f"yolo_eval_mixed: feature map of shape {m.shape}, expected [{F}, gh, gw, {3 * (5 + num_classes)}]")
        if not 1 <= F <= MAX_CLIP_FRAMES:
            raise ValueError(f"yolo_eval_mixed: {F} images, expected 1..{MAX_CLIP_FRAMES}")
        try:
            shapes = np.ascontiguousarray(image_shapes, np.float32)
        except (TypeError, ValueError):
            raise ValueError("yolo_eval_mixed: image_shapes must be [F,2] = (h, w) per image") from None
        if shapes.shape != (F, 2) or not (shapes > 0).all():
            raise ValueError(f"yolo_eval_mixed: image_shapes must be [{F},2] = positive (h, w) per image, got shape {shapes.shape}")
        if max_boxes < 1:
            raise ValueError("yolo_eval_mixed: max_boxes must be >= 1")
        anchors = np.ascontiguousarray(anchors, np.float32).reshape(-1, 2)
        L = len(maps)
        ptrs = (_P * L)(*[_ptr(m) for m in maps])
        gh = np.array([m.shape[1] for m in maps], np.int32)
        gw = np.array([m.shape[2] for m in maps], np.int32)
        n_all = int(sum(m.shape[1] * m.shape[2] * 3 for m in maps))
        cap = num_classes * min(int(max_boxes), n_all)
        boxes, scores = np.empty((F, cap, 4), np.float32), np.empty((F, cap), np.float32)
        classes, index, counts = np.empty((F, cap), np.int32), np.empty((F, cap), np.int32), np.zeros(F, np.int32)
        self._check(self._lib.whenet_yolo_eval_mixed(self._h, ptrs, F, _ptr(gh), _ptr(gw), L, _ptr(anchors), anchors.shape[0], num_classes,
                                                     _ptr(shapes), float(score_threshold), float(iou_threshold), int(max_boxes),
                                                     _ptr(boxes), _ptr(scores), _ptr(classes), _ptr(index), _ptr(counts)))
        return [tuple(a[f, :counts[f]].copy() for a in (boxes, scores, classes, index)) for f in range(F)]

    def letterbox_cache_stats(self) -> dict:
        """The letterbox geometry cache of the handle's engines (option "letterbox_cache", 1..32 entries per engine, default 16):
        {"entries", "hits", "misses", "host_waits"}.  A warmed set of frame sizes costs no miss and no wait."""
        out = (C.c_int32 * 4)()
        self._check(self._lib.whenet_letterbox_cache_stats(self._h, C.byref(out)))
        return dict(zip(("entries", "hits", "misses", "host_waits"), (int(v) for v in out)))

    def op_head_compact(self, valid, count, max_heads: int):
        """The numbering of a clip's heads alone: valid int32 [F,K], count int32 [F] -> (row int32 [F,K], slot_of_row int32
        [max_heads], rows_used, overflow)."""
        valid = np.ascontiguousarray(valid, np.int32)
        count = np.ascontiguousarray(count, np.int32).reshape(-1)
        if valid.ndim != 2 or valid.shape[0] != count.shape[0]:
            raise ValueError(f"op_head_compact: valid must be [F,K] and count [F], got {valid.shape} and {count.shape}")
        check_max_heads(int(max_heads))
        F, K = valid.shape
        row, sor = np.empty((F, K), np.int32), np.empty(int(max_heads), np.int32)
        used, over = np.zeros(1, np.int32), np.zeros(1, np.int32)
        self._check(self._lib.whenet_op_head_compact(self._h, _ptr(valid), _ptr(count), F, K, int(max_heads), _ptr(row), _ptr(sor),
                                                     _ptr(used), _ptr(over)))
        return row, sor, int(used[0]), int(over[0])

    def op_head_plan(self, frame_h: int, frame_w: int, boxes, want_plans: bool = True):
        """The window / crop plan kernel alone on caller boxes [k,4] (y_min, x_min, y_max, x_max), 1 <= k <= 2048:
        (rects int32 [k,4], valid int32 [k], plans int32 [k, CROP_PLAN_INTS] or None)."""
        b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
        k = b.shape[0]
        rects, valid = np.empty((k, 4), np.int32), np.empty(k, np.int32)
        plans = np.empty((k, CROP_PLAN_INTS), np.int32) if want_plans else None
        self._check(self._lib.whenet_op_head_plan(self._h, int(frame_h), int(frame_w), _ptr(b), k, _ptr(rects), _ptr(valid), _ptr(plans)))
        return rects, valid, plans

    def op_dconv(self, x: np.ndarray, kernel: np.ndarray, bias: np.ndarray, stride: int = 1, leaky: bool = True, x2=None, skip=None,
                 f32_out: bool = False) -> np.ndarray:
        """One convolution of the body on caller tensors: x [n,H,W,cin] (with x2 [n,2H,2W,cin2]: the half-resolution source of the
        upsample + concatenate read), kernel HWIO, bias [cout] -> [n,Ho,Wo,cout] float32."""
        x = np.ascontiguousarray(x, np.float32)
        kernel = np.ascontiguousarray(kernel, np.float32)
        bias = np.ascontiguousarray(bias, np.float32)
        k, _, ctot, cout = kernel.shape
        n, cin = x.shape[0], x.shape[3]
        if x2 is not None:
            x2 = np.ascontiguousarray(x2, np.float32)
            H, W, cin2 = x2.shape[1], x2.shape[2], x2.shape[3]
            assert x.shape[1:3] == (H // 2, W // 2) and x2.shape[0] == n, (x.shape, x2.shape)
        else:
            H, W, cin2 = x.shape[1], x.shape[2], 0
        assert kernel.shape[0] == kernel.shape[1] and ctot == cin + cin2 and bias.shape == (cout,), (kernel.shape, cin, cin2, bias.shape)
        Ho, Wo = ((H - 2) // 2 + 1, (W - 2) // 2 + 1) if stride == 2 else (H, W)
        if skip is not None:
            skip = np.ascontiguousarray(skip, np.float32)
            assert skip.shape == (n, Ho, Wo, cout), skip.shape
        out = np.empty((n, Ho, Wo, cout), np.float32)
        self._check(self._lib.whenet_op_dconv(self._h, _ptr(x), n, H, W, cin, _ptr(x2), cin2, _ptr(kernel), _ptr(bias), k, int(stride),
                                              cout, int(bool(leaky)), _ptr(skip), int(bool(f32_out)), _ptr(out)))
        return out

    def op_dpool(self, x: np.ndarray, stride: int) -> np.ndarray:
        """MaxPooling2D(2, strides=stride, 'same') of the tiny body on x [n,H,W,c] -> float32."""
        x = np.ascontiguousarray(x, np.float32)
        n, H, W, c = x.shape
        Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if stride == 2 else (H, W)
        out = np.empty((n, Ho, Wo, c), np.float32)
        self._check(self._lib.whenet_op_dpool(self._h, _ptr(x), n, H, W, c, int(stride), _ptr(out)))
        return out

    def op_annotate(self, frame: np.ndarray, rects, valid, ypr, surface: SurfaceC, bgr: bool = True, display: int = DISPLAY_SIMPLE) -> None:
        """`whenet_op_annotate_ex`: the overlay kernels alone, host to host (works on a postproc handle)."""
        frame = np.ascontiguousarray(frame, np.uint8)
        if frame.ndim != 3 or frame.shape[2] != 3:
            raise ValueError(f"frame must be uint8 [H,W,3], got {frame.shape}")
        rects, valid, ypr = overlay_heads(rects, valid, ypr)
        self._check(self._lib.whenet_op_annotate_ex(self._h, _ptr(frame), frame.shape[0], frame.shape[1], BGR if bgr else RGB, _ptr(rects),
                                                    _ptr(valid), _ptr(ypr), rects.shape[0], C.byref(surface), int(display)))

    def op_jpeg_encode(self, surface: SurfaceC, h: int, w: int, bgr: bool, quality: int, out: np.ndarray, sampling: str = "4:2:0",
                       optimize: bool = False, hist=None):
        """`whenet_op_jpeg_encode_ex`: the encoder's kernels alone, host to host (works on a postproc handle), into the uint8 array
        `out` (its size is the capacity): (return code OK or EOVERFLOW, the stream's full length).  `hist`: None or a uint32 [4,256]
        array for the device histograms of optimize=True."""
        size = C.c_int64(0)
        rc = self._lib.whenet_op_jpeg_encode_ex(self._h, C.byref(surface), int(h), int(w), BGR if bgr else RGB, int(quality),
                                                jpeg_sampling_code(sampling), int(bool(optimize)), _ptr(out) if out.size else None,
                                                int(out.size), C.byref(size), None if hist is None else _ptr(_hist_array(hist)))
        if rc != EOVERFLOW:
            self._check(rc)
        return rc, int(size.value)

    def jpeg_encode_device(self, surface: SurfaceC, h: int, w: int, bgr: bool, quality: int, dst: int, cap: int, dsize: int, stream=None,
                           sampling: str = "4:2:0", optimize: bool = False) -> None:
        """`whenet_jpeg_encode_device_ex`: enqueue the encoder on a surface in device memory; `dst` (cap bytes) and `dsize` (one
        int64) are device addresses.  The host does not wait."""
        self._check(self._lib.whenet_jpeg_encode_device_ex(self._h, C.byref(surface), int(h), int(w), BGR if bgr else RGB, int(quality),
                                                           jpeg_sampling_code(sampling), int(bool(optimize)), _P(int(dst)), int(cap),
                                                           _P(int(dsize)), _stream(stream)))

    def frame_annotate_jpeg(self, ticket: int, frame_index: int, display: int, quality: int, out: np.ndarray, result: np.ndarray,
                            sampling: str = "4:2:0", optimize: bool = False) -> None:
        """`whenet_frame_annotate_jpeg_ex`: enqueue the annotated frame of a ticket as a JPEG stream into the uint8 array `out` (its
        size is the capacity); result = int64 [2]: the stream's length and the status.  Both are complete when the ticket's collect
        call returns and must stay alive until then."""
        status = result[1:].view(np.int32)
        self._check(self._lib.whenet_frame_annotate_jpeg_ex(self._h, int(ticket), int(frame_index), int(display), int(quality),
                                                            jpeg_sampling_code(sampling), int(bool(optimize)),
                                                            _ptr(out) if out.size else None, int(out.size), _ptr(result), _ptr(status)))

    def op_jpeg_decode(self, data, surface: SurfaceC, bgr: bool) -> np.ndarray:
        """`whenet_op_jpeg_decode`: the decoder's kernels alone, host to host (works on a postproc handle), into a host surface: the
        two status words int32 [2] (OK or EFORMAT, the first bad interval or -1)."""
        a = _stream_array(data)
        status = np.zeros(2, np.int32)
        self._check(self._lib.whenet_op_jpeg_decode(self._h, _ptr(a) if a.size else None, int(a.size), C.byref(surface),
                                                    BGR if bgr else RGB, _ptr(status)))
        return status

    def op_jpeg_decode_ex(self, data, surface: SurfaceC, bgr: bool, entropy: int, seg_bytes: int = 128):
        """`whenet_op_jpeg_decode_ex`: `op_jpeg_decode` with the entropy stage's form forced (0: an interval per lane, 1: segmented with
        segments of `seg_bytes`): (the two status words, the statistics int64 [8] read back from the device)."""
        a = _stream_array(data)
        status, stats = np.zeros(2, np.int32), np.zeros(8, np.int64)
        self._check(self._lib.whenet_op_jpeg_decode_ex(self._h, _ptr(a) if a.size else None, int(a.size), C.byref(surface),
                                                       BGR if bgr else RGB, int(entropy), int(seg_bytes), _ptr(status), _ptr(stats)))
        return status, stats

    def op_jpeg_decode_rule(self, data, surface: SurfaceC, bgr: bool, entropy: int = -1, seg_bytes: int = 128, rule=None):
        """`whenet_op_jpeg_decode_rule`: the decoder's kernels alone by the rule "own", "libjpeg" or None (the handle's option
        "jpeg_rule"); entropy -1 (the handle's options), 0 or 1: (the two status words, the statistics int64 [8])."""
        a = _stream_array(data)
        status, stats = np.zeros(2, np.int32), np.zeros(8, np.int64)
        self._check(self._lib.whenet_op_jpeg_decode_rule(self._h, _ptr(a) if a.size else None, int(a.size), C.byref(surface),
                                                         BGR if bgr else RGB, int(entropy), int(seg_bytes), jpeg_rule_code(rule),
                                                         _ptr(status), _ptr(stats)))
        return status, stats

    def op_jpeg_decode_progressive(self, data, surface: SurfaceC, bgr: bool, rule=None):
        """`whenet_op_jpeg_decode_progressive`: the kernels alone on a baseline or progressive stream: (the two status words, the
        statistics int64 [8]: for a progressive stream items, levels, scans, scan-kernel launches)."""
        a = _stream_array(data)
        status, stats = np.zeros(2, np.int32), np.zeros(8, np.int64)
        self._check(self._lib.whenet_op_jpeg_decode_progressive(self._h, _ptr(a) if a.size else None, int(a.size), C.byref(surface),
                                                                BGR if bgr else RGB, jpeg_rule_code(rule), _ptr(status), _ptr(stats)))
        return status, stats

    def jpeg_progressive_counters(self) -> dict:
        """Host-side counts of the progressive decodes the handle's engines enqueued: {"decodes", "launches" of the scan kernel (a
        level each by default), "scans" in them}."""
        out = (C.c_int64 * 4)()
        self._check(self._lib.whenet_jpeg_progressive_counters(self._h, C.byref(out)))
        return {"decodes": int(out[0]), "launches": int(out[1]), "scans": int(out[2])}

    def jpeg_decode_counters(self) -> dict:
        """Host-side counts of the JPEG decodes the handle's engines launched in each form of the entropy stage:
        {"interval": form 0, "segmented": form 1} (options "jpeg_entropy", "jpeg_seg_bytes")."""
        out = (C.c_int64 * 4)()
        self._check(self._lib.whenet_jpeg_decode_counters(self._h, C.byref(out)))
        return {"interval": int(out[0]), "segmented": int(out[1])}

    def jpeg_decode_device(self, info: JpegInfoC, d_entropy: int, nbytes: int, surface: SurfaceC, bgr: bool, d_status: int, stream=None) -> None:
        """`whenet_jpeg_decode_device`: enqueue the decoder on entropy data in device memory; `d_entropy` (nbytes bytes) and
        `d_status` (two int32) are device addresses, `surface` is a device surface.  The host does not wait."""
        self._check(self._lib.whenet_jpeg_decode_device(self._h, C.byref(info), _P(int(d_entropy)), int(nbytes), C.byref(surface),
                                                        BGR if bgr else RGB, _P(int(d_status)), _stream(stream)))

    def frame_begin_jpeg(self, data, status: np.ndarray, bgr: bool = True, rule=None, progressive=None) -> int:
        """`whenet_frame_begin_jpeg`: `frame_begin` from the bytes of a JPEG stream, decoded on the device.  status = int32 [2], complete
        when the ticket's collect call returns; it must stay alive until then.  rule: None (the handle's option "jpeg_rule"), or "own" /
        "libjpeg" for this call (`whenet_frame_begin_jpeg_rule`)."""
        a = _stream_array(data)
        if status.dtype != np.int32 or status.size != 2 or not status.flags.c_contiguous:
            raise ValueError("status must be a contiguous int32 [2] array")
        t = C.c_int(-1)
        if progressive:      # (None / False: the handle's option "jpeg_progressive" decides, as in the calls below)
            self._check(self._lib.whenet_frame_begin_jpeg_progressive(self._h, _ptr(a) if a.size else None, int(a.size), BGR if bgr else RGB,
                                                                      jpeg_rule_code(rule), C.byref(t), _ptr(status)))
            return t.value
        if rule is not None:
            self._check(self._lib.whenet_frame_begin_jpeg_rule(self._h, _ptr(a) if a.size else None, int(a.size), BGR if bgr else RGB,
                                                               jpeg_rule_code(rule), C.byref(t), _ptr(status)))
            return t.value
        self._check(self._lib.whenet_frame_begin_jpeg(self._h, _ptr(a) if a.size else None, int(a.size), BGR if bgr else RGB, C.byref(t),
                                                      _ptr(status)))
        return t.value

    def clip_begin_jpeg(self, datas, status: np.ndarray, bgr: bool = True, rule=None, progressive: bool = False) -> int:
        """`whenet_clip_begin_jpeg`: `clip_begin` / `clip_begin_mixed` from the bytes of 1..16 JPEG streams, decoded on the device in one
        submission.  status = int32 [F,2], complete when the ticket's collect call returns; it must stay alive until then.  rule: as
        `frame_begin_jpeg` (`whenet_clip_begin_jpeg_rule`).  progressive=True: progressive (SOF2) streams are accepted too
        (`whenet_clip_begin_jpeg_progressive`); the handle's option "jpeg_progressive" is not read here."""
        arrs, ptrs, sizes = _clip_streams(datas)
        if status.dtype != np.int32 or status.size != 2 * len(arrs) or not status.flags.c_contiguous:
            raise ValueError("status must be a contiguous int32 [F,2] array")
        t = C.c_int(-1)
        if progressive:
            self._check(self._lib.whenet_clip_begin_jpeg_progressive(self._h, ptrs, _ptr(sizes) if sizes.size else None, len(arrs),
                                                                     BGR if bgr else RGB, jpeg_rule_code(rule), C.byref(t),
                                                                     _ptr(status) if status.size else None))
            return t.value
        if rule is not None:
            self._check(self._lib.whenet_clip_begin_jpeg_rule(self._h, ptrs, _ptr(sizes) if sizes.size else None, len(arrs), BGR if bgr else RGB,
                                                              jpeg_rule_code(rule), C.byref(t), _ptr(status) if status.size else None))
            return t.value
        self._check(self._lib.whenet_clip_begin_jpeg(self._h, ptrs, _ptr(sizes) if sizes.size else None, len(arrs), BGR if bgr else RGB,
                                                     C.byref(t), _ptr(status) if status.size else None))
        return t.value

    def op_jpeg_decode_clip(self, datas, surfaces, bgr: bool, entropy: int = -1, seg_bytes: int = 128) -> np.ndarray:
        """`whenet_op_jpeg_decode_clip`: the clip kernels alone, host to host (works on a postproc handle), stream f into host surface
        f; entropy -1 (the handle's options), 0 or 1.  The status words int32 [F,2]."""
        arrs, ptrs, sizes = _clip_streams(datas)
        surf = (SurfaceC * max(len(surfaces), 1))(*surfaces)
        status = np.zeros((len(arrs), 2), np.int32)
        self._check(self._lib.whenet_op_jpeg_decode_clip(self._h, ptrs, _ptr(sizes) if sizes.size else None, len(arrs), surf,
                                                         BGR if bgr else RGB, _ptr(status) if status.size else None, int(entropy),
                                                         int(seg_bytes)))
        return status

    def op_jpeg_decode_clip_rule(self, datas, surfaces, bgr: bool, entropy: int = -1, seg_bytes: int = 128, rule=None) -> np.ndarray:
        """`whenet_op_jpeg_decode_clip_rule`: `op_jpeg_decode_clip` by the rule "own", "libjpeg" or None (the handle's option)."""
        arrs, ptrs, sizes = _clip_streams(datas)
        surf = (SurfaceC * max(len(surfaces), 1))(*surfaces)
        status = np.zeros((len(arrs), 2), np.int32)
        self._check(self._lib.whenet_op_jpeg_decode_clip_rule(self._h, ptrs, _ptr(sizes) if sizes.size else None, len(arrs), surf,
                                                              BGR if bgr else RGB, _ptr(status) if status.size else None, int(entropy),
                                                              int(seg_bytes), jpeg_rule_code(rule)))
        return status

    def op_jpeg_decode_clip_progressive(self, datas, surfaces, bgr: bool, entropy: int = -1, seg_bytes: int = 128, rule=None) -> np.ndarray:
        """`whenet_op_jpeg_decode_clip_progressive`: `op_jpeg_decode_clip_rule` for clips that may hold progressive (SOF2) streams."""
        arrs, ptrs, sizes = _clip_streams(datas)
        surf = (SurfaceC * max(len(surfaces), 1))(*surfaces)
        status = np.zeros((len(arrs), 2), np.int32)
        self._check(self._lib.whenet_op_jpeg_decode_clip_progressive(self._h, ptrs, _ptr(sizes) if sizes.size else None, len(arrs), surf,
                                                                     BGR if bgr else RGB, _ptr(status) if status.size else None,
                                                                     int(entropy), int(seg_bytes), jpeg_rule_code(rule)))
        return status

    def op_jpeg_decode_oriented(self, data, surface: SurfaceC, bgr: bool, entropy: int = -1, seg_bytes: int = 128, rule=None,
                                progressive=None, orient=True):
        """`whenet_op_jpeg_decode_oriented`: the kernels alone into a surface of the ORIENTED size; progressive / orient: None (the
        handle's option), False or True: (the two status words, the statistics int64 [8], the orientation applied)."""
        a = _stream_array(data)
        status, stats, applied = np.zeros(2, np.int32), np.zeros(8, np.int64), np.ones(1, np.int32)
        self._check(self._lib.whenet_op_jpeg_decode_oriented(self._h, _ptr(a) if a.size else None, int(a.size), C.byref(surface),
                                                             BGR if bgr else RGB, int(entropy), int(seg_bytes), jpeg_rule_code(rule),
                                                             jpeg_tristate(progressive), jpeg_tristate(orient), _ptr(status), _ptr(stats),
                                                             _ptr(applied)))
        return status, stats, int(applied[0])

    def op_jpeg_decode_clip_oriented(self, datas, surfaces, bgr: bool, entropy: int = -1, seg_bytes: int = 128, rule=None,
                                     progressive: bool = False, orient: bool = True):
        """`whenet_op_jpeg_decode_clip_oriented`: (the status words int32 [F,2], the orientation applied to each frame int32 [F])."""
        arrs, ptrs, sizes = _clip_streams(datas)
        surf = (SurfaceC * max(len(surfaces), 1))(*surfaces)
        status, applied = np.zeros((len(arrs), 2), np.int32), np.ones(max(len(arrs), 1), np.int32)
        self._check(self._lib.whenet_op_jpeg_decode_clip_oriented(self._h, ptrs, _ptr(sizes) if sizes.size else None, len(arrs), surf,
                                                                  BGR if bgr else RGB, _ptr(status) if status.size else None, int(entropy),
                                                                  int(seg_bytes), jpeg_rule_code(rule), int(bool(progressive)),
                                                                  int(bool(orient)), _ptr(applied)))
        return status, applied[:len(arrs)]

    def frame_begin_jpeg_oriented(self, data, status: np.ndarray, bgr: bool = True, rule=None, progressive=None, orient=True):
        """`whenet_frame_begin_jpeg_oriented`: `frame_begin_jpeg` whose frame is the oriented one; progressive / orient: None (the
        handle's option), False or True: (ticket, the orientation applied)."""
        a = _stream_array(data)
        if status.dtype != np.int32 or status.size != 2 or not status.flags.c_contiguous:
            raise ValueError("status must be a contiguous int32 [2] array")
        t, applied = C.c_int(-1), np.ones(1, np.int32)
        self._check(self._lib.whenet_frame_begin_jpeg_oriented(self._h, _ptr(a) if a.size else None, int(a.size), BGR if bgr else RGB,
                                                               jpeg_rule_code(rule), jpeg_tristate(progressive), jpeg_tristate(orient),
                                                               C.byref(t), _ptr(status), _ptr(applied)))
        return t.value, int(applied[0])

    def clip_begin_jpeg_oriented(self, datas, status: np.ndarray, bgr: bool = True, rule=None, progressive: bool = False, orient: bool = True):
        """`whenet_clip_begin_jpeg_oriented`: `clip_begin_jpeg` whose frames are the oriented ones: (ticket, the orientations int32 [F])."""
        arrs, ptrs, sizes = _clip_streams(datas)
        if status.dtype != np.int32 or status.size != 2 * len(arrs) or not status.flags.c_contiguous:
            raise ValueError("status must be a contiguous int32 [F,2] array")
        t, applied = C.c_int(-1), np.ones(max(len(arrs), 1), np.int32)
        self._check(self._lib.whenet_clip_begin_jpeg_oriented(self._h, ptrs, _ptr(sizes) if sizes.size else None, len(arrs),
                                                              BGR if bgr else RGB, jpeg_rule_code(rule), int(bool(progressive)),
                                                              int(bool(orient)), C.byref(t), _ptr(status) if status.size else None,
                                                              _ptr(applied)))
        return t.value, applied[:len(arrs)]

    # ---- the accept bits (JPEG DECODER, LAYOUTS): `accept` None = the handle's options (single streams only) ----
    def op_jpeg_decode_accept(self, data, surface: SurfaceC, bgr: bool, entropy: int = -1, seg_bytes: int = 128, rule=None, accept=None,
                              orient=False):
        """`whenet_op_jpeg_decode_accept`: `op_jpeg_decode_oriented` with the accept bits: (status, statistics, the orientation applied)."""
        a = _stream_array(data)
        status, stats, applied = np.zeros(2, np.int32), np.zeros(8, np.int64), np.ones(1, np.int32)
        self._check(self._lib.whenet_op_jpeg_decode_accept(self._h, _ptr(a) if a.size else None, int(a.size), C.byref(surface),
                                                           BGR if bgr else RGB, int(entropy), int(seg_bytes), jpeg_rule_code(rule),
                                                           -1 if accept is None else int(accept), jpeg_tristate(orient), _ptr(status),
                                                           _ptr(stats), _ptr(applied)))
        return status, stats, int(applied[0])

    def op_jpeg_decode_clip_accept(self, datas, surfaces, bgr: bool, entropy: int = -1, seg_bytes: int = 128, rule=None, accept: int = 0,
                                   orient: bool = False):
        """`whenet_op_jpeg_decode_clip_accept`: (the status words int32 [F,2], the orientation applied to each frame int32 [F])."""
        arrs, ptrs, sizes = _clip_streams(datas)
        surf = (SurfaceC * max(len(surfaces), 1))(*surfaces)
        status, applied = np.zeros((len(arrs), 2), np.int32), np.ones(max(len(arrs), 1), np.int32)
        self._check(self._lib.whenet_op_jpeg_decode_clip_accept(self._h, ptrs, _ptr(sizes) if sizes.size else None, len(arrs), surf,
                                                                BGR if bgr else RGB, _ptr(status) if status.size else None, int(entropy),
                                                                int(seg_bytes), jpeg_rule_code(rule), int(accept), int(bool(orient)),
                                                                _ptr(applied)))
        return status, applied[:len(arrs)]

    def frame_begin_jpeg_accept(self, data, status: np.ndarray, bgr: bool = True, rule=None, accept=None, orient=False):
        """`whenet_frame_begin_jpeg_accept`: `frame_begin_jpeg_oriented` with the accept bits: (ticket, the orientation applied)."""
        a = _stream_array(data)
        if status.dtype != np.int32 or status.size != 2 or not status.flags.c_contiguous:
            raise ValueError("status must be a contiguous int32 [2] array")
        t, applied = C.c_int(-1), np.ones(1, np.int32)
        self._check(self._lib.whenet_frame_begin_jpeg_accept(self._h, _ptr(a) if a.size else None, int(a.size), BGR if bgr else RGB,
                                                             jpeg_rule_code(rule), -1 if accept is None else int(accept),
                                                             jpeg_tristate(orient), C.byref(t), _ptr(status), _ptr(applied)))
        return t.value, int(applied[0])

    def clip_begin_jpeg_accept(self, datas, status: np.ndarray, bgr: bool = True, rule=None, accept: int = 0, orient: bool = False):
        """`whenet_clip_begin_jpeg_accept`: `clip_begin_jpeg_oriented` with the accept bits: (ticket, the orientations int32 [F])."""
        arrs, ptrs, sizes = _clip_streams(datas)
        if status.dtype != np.int32 or status.size != 2 * len(arrs) or not status.flags.c_contiguous:
            raise ValueError("status must be a contiguous int32 [F,2] array")
        t, applied = C.c_int(-1), np.ones(max(len(arrs), 1), np.int32)
        self._check(self._lib.whenet_clip_begin_jpeg_accept(self._h, ptrs, _ptr(sizes) if sizes.size else None, len(arrs),
                                                            BGR if bgr else RGB, jpeg_rule_code(rule), int(accept), int(bool(orient)),
                                                            C.byref(t), _ptr(status) if status.size else None, _ptr(applied)))
        return t.value, applied[:len(arrs)]

    def jpeg_clip_counters(self) -> dict:
        """`whenet_jpeg_clip_counters`: host-side counts over the handle's engines: {"clips", "frames", "enqueues" (kernel launches plus
        memsets), "h2d"}."""
        out = (C.c_int64 * 4)()
        self._check(self._lib.whenet_jpeg_clip_counters(self._h, C.byref(out)))
        return {"clips": int(out[0]), "frames": int(out[1]), "enqueues": int(out[2]), "h2d": int(out[3])}

    def frame_annotate(self, ticket: int, frame_index: int, surface: SurfaceC, stream=None, display: int = DISPLAY_SIMPLE) -> None:
        """`whenet_frame_annotate_ex`: enqueue the annotated frame of a ticket whose heads are enqueued.  A host surface is complete
        when the ticket's collect call returns: the caller keeps its memory alive until then."""
        self._check(self._lib.whenet_frame_annotate_ex(self._h, int(ticket), int(frame_index), C.byref(surface), _stream(stream), int(display)))

    def collect(self, ticket: int, n: int, want_logits: bool = False):
        ypr = np.empty((n, 3), np.float32)
        am = np.empty((n, 3), np.int32)
        lg = np.empty((n, 252), np.float32) if want_logits else None
        self._check(self._lib.whenet_collect(self._h, ticket, _ptr(ypr), _ptr(am), _ptr(lg)))
        return ypr, am, lg

    # ---- misc -------------------------------------------------------------------------
    def set_option(self, key: str, value: int):
        self._check(self._lib.whenet_set_option(self._h, key.encode(), int(value)))
        if key == "detector_dtype":
            self._detector_dtype = int(value)

    def info(self) -> Info:
        out = Info()
        self._check(self._lib.whenet_get_info(self._h, C.byref(out)))
        return out

    def profile(self, d_crops: int, n: int, iters: int = 10):
        cap = 128
        arr = (LaunchStat * cap)()
        cnt = C.c_int(0)
        self._check(self._lib.whenet_profile(self._h, d_crops, n, iters, arr, cap, C.byref(cnt)))
        out = []
        for i in range(min(cnt.value, cap)):
            s = arr[i]
            out.append({"layer": s.layer.decode(), "kind": s.kind.decode(), "kernel": s.kernel.decode(),
                        "avg_us": s.avg_us, "alg_bytes": s.alg_bytes, "alg_flops": s.alg_flops,
                        "crops": int(s.crops), "chains": int(s.chains)})
        return out

    def device_alloc(self, nbytes: int) -> int:
        p = _P()
        self._check(self._lib.whenet_device_alloc(self._h, nbytes, C.byref(p)))
        return p.value

    def device_free(self, ptr: int):
        self._check(self._lib.whenet_device_free(self._h, ptr))

    def h2d(self, d_ptr: int, a: np.ndarray):
        a = np.ascontiguousarray(a)
        self._check(self._lib.whenet_memcpy_h2d(self._h, d_ptr, _ptr(a), a.nbytes))

    def d2h(self, a: np.ndarray, d_ptr: int):
        self._check(self._lib.whenet_memcpy_d2h(self._h, _ptr(a), d_ptr, a.nbytes))

    # ---- single-stage entry points (tests) ----------------------------------------------
    def op_stem(self, crops: np.ndarray) -> np.ndarray:
        n = crops.shape[0]
        out = np.empty((n, 112, 112, 32), np.float32)
        self._check(self._lib.whenet_op_stem(self._h, _ptr(crops), n, _ptr(out)))
        return out

    def op_block(self, index: int, x: np.ndarray):
        from . import spec
        b = spec.blocks()[index - 1]
        x = np.ascontiguousarray(x, np.float32)
        n = x.shape[0]
        assert x.shape[1:] == (b.h_in, b.h_in, b.cin), (x.shape, b)
        ex = np.empty((n, b.h_in, b.h_in, b.cexp), np.float32) if b.has_expand else None
        dw = np.empty((n, b.h_out, b.h_out, b.cexp), np.float32)
        gate = np.empty((n, b.cexp), np.float32)
        out = np.empty((n, b.h_out, b.h_out, b.cout), np.float32)
        self._check(self._lib.whenet_op_block(self._h, index, _ptr(x), n, _ptr(ex), _ptr(dw), _ptr(gate), _ptr(out)))
        return {"expand": ex, "dw": dw, "gate": gate, "out": out}

    def op_block_range(self, first: int, last: int, x: np.ndarray) -> np.ndarray:
        """Blocks first..last as the forward pass chains them (with option fold12 when the range holds 1 and 2)."""
        from . import spec
        bi, bo = spec.blocks()[first - 1], spec.blocks()[last - 1]
        x = np.ascontiguousarray(x, np.float32)
        n = x.shape[0]
        assert x.shape[1:] == (bi.h_in, bi.h_in, bi.cin), (x.shape, bi)
        out = np.empty((n, bo.h_out, bo.h_out, bo.cout), np.float32)
        self._check(self._lib.whenet_op_block_range(self._h, first, last, _ptr(x), n, _ptr(out)))
        return out

    def op_head(self, x: np.ndarray):
        x = np.ascontiguousarray(x, np.float32)
        n = x.shape[0]
        assert x.shape[1:] == (7, 7, 320)
        feat = np.empty((n, 1280), np.float32)
        lg = np.empty((n, 252), np.float32)
        ypr = np.empty((n, 3), np.float32)
        am = np.empty((n, 3), np.int32)
        self._check(self._lib.whenet_op_head(self._h, _ptr(x), n, _ptr(feat), _ptr(lg), _ptr(ypr), _ptr(am)))
        return {"feat": feat, "logits": lg, "ypr": ypr, "argmax": am}

    def op_decode(self, logits: np.ndarray):
        lg = np.ascontiguousarray(logits, np.float32)
        n = lg.shape[0]
        ypr = np.empty((n, 3), np.float32)
        am = np.empty((n, 3), np.int32)
        self._check(self._lib.whenet_op_decode(self._h, _ptr(lg), n, _ptr(ypr), _ptr(am)))
        return ypr, am


def block_spec(index: int):
    lib = load()
    out = (C.c_int32 * 8)()
    rc = lib.whenet_block_spec(index, C.byref(out))
    if rc != OK:
        raise_for(rc, f"whenet_block_spec({index})")
    return tuple(out)


def dw_plan(dtype: int, index: int) -> dict:
    lib = load()
    out = (C.c_int32 * 12)()
    rc = lib.whenet_dw_plan(dtype, index, C.byref(out))
    if rc != OK:
        raise_for(rc, f"whenet_dw_plan({dtype},{index})")
    keys = ("threads", "CV", "TH", "NSX", "tiles_x", "tiles_y", "chunks", "IH", "IW", "lds_bytes", "pad", "C")
    return dict(zip(keys, out))


def front_plan(dtype: int, index: int) -> dict:
    lib = load()
    out = (C.c_int32 * 12)()
    rc = lib.whenet_front_plan(dtype, index, C.byref(out))
    if rc != OK:
        raise_for(rc, f"whenet_front_plan({dtype},{index})")
    keys = ("threads", "CC", "TH", "NSX", "tiles_x", "tiles_y", "chunks", "EH", "EW", "lds_bytes", "w_off", "C")
    return dict(zip(keys, out))


DETECTOR_SPEC_KEYS = ("op", "k", "stride", "cin", "cout", "bn", "leaky", "src0", "src1", "skip", "is_output", "cin0")


def detector_spec(kind: int, anchors_per_scale: int = 3, num_classes: int = 1):
    """The detector body's layer table as the engine builds it (pure host logic, no GPU): a list of dicts, one per convolution
    or pool in the reference's layer-creation order (kind 0 = yolo_body, 1 = tiny_yolo_body)."""
    lib = load()
    count = C.c_int(0)
    raise_for(lib.whenet_detector_spec(int(kind), int(anchors_per_scale), int(num_classes), 0, None, C.byref(count)),
              f"whenet_detector_spec(kind={kind}, anchors_per_scale={anchors_per_scale}, num_classes={num_classes}): kind 0 / 1, both counts >= 1")
    rows = []
    out = (C.c_int32 * 12)()
    for i in range(count.value):
        raise_for(lib.whenet_detector_spec(int(kind), int(anchors_per_scale), int(num_classes), i, C.byref(out), None),
                  "whenet_detector_spec: bad arguments")
        rows.append(dict(zip(DETECTOR_SPEC_KEYS, (int(v) for v in out))))
    return rows
