"""fanlin-rs_amd -- host-side mirror of the fanlin-rs image hot path over the MI355X C ABI.

The directory name follows the reference (``fanlin-rs``) and is not a valid Python
identifier; load it with :func:`importlib` under the name ``fanlin_rs_amd`` (see
``tests/conftest.py`` / ``__graft_entry__.py``).

Everything here is plumbing over ``libfanlin_gpu.so`` (``include/fanlin_gpu.h``):

* :class:`Query`  mirrors ``query::Query`` (reference ``src/query.rs:3-94``),
* :class:`Format` mirrors ``content::Format`` (``src/content.rs:12-48``),
* :class:`State`  mirrors the pixel part of ``handler::State::process_image``
  (``src/handler.rs:185-309``): same parameter meaning, same order of operations,
  errors surface as :class:`FanlinError` exactly where the reference returns ``Err``.

There is no CPU fallback: if the shared library is missing or no HIP device is
present, construction fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FLGPU_LIB") or os.path.join(_HERE, "libfanlin_gpu.so")

FE_NONE, FE_JFIF444, FE_WEBP420, FE_JPEG, FE_PNG = 0, 1, 2, 3, 4
FE_WEBP_LOSSLESS = 6  # (5 is not a front end)
FE_WEBP_LOSSY = 9  # (7 and 8 are not front ends)
FE_WEBP_LOSSY_I4 = 10  # FE_WEBP_LOSSY whose macroblocks may be B_PRED (sixteen 4x4 sub-block predictors)
FE_WEBP_LOSSY_AP = 12  # FE_WEBP_LOSSY with per-picture coefficient probabilities (11 is not a front end)
FE_WEBP_LOSSY_I4_AP = 13  # FE_WEBP_LOSSY_I4 with per-picture coefficient probabilities
# the loop-filtered twin of each of the four: the frame header's loop filter level is picked on the device (14 and 15 are not front ends)
FE_WEBP_LOSSY_LF, FE_WEBP_LOSSY_I4_LF, FE_WEBP_LOSSY_AP_LF, FE_WEBP_LOSSY_I4_AP_LF = 16, 17, 18, 19
FE_WEBP_LOSSY_ALL = (9, 10, 12, 13, 16, 17, 18, 19)
ACCEPT_WEBP, ACCEPT_AVIF = 1, 2
ENCODE_PNG = 0x100  # accept_flags bit, not a content::Format bit: finish image/png bodies on the device (FE_PNG)
DECODE_PNG_INFLATE = 0x100000  # accept_flags bit, not a content::Format bit: State.process_png has the deflate stream inflated on the device
DECODE_PNG_ADAM7 = 0x10000  # accept_flags bit, not a content::Format bit: State.process_png also takes Adam7-interlaced files
ENCODE_WEBP_LOSSLESS = 0x200  # accept_flags bit: finish lossless image/webp bodies (q == 100) on the device (FE_WEBP_LOSSLESS)
ENCODE_WEBP_LOSSY = 0x800  # accept_flags bit: finish lossy image/webp bodies (q < 100) on the device (FE_WEBP_LOSSY)
ENCODE_WEBP_LOSSY_I4 = 0x1000  # accept_flags bit: with ENCODE_WEBP_LOSSY, those bodies come from FE_WEBP_LOSSY_I4; alone it does nothing
ENCODE_WEBP_LOSSY_FILTER = 0x4000  # accept_flags bit: with ENCODE_WEBP_LOSSY, the loop-filtered twin of whatever the other bits select; alone, or without it, nothing
ENCODE_WEBP_LOSSY_ALPHA = 0x20000  # accept_flags bit: with ENCODE_WEBP_LOSSY, a translucent picture's alpha plane goes out as a VP8L stream wherever that is smaller (FEO_ALPHA_VP8L); alone, or without it, nothing
ENCODE_WEBP_LOSSY_SEGMENTS = 0x40000  # accept_flags bit: with ENCODE_WEBP_LOSSY, segment-adaptive quantisers -- up to four classes of macroblocks by activity (FEO_SEGMENTS); alone, or without it, nothing
ENCODE_JPEG_OPTIMIZE = 0x80000  # accept_flags bit: a JPEG that stays JPEG is coded with Huffman tables from the picture's own symbol counts (FEO_JPEG_OPTIMIZE); never a larger file, nothing else changes
ENCODE_JPEG_420 = 0x200000  # accept_flags bit: a JPEG that stays JPEG is coded with 4:2:0 chroma subsampling (FEO_JPEG_420); alone or with ENCODE_JPEG_OPTIMIZE
ENCODE_JPEG_PROGRESSIVE = 0x400000  # accept_flags bit: a JPEG that stays JPEG is written as a progressive file of five scans (FEO_JPEG_PROGRESSIVE); the same file with ENCODE_JPEG_OPTIMIZE, ignored beside ENCODE_JPEG_420
FEO_JPEG_PROGRESSIVE = 16  # the `options` byte, FE_JPEG only: see ENCODE_JPEG_PROGRESSIVE
FEO_JPEG_420 = 8  # the `options` byte, FE_JPEG only: see ENCODE_JPEG_420
FEO_JPEG_OPTIMIZE = 4  # flgpu_params.reserved[0] (the header's `options` byte), FE_JPEG only: see ENCODE_JPEG_OPTIMIZE
FEO_SEGMENTS = 2  # flgpu_params.reserved[0] (the header's `options` byte), the lossy WebP front ends only: see ENCODE_WEBP_LOSSY_SEGMENTS
FEO_ALPHA_VP8L = 1  # flgpu_params.reserved[0] (the header's `options` byte), the lossy WebP front ends only: see ENCODE_WEBP_LOSSY_ALPHA
ENCODE_WEBP_LOSSY_PROBS = 0x2000  # accept_flags bit: with ENCODE_WEBP_LOSSY (and _I4), FE_WEBP_LOSSY_AP (FE_WEBP_LOSSY_I4_AP); alone, or with only _I4, nothing
OUT_KEEP, OUT_WEBP, OUT_AVIF = 0, 1, 2
ENCODE_GIF_QUANTIZE = 0x8000  # accept_flags bit: with ENCODE_GIF, a frame above 256 colours is quantised on the device (the library's own rule) and the file is finished; alone, nothing
ENCODE_GIF = 0x400  # accept_flags bit: State.process_gif finishes the image/gif body on the device where every frame has at most 256 colours
IN_OTHER, IN_JPEG, IN_PNG, IN_WEBP, IN_GIF_FRAME = 0, 1, 2, 3, 4
RESULT_AS_IS, RESULT_JPEG_STREAM, RESULT_WEBP_PLANES, RESULT_PIXELS, RESULT_PNG_STREAM, RESULT_WEBP_STREAM = 0, 1, 2, 3, 4, 5
RESULT_GIF_STREAM = 6  # process_gif with ENCODE_GIF only: one file from all the frames, not a per-picture front end
GIF_SEG_INDICES = 2048  # csrc/fl_gif.h kGifSegIndices: indices per independently coded LZW segment


def gif_max_frame_bytes(pixels: int) -> int:
    """csrc/fl_gif.h gif_max_frame_bytes: control extension 8 + descriptor 10 + table 768 + code size 1 + the data (a clear code,
    one code per index, every segment's closing code, all at 12 bits) in sub-blocks of 255 + the terminator."""
    d = (12 * (pixels + 1 + (pixels + GIF_SEG_INDICES - 1) // GIF_SEG_INDICES) + 7) // 8
    return 8 + 10 + 768 + 1 + d + (d + 254) // 255 + 1
_RESULT_FE = {RESULT_JPEG_STREAM: FE_JPEG, RESULT_WEBP_PLANES: FE_WEBP420, RESULT_PIXELS: FE_NONE, RESULT_PNG_STREAM: FE_PNG,
              RESULT_WEBP_STREAM: FE_WEBP_LOSSLESS}  # (or FE_WEBP_LOSSY, by the clamped quality: result_front_end; both are streams)
MIME = {IN_JPEG: "image/jpeg", IN_PNG: "image/png", IN_WEBP: "image/webp", IN_GIF_FRAME: "image/gif"}
IMG_FRONTEND_PLANES, IMG_HAS_ALPHA, IMG_ENCODED, IMG_PINNED, IMG_JPEG_SOURCE, IMG_PNG_SOURCE, IMG_WEBP_SOURCE = 1, 2, 4, 8, 16, 32, 64
IMG_VP8_SOURCE = 128
IMG_PNG_INFLATE = 512  # beside IMG_PNG_SOURCE: the deflate stream is inflated on the device, the compressed payload crosses PCIe
IMG_PNG_ADAM7 = 256  # beside IMG_PNG_SOURCE: the caller also hands in Adam7-interlaced PNG files
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
BATCH_SAME_PARAMS = 1
(OK, ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_NO_DEVICE, ERR_OOM, ERR_DEVICE, ERR_PARSE, ERR_BUFFER_TOO_SMALL,
 ERR_SHUTDOWN) = range(9)


class FanlinError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"flgpu status {status}: {message}")
        self.status = status


class flgpu_image(C.Structure):
    _fields_ = [("data", C.c_void_p), ("capacity", C.c_uint64), ("width", C.c_uint32), ("height", C.c_uint32),
                ("channels", C.c_uint32), ("flags", C.c_uint32), ("bytes", C.c_uint64)]


class flgpu_query(C.Structure):
    _fields_ = [(n, C.c_uint8) for n in ("has_w", "has_h", "has_rgb", "has_quality", "has_crop", "has_blur",
                                          "has_grayscale", "has_inverse", "has_avif", "has_webp",
                                          "quality", "crop", "blur", "grayscale", "inverse", "avif", "webp", "reserved")] + \
               [("w", C.c_uint32), ("h", C.c_uint32), ("rgb", C.c_char * 112)]


class flgpu_params(C.Structure):
    _fields_ = [("has_dims", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32),
                ("fill_r", C.c_uint8), ("fill_g", C.c_uint8), ("fill_b", C.c_uint8), ("crop", C.c_uint8),
                ("blur_sigma", C.c_float),
                ("grayscale", C.c_uint8), ("inverse", C.c_uint8), ("quality", C.c_uint8), ("front_end", C.c_uint8),
                ("orientation", C.c_uint8), ("filter", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class flgpu_plan(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("src_w", "src_h", "mid_c", "resampled", "resized_w", "resized_h", "crop_x", "crop_y",
                                           "letterboxed", "place_x", "place_y", "out_w", "out_h", "out_c",
                                           "plane_w", "plane_h", "chroma_w", "chroma_h")] + \
               [("pixel_bytes", C.c_uint64), ("out_bytes", C.c_uint64), ("max_out_bytes", C.c_uint64)]


MAX_DEVICES = 8


class flgpu_config(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_batch", C.c_uint32), ("flush_timeout_us", C.c_uint32),
                ("profile", C.c_uint32), ("queue_lanes", C.c_uint32), ("n_devices", C.c_uint32), ("use_embedded_profile", C.c_uint32),
                ("decode_threads", C.c_uint32),
                ("devices", C.c_int32 * MAX_DEVICES)]


class flgpu_stats(C.Structure):
    _fields_ = [("images", C.c_uint64), ("batches", C.c_uint64), ("queue_flushes", C.c_uint64),
                ("tables_built", C.c_uint64), ("resample_launches", C.c_uint64), ("resample_ms", C.c_double),
                ("resample_src_bytes", C.c_uint64), ("resample_dst_bytes", C.c_uint64),
                ("generic_launches", C.c_uint64), ("blur_launches", C.c_uint64), ("blur_ms", C.c_double),
                ("frontend_launches", C.c_uint64), ("frontend_ms", C.c_double),
                ("cmyk_pixels", C.c_uint64), ("cmyk_tables_baked", C.c_uint64),
                ("jpeg_sources", C.c_uint64), ("jpeg_file_bytes", C.c_uint64), ("jpeg_upload_bytes", C.c_uint64),
                ("mfma_launches", C.c_uint64), ("jpeg_device_huffman", C.c_uint64), ("jpeg_device_huffman_retries", C.c_uint64),
                ("wtile_launches", C.c_uint64)]


class flgpu_jpeg_info(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "components", "channels", "progressive", "restart_interval",
                                           "h_max", "v_max", "exif_orientation", "supported", "adobe_transform", "has_icc_profile")]


class flgpu_png_info(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "color_type", "bit_depth", "channels", "interlaced", "has_trns", "supported")]


class flgpu_webp_info(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "channels", "has_alpha", "extended", "animated", "lossless", "exif_orientation",
                                           "transforms", "color_cache_bits", "prefix_groups", "supported")]


class flgpu_vp8_info(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "channels", "has_alpha", "extended", "animated", "exif_orientation", "supported",
                                           "version", "segmentation", "update_map", "filter_type", "filter_level", "sharpness", "partitions",
                                           "alpha_compression", "alpha_filter", "segment_quantizers", "segment_filter_levels",
                                           "coef_prob_updates", "macroblocks", "bpred_macroblocks", "skipped_macroblocks",
                                           "skipped_bpred_macroblocks", "bmodes_mask", "ymodes_mask", "uvmodes_mask", "cat6_tokens",
                                           "blob_bytes")] + [("reserved", C.c_uint32 * 3)]


class flgpu_gif_info(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "frames", "has_global_table", "interlaced_frames", "transparent_frames",
                                           "disposal_mask", "max_code_size")] + [("decoded_bytes", C.c_uint64), ("supported", C.c_uint32),
                                                                                 ("reserved", C.c_uint32)]


# every symbol include/fanlin_gpu.h declares
EXPORTED_SYMBOLS = (
    "flgpu_query_parse", "flgpu_query_dimensions", "flgpu_query_fill_color", "flgpu_query_quality",
    "flgpu_query_cropping", "flgpu_query_blur", "flgpu_query_grayscale", "flgpu_query_inverse",
    "flgpu_query_use_avif", "flgpu_query_use_webp", "flgpu_query_as_is", "flgpu_query_unsupported_scale_size",
    "flgpu_params_from_query", "flgpu_plan_output", "flgpu_process_image", "flgpu_process_image_plan", "flgpu_create", "flgpu_destroy", "flgpu_transform",
    "flgpu_transform_batch", "flgpu_transform_batch_device", "flgpu_batch_results", "flgpu_plan_shards", "flgpu_devices",
    "flgpu_cmyk_distribution", "flgpu_rccl_selftest", "flgpu_jpeg_info_of", "flgpu_decode_jpeg", "flgpu_process_jpeg", "flgpu_process_jpeg_plan",
    "flgpu_png_info_of", "flgpu_decode_png", "flgpu_process_png", "flgpu_process_png_plan", "flgpu_debug_png_scanlines",
    "flgpu_png_info_of_flags", "flgpu_decode_png_flags", "flgpu_debug_png_scanlines_flags", "flgpu_debug_png_inflate_device", "flgpu_debug_png_inflate_model",
    "flgpu_webp_info_of", "flgpu_decode_webp", "flgpu_process_webp", "flgpu_process_webp_plan", "flgpu_debug_webp_residuals",
    "flgpu_vp8_info_of", "flgpu_decode_webp_lossy", "flgpu_debug_vp8_planes", "flgpu_debug_vp8_blob", "flgpu_debug_vp8_filter_costs", "flgpu_debug_jpeg_optimize_tables", "flgpu_debug_jpeg_progressive_scans",
    "flgpu_gif_info_of", "flgpu_decode_gif", "flgpu_process_gif", "flgpu_process_gif_plan", "flgpu_debug_gif_blob", "flgpu_host_alloc", "flgpu_host_free", "flgpu_ycck_to_cmyk",
    "flgpu_set_cmyk_profile", "flgpu_cmyk_bake_available", "flgpu_set_cmyk_clut", "flgpu_get_cmyk_clut",
    "flgpu_cmyk_to_rgb", "flgpu_cmyk_to_rgb_device", "flgpu_export_tables", "flgpu_copy_tables",
    "flgpu_import_tables", "flgpu_get_stats",
    "flgpu_reset_stats", "flgpu_debug_set", "flgpu_debug_get", "flgpu_strerror", "flgpu_last_error", "flgpu_abi_version", "flgpu_build_info",
    "flgpu_debug_axis_table", "flgpu_debug_stream_schedulable", "flgpu_debug_jpeg_blob", "flgpu_debug_mfma_plan", "flgpu_debug_mfma_plan_arith", "flgpu_debug_assign_items",
)

_lib = None


def load_library() -> C.CDLL:
    """Loads libfanlin_gpu.so (built by ``__graft_entry__.build()``); raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(there is no CPU fallback)")
    # PyTorch ships its own copy of the HIP runtime (torch/lib/libamdhip64.so).  Two HIP runtimes in one
    # process cannot both own the device, so when torch is installed it must be loaded first: the
    # library's libamdhip64.so.7 dependency then binds to torch's copy and both share one runtime.
    # Without torch (e.g. under the Rust host) the system ROCm runtime is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    lib.flgpu_query_parse.argtypes = [C.c_char_p, C.POINTER(flgpu_query)]
    lib.flgpu_query_parse.restype = C.c_int
    lib.flgpu_query_dimensions.argtypes = [C.POINTER(flgpu_query), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.flgpu_query_fill_color.argtypes = [C.POINTER(flgpu_query)] + [C.POINTER(C.c_uint8)] * 3
    lib.flgpu_query_fill_color.restype = None
    lib.flgpu_query_quality.argtypes = [C.POINTER(flgpu_query)]
    lib.flgpu_query_quality.restype = C.c_uint8
    lib.flgpu_query_blur.argtypes = [C.POINTER(flgpu_query)]
    lib.flgpu_query_blur.restype = C.c_float
    for name in ("cropping", "grayscale", "inverse", "use_avif", "use_webp", "as_is", "unsupported_scale_size"):
        f = getattr(lib, "flgpu_query_" + name)
        f.argtypes = [C.POINTER(flgpu_query)]
        f.restype = C.c_int
    lib.flgpu_params_from_query.argtypes = [C.POINTER(flgpu_query), C.c_uint32, C.c_int, C.POINTER(flgpu_params), C.POINTER(C.c_int)]
    lib.flgpu_process_image.argtypes = [C.c_void_p, C.POINTER(flgpu_image), C.c_uint8, C.c_char_p, C.c_uint32, C.c_int, C.POINTER(flgpu_image),
                                        C.POINTER(flgpu_plan), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.flgpu_process_image_plan.argtypes = [C.POINTER(flgpu_image), C.c_uint8, C.c_char_p, C.c_uint32, C.c_int, C.POINTER(flgpu_plan), C.POINTER(C.c_int)]
    lib.flgpu_plan_output.argtypes = [C.POINTER(flgpu_params), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(flgpu_plan)]
    lib.flgpu_create.argtypes = [C.POINTER(flgpu_config), C.POINTER(C.c_int)]
    lib.flgpu_create.restype = C.c_void_p
    lib.flgpu_destroy.argtypes = [C.c_void_p]
    lib.flgpu_destroy.restype = None
    lib.flgpu_transform.argtypes = [C.c_void_p, C.POINTER(flgpu_image), C.POINTER(flgpu_params), C.POINTER(flgpu_image)]
    lib.flgpu_transform_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(flgpu_image), C.POINTER(flgpu_params), C.POINTER(flgpu_image)]
    lib.flgpu_transform_batch_device.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(flgpu_image), C.POINTER(flgpu_params),
                                                 C.POINTER(flgpu_image), C.c_void_p, C.c_uint32]
    lib.flgpu_host_alloc.argtypes = [C.c_void_p, C.c_uint64]
    lib.flgpu_host_alloc.restype = C.c_void_p
    lib.flgpu_host_free.argtypes = [C.c_void_p, C.c_void_p]
    lib.flgpu_host_free.restype = None
    lib.flgpu_batch_results.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(flgpu_image)]
    lib.flgpu_plan_shards.argtypes = [C.c_uint32, C.c_size_t, C.POINTER(flgpu_image), C.POINTER(flgpu_params), C.c_uint32,
                                      C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    lib.flgpu_jpeg_info_of.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(flgpu_jpeg_info)]
    lib.flgpu_decode_jpeg.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(flgpu_image)]
    lib.flgpu_process_jpeg.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint32, C.POINTER(flgpu_image), C.POINTER(flgpu_plan),
                                       C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.flgpu_process_jpeg_plan.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint32, C.POINTER(flgpu_plan), C.POINTER(C.c_int)]
    if hasattr(lib, "flgpu_png_info_of"):   # (older libraries loaded through FLGPU_LIB by the A/B tools have no PNG sources)
        lib.flgpu_png_info_of.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(flgpu_png_info)]
        lib.flgpu_decode_png.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(flgpu_image)]
        lib.flgpu_process_png.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint32, C.POINTER(flgpu_image), C.POINTER(flgpu_plan),
                                          C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.flgpu_process_png_plan.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint32, C.POINTER(flgpu_plan), C.POINTER(C.c_int)]
        lib.flgpu_debug_png_scanlines.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    if hasattr(lib, "flgpu_png_info_of_flags"):  # (Adam7-interlaced PNG sources)
        lib.flgpu_png_info_of_flags.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.POINTER(flgpu_png_info)]
        lib.flgpu_decode_png_flags.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint32, C.POINTER(flgpu_image)]
        lib.flgpu_debug_png_scanlines_flags.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    if hasattr(lib, "flgpu_debug_png_inflate_model"):  # (PNG sources whose deflate stream the device inflates)
        lib.flgpu_debug_png_inflate_device.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        lib.flgpu_debug_png_inflate_model.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    if hasattr(lib, "flgpu_webp_info_of"):  # (the same for lossless WebP sources)
        lib.flgpu_webp_info_of.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(flgpu_webp_info)]
        lib.flgpu_decode_webp.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(flgpu_image)]
        lib.flgpu_process_webp.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint32, C.POINTER(flgpu_image), C.POINTER(flgpu_plan),
                                           C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.flgpu_process_webp_plan.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint32, C.POINTER(flgpu_plan), C.POINTER(C.c_int)]
        lib.flgpu_debug_webp_residuals.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    if hasattr(lib, "flgpu_vp8_info_of"):  # (the same for lossy WebP sources)
        lib.flgpu_vp8_info_of.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(flgpu_vp8_info)]
        lib.flgpu_decode_webp_lossy.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(flgpu_image)]
        lib.flgpu_debug_vp8_blob.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        lib.flgpu_debug_vp8_planes.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    if hasattr(lib, "flgpu_debug_vp8_filter_costs"):  # (the lossy WebP encoder's loop-filtered variants)
        lib.flgpu_debug_vp8_filter_costs.argtypes = [C.c_void_p, C.POINTER(flgpu_image), C.POINTER(flgpu_params), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                                     C.POINTER(C.c_uint32)]
    if hasattr(lib, "flgpu_gif_info_of"):  # (the same for GIF files)
        lib.flgpu_gif_info_of.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(flgpu_gif_info)]
        lib.flgpu_decode_gif.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(flgpu_image), C.POINTER(C.c_uint32)]
        lib.flgpu_process_gif.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint32, C.POINTER(flgpu_image), C.POINTER(flgpu_plan),
                                          C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.flgpu_process_gif_plan.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint32, C.POINTER(flgpu_plan), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        lib.flgpu_debug_gif_blob.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.flgpu_devices.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_uint32]
    lib.flgpu_devices.restype = C.c_uint32
    lib.flgpu_cmyk_distribution.argtypes = [C.c_void_p]
    lib.flgpu_rccl_selftest.argtypes = [C.c_int, C.POINTER(C.c_uint32)]
    lib.flgpu_rccl_selftest.restype = C.c_int
    lib.flgpu_ycck_to_cmyk.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    lib.flgpu_set_cmyk_profile.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64]
    lib.flgpu_set_cmyk_clut.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.flgpu_get_cmyk_clut.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32)]
    lib.flgpu_cmyk_to_rgb.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint32]
    lib.flgpu_cmyk_to_rgb_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    lib.flgpu_export_tables.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.flgpu_copy_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.flgpu_import_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    lib.flgpu_get_stats.argtypes = [C.c_void_p, C.POINTER(flgpu_stats)]
    lib.flgpu_reset_stats.argtypes = [C.c_void_p]
    if hasattr(lib, "flgpu_debug_set"):   # (libraries of rounds 1-4, loaded through FLGPU_LIB by the A/B tools, have no such entry point)
        lib.flgpu_debug_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        lib.flgpu_debug_get.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]
    lib.flgpu_strerror.argtypes = [C.c_int]
    lib.flgpu_strerror.restype = C.c_char_p
    lib.flgpu_last_error.argtypes = [C.c_void_p]
    lib.flgpu_last_error.restype = C.c_char_p
    lib.flgpu_abi_version.restype = C.c_uint32
    lib.flgpu_build_info.restype = C.c_char_p
    lib.flgpu_debug_axis_table.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                           C.POINTER(C.c_float), C.c_uint64, C.POINTER(C.c_uint64)]
    lib.flgpu_debug_stream_schedulable.argtypes = [C.c_uint32] * 4 + [C.POINTER(C.c_uint32)]
    lib.flgpu_debug_mfma_plan.argtypes = [C.c_uint32] * 9 + [C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
    lib.flgpu_debug_mfma_plan_arith.argtypes = [C.c_uint32] * 10 + [C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
    _lib = lib
    return lib


def build_info() -> str:
    """flgpu_build_info(): which sources (hash), compiler and flags the loaded library was built from."""
    return load_library().flgpu_build_info().decode()


def source_hash() -> str:
    """The hash csrc/Makefile computes over the library's sources as they are on disk now (same file order)."""
    import hashlib
    import re
    csrc = os.path.join(_HERE, "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, re.M).group(1).split()
    hdrs = re.search(r"^HDRS\s*=\s*(.*)$", mk, re.M).group(1).split()
    h = hashlib.sha256()
    for f in srcs + hdrs + ["Makefile"]:
        h.update(open(os.path.join(csrc, f), "rb").read())
    return h.hexdigest()[:16]


def _check(status: int, ctx: Optional[int] = None) -> None:
    if status == 0:
        return
    lib = load_library()
    msg = lib.flgpu_strerror(status).decode()
    if ctx:
        detail = lib.flgpu_last_error(ctx).decode()
        if detail:
            msg += f" ({detail})"
    raise FanlinError(status, msg)


class Format:
    """content::Format (reference src/content.rs:12-48): bit 0 webp, bit 1 avif."""

    def __init__(self, flags: int = 0):
        self.flags = flags

    def accept_webp(self) -> None:
        self.flags |= ACCEPT_WEBP

    def webp_accepted(self) -> bool:
        return (self.flags & ACCEPT_WEBP) == ACCEPT_WEBP

    def accept_avif(self) -> None:
        self.flags |= ACCEPT_AVIF

    def avif_accepted(self) -> bool:
        return (self.flags & ACCEPT_AVIF) == ACCEPT_AVIF

    @classmethod
    def from_accept_header(cls, value: str) -> "Format":
        """extract_accepted_image_formats (reference src/main.rs:255-274): exact MIME items, comma separated."""
        f = cls()
        for item in value.split(","):
            if item == "image/webp":
                f.accept_webp()
            elif item == "image/avif":
                f.accept_avif()
        return f


class Query:
    """query::Query (reference src/query.rs:3-94), parsed with axum's Query extractor semantics."""

    def __init__(self, raw: flgpu_query):
        self._q = raw

    @classmethod
    def parse(cls, query_string: str) -> "Query":
        q = flgpu_query()
        _check(load_library().flgpu_query_parse(query_string.encode(), C.byref(q)))
        return cls(q)

    def fields(self) -> dict:
        """Option fields as a dict (None = absent), for comparing with the reference's `want` structs."""
        q = self._q
        return {
            "w": q.w if q.has_w else None, "h": q.h if q.has_h else None,
            "rgb": q.rgb.decode() if q.has_rgb else None,
            "quality": q.quality if q.has_quality else None, "crop": bool(q.crop) if q.has_crop else None,
            "blur": q.blur if q.has_blur else None, "grayscale": bool(q.grayscale) if q.has_grayscale else None,
            "inverse": bool(q.inverse) if q.has_inverse else None, "avif": bool(q.avif) if q.has_avif else None,
            "webp": bool(q.webp) if q.has_webp else None,
        }

    def dimensions(self) -> Optional[Tuple[int, int]]:
        w, h = C.c_uint32(), C.c_uint32()
        return (w.value, h.value) if load_library().flgpu_query_dimensions(C.byref(self._q), C.byref(w), C.byref(h)) else None

    def fill_color(self) -> Tuple[int, int, int]:
        r, g, b = C.c_uint8(), C.c_uint8(), C.c_uint8()
        load_library().flgpu_query_fill_color(C.byref(self._q), C.byref(r), C.byref(g), C.byref(b))
        return (r.value, g.value, b.value)

    def quality(self) -> int:
        return int(load_library().flgpu_query_quality(C.byref(self._q)))

    def cropping(self) -> bool:
        return bool(load_library().flgpu_query_cropping(C.byref(self._q)))

    def blur(self) -> float:
        return float(load_library().flgpu_query_blur(C.byref(self._q)))

    def grayscale(self) -> bool:
        return bool(load_library().flgpu_query_grayscale(C.byref(self._q)))

    def inverse(self) -> bool:
        return bool(load_library().flgpu_query_inverse(C.byref(self._q)))

    def use_avif(self) -> bool:
        return bool(load_library().flgpu_query_use_avif(C.byref(self._q)))

    def use_webp(self) -> bool:
        return bool(load_library().flgpu_query_use_webp(C.byref(self._q)))

    def as_is(self) -> bool:
        return bool(load_library().flgpu_query_as_is(C.byref(self._q)))

    def unsupported_scale_size(self) -> bool:
        return bool(load_library().flgpu_query_unsupported_scale_size(C.byref(self._q)))

    def to_params(self, content: Format = None, input_is_jpeg: bool = False) -> Tuple[flgpu_params, int]:
        p, fmt = flgpu_params(), C.c_int()
        _check(load_library().flgpu_params_from_query(C.byref(self._q), content.flags if content else 0,
                                                      int(input_is_jpeg), C.byref(p), C.byref(fmt)))
        return p, fmt.value


FILTER_LANCZOS3, FILTER_NEAREST = 0, 1
CMYK_GRID, CMYK_INPUT_YCCK = 17, 1


def make_params(w: Optional[int] = None, h: Optional[int] = None, fill=(32, 32, 32), crop=False, blur_sigma=0.0,
                grayscale=False, inverse=False, quality=75, front_end=FE_NONE, orientation=1, filter=FILTER_LANCZOS3,
                alpha_vp8l=False, segments=False, jpeg_optimize=False, jpeg_420=False, jpeg_progressive=False) -> flgpu_params:
    p = flgpu_params()
    p.has_dims = 1 if (w is not None and h is not None) else 0
    p.w, p.h = (w or 0), (h or 0)
    p.fill_r, p.fill_g, p.fill_b = fill
    p.crop = int(crop)
    p.blur_sigma = blur_sigma
    p.grayscale, p.inverse = int(grayscale), int(inverse)
    p.quality, p.front_end = quality, front_end
    p.orientation = orientation
    p.filter = filter
    p.reserved[0] = ((FEO_ALPHA_VP8L if alpha_vp8l else 0) | (FEO_SEGMENTS if segments else 0) | (FEO_JPEG_OPTIMIZE if jpeg_optimize else 0)
                     | (FEO_JPEG_420 if jpeg_420 else 0) | (FEO_JPEG_PROGRESSIVE if jpeg_progressive else 0))  # the options byte
    return p


def plan_output(params: flgpu_params, sw: int, sh: int, sc: int) -> flgpu_plan:
    plan = flgpu_plan()
    _check(load_library().flgpu_plan_output(C.byref(params), sw, sh, sc, C.byref(plan)))
    return plan


def rccl_selftest(device: int = 0) -> dict:
    """flgpu_rccl_selftest: the RCCL path of the CMYK table distribution, exercised with one rank on one device."""
    info = (C.c_uint32 * 4)()
    status = load_library().flgpu_rccl_selftest(device, info)
    return {"status": status, "rccl_version": info[0], "bytes_intact": info[1], "tail_untouched": bool(info[2]), "communicator_destroyed": bool(info[3])}


class Adam7Png(bytes):
    """A PNG file for State.process_batch that may be Adam7-interlaced: handed over as FLGPU_IMG_PNG_SOURCE | FLGPU_IMG_PNG_ADAM7.
    (Bare ``bytes`` holding a PNG file are a FLGPU_IMG_PNG_SOURCE alone, for which an interlaced file is ERR_UNSUPPORTED.)"""


class InflatePng(bytes):
    """A PNG file for State.process_batch whose deflate stream the device inflates: handed over as FLGPU_IMG_PNG_SOURCE |
    FLGPU_IMG_PNG_INFLATE, and with ``adam7=True`` | FLGPU_IMG_PNG_ADAM7 as well."""
    adam7 = False

    def __new__(cls, data, adam7: bool = False):
        self = super().__new__(cls, data)
        self.adam7 = bool(adam7)
        return self


class LossyWebp(bytes):
    """A lossy WebP file for State.process_batch: handed over as FLGPU_IMG_VP8_SOURCE.  (Bare ``bytes`` holding a WebP file are a
    FLGPU_IMG_WEBP_SOURCE, which takes lossless files only.)"""


@dataclass(frozen=True)
class _FileFormat:
    """One row per format a file request can have: everything the public wrappers below differ in."""
    name: str                      # flgpu_<name>_info_of
    info: type                     # ... and the struct it fills
    hidden: Tuple[str, ...] = ()   # fields of it that the info dict leaves out
    flag: int = 0                  # what a flgpu_image of the file carries
    decode: str = ""               # the decode call
    process: str = ""              # flgpu_process_<X>, flgpu_process_<X>_plan (both WebP kinds: the library goes by the chunk type)
    input_format: int = IN_OTHER   # MIME[input_format] is the MIME of a result that keeps its format
    as_is_file: bool = True        # AS_IS hands the file itself back; a JPEG gives None, as process_image does


_JPEG = _FileFormat("jpeg", flgpu_jpeg_info, (), IMG_JPEG_SOURCE, "flgpu_decode_jpeg", "flgpu_process_jpeg", IN_JPEG, as_is_file=False)
_PNG = _FileFormat("png", flgpu_png_info, (), IMG_PNG_SOURCE, "flgpu_decode_png", "flgpu_process_png", IN_PNG)
_WEBP = _FileFormat("webp", flgpu_webp_info, (), IMG_WEBP_SOURCE, "flgpu_decode_webp", "flgpu_process_webp", IN_WEBP)
_VP8 = _FileFormat("vp8", flgpu_vp8_info, ("reserved",), IMG_VP8_SOURCE, "flgpu_decode_webp_lossy", "flgpu_process_webp", IN_WEBP)
_GIF = _FileFormat("gif", flgpu_gif_info, ("reserved",), input_format=IN_GIF_FRAME)   # (no source of a batch: State.process_gif has a body of its own)


def _file_call(entry: str, head: tuple, data: bytes, src_flags: int, *args) -> int:
    """flgpu_<entry>(*head, data, len(data), *args), or -- where the source carries more than its format's flag (IMG_PNG_ADAM7) -- the
    entry point's ``_flags`` twin with ``src_flags`` behind the length."""
    lib = load_library()
    if src_flags:
        return getattr(lib, entry + "_flags")(*head, data, len(data), src_flags, *args)
    return getattr(lib, entry)(*head, data, len(data), *args)


def _file_info(fmt: _FileFormat, data: bytes, src_flags: int = 0) -> dict:
    info = fmt.info()
    _check(_file_call(f"flgpu_{fmt.name}_info_of", (), data, src_flags, C.byref(info)))
    return {n: getattr(info, n) for n, _ in fmt.info._fields_ if n not in fmt.hidden}


def _sized_call(entry: str, data: bytes, src_flags: int = 0) -> bytes:
    """A host half alone: asked for the size first (for a GIF a bound), then for the bytes."""
    used = C.c_uint64()
    _check(_file_call(entry, (), data, src_flags, None, 0, C.byref(used)))
    out = np.zeros(max(used.value, 1), np.uint8)
    _check(_file_call(entry, (), data, src_flags, out.ctypes.data, out.nbytes, C.byref(used)))
    return out[: used.value].tobytes()


def jpeg_info(data: bytes) -> dict:
    """flgpu_jpeg_info_of: header fields of a JPEG file (pure host function); raises FanlinError(ERR_PARSE) if it is none."""
    return _file_info(_JPEG, data)


def _png_flags(adam7: bool, device_inflate: bool) -> int:
    return (IMG_PNG_ADAM7 if adam7 else 0) | (IMG_PNG_INFLATE if device_inflate else 0)


def png_info(data: bytes, adam7: bool = False, device_inflate: bool = False) -> dict:
    """flgpu_png_info_of: header fields of a PNG file (pure host function); raises FanlinError(ERR_PARSE) if the container is damaged.
    ``adam7``: flgpu_png_info_of_flags with IMG_PNG_ADAM7 -- an Adam7-interlaced file of up to 8 bits per sample is supported too.
    ``device_inflate``: with IMG_PNG_INFLATE -- accepted, and reports what it reports without it."""
    return _file_info(_PNG, data, _png_flags(adam7, device_inflate))


def debug_png_inflate_model(data: bytes):
    """flgpu_debug_png_inflate_model: the host twin of the inflate kernel on a PNG file -> (scanlines, stats); stats = dict(blocks, strips,
    sync_rounds, resolve_rounds, tokens, tokens_again, max_sync_rounds, max_resolve_rounds).  FanlinError(ERR_PARSE) = the device's "no"."""
    lib = load_library()
    used, stats = C.c_uint64(), (C.c_uint32 * 8)()
    _check(lib.flgpu_debug_png_inflate_model(data, len(data), None, 0, C.byref(used), stats))
    out = np.zeros(max(used.value, 1), np.uint8)
    _check(lib.flgpu_debug_png_inflate_model(data, len(data), out.ctypes.data, out.nbytes, C.byref(used), stats))
    names = ("blocks", "strips", "sync_rounds", "resolve_rounds", "tokens", "tokens_again", "max_sync_rounds", "max_resolve_rounds")
    return out[: used.value].tobytes(), dict(zip(names, (int(v) for v in stats)))


def debug_png_scanlines(data: bytes, adam7: bool = False) -> bytes:
    """Host half of the PNG decode front end alone: the inflated IDAT stream (filtered scanlines), Adler-32 and filter bytes checked.
    ``adam7``: flgpu_debug_png_scanlines_flags with IMG_PNG_ADAM7 -- for an interlaced file the seven passes' scanlines back to back."""
    return _sized_call("flgpu_debug_png_scanlines", data, IMG_PNG_ADAM7 if adam7 else 0)


def debug_jpeg_optimize_tables(counts, fallback: bool = False) -> dict:
    """flgpu_debug_jpeg_optimize_tables: the table rule of FEO_JPEG_OPTIMIZE on the host (the code the device runs) for counts[4][256] in
    DHT order (DC luma, AC luma, DC chroma, AC chroma) -> dict(luts = uint32[4][256] of length << 16 | code, dht = the four DHT
    segments, optimized = the never-larger decision for these counts)."""
    lib = load_library()
    cnt = np.ascontiguousarray(counts, dtype=np.uint32).reshape(4, 256)
    luts, dht = np.zeros((4, 256), np.uint32), np.zeros(1108, np.uint8)
    n, on = C.c_uint32(), C.c_int()
    lib.flgpu_debug_jpeg_optimize_tables.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
    _check(lib.flgpu_debug_jpeg_optimize_tables(cnt.ctypes.data, int(bool(fallback)), luts.ctypes.data, dht.ctypes.data, C.byref(n), C.byref(on)))
    return dict(luts=luts, dht=dht[:n.value].tobytes(), optimized=bool(on.value))


def debug_jpeg_progressive_scans(coef, prefix: bytes) -> dict:
    """flgpu_debug_jpeg_progressive_scans: FEO_JPEG_PROGRESSIVE on the host in plain loops (the rules the device runs) for the quantised
    coefficients coef[3 * blocks][64] (unit = 3 * block + component, zig-zag) and the first 177 bytes of FE_JPEG's header ->
    dict(counts = uint32[6][256] in file order (DC luma, DC chroma, the AC tables of scans 2-5), file = the progressive file)."""
    lib = load_library()
    cf = np.ascontiguousarray(coef, dtype=np.int16).reshape(-1, 64)
    assert len(cf) % 3 == 0 and len(prefix) >= 177
    head = np.frombuffer(bytes(prefix[:177]), np.uint8)
    counts, n = np.zeros((6, 256), np.uint32), C.c_uint64()
    lib.flgpu_debug_jpeg_progressive_scans.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    rc = lib.flgpu_debug_jpeg_progressive_scans(cf.ctypes.data, len(cf) // 3, head.ctypes.data, counts.ctypes.data, None, 0, C.byref(n))
    if rc != ERR_BUFFER_TOO_SMALL:
        _check(rc)
    out = np.zeros(n.value, np.uint8)
    _check(lib.flgpu_debug_jpeg_progressive_scans(cf.ctypes.data, len(cf) // 3, head.ctypes.data, counts.ctypes.data, out.ctypes.data, out.size, C.byref(n)))
    return dict(counts=counts, file=out[:n.value].tobytes())


def webp_info(data: bytes) -> dict:
    """flgpu_webp_info_of: container, VP8L header, transforms and code groups of a WebP file (pure host function); raises
    FanlinError(ERR_PARSE) if the container or the headers are damaged."""
    return _file_info(_WEBP, data)


def debug_webp_residuals(data: bytes) -> bytes:
    """Host half of the lossless WebP decode front end alone: the blob that is uploaded (header, sub-images, residual picture)."""
    return _sized_call("flgpu_debug_webp_residuals", data)


def vp8_info(data: bytes) -> dict:
    """flgpu_vp8_info_of: container, frame header and -- for a supported file -- what the partitions of a lossy WebP file use (pure
    host function); raises FanlinError(ERR_PARSE) if the file is damaged or is no lossy WebP."""
    return _file_info(_VP8, data)


def debug_vp8_blob(data: bytes) -> bytes:
    """Host half of the lossy WebP decode front end alone: the blob that is uploaded (header, macroblock records, levels, ALPH plane)."""
    return _sized_call("flgpu_debug_vp8_blob", data)


def gif_info(data: bytes) -> dict:
    """flgpu_gif_info_of: canvas, frames and what the frames use, from the container and the LZW stage of a GIF file (pure host
    function); raises FanlinError(ERR_PARSE) if the file is damaged."""
    return _file_info(_GIF, data)


def debug_gif_blob(data: bytes) -> bytes:
    """Host half of the GIF decode front end alone: the blob that is uploaded (header, frame records, index bytes, palettes)."""
    return _sized_call("flgpu_debug_gif_blob", data)


def _source_info(data):
    """(header dict, source flags) of a file handed over as a source: LossyWebp and Adam7Png say what they are, PNG and WebP go by their
    signatures, anything else is a JPEG."""
    more = IMG_PNG_ADAM7 if isinstance(data, Adam7Png) else 0
    if isinstance(data, InflatePng):
        more = IMG_PNG_INFLATE | (IMG_PNG_ADAM7 if data.adam7 else 0)
    if isinstance(data, LossyWebp):
        fmt = _VP8
    elif more or bytes(data[:8]) == PNG_SIGNATURE:
        fmt = _PNG
    else:
        fmt = _WEBP if bytes(data[:4]) == b"RIFF" and bytes(data[8:12]) == b"WEBP" else _JPEG
    return _file_info(fmt, bytes(data), more), fmt.flag | more


def debug_jpeg_blob(data: bytes):
    """Host half of the JPEG decode front end: returns (header dict, quantised coefficients [block][64] zig-zag, raw blob)."""
    lib = load_library()
    lib.flgpu_debug_jpeg_blob.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    used = C.c_uint64()
    _check(lib.flgpu_debug_jpeg_blob(data, len(data), None, 0, C.byref(used)))
    blob = np.zeros(used.value, np.uint8)
    _check(lib.flgpu_debug_jpeg_blob(data, len(data), blob.ctypes.data, blob.size, C.byref(used)))
    blob = blob[: used.value]
    u32 = blob[: (blob.size // 4) * 4].view(np.uint32)
    hdr = dict(zip(("magic", "width", "height", "nc", "hmax", "vmax", "is_rgb", "nblocks", "blocks_off", "coef_off", "plane_bytes", "total_bytes"), u32[:12].tolist()))
    words = blob[hdr["blocks_off"]: hdr["blocks_off"] + 4 * hdr["nblocks"]].view(np.uint32)
    data = blob[hdr["coef_off"]:]
    out = np.zeros((hdr["nblocks"], 64), np.int16)
    HEAD = 4  # kJpegWideHead
    for b, w in enumerate(words.tolist()):
        cnt, wide, first = ((w >> 1) & 63) + 1, w & 1, (w >> 7) * 2
        head = cnt if wide else min(cnt, HEAD)
        out[b, :head] = data[first: first + 2 * head].view(np.int16)
        if cnt > head:
            out[b, head:cnt] = data[first + 2 * head: first + 2 * head + cnt - head].view(np.int8)
    return hdr, out, blob


def plan_shards(n_shards: int, shapes: Sequence[Tuple[int, int, int]], params) -> Tuple[np.ndarray, np.ndarray]:
    """flgpu_plan_shards: (shard_of[n], shard_bytes[n_shards]) for images of shapes[i] = (height, width, channels);
    ``params`` is one flgpu_params (shared) or a sequence of n.  Pure host function."""
    n = len(shapes)
    srcs = (flgpu_image * max(n, 1))(*[flgpu_image(None, shapes[i][0] * shapes[i][1] * shapes[i][2], shapes[i][1], shapes[i][0],
                                                   shapes[i][2], 0) for i in range(n)])
    if isinstance(params, flgpu_params):
        ps, flags = (flgpu_params * 1)(params), BATCH_SAME_PARAMS
    else:
        ps, flags = (flgpu_params * max(n, 1))(*params), 0
    shard_of = (C.c_uint32 * max(n, 1))()
    shard_bytes = (C.c_uint64 * n_shards)()
    _check(load_library().flgpu_plan_shards(n_shards, n, srcs, ps, flags, shard_of, shard_bytes))
    return np.array(shard_of[:n], dtype=np.uint32), np.array(shard_bytes[:], dtype=np.uint64)


def debug_axis_table(in_size: int, out_size: int, gaussian: bool = False, sigma: float = 0.0):
    """(left, count, weights) exactly as the runtime uploads them for one axis."""
    lib = load_library()
    left = (C.c_uint32 * out_size)()
    count = (C.c_uint32 * out_size)()
    ratio = max(in_size / out_size, 1.0)
    cap = int(out_size * (2 * (2.0 * sigma if gaussian else 3.0) * ratio + 4)) + 16
    w = (C.c_float * cap)()
    total = C.c_uint64()
    _check(lib.flgpu_debug_axis_table(in_size, out_size, int(gaussian), sigma, left, count, w, cap, C.byref(total)))
    return (np.array(left, dtype=np.uint32), np.array(count, dtype=np.uint32), np.array(w[: total.value], dtype=np.float32))


def debug_mfma_plan(sw: int, sh: int, channels: int, rw: int, rh: int, crop=None, packed: bool = False) -> Optional[dict]:
    """Builds and self-checks the matrix-pipe kernel's tables on the host (csrc/fl_query.cpp flgpu_debug_mfma_plan_arith); None
    if the geometry does not fit the kernel.  crop = (cx, cy, cw, ch) in resized coordinates, default the whole picture.
    packed: the tables of rounds 2-3's arithmetic (FLGPU_MFMA_ARITH=packed) instead of the full-width one."""
    lib = load_library()
    cx, cy, cw, ch = crop if crop else (0, 0, rw, rh)
    info = (C.c_uint32 * 8)()
    err = (C.c_double * 2)()
    if not lib.flgpu_debug_mfma_plan_arith(sw, sh, channels, rw, rh, cx, cy, cw, ch, 0 if packed else 1, info, err):
        return None
    keys = ("tiles", "k_blocks", "strips", "max_operands", "hs", "tail", "bad_horizontal", "bad_vertical")
    d = dict(zip(keys, (int(x) for x in info)))
    d["vertical_weight_error"], d["horizontal_weight_error"] = float(err[0]), float(err[1])
    return d


def debug_assign_items(pictures: int, strips: int, tiles: int = 11, workgroups: int = 256):
    """(job, strip, tile0, tile1, lists): the items of a uniform persistent matrix-pipe launch in launch order and, per workgroup,
    (first item, count) -- csrc/fl_batch.cpp assign_items."""
    lib = load_library()
    cap = pictures * strips * tiles
    arrs = [(C.c_uint32 * cap)() for _ in range(4)]
    lists, n = (C.c_uint32 * (2 * workgroups))(), C.c_uint32()
    lib.flgpu_debug_assign_items.argtypes = [C.c_uint32] * 5 + [C.POINTER(C.c_uint32)] * 6
    _check(lib.flgpu_debug_assign_items(pictures, strips, tiles, workgroups, cap, *arrs, lists, C.byref(n)))
    k = int(n.value)
    g = min(workgroups, pictures * strips)
    return tuple(np.array(a[:k], np.int64) for a in arrs) + (np.array(lists[:2 * g], np.int64).reshape(g, 2),)


def debug_stream_schedulable(in_size: int, out_size: int, y0: int = 0, y1: Optional[int] = None) -> Tuple[bool, int]:
    peak = C.c_uint32()
    ok = load_library().flgpu_debug_stream_schedulable(in_size, out_size, y0, out_size if y1 is None else y1, C.byref(peak))
    return bool(ok), peak.value


@dataclass
class Planes:
    """Encoder front-end output: luma plane and two chroma planes (u8)."""
    y: np.ndarray
    u: np.ndarray
    v: np.ndarray
    has_alpha: bool = False
    a: Optional[np.ndarray] = None   # WebP: the alpha plane (all 255 unless has_alpha)


def _as_image_array(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or not (1 <= a.shape[2] <= 4):
        raise ValueError("image must be HxW or HxWxC with C in 1..4, dtype uint8")
    return a


def vp8_front_end(i4: bool = False, ap: bool = False, lf: bool = False) -> int:
    """csrc/fl_vp8_variant.h vp8_front_end: the lossy WebP front end of a variant -- i4: macroblocks may be B_PRED, ap: per-picture
    coefficient probabilities, lf: a loop filter level picked on the device."""
    return (FE_WEBP_LOSSY_LF + (2 if ap else 0) if lf else FE_WEBP_LOSSY_AP if ap else FE_WEBP_LOSSY) + (1 if i4 else 0)


def vp8_variant(front_end: int) -> Optional[Tuple[bool, bool, bool]]:
    """csrc/fl_vp8_variant.h vp8_variant_of: (i4, ap, lf) of a lossy WebP front end, None for anything else."""
    for f in range(8):
        v = (bool(f & 1), bool(f & 2), bool(f & 4))
        if vp8_front_end(*v) == front_end:
            return v
    return None


def _vp8_part0_bools(i4: bool, ap: bool, seg: bool) -> Tuple[int, int]:
    """csrc/fl_vp8_core.h vp8_part0_fixed_bools, vp8_part0_mb_bools: the first partition's worst case in booleans, fixed (1126; 9574
    with ap, each of the 1056 update flags may carry 8 bits; 98 more with seg) and per macroblock (7; 117 with i4; 2 more with seg)."""
    return (29 + 1056 * 9 + 9 + 32 if ap else 29 + 1056 + 9 + 32) + (98 if seg else 0), (1 + 1 + 16 * 7 + 3 if i4 else 7) + (2 if seg else 0)


def vp8_max_mbs(i4: bool = False, ap: bool = False, seg: bool = False) -> int:
    """csrc/fl_vp8_core.h vp8_max_mbs: the most macroblocks whose worst-case first partition (7 bits a boolean) fits its 19-bit size
    field."""
    fixed, per_mb = _vp8_part0_bools(i4, ap, seg)
    return (((1 << 19) - 1) * 8 // 7 - fixed) // per_mb


def vp8_max_out_bytes(w: int, h: int, i4: bool = False, ap: bool = False, seg: bool = False) -> int:
    """csrc/fl_vp8_core.h vp8_max_out_bytes: the worst case of a lossy WebP file of that variant (the loop filter adds nothing)."""
    mbs = ((w + 15) // 16) * ((h + 15) // 16)
    fixed, per_mb = _vp8_part0_bools(i4, ap, seg)
    return 80 + w * h + (7 * (fixed + per_mb * mbs) + 7) // 8 + (7 * (384 * 19 * mbs + 256) + 7) // 8


def result_front_end(kind: int, quality: int = 100, accept_flags: int = 0, w: int = 1, h: int = 1) -> int:
    """The front end behind a result kind.  RESULT_WEBP_STREAM is the lossless coder's at (clamped) quality 100 and the lossy
    coder's below it: B_PRED macroblocks where accept_flags has ENCODE_WEBP_LOSSY_I4 and the w x h output is within that variant's
    limits; per-picture probabilities with ENCODE_WEBP_LOSSY_PROBS (without B_PRED where the output is over the limits of both
    together); the loop filter with ENCODE_WEBP_LOSSY_FILTER."""
    if kind == RESULT_WEBP_STREAM and min(max(int(quality), 1), 100) < 100:
        mbs = ((w + 15) // 16) * ((h + 15) // 16)
        ap = bool(accept_flags & ENCODE_WEBP_LOSSY_PROBS)
        i4 = bool(accept_flags & ENCODE_WEBP_LOSSY_I4) and mbs <= vp8_max_mbs(True, ap)
        return vp8_front_end(i4, ap, bool(accept_flags & ENCODE_WEBP_LOSSY_FILTER))
    return _RESULT_FE[kind]


def _split_output(buf: np.ndarray, plan: flgpu_plan, front_end: int, flags: int, nbytes: int = 0):
    if front_end == FE_NONE:
        return buf[: plan.pixel_bytes].reshape(plan.out_h, plan.out_w, plan.out_c)
    if front_end in (FE_JPEG, FE_PNG, FE_WEBP_LOSSLESS) + FE_WEBP_LOSSY_ALL:
        return buf[:nbytes].tobytes()
    ny = plan.plane_w * plan.plane_h
    nc = plan.chroma_w * plan.chroma_h
    return Planes(y=buf[:ny].reshape(plan.plane_h, plan.plane_w),
                  u=buf[ny:ny + nc].reshape(plan.chroma_h, plan.chroma_w),
                  v=buf[ny + nc:ny + 2 * nc].reshape(plan.chroma_h, plan.chroma_w),
                  has_alpha=bool(flags & IMG_HAS_ALPHA),
                  a=buf[ny + 2 * nc:2 * ny + 2 * nc].reshape(plan.plane_h, plan.plane_w) if front_end == FE_WEBP420 else None)


class State:
    """Device context + the pixel part of handler::State::process_image.

    ``process_pixels`` is the single-request entry (goes through the request-batching
    queue, like one tokio worker calling ``process_image``); ``process_batch`` runs
    many host images in one set of launches; ``process_batch_device`` takes device
    pointers (PyTorch tensors) for HBM-resident batches.
    """

    def __init__(self, device: int = -1, max_batch: int = 0, flush_timeout_us: int = 0, profile: bool = False,
                 queue_lanes: int = 0, devices: Optional[Sequence[int]] = None, use_embedded_profile: bool = False,
                 decode_threads: int = 0):
        """``devices``: two or more HIP ordinals make ONE context that shards every batch across those GPUs (an ordinal
        may repeat: two shards on one GPU); None / one entry = a single-device context."""
        lib = load_library()
        cfg = flgpu_config()
        cfg.device, cfg.max_batch, cfg.flush_timeout_us, cfg.profile = device, max_batch, flush_timeout_us, int(profile)
        cfg.queue_lanes = queue_lanes
        cfg.use_embedded_profile = int(use_embedded_profile)
        cfg.decode_threads = decode_threads  # callers that may run the host half of the JPEG decoder at once (0 = the CPUs the process may use)
        if devices:
            if len(devices) > MAX_DEVICES:
                raise ValueError("at most 8 devices")
            cfg.n_devices = len(devices)
            for k, d in enumerate(devices):
                cfg.devices[k] = d
        st = C.c_int()
        self._ctx = lib.flgpu_create(C.byref(cfg), C.byref(st))
        if not self._ctx:
            _check(st.value or 3)
        self._lib = lib

    def close(self) -> None:
        if getattr(self, "_ctx", None):
            self._lib.flgpu_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- host memory ---------------------------------------------------------
    def process_pixels(self, image: np.ndarray, params: flgpu_params, capacity: int = 0):
        img = _as_image_array(image)
        plan = plan_output(params, img.shape[1], img.shape[0], img.shape[2])
        # capacity < 0: exactly -capacity bytes (tests of the too-small path); otherwise the format's worst case, so that the
        # call fails as rarely as JpegEncoder::encode_image into a Vec does (never)
        out = np.empty(-capacity if capacity < 0 else max(int(plan.max_out_bytes), capacity, 1), dtype=np.uint8)
        src = flgpu_image(img.ctypes.data, img.nbytes, img.shape[1], img.shape[0], img.shape[2], 0)
        dst = flgpu_image(out.ctypes.data, out.nbytes, 0, 0, 0, 0)
        _check(self._lib.flgpu_transform(self._ctx, C.byref(src), C.byref(params), C.byref(dst)), self._ctx)
        return _split_output(out, plan, params.front_end, dst.flags, dst.bytes)

    def _finish(self, plan: flgpu_plan, kind, input_format: int, run):
        """The tail of every process_* call that is no AS_IS: the buffer at the plan's worst case, ``run(dst, plan, kind, out_format)`` (the
        ABI call, all four by reference), then (mime, kind, payload)."""
        out = np.empty(max(int(plan.max_out_bytes), 1), dtype=np.uint8)
        dst = flgpu_image(out.ctypes.data, out.nbytes, 0, 0, 0, 0)
        fmt = C.c_int()
        _check(run(C.byref(dst), C.byref(plan), C.byref(kind), C.byref(fmt)), self._ctx)
        mime = "image/webp" if fmt.value == OUT_WEBP else "image/avif" if fmt.value == OUT_AVIF else MIME.get(input_format, "application/octet-stream")
        return mime, kind.value, _split_output(out, plan, _RESULT_FE[kind.value], dst.flags, dst.bytes)

    def process_image(self, decoded: np.ndarray, query_string: str, content: "Format" = None, input_format: int = IN_JPEG,
                      orientation: int = 1):
        """State::process_image after the decoder (reference src/handler.rs:198-308): returns (mime, kind, payload) where
        payload is None (AS_IS), the JPEG body (bytes), WebP planes (Planes) or the pixels for a host encoder (ndarray);
        with ENCODE_PNG in the content flags a PNG input that stays PNG gives the PNG body (bytes, RESULT_PNG_STREAM); with
        ENCODE_WEBP_LOSSLESS the WebP arm at quality 100 gives the lossless WebP body (bytes, RESULT_WEBP_STREAM), with
        ENCODE_WEBP_LOSSY the arm below quality 100 the lossy one (same kind; with ENCODE_WEBP_LOSSY_I4 and / or ENCODE_WEBP_LOSSY_PROBS
        too, the file of the variant they select)."""
        img = _as_image_array(decoded)
        src = flgpu_image(img.ctypes.data, img.nbytes, img.shape[1], img.shape[0], img.shape[2], 0)
        plan, kind = flgpu_plan(), C.c_int()
        flags = content.flags if content else 0
        qs = query_string.encode()
        _check(self._lib.flgpu_process_image_plan(C.byref(src), orientation, qs, flags, input_format, C.byref(plan), C.byref(kind)))
        if kind.value == RESULT_AS_IS:
            return MIME.get(input_format, "application/octet-stream"), RESULT_AS_IS, None
        return self._finish(plan, kind, input_format, lambda *out: self._lib.flgpu_process_image(self._ctx, C.byref(src), orientation, qs, flags, input_format, *out))

    # -- file requests: one path for JPEG, PNG and both WebP kinds (the rows of _FileFormat); the public methods say what each is ----------
    def _process_file(self, fmt: _FileFormat, data: bytes, query_string: str, content: "Format"):
        plan, kind = flgpu_plan(), C.c_int()
        flags = content.flags if content else 0
        qs = query_string.encode()
        _check(getattr(self._lib, fmt.process + "_plan")(data, len(data), qs, flags, C.byref(plan), C.byref(kind)))
        if kind.value == RESULT_AS_IS:
            return MIME[fmt.input_format], RESULT_AS_IS, data if fmt.as_is_file else None
        return self._finish(plan, kind, fmt.input_format, lambda *out: getattr(self._lib, fmt.process)(self._ctx, data, len(data), qs, flags, *out))

    def _decode_file(self, fmt: _FileFormat, data: bytes, src_flags: int = 0) -> np.ndarray:
        info = _file_info(fmt, data, src_flags)
        out = np.empty((info["height"], info["width"], max(info["channels"], 1)), np.uint8)
        dst = flgpu_image(out.ctypes.data, out.nbytes, 0, 0, 0, 0)
        _check(_file_call(fmt.decode, (self._ctx,), data, src_flags, C.byref(dst)), self._ctx)
        return out

    def _process_file_pixels(self, fmt: _FileFormat, data: bytes, params: flgpu_params, shape: Optional[Tuple[int, int, int]] = None, src_flags: int = 0):
        if shape is None:
            info = _file_info(fmt, data, src_flags)
            shape = (info["height"], info["width"], max(info["channels"], 1))
        plan = plan_output(params, shape[1], shape[0], shape[2])
        out = np.empty(max(int(plan.max_out_bytes), 1), dtype=np.uint8)
        buf = C.create_string_buffer(data, len(data))
        src = flgpu_image(C.cast(buf, C.c_void_p).value, len(data), shape[1], shape[0], shape[2], fmt.flag | src_flags)
        dst = flgpu_image(out.ctypes.data, out.nbytes, 0, 0, 0, 0)
        _check(self._lib.flgpu_transform(self._ctx, C.byref(src), C.byref(params), C.byref(dst)), self._ctx)
        return _split_output(out, plan, params.front_end, dst.flags, dst.bytes)

    # -- JPEG sources: the decode front end (handler.rs:205-220) --------------------------------------------------
    def decode_jpeg(self, data: bytes) -> np.ndarray:
        """DynamicImage::from_decoder(JpegDecoder::new(..)) on the device: (h, w, 1 or 3) uint8."""
        return self._decode_file(_JPEG, data)

    def process_jpeg_pixels(self, data: bytes, params: flgpu_params):
        """process_pixels with a JPEG FILE as the source (FLGPU_IMG_JPEG_SOURCE): decode + pipeline in one device pass."""
        return self._process_file_pixels(_JPEG, data, params)

    def process_jpeg(self, data: bytes, query_string: str, content: "Format" = None):
        """State::process_image for a JPEG input from the file bytes on: (mime, kind, payload) as process_image."""
        return self._process_file(_JPEG, data, query_string, content)

    # -- PNG sources: the decode front end (handler.rs:218-220) ----------------------------------------------------
    def decode_png(self, data: bytes, adam7: bool = False, device_inflate: bool = False) -> np.ndarray:
        """DynamicImage::from_decoder(PngDecoder::new(..)) on the device: (h, w, 1..4) uint8.  ``adam7``: flgpu_decode_png_flags with
        IMG_PNG_ADAM7 -- Adam7-interlaced files are decoded too.  ``device_inflate``: with IMG_PNG_INFLATE -- the deflate stream is
        inflated on the device."""
        return self._decode_file(_PNG, data, _png_flags(adam7, device_inflate))

    def process_png_pixels(self, data: bytes, params: flgpu_params, shape: Optional[Tuple[int, int, int]] = None, adam7: bool = False,
                           device_inflate: bool = False):
        """process_pixels with a PNG FILE as the source (FLGPU_IMG_PNG_SOURCE): inflate on this thread, the rest in one device pass.
        ``shape`` = (height, width, channels) to announce instead of what flgpu_png_info_of says (tests of rejected inputs).
        ``adam7``: the source carries FLGPU_IMG_PNG_ADAM7 as well -- it may be an Adam7-interlaced file.
        ``device_inflate``: the source carries FLGPU_IMG_PNG_INFLATE -- this thread only stages the file, the device inflates it."""
        return self._process_file_pixels(_PNG, data, params, shape, _png_flags(adam7, device_inflate))

    def debug_png_inflate_device(self, data: bytes, adam7: bool = False) -> bytes:
        """flgpu_debug_png_inflate_device: the scanlines of a PNG file exactly as the inflate kernel leaves them (no host re-run: a device
        "no" raises FanlinError(ERR_PARSE))."""
        flags = _png_flags(adam7, True)
        used = C.c_uint64()
        _check(self._lib.flgpu_debug_png_inflate_device(self._ctx, data, len(data), flags, None, 0, C.byref(used)), self._ctx)
        out = np.zeros(max(used.value, 1), np.uint8)
        _check(self._lib.flgpu_debug_png_inflate_device(self._ctx, data, len(data), flags, out.ctypes.data, out.nbytes, C.byref(used)), self._ctx)
        return out[: used.value].tobytes()

    def process_png(self, data: bytes, query_string: str, content: "Format" = None):
        """State::process_image for a PNG input from the file bytes on: (mime, kind, payload) as process_image; AS_IS hands the
        file itself back.  With DECODE_PNG_ADAM7 in the content flags Adam7-interlaced files are taken too; with DECODE_PNG_INFLATE the
        deflate stream is inflated on the device."""
        return self._process_file(_PNG, data, query_string, content)

    # -- lossless WebP sources: the decode front end (handler.rs:205-220) ------------------------------------------
    def decode_webp(self, data: bytes) -> np.ndarray:
        """DynamicImage::from_decoder(WebPDecoder::new(..)) on the device: (h, w, 3 or 4) uint8; the EXIF orientation is not applied."""
        return self._decode_file(_WEBP, data)

    def process_webp_pixels(self, data: bytes, params: flgpu_params, shape: Optional[Tuple[int, int, int]] = None):
        """process_pixels with a lossless WebP FILE as the source (FLGPU_IMG_WEBP_SOURCE): entropy decode on this thread, the rest in
        one device pass.  ``shape`` = (height, width, channels) to announce instead of what flgpu_webp_info_of says."""
        return self._process_file_pixels(_WEBP, data, params, shape)

    def process_webp(self, data: bytes, query_string: str, content: "Format" = None):
        """State::process_image for a WebP input from the file bytes on: (mime, kind, payload) as process_image; AS_IS hands the
        file itself back."""
        return self._process_file(_WEBP, data, query_string, content)

    # -- lossy WebP sources: the decode front end (handler.rs:205-220) -----------------------------------------------
    def decode_webp_lossy(self, data: bytes) -> np.ndarray:
        """flgpu_decode_webp_lossy: (h, w, 3 or 4) uint8, libwebp's WebPDecodeRGB / WebPDecodeRGBA; the EXIF orientation is not applied."""
        return self._decode_file(_VP8, data)

    def process_vp8_pixels(self, data: bytes, params: flgpu_params, shape: Optional[Tuple[int, int, int]] = None):
        """process_pixels with a lossy WebP FILE as the source (FLGPU_IMG_VP8_SOURCE): boolean decoding on this thread, the rest in
        one device pass.  ``shape`` = (height, width, channels) to announce instead of what flgpu_vp8_info_of says."""
        return self._process_file_pixels(_VP8, data, params, shape)

    def debug_vp8_planes(self, data: bytes, filtered: bool = True):
        """flgpu_debug_vp8_planes: the device's (y, u, v) of a lossy WebP file, cut to the picture, before or behind the loop filter."""
        info = vp8_info(data)
        w, h = info["width"], info["height"]
        mbw, mbh = (w + 15) // 16, (h + 15) // 16
        used = C.c_uint64()
        out = np.zeros(mbw * mbh * 384, np.uint8)
        _check(self._lib.flgpu_debug_vp8_planes(self._ctx, data, len(data), int(filtered), out.ctypes.data, out.nbytes, C.byref(used)), self._ctx)
        y = out[:mbw * mbh * 256].reshape(mbh * 16, mbw * 16)
        u = out[mbw * mbh * 256:mbw * mbh * 320].reshape(mbh * 8, mbw * 8)
        v = out[mbw * mbh * 320:].reshape(mbh * 8, mbw * 8)
        return y[:h, :w].copy(), u[:(h + 1) // 2, :(w + 1) // 2].copy(), v[:(h + 1) // 2, :(w + 1) // 2].copy()

    def debug_vp8_filter_costs(self, image: np.ndarray, params: flgpu_params) -> dict:
        """flgpu_debug_vp8_filter_costs: one picture through a loop-filtered lossy WebP front end's ordinary launches -> dict(levels =
        the four candidate levels, D = their squared-error words as the device left them, chosen = the level in the frame header).
        debug_set("vp8_filter_base", v) forces the base level the candidates are made from (-1: from the quantiser)."""
        img = _as_image_array(image)
        src = flgpu_image(img.ctypes.data, img.nbytes, img.shape[1], img.shape[0], img.shape[2], 0)
        levels, costs, chosen = (C.c_uint32 * 4)(), (C.c_uint64 * 4)(), C.c_uint32()
        _check(self._lib.flgpu_debug_vp8_filter_costs(self._ctx, C.byref(src), C.byref(params), levels, costs, C.byref(chosen)), self._ctx)
        return dict(levels=list(levels), D=list(costs), chosen=int(chosen.value))

    # -- GIF files: decode, compositing and the per-frame pipeline (handler.rs:311-353) -------------------------------
    def decode_gif(self, data: bytes) -> np.ndarray:
        """GifDecoder::new(..).into_frames().collect_frames() on the device: (frames, h, w, 4) uint8, every frame the composited canvas."""
        info = gif_info(data)
        out = np.empty((max(info["frames"], 1), info["height"], info["width"], 4), np.uint8)
        dst = flgpu_image(out.ctypes.data, out.nbytes, 0, 0, 0, 0)
        frames = C.c_uint32()
        _check(self._lib.flgpu_decode_gif(self._ctx, data, len(data), C.byref(dst), C.byref(frames)), self._ctx)
        return out[: frames.value]

    def process_gif(self, data: bytes, query_string: str, content: "Format" = None):
        """process_gif from the file bytes on: (mime, kind, payload); payload is the file itself for AS_IS, else the list of the
        frames' pixels (out_h, out_w, out_c), in frame order, for the host's GIF encoder.  With ENCODE_GIF in the content flags
        and no frame above 256 colours the payload is the finished file (bytes, RESULT_GIF_STREAM); with ENCODE_GIF_QUANTIZE as well
        frames above 256 colours are quantised on the device and the payload is the file then too."""
        plan, kind, fmt, frames = flgpu_plan(), C.c_int(), C.c_int(), C.c_uint32()
        flags = content.flags if content else 0
        qs = query_string.encode()
        _check(self._lib.flgpu_process_gif_plan(data, len(data), qs, flags, C.byref(plan), C.byref(frames), C.byref(kind)))
        if kind.value == RESULT_AS_IS:
            return "image/gif", RESULT_AS_IS, data
        size = int(plan.out_bytes) * frames.value
        if kind.value == RESULT_GIF_STREAM:  # either outcome fits
            size = 64 + frames.value * int(plan.max_out_bytes)
        out = np.empty(max(size, 1), dtype=np.uint8)
        dst = flgpu_image(out.ctypes.data, out.nbytes, 0, 0, 0, 0)
        _check(self._lib.flgpu_process_gif(self._ctx, data, len(data), qs, flags, C.byref(dst), C.byref(plan), C.byref(frames), C.byref(kind),
                                           C.byref(fmt)), self._ctx)
        if kind.value == RESULT_GIF_STREAM:
            return "image/gif", kind.value, out[: int(dst.bytes)].tobytes()
        px = out[: int(plan.out_bytes) * frames.value].reshape(frames.value, plan.out_h, plan.out_w, plan.out_c)
        return "image/gif", kind.value, [px[f] for f in range(frames.value)]

    def gif_counters(self) -> dict:
        """The GIF decode front end's counters (flgpu_debug_get)."""
        return {k: self.debug_get(k) for k in ("gif_sources", "gif_frames", "gif_file_bytes", "gif_upload_bytes")}

    def gif_encode_counters(self) -> dict:
        """The GIF encoder's counters (flgpu_debug_get): files finished on the device, their bytes, files handed back as pixels."""
        return {k: self.debug_get(k) for k in ("gif_encoded", "gif_encode_fallbacks", "gif_encoded_bytes")}

    def gif_quantized_frames(self) -> int:
        """Frames above 256 colours that ENCODE_GIF_QUANTIZE gave a table on the device (flgpu_debug_get)."""
        return self.debug_get("gif_quantized_frames")

    def webp_counters(self) -> dict:
        """The lossless WebP decode front end's counters (flgpu_debug_get)."""
        return {k: self.debug_get(k) for k in ("webp_sources", "webp_file_bytes", "webp_upload_bytes")}

    def vp8_counters(self) -> dict:
        """The lossy WebP decode front end's counters (flgpu_debug_get): pictures decoded, their file bytes, what crossed PCIe for them."""
        return {k: self.debug_get(k) for k in ("vp8_sources", "vp8_file_bytes", "vp8_upload_bytes")}

    def png_counters(self) -> dict:
        """The PNG decode front end's counters (flgpu_debug_get): pictures decoded, their file bytes, what crossed PCIe for them."""
        return {k: self.debug_get(k) for k in ("png_sources", "png_file_bytes", "png_upload_bytes")}

    def process_batch(self, images: Sequence, params: Sequence[flgpu_params]) -> List:
        """images[i]: an ndarray of pixels, or `bytes` holding a JPEG, a PNG or a lossless WebP file, or a LossyWebp, or an Adam7Png, or an InflatePng (decoded by the library)."""
        n = len(images)
        srcinfo = [_source_info(a) if isinstance(a, (bytes, bytearray)) else (None, 0) for a in images]
        infos = [s[0] for s in srcinfo]
        keep = [C.create_string_buffer(bytes(a), len(a)) if infos[i] else None for i, a in enumerate(images)]
        imgs = [None if infos[i] else _as_image_array(a) for i, a in enumerate(images)]
        shapes = [(infos[i]["height"], infos[i]["width"], max(infos[i]["channels"], 1)) if infos[i] else imgs[i].shape for i in range(n)]
        plans = [plan_output(params[i], shapes[i][1], shapes[i][0], shapes[i][2]) for i in range(n)]
        outs = [np.empty(max(int(pl.max_out_bytes), 1), dtype=np.uint8) for pl in plans]
        srcs = (flgpu_image * n)(*[flgpu_image(C.cast(keep[i], C.c_void_p).value, len(images[i]), shapes[i][1], shapes[i][0], shapes[i][2], srcinfo[i][1])
                                   if infos[i] else flgpu_image(imgs[i].ctypes.data, imgs[i].nbytes, shapes[i][1], shapes[i][0], shapes[i][2], 0) for i in range(n)])
        dsts = (flgpu_image * n)(*[flgpu_image(o.ctypes.data, o.nbytes, 0, 0, 0, 0) for o in outs])
        ps = (flgpu_params * n)(*params)
        _check(self._lib.flgpu_transform_batch(self._ctx, n, srcs, ps, dsts), self._ctx)
        return [_split_output(outs[i], plans[i], params[i].front_end, dsts[i].flags, dsts[i].bytes) for i in range(n)]

    # -- device memory -------------------------------------------------------
    def process_batch_device(self, src_ptrs: Sequence[int], shapes: Sequence[Tuple[int, int, int]],
                             params, dst_ptrs: Sequence[int], dst_caps: Sequence[int], stream: int = 0) -> None:
        """Enqueues n HBM-resident images. shapes[i] = (height, width, channels). ``params`` is one
        flgpu_params (shared) or a sequence of n.  Asynchronous on ``stream`` (a hipStream_t value)."""
        n = len(src_ptrs)
        srcs = (flgpu_image * n)(*[flgpu_image(src_ptrs[i], shapes[i][0] * shapes[i][1] * shapes[i][2], shapes[i][1],
                                               shapes[i][0], shapes[i][2], 0) for i in range(n)])
        dsts = (flgpu_image * n)(*[flgpu_image(dst_ptrs[i], dst_caps[i], 0, 0, 0, 0) for i in range(n)])
        if isinstance(params, flgpu_params):
            ps, flags = (flgpu_params * 1)(params), BATCH_SAME_PARAMS
        else:
            ps, flags = (flgpu_params * n)(*params), 0
        self._keep = (srcs, dsts, ps)
        _check(self._lib.flgpu_transform_batch_device(self._ctx, n, srcs, ps, dsts, C.c_void_p(stream), flags), self._ctx)

    def batch_results(self) -> List[Tuple[int, int]]:
        """(flags, bytes) of every image of the last ``process_batch_device`` call; waits for it."""
        srcs, dsts, ps = self._keep
        _check(self._lib.flgpu_batch_results(self._ctx, len(dsts), dsts), self._ctx)
        return [(d.flags, d.bytes) for d in dsts]

    def prepared_batch(self, src_ptrs, shapes, params, dst_ptrs, dst_caps):
        """Pre-marshals a device batch so that the timed loop only pays for the C call."""
        n = len(src_ptrs)
        srcs = (flgpu_image * n)(*[flgpu_image(src_ptrs[i], shapes[i][0] * shapes[i][1] * shapes[i][2], shapes[i][1],
                                               shapes[i][0], shapes[i][2], 0) for i in range(n)])
        dsts = (flgpu_image * n)(*[flgpu_image(dst_ptrs[i], dst_caps[i], 0, 0, 0, 0) for i in range(n)])
        if isinstance(params, flgpu_params):
            ps, flags = (flgpu_params * 1)(params), BATCH_SAME_PARAMS
        else:
            ps, flags = (flgpu_params * n)(*params), 0
        ctx, lib = self._ctx, self._lib

        def run(stream: int = 0):
            _check(lib.flgpu_transform_batch_device(ctx, n, srcs, ps, dsts, C.c_void_p(stream), flags), ctx)
        run._keep = (srcs, dsts, ps)
        self._keep = run._keep   # (so that batch_results() can collect the last run of a prepared batch too)
        return run

    def ycck_to_cmyk(self, raw: np.ndarray) -> np.ndarray:
        """handler.rs:423-438 on an (..., 4) uint8 array of (Y, Cb, Cr, K) pixels; returns a converted copy."""
        a = np.ascontiguousarray(raw, dtype=np.uint8).copy()
        if a.size % 4:
            raise ValueError("expected 4 bytes per pixel")
        _check(self._lib.flgpu_ycck_to_cmyk(self._ctx, a.ctypes.data, a.size // 4), self._ctx)
        return a

    # ---- CMYK / YCCK JPEG sources (handler.rs:398-493) ----
    def set_cmyk_profile(self, icc: bytes) -> None:
        """create_cmyk_to_rgb_converter (main.rs:74-76): bakes the profile's CMYK_8 -> sRGB device-link table."""
        _check(self._lib.flgpu_set_cmyk_profile(self._ctx, icc, len(icc)), self._ctx)

    def set_cmyk_clut(self, rgb_nodes: np.ndarray) -> None:
        a = np.ascontiguousarray(rgb_nodes, dtype=np.uint16)
        if a.size != CMYK_GRID ** 4 * 3:
            raise ValueError("expected a 17^4 x 3 table")
        _check(self._lib.flgpu_set_cmyk_clut(self._ctx, CMYK_GRID, a.ctypes.data), self._ctx)

    def get_cmyk_clut(self) -> np.ndarray:
        a = np.zeros((CMYK_GRID,) * 4 + (3,), np.uint16)
        grid = C.c_uint32()
        _check(self._lib.flgpu_get_cmyk_clut(self._ctx, a.ctypes.data, a.size, C.byref(grid)), self._ctx)
        return a

    def cmyk_to_rgb(self, cmyk: np.ndarray, embedded_icc: Optional[bytes] = None, ycck: bool = False) -> np.ndarray:
        """CMYK2RGB::convert (handler.rs:490-492) on an (..., 4) uint8 array; returns (..., 3)."""
        a = np.ascontiguousarray(cmyk, dtype=np.uint8)
        if a.ndim < 1 or a.shape[-1] != 4:
            raise ValueError("expected 4 bytes per pixel")
        out = np.empty(a.shape[:-1] + (3,), np.uint8)
        n = a.size // 4
        _check(self._lib.flgpu_cmyk_to_rgb(self._ctx, a.ctypes.data, n, out.ctypes.data, embedded_icc,
                                           len(embedded_icc) if embedded_icc else 0, CMYK_INPUT_YCCK if ycck else 0), self._ctx)
        return out

    def cmyk_to_rgb_device(self, d_cmyk: int, d_rgb: int, n_pixels: int, ycck: bool = False, stream: int = 0) -> None:
        _check(self._lib.flgpu_cmyk_to_rgb_device(self._ctx, C.c_void_p(d_cmyk), C.c_void_p(d_rgb), n_pixels,
                                                  CMYK_INPUT_YCCK if ycck else 0, C.c_void_p(stream)), self._ctx)

    def cmyk_distribution(self) -> int:
        """How the configured CMYK table reached the devices of a multi-device context: 2 = RCCL broadcast, 1 = copies, 0 = n/a."""
        return int(self._lib.flgpu_cmyk_distribution(self._ctx))

    def devices(self) -> List[int]:
        buf = (C.c_int32 * MAX_DEVICES)()
        n = self._lib.flgpu_devices(self._ctx, buf, MAX_DEVICES)
        return [int(buf[k]) for k in range(n)]

    def export_tables(self) -> Tuple[int, int]:
        ptr, nbytes = C.c_void_p(), C.c_uint64()
        _check(self._lib.flgpu_export_tables(self._ctx, C.byref(ptr), C.byref(nbytes)), self._ctx)
        return int(ptr.value or 0), int(nbytes.value)

    def copy_tables(self, dst_ptr: int, capacity: int) -> int:
        """Device-to-device copy of the table blob into a caller-owned buffer; returns its size."""
        nbytes = C.c_uint64()
        _check(self._lib.flgpu_copy_tables(self._ctx, C.c_void_p(dst_ptr), capacity, C.byref(nbytes)), self._ctx)
        return int(nbytes.value)

    def import_tables(self, src_ptr: int, nbytes: int) -> None:
        _check(self._lib.flgpu_import_tables(self._ctx, C.c_void_p(src_ptr), nbytes), self._ctx)

    def stats(self) -> dict:
        s = flgpu_stats()
        _check(self._lib.flgpu_get_stats(self._ctx, C.byref(s)), self._ctx)
        return {name: getattr(s, name) for name, _ in flgpu_stats._fields_}

    def reset_stats(self) -> None:
        _check(self._lib.flgpu_reset_stats(self._ctx), self._ctx)

    # -- test / experiment switches (flgpu_debug_set: the library reads the environment only in flgpu_create) ---------------
    def debug_set(self, key: str, value: int = 1) -> None:
        """``key``: "no_mfma", "no_wtile", "mfma_arith" (1 = packed), "force_bands", "host_huffman", ... (include/fanlin_gpu.h);
        "reset" restores every default."""
        _check(self._lib.flgpu_debug_set(self._ctx, key.encode(), int(value)), self._ctx)

    def debug_get(self, key: str) -> int:
        v = C.c_int64()
        _check(self._lib.flgpu_debug_get(self._ctx, key.encode(), C.byref(v)), self._ctx)
        return int(v.value)

    def switches(self, **kw):
        """``with state.switches(no_mfma=1, force_bands=3): ...`` -- sets the switches, restores their old values on exit."""
        state = self

        class _Scope:
            def __enter__(self_inner):
                self_inner.old = {k: state.debug_get(k) for k in kw}
                for k, v in kw.items():
                    state.debug_set(k, v)
                return state

            def __exit__(self_inner, *exc):
                for k, v in self_inner.old.items():
                    state.debug_set(k, v)
                return False

        return _Scope()
