"""ctypes binding of libjpegx.so (C ABI: include/jpegx.h) -- the only road from the Python
host code to the gfx950 kernels.  No PyTorch, no fallback: if the shared library is missing
or no GPU is usable every entry point raises :class:`JpegxError`.

Layers in this module
  * ``lib()``            the raw ``ctypes.CDLL`` with argtypes set for every symbol of jpegx.h;
  * ``Device*`` helpers  thin RAII wrappers for device buffers, streams and events;
  * host conveniences    NumPy in / NumPy out wrappers of the ``jpegx_host_*`` entry points,
                         used by the reference-compatible step classes in ``pipeline/``.
"""
import ctypes
import functools
import os

import numpy as np

from . import synth  # noqa: F401  (re-export: jpegx.synth.generate_plane)

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# JPEGX_LIB_PATH: load another build of the same library (A/B measurements of compiler flags)
LIB_PATH = os.environ.get("JPEGX_LIB_PATH") or os.path.join(_PKG_ROOT, "libjpegx.so")

Q_NONE, Q_DISCARD, Q_DIVIDE, Q_QTABLE = 0, 1, 2, 3
MODE_BY_NAME = {"none": Q_NONE, "discard": Q_DISCARD, "divide": Q_DIVIDE, "qtable": Q_QTABLE}
F_PIXEL_INPUT = 1
F_CLAMP_U8 = 2
F_TUNE_F64_LANE_PER_BLOCK = 0x4
F_TUNE_DIRECT_STORE = 0x8
F_TUNE_F64_KERNEL = 0x4000
F_TUNE_NO_F64_KERNEL = 0x8000
F_TUNE_NO_NT = 0x100
F_TUNE_NO_STRIP = 0x200
F_TUNE_SKIP_EXACT = 0x400
F_TUNE_WAVE_PER_BLOCK = 0x800
F_TUNE_POOL_ROWS_LO = 0x1000
F_TUNE_POOL_ROWS_HI = 0x2000
F_TUNE_XCD_CONTIG = 0x10000
F_TUNE_NO_XCD_CONTIG = 0x20000
F_TUNE_COLUMN_UNITS = 0x40000
F_TUNE_NO_COLUMN_UNITS = 0x80000


def F_TUNE_XCD_RUN(logr):
    """JPEGX_F_TUNE_XCD_RUN: run length 2^logr strips of the XCD-private order (31 = one run per XCD)."""
    return (int(logr) & 31) << 20


OUT_F32, OUT_I16, OUT_U8 = 0, 1, 2
_OUT_DTYPES = {OUT_F32: np.float32, OUT_I16: np.int16, OUT_U8: np.uint8}
_OUT_BY_NAME = {"f32": OUT_F32, "i16": OUT_I16, "u8": OUT_U8}


class JpegxError(RuntimeError):
    """A libjpegx call failed (or the library / GPU is missing)."""


_lib = None

_c = ctypes
_vp, _int, _dbl, _uint, _sz, _pd = _c.c_void_p, _c.c_int, _c.c_double, _c.c_uint, _c.c_size_t, _c.c_ssize_t
_u32 = _c.c_uint32

# name -> argtypes; every symbol declared in include/jpegx.h (tests/test_abi.py checks the set)
SIGNATURES = {
    "jpegx_init": [_int],
    "jpegx_shutdown": [],
    "jpegx_version": [],
    "jpegx_device_count": [_c.POINTER(_int)],
    "jpegx_set_device": [_int],
    "jpegx_get_device": [_c.POINTER(_int)],
    "jpegx_device_name": [_int, _c.c_char_p, _sz],
    "jpegx_device_synchronize": [],
    "jpegx_malloc": [_c.POINTER(_vp), _sz],
    "jpegx_free": [_vp],
    "jpegx_memset": [_vp, _int, _sz, _vp],
    "jpegx_memcpy_h2d": [_vp, _vp, _sz, _vp],
    "jpegx_memcpy_d2h": [_vp, _vp, _sz, _vp],
    "jpegx_memcpy_d2d": [_vp, _vp, _sz, _vp],
    "jpegx_stream_create": [_c.POINTER(_vp)],
    "jpegx_stream_destroy": [_vp],
    "jpegx_stream_synchronize": [_vp],
    "jpegx_event_create": [_c.POINTER(_vp)],
    "jpegx_event_destroy": [_vp],
    "jpegx_event_record": [_vp, _vp],
    "jpegx_event_synchronize": [_vp],
    "jpegx_stream_wait_event": [_vp, _vp],
    "jpegx_event_elapsed_ms": [_vp, _vp, _c.POINTER(_c.c_float)],
    "jpegx_generate_plane": [_vp, _int, _int, _pd, _int, _u32, _u32, _int, _vp],
    "jpegx_forward_fused": [_vp, _int, _int, _pd, _int, _dbl, _uint, _vp, _vp],
    "jpegx_forward_fused_on": [_int, _vp, _int, _int, _pd, _int, _dbl, _uint, _vp, _vp],
    "jpegx_forward_fused_pooled": [_vp, _int, _int, _pd, _int, _int, _dbl, _uint, _vp, _vp],
    "jpegx_forward_fused_u8": [_vp, _int, _int, _pd, _int, _int, _dbl, _uint, _vp, _vp],
    "jpegx_forward_fused_planes": [_vp, _int, _int, _dbl, _uint, _vp],
    "jpegx_forward_fused_f64": [_vp, _int, _int, _pd, _int, _dbl, _uint, _vp, _vp],
    "jpegx_mean_pool_f64": [_vp, _int, _int, _int, _pd, _int, _vp, _pd, _vp],
    "jpegx_inverse_fused": [_vp, _int, _int, _int, _dbl, _uint, _vp, _pd, _int, _vp],
    "jpegx_inverse_fused_on": [_int, _vp, _int, _int, _int, _dbl, _uint, _vp, _pd, _int, _vp],
    "jpegx_inverse_fused_u8_inflated": [_vp, _int, _int, _int, _dbl, _uint, _int, _vp, _pd, _vp],
    "jpegx_dct8x8_f32": [_vp, _int, _int, _pd, _vp, _pd, _vp],
    "jpegx_idct8x8_f32": [_vp, _int, _int, _pd, _vp, _pd, _vp],
    "jpegx_dct8x8_f64": [_vp, _int, _int, _pd, _vp, _pd, _vp],
    "jpegx_idct8x8_f64": [_vp, _int, _int, _pd, _vp, _pd, _int, _vp],
    "jpegx_quantize_f64": [_vp, _int, _int, _pd, _int, _dbl, _vp, _pd, _vp],
    "jpegx_restore_f64": [_vp, _int, _int, _pd, _int, _dbl, _vp, _pd, _vp],
    "jpegx_zigzag": [_vp, _int, _int, _pd, _int, _vp, _vp],
    "jpegx_unzigzag": [_vp, _int, _int, _int, _vp, _pd, _vp],
    "jpegx_host_forward_fused": [_vp, _int, _int, _pd, _int, _dbl, _uint, _vp],
    "jpegx_host_forward_fused_f64": [_vp, _int, _int, _int, _dbl, _uint, _vp],
    "jpegx_host_inverse_fused": [_vp, _int, _int, _int, _dbl, _uint, _vp, _pd, _int],
    "jpegx_host_inverse_fused_u8_inflated": [_vp, _int, _int, _int, _dbl, _uint, _int, _vp, _pd],
    "jpegx_host_dct8x8_f64": [_vp, _int, _int, _vp],
    "jpegx_host_idct8x8_f64": [_vp, _int, _int, _vp, _int],
    "jpegx_host_quantize_f64": [_vp, _int, _int, _int, _dbl, _vp],
    "jpegx_host_restore_f64": [_vp, _int, _int, _int, _dbl, _vp],
    "jpegx_host_zigzag": [_vp, _int, _int, _int, _vp],
    "jpegx_host_unzigzag": [_vp, _int, _int, _int, _vp],
    "jpegx_host_dct8x8_f32": [_vp, _int, _int, _vp],
    "jpegx_host_idct8x8_f32": [_vp, _int, _int, _vp],
    "jpegx_set_debug_counters": [_vp],
    "jpegx_host_compress_begin": [_vp, _int, _int, _int, _pd, _int, _int, _dbl, _c.POINTER(_sz)],
    "jpegx_host_compress_finish": [_vp],
    "jpegx_host_compress_abort": [],
    "jpegx_host_pool_release": [],
    "jpegx_host_decompress_plane": [_vp, _sz, _int, _int, _int, _int, _dbl, _vp, _pd],
    "jpegx_host_decompress_plane_i64": [_vp, _sz, _int, _int, _int, _int, _dbl, _vp, _int, _int],
    "jpegx_host_entropy_decode_gpu": [_vp, _sz, _c.c_longlong, _vp],
    "jpegx_host_compress_image": [_vp, _int, _int, _int, _int, _pd, _int, _int, _dbl, _vp, _sz, _int, _vp, _vp, _c.POINTER(_sz)],
    "jpegx_host_decompress_image": [_vp, _c.POINTER(_sz), _int, _int, _int, _int, _int, _dbl, _vp, _pd, _int, _int, _int],
    "jpegx_host_compress_image_packed": [_vp, _int, _int, _int, _pd, _int, _int, _dbl, _vp, _sz, _int, _vp, _vp, _c.POINTER(_sz)],
    "jpegx_padded_shape": [_int, _int, _int, _c.POINTER(_int), _c.POINTER(_int)],
    "jpegx_pad_edges": [_vp, _int, _int, _int, _int, _int, _pd, _vp],
    "jpegx_host_compress_begin_ragged": [_vp, _int, _int, _int, _pd, _int, _int, _dbl, _c.POINTER(_sz)],
    "jpegx_host_compress_image_ragged": [_vp, _int, _int, _int, _int, _pd, _int, _int, _dbl, _vp, _sz, _int, _vp, _vp, _c.POINTER(_sz)],
    "jpegx_host_compress_image_packed_ragged": [_vp, _int, _int, _int, _pd, _int, _int, _dbl, _vp, _sz, _int, _vp, _vp, _c.POINTER(_sz)],
    "jpegx_interleave_u8": [_vp, _int, _int, _int, _pd, _vp, _pd, _vp],
    "jpegx_deinterleave_u8": [_vp, _pd, _int, _int, _int, _vp, _pd, _vp],
    "jpegx_entropy_workspace_bytes": [_c.c_longlong],
    "jpegx_entropy_sizes": [_vp, _c.c_longlong, _vp, _vp],
    "jpegx_entropy_total": [_vp, _c.POINTER(_c.c_ulonglong), _vp],
    "jpegx_entropy_block_sizes": [_vp, _c.c_longlong, _vp, _vp],
    "jpegx_entropy_emit": [_vp, _c.c_longlong, _vp, _vp, _vp],
    "jpegx_host_entropy_encode": [_vp, _c.c_longlong, _vp, _sz, _c.POINTER(_sz)],
    "jpegx_entropy_workspace_bytes_n": [_c.c_longlong, _int],
    "jpegx_entropy_sizes_n": [_vp, _c.c_longlong, _int, _vp, _vp],
    "jpegx_entropy_emit_n": [_vp, _c.c_longlong, _int, _vp, _vp, _vp],
    "jpegx_host_compress_begin_n": [_vp, _int, _int, _pd, _int, _int, _dbl, _c.POINTER(_sz)],
    "jpegx_host_entropy_decode": [_vp, _sz, _c.c_longlong, _vp],
    "jpegx_entropy_decode_workspace_bytes": [_sz, _c.c_longlong],
    "jpegx_entropy_decode": [_vp, _sz, _c.c_longlong, _vp, _vp, _int, _vp],
    "jpegx_entropy_decode_status": [_vp, _vp],
    "jpegx_batch_workspace_bytes": [_int, _int, _int],
    "jpegx_batch_max_bytes": [_int, _int, _int],
    "jpegx_batch_compress": [_vp, _int, _int, _int, _int, _pd, _int, _int, _dbl, _uint, _vp, _vp, _sz, _vp],
    "jpegx_batch_compress_status": [_vp, _int, _int, _int, _c.POINTER(_c.c_ulonglong), _vp, _vp],
    "jpegx_batch_emit": [_vp, _int, _int, _int, _vp, _sz, _vp],
    "jpegx_batch_decompress_workspace_bytes": [_sz, _int, _int, _int],
    "jpegx_batch_decompress": [_vp, _vp, _int, _int, _int, _int, _int, _dbl, _uint, _vp, _vp, _pd, _int, _vp],
    "jpegx_forward_fused_n": [_vp, _int, _int, _pd, _int, _int, _dbl, _vp, _vp],
    "jpegx_inverse_fused_n": [_vp, _int, _int, _int, _int, _dbl, _uint, _vp, _pd, _vp],
    "jpegx_dct_f64_n": [_vp, _int, _int, _pd, _int, _vp, _pd, _vp],
    "jpegx_idct_f64_n": [_vp, _int, _int, _pd, _int, _vp, _pd, _int, _vp],
    "jpegx_dct_tables_n": [_int, _vp, _vp, _vp, _vp],
    "jpegx_host_forward_fused_n": [_vp, _int, _int, _int, _int, _dbl, _vp],
    "jpegx_host_inverse_fused_n": [_vp, _int, _int, _int, _int, _dbl, _uint, _vp, _pd],
    "jpegx_host_dct_f64_n": [_vp, _int, _int, _int, _vp],
    "jpegx_host_idct_f64_n": [_vp, _int, _int, _int, _vp, _int],
    "jpegx_host_entropy_encode_n": [_vp, _c.c_longlong, _int, _vp, _sz, _c.POINTER(_sz)],
    "jpegx_host_entropy_decode_n": [_vp, _sz, _c.c_longlong, _int, _vp],
    "jpegx_entropy_decode_workspace_bytes_n": [_sz, _c.c_longlong, _int],
    "jpegx_entropy_decode_n": [_vp, _sz, _c.c_longlong, _int, _vp, _vp, _vp],
    "jpegx_entropy_decode_status_n": [_vp, _vp],
    "jpegx_host_entropy_decode_n_gpu": [_vp, _sz, _c.c_longlong, _int, _vp],
    "jpegx_host_decompress_plane_n": [_vp, _sz, _int, _int, _int, _int, _dbl, _uint, _vp, _pd],
    "jpegx_band_shape_n": [_int, _int, _int, _int, _c.POINTER(_int), _c.POINTER(_int)],
    "jpegx_band_plane_n": [_vp, _int, _int, _pd, _int, _int, _vp, _pd, _vp],
    "jpegx_host_compress_begin_band_n": [_vp, _int, _int, _int, _pd, _int, _int, _int, _dbl, _c.POINTER(_sz)],
    "jpegx_inflate_crop_u8": [_vp, _pd, _int, _int, _int, _vp, _pd, _vp],
    "jpegx_host_decompress_band_n": [_vp, _sz, _int, _int, _int, _int, _int, _dbl, _vp, _pd],
    "jpegx_host_decompress_band_i64_n": [_vp, _sz, _int, _int, _int, _int, _int, _dbl, _vp],
    "jpegx_band_planes_packed_n": [_vp, _int, _int, _int, _pd, _int, _int, _vp, _pd, _vp],
    "jpegx_inflate_crop_pack_u8": [_vp, _int, _pd, _int, _int, _int, _vp, _pd, _vp],
    "jpegx_host_compress_image_packed_n": [_vp, _int, _int, _int, _pd, _int, _int, _int, _dbl, _vp, _sz, _int, _vp, _vp, _c.POINTER(_sz)],
    "jpegx_host_decompress_image_n": [_vp, _c.POINTER(_sz), _int, _int, _int, _int, _int, _int, _dbl, _vp, _pd, _int],
    "jpegx_rgb_to_ycbcr_u8": [_vp, _pd, _int, _int, _vp, _pd, _vp],
    "jpegx_ycbcr_to_rgb_u8": [_vp, _pd, _int, _int, _vp, _pd, _vp],
    "jpegx_host_compress_image_rgb": [_vp, _int, _int, _pd, _int, _int, _dbl, _vp, _sz, _int, _vp, _vp, _c.POINTER(_sz)],
    "jpegx_host_decompress_image_rgb": [_vp, _c.POINTER(_sz), _int, _int, _int, _int, _dbl, _vp, _pd, _int, _int],
    "jpegx_host_compress_image_rgb_n": [_vp, _int, _int, _pd, _int, _int, _int, _dbl, _vp, _sz, _int, _vp, _vp, _c.POINTER(_sz)],
    "jpegx_host_decompress_image_rgb_n": [_vp, _c.POINTER(_sz), _int, _int, _int, _int, _int, _dbl, _vp, _pd],
    "jpegx_band_planes_stacked_n": [_vp, _int, _int, _int, _pd, _int, _int, _vp, _pd, _vp],
    "jpegx_inflate_crop_stacked_u8": [_vp, _int, _int, _pd, _int, _int, _int, _vp, _pd, _vp],
    "jpegx_batch_workspace_bytes_n": [_int, _int, _int, _int, _int, _int],
    "jpegx_batch_max_bytes_n": [_int, _int, _int, _int, _int],
    "jpegx_batch_compress_n": [_vp, _int, _int, _int, _pd, _int, _int, _int, _dbl, _int, _vp, _vp, _sz, _vp],
    "jpegx_batch_compress_status_n": [_vp, _int, _int, _int, _int, _int, _int, _c.POINTER(_c.c_ulonglong), _vp, _vp],
    "jpegx_batch_emit_n": [_vp, _int, _int, _int, _int, _int, _int, _vp, _sz, _vp],
    "jpegx_batch_groups_n": [_vp, _int, _int, _int, _int, _int, _int, _vp, _c.POINTER(_int)],
    "jpegx_batch_decompress_workspace_bytes_n": [_sz, _int, _int, _int, _int, _int, _int],
    "jpegx_batch_decompress_n": [_vp, _vp, _int, _int, _int, _int, _int, _int, _dbl, _int, _vp, _vp, _pd, _vp],
    "jpegx_band_planes_packed_stacked_n": [_vp, _int, _int, _int, _int, _pd, _int, _int, _int, _vp, _pd, _vp],
    "jpegx_inflate_crop_pack_stacked_u8": [_vp, _int, _int, _int, _pd, _int, _int, _int, _int, _vp, _pd, _vp],
    "jpegx_batch_group_planes_pictures_n": [_int, _int, _int, _int, _int],
    "jpegx_batch_compress_pictures_n": [_vp, _int, _int, _int, _int, _pd, _int, _int, _int, _int, _dbl, _int, _vp, _vp, _sz, _vp],
    "jpegx_batch_groups_pictures_n": [_vp, _int, _int, _int, _int, _int, _int, _int, _vp, _c.POINTER(_int)],
    "jpegx_batch_decompress_pictures_workspace_bytes_n": [_sz, _int, _int, _int, _int, _int, _int, _int],
    "jpegx_batch_decompress_pictures_n": [_vp, _vp, _int, _int, _int, _int, _int, _int, _int, _dbl, _int, _int, _vp, _vp, _pd, _vp],
    "jpegx_probe_sizes_n": [_vp, _int, _int, _int, _pd, _int, _int, _vp, _int, _vp, _vp],
    "jpegx_batch_probe_pictures_workspace_bytes_n": [_int, _int, _int, _int, _int, _int, _int],
    "jpegx_batch_probe_pictures_n": [_vp, _int, _int, _int, _int, _pd, _int, _int, _int, _int, _vp, _int, _int, _vp, _vp, _vp],
    "jpegx_band_moments_packed_stacked_n": [_vp, _int, _int, _int, _int, _pd, _int, _int, _int, _vp, _pd, _vp],
    "jpegx_probe_distortion_n": [_vp, _vp, _int, _int, _int, _pd, _pd, _int, _int, _int, _int, _int, _vp, _int, _vp, _vp],
    "jpegx_batch_probe_distortion_pictures_workspace_bytes_n": [_int, _int, _int, _int, _int, _int, _int],
    "jpegx_batch_probe_distortion_pictures_n": [_vp, _int, _int, _int, _int, _pd, _int, _int, _int, _int, _vp, _int, _int, _vp, _vp, _vp],
    "jpegx_probe_sizes_8": [_vp, _int, _int, _int, _pd, _int, _vp, _int, _vp, _vp],
    "jpegx_probe_distortion_8": [_vp, _vp, _int, _int, _int, _pd, _pd, _int, _int, _int, _int, _vp, _int, _vp, _vp],
    "jpegx_batch_probe_pictures_workspace_bytes": [_int, _int, _int, _int, _int, _int],
    "jpegx_batch_probe_pictures": [_vp, _int, _int, _int, _int, _pd, _int, _int, _int, _vp, _int, _int, _vp, _vp, _vp],
    "jpegx_batch_probe_distortion_pictures_workspace_bytes": [_int, _int, _int, _int, _int, _int],
    "jpegx_batch_probe_distortion_pictures": [_vp, _int, _int, _int, _int, _pd, _int, _int, _int, _vp, _int, _int, _vp, _vp, _vp],
    "jpegx_picture_planes_stacked_u8": [_vp, _int, _int, _int, _int, _pd, _int, _int, _vp, _pd, _vp],
    "jpegx_batch_pictures_workspace_bytes": [_int, _int, _int, _int, _int, _int],
    "jpegx_batch_compress_pictures": [_vp, _int, _int, _int, _int, _pd, _int, _int, _int, _dbl, _int, _vp, _vp, _sz, _vp],
    "jpegx_batch_decompress_pictures_workspace_bytes": [_sz, _int, _int, _int, _int, _int],
    "jpegx_batch_decompress_pictures": [_vp, _vp, _int, _int, _int, _int, _int, _int, _dbl, _int, _vp, _vp, _pd, _vp],
    "jpegx_picture_set_table_bytes": [_int],
    "jpegx_picture_set_table": [_vp, _int, _int, _int, _int, _vp, _c.POINTER(_c.c_longlong)],
    "jpegx_picture_set_blocks_n": [_vp, _vp, _vp, _int, _int, _int, _vp, _vp],
    "jpegx_picture_set_pixels_u8": [_vp, _vp, _vp, _int, _int, _int, _vp, _vp],
    "jpegx_batch_set_workspace_bytes_n": [_vp, _c.c_longlong],
    "jpegx_batch_set_max_bytes_n": [_vp],
    "jpegx_batch_compress_picture_set_n": [_vp, _vp, _vp, _int, _int, _dbl, _c.c_longlong, _vp, _vp, _sz, _vp],
    "jpegx_batch_compress_status_set_n": [_vp, _vp, _c.c_longlong, _c.POINTER(_c.c_ulonglong), _vp, _vp],
    "jpegx_batch_emit_set_n": [_vp, _vp, _vp, _c.c_longlong, _vp, _sz, _vp],
    "jpegx_batch_groups_set_n": [_vp, _vp, _c.c_longlong, _vp, _c.POINTER(_int)],
    "jpegx_batch_decompress_set_workspace_bytes_n": [_sz, _vp, _c.c_longlong],
    "jpegx_batch_decompress_picture_set_n": [_vp, _vp, _vp, _vp, _int, _dbl, _int, _c.c_longlong, _vp, _vp, _vp],
    "jpegx_probe_sizes_set_n": [_vp, _vp, _vp, _int, _int, _int, _vp, _int, _vp, _vp],
    "jpegx_batch_probe_picture_set_workspace_bytes_n": [_vp, _c.c_longlong],
    "jpegx_batch_probe_picture_set_n": [_vp, _vp, _vp, _int, _int, _vp, _int, _c.c_longlong, _vp, _vp, _vp],
    "jpegx_picture_set_moments_n": [_vp, _vp, _vp, _int, _int, _int, _vp, _vp],
    "jpegx_probe_distortion_set_n": [_vp, _vp, _vp, _vp, _int, _int, _int, _vp, _int, _vp, _vp],
    "jpegx_batch_probe_distortion_picture_set_workspace_bytes_n": [_vp, _c.c_longlong],
    "jpegx_batch_probe_distortion_picture_set_n": [_vp, _vp, _vp, _int, _int, _vp, _int, _c.c_longlong, _vp, _vp, _vp],
    "jpegx_picture_set_blocks_u8": [_vp, _vp, _vp, _int, _int, _int, _vp, _vp],
    "jpegx_batch_set_workspace_bytes": [_vp, _c.c_longlong],
    "jpegx_batch_set_max_bytes": [_vp],
    "jpegx_batch_compress_picture_set": [_vp, _vp, _vp, _int, _int, _dbl, _c.c_longlong, _vp, _vp, _sz, _vp],
    "jpegx_batch_compress_status_set": [_vp, _vp, _c.c_longlong, _c.POINTER(_c.c_ulonglong), _vp, _vp],
    "jpegx_batch_emit_set": [_vp, _vp, _vp, _c.c_longlong, _vp, _sz, _vp],
    "jpegx_batch_groups_set": [_vp, _vp, _c.c_longlong, _vp, _c.POINTER(_int)],
    "jpegx_batch_decompress_set_workspace_bytes": [_sz, _vp, _c.c_longlong],
    "jpegx_batch_decompress_picture_set": [_vp, _vp, _vp, _vp, _int, _dbl, _int, _c.c_longlong, _vp, _vp, _vp],
    "jpegx_comm_available": [],
    "jpegx_comm_unique_id": [_vp],
    "jpegx_comm_create": [_c.POINTER(_vp), _int, _int, _vp],
    "jpegx_comm_create_deadline": [_c.POINTER(_vp), _int, _int, _vp, _dbl],
    "jpegx_comm_destroy": [_vp],
    "jpegx_comm_abort": [_vp],
    "jpegx_comm_count": [_vp, _c.POINTER(_int)],
    "jpegx_comm_gather_bytes": [_vp, _vp, _sz, _vp, _c.POINTER(_sz), _c.POINTER(_sz), _int, _vp],
}
# explicit-device forms (csrc/jpegx_on.cpp): the plain signature behind a leading device index
for _name in ("jpegx_malloc", "jpegx_free", "jpegx_stream_create", "jpegx_generate_plane", "jpegx_forward_fused_pooled",
              "jpegx_forward_fused_u8", "jpegx_forward_fused_f64", "jpegx_forward_fused_planes", "jpegx_mean_pool_f64",
              "jpegx_inverse_fused_u8_inflated", "jpegx_entropy_sizes", "jpegx_entropy_total", "jpegx_entropy_block_sizes",
              "jpegx_entropy_emit", "jpegx_entropy_decode", "jpegx_entropy_decode_status", "jpegx_batch_compress",
              "jpegx_batch_compress_status", "jpegx_batch_emit", "jpegx_batch_decompress", "jpegx_host_compress_begin", "jpegx_host_compress_image", "jpegx_host_compress_image_packed", "jpegx_host_decompress_plane",
              "jpegx_host_decompress_plane_i64", "jpegx_host_decompress_image", "jpegx_host_entropy_decode_gpu",
              "jpegx_host_pool_release", "jpegx_comm_create_deadline", "jpegx_pad_edges", "jpegx_host_compress_begin_ragged",
              "jpegx_host_compress_image_ragged", "jpegx_host_compress_image_packed_ragged", "jpegx_forward_fused_n",
              "jpegx_inverse_fused_n", "jpegx_dct_f64_n", "jpegx_idct_f64_n", "jpegx_entropy_sizes_n", "jpegx_entropy_emit_n",
              "jpegx_host_compress_begin_n", "jpegx_entropy_decode_n", "jpegx_entropy_decode_status_n",
              "jpegx_host_entropy_decode_n_gpu", "jpegx_host_decompress_plane_n", "jpegx_band_shape_n", "jpegx_band_plane_n",
              "jpegx_host_compress_begin_band_n", "jpegx_inflate_crop_u8", "jpegx_host_decompress_band_n",
              "jpegx_host_decompress_band_i64_n", "jpegx_band_planes_packed_n", "jpegx_inflate_crop_pack_u8",
              "jpegx_host_compress_image_packed_n", "jpegx_host_decompress_image_n", "jpegx_rgb_to_ycbcr_u8",
              "jpegx_ycbcr_to_rgb_u8", "jpegx_host_compress_image_rgb", "jpegx_host_decompress_image_rgb",
              "jpegx_host_compress_image_rgb_n", "jpegx_host_decompress_image_rgb_n", "jpegx_band_planes_stacked_n",
              "jpegx_inflate_crop_stacked_u8", "jpegx_batch_compress_n", "jpegx_batch_compress_status_n", "jpegx_batch_emit_n",
              "jpegx_batch_decompress_n", "jpegx_band_planes_packed_stacked_n", "jpegx_inflate_crop_pack_stacked_u8",
              "jpegx_batch_compress_pictures_n", "jpegx_batch_decompress_pictures_n", "jpegx_picture_planes_stacked_u8",
              "jpegx_batch_compress_pictures", "jpegx_batch_decompress_pictures", "jpegx_picture_set_blocks_n",
              "jpegx_picture_set_pixels_u8", "jpegx_batch_compress_picture_set_n", "jpegx_batch_compress_status_set_n",
              "jpegx_batch_emit_set_n", "jpegx_batch_decompress_picture_set_n", "jpegx_picture_set_blocks_u8",
              "jpegx_batch_compress_picture_set", "jpegx_batch_compress_status_set", "jpegx_batch_emit_set",
              "jpegx_batch_decompress_picture_set", "jpegx_probe_sizes_n", "jpegx_batch_probe_pictures_n",
              "jpegx_probe_sizes_set_n", "jpegx_batch_probe_picture_set_n", "jpegx_band_moments_packed_stacked_n",
              "jpegx_probe_distortion_n", "jpegx_batch_probe_distortion_pictures_n", "jpegx_picture_set_moments_n",
              "jpegx_probe_distortion_set_n", "jpegx_batch_probe_distortion_picture_set_n", "jpegx_probe_sizes_8",
              "jpegx_probe_distortion_8", "jpegx_batch_probe_pictures", "jpegx_batch_probe_distortion_pictures"):
    SIGNATURES[_name + "_on"] = [_int] + SIGNATURES[_name]
RESTYPES = {"jpegx_entropy_workspace_bytes": _sz, "jpegx_entropy_workspace_bytes_n": _sz, "jpegx_entropy_decode_workspace_bytes": _sz, "jpegx_entropy_decode_workspace_bytes_n": _sz,
            "jpegx_batch_workspace_bytes": _sz,
            "jpegx_batch_max_bytes": _sz, "jpegx_batch_decompress_workspace_bytes": _sz, "jpegx_batch_workspace_bytes_n": _sz,
            "jpegx_batch_max_bytes_n": _sz, "jpegx_batch_decompress_workspace_bytes_n": _sz,
            "jpegx_batch_decompress_pictures_workspace_bytes_n": _sz, "jpegx_batch_pictures_workspace_bytes": _sz,
            "jpegx_batch_decompress_pictures_workspace_bytes": _sz, "jpegx_picture_set_table_bytes": _sz,
            "jpegx_batch_set_workspace_bytes_n": _sz, "jpegx_batch_set_max_bytes_n": _sz,
            "jpegx_batch_decompress_set_workspace_bytes_n": _sz, "jpegx_batch_set_workspace_bytes": _sz,
            "jpegx_batch_set_max_bytes": _sz, "jpegx_batch_decompress_set_workspace_bytes": _sz,
            "jpegx_batch_probe_pictures_workspace_bytes_n": _sz,
            "jpegx_batch_probe_distortion_pictures_workspace_bytes_n": _sz,
            "jpegx_batch_probe_picture_set_workspace_bytes_n": _sz,
            "jpegx_batch_probe_distortion_picture_set_workspace_bytes_n": _sz,
            "jpegx_batch_probe_pictures_workspace_bytes": _sz,
            "jpegx_batch_probe_distortion_pictures_workspace_bytes": _sz}   # everything else returns int


def lib():
    """Load libjpegx.so once; raise JpegxError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise JpegxError(
                "libjpegx.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` or `make -C implementing-jpeg-compression_amd/csrc` (there is no CPU fallback)"
                % LIB_PATH)
        try:
            L = ctypes.CDLL(LIB_PATH)
        except OSError as exc:  # missing libamdhip64 etc.
            raise JpegxError("cannot load %s: %s" % (LIB_PATH, exc))
        L.jpegx_last_error.restype = ctypes.c_char_p
        L.jpegx_last_error.argtypes = []
        for name, argtypes in SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = RESTYPES.get(name, ctypes.c_int)
        _lib = L
    return _lib


def check(rc, what="jpegx call"):
    if rc != 0:
        raise JpegxError("%s failed (%d): %s" % (what, rc, lib().jpegx_last_error().decode("utf-8", "replace")))


def device_count():
    n = ctypes.c_int(0)
    rc = lib().jpegx_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


def require_device():
    if device_count() < 1:
        raise JpegxError("no usable HIP device: " + lib().jpegx_last_error().decode("utf-8", "replace"))


def device_name(device=0):
    buf = ctypes.create_string_buffer(256)
    check(lib().jpegx_device_name(device, buf, 256), "jpegx_device_name")
    return buf.value.decode()


def mode_of(mode):
    if isinstance(mode, str):
        try:
            return MODE_BY_NAME[mode]
        except KeyError:
            raise JpegxError("unknown quantiser %r" % (mode,))
    return int(mode)


# ---------------------------------------------------------------------------------------------
# device-side helpers (bench.py, tests, multi-GPU driver)
# ---------------------------------------------------------------------------------------------
class DeviceBuffer:
    """hipMalloc'ed span owned by this object."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        check(lib().jpegx_malloc(ctypes.byref(p), self.nbytes), "jpegx_malloc")
        self.ptr = p.value

    def free(self):
        if self.ptr:
            lib().jpegx_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def upload(self, array, stream=None, offset=0):
        a = np.ascontiguousarray(array)
        assert offset + a.nbytes <= self.nbytes
        check(lib().jpegx_memcpy_h2d(self.ptr + offset, a.ctypes.data, a.nbytes, stream), "jpegx_memcpy_h2d")
        check(lib().jpegx_stream_synchronize(stream), "jpegx_stream_synchronize")

    def download(self, shape, dtype, stream=None, offset=0):
        out = np.empty(shape, dtype=dtype)
        assert offset + out.nbytes <= self.nbytes
        check(lib().jpegx_memcpy_d2h(out.ctypes.data, self.ptr + offset, out.nbytes, stream), "jpegx_memcpy_d2h")
        check(lib().jpegx_stream_synchronize(stream), "jpegx_stream_synchronize")
        return out


class Event:
    def __init__(self):
        p = ctypes.c_void_p()
        check(lib().jpegx_event_create(ctypes.byref(p)), "jpegx_event_create")
        self.handle = p.value

    def record(self, stream=None):
        check(lib().jpegx_event_record(self.handle, stream), "jpegx_event_record")

    def synchronize(self):
        check(lib().jpegx_event_synchronize(self.handle), "jpegx_event_synchronize")

    def elapsed_ms(self, later):
        ms = ctypes.c_float()
        check(lib().jpegx_event_elapsed_ms(self.handle, later.handle, ctypes.byref(ms)), "jpegx_event_elapsed_ms")
        return ms.value

    def __del__(self):
        try:
            if self.handle:
                lib().jpegx_event_destroy(self.handle)
        except Exception:
            pass


def generate_plane_device(ptr, height, width, kind, seed=0, plane=0, row0=0, pitch=None, stream=None):
    k = synth._KINDS[kind] if isinstance(kind, str) else int(kind)
    check(lib().jpegx_generate_plane(ptr, height, width, pitch or width, k, seed, plane, row0, stream),
          "jpegx_generate_plane")


def forward_fused_device(in_ptr, height, width, out_ptr, mode="qtable", param=0.0, flags=F_PIXEL_INPUT,
                         pitch=None, pool=1, stream=None):
    """Enqueue steps 4+5+6 on device pointers (fp32 plane -> int16 zigzag stream)."""
    check(lib().jpegx_forward_fused_pooled(in_ptr, height, width, pitch or width * pool, pool, mode_of(mode),
                                           float(param), flags, out_ptr, stream), "jpegx_forward_fused")


class PlaneDesc(ctypes.Structure):
    """struct jpegx_plane_desc (include/jpegx.h)."""
    _fields_ = [("d_in", _vp), ("d_out", _vp), ("H", _int), ("W", _int), ("pitch", _pd), ("bs", _int)]


def forward_fused_planes_device(planes, mode="qtable", param=0.0, flags=F_PIXEL_INPUT, stream=None):
    """Enqueue steps (1+)4+5+6 for several planes as ONE launch.  ``planes``: iterable of
    (in_ptr, height, width, pitch_elems, block_size, out_ptr) with height/width AFTER pooling."""
    planes = list(planes)
    arr = (PlaneDesc * len(planes))()
    for d, (in_ptr, h, w, pitch, bs, out_ptr) in zip(arr, planes):
        d.d_in, d.d_out, d.H, d.W, d.pitch, d.bs = in_ptr, out_ptr, h, w, pitch, bs
    check(lib().jpegx_forward_fused_planes(arr, len(planes), mode_of(mode), float(param), flags, stream),
          "jpegx_forward_fused_planes")


def forward_fused_u8_device(in_ptr, height, width, out_ptr, mode="qtable", param=0.0, flags=0, pitch=None,
                            pool=1, stream=None):
    """Enqueue steps (1+)4+5+6 on a uint8 device plane of (height*pool, width*pool) bytes."""
    check(lib().jpegx_forward_fused_u8(in_ptr, height, width, pitch or width * pool, pool, mode_of(mode),
                                       float(param), flags, out_ptr, stream), "jpegx_forward_fused_u8")


def u8_path_ok(width_out, pool, pitch_bytes, mode="qtable", param=0.0):
    """What the uint8 kernels accept: block_size 1 (W % 16 == 0), 2 or 4, 16-byte aligned rows, and a
    quantiser whose multiplier is at most 2 (they pack to int16 without saturating)."""
    if mode_of(mode) == Q_DIVIDE and abs(float(param)) < 0.5:
        return False
    return pool in (1, 2, 4) and pitch_bytes % 16 == 0 and (pool > 1 or width_out % 16 == 0)


def inverse_fused_device(in_ptr, height, width, out_ptr, mode="qtable", param=0.0, flags=0, out_type=OUT_F32,
                         out_pitch=None, stream=None):
    check(lib().jpegx_inverse_fused(in_ptr, height, width, mode_of(mode), float(param), flags, out_ptr,
                                    out_pitch or width, out_type, stream), "jpegx_inverse_fused")


# ---------------------------------------------------------------------------------------------
# NumPy-in / NumPy-out conveniences (synchronous; H2D + kernel + D2H inside the library)
# ---------------------------------------------------------------------------------------------
class _Buffers:
    """``with _Buffers() as dev:`` -- every ``dev(nbytes)`` inside is a DeviceBuffer that is freed when the block ends,
    however it ends; one allocated late, once a size is known, included."""

    def __enter__(self):
        self._held = []
        return self

    def __call__(self, nbytes):
        self._held.append(DeviceBuffer(nbytes))
        return self._held[-1]

    def __exit__(self, *exc):
        for b in self._held:
            b.free()


def _coded(blob):
    """Coded bytes for a native decoder: (pointer, or None for an empty string; size; the array that keeps the pointer
    alive for as long as the caller holds it)."""
    buf = np.frombuffer(bytes(blob), dtype=np.uint8)                    # bytes(b) of an exact bytes object is b itself
    return (buf.ctypes.data if buf.size else None), buf.size, buf


def _plane(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.ndim != 2:
        raise JpegxError("expected a 2-D plane, got shape %r" % (a.shape,))
    return a


def is_pixel_like(a, block_size=1):
    """True when the plane keeps the promise of JPEGX_F_PIXEL_INPUT (include/jpegx.h): every sample a non-negative
    multiple of 2^-8, at most 255; for a plane that is mean-pooled on load (block_size 2, 4): every sample an integer
    0 .. 255."""
    a = np.asarray(a)
    if a.size == 0:
        return False
    if a.dtype.kind in "ui":
        return bool(a.min() >= 0 and a.max() <= 255)
    s = a * 256.0 if int(block_size) == 1 else a
    return bool(np.all(a >= 0) and np.all(a <= 255) and np.all(s == np.rint(s)))


def forward_fused(plane, mode="qtable", param=0.0, pixel_input=None, flags_extra=0):
    """fp32 plane (H, W) -> int16 (H/8, W/8, 64): BasisChange+Quantization+ZigzagOrder.execute."""
    a = _plane(plane, np.float32)
    h, w = a.shape
    if pixel_input is None:
        pixel_input = is_pixel_like(a)
    out = np.empty((h // 8, w // 8, 64), dtype=np.int16)
    check(lib().jpegx_host_forward_fused(a.ctypes.data, h, w, w, mode_of(mode), float(param),
                                         (F_PIXEL_INPUT if pixel_input else 0) | flags_extra, out.ctypes.data),
          "jpegx_host_forward_fused")
    return out


def mean_pool_f64(plane, block_size):
    """SubSampling.execute on the device for any block_size: uint8 / integer-valued fp32 plane -> float64 means."""
    a = np.ascontiguousarray(plane)
    if a.dtype != np.uint8:
        a = a.astype(np.float32)
    bs = int(block_size)
    hh, ww = a.shape
    if hh % bs or ww % bs:
        raise JpegxError("plane must be a multiple of block_size in both dimensions")
    h, w = hh // bs, ww // bs
    with _Buffers() as dev:
        din, dout = dev(a.nbytes), dev(h * w * 8)
        din.upload(a)
        check(lib().jpegx_mean_pool_f64(din.ptr, a.dtype.itemsize, h, w, ww, bs, dout.ptr, w, None), "jpegx_mean_pool_f64")
        return dout.download((h, w), np.float64)


def forward_fused_f64(plane, mode="qtable", param=0.0, flags_extra=0):
    """float64 plane (H, W) -> int16 (H/8, W/8, 64): steps 4+5+6 entirely in float64 in the reference's
    operation order (for samples that are not exact in fp32)."""
    a = _plane(plane, np.float64)
    h, w = a.shape
    out = np.empty((h // 8, w // 8, 64), dtype=np.int16)
    check(lib().jpegx_host_forward_fused_f64(a.ctypes.data, h, w, mode_of(mode), float(param), int(flags_extra), out.ctypes.data),
          "jpegx_host_forward_fused_f64")
    return out


def forward_fused_pooled(plane, block_size, mode="qtable", param=0.0, pixel_input=None):
    """Like forward_fused with the SubSampling mean-pool (block_size in 1,2,4) fused in."""
    a = _plane(plane, np.float32)
    hh, ww = a.shape
    bs = int(block_size)
    if hh % (8 * bs) or ww % (8 * bs):
        raise JpegxError("pooled plane must be a multiple of 8*block_size in both dimensions")
    h, w = hh // bs, ww // bs
    if pixel_input is None:
        pixel_input = is_pixel_like(a, bs)
    out = np.empty((h // 8, w // 8, 64), dtype=np.int16)
    with _Buffers() as dev:
        din, dout = dev(a.nbytes), dev(out.nbytes)
        din.upload(a)
        forward_fused_device(din.ptr, h, w, dout.ptr, mode, param, F_PIXEL_INPUT if pixel_input else 0,
                             pitch=ww, pool=bs)
        return dout.download(out.shape, np.int16)


def forward_fused_u8(plane, block_size=1, mode="qtable", param=0.0, flags_extra=0):
    """uint8 plane (H*bs, W*bs) -> int16 (H/8, W/8, 64): SubSampling (bs=2) + steps 4-6, 4x less PCIe."""
    a = _plane(plane, np.uint8)
    bs = int(block_size)
    hh, ww = a.shape
    if hh % (8 * bs) or ww % (8 * bs):
        raise JpegxError("plane must be a multiple of 8*block_size in both dimensions")
    h, w = hh // bs, ww // bs
    out = np.empty((h // 8, w // 8, 64), dtype=np.int16)
    with _Buffers() as dev:
        din, dout = dev(a.nbytes), dev(out.nbytes)
        din.upload(a)
        forward_fused_u8_device(din.ptr, h, w, dout.ptr, mode, param, flags_extra, pitch=ww, pool=bs)
        return dout.download(out.shape, np.int16)


def inverse_fused(zz, mode="qtable", param=0.0, out="f32", clamp=False):
    """int16 (H/8, W/8, 64) -> (H, W) samples: ZigzagOrder+Quantization+BasisChange.invert (rounded)."""
    z = np.ascontiguousarray(zz, dtype=np.int16)
    if z.ndim != 3 or z.shape[2] != 64:
        raise JpegxError("expected a (H/8, W/8, 64) coefficient stream, got %r" % (z.shape,))
    h, w = z.shape[0] * 8, z.shape[1] * 8
    ot = _OUT_BY_NAME[out] if isinstance(out, str) else int(out)
    res = np.empty((h, w), dtype=_OUT_DTYPES[ot])
    check(lib().jpegx_host_inverse_fused(z.ctypes.data, h, w, mode_of(mode), float(param),
                                         F_CLAMP_U8 if clamp else 0, res.ctypes.data, w, ot),
          "jpegx_host_inverse_fused")
    return res


def inverse_fused_u8(zz, mode="qtable", param=0.0, inflate=1):
    """int16 (H/8, W/8, 64) -> uint8 (H*inflate, W*inflate): fused inverse + clamp + SubSampling.invert."""
    z = np.ascontiguousarray(zz, dtype=np.int16)
    if z.ndim != 3 or z.shape[2] != 64:
        raise JpegxError("expected a (H/8, W/8, 64) coefficient stream, got %r" % (z.shape,))
    h, w = z.shape[0] * 8, z.shape[1] * 8
    bs = int(inflate)
    pitch = (w * bs + 15) // 16 * 16                         # the kernel wants 16-byte aligned rows
    out = np.empty((h * bs, pitch), dtype=np.uint8)
    check(lib().jpegx_host_inverse_fused_u8_inflated(z.ctypes.data, h, w, mode_of(mode), float(param), 0, bs,
                                                     out.ctypes.data, pitch), "jpegx_host_inverse_fused_u8_inflated")
    return out[:, :w * bs]


def dct8x8_f64(a):
    """BasisChange.execute (DCT, dct_size 8), bit-identical float64."""
    a = _plane(a, np.float64)
    out = np.empty_like(a)
    check(lib().jpegx_host_dct8x8_f64(a.ctypes.data, a.shape[0], a.shape[1], out.ctypes.data), "jpegx_host_dct8x8_f64")
    return out


def idct8x8_f64(a, do_round=True):
    """BasisChange.invert (DCT, dct_size 8); do_round applies the np.round of basis_change.py:43."""
    a = _plane(a, np.float64)
    out = np.empty_like(a)
    check(lib().jpegx_host_idct8x8_f64(a.ctypes.data, a.shape[0], a.shape[1], out.ctypes.data, 1 if do_round else 0),
          "jpegx_host_idct8x8_f64")
    return out


def quantize_f64(a, mode, param=0.0):
    a = _plane(a, np.float64)
    out = np.empty_like(a)
    check(lib().jpegx_host_quantize_f64(a.ctypes.data, a.shape[0], a.shape[1], mode_of(mode), float(param),
                                        out.ctypes.data), "jpegx_host_quantize_f64")
    return out


def restore_f64(a, mode, param=0.0):
    a = _plane(a, np.float64)
    out = np.empty_like(a)
    check(lib().jpegx_host_restore_f64(a.ctypes.data, a.shape[0], a.shape[1], mode_of(mode), float(param),
                                       out.ctypes.data), "jpegx_host_restore_f64")
    return out


def zigzag(a):
    """ZigzagOrder.execute for dct_size 8 on any 2/4/8/16-byte dtype -> (H/8, W/8, 64)."""
    a = np.ascontiguousarray(a)
    if a.ndim != 2:
        raise JpegxError("expected a 2-D plane")
    h, w = a.shape
    out = np.empty((h // 8, w // 8, 64), dtype=a.dtype)
    check(lib().jpegx_host_zigzag(a.ctypes.data, h, w, a.dtype.itemsize, out.ctypes.data), "jpegx_host_zigzag")
    return out


def unzigzag(z):
    """ZigzagOrder.invert for dct_size 8."""
    z = np.ascontiguousarray(z)
    if z.ndim != 3 or z.shape[2] != 64:
        raise JpegxError("expected a (H/8, W/8, 64) array")
    h, w = z.shape[0] * 8, z.shape[1] * 8
    out = np.empty((h, w), dtype=z.dtype)
    check(lib().jpegx_host_unzigzag(z.ctypes.data, h, w, z.dtype.itemsize, out.ctypes.data), "jpegx_host_unzigzag")
    return out


def dct8x8_f32(a):
    a = _plane(a, np.float32)
    out = np.empty_like(a)
    check(lib().jpegx_host_dct8x8_f32(a.ctypes.data, a.shape[0], a.shape[1], out.ctypes.data), "jpegx_host_dct8x8_f32")
    return out


def idct8x8_f32(a):
    a = _plane(a, np.float32)
    out = np.empty_like(a)
    check(lib().jpegx_host_idct8x8_f32(a.ctypes.data, a.shape[0], a.shape[1], out.ctypes.data), "jpegx_host_idct8x8_f32")
    return out


def entropy_encode(zz):
    """int16 (..., 64) zigzag stream -> bytes: RunLengthEncoding.execute + RleBytestream.execute on the GPU."""
    z = np.ascontiguousarray(zz, dtype=np.int16)
    if z.ndim < 1 or z.shape[-1] != 64 or z.size == 0:
        raise JpegxError("expected a (..., 64) coefficient stream, got %r" % (z.shape,))
    nblocks = z.size // 64
    n = ctypes.c_size_t(0)
    check(lib().jpegx_host_entropy_encode(z.ctypes.data, nblocks, None, 0, ctypes.byref(n)), "jpegx_host_entropy_encode")
    out = np.empty(max(1, n.value), dtype=np.uint8)
    check(lib().jpegx_host_entropy_encode(z.ctypes.data, nblocks, out.ctypes.data, out.size, ctypes.byref(n)),
          "jpegx_host_entropy_encode")
    return out[:n.value].tobytes()


def entropy_block_sizes(zz):
    """Bytes of every block's code string as the device sizes pass computes them (uint32 per block)."""
    z = np.ascontiguousarray(zz, dtype=np.int16)
    if z.ndim < 1 or z.shape[-1] != 64 or z.size == 0:
        raise JpegxError("expected a (..., 64) coefficient stream, got %r" % (z.shape,))
    nblocks = z.size // 64
    L = lib()
    with _Buffers() as dev:
        dzz, dws = dev(z.nbytes), dev(L.jpegx_entropy_workspace_bytes(nblocks))
        dzz.upload(z)
        check(L.jpegx_entropy_sizes(dzz.ptr, nblocks, dws.ptr, None), "jpegx_entropy_sizes")
        out = np.empty(nblocks, dtype=np.uint32)
        check(L.jpegx_entropy_block_sizes(dws.ptr, nblocks, out.ctypes.data, None), "jpegx_entropy_block_sizes")
        return out


def last_decode_level():
    """Which scheme took the last stream the device decoder saw on this thread: 0 segments sized from the stream's average,
    1 the smallest segments (second try), 2 the whole-stream scheme (test hook, not part of include/jpegx.h)."""
    L = lib()
    L.jpegx_internal_last_decode_level.restype = ctypes.c_int
    return int(L.jpegx_internal_last_decode_level())


def forward_u8_block_sizes(plane, block_size=1, mode="qtable", param=0.0):
    """What compress_band's first two launches leave behind for a uint8 plane: the coefficient stream, the bytes of every
    block's code string as the forward kernel itself counts them, the stream's total and the error flag of the scan
    (the library's internal entries; test and measurement hook, not part of include/jpegx.h)."""
    a = np.ascontiguousarray(plane, dtype=np.uint8)
    hh, ww = a.shape
    if block_size not in (1, 2, 4) or hh % (8 * block_size) or ww % (8 * block_size):
        raise JpegxError("uint8 plane of multiples of 8 * block_size expected")
    H, W = hh // block_size, ww // block_size
    nblocks = (H // 8) * (W // 8)
    L = lib()
    L.jpegx_internal_entropy_views.argtypes = [ctypes.c_void_p, ctypes.c_longlong] + [ctypes.POINTER(ctypes.c_void_p)] * 3
    L.jpegx_internal_entropy_views.restype = None
    L.jpegx_internal_forward_u8_sized.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_ssize_t, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                                  ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.jpegx_internal_forward_u8_sized.restype = ctypes.c_int
    L.jpegx_internal_entropy_scan.argtypes = [ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p]
    L.jpegx_internal_entropy_scan.restype = ctypes.c_int
    with _Buffers() as dev:
        din, dzz, dws = dev(a.nbytes), dev(nblocks * 128), dev(L.jpegx_entropy_workspace_bytes(nblocks))
        din.upload(a)
        bb, wb, hb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        L.jpegx_internal_entropy_views(dws.ptr, nblocks, ctypes.byref(bb), ctypes.byref(wb), ctypes.byref(hb))
        check(L.jpegx_internal_forward_u8_sized(din.ptr, H, W, ww, block_size, mode_of(mode), float(param), 0, dzz.ptr, bb, wb, hb, None), "forward_u8_sized")
        check(L.jpegx_internal_entropy_scan(nblocks, dws.ptr, None), "entropy_scan")
        tot = ctypes.c_ulonglong(0)
        rc = L.jpegx_entropy_total(dws.ptr, ctypes.byref(tot), None)
        sizes = np.empty(nblocks, dtype=np.uint32)
        check(L.jpegx_entropy_block_sizes(dws.ptr, nblocks, sizes.ctypes.data, None), "jpegx_entropy_block_sizes")
        return dzz.download((H // 8, W // 8, 64), np.int16), sizes, int(tot.value), rc


def padded_shape(rows, cols, block_size=1):
    """(H, W) of a rows x cols band after pooling and DCT padding, both multiples of 8 (jpegx_padded_shape; host
    arithmetic, no device needed): the padded raw plane is (H * block_size, W * block_size)."""
    h, w = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().jpegx_padded_shape(int(rows), int(cols), int(block_size), ctypes.byref(h), ctypes.byref(w)), "jpegx_padded_shape")
    return h.value, w.value


def edge_source_indices(n, block_size=1):
    """The written specification of jpegx_pad_edges for one axis of n samples: the int64 vector src of length N such
    that padded[x] = band[src[x]], where P = ceil(n / bs) is the number of pooled samples, N = ceil(P / 8) * 8 * bs the
    padded raw extent and src[x] = min(min(x // bs, P - 1) * bs + x % bs, n - 1).  Pooling band[src_y][:, src_x] over
    bs x bs tiles gives what the reference makes of the band with Padding, SubSampling and DCTPadding."""
    n, bs = int(n), int(block_size)
    if n < 1 or bs < 1:
        raise JpegxError("edge_source_indices: n and block_size must be at least 1")
    pooled = -(-n // bs)
    x = np.arange(-(-pooled // 8) * 8 * bs, dtype=np.int64)
    return np.minimum(np.minimum(x // bs, pooled - 1) * bs + x % bs, n - 1)


def pad_edges(planes, rows, cols, block_size=1, pitch=None):
    """jpegx_pad_edges on a host array (test convenience, like the other stage wrappers): ``planes`` is the stacked
    buffer [nplanes * H * bs][pitch] of uint8 or float32 with every rows x cols picture in the top left corner of its
    plane; it goes up as it is, the margins are filled on the device, and the whole buffer comes back."""
    a = np.ascontiguousarray(planes)
    if a.ndim != 2 or a.dtype not in (np.uint8, np.float32):
        raise JpegxError("expected a 2-D uint8 or float32 buffer of stacked planes")
    bs = int(block_size)
    h, _w = padded_shape(rows, cols, bs)
    if a.shape[0] == 0 or a.shape[0] % (h * bs):
        raise JpegxError("the buffer's rows must be a whole number of padded planes")
    require_device()
    with _Buffers() as dev:
        buf = dev(a.nbytes)
        buf.upload(a)
        check(lib().jpegx_pad_edges(buf.ptr, a.dtype.itemsize, a.shape[0] // (h * bs), int(rows), int(cols), bs,
                                    a.shape[1] if pitch is None else int(pitch), None), "jpegx_pad_edges")
        return buf.download(a.shape, a.dtype)


_ELEM_OF = {np.dtype(np.uint8): 1, np.dtype(np.int32): 4, np.dtype(np.int64): 8}
_pyapi = ctypes.pythonapi
_pyapi.PyBytes_FromStringAndSize.restype = ctypes.py_object
_pyapi.PyBytes_FromStringAndSize.argtypes = [ctypes.c_void_p, ctypes.c_ssize_t]
_pyapi.PyBytes_AsString.restype = ctypes.c_void_p
_pyapi.PyBytes_AsString.argtypes = [ctypes.py_object]


def _ragged_refused(hh, ww, bs, mode, param):
    """What the ragged native entries do not take: an empty band, a block_size beyond 1..255 and, at block sizes 1, 2, 4,
    a quantiser the uint8 kernels refuse (u8_path_ok: a divisor below 0.5)."""
    if hh == 0 or ww == 0 or not 1 <= bs <= 255:
        return True
    return bs in (1, 2, 4) and not u8_path_ok(16, bs, 16, mode, param)


def _tiles_refused(hh, ww, bs, mode, param):
    """What the native entries for planes of whole tiles do not take: an empty plane, one that is not whole
    8 * block_size tiles, a block_size beyond 1..255 and, at block sizes 1, 2, 4, rows that are no multiple of 16 samples
    or a quantiser the uint8 kernels refuse (u8_path_ok)."""
    if hh == 0 or hh % (8 * bs) or ww % (8 * bs) or not 1 <= bs <= 255:
        return True
    return bs in (1, 2, 4) and bool(ww % 16 or not u8_path_ok(ww // bs, bs, ww, mode, param))


def _finish_compress(nbytes):
    """The end of an open compress job (a jpegx_host_compress_begin* that succeeded and reported ``nbytes``): the bytes
    object the job's stream is copied into from the device; the job is aborted if making it fails."""
    L = lib()
    try:
        blob = _pyapi.PyBytes_FromStringAndSize(None, nbytes)          # uninitialised bytes, filled below
        rc = L.jpegx_host_compress_finish(_pyapi.PyBytes_AsString(blob))
    except BaseException:
        L.jpegx_host_compress_abort()
        raise
    check(rc, "jpegx_host_compress_finish")
    return blob


ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)   # jpegx_alloc_fn


def _container(nbands, prefix):
    """The end that the picture jobs share: (tail, result).  ``tail`` holds the trailing arguments of a
    jpegx_host_compress_image* entry -- prefix, its length, length_prefixes, the allocator callback through which libjpegx
    asks for ONE bytes object once all byte counts are known, its user pointer, the array of the bands' sizes -- and must
    stay referenced across the native call, since it alone keeps the callback alive.  ``result()`` after a successful call:
    the whole file when there is a ``prefix``, else the list of the bands' byte strings."""
    box = []

    def alloc(_user, nbytes):
        blob = _pyapi.PyBytes_FromStringAndSize(None, nbytes)       # uninitialised bytes, filled by the device copies
        box.append(blob)
        return _pyapi.PyBytes_AsString(blob)
    sizes = (ctypes.c_size_t * nbands)()
    head = bytes(prefix) if prefix is not None else b""

    def result():
        whole = box[0]
        if prefix is not None:
            return whole
        out, at = [], 0
        for n in sizes:
            out.append(whole[at:at + n])
            at += n
        return out
    return (head, len(head), 1 if prefix is not None else 0, ALLOC_FN(alloc), None, sizes), result


def compress_plane_native(plane, block_size=1, mode="qtable", param=0.0, ragged=False):
    """compress_plane through libjpegx's native host pipeline (jpegx_host_compress_begin / _finish): pooled
    device buffers and stream, range check + narrowing of int32 / int64 bands in native threads, and the
    byte stream copied from the device straight into the returned ``bytes`` object.  Returns None when the
    plane is not an 8-bit band in a layout that path takes (the caller then uses compress_plane).
    ``ragged``: a band of ANY rows x cols, padded on the device (jpegx_host_compress_begin_ragged: Padding and
    DCTPadding as a margin fill in the padded device plane) -- the bytes of the reference's compress_band; without it
    the plane must be whole 8 * block_size tiles already, as before."""
    src = plane if isinstance(plane, np.ndarray) else np.asarray(plane)
    bs = int(block_size)
    elem = _ELEM_OF.get(src.dtype)
    if elem is None or src.ndim != 2 or not src.flags.c_contiguous:
        return None
    hh, ww = src.shape
    L = lib()
    n = ctypes.c_size_t(0)
    if ragged:
        if _ragged_refused(hh, ww, bs, mode, param):
            return None
        rc = L.jpegx_host_compress_begin_ragged(src.ctypes.data, elem, hh, ww, ww, bs, mode_of(mode), float(param), ctypes.byref(n))
    else:
        if _tiles_refused(hh, ww, bs, mode, param):
            return None
        rc = L.jpegx_host_compress_begin(src.ctypes.data, elem, hh // bs, ww // bs, ww, bs, mode_of(mode), float(param),
                                         ctypes.byref(n))
    if rc == -4:                                        # JPEGX_E_UNSUPPORTED: not an 8-bit band after all
        return None
    check(rc, "jpegx_host_compress_begin")
    return _finish_compress(n.value)


def compress_image_native(planes, block_size=1, mode="qtable", param=0.0, prefix=None, ragged=False):
    """Steps 1-8 for all bands of one picture in ONE native job (jpegx_host_compress_image): the bands share one lock
    of the device's pool and alternate between two streams; once all byte counts are known libjpegx asks (through a
    callback) for ONE ``bytes`` object and copies every band from the device straight to its place in it.
    ``planes``: 2-D arrays of one shape and dtype (uint8 / int32 / int64), already padded to a multiple of
    8 * block_size.  With ``prefix`` (the container header) the result is the finished file -- prefix, then every
    band behind its '<L' byte count (file_format.generate_data); without it the list of the bands' byte strings.
    None when the bands are not 8-bit planes in a layout this path takes.
    ``ragged``: bands of ANY rows x cols, padded on the device (jpegx_host_compress_image_ragged)."""
    arrs = [p if isinstance(p, np.ndarray) else np.asarray(p) for p in planes]
    bs = int(block_size)
    if not arrs or len(arrs) > 4:
        return None
    a0 = arrs[0]
    elem = _ELEM_OF.get(a0.dtype)
    if elem is None or a0.ndim != 2:
        return None
    if any(a.shape != a0.shape or a.dtype != a0.dtype or not a.flags.c_contiguous for a in arrs):
        return None
    hh, ww = a0.shape
    if (_ragged_refused if ragged else _tiles_refused)(hh, ww, bs, mode, param):
        return None
    L = lib()
    ptrs = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    tail, result = _container(len(arrs), prefix)
    tail = (ww, bs, mode_of(mode), float(param)) + tail
    if ragged:
        rc = L.jpegx_host_compress_image_ragged(ptrs, len(arrs), elem, hh, ww, *tail)
    else:
        rc = L.jpegx_host_compress_image(ptrs, len(arrs), elem, hh // bs, ww // bs, *tail)
    if rc == -4:                                        # JPEGX_E_UNSUPPORTED: not 8-bit bands after all
        return None
    check(rc, "jpegx_host_compress_image")
    return result()


def _colour_keyword(plain, rgb_form):
    """``plain`` with the picture jobs' keyword ``colour``: None (the default: ``plain`` itself is called, as it always
    was -- the bands as they come) or 'rgb' (``rgb_form``, same arguments: three-band RGB pixels outside, Pillow's
    conversion to or from YCbCr inside the job).  The keyword is added here and not to ``plain``, whose signature and
    calls stay what they are."""
    @functools.wraps(plain)
    def entry(*args, colour=None, **kwargs):
        if colour is None:
            return plain(*args, **kwargs)
        if colour != "rgb":
            raise JpegxError("%s: colour must be None or 'rgb', got %r" % (plain.__name__, colour))
        return rgb_form(*args, **kwargs)
    return entry


def _three_bands(rgb, nbands, what):
    if rgb and nbands != 3:
        raise JpegxError("%s: colour='rgb' takes three bands, got %d" % (what, nbands))


def _convert_pixels(pixels, entry):
    a = _pixels_u8(pixels)
    if a.shape[2] != 3:
        raise JpegxError("%s: expected pixels (rows, cols, 3), got %r" % (entry, a.shape))
    rows, cols = a.shape[:2]
    if rows * cols > 2 ** 31 - 1:
        raise JpegxError("%s: more than 2^31 - 1 pixels in one picture" % entry)
    require_device()
    with _Buffers() as dev:
        buf = dev(a.nbytes)
        buf.upload(a)
        check(getattr(lib(), entry)(buf.ptr, cols * 3, rows, cols, buf.ptr, cols * 3, None), entry)
        return buf.download(a.shape, np.uint8)


def rgb_to_ycbcr(pixels):
    """uint8 RGB pixels (rows, cols, 3) -> the YCbCr pixels Pillow's Image.convert('YCbCr') gives, byte for byte, on the
    device (jpegx_rgb_to_ycbcr_u8, in place on the uploaded copy)."""
    return _convert_pixels(pixels, "jpegx_rgb_to_ycbcr_u8")


def ycbcr_to_rgb(pixels):
    """uint8 YCbCr pixels (rows, cols, 3) -> the RGB pixels Pillow's Image.convert('RGB') gives, byte for byte, on the
    device (jpegx_ycbcr_to_rgb_u8)."""
    return _convert_pixels(pixels, "jpegx_ycbcr_to_rgb_u8")


def _compress_image_packed(rgb, pixels, block_size=1, mode="qtable", param=0.0, prefix=None, ragged=False):
    a = pixels if isinstance(pixels, np.ndarray) else np.asarray(pixels)
    bs = int(block_size)
    if a.ndim != 3 or a.dtype != np.uint8 or not 1 <= a.shape[2] <= 4 or not a.flags.c_contiguous:
        return None
    hh, ww, nb = a.shape
    _three_bands(rgb, nb, "compress_image_packed")
    if hh > 65535:
        return None
    if (_ragged_refused if ragged else _tiles_refused)(hh, ww, bs, mode, param):
        return None
    L = lib()
    tail, result = _container(nb, prefix)
    tail = (ww * nb, bs, mode_of(mode), float(param)) + tail
    if rgb:
        check(L.jpegx_host_compress_image_rgb(a.ctypes.data, hh, ww, *tail), "jpegx_host_compress_image_rgb")
    elif ragged:
        check(L.jpegx_host_compress_image_packed_ragged(a.ctypes.data, nb, hh, ww, *tail), "jpegx_host_compress_image_packed_ragged")
    else:
        check(L.jpegx_host_compress_image_packed(a.ctypes.data, nb, hh // bs, ww // bs, *tail), "jpegx_host_compress_image_packed")
    return result()


def compress_image_packed(pixels, block_size=1, mode="qtable", param=0.0, prefix=None, ragged=False):
    """compress_image_native from pixel-interleaved samples: ``pixels`` is the (rows, cols, nbands) uint8 array that
    np.asarray(image) gives for a multi-band PIL image -- half the host time of image.split() plus an array per band; the
    planes are made on the device (jpegx_host_compress_image_packed).  rows and cols must be multiples of 8 * block_size
    unless ``ragged`` (jpegx_host_compress_image_packed_ragged: any rows x cols, padded on the device).  Same bytes as
    compress_image_native; None when this road does not apply.  Keyword ``colour='rgb'``: the pixels are RGB and become Pillow's
    YCbCr on the device first (jpegx_host_compress_image_rgb, the ragged job) -- the bytes of this call on
    np.asarray(image.convert('YCbCr'))."""
    return _compress_image_packed(False, pixels, block_size, mode, param, prefix, ragged)


def _decompress_image_native(rgb, blobs, height, width, block_size, mode, param, rows, cols, interleave=True):
    coded = [_coded(b) for b in blobs]
    n = len(coded)
    ptrs = (ctypes.c_void_p * n)(*[c[0] for c in coded])
    sizes = (ctypes.c_size_t * n)(*[c[1] for c in coded])
    _three_bands(rgb, n, "decompress_image_native")
    if rgb and not interleave:
        raise JpegxError("decompress_image_native: colour='rgb' gives interleaved pixels")
    out = np.empty((rows, cols, n) if interleave else (n, rows, cols), dtype=np.uint8)
    if rgb:
        check(lib().jpegx_host_decompress_image_rgb(ptrs, sizes, int(height), int(width), int(block_size), mode_of(mode), float(param),
                                                    out.ctypes.data, cols * 3, int(rows), int(cols)), "jpegx_host_decompress_image_rgb")
        return out
    check(lib().jpegx_host_decompress_image(ptrs, sizes, n, int(height), int(width), int(block_size), mode_of(mode), float(param),
                                            out.ctypes.data, cols * n if interleave else cols, int(rows), int(cols), 1 if interleave else 0),
          "jpegx_host_decompress_image")
    return out


def decompress_image_native(blobs, height, width, block_size, mode, param, rows, cols, interleave=True):
    """All bands of one picture back in ONE native job (jpegx_host_decompress_image).  (height, width): a band after
    pooling (multiples of 8); the result is cropped to (rows, cols): uint8 (rows, cols, nbands) when ``interleave``
    (what PIL's Image.fromarray takes), else (nbands, rows, cols).  Keyword ``colour='rgb'``: the three bands are Y, Cb, Cr and the
    interleaved result is Pillow's RGB of them, converted on the device (jpegx_host_decompress_image_rgb)."""
    return _decompress_image_native(False, blobs, height, width, block_size, mode, param, rows, cols, interleave)


compress_image_packed = _colour_keyword(compress_image_packed, functools.partial(_compress_image_packed, True))
decompress_image_native = _colour_keyword(decompress_image_native, functools.partial(_decompress_image_native, True))


def compress_plane(plane, block_size=1, mode="qtable", param=0.0):
    """Steps 1-8 of the codec for one (already padded) plane with everything on the device:
    fused mean-pool + DCT + quantise + zigzag, then the entropy stage; only the final bytes come back."""
    src = np.asarray(plane)
    bs = int(block_size)
    if src.ndim != 2:
        raise JpegxError("expected a 2-D plane, got shape %r" % (src.shape,))
    hh, ww = src.shape
    if hh % (8 * bs) or ww % (8 * bs):
        raise JpegxError("plane must be a multiple of 8*block_size in both dimensions")
    blob = compress_plane_native(src, bs, mode, param)
    if blob is not None:
        return blob
    h, w = hh // bs, ww // bs
    nblocks = (h // 8) * (w // 8)
    as_u8 = (src.dtype == np.uint8 or (src.dtype.kind in "ui" and src.size and src.min() >= 0 and src.max() <= 255)) \
        and u8_path_ok(w, bs, ww, mode, param)
    a = np.ascontiguousarray(src, dtype=np.uint8 if as_u8 else np.float32)
    L = lib()
    with _Buffers() as dev:
        din, dzz = dev(a.nbytes), dev(h * w * 2)
        dws = dev(L.jpegx_entropy_workspace_bytes(nblocks))
        din.upload(a)
        if as_u8:
            forward_fused_u8_device(din.ptr, h, w, dzz.ptr, mode, param, 0, pitch=ww, pool=bs)
        else:
            forward_fused_device(din.ptr, h, w, dzz.ptr, mode, param, F_PIXEL_INPUT if is_pixel_like(a, bs) else 0,
                                 pitch=ww, pool=bs)
        check(L.jpegx_entropy_sizes(dzz.ptr, nblocks, dws.ptr, None), "jpegx_entropy_sizes")
        total = ctypes.c_ulonglong(0)
        check(L.jpegx_entropy_total(dws.ptr, ctypes.byref(total), None), "jpegx_entropy_total")
        dout = dev(max(1, total.value))
        check(L.jpegx_entropy_emit(dzz.ptr, nblocks, dws.ptr, dout.ptr, None), "jpegx_entropy_emit")
        return dout.download((total.value,), np.uint8).tobytes()


def entropy_decode_gpu(blob, nblocks):
    """bytes -> int16 (nblocks, 64) with the parallel decoder on the device (jpegx_entropy_decode.hip)."""
    ptr, size, _keep = _coded(blob)
    out = np.empty((int(nblocks), 64), dtype=np.int16)
    check(lib().jpegx_host_entropy_decode_gpu(ptr, size, int(nblocks), out.ctypes.data), "jpegx_host_entropy_decode_gpu")
    return out


def decompress_plane(blob, height, width, block_size=1, mode="qtable", param=0.0):
    """Steps 8-1 inverted for one plane, everything on the device: entropy decoding, un-zigzag, dequantise, IDCT,
    round, clamp, replicate block_size x block_size.  (height, width) = the plane AFTER pooling, multiples of 8.
    Returns uint8 (height * block_size, width * block_size)."""
    ptr, size, _keep = _coded(blob)
    bs = int(block_size)
    pitch = (width * bs + 15) // 16 * 16
    out = np.empty((height * bs, pitch), dtype=np.uint8)
    check(lib().jpegx_host_decompress_plane(ptr, size, int(height), int(width), bs,
                                            mode_of(mode), float(param), out.ctypes.data, pitch), "jpegx_host_decompress_plane")
    return out[:, :width * bs]


def decompress_plane_i64(blob, height, width, block_size, mode, param, rows, cols):
    """decompress_plane as the (rows, cols) int64 band the reference's decompress_band returns."""
    ptr, size, _keep = _coded(blob)
    out = np.empty((int(rows), int(cols)), dtype=np.int64)
    check(lib().jpegx_host_decompress_plane_i64(ptr, size, int(height), int(width),
                                                int(block_size), mode_of(mode), float(param), out.ctypes.data, int(rows), int(cols)),
          "jpegx_host_decompress_plane_i64")
    return out


def entropy_decode_device(d_bytes, nbytes, nblocks, d_workspace, d_zz, stream=None):
    """The device decoder on the caller's device buffers (jpegx_entropy_decode / _status): first try, then -- if that
    could not take the stream -- the second; returns the level that took it.  d_bytes: the stream with 16 zero bytes
    behind it; d_workspace: jpegx_entropy_decode_workspace_bytes(nbytes, nblocks) bytes, 256-byte aligned.  Raises
    JpegxError for a malformed stream, and for the (degenerate) streams only the whole-stream scheme takes."""
    L = lib()
    for level in (0, 1):
        check(L.jpegx_entropy_decode(d_bytes, int(nbytes), int(nblocks), d_workspace, d_zz, level, stream), "jpegx_entropy_decode")
        rc = L.jpegx_entropy_decode_status(d_workspace, stream)
        if rc == 0:
            return level
        if rc != 1:
            check(rc, "jpegx_entropy_decode_status")
    raise JpegxError("jpegx_entropy_decode: neither level took the stream (more block starts than a segment's tables hold)")


def entropy_decode(blob, nblocks):
    """bytes -> int16 (nblocks, 64): RleBytestream.invert + RunLengthEncoding.invert (host, sequential)."""
    ptr, size, _keep = _coded(blob)
    out = np.empty((int(nblocks), 64), dtype=np.int16)
    check(lib().jpegx_host_entropy_decode(ptr, size, int(nblocks), out.ctypes.data), "jpegx_host_entropy_decode")
    return out


# ---------------------------------------------------------------------------------------------
# any DCT size (csrc/jpegx_dctn.hip): transform 'DCT', dct_size N in 2..32, all float64 in one documented order
# ---------------------------------------------------------------------------------------------
def _plane_n(a, n, dtype=np.float64):
    a = _plane(a, dtype)
    n = int(n)
    if a.size == 0 or a.shape[0] % max(n, 1) or a.shape[1] % max(n, 1):
        raise JpegxError("expected a non-empty plane of whole %d x %d blocks, got shape %r" % (n, n, a.shape))
    return a, n


def _stream_n(zz, n):
    z = np.ascontiguousarray(zz, dtype=np.int32)
    n = int(n)
    if z.ndim != 3 or z.shape[2] != n * n or z.size == 0:
        raise JpegxError("expected a (H/N, W/N, N*N) coefficient stream for N = %d, got %r" % (n, z.shape))
    return z, n


def dct_tables_n(n):
    """(C, Cn, Dinv, zigzag) as the dct_size-n kernels use them: transforms.dct_matrix, dct_matrix_normalized, the
    diagonal of normalization_matrix and Zigzag(n).flat_indices().  Host arithmetic only, no device needed."""
    n = int(n)
    m = max(n, 1)
    c, cn, dinv, zig = np.empty((m, m)), np.empty((m, m)), np.empty(m), np.empty(m * m, dtype=np.uint16)
    check(lib().jpegx_dct_tables_n(n, c.ctypes.data, cn.ctypes.data, dinv.ctypes.data, zig.ctypes.data), "jpegx_dct_tables_n")
    return c, cn, dinv, zig


def forward_fused_n(plane, n, mode="none", param=0.0):
    """float64 plane (H, W) -> int32 (H/n, W/n, n*n): BasisChange + Quantization + ZigzagOrder.execute for dct_size n."""
    a, n = _plane_n(plane, n)
    h, w = a.shape
    out = np.empty((h // n, w // n, n * n), dtype=np.int32)
    check(lib().jpegx_host_forward_fused_n(a.ctypes.data, h, w, n, mode_of(mode), float(param), out.ctypes.data),
          "jpegx_host_forward_fused_n")
    return out


def inverse_fused_n(zz, n, mode="none", param=0.0, out="i32", out_pitch=None):
    """int32 (H/n, W/n, n*n) -> (H, W) samples: ZigzagOrder + Quantization + BasisChange.invert (rounded) for dct_size n;
    out 'i32' (unclamped) or 'u8' (clamped to 0..255, Normalization.invert fused)."""
    z, n = _stream_n(zz, n)
    h, w = z.shape[0] * n, z.shape[1] * n
    if out not in ("i32", "u8"):
        raise JpegxError("inverse_fused_n: out must be 'i32' or 'u8'")
    pitch = w if out_pitch is None else int(out_pitch)
    res = np.zeros((h, max(pitch, w)), dtype=np.int32 if out == "i32" else np.uint8)
    check(lib().jpegx_host_inverse_fused_n(z.ctypes.data, h, w, n, mode_of(mode), float(param), F_CLAMP_U8 if out == "u8" else 0,
                                           res.ctypes.data, pitch), "jpegx_host_inverse_fused_n")
    return res if pitch == w else res[:, :w]


def dct_f64_n(plane, n):
    """BasisChange.execute (DCT, dct_size n): the float64 coefficients of every n x n block in its place."""
    a, n = _plane_n(plane, n)
    out = np.empty_like(a)
    check(lib().jpegx_host_dct_f64_n(a.ctypes.data, a.shape[0], a.shape[1], n, out.ctypes.data), "jpegx_host_dct_f64_n")
    return out


def idct_f64_n(plane, n, do_round=True):
    """BasisChange.invert (DCT, dct_size n); do_round applies the np.round of basis_change.py:43."""
    a, n = _plane_n(plane, n)
    out = np.empty_like(a)
    check(lib().jpegx_host_idct_f64_n(a.ctypes.data, a.shape[0], a.shape[1], n, out.ctypes.data, 1 if do_round else 0),
          "jpegx_host_idct_f64_n")
    return out


def _stream_any_n(zz, block_len):
    """The argument checks of entropy_encode_n and entropy_encode_n_gpu: (contiguous int32 stream, block_len, nblocks)."""
    z = np.ascontiguousarray(zz, dtype=np.int32)
    block_len = int(z.shape[-1] if block_len is None and z.ndim else block_len or 0)
    if z.size == 0 or block_len < 1 or z.size % block_len:
        raise JpegxError("expected a non-empty stream of whole blocks of %d coefficients, got %r" % (block_len, z.shape))
    return z, block_len, z.size // block_len


def entropy_encode_n(zz, block_len=None):
    """int32 (..., block_len) zigzag stream -> bytes: RunLengthEncoding.execute + RleBytestream.execute for blocks of any
    length, sequentially on the host (no device needed)."""
    z, block_len, nblocks = _stream_any_n(zz, block_len)
    n = ctypes.c_size_t(0)
    L = lib()
    check(L.jpegx_host_entropy_encode_n(z.ctypes.data, nblocks, block_len, None, 0, ctypes.byref(n)), "jpegx_host_entropy_encode_n")
    blob = _pyapi.PyBytes_FromStringAndSize(None, n.value)          # uninitialised bytes, filled below
    check(L.jpegx_host_entropy_encode_n(z.ctypes.data, nblocks, block_len, _pyapi.PyBytes_AsString(blob), n.value, ctypes.byref(n)),
          "jpegx_host_entropy_encode_n")
    return blob


def entropy_encode_n_gpu(zz, block_len=None):
    """entropy_encode_n on the device (csrc/jpegx_entropy_n.hip): upload, jpegx_entropy_sizes_n, jpegx_entropy_total,
    jpegx_entropy_emit_n, download.  Same bytes, same refusals."""
    z, block_len, nblocks = _stream_any_n(zz, block_len)
    L = lib()
    ws_bytes = L.jpegx_entropy_workspace_bytes_n(nblocks, block_len)
    if ws_bytes == 0:
        raise JpegxError("the device coder takes blocks of 1 .. 1024 coefficients and streams below 2^31 coefficients, got %r" % (z.shape,))
    with _Buffers() as dev:
        dzz, dws = dev(z.nbytes), dev(ws_bytes)
        dzz.upload(z)
        check(L.jpegx_entropy_sizes_n(dzz.ptr, nblocks, block_len, dws.ptr, None), "jpegx_entropy_sizes_n")
        total = ctypes.c_ulonglong(0)
        check(L.jpegx_entropy_total(dws.ptr, ctypes.byref(total), None), "jpegx_entropy_total")
        dout = dev(max(total.value, 1))
        check(L.jpegx_entropy_emit_n(dzz.ptr, nblocks, block_len, dws.ptr, dout.ptr, None), "jpegx_entropy_emit_n")
        return dout.download((total.value,), np.uint8).tobytes()


def compress_plane_n(plane, n, mode="none", param=0.0):
    """float64 plane (H, W) of whole n x n blocks -> bytes: steps 4-8 for dct_size n as one pooled device job
    (jpegx_host_compress_begin_n / _finish) -- what entropy_encode_n(forward_fused_n(plane, n, mode, param)) returns, without
    the coefficient stream leaving the device.  JpegxError naming BadRleCodeError for an amplitude beyond 15 bits."""
    a, n = _plane_n(plane, n)
    h, w = a.shape
    L = lib()
    nbytes = ctypes.c_size_t(0)
    check(L.jpegx_host_compress_begin_n(a.ctypes.data, h, w, w, n, mode_of(mode), float(param), ctypes.byref(nbytes)),
          "jpegx_host_compress_begin_n")
    return _finish_compress(nbytes.value)


def band_shape_n(rows, cols, bs, n):
    """(H, W) of the plane that leaves step 3 for a rows x cols band at block_size bs and dct_size n
    (jpegx_band_shape_n: pipeline.geometry.band_geometry's last pair; host arithmetic, no device needed)."""
    h, w = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().jpegx_band_shape_n(int(rows), int(cols), int(bs), int(n), ctypes.byref(h), ctypes.byref(w)), "jpegx_band_shape_n")
    return h.value, w.value


def _band_u8(band):
    a = band if isinstance(band, np.ndarray) else np.asarray(band)
    if a.ndim != 2 or a.size == 0 or a.dtype.kind not in "ui":
        raise JpegxError("expected a non-empty 2-D band of an integer dtype, got %r of %s" % (a.shape, a.dtype))
    if a.dtype != np.uint8:
        if a.min() < 0 or a.max() > 255:
            raise JpegxError("samples outside 0..255: not an 8-bit band")
        a = a.astype(np.uint8)
    return np.ascontiguousarray(a)


def band_plane_n(band, bs, n):
    """8-bit band (rows, cols) -> the float64 plane (H, W) that leaves step 3: Padding, SubSampling, DCTPadding and
    Normalization.execute for block_size bs and dct_size n as one launch (jpegx_band_plane_n), bit for bit what the
    host step classes make of the band."""
    a = _band_u8(band)
    rows, cols = a.shape
    h, w = band_shape_n(rows, cols, bs, n)
    require_device()
    with _Buffers() as dev:
        din, dout = dev(a.nbytes), dev(h * w * 8)
        din.upload(a)
        check(lib().jpegx_band_plane_n(din.ptr, rows, cols, cols, int(bs), int(n), dout.ptr, w, None), "jpegx_band_plane_n")
        return dout.download((h, w), np.float64)


def compress_band_n(band, bs, n, mode="none", param=0.0):
    """Integer band (rows, cols) of uint8 / int32 / int64 -> bytes: all nine steps of compress_band for dct_size n as one
    pooled device job (jpegx_host_compress_begin_band_n / _finish) -- the band goes up as bytes, steps 0-3 are one launch
    (jpegx_band_plane_n), steps 4-8 those of compress_plane_n.  None when the native entry says "not an 8-bit band" (a
    sample outside 0..255, another dtype or layout); JpegxError naming BadRleCodeError for an amplitude beyond 15 bits."""
    src = band if isinstance(band, np.ndarray) else np.asarray(band)
    elem = _ELEM_OF.get(src.dtype)
    if elem is None or src.ndim != 2 or src.size == 0:
        return None
    if src.strides[1] != elem or src.strides[0] < src.shape[1] * elem or src.strides[0] % elem:
        src = np.ascontiguousarray(src)                                 # anything but rows a fixed number of samples apart
    rows, cols = src.shape
    L = lib()
    nbytes = ctypes.c_size_t(0)
    rc = L.jpegx_host_compress_begin_band_n(src.ctypes.data, elem, rows, cols, src.strides[0] // elem, int(bs), int(n), mode_of(mode),
                                            float(param), ctypes.byref(nbytes))
    if rc == -4:                                        # JPEGX_E_UNSUPPORTED: not an 8-bit band after all
        return None
    check(rc, "jpegx_host_compress_begin_band_n")
    return _finish_compress(nbytes.value)


def entropy_decode_n(blob, nblocks, block_len):
    """bytes -> int32 (nblocks, block_len): RleBytestream.invert + RunLengthEncoding.invert (host, sequential)."""
    ptr, size, _keep = _coded(blob)
    out = np.empty((max(int(nblocks), 0), max(int(block_len), 0)), dtype=np.int32)
    check(lib().jpegx_host_entropy_decode_n(ptr, size, int(nblocks), int(block_len),
                                            out.ctypes.data if out.size else None), "jpegx_host_entropy_decode_n")
    return out


def entropy_decode_n_gpu(blob, nblocks, block_len):
    """entropy_decode_n on the device (csrc/jpegx_entropy_decode_n.hip): bytes -> int32 (nblocks, block_len), the same
    arrays; JpegxError for a stream the device refuses."""
    ptr, size, _keep = _coded(blob)
    out = np.empty((max(int(nblocks), 0), max(int(block_len), 0)), dtype=np.int32)
    check(lib().jpegx_host_entropy_decode_n_gpu(ptr, size, int(nblocks), int(block_len),
                                                out.ctypes.data if out.size else None), "jpegx_host_entropy_decode_n_gpu")
    return out


def entropy_decode_n_device(d_bytes, nbytes, nblocks, block_len, d_workspace, d_zz, stream=None):
    """The run-time block length decoder on the caller's device buffers (jpegx_entropy_decode_n / _status_n).  d_bytes: the
    stream, dword aligned, with 16 zero bytes behind it; d_workspace: jpegx_entropy_decode_workspace_bytes_n(nbytes,
    nblocks, block_len) bytes, 16-byte aligned, reusable as it is; d_zz: nblocks * block_len int32, 4-byte aligned.
    Synchronises the stream; raises JpegxError for a stream that is not nblocks well-formed blocks."""
    L = lib()
    check(L.jpegx_entropy_decode_n(d_bytes, int(nbytes), int(nblocks), int(block_len), d_workspace, d_zz, stream), "jpegx_entropy_decode_n")
    check(L.jpegx_entropy_decode_status_n(d_workspace, stream), "jpegx_entropy_decode_status_n")


def decompress_plane_n(blob, height, width, n, mode="none", param=0.0, out="u8"):
    """Steps 8-4 inverted for dct_size n as one pooled device job (jpegx_host_decompress_plane_n): what
    inverse_fused_n(entropy_decode_n(blob, ...), n, mode, param, out) returns, without the coefficient stream on the host.
    (height, width): the plane of whole n x n blocks; out 'u8' (clamped) or 'i32'.  JpegxError for a refused stream."""
    if out not in ("i32", "u8"):
        raise JpegxError("decompress_plane_n: out must be 'i32' or 'u8'")
    ptr, size, _keep = _coded(blob)
    h, w = int(height), int(width)
    res = np.empty((max(h, 0), max(w, 0)), dtype=np.int32 if out == "i32" else np.uint8)
    check(lib().jpegx_host_decompress_plane_n(ptr, size, h, w, int(n), mode_of(mode), float(param),
                                              F_CLAMP_U8 if out == "u8" else 0, res.ctypes.data if res.size else None, w),
          "jpegx_host_decompress_plane_n")
    return res


def inflate_crop_u8(plane, bs, rows, cols):
    """uint8 plane (the clamped output of inverse_fused_n, at least ceil(rows / bs) x ceil(cols / bs)) -> the uint8 band
    (rows, cols): DCTPadding.invert, SubSampling.invert and Padding.invert for block_size bs as one launch
    (jpegx_inflate_crop_u8), out[y][x] = plane[y // bs][x // bs]."""
    a = plane if isinstance(plane, np.ndarray) else np.asarray(plane)
    if a.ndim != 2 or a.size == 0 or a.dtype != np.uint8:
        raise JpegxError("expected a non-empty 2-D uint8 plane, got %r of %s" % (a.shape, a.dtype))
    a = np.ascontiguousarray(a)
    rows, cols, bs = int(rows), int(cols), int(bs)
    if rows < 1 or cols < 1:                        # the entry's refusals, before anything is allocated
        raise JpegxError("inflate_crop_u8: rows and cols must be at least 1")
    if not 1 <= bs <= 255:
        raise JpegxError("inflate_crop_u8: block_size must be in 1..255")
    if rows * cols > 2 ** 31 - 1:
        raise JpegxError("inflate_crop_u8: more than 2^31 - 1 samples in one band")
    if a.shape[0] < -(-rows // bs) or a.shape[1] < -(-cols // bs):
        raise JpegxError("inflate_crop_u8: a %d x %d plane is smaller than the pooled band" % a.shape)
    require_device()
    with _Buffers() as dev:
        din, dout = dev(a.nbytes), dev(rows * cols)
        din.upload(a)
        check(lib().jpegx_inflate_crop_u8(din.ptr, a.shape[1], rows, cols, bs, dout.ptr, cols, None), "jpegx_inflate_crop_u8")
        return dout.download((rows, cols), np.uint8)


def decompress_band_n(blob, rows, cols, bs, n, mode="none", param=0.0, out="u8"):
    """All nine steps of decompress_band for dct_size n as one pooled device job (jpegx_host_decompress_band_n /
    _band_i64_n): the band (rows, cols) at its configured size, uint8 for out 'u8' or -- what the reference's
    decompress_band returns -- int64 for 'i64'; the plane of whole blocks never reaches the host.  JpegxError for a refused
    stream."""
    if out not in ("u8", "i64"):
        raise JpegxError("decompress_band_n: out must be 'u8' or 'i64'")
    ptr, size, _keep = _coded(blob)
    rows, cols = int(rows), int(cols)
    if rows * cols > 2 ** 31 - 1:                   # before NumPy is asked for it
        raise JpegxError("decompress_band_n: more than 2^31 - 1 samples in one band")
    res = np.empty((max(rows, 0), max(cols, 0)), dtype=np.uint8 if out == "u8" else np.int64)
    args = (ptr, size, rows, cols, int(bs), int(n), mode_of(mode), float(param), res.ctypes.data if res.size else None)
    if out == "u8":
        check(lib().jpegx_host_decompress_band_n(*args, cols), "jpegx_host_decompress_band_n")
    else:
        check(lib().jpegx_host_decompress_band_i64_n(*args), "jpegx_host_decompress_band_i64_n")
    return res


def _pixels_u8(pixels):
    a = pixels if isinstance(pixels, np.ndarray) else np.asarray(pixels)
    if a.ndim != 3 or a.size == 0 or a.dtype != np.uint8 or not 1 <= a.shape[2] <= 4:
        raise JpegxError("expected non-empty uint8 pixels (rows, cols, 1..4), got %r of %s" % (a.shape, a.dtype))
    return np.ascontiguousarray(a)


def band_planes_packed_n(pixels, bs, n, pitch=None, out_pitch=None):
    """uint8 pixels (rows, cols, nb) -> the list of nb float64 planes (H, W) that leave step 3, every band in one launch
    (jpegx_band_planes_packed_n): plane k is bit for bit band_plane_n(pixels[:, :, k], bs, n).  ``pitch``: bytes between the
    rows of the packed picture on the device (default cols * nb); ``out_pitch``: doubles between the planes' rows (default W)."""
    a = _pixels_u8(pixels)
    rows, cols, nb = a.shape
    h, w = band_shape_n(rows, cols, bs, n)
    pitch = cols * nb if pitch is None else int(pitch)
    opitch = w if out_pitch is None else int(out_pitch)
    if pitch < cols * nb or opitch < w:
        raise JpegxError("band_planes_packed_n: pitch smaller than the row")
    require_device()
    with _Buffers() as dev:
        din = dev(rows * pitch)
        douts = [dev(h * opitch * 8) for _ in range(nb)]
        staged = np.zeros((rows, pitch), np.uint8)
        staged[:, :cols * nb] = a.reshape(rows, cols * nb)
        din.upload(staged)
        ptrs = (ctypes.c_void_p * nb)(*[d.ptr for d in douts])
        check(lib().jpegx_band_planes_packed_n(din.ptr, nb, rows, cols, pitch, int(bs), int(n), ptrs, opitch, None), "jpegx_band_planes_packed_n")
        return [np.ascontiguousarray(d.download((h, opitch), np.float64)[:, :w]) for d in douts]


def inflate_crop_pack_u8(planes, rows, cols, bs, pitch=None, out_pitch=None):
    """nb uint8 planes of one shape (the clamped outputs of inverse_fused_n, at least ceil(rows / bs) x ceil(cols / bs)) ->
    uint8 pixels (rows, cols, nb): DCTPadding.invert, SubSampling.invert, Padding.invert and the np.dstack of Jpeg.decompress
    as one launch (jpegx_inflate_crop_pack_u8), out[y][x][k] = planes[k][y // bs][x // bs].  ``pitch``: bytes between the
    planes' rows on the device (default their width); ``out_pitch``: bytes between the picture's rows (default cols * nb)."""
    arrs = [np.ascontiguousarray(p) for p in planes]
    nb = len(arrs)
    if not 1 <= nb <= 4 or any(a.ndim != 2 or a.size == 0 or a.dtype != np.uint8 or a.shape != arrs[0].shape for a in arrs):
        raise JpegxError("expected 1..4 non-empty 2-D uint8 planes of one shape")
    rows, cols, bs = int(rows), int(cols), int(bs)
    if rows < 1 or cols < 1:                        # the entry's refusals, before anything is allocated
        raise JpegxError("inflate_crop_pack_u8: rows and cols must be at least 1")
    if not 1 <= bs <= 255:
        raise JpegxError("inflate_crop_pack_u8: block_size must be in 1..255")
    if rows * cols > 2 ** 31 - 1:
        raise JpegxError("inflate_crop_pack_u8: more than 2^31 - 1 samples in one band")
    ph, pw = arrs[0].shape
    if ph < -(-rows // bs) or pw < -(-cols // bs):
        raise JpegxError("inflate_crop_pack_u8: a %d x %d plane is smaller than the pooled band" % (ph, pw))
    pitch = pw if pitch is None else int(pitch)
    opitch = cols * nb if out_pitch is None else int(out_pitch)
    if pitch < pw or opitch < cols * nb:
        raise JpegxError("inflate_crop_pack_u8: pitch smaller than the row")
    require_device()
    with _Buffers() as dev:
        dins, dout = [dev(ph * pitch) for _ in range(nb)], dev(rows * opitch)
        for d, a in zip(dins, arrs):
            staged = np.zeros((ph, pitch), np.uint8)
            staged[:, :pw] = a
            d.upload(staged)
        ptrs = (ctypes.c_void_p * nb)(*[d.ptr for d in dins])
        check(lib().jpegx_inflate_crop_pack_u8(ptrs, nb, pitch, rows, cols, bs, dout.ptr, opitch, None), "jpegx_inflate_crop_pack_u8")
        return np.ascontiguousarray(dout.download((rows, opitch), np.uint8)[:, :cols * nb]).reshape(rows, cols, nb)


def _compress_image_packed_n(rgb, pixels, bs, n, mode="none", param=0.0, prefix=None):
    a = pixels if isinstance(pixels, np.ndarray) else np.asarray(pixels)
    if a.ndim != 3 or a.size == 0 or a.dtype != np.uint8 or not 1 <= a.shape[2] <= 4 or not a.flags.c_contiguous:
        return None
    rows, cols, nb = a.shape
    _three_bands(rgb, nb, "compress_image_packed_n")
    tail, result = _container(nb, prefix)
    if rgb:
        check(lib().jpegx_host_compress_image_rgb_n(a.ctypes.data, rows, cols, cols * 3, int(bs), int(n), mode_of(mode), float(param), *tail),
              "jpegx_host_compress_image_rgb_n")
    else:
        check(lib().jpegx_host_compress_image_packed_n(a.ctypes.data, nb, rows, cols, cols * nb, int(bs), int(n), mode_of(mode), float(param),
                                                       *tail), "jpegx_host_compress_image_packed_n")
    return result()


def compress_image_packed_n(pixels, bs, n, mode="none", param=0.0, prefix=None):
    """compress_image_packed for dct_size n: ``pixels`` is the C-contiguous (rows, cols, 1..4) uint8 array np.asarray(image)
    gives; all bands through ONE pooled device job (jpegx_host_compress_image_packed_n).  With ``prefix`` (the container
    header) the finished file -- prefix, then every band behind its '<L' byte count; without it the list of the bands' byte
    strings, each what compress_band_n returns for its band.  None when the pixels are not in that layout; JpegxError
    naming BadRleCodeError for an amplitude beyond 15 bits.  Keyword ``colour='rgb'``: the pixels are RGB and become Pillow's YCbCr
    on the device first (jpegx_host_compress_image_rgb_n)."""
    return _compress_image_packed_n(False, pixels, bs, n, mode, param, prefix)


def _decompress_image_n(rgb, blobs, rows, cols, bs, n, mode="none", param=0.0, interleave=True):
    coded = [_coded(b) for b in blobs]
    nb = len(coded)
    rows, cols = int(rows), int(cols)
    if not 1 <= nb <= 4:
        raise JpegxError("decompress_image_n takes 1..4 bands")
    _three_bands(rgb, nb, "decompress_image_n")
    if rgb and not interleave:
        raise JpegxError("decompress_image_n: colour='rgb' gives interleaved pixels")
    if rows < 1 or cols < 1 or rows * cols > 2 ** 31 - 1:      # before NumPy is asked for it
        raise JpegxError("decompress_image_n: rows and cols must be at least 1 and hold at most 2^31 - 1 samples")
    ptrs = (ctypes.c_void_p * nb)(*[c[0] for c in coded])
    sizes = (ctypes.c_size_t * nb)(*[c[1] for c in coded])
    out = np.empty((rows, cols, nb) if interleave else (nb, rows, cols), dtype=np.uint8)
    if rgb:
        check(lib().jpegx_host_decompress_image_rgb_n(ptrs, sizes, rows, cols, int(bs), int(n), mode_of(mode), float(param), out.ctypes.data, cols * 3),
              "jpegx_host_decompress_image_rgb_n")
        return out
    check(lib().jpegx_host_decompress_image_n(ptrs, sizes, nb, rows, cols, int(bs), int(n), mode_of(mode), float(param), out.ctypes.data,
                                              cols * nb if interleave else cols, 1 if interleave else 0),
          "jpegx_host_decompress_image_n")
    return out


def decompress_image_n(blobs, rows, cols, bs, n, mode="none", param=0.0, interleave=True):
    """All bands of one picture back at dct_size n in ONE pooled device job (jpegx_host_decompress_image_n): uint8
    (rows, cols, nbands) when ``interleave`` (what PIL's Image.fromarray takes), else (nbands, rows, cols); every band is
    what decompress_band_n returns for its bytes.  JpegxError when the device refuses a band's stream.  Keyword ``colour='rgb'``:
    the three bands are Y, Cb, Cr and the interleaved result is Pillow's RGB of them (jpegx_host_decompress_image_rgb_n)."""
    return _decompress_image_n(False, blobs, rows, cols, bs, n, mode, param, interleave)


compress_image_packed_n = _colour_keyword(compress_image_packed_n, functools.partial(_compress_image_packed_n, True))
decompress_image_n = _colour_keyword(decompress_image_n, functools.partial(_decompress_image_n, True))


# ---------------------------------------------------------------------------------------------
# what the device wrappers and host conveniences of the batch codec share
# ---------------------------------------------------------------------------------------------
def _entry(name, device, *args):
    """The return code of the C entry ``name``, or with a ``device`` of its ``_on`` form there.  Through lib() on every call."""
    L = lib()
    return getattr(L, name)(*args) if device is None else getattr(L, name + "_on")(int(device), *args)


def _entry_checked(name, device, *args):
    check(_entry(name, device, *args), name)


def _compress_status(name, device, nplanes, head, stream):
    """(rc, total, offsets) of a jpegx_batch_compress_status* entry, ``head`` its arguments in front of h_total: rc 0, 1 or -1
    are the entry's verdicts, anything else raises."""
    total = ctypes.c_ulonglong(0)
    off = np.zeros(int(nplanes) + 1, dtype=np.uint64)
    rc = _entry(name, device, *head, ctypes.byref(total), off.ctypes.data, stream)
    if rc not in (0, 1, -1):
        check(rc, name)
    return rc, total.value, off


def _plane_offsets(plane_offsets, nplanes, words):
    off = np.ascontiguousarray(plane_offsets, dtype=np.uint64)
    if off.shape != (int(nplanes) + 1,):
        raise JpegxError("plane_offsets must hold %s + 1 entries" % words)
    return off


def _blob_offsets(flat):
    """(offsets, total) of byte strings laid behind each other."""
    off = np.zeros(len(flat) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(b) for b in flat])
    return off, int(off[-1])


def _cut_blobs(blob, off, k, nb=None):
    """The coded stream back as k byte strings, or with ``nb`` as k lists of nb (picture-major)."""
    flat = [blob[int(off[p]):int(off[p + 1])].tobytes() for p in range(k * (nb or 1))]
    return flat if nb is None else [flat[p * nb:(p + 1) * nb] for p in range(k)]


def _picture_stack(pixels):
    src = pixels if isinstance(pixels, np.ndarray) else np.asarray(pixels)
    if src.ndim != 4 or src.size == 0 or src.dtype != np.uint8:
        raise JpegxError("expected non-empty [n][rows][cols][bands] uint8 pictures, got %r of %s" % (src.shape, src.dtype))
    return np.ascontiguousarray(src)


def _picture_list(pictures):
    pics = [p if isinstance(p, np.ndarray) else np.asarray(p) for p in pictures]
    if not pics or any(p.ndim != 3 or p.size == 0 or p.dtype != np.uint8 for p in pics) or len({p.shape[2] for p in pics}) != 1:
        raise JpegxError("expected at least one non-empty [rows][cols][bands] uint8 picture, and the same number of bands in each")
    return pics


def _picture_blobs(blobs, sizes=None):
    """(blobs as lists of bytes, pictures, bands) of what a picture compress returned; with ``sizes``, one size per picture."""
    blobs = [[bytes(b) for b in picture] for picture in blobs]
    k = len(blobs)
    nb = len(blobs[0]) if k else 0
    if k < 1 or nb < 1 or any(len(picture) != nb for picture in blobs) or (sizes is not None and len(sizes) != k):
        raise JpegxError("expected at least one picture, and the same number of bands in each" if sizes is None
                         else "expected at least one picture, the same number of bands in each, and a size for each")
    return blobs, k, nb


def _probe_answer(raw):
    """A probe's uint64 totals -> (bits 0..62, the bad-amplitude flag of bit 63)."""
    return raw & np.uint64(PROBE_BAD - 1), (raw >> np.uint64(63)).astype(bool)


def _emit_exactly(dev, status, emit, emit_name):
    """After a sizes-only compress: read the total (status() -> (rc, total, offsets)), emit into a buffer of exactly that
    (emit(d_out, cap)), check that the second verdict agrees, download.  (stream, offsets)."""
    rc, total, off = status()
    if rc != 0:
        check(rc, emit_name.replace("_emit", "_compress_status"))
    dout = dev(max(1, total))
    emit(dout.ptr, total)
    rc, total2, off = status()
    if rc != 0 or total2 != total:
        check(rc if rc else -1, emit_name)
    return dout.download((total,), np.uint8), off


# ---------------------------------------------------------------------------------------------
# batch codec on device buffers: a stack of planes -> one coded stream with a plane index, and back
# ---------------------------------------------------------------------------------------------
def batch_workspace_bytes(nplanes, height, width):
    return lib().jpegx_batch_workspace_bytes(int(nplanes), int(height), int(width))


def batch_max_bytes(nplanes, height, width):
    return lib().jpegx_batch_max_bytes(int(nplanes), int(height), int(width))


def batch_decompress_workspace_bytes(nbytes, nplanes, height, width):
    return lib().jpegx_batch_decompress_workspace_bytes(int(nbytes), int(nplanes), int(height), int(width))


def batch_compress_device(in_ptr, elem_size, nplanes, height, width, d_workspace, d_out, out_cap, mode="qtable", param=0.0,
                          flags=0, pitch=None, block_size=1, stream=None, device=None):
    """Enqueue jpegx_batch_compress: planes stacked [nplanes * height * block_size][pitch] (height, width after pooling;
    pitch in elements, default width * block_size) -> coded bytes at d_out (None: sizes only).  Verdict and plane
    index: batch_compress_status."""
    args = (in_ptr, int(elem_size), int(nplanes), int(height), int(width), int(width * block_size if pitch is None else pitch),
            int(block_size), mode_of(mode), float(param), int(flags), d_workspace, d_out, int(out_cap), stream)
    _entry_checked("jpegx_batch_compress", device, *args)


def batch_compress_status(d_workspace, nplanes, height, width, stream=None, device=None):
    """Synchronises; returns (rc, total, offsets): rc 0, 1 (did not fit the capacity of the last compress / emit) or
    JPEGX_E_INVALID (-1: an amplitude beyond 15 bits); offsets: uint64 (nplanes + 1,), the last one = total."""
    return _compress_status("jpegx_batch_compress_status", device, int(nplanes),
                            (d_workspace, int(nplanes), int(height), int(width)), stream)


def batch_emit_device(d_workspace, nplanes, height, width, d_out, out_cap, stream=None, device=None):
    args = (d_workspace, int(nplanes), int(height), int(width), d_out, int(out_cap), stream)
    _entry_checked("jpegx_batch_emit", device, *args)


def batch_decompress_device(d_bytes, plane_offsets, nplanes, height, width, d_workspace, d_out, out_pitch, block_size=1,
                            mode="qtable", param=0.0, flags=0, out_type=OUT_U8, stream=None, device=None):
    """jpegx_batch_decompress (synchronises the stream between groups and levels); plane_offsets: nplanes + 1 host
    integers.  Returns the C return code's success; raises JpegxError otherwise."""
    off = _plane_offsets(plane_offsets, int(nplanes), "nplanes")
    args = (d_bytes, off.ctypes.data, int(nplanes), int(height), int(width), int(block_size), mode_of(mode), float(param),
            int(flags), d_workspace, d_out, int(out_pitch), int(out_type), stream)
    _entry_checked("jpegx_batch_decompress", device, *args)


def batch_compress(planes, block_size=1, mode="qtable", param=0.0, pixel_input=None):
    """[n][rows][cols] uint8 or float32 planes -> list of n byte strings, each what compress_plane gives for that plane.
    Host convenience over the device entries (upload, sizes-only compress, status, emit into a buffer of exactly the
    total, download); float32 planes take block_size 1 only."""
    src = np.asarray(planes)
    bs = int(block_size)
    if src.ndim != 3 or src.shape[0] < 1:
        raise JpegxError("expected [n][rows][cols] planes, got shape %r" % (src.shape,))
    if src.dtype != np.uint8:
        src = np.ascontiguousarray(src, dtype=np.float32)
    n, hh, ww = src.shape
    if hh % (8 * bs) or ww % (8 * bs):
        raise JpegxError("planes must be a multiple of 8*block_size in both dimensions")
    h, w = hh // bs, ww // bs
    elem = 1 if src.dtype == np.uint8 else 4
    flags = 0
    if elem == 4 and (is_pixel_like(src.reshape(n * hh, ww)) if pixel_input is None else pixel_input):
        flags = F_PIXEL_INPUT
    pitch = (ww + 15) // 16 * 16 if elem == 1 else (ww + 3) // 4 * 4
    a = np.zeros((n * hh, pitch), dtype=src.dtype)
    a[:, :ww] = src.reshape(n * hh, ww)
    require_device()
    with _Buffers() as dev:
        din, dws = dev(a.nbytes), dev(batch_workspace_bytes(n, h, w))
        din.upload(a)
        batch_compress_device(din.ptr, elem, n, h, w, dws.ptr, None, 0, mode, param, flags, pitch=pitch, block_size=bs)
        blob, off = _emit_exactly(dev, lambda: batch_compress_status(dws.ptr, n, h, w),
                                  lambda d_out, cap: batch_emit_device(dws.ptr, n, h, w, d_out, cap), "jpegx_batch_emit")
        return _cut_blobs(blob, off, n)


def batch_decompress(blobs, height, width, block_size=1, mode="qtable", param=0.0, out="u8"):
    """n byte strings (one per plane, as batch_compress returns them) -> ndarray [n][height * block_size][width *
    block_size]; (height, width) = the planes AFTER pooling.  out: "u8" (clamped, replicated block_size x block_size),
    "i16" or "f32" (block_size 1)."""
    blobs = [bytes(b) for b in blobs]
    n, bs = len(blobs), int(block_size)
    if n < 1:
        raise JpegxError("expected at least one plane")
    out_type = _OUT_BY_NAME[out]
    dtype = np.dtype(_OUT_DTYPES[out_type])
    off, total = _blob_offsets(blobs)
    stream_bytes = np.zeros(total + 16, dtype=np.uint8)               # 16 zero bytes behind the stream
    stream_bytes[:total] = np.frombuffer(b"".join(blobs), dtype=np.uint8)
    pitch = (width * bs * dtype.itemsize + 15) // 16 * 16 // dtype.itemsize
    require_device()
    with _Buffers() as dev:
        din = dev(stream_bytes.nbytes)
        dws = dev(max(256, batch_decompress_workspace_bytes(total, n, height, width)))
        dout = dev(n * height * bs * pitch * dtype.itemsize)
        din.upload(stream_bytes)
        batch_decompress_device(din.ptr, off, n, height, width, dws.ptr, dout.ptr, pitch, bs, mode, param, 0, out_type)
        res = dout.download((n, height * bs, pitch), dtype)
        return np.ascontiguousarray(res[:, :, :width * bs])


# ---------------------------------------------------------------------------------------------
# the batch codec for any DCT size: a stack of 8-bit bands -> one coded stream with a plane index, and back
# ---------------------------------------------------------------------------------------------
def batch_workspace_bytes_n(nplanes, rows, cols, bs, n, group_planes=0):
    return lib().jpegx_batch_workspace_bytes_n(int(nplanes), int(rows), int(cols), int(bs), int(n), int(group_planes))


def batch_max_bytes_n(nplanes, rows, cols, bs, n):
    return lib().jpegx_batch_max_bytes_n(int(nplanes), int(rows), int(cols), int(bs), int(n))


def batch_decompress_workspace_bytes_n(nbytes, nplanes, rows, cols, bs, n, group_planes=0):
    return lib().jpegx_batch_decompress_workspace_bytes_n(int(nbytes), int(nplanes), int(rows), int(cols), int(bs), int(n),
                                                          int(group_planes))


def batch_groups_n(plane_offsets, nplanes, rows, cols, bs, n, group_planes=0):
    """The cut of a coded batch into decoding groups (jpegx_batch_groups_n; host arithmetic, no device needed): the first
    plane of every group and, last, nplanes."""
    off = _plane_offsets(plane_offsets, int(nplanes), "nplanes")
    first = np.zeros(int(nplanes) + 1, dtype=np.int32)
    ngroups = ctypes.c_int(0)
    check(lib().jpegx_batch_groups_n(off.ctypes.data, int(nplanes), int(rows), int(cols), int(bs), int(n), int(group_planes),
                                     first.ctypes.data, ctypes.byref(ngroups)), "jpegx_batch_groups_n")
    return first[:ngroups.value + 1].copy()


def band_planes_stacked_n_device(d_bands, nplanes, rows, cols, bs, n, d_out, pitch=None, out_pitch=None, stream=None, device=None):
    """Enqueue jpegx_band_planes_stacked_n: bands stacked [nplanes * rows][pitch] (default cols) -> float64 planes stacked
    [nplanes * H][out_pitch] (default W), (H, W) = band_shape_n(rows, cols, bs, n)."""
    args = (d_bands, int(nplanes), int(rows), int(cols), int(cols if pitch is None else pitch), int(bs), int(n), d_out,
            int(band_shape_n(rows, cols, bs, n)[1] if out_pitch is None else out_pitch), stream)
    _entry_checked("jpegx_band_planes_stacked_n", device, *args)


def inflate_crop_stacked_u8_device(d_planes, nplanes, height, pitch, rows, cols, bs, d_out, out_pitch=None, stream=None, device=None):
    """Enqueue jpegx_inflate_crop_stacked_u8: uint8 planes stacked [nplanes * height][pitch] -> bands stacked
    [nplanes * rows][out_pitch] (default cols)."""
    args = (d_planes, int(nplanes), int(height), int(pitch), int(rows), int(cols), int(bs), d_out,
            int(cols if out_pitch is None else out_pitch), stream)
    _entry_checked("jpegx_inflate_crop_stacked_u8", device, *args)


def batch_compress_n_device(d_bands, nplanes, rows, cols, bs, n, d_workspace, d_out, out_cap, mode="none", param=0.0,
                            group_planes=0, pitch=None, stream=None, device=None):
    """Enqueue jpegx_batch_compress_n: bands stacked [nplanes * rows][pitch] (bytes, default cols) -> coded bytes at d_out
    (None: sizes only).  Verdict and plane index: batch_compress_status_n."""
    args = (d_bands, int(nplanes), int(rows), int(cols), int(cols if pitch is None else pitch), int(bs), int(n), mode_of(mode),
            float(param), int(group_planes), d_workspace, d_out, int(out_cap), stream)
    _entry_checked("jpegx_batch_compress_n", device, *args)


def batch_compress_status_n(d_workspace, nplanes, rows, cols, bs, n, group_planes=0, stream=None, device=None):
    """Synchronises; returns (rc, total, offsets) as batch_compress_status does."""
    return _compress_status("jpegx_batch_compress_status_n", device, int(nplanes),
                            (d_workspace, int(nplanes), int(rows), int(cols), int(bs), int(n), int(group_planes)), stream)


def batch_emit_n_device(d_workspace, nplanes, rows, cols, bs, n, d_out, out_cap, group_planes=0, stream=None, device=None):
    args = (d_workspace, int(nplanes), int(rows), int(cols), int(bs), int(n), int(group_planes), d_out, int(out_cap), stream)
    _entry_checked("jpegx_batch_emit_n", device, *args)


def batch_decompress_n_device(d_bytes, plane_offsets, nplanes, rows, cols, bs, n, d_workspace, d_out, out_pitch=None, mode="none",
                              param=0.0, group_planes=0, stream=None, device=None):
    """jpegx_batch_decompress_n (synchronises the stream once per group); plane_offsets: nplanes + 1 host integers; bands
    stacked [nplanes * rows][out_pitch] (default cols) at d_out.  Raises JpegxError for whatever the entry refuses."""
    off = _plane_offsets(plane_offsets, int(nplanes), "nplanes")
    args = (d_bytes, off.ctypes.data, int(nplanes), int(rows), int(cols), int(bs), int(n), mode_of(mode), float(param),
            int(group_planes), d_workspace, d_out, int(cols if out_pitch is None else out_pitch), stream)
    _entry_checked("jpegx_batch_decompress_n", device, *args)


def batch_compress_n(bands, bs, n, mode="none", param=0.0, group_planes=0):
    """[k][rows][cols] uint8 bands -> list of k byte strings, each what compress_band_n gives for that band.  Host
    convenience over the device entries (upload, sizes-only compress, status, emit into a buffer of exactly the total,
    download).  JpegxError naming BadRleCodeError for an amplitude beyond 15 bits anywhere in the batch."""
    src = bands if isinstance(bands, np.ndarray) else np.asarray(bands)
    if src.ndim != 3 or src.size == 0 or src.dtype != np.uint8:
        raise JpegxError("expected non-empty [n][rows][cols] uint8 bands, got %r of %s" % (src.shape, src.dtype))
    src = np.ascontiguousarray(src)
    k, rows, cols = src.shape
    shape = (k, rows, cols, int(bs), int(n))
    nws = batch_workspace_bytes_n(*shape, group_planes)
    if nws == 0:                                        # the entry names the refusal, before any device is touched
        batch_compress_n_device(1, *shape, 16, None, 0, mode, param, group_planes)
    mode_of(mode)
    require_device()
    with _Buffers() as dev:
        din, dws = dev(src.nbytes), dev(nws)
        din.upload(src)
        batch_compress_n_device(din.ptr, *shape, dws.ptr, None, 0, mode, param, group_planes)
        blob, off = _emit_exactly(dev, lambda: batch_compress_status_n(dws.ptr, *shape, group_planes),
                                  lambda d_out, cap: batch_emit_n_device(dws.ptr, *shape, d_out, cap, group_planes), "jpegx_batch_emit_n")
        return _cut_blobs(blob, off, k)


def batch_decompress_n(blobs, rows, cols, bs, n, mode="none", param=0.0, group_planes=0):
    """k byte strings (one per band, as batch_compress_n or compress_band_n return them) -> uint8 [k][rows][cols], band p what
    decompress_band_n gives for blobs[p].  JpegxError naming a plane range for a stream the device refuses."""
    blobs = [bytes(b) for b in blobs]
    k = len(blobs)
    if k < 1:
        raise JpegxError("expected at least one band")
    rows, cols = int(rows), int(cols)
    off, total = _blob_offsets(blobs)
    shape = (k, rows, cols, int(bs), int(n))
    nws = batch_decompress_workspace_bytes_n(max(total, 1), *shape, group_planes)
    if nws == 0 or total == 0:                          # the entry names the refusal, before any device is touched
        batch_decompress_n_device(1, off, *shape, 16, 1, None, mode, param, group_planes)
        raise JpegxError("batch_decompress_n: empty stream")
    require_device()
    with _Buffers() as dev:
        din, dws, dout = dev(total), dev(nws), dev(k * rows * cols)
        din.upload(np.frombuffer(b"".join(blobs), dtype=np.uint8))
        batch_decompress_n_device(din.ptr, off, *shape, dws.ptr, dout.ptr, cols, mode, param, group_planes)
        return dout.download((k, rows, cols), np.uint8)


# ---------------------------------------------------------------------------------------------
# the batch codec for whole pictures at any DCT size: a stack of pixel-interleaved pictures -> the coded bytes of every
# band, picture-major, and back.  A stack of k pictures of nb bands is the band batch above of nb * k planes: workspace,
# worst case, status and emit are batch_workspace_bytes_n / batch_max_bytes_n / batch_compress_status_n / batch_emit_n_device
# with that plane count.  dct_size 8 has its own entries, at the end of this file.
# ---------------------------------------------------------------------------------------------
def _colour_flag(colour, nbands, what):
    """The C entries' ``colour``: None -> 0 (the bytes as they are), 'rgb' -> 1 (RGB pixels outside, Pillow's YCbCr inside)."""
    if colour is None:
        return 0
    if colour != "rgb":
        raise JpegxError("%s: colour must be None or 'rgb', got %r" % (what, colour))
    _three_bands(True, nbands, what)
    return 1


def batch_group_planes_pictures_n(nbands, rows, cols, bs, n):
    """The recommended group_planes of the picture entries (jpegx_batch_group_planes_pictures_n): the largest multiple of
    nbands whose planes stay within 2^26 samples, nbands at least; 0 for a shape the entries refuse."""
    return lib().jpegx_batch_group_planes_pictures_n(int(nbands), int(rows), int(cols), int(bs), int(n))


def batch_decompress_pictures_workspace_bytes_n(nbytes, npictures, nbands, rows, cols, bs, n, group_planes):
    return lib().jpegx_batch_decompress_pictures_workspace_bytes_n(int(nbytes), int(npictures), int(nbands), int(rows), int(cols),
                                                                   int(bs), int(n), int(group_planes))


def batch_groups_pictures_n(plane_offsets, npictures, nbands, rows, cols, bs, n, group_planes):
    """The cut of a coded batch of pictures into decoding groups on picture boundaries (jpegx_batch_groups_pictures_n; host
    arithmetic, no device needed): the first PICTURE of every group and, last, npictures."""
    off = _plane_offsets(plane_offsets, int(npictures) * int(nbands), "nbands * npictures")
    first = np.zeros(int(npictures) + 1, dtype=np.int32)
    ngroups = ctypes.c_int(0)
    check(lib().jpegx_batch_groups_pictures_n(off.ctypes.data, int(npictures), int(nbands), int(rows), int(cols), int(bs), int(n),
                                              int(group_planes), first.ctypes.data, ctypes.byref(ngroups)), "jpegx_batch_groups_pictures_n")
    return first[:ngroups.value + 1].copy()


def band_planes_packed_stacked_n_device(d_pixels, npictures, nbands, rows, cols, bs, n, d_out, colour=0, pitch=None, out_pitch=None,
                                        stream=None, device=None):
    """Enqueue jpegx_band_planes_packed_stacked_n: pictures stacked [npictures * rows][pitch] (bytes, default cols * nbands)
    -> float64 planes stacked picture-major [npictures * nbands * H][out_pitch] (default W); colour 0 or 1 as in the header."""
    args = (d_pixels, int(npictures), int(nbands), int(rows), int(cols), int(cols * nbands if pitch is None else pitch), int(colour),
            int(bs), int(n), d_out, int(band_shape_n(rows, cols, bs, n)[1] if out_pitch is None else out_pitch), stream)
    _entry_checked("jpegx_band_planes_packed_stacked_n", device, *args)


def inflate_crop_pack_stacked_u8_device(d_planes, npictures, nbands, height, pitch, rows, cols, bs, d_out, colour=0, out_pitch=None,
                                        stream=None, device=None):
    """Enqueue jpegx_inflate_crop_pack_stacked_u8: uint8 planes stacked [npictures * nbands * height][pitch] -> pictures
    stacked [npictures * rows][out_pitch] (bytes, default cols * nbands)."""
    args = (d_planes, int(npictures), int(nbands), int(height), int(pitch), int(rows), int(cols), int(bs), int(colour), d_out,
            int(cols * nbands if out_pitch is None else out_pitch), stream)
    _entry_checked("jpegx_inflate_crop_pack_stacked_u8", device, *args)


def batch_compress_pictures_n_device(d_pixels, npictures, nbands, rows, cols, bs, n, d_workspace, d_out, out_cap, group_planes,
                                     mode="none", param=0.0, colour=0, pitch=None, stream=None, device=None):
    """Enqueue jpegx_batch_compress_pictures_n: pictures stacked [npictures * rows][pitch] (bytes, default cols * nbands) ->
    coded bytes at d_out (None: sizes only).  Verdict and plane index: batch_compress_status_n with nbands * npictures planes."""
    args = (d_pixels, int(npictures), int(nbands), int(rows), int(cols), int(cols * nbands if pitch is None else pitch), int(colour),
            int(bs), int(n), mode_of(mode), float(param), int(group_planes), d_workspace, d_out, int(out_cap), stream)
    _entry_checked("jpegx_batch_compress_pictures_n", device, *args)


def batch_decompress_pictures_n_device(d_bytes, plane_offsets, npictures, nbands, rows, cols, bs, n, d_workspace, d_out, group_planes,
                                       out_pitch=None, mode="none", param=0.0, colour=0, stream=None, device=None):
    """jpegx_batch_decompress_pictures_n (synchronises the stream once per group); plane_offsets: nbands * npictures + 1 host
    integers; pictures stacked [npictures * rows][out_pitch] (default cols * nbands) at d_out.  Raises JpegxError for whatever
    the entry refuses."""
    off = _plane_offsets(plane_offsets, int(npictures) * int(nbands), "nbands * npictures")
    args = (d_bytes, off.ctypes.data, int(npictures), int(nbands), int(rows), int(cols), int(bs), int(n), mode_of(mode), float(param),
            int(colour), int(group_planes), d_workspace, d_out, int(cols * nbands if out_pitch is None else out_pitch), stream)
    _entry_checked("jpegx_batch_decompress_pictures_n", device, *args)


def batch_compress_pictures_n(pixels, bs, n, mode="none", param=0.0, colour=None, group_planes=None):
    """uint8 pictures [k][rows][cols][nb] -> a list of k lists of nb byte strings, each what compress_band_n gives for that band
    of that picture (with colour='rgb': of the picture's Pillow YCbCr).  Host convenience over the device entries (upload,
    sizes-only compress, status, emit into a buffer of exactly the total, download).  group_planes None: the recommended
    value.  JpegxError naming BadRleCodeError for an amplitude beyond 15 bits anywhere in the batch."""
    src = _picture_stack(pixels)
    k, rows, cols, nb = src.shape
    flag = _colour_flag(colour, nb, "batch_compress_pictures_n")
    if group_planes is None:
        group_planes = batch_group_planes_pictures_n(nb, rows, cols, bs, n) or nb
    pics, planes = (k, nb, rows, cols, int(bs), int(n)), (k * nb, rows, cols, int(bs), int(n))
    nws = batch_workspace_bytes_n(*planes, group_planes) if group_planes > 0 and group_planes % nb == 0 else 0
    if nws == 0:                                        # the entry names the refusal, before any device is touched
        batch_compress_pictures_n_device(1, *pics, 16, None, 0, group_planes, mode, param, flag)
        raise JpegxError("batch_compress_pictures_n: the batch was refused")
    mode_of(mode)
    require_device()
    with _Buffers() as dev:
        din, dws = dev(src.nbytes), dev(nws)
        din.upload(src)
        batch_compress_pictures_n_device(din.ptr, *pics, dws.ptr, None, 0, group_planes, mode, param, flag)
        blob, off = _emit_exactly(dev, lambda: batch_compress_status_n(dws.ptr, *planes, group_planes),
                                  lambda d_out, cap: batch_emit_n_device(dws.ptr, *planes, d_out, cap, group_planes), "jpegx_batch_emit_n")
        return _cut_blobs(blob, off, k, nb)


def batch_decompress_pictures_n(blobs, rows, cols, bs, n, mode="none", param=0.0, colour=None, group_planes=None):
    """k lists of nb byte strings (as batch_compress_pictures_n returns them) -> uint8 [k][rows][cols][nb], picture p the
    np.dstack of what decompress_band_n gives for its bands (with colour='rgb': Pillow's RGB of that).  JpegxError naming a
    picture range for a stream the device refuses."""
    blobs, k, nb = _picture_blobs(blobs)
    flag = _colour_flag(colour, nb, "batch_decompress_pictures_n")
    rows, cols = int(rows), int(cols)
    if group_planes is None:
        group_planes = batch_group_planes_pictures_n(nb, rows, cols, bs, n) or nb
    flat = [b for picture in blobs for b in picture]
    off, total = _blob_offsets(flat)
    pics = (k, nb, rows, cols, int(bs), int(n))
    nws = batch_decompress_pictures_workspace_bytes_n(max(total, 1), *pics, group_planes)
    if nws == 0 or total == 0:                          # the entry names the refusal, before any device is touched
        batch_decompress_pictures_n_device(1, off, *pics, 16, 1, group_planes, None, mode, param, flag)
        raise JpegxError("batch_decompress_pictures_n: empty stream")
    require_device()
    with _Buffers() as dev:
        din, dws, dout = dev(total), dev(nws), dev(k * rows * cols * nb)
        din.upload(np.frombuffer(b"".join(flat), dtype=np.uint8))
        batch_decompress_pictures_n_device(din.ptr, off, *pics, dws.ptr, dout.ptr, group_planes, None, mode, param, flag)
        return dout.download((k, rows, cols, nb), np.uint8)


# ---------------------------------------------------------------------------------------------
# the size probe: what every plane would weigh under each of K candidate quantiser parameters, in one pass over the planes
# (csrc/jpegx_probe_n.hip) -- no coefficient stream, no per-candidate compression.  dct_size 2..32 through the run-time-N kernels.
# ---------------------------------------------------------------------------------------------
PROBE_MAX_CANDIDATES = 32
PROBE_BAD = 1 << 63                                     # bit 63 of a total: an amplitude beyond 15 bits (BadRleCodeError)


def _probe_params(params):
    """The candidates as a host float64 array (kept alive by the caller for the length of the call) and their count."""
    h = np.ascontiguousarray(np.atleast_1d(np.asarray(params, dtype=np.float64)).ravel())
    return h, int(h.size)


def probe_sizes_n_device(d_planes, nplanes, height, width, n, mode, params, d_totals, pitch=None, stream=None, device=None):
    """Enqueue jpegx_probe_sizes_n: nplanes float64 planes stacked [nplanes * height][pitch] (elements, default width) ->
    uint64 d_totals [nplanes][K]: bits 0..62 the coded bytes of the plane under candidate q, bit 63 the bad-amplitude flag.
    ``params``: the K candidates (host numbers)."""
    h, k = _probe_params(params)
    args = (d_planes, int(nplanes), int(height), int(width), int(width if pitch is None else pitch), int(n), mode_of(mode),
            h.ctypes.data, k, d_totals, stream)
    _entry_checked("jpegx_probe_sizes_n", device, *args)


def batch_probe_pictures_workspace_bytes_n(npictures, nbands, rows, cols, bs, n, group_planes):
    return lib().jpegx_batch_probe_pictures_workspace_bytes_n(int(npictures), int(nbands), int(rows), int(cols), int(bs), int(n),
                                                              int(group_planes))


def batch_probe_pictures_n_device(d_pixels, npictures, nbands, rows, cols, bs, n, mode, params, group_planes, d_workspace, d_totals,
                                  colour=0, pitch=None, stream=None, device=None):
    """Enqueue jpegx_batch_probe_pictures_n: pictures stacked [npictures * rows][pitch] (bytes, default cols * nbands) ->
    uint64 d_totals [nbands * npictures][K], plane-major in the batch's picture-major plane order."""
    h, k = _probe_params(params)
    args = (d_pixels, int(npictures), int(nbands), int(rows), int(cols), int(cols * nbands if pitch is None else pitch), int(colour),
            int(bs), int(n), mode_of(mode), h.ctypes.data, k, int(group_planes), d_workspace, d_totals, stream)
    _entry_checked("jpegx_batch_probe_pictures_n", device, *args)


def batch_probe_pictures_n(pixels, bs, n, mode, params, colour=None, group_planes=None):
    """uint8 pictures [k][rows][cols][nb] -> (sizes, bad): sizes uint64 [k][nb][K], the length of band b of picture p as
    batch_compress_pictures_n would code it under candidate q; bad bool [k][nb][K], True where that band holds an amplitude
    beyond 15 bits under that candidate (its size is then meaningless).  Host convenience: upload, probe, one download.
    group_planes None: the recommended value."""
    src = _picture_stack(pixels)
    k, rows, cols, nb = src.shape
    flag = _colour_flag(colour, nb, "batch_probe_pictures_n")
    if group_planes is None:
        group_planes = batch_group_planes_pictures_n(nb, rows, cols, bs, n) or nb
    h, nk = _probe_params(params)
    pics = (k, nb, rows, cols, int(bs), int(n))
    nws = batch_probe_pictures_workspace_bytes_n(*pics, group_planes)
    if nws == 0 or not 1 <= nk <= PROBE_MAX_CANDIDATES:     # the entry names the refusal, before any device is touched
        batch_probe_pictures_n_device(1, *pics, mode, h, group_planes, 16, 8, flag)
        raise JpegxError("batch_probe_pictures_n: the batch was refused")
    mode_of(mode)
    require_device()
    with _Buffers() as dev:
        din, dws, dtot = dev(src.nbytes), dev(nws), dev(k * nb * nk * 8)
        din.upload(src)
        batch_probe_pictures_n_device(din.ptr, *pics, mode, h, group_planes, dws.ptr, dtot.ptr, flag)
        raw = dtot.download((k, nb, nk), np.uint64)
    return _probe_answer(raw)


# ---------------------------------------------------------------------------------------------
# the distortion probe: what every decoded band would lose (sum of squared differences over its pixels) under each of K
# candidate quantiser parameters, in one pass over the planes (csrc/jpegx_distort_n.hip) -- no coefficient stream, no decoded
# plane, no per-candidate round trip.  dct_size 2..32 through the run-time-N kernels, stacks of pictures of one size.
# ---------------------------------------------------------------------------------------------
def band_moments_packed_stacked_n_device(d_pixels, npictures, nbands, rows, cols, bs, n, d_moments, colour=0, pitch=None, out_pitch=None,
                                         stream=None, device=None):
    """Enqueue jpegx_band_moments_packed_stacked_n: pictures stacked [npictures * rows][pitch] (bytes, default cols * nbands)
    -> uint64 words stacked picture-major [npictures * nbands * H][out_pitch] (default W), S2 << 32 | S1 of every sample's live
    pixels; colour 0 or 1 as in the header."""
    args = (d_pixels, int(npictures), int(nbands), int(rows), int(cols), int(cols * nbands if pitch is None else pitch), int(colour),
            int(bs), int(n), d_moments, int(band_shape_n(rows, cols, bs, n)[1] if out_pitch is None else out_pitch), stream)
    _entry_checked("jpegx_band_moments_packed_stacked_n", device, *args)


def probe_distortion_n_device(d_planes, d_moments, nplanes, height, width, n, bs, rows, cols, mode, params, d_totals, pitch=None, mpitch=None,
                              stream=None, device=None):
    """Enqueue jpegx_probe_distortion_n: nplanes float64 planes stacked [nplanes * height][pitch] and their moments
    [nplanes * height][mpitch] (elements, default width), every plane a rows x cols band pooled bs x bs -> uint64 d_totals
    [nplanes][K]: bits 0..62 the sum of squared differences of the band under candidate q, bit 63 the bad-amplitude flag."""
    h, k = _probe_params(params)
    args = (d_planes, d_moments, int(nplanes), int(height), int(width), int(width if pitch is None else pitch),
            int(width if mpitch is None else mpitch), int(n), int(bs), int(rows), int(cols), mode_of(mode), h.ctypes.data, k, d_totals, stream)
    _entry_checked("jpegx_probe_distortion_n", device, *args)


def batch_probe_distortion_pictures_workspace_bytes_n(npictures, nbands, rows, cols, bs, n, group_planes):
    return lib().jpegx_batch_probe_distortion_pictures_workspace_bytes_n(int(npictures), int(nbands), int(rows), int(cols), int(bs), int(n),
                                                                         int(group_planes))


def batch_probe_distortion_pictures_n_device(d_pixels, npictures, nbands, rows, cols, bs, n, mode, params, group_planes, d_workspace, d_totals,
                                             colour=0, pitch=None, stream=None, device=None):
    """Enqueue jpegx_batch_probe_distortion_pictures_n: pictures stacked [npictures * rows][pitch] (bytes, default cols * nbands)
    -> uint64 d_totals [nbands * npictures][K], plane-major in the batch's picture-major plane order."""
    h, k = _probe_params(params)
    args = (d_pixels, int(npictures), int(nbands), int(rows), int(cols), int(cols * nbands if pitch is None else pitch), int(colour),
            int(bs), int(n), mode_of(mode), h.ctypes.data, k, int(group_planes), d_workspace, d_totals, stream)
    _entry_checked("jpegx_batch_probe_distortion_pictures_n", device, *args)


def batch_probe_distortion_pictures_n(pixels, bs, n, mode, params, colour=None, group_planes=None):
    """uint8 pictures [k][rows][cols][nb] -> (sse, bad): sse uint64 [k][nb][K], the sum of squared differences between band b of
    picture p and what batch_decompress_pictures_n gives back of batch_compress_pictures_n's bytes under candidate q (with
    colour='rgb': in the coded YCbCr bands); bad bool [k][nb][K], True where that band holds an amplitude beyond 15 bits under
    that candidate (it cannot be coded; its sum is then meaningless).  Host convenience: upload, probe, one download.
    group_planes None: the recommended value."""
    src = _picture_stack(pixels)
    k, rows, cols, nb = src.shape
    flag = _colour_flag(colour, nb, "batch_probe_distortion_pictures_n")
    if group_planes is None:
        group_planes = batch_group_planes_pictures_n(nb, rows, cols, bs, n) or nb
    h, nk = _probe_params(params)
    pics = (k, nb, rows, cols, int(bs), int(n))
    nws = batch_probe_distortion_pictures_workspace_bytes_n(*pics, group_planes)
    if nws == 0 or not 1 <= nk <= PROBE_MAX_CANDIDATES:     # the entry names the refusal, before any device is touched
        batch_probe_distortion_pictures_n_device(1, *pics, mode, h, group_planes, 16, 8, flag)
        raise JpegxError("batch_probe_distortion_pictures_n: the batch was refused")
    mode_of(mode)
    require_device()
    with _Buffers() as dev:
        din, dws, dtot = dev(src.nbytes), dev(nws), dev(k * nb * nk * 8)
        din.upload(src)
        batch_probe_distortion_pictures_n_device(din.ptr, *pics, mode, h, group_planes, dws.ptr, dtot.ptr, flag)
        raw = dtot.download((k, nb, nk), np.uint64)
    return _probe_answer(raw)


# ---------------------------------------------------------------------------------------------
# the batch codec for a SET of pictures of unequal sizes at any DCT size but 8: each picture at its own place in one device
# buffer, described by a table (jpegx_picture_set_table) that the entries take twice, as the host blob and as its device copy.
# ---------------------------------------------------------------------------------------------
PICTURE_DESC_DTYPE = np.dtype([("rows", np.int32), ("cols", np.int32), ("offset", np.uint64), ("pitch", np.int64)])
PICTURE_SET_HEAD_DTYPE = np.dtype([("magic", np.uint32), ("npictures", np.int32), ("nbands", np.int32), ("bs", np.int32), ("N", np.int32),
                                   ("pad", np.int32), ("total_blocks", np.int64)])
PICTURE_SET_ENTRY_DTYPE = np.dtype([("offset", np.uint64), ("pitch", np.int64), ("first", np.int64), ("lanes", np.int64), ("rows", np.int32),
                                    ("cols", np.int32), ("H", np.int32), ("W", np.int32), ("prows", np.int32), ("pcols", np.int32),
                                    ("wb", np.int32), ("nb", np.int32)])


class PictureSetTable:
    """The host blob of jpegx_picture_set_table with views of its three parts: ``head`` (one record), ``entries`` (npictures + 1
    records, the last the end) and ``plane_first`` (nbands * npictures + 1 block indices).  ``blob`` is what is uploaded."""

    def __init__(self, blob, npictures, nbands, total_blocks):
        self.blob, self.npictures, self.nbands, self.total_blocks = blob, int(npictures), int(nbands), int(total_blocks)
        raw = blob.view(np.uint8)
        self.head = raw[:32].view(PICTURE_SET_HEAD_DTYPE)[0]
        self.entries = raw[32:32 + 64 * (self.npictures + 1)].view(PICTURE_SET_ENTRY_DTYPE)
        at = 32 + 64 * (self.npictures + 1)
        self.plane_first = raw[at:at + 8 * (self.npictures * self.nbands + 1)].view(np.int64)
        self.nbytes = at + 8 * (self.npictures * self.nbands + 1)       # what the kernels read; the blob may be longer

    @property
    def ptr(self):
        return self.blob.ctypes.data


def picture_set_table(sizes, nbands, bs, n, offsets=None, pitches=None):
    """The table of a set of pictures (jpegx_picture_set_table; host arithmetic, no device needed).  sizes: (rows, cols) per
    picture; offsets: the byte offset of each picture's first pixel in one device buffer (default: the pictures back to
    back); pitches: bytes from a row to the next (default cols * nbands).  Raises JpegxError for whatever the entry refuses."""
    sizes = [(int(r), int(c)) for r, c in sizes]
    k = len(sizes)
    desc = np.zeros(max(k, 1), dtype=PICTURE_DESC_DTYPE)
    if pitches is None:
        pitches = [c * int(nbands) for _, c in sizes]
    if offsets is None:
        offsets = np.concatenate([[0], np.cumsum([r * int(p) for (r, _), p in zip(sizes, pitches)], dtype=np.int64)])[:k]
    for p, ((r, c), o, q) in enumerate(zip(sizes, offsets, pitches)):
        desc[p] = (r, c, int(o), int(q))
    blob = np.zeros(max(lib().jpegx_picture_set_table_bytes(k), 8) // 8, dtype=np.uint64)
    total = ctypes.c_longlong(0)
    check(lib().jpegx_picture_set_table(desc.ctypes.data, k, int(nbands), int(bs), int(n), blob.ctypes.data, ctypes.byref(total)),
          "jpegx_picture_set_table")
    return PictureSetTable(blob, k, nbands, total.value)


def batch_set_workspace_bytes_n(table, group_samples=0):
    return lib().jpegx_batch_set_workspace_bytes_n(table.ptr, int(group_samples))


def batch_set_max_bytes_n(table):
    return lib().jpegx_batch_set_max_bytes_n(table.ptr)


def batch_decompress_set_workspace_bytes_n(nbytes, table, group_samples=0):
    return lib().jpegx_batch_decompress_set_workspace_bytes_n(int(nbytes), table.ptr, int(group_samples))


def batch_groups_set_n(plane_offsets, table, group_samples=0):
    """The cut of a coded set into decoding groups on picture boundaries (jpegx_batch_groups_set_n; host arithmetic): the first
    PICTURE of every group and, last, npictures."""
    off = _plane_offsets(plane_offsets, table.npictures * table.nbands, "nbands * npictures")
    first = np.zeros(table.npictures + 1, dtype=np.int32)
    ngroups = ctypes.c_int(0)
    check(lib().jpegx_batch_groups_set_n(off.ctypes.data, table.ptr, int(group_samples), first.ctypes.data, ctypes.byref(ngroups)),
          "jpegx_batch_groups_set_n")
    return first[:ngroups.value + 1].copy()


def picture_set_blocks_n_device(d_pixels, table, d_table, p0, k, d_strip, colour=0, stream=None, device=None):
    """Enqueue jpegx_picture_set_blocks_n: pixels of pictures p0 .. p0 + k - 1 -> their float64 block strip at d_strip."""
    args = (d_pixels, table.ptr, d_table, int(p0), int(k), int(colour), d_strip, stream)
    _entry_checked("jpegx_picture_set_blocks_n", device, *args)


def picture_set_pixels_u8_device(d_strip, table, d_table, p0, k, d_out, colour=0, stream=None, device=None):
    """Enqueue jpegx_picture_set_pixels_u8: the uint8 block strip of pictures p0 .. p0 + k - 1 -> their pixels in d_out."""
    args = (d_strip, table.ptr, d_table, int(p0), int(k), int(colour), d_out, stream)
    _entry_checked("jpegx_picture_set_pixels_u8", device, *args)


def batch_compress_picture_set_n_device(d_pixels, table, d_table, d_workspace, d_out, out_cap, mode="none", param=0.0, colour=0,
                                        group_samples=0, stream=None, device=None):
    """Enqueue jpegx_batch_compress_picture_set_n -> coded bytes at d_out (None: sizes only).  Verdict and plane index:
    batch_compress_status_set_n."""
    args = (d_pixels, table.ptr, d_table, int(colour), mode_of(mode), float(param), int(group_samples), d_workspace, d_out, int(out_cap), stream)
    _entry_checked("jpegx_batch_compress_picture_set_n", device, *args)


def batch_compress_status_set_n(d_workspace, table, group_samples=0, stream=None, device=None):
    """Synchronises; returns (rc, total, offsets) as batch_compress_status_n does."""
    return _compress_status("jpegx_batch_compress_status_set_n", device, table.npictures * table.nbands,
                            (d_workspace, table.ptr, int(group_samples)), stream)


def batch_emit_set_n_device(d_workspace, table, d_table, d_out, out_cap, group_samples=0, stream=None, device=None):
    args = (d_workspace, table.ptr, d_table, int(group_samples), d_out, int(out_cap), stream)
    _entry_checked("jpegx_batch_emit_set_n", device, *args)


def batch_decompress_picture_set_n_device(d_bytes, plane_offsets, table, d_table, d_workspace, d_out, mode="none", param=0.0, colour=0,
                                          group_samples=0, stream=None, device=None):
    """jpegx_batch_decompress_picture_set_n (synchronises the stream once per group); plane_offsets: nbands * npictures + 1 host
    integers; every picture at its offset and pitch in d_out.  Raises JpegxError for whatever the entry refuses."""
    off = _plane_offsets(plane_offsets, table.npictures * table.nbands, "nbands * npictures")
    args = (d_bytes, off.ctypes.data, table.ptr, d_table, mode_of(mode), float(param), int(colour), int(group_samples), d_workspace, d_out, stream)
    _entry_checked("jpegx_batch_decompress_picture_set_n", device, *args)


def batch_compress_picture_set_n(pictures, bs, n, mode="none", param=0.0, colour=None, group_samples=0):
    """A sequence of uint8 pictures [rows_p][cols_p][nb], sizes as they come -> per picture the list of its nb bands' bytes, each
    what compress_band_n gives for that band of that picture (with colour='rgb': of the picture's Pillow YCbCr).  Host
    convenience over the device entries (ONE flat upload, sizes-only compress, status, emit into a buffer of exactly the total,
    download).  JpegxError naming BadRleCodeError for an amplitude beyond 15 bits anywhere in the set."""
    pics = _picture_list(pictures)
    nb = pics[0].shape[2]
    flag = _colour_flag(colour, nb, "batch_compress_picture_set_n")
    table = picture_set_table([p.shape[:2] for p in pics], nb, bs, n)      # names the refusal, before any device is touched
    mode_of(mode)
    nws = batch_set_workspace_bytes_n(table, group_samples)
    if nws == 0:
        batch_compress_picture_set_n_device(1, table, 8, 16, None, 0, mode, param, flag, group_samples)
        raise JpegxError("batch_compress_picture_set_n: the set was refused")
    require_device()
    flat = np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in pics])
    with _Buffers() as dev:
        din, dtab, dws = dev(flat.nbytes), dev(table.nbytes), dev(nws)
        din.upload(flat)
        dtab.upload(table.blob.view(np.uint8)[:table.nbytes])
        batch_compress_picture_set_n_device(din.ptr, table, dtab.ptr, dws.ptr, None, 0, mode, param, flag, group_samples)
        blob, off = _emit_exactly(dev, lambda: batch_compress_status_set_n(dws.ptr, table, group_samples),
                                  lambda d_out, cap: batch_emit_set_n_device(dws.ptr, table, dtab.ptr, d_out, cap, group_samples), "jpegx_batch_emit_set_n")
        return _cut_blobs(blob, off, len(pics), nb)


def batch_decompress_picture_set_n(blobs, sizes, bs, n, mode="none", param=0.0, colour=None, group_samples=0):
    """k lists of nb byte strings (as batch_compress_picture_set_n returns them) and the k (rows, cols) -> a list of uint8 arrays
    [rows_p][cols_p][nb], picture p the np.dstack of what decompress_band_n gives for its bands (with colour='rgb': Pillow's RGB
    of that).  JpegxError naming a picture range for a stream the device refuses."""
    sizes = [(int(r), int(c)) for r, c in sizes]
    blobs, k, nb = _picture_blobs(blobs, sizes)
    flag = _colour_flag(colour, nb, "batch_decompress_picture_set_n")
    table = picture_set_table(sizes, nb, bs, n)
    mode_of(mode)
    flat = [b for picture in blobs for b in picture]
    off, total = _blob_offsets(flat)
    nws = batch_decompress_set_workspace_bytes_n(max(total, 1), table, group_samples)
    if nws == 0 or total == 0:                          # the entry names the refusal, before any device is touched
        batch_decompress_picture_set_n_device(1, off, table, 8, 16, 1, mode, param, flag, group_samples)
        raise JpegxError("batch_decompress_picture_set_n: empty stream")
    require_device()
    nout = sum(r * c * nb for r, c in sizes)
    with _Buffers() as dev:
        din, dtab, dws, dout = dev(total), dev(table.nbytes), dev(nws), dev(nout)
        din.upload(np.frombuffer(b"".join(flat), dtype=np.uint8))
        dtab.upload(table.blob.view(np.uint8)[:table.nbytes])
        batch_decompress_picture_set_n_device(din.ptr, off, table, dtab.ptr, dws.ptr, dout.ptr, mode, param, flag, group_samples)
        out = dout.download((nout,), np.uint8)
    at = np.concatenate([[0], np.cumsum([r * c * nb for r, c in sizes])])
    return [out[int(at[p]):int(at[p + 1])].reshape(r, c, nb) for p, (r, c) in enumerate(sizes)]


# the size probe over a set: planes of unequal block counts through the probe's kernel, which looks a block's plane up in the
# table's device array of first blocks (csrc/jpegx_probe_n.hip, k_probe_n<true>)
def probe_sizes_set_n_device(d_strip, table, d_table, p0, k, mode, params, d_totals, stream=None, device=None):
    """Enqueue jpegx_probe_sizes_set_n: the float64 block strip of pictures p0 .. p0 + k - 1 (picture_set_blocks_n_device) ->
    uint64 d_totals [k * nbands][K] in the table's plane order: bits 0..62 the coded bytes of the plane under candidate q, bit
    63 the bad-amplitude flag.  ``params``: the K candidates (host numbers)."""
    h, nk = _probe_params(params)
    args = (d_strip, table.ptr, d_table, int(p0), int(k), mode_of(mode), h.ctypes.data, nk, d_totals, stream)
    _entry_checked("jpegx_probe_sizes_set_n", device, *args)


def batch_probe_picture_set_workspace_bytes_n(table, group_samples=0):
    return lib().jpegx_batch_probe_picture_set_workspace_bytes_n(table.ptr, int(group_samples))


def batch_probe_picture_set_n_device(d_pixels, table, d_table, mode, params, d_workspace, d_totals, colour=0, group_samples=0, stream=None,
                                     device=None):
    """Enqueue jpegx_batch_probe_picture_set_n: every picture at its offset in d_pixels -> uint64 d_totals
    [npictures * nbands][K] in the table's plane order."""
    h, nk = _probe_params(params)
    args = (d_pixels, table.ptr, d_table, int(colour), mode_of(mode), h.ctypes.data, nk, int(group_samples), d_workspace, d_totals, stream)
    _entry_checked("jpegx_batch_probe_picture_set_n", device, *args)


def batch_probe_picture_set_n(pictures, bs, n, mode, params, colour=None, group_samples=0):
    """A sequence of uint8 pictures [rows_p][cols_p][nb], sizes as they come -> (sizes, bad): sizes uint64 [npictures][nb][K],
    the length of band b of picture p as batch_compress_picture_set_n would code it under candidate q; bad bool of the same
    shape, True where that band holds an amplitude beyond 15 bits under that candidate (its size is then meaningless).  Host
    convenience: ONE flat upload, the probe, one download.  JpegxError for more than 32 candidates."""
    pics = _picture_list(pictures)
    nb = pics[0].shape[2]
    flag = _colour_flag(colour, nb, "batch_probe_picture_set_n")
    table = picture_set_table([p.shape[:2] for p in pics], nb, bs, n)      # names the refusal, before any device is touched
    h, nk = _probe_params(params)
    nws = batch_probe_picture_set_workspace_bytes_n(table, group_samples)
    if nws == 0 or not 1 <= nk <= PROBE_MAX_CANDIDATES:     # the entry names the refusal, before any device is touched
        batch_probe_picture_set_n_device(1, table, 8, mode, h, 16, 8, flag, group_samples)
        raise JpegxError("batch_probe_picture_set_n: the set was refused")
    mode_of(mode)
    require_device()
    flat = np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in pics])
    with _Buffers() as dev:
        din, dtab, dws, dtot = dev(flat.nbytes), dev(table.nbytes), dev(nws), dev(len(pics) * nb * nk * 8)
        din.upload(flat)
        dtab.upload(table.blob.view(np.uint8)[:table.nbytes])
        batch_probe_picture_set_n_device(din.ptr, table, dtab.ptr, mode, h, dws.ptr, dtot.ptr, flag, group_samples)
        raw = dtot.download((len(pics), nb, nk), np.uint64)
    return _probe_answer(raw)


# the distortion probe over a set: the moments gathered onto the block strip, and the probe's kernel with a block's plane, its
# place in the band and the band's size looked up in the table (csrc/jpegx_distort_n.hip, k_distort_n<true>)
def picture_set_moments_n_device(d_pixels, table, d_table, p0, k, d_moments, colour=0, stream=None, device=None):
    """Enqueue jpegx_picture_set_moments_n: pixels of pictures p0 .. p0 + k - 1 -> uint64 words S2 << 32 | S1 over the live pixels
    of every sample's tile, in the block and element order of picture_set_blocks_n_device, at d_moments (16-byte aligned)."""
    args = (d_pixels, table.ptr, d_table, int(p0), int(k), int(colour), d_moments, stream)
    _entry_checked("jpegx_picture_set_moments_n", device, *args)


def probe_distortion_set_n_device(d_strip, d_moments, table, d_table, p0, k, mode, params, d_totals, stream=None, device=None):
    """Enqueue jpegx_probe_distortion_set_n: the float64 block strip of pictures p0 .. p0 + k - 1 and their moments ->
    uint64 d_totals [k * nbands][K] in the table's plane order: bits 0..62 the band's sum of squared differences over its own
    rows x cols pixels under candidate q, bit 63 the bad-amplitude flag.  ``params``: the K candidates (host numbers)."""
    h, nk = _probe_params(params)
    args = (d_strip, d_moments, table.ptr, d_table, int(p0), int(k), mode_of(mode), h.ctypes.data, nk, d_totals, stream)
    _entry_checked("jpegx_probe_distortion_set_n", device, *args)


def batch_probe_distortion_picture_set_workspace_bytes_n(table, group_samples=0):
    return lib().jpegx_batch_probe_distortion_picture_set_workspace_bytes_n(table.ptr, int(group_samples))


def batch_probe_distortion_picture_set_n_device(d_pixels, table, d_table, mode, params, d_workspace, d_totals, colour=0, group_samples=0,
                                                stream=None, device=None):
    """Enqueue jpegx_batch_probe_distortion_picture_set_n: every picture at its offset in d_pixels -> uint64 d_totals
    [npictures * nbands][K] in the table's plane order."""
    h, nk = _probe_params(params)
    args = (d_pixels, table.ptr, d_table, int(colour), mode_of(mode), h.ctypes.data, nk, int(group_samples), d_workspace, d_totals, stream)
    _entry_checked("jpegx_batch_probe_distortion_picture_set_n", device, *args)


def batch_probe_distortion_picture_set_n(pictures, bs, n, mode, params, colour=None, group_samples=0):
    """A sequence of uint8 pictures [rows_p][cols_p][nb], sizes as they come -> (sse, bad): sse uint64 [npictures][nb][K], the
    sum over band b of picture p of (pixel - decoded pixel)^2 after batch_compress_picture_set_n and
    batch_decompress_picture_set_n under candidate q (with colour='rgb': between the YCbCr bands); bad bool of the same shape,
    True where that band holds an amplitude beyond 15 bits under that candidate (it cannot be coded; its sum is then
    meaningless).  Host convenience: ONE flat upload, the probe, one download.  JpegxError for more than 32 candidates."""
    pics = _picture_list(pictures)
    nb = pics[0].shape[2]
    flag = _colour_flag(colour, nb, "batch_probe_distortion_picture_set_n")
    table = picture_set_table([p.shape[:2] for p in pics], nb, bs, n)      # names the refusal, before any device is touched
    h, nk = _probe_params(params)
    nws = batch_probe_distortion_picture_set_workspace_bytes_n(table, group_samples)
    if nws == 0 or not 1 <= nk <= PROBE_MAX_CANDIDATES:     # the entry names the refusal, before any device is touched
        batch_probe_distortion_picture_set_n_device(1, table, 8, mode, h, 16, 8, flag, group_samples)
        raise JpegxError("batch_probe_distortion_picture_set_n: the set was refused")
    mode_of(mode)
    require_device()
    flat = np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in pics])
    with _Buffers() as dev:
        din, dtab, dws, dtot = dev(flat.nbytes), dev(table.nbytes), dev(nws), dev(len(pics) * nb * nk * 8)
        din.upload(flat)
        dtab.upload(table.blob.view(np.uint8)[:table.nbytes])
        batch_probe_distortion_picture_set_n_device(din.ptr, table, dtab.ptr, mode, h, dws.ptr, dtot.ptr, flag, group_samples)
        raw = dtot.download((len(pics), nb, nk), np.uint64)
    return _probe_answer(raw)


# ---------------------------------------------------------------------------------------------
# the batch codec for whole pictures at dct_size 8: the same stack of pictures through the 8x8 batch.  k pictures of nb bands
# are the 8x8 batch of nb * k planes of (h, w) = padded_shape(rows, cols, block_size): verdicts, plane index and emit are
# batch_compress_status / batch_emit_device with that plane count, the worst case batch_max_bytes.
# ---------------------------------------------------------------------------------------------
def batch_pictures_workspace_bytes(npictures, nbands, rows, cols, block_size, group_planes):
    return lib().jpegx_batch_pictures_workspace_bytes(int(npictures), int(nbands), int(rows), int(cols), int(block_size), int(group_planes))


def batch_decompress_pictures_workspace_bytes(nbytes, npictures, nbands, rows, cols, block_size):
    return lib().jpegx_batch_decompress_pictures_workspace_bytes(int(nbytes), int(npictures), int(nbands), int(rows), int(cols),
                                                                 int(block_size))


def picture_planes_stacked_u8_device(d_pixels, npictures, nbands, rows, cols, block_size, d_out, out_pitch, colour=0, pitch=None,
                                     stream=None, device=None):
    """Enqueue jpegx_picture_planes_stacked_u8: pictures stacked [npictures * rows][pitch] (bytes, default cols * nbands) ->
    padded raw uint8 planes stacked picture-major [npictures * nbands * H * block_size][out_pitch]."""
    args = (d_pixels, int(npictures), int(nbands), int(rows), int(cols), int(cols * nbands if pitch is None else pitch), int(colour),
            int(block_size), d_out, int(out_pitch), stream)
    _entry_checked("jpegx_picture_planes_stacked_u8", device, *args)


def picture_planes_stacked_u8(pixels, block_size=1, colour=None):
    """jpegx_picture_planes_stacked_u8 on a host array (test convenience, like pad_edges): uint8 pictures
    [k][rows][cols][nb] -> the padded raw planes [k][nb][H * block_size][W * block_size], (H, W) = padded_shape(rows, cols,
    block_size); with colour='rgb' of the pictures' Pillow YCbCr."""
    src = np.ascontiguousarray(pixels)
    if src.ndim != 4 or src.size == 0 or src.dtype != np.uint8:
        raise JpegxError("expected non-empty [n][rows][cols][bands] uint8 pictures, got %r of %s" % (src.shape, src.dtype))
    k, rows, cols, nb = src.shape
    bs = int(block_size)
    flag = _colour_flag(colour, nb, "picture_planes_stacked_u8")
    h, w = padded_shape(rows, cols, bs)
    pitch = (w * bs + 15) // 16 * 16
    require_device()
    with _Buffers() as dev:
        din, dout = dev(src.nbytes), dev(k * nb * h * bs * pitch)
        din.upload(src)
        picture_planes_stacked_u8_device(din.ptr, k, nb, rows, cols, bs, dout.ptr, pitch, flag)
        out = dout.download((k, nb, h * bs, pitch), np.uint8)
        return np.ascontiguousarray(out[..., :w * bs])


def batch_compress_pictures_device(d_pixels, npictures, nbands, rows, cols, block_size, d_workspace, d_out, out_cap, group_planes,
                                   mode="qtable", param=0.0, colour=0, pitch=None, stream=None, device=None):
    """Enqueue jpegx_batch_compress_pictures: pictures stacked [npictures * rows][pitch] (bytes, default cols * nbands) ->
    coded bytes at d_out (None: sizes only).  Verdict and plane index: batch_compress_status with nbands * npictures planes
    of padded_shape(rows, cols, block_size)."""
    args = (d_pixels, int(npictures), int(nbands), int(rows), int(cols), int(cols * nbands if pitch is None else pitch), int(colour),
            int(block_size), mode_of(mode), float(param), int(group_planes), d_workspace, d_out, int(out_cap), stream)
    _entry_checked("jpegx_batch_compress_pictures", device, *args)


def batch_decompress_pictures_device(d_bytes, plane_offsets, npictures, nbands, rows, cols, block_size, d_workspace, d_out,
                                     out_pitch=None, mode="qtable", param=0.0, colour=0, stream=None, device=None):
    """jpegx_batch_decompress_pictures (synchronises the stream between groups and levels); plane_offsets: nbands * npictures + 1
    host integers; pictures stacked [npictures * rows][out_pitch] (default cols * nbands) at d_out.  Raises JpegxError for
    whatever the entry refuses; d_out is untouched then."""
    off = _plane_offsets(plane_offsets, int(npictures) * int(nbands), "nbands * npictures")
    args = (d_bytes, off.ctypes.data, int(npictures), int(nbands), int(rows), int(cols), int(block_size), mode_of(mode), float(param),
            int(colour), d_workspace, d_out, int(cols * nbands if out_pitch is None else out_pitch), stream)
    _entry_checked("jpegx_batch_decompress_pictures", device, *args)


def batch_compress_pictures(pixels, block_size=1, mode="qtable", param=0.0, colour=None, group_planes=None):
    """uint8 pictures [k][rows][cols][nb] -> a list of k lists of nb byte strings, each what compress_plane_native(band,
    ragged=True) gives for that band of that picture (with colour='rgb': of the picture's Pillow YCbCr).  Host convenience over
    the device entries (upload, sizes-only compress, status, emit into a buffer of exactly the total, download).  group_planes
    None: the recommended value.  JpegxError naming BadRleCodeError for an amplitude beyond 15 bits anywhere in the batch."""
    src = _picture_stack(pixels)
    k, rows, cols, nb = src.shape
    bs = int(block_size)
    flag = _colour_flag(colour, nb, "batch_compress_pictures")
    if group_planes is None:
        group_planes = batch_group_planes_pictures_n(nb, rows, cols, bs, 8) or nb
    pics = (k, nb, rows, cols, bs)
    nws = batch_pictures_workspace_bytes(*pics, group_planes)
    if nws == 0:                                        # the entry names the refusal, before any device is touched
        batch_compress_pictures_device(1, *pics, 16, None, 0, group_planes, mode, param, flag)
        raise JpegxError("batch_compress_pictures: the batch was refused")
    mode_of(mode)
    planes = (k * nb,) + padded_shape(rows, cols, bs)
    require_device()
    with _Buffers() as dev:
        din, dws = dev(src.nbytes), dev(nws)
        din.upload(src)
        batch_compress_pictures_device(din.ptr, *pics, dws.ptr, None, 0, group_planes, mode, param, flag)
        blob, off = _emit_exactly(dev, lambda: batch_compress_status(dws.ptr, *planes),
                                  lambda d_out, cap: batch_emit_device(dws.ptr, *planes, d_out, cap), "jpegx_batch_emit")
        return _cut_blobs(blob, off, k, nb)


def batch_decompress_pictures(blobs, rows, cols, block_size=1, mode="qtable", param=0.0, colour=None):
    """k lists of nb byte strings (as batch_compress_pictures returns them) -> uint8 [k][rows][cols][nb], picture p the np.dstack
    of its decoded bands cropped to rows x cols (with colour='rgb': Pillow's RGB of that).  JpegxError naming a plane range for a
    stream the device refuses."""
    blobs, k, nb = _picture_blobs(blobs)
    flag = _colour_flag(colour, nb, "batch_decompress_pictures")
    rows, cols = int(rows), int(cols)
    flat = [b for picture in blobs for b in picture]
    off, total = _blob_offsets(flat)
    pics = (k, nb, rows, cols, int(block_size))
    nws = batch_decompress_pictures_workspace_bytes(max(total, 1), *pics)
    if nws == 0 or total == 0:                          # the entry names the refusal, before any device is touched
        batch_decompress_pictures_device(1, off, *pics, 256, 16, None, mode, param, flag)
        raise JpegxError("batch_decompress_pictures: empty stream")
    mode_of(mode)
    stream_bytes = np.zeros(total + 16, dtype=np.uint8)                # 16 zero bytes behind the stream
    stream_bytes[:total] = np.frombuffer(b"".join(flat), dtype=np.uint8)
    require_device()
    with _Buffers() as dev:
        din, dws, dout = dev(stream_bytes.nbytes), dev(max(256, nws)), dev(k * rows * cols * nb)
        din.upload(stream_bytes)
        batch_decompress_pictures_device(din.ptr, off, *pics, dws.ptr, dout.ptr, None, mode, param, flag)
        return dout.download((k, rows, cols, nb), np.uint8)


# ---------------------------------------------------------------------------------------------
# the size probe and the distortion probe at dct_size 8 (csrc/jpegx_probe_8.hip): the probes above for the 8x8 roads, shaped
# like their _n namesakes without n.  All four quantiser modes; 'none' and 'qtable' have no parameter: one candidate, not read.
# ---------------------------------------------------------------------------------------------
def probe_sizes_8_device(d_planes, nplanes, height, width, mode, params, d_totals, pitch=None, stream=None, device=None):
    """Enqueue jpegx_probe_sizes_8: nplanes float64 planes stacked [nplanes * height][pitch] (elements, default width) ->
    uint64 d_totals [nplanes][K]: bits 0..62 the coded bytes of the plane under candidate q, bit 63 the bad-amplitude flag."""
    h, k = _probe_params(params)
    args = (d_planes, int(nplanes), int(height), int(width), int(width if pitch is None else pitch), mode_of(mode), h.ctypes.data, k,
            d_totals, stream)
    _entry_checked("jpegx_probe_sizes_8", device, *args)


def probe_distortion_8_device(d_planes, d_moments, nplanes, height, width, bs, rows, cols, mode, params, d_totals, pitch=None, mpitch=None,
                              stream=None, device=None):
    """Enqueue jpegx_probe_distortion_8: nplanes float64 planes stacked [nplanes * height][pitch] and their moments
    [nplanes * height][mpitch] (elements, default width), every plane a rows x cols band pooled bs x bs -> uint64 d_totals
    [nplanes][K]: bits 0..62 the sum of squared differences of the band under candidate q, bit 63 the bad-amplitude flag."""
    h, k = _probe_params(params)
    args = (d_planes, d_moments, int(nplanes), int(height), int(width), int(width if pitch is None else pitch),
            int(width if mpitch is None else mpitch), int(bs), int(rows), int(cols), mode_of(mode), h.ctypes.data, k, d_totals, stream)
    _entry_checked("jpegx_probe_distortion_8", device, *args)


def _float64_planes(planes, who):
    src = np.ascontiguousarray(planes, dtype=np.float64)
    if src.ndim != 3 or src.size == 0:
        raise JpegxError("%s: expected non-empty [nplanes][H][W] float64 planes, got %r" % (who, src.shape))
    return src


def probe_sizes_8(planes, mode, params):
    """float64 planes [nplanes][H][W] of whole 8x8 blocks -> (sizes, bad), each [nplanes][K]: what every plane's stream weighs
    under candidate q (the bytes of compress_plane_native on that plane), and where an amplitude beyond 15 bits makes that
    meaningless.  Host convenience: upload, probe, one download."""
    src = _float64_planes(planes, "probe_sizes_8")
    n, hh, ww = src.shape
    h, nk = _probe_params(params)
    if not 1 <= nk <= PROBE_MAX_CANDIDATES or hh % 8 or ww % 8:     # the entry names the refusal, before any device is touched
        probe_sizes_8_device(8, n, hh, ww, mode, h, 8)
        raise JpegxError("probe_sizes_8: the planes were refused")
    mode_of(mode)
    require_device()
    with _Buffers() as dev:
        din, dtot = dev(src.nbytes), dev(n * nk * 8)
        din.upload(src)
        probe_sizes_8_device(din.ptr, n, hh, ww, mode, h, dtot.ptr)
        raw = dtot.download((n, nk), np.uint64)
    return _probe_answer(raw)


def probe_distortion_8(planes, moments, bs, rows, cols, mode, params):
    """float64 planes [nplanes][H][W] and their uint64 moments [nplanes][H][W] (S2 << 32 | S1 of every sample's live pixels),
    every plane a rows x cols band pooled bs x bs -> (sse, bad), each [nplanes][K].  Host convenience."""
    src = _float64_planes(planes, "probe_distortion_8")
    mom = np.ascontiguousarray(moments, dtype=np.uint64)
    if mom.shape != src.shape:
        raise JpegxError("probe_distortion_8: the moments must have the planes' shape")
    n, hh, ww = src.shape
    h, nk = _probe_params(params)
    if not 1 <= nk <= PROBE_MAX_CANDIDATES or hh % 8 or ww % 8 or _padded_shape_or_none(rows, cols, bs) != (hh, ww):
        probe_distortion_8_device(8, 8, n, hh, ww, bs, rows, cols, mode, h, 8)
        raise JpegxError("probe_distortion_8: the planes were refused")
    mode_of(mode)
    require_device()
    with _Buffers() as dev:
        din, dmo, dtot = dev(src.nbytes), dev(mom.nbytes), dev(n * nk * 8)
        din.upload(src)
        dmo.upload(mom)
        probe_distortion_8_device(din.ptr, dmo.ptr, n, hh, ww, bs, rows, cols, mode, h, dtot.ptr)
        raw = dtot.download((n, nk), np.uint64)
    return _probe_answer(raw)


def _padded_shape_or_none(rows, cols, bs):
    try:
        return tuple(padded_shape(rows, cols, bs))
    except JpegxError:
        return None


def batch_probe_pictures_workspace_bytes(npictures, nbands, rows, cols, bs, group_planes):
    return lib().jpegx_batch_probe_pictures_workspace_bytes(int(npictures), int(nbands), int(rows), int(cols), int(bs), int(group_planes))


def batch_probe_distortion_pictures_workspace_bytes(npictures, nbands, rows, cols, bs, group_planes):
    return lib().jpegx_batch_probe_distortion_pictures_workspace_bytes(int(npictures), int(nbands), int(rows), int(cols), int(bs),
                                                                       int(group_planes))


def batch_probe_pictures_device(d_pixels, npictures, nbands, rows, cols, bs, mode, params, group_planes, d_workspace, d_totals, colour=0,
                                pitch=None, stream=None, device=None):
    """Enqueue jpegx_batch_probe_pictures: pictures stacked [npictures * rows][pitch] (bytes, default cols * nbands) -> uint64
    d_totals [nbands * npictures][K], plane-major in the batch's picture-major plane order."""
    h, k = _probe_params(params)
    args = (d_pixels, int(npictures), int(nbands), int(rows), int(cols), int(cols * nbands if pitch is None else pitch), int(colour),
            int(bs), mode_of(mode), h.ctypes.data, k, int(group_planes), d_workspace, d_totals, stream)
    _entry_checked("jpegx_batch_probe_pictures", device, *args)


def batch_probe_distortion_pictures_device(d_pixels, npictures, nbands, rows, cols, bs, mode, params, group_planes, d_workspace, d_totals,
                                           colour=0, pitch=None, stream=None, device=None):
    """Enqueue jpegx_batch_probe_distortion_pictures: as batch_probe_pictures_device, the totals the sums of squared differences."""
    h, k = _probe_params(params)
    args = (d_pixels, int(npictures), int(nbands), int(rows), int(cols), int(cols * nbands if pitch is None else pitch), int(colour),
            int(bs), mode_of(mode), h.ctypes.data, k, int(group_planes), d_workspace, d_totals, stream)
    _entry_checked("jpegx_batch_probe_distortion_pictures", device, *args)


def _batch_probe_8(who, workspace_bytes, enqueue, pixels, bs, mode, params, colour, group_planes):
    src = _picture_stack(pixels)
    k, rows, cols, nb = src.shape
    flag = _colour_flag(colour, nb, who)
    if group_planes is None:
        group_planes = batch_group_planes_pictures_n(nb, rows, cols, bs, 8) or nb
    h, nk = _probe_params(params)
    pics = (k, nb, rows, cols, int(bs))
    nws = workspace_bytes(*pics, group_planes)
    if nws == 0 or not 1 <= nk <= PROBE_MAX_CANDIDATES:     # the entry names the refusal, before any device is touched
        enqueue(1, *pics, mode, h, group_planes, 16, 8, flag)
        raise JpegxError("%s: the batch was refused" % who)
    mode_of(mode)
    require_device()
    with _Buffers() as dev:
        din, dws, dtot = dev(src.nbytes), dev(nws), dev(k * nb * nk * 8)
        din.upload(src)
        enqueue(din.ptr, *pics, mode, h, group_planes, dws.ptr, dtot.ptr, flag)
        raw = dtot.download((k, nb, nk), np.uint64)
    return _probe_answer(raw)


def batch_probe_pictures(pixels, bs, mode, params, colour=None, group_planes=None):
    """uint8 pictures [k][rows][cols][nb] -> (sizes, bad): sizes uint64 [k][nb][K], the length of band b of picture p as
    batch_compress_pictures would code it under candidate q; bad bool [k][nb][K], True where that band holds an amplitude
    beyond 15 bits under that candidate (its size is then meaningless).  Host convenience: upload, probe, one download.
    group_planes None: the recommended value."""
    return _batch_probe_8("batch_probe_pictures", batch_probe_pictures_workspace_bytes, batch_probe_pictures_device, pixels, bs, mode,
                          params, colour, group_planes)


def batch_probe_distortion_pictures(pixels, bs, mode, params, colour=None, group_planes=None):
    """uint8 pictures [k][rows][cols][nb] -> (sse, bad): sse uint64 [k][nb][K], the sum of squared differences between band b of
    picture p and what batch_decompress_pictures gives back of batch_compress_pictures's bytes under candidate q (with
    colour='rgb': in the coded YCbCr bands); bad as batch_probe_pictures gives it (the band cannot be coded; its sum is then
    meaningless).  Host convenience: upload, probe, one download.  group_planes None: the recommended value."""
    return _batch_probe_8("batch_probe_distortion_pictures", batch_probe_distortion_pictures_workspace_bytes,
                          batch_probe_distortion_pictures_device, pixels, bs, mode, params, colour, group_planes)


# ---------------------------------------------------------------------------------------------
# the batch codec for a SET of pictures of unequal sizes at dct_size 8: the set entries above with the table of N = 8
# (picture_set_table(sizes, nbands, bs, 8)), the int16 stream and the 8x8 stage, so qtable is taken.
# ---------------------------------------------------------------------------------------------
def batch_set_workspace_bytes(table, group_samples=0):
    return lib().jpegx_batch_set_workspace_bytes(table.ptr, int(group_samples))


def batch_set_max_bytes(table):
    return lib().jpegx_batch_set_max_bytes(table.ptr)


def batch_decompress_set_workspace_bytes(nbytes, table, group_samples=0):
    return lib().jpegx_batch_decompress_set_workspace_bytes(int(nbytes), table.ptr, int(group_samples))


def batch_groups_set(plane_offsets, table, group_samples=0):
    """The cut of a coded set into decoding groups on picture boundaries (jpegx_batch_groups_set; host arithmetic): the first
    PICTURE of every group and, last, npictures."""
    off = _plane_offsets(plane_offsets, table.npictures * table.nbands, "nbands * npictures")
    first = np.zeros(table.npictures + 1, dtype=np.int32)
    ngroups = ctypes.c_int(0)
    check(lib().jpegx_batch_groups_set(off.ctypes.data, table.ptr, int(group_samples), first.ctypes.data, ctypes.byref(ngroups)),
          "jpegx_batch_groups_set")
    return first[:ngroups.value + 1].copy()


def picture_set_strip_bytes_u8(table, p0=0, k=None):
    """Bytes of the raw uint8 block strip of pictures p0 .. p0 + k - 1 (jpegx_picture_set_blocks_u8): 64 * bs * bs a block, at
    block_size 1 with the pad block behind an odd count."""
    k = table.npictures - p0 if k is None else k
    blocks = int(table.entries["first"][p0 + k] - table.entries["first"][p0])
    bs = int(table.head["bs"])
    return (blocks + (blocks & 1 if bs == 1 else 0)) * 64 * bs * bs


def picture_set_blocks_u8_device(d_pixels, table, d_table, p0, k, d_strip, colour=0, stream=None, device=None):
    """Enqueue jpegx_picture_set_blocks_u8: pixels of pictures p0 .. p0 + k - 1 -> their raw uint8 block strip at d_strip."""
    args = (d_pixels, table.ptr, d_table, int(p0), int(k), int(colour), d_strip, stream)
    _entry_checked("jpegx_picture_set_blocks_u8", device, *args)


def picture_set_blocks_u8(pictures, block_size=1, colour=None):
    """jpegx_picture_set_blocks_u8 on host arrays (test convenience, like picture_planes_stacked_u8): a sequence of uint8
    pictures [rows_p][cols_p][nb] -> the raw uint8 strip as the forward kernel sees it, [T * 8 bs][8 bs] at block_size 2 and 4,
    [ceil(T / 2) * 8][16] at block_size 1 (an odd T: with the pad block of zeros)."""
    pics = [np.ascontiguousarray(p) for p in pictures]
    if not pics or any(p.ndim != 3 or p.size == 0 or p.dtype != np.uint8 for p in pics) or len({p.shape[2] for p in pics}) != 1:
        raise JpegxError("expected at least one non-empty [rows][cols][bands] uint8 picture, and the same number of bands in each")
    nb, bs = pics[0].shape[2], int(block_size)
    flag = _colour_flag(colour, nb, "picture_set_blocks_u8")
    table = picture_set_table([p.shape[:2] for p in pics], nb, bs, 8)
    if bs not in (1, 2, 4):
        picture_set_blocks_u8_device(1, table, 8, 0, len(pics), 16, flag)
    nbytes = picture_set_strip_bytes_u8(table)
    require_device()
    flat = np.concatenate([p.reshape(-1) for p in pics])
    with _Buffers() as dev:
        din, dtab, dout = dev(flat.nbytes), dev(table.nbytes), dev(nbytes)
        din.upload(flat)
        dtab.upload(table.blob.view(np.uint8)[:table.nbytes])
        picture_set_blocks_u8_device(din.ptr, table, dtab.ptr, 0, len(pics), dout.ptr, flag)
        return dout.download((nbytes // (16 if bs == 1 else 8 * bs), 16 if bs == 1 else 8 * bs), np.uint8)


def batch_compress_picture_set_device(d_pixels, table, d_table, d_workspace, d_out, out_cap, mode="qtable", param=0.0, colour=0,
                                      group_samples=0, stream=None, device=None):
    """Enqueue jpegx_batch_compress_picture_set -> coded bytes at d_out (None: sizes only).  Verdict and plane index:
    batch_compress_status_set."""
    args = (d_pixels, table.ptr, d_table, int(colour), mode_of(mode), float(param), int(group_samples), d_workspace, d_out, int(out_cap), stream)
    _entry_checked("jpegx_batch_compress_picture_set", device, *args)


def batch_compress_status_set(d_workspace, table, group_samples=0, stream=None, device=None):
    """Synchronises; returns (rc, total, offsets) as batch_compress_status does."""
    return _compress_status("jpegx_batch_compress_status_set", device, table.npictures * table.nbands,
                            (d_workspace, table.ptr, int(group_samples)), stream)


def batch_emit_set_device(d_workspace, table, d_table, d_out, out_cap, group_samples=0, stream=None, device=None):
    args = (d_workspace, table.ptr, d_table, int(group_samples), d_out, int(out_cap), stream)
    _entry_checked("jpegx_batch_emit_set", device, *args)


def batch_decompress_picture_set_device(d_bytes, plane_offsets, table, d_table, d_workspace, d_out, mode="qtable", param=0.0, colour=0,
                                        group_samples=0, stream=None, device=None):
    """jpegx_batch_decompress_picture_set (synchronises the stream per group and level); plane_offsets: nbands * npictures + 1
    host integers; every picture at its offset and pitch in d_out.  Raises JpegxError for whatever the entry refuses."""
    off = _plane_offsets(plane_offsets, table.npictures * table.nbands, "nbands * npictures")
    args = (d_bytes, off.ctypes.data, table.ptr, d_table, mode_of(mode), float(param), int(colour), int(group_samples), d_workspace, d_out, stream)
    _entry_checked("jpegx_batch_decompress_picture_set", device, *args)


def batch_compress_picture_set(pictures, block_size=1, mode="qtable", param=0.0, colour=None, group_samples=0):
    """A sequence of uint8 pictures [rows_p][cols_p][nb], sizes as they come -> per picture the list of its nb bands' bytes, each
    what compress_plane_native(band, ragged=True) gives for that band of that picture (with colour='rgb': of the picture's
    Pillow YCbCr).  Host convenience over the device entries, as batch_compress_picture_set_n."""
    pics = _picture_list(pictures)
    nb = pics[0].shape[2]
    flag = _colour_flag(colour, nb, "batch_compress_picture_set")
    table = picture_set_table([p.shape[:2] for p in pics], nb, block_size, 8)      # names the refusal, before any device is touched
    mode_of(mode)
    nws = batch_set_workspace_bytes(table, group_samples)
    if nws == 0:
        batch_compress_picture_set_device(1, table, 8, 16, None, 0, mode, param, flag, group_samples)
        raise JpegxError("batch_compress_picture_set: the set was refused")
    require_device()
    flat = np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in pics])
    with _Buffers() as dev:
        din, dtab, dws = dev(flat.nbytes), dev(table.nbytes), dev(nws)
        din.upload(flat)
        dtab.upload(table.blob.view(np.uint8)[:table.nbytes])
        batch_compress_picture_set_device(din.ptr, table, dtab.ptr, dws.ptr, None, 0, mode, param, flag, group_samples)
        blob, off = _emit_exactly(dev, lambda: batch_compress_status_set(dws.ptr, table, group_samples),
                                  lambda d_out, cap: batch_emit_set_device(dws.ptr, table, dtab.ptr, d_out, cap, group_samples), "jpegx_batch_emit_set")
        return _cut_blobs(blob, off, len(pics), nb)


def batch_decompress_picture_set(blobs, sizes, block_size=1, mode="qtable", param=0.0, colour=None, group_samples=0):
    """k lists of nb byte strings (as batch_compress_picture_set returns them) and the k (rows, cols) -> a list of uint8 arrays
    [rows_p][cols_p][nb], picture p the np.dstack of its decoded bands cropped to its size (with colour='rgb': Pillow's RGB of
    that).  JpegxError naming a picture range for a stream the device refuses."""
    sizes = [(int(r), int(c)) for r, c in sizes]
    blobs, k, nb = _picture_blobs(blobs, sizes)
    flag = _colour_flag(colour, nb, "batch_decompress_picture_set")
    table = picture_set_table(sizes, nb, block_size, 8)
    mode_of(mode)
    flat = [b for picture in blobs for b in picture]
    off, total = _blob_offsets(flat)
    nws = batch_decompress_set_workspace_bytes(max(total, 1), table, group_samples)
    if nws == 0 or total == 0:                          # the entry names the refusal, before any device is touched
        batch_decompress_picture_set_device(1, off, table, 8, 256, 1, mode, param, flag, group_samples)
        raise JpegxError("batch_decompress_picture_set: empty stream")
    require_device()
    nout = sum(r * c * nb for r, c in sizes)
    with _Buffers() as dev:
        din, dtab, dws, dout = dev(total), dev(table.nbytes), dev(max(256, nws)), dev(nout)
        din.upload(np.frombuffer(b"".join(flat), dtype=np.uint8))
        dtab.upload(table.blob.view(np.uint8)[:table.nbytes])
        batch_decompress_picture_set_device(din.ptr, off, table, dtab.ptr, dws.ptr, dout.ptr, mode, param, flag, group_samples)
        out = dout.download((nout,), np.uint8)
    at = np.concatenate([[0], np.cumsum([r * c * nb for r, c in sizes])])
    return [out[int(at[p]):int(at[p + 1])].reshape(r, c, nb) for p, (r, c) in enumerate(sizes)]
