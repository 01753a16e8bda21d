"""ctypes binding of libwvgpu.so (include/wvgpu.h).

The product path has exactly one implementation: the HIP kernels inside
libwvgpu.so.  There is no CPU fallback -- if the library is missing or no
GPU is visible, every decode entry point raises.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WVG_LIB") or os.path.join(_PKG, "build", "libwvgpu.so")  # WVG_LIB: experiment builds

WVG_ST_CRC_CHECKED = 0x01
WVG_ST_CRC_ERROR = 0x02
WVG_ST_MUTED = 0x04
WVG_ST_BITS_ERROR = 0x08
WVG_ST_EXCEPTION = 0x10
WVG_ST_UNSUPPORTED = 0x20
WVG_ST_DSD_MUTE = 0x40
WVG_ST_NONDET = 0x80
WVG_ST_TIMEOUT = 0x100
WVG_ST_REDONE = 0x200  # block status only: decoded by the lane kernel's fallback
WVG_ST_UNWRITTEN = 0x40000000  # block status only: no decode stored it since wvg_batch_poison
WVG_ERR_ARG = -2
WVG_ERR_OPEN = -3
WVG_ERR_SPACE = -4
WVG_ERR_TIMEOUT = -5
WVG_ERR_EXCEPTION = -6
WVG_KERNEL_TWO_WAVE = 0
WVG_KERNEL_LANE = 1
WVG_KERNEL_AUTO = 2
WVG_MD5_NONE = 0
WVG_MD5_MATCH = 1
WVG_MD5_MISMATCH = 2
WVG_MD5_NOT_COMPARABLE = 3


class WvgFileInfo(ctypes.Structure):
    _fields_ = [
        ("open_ok", ctypes.c_int32), ("num_channels", ctypes.c_int32), ("reduced_channels", ctypes.c_int32),
        ("bits_per_sample", ctypes.c_int32), ("bytes_per_sample", ctypes.c_int32), ("version", ctypes.c_int32),
        ("mode", ctypes.c_int32), ("is_float", ctypes.c_int32), ("is_five", ctypes.c_int32),
        ("file_format", ctypes.c_int32), ("lossy", ctypes.c_int32), ("dsd_multiplier", ctypes.c_uint32),
        ("sample_rate", ctypes.c_int64), ("total_samples", ctypes.c_int64), ("out_frames", ctypes.c_int64),
        ("out_offset", ctypes.c_int64), ("header_off", ctypes.c_int64), ("header_len", ctypes.c_int64),
        ("trailer_off", ctypes.c_int64), ("trailer_len", ctypes.c_int64), ("error", ctypes.c_char * 96),
        ("seek_result", ctypes.c_int32), ("reserved", ctypes.c_int32), ("sample_index0", ctypes.c_int64),
    ]


class WvgFileMd5(ctypes.Structure):
    _fields_ = [
        ("computed", ctypes.c_uint8 * 16), ("stored", ctypes.c_uint8 * 16), ("has_stored", ctypes.c_int32),
        ("verdict", ctypes.c_int32), ("bytes", ctypes.c_int64),
    ]


# wvg_channel_levels (include/wvgpu.h): one 64-byte record per (measurable file, channel)
LEVELS_DTYPE = [("min", "<i4"), ("max", "<i4"), ("sum", "<i8"), ("sumsq_lo", "<u8"), ("sumsq_hi", "<u8"),
                ("clipped", "<i8"), ("active", "<i8"), ("first_active", "<i8"), ("last_active", "<i8")]

# wvg_channel_true_peak (include/wvgpu.h): one 48-byte record per (measurable file, channel)
TRUE_PEAK_DTYPE = [("true_peak", "<i8"), ("true_peak_pos", "<i8"), ("overs", "<i8"), ("sample_peak", "<i8"),
                   ("sample_peak_frame", "<i8"), ("oversample", "<i4"), ("k", "<i4")]

# wvg_file_loudness (include/wvgpu.h): one 64-byte record per measurable file
LOUDNESS_DTYPE = [("power", "<f8"), ("ungated_power", "<f8"), ("max_block_power", "<f8"), ("blocks", "<i8"),
                  ("abs_blocks", "<i8"), ("gated_blocks", "<i8"), ("block_offset", "<i8"), ("step_frames", "<i4"),
                  ("channels", "<i4")]

# wvg_file_loudness_range (include/wvgpu.h): one 64-byte record per measurable file
LOUDNESS_RANGE_DTYPE = [("low_power", "<f8"), ("high_power", "<f8"), ("max_short_power", "<f8"),
                        ("ungated_short_power", "<f8"), ("shorts", "<i8"), ("abs_shorts", "<i8"),
                        ("gated_shorts", "<i8"), ("short_offset", "<i8")]


class WvgFileResult(ctypes.Structure):
    _fields_ = [
        ("frames", ctypes.c_int64), ("crc_errors", ctypes.c_int64), ("lossy", ctypes.c_int32),
        ("exception", ctypes.c_int32), ("status_or", ctypes.c_uint32), ("num_blocks", ctypes.c_int32),
        ("exception_frame", ctypes.c_int64),
    ]


_lib = None


class NativeLibraryMissing(RuntimeError):
    pass


def build() -> str:
    """Compile libwvgpu.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-s", "-C", _PKG])
    return LIB_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryMissing(
            f"{LIB_PATH} is missing: build it with `make -C wavpackdecoder_amd` (or __graft_entry__.build()). "
            "There is no CPU fallback for the decode path.")
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint32
    sig = {
        "wvg_open": (vp, [i32]),
        "wvg_close": (None, [vp]),
        "wvg_last_error": (ctypes.c_char_p, [vp]),
        "wvg_batch_new": (vp, [vp, i32]),
        "wvg_batch_free": (None, [vp]),
        "wvg_batch_add_file": (i32, [vp, ctypes.c_char_p, ctypes.c_size_t, u32, ctypes.POINTER(WvgFileInfo)]),
        "wvg_batch_add_file_at": (i32, [vp, ctypes.c_char_p, ctypes.c_size_t, u32, i64, ctypes.POINTER(WvgFileInfo)]),
        "wvg_batch_add_files": (i32, [vp, i32, vp, vp, u32, i32, vp, vp]),
        "wvg_batch_add_files_device": (i32, [vp, i32, vp, vp, vp]),
        "wvg_batch_add_file_wvc": (i32, [vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, u32,
                                         ctypes.POINTER(WvgFileInfo)]),
        "wvg_batch_file_info": (i32, [vp, i32, ctypes.POINTER(WvgFileInfo)]),
        "wvg_batch_file_infos": (i32, [vp, i32, i32, vp]),
        "wvg_batch_framing_stats": (i32, [vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
        "wvg_batch_lane_groups": (i32, [vp, ctypes.POINTER(ctypes.c_uint32)]),
        "wvg_batch_upload": (i32, [vp]),
        "wvg_batch_reset": (i32, [vp]),
        "wvg_batch_decode": (i32, [vp, vp]),
        "wvg_batch_sync": (i32, [vp]),
        "wvg_batch_stream": (vp, [vp]),
        "wvg_batch_poison": (i32, [vp, i32]),
        "wvg_batch_set_timing": (i32, [vp, i32]),
        "wvg_batch_set_kernel": (i32, [vp, i32]),
        "wvg_batch_timed": (i32, [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)]),
        "wvg_batch_group_times": (i32, [vp, vp, i32]),
        "wvg_batch_out_ints": (i64, [vp]),
        "wvg_batch_device_out": (vp, [vp]),
        "wvg_batch_num_blocks": (i64, [vp]),
        "wvg_batch_bytes_in": (i64, [vp]),
        "wvg_batch_frames": (i64, [vp]),
        "wvg_batch_download": (i32, [vp, vp, i64]),
        "wvg_batch_host_out": (vp, [vp]),
        "wvg_batch_file_result": (i32, [vp, i32, ctypes.POINTER(WvgFileResult)]),
        "wvg_batch_block_status": (i32, [vp, vp, i64]),
        "wvg_batch_lane_counters": (i32, [vp, i32, vp, i64]),
        "wvg_batch_file_blocks": (i32, [vp, i32, vp, vp, i64]),
        "wvg_batch_time": (i32, [vp, i32, ctypes.POINTER(ctypes.c_float)]),
        "wvg_decode_file": (i32, [vp, ctypes.c_char_p, ctypes.c_size_t, i32, vp, i64, ctypes.POINTER(WvgFileInfo),
                                  ctypes.POINTER(WvgFileResult)]),
        "wvg_probe_file": (i32, [ctypes.c_char_p, ctypes.c_size_t, u32, i32, ctypes.POINTER(WvgFileInfo)]),
        "wvg_format_samples": (i32, [vp, i64, i32, vp, i64, i32, i32]),
        "wvg_batch_format": (i32, [vp, i32, vp]),
        "wvg_batch_pcm_bytes": (i64, [vp]),
        "wvg_batch_pcm_offset": (i64, [vp, i32]),
        "wvg_batch_device_pcm": (vp, [vp]),
        "wvg_batch_download_pcm": (i32, [vp, vp, i64]),
        "wvg_batch_host_pcm": (vp, [vp]),
        "wvg_batch_download_pcm_async": (i32, [vp]),
        "wvg_batch_wav": (i32, [vp, i32, vp, i64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)]),
        "wvg_stream_open": (vp, [vp, ctypes.c_char_p, ctypes.c_size_t, u32, i64, ctypes.POINTER(WvgFileInfo)]),
        "wvg_stream_unpack": (i64, [vp, vp, i64]),
        "wvg_stream_set_sample": (i32, [vp, i64]),
        "wvg_stream_state": (i32, [vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                   ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
        "wvg_stream_close": (None, [vp]),
        "wvg_batch_md5": (i32, [vp, vp]),
        "wvg_batch_file_md5": (i32, [vp, i32, ctypes.POINTER(WvgFileMd5)]),
        "wvg_probe_file_md5": (i32, [ctypes.c_char_p, ctypes.c_size_t, vp]),
        "wvg_md5_bytes": (i32, [vp, ctypes.c_size_t, vp]),
        "wvg_probe_file_streams": (i32, [ctypes.c_char_p, ctypes.c_size_t, vp, i32, ctypes.POINTER(ctypes.c_uint32)]),
        "wvg_batch_file_streams": (i32, [vp, i32, vp, i32, ctypes.POINTER(ctypes.c_uint32)]),
        "wvg_interleave_streams": (i32, [vp, vp, i32, i64, vp]),
        "wvg_interleave_tile_frames": (i32, [i32]),
        "wvg_batch_planar": (i32, [vp, i64, vp, i64, vp]),
        "wvg_batch_planar_floats": (i64, [vp, i64]),
        "wvg_batch_file_planar": (i32, [vp, i32, i64, ctypes.POINTER(i64), ctypes.POINTER(i64),
                                        ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(i64)]),
        "wvg_batch_device_planar": (vp, [vp]),
        "wvg_batch_download_planar": (i32, [vp, vp, i64]),
        "wvg_planar_float": (i32, [vp, i64, i32, i32, i64, i64, vp]),
        "wvg_planar_tile_frames": (i32, [i32]),
        "wvg_batch_resample": (i32, [vp, i64, i64, vp, i64, vp]),
        "wvg_batch_resample_floats": (i64, [vp, i64, i64]),
        "wvg_batch_file_resample": (i32, [vp, i32, i64, i64, ctypes.POINTER(i64), ctypes.POINTER(i64),
                                          ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(i64)]),
        "wvg_batch_device_resampled": (vp, [vp]),
        "wvg_batch_download_resampled": (i32, [vp, vp, i64]),
        "wvg_resample_filter": (i32, [i64, i64, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                      ctypes.POINTER(ctypes.c_int32), vp, i64]),
        "wvg_resample_float": (i32, [vp, i64, i32, i32, i64, i64, i64, i64, vp]),
        "wvg_resample_tile_frames": (i32, [i64, i64, i32]),
        "wvg_batch_levels": (i32, [vp, u32, vp]),
        "wvg_batch_file_levels": (i32, [vp, i32, vp, i32]),
        "wvg_levels_ints": (i32, [vp, i64, i32, i32, u32, vp]),
        "wvg_levels_tile_frames": (i32, [i32]),
        "wvg_batch_true_peak": (i32, [vp, i32, vp]),
        "wvg_batch_file_true_peak": (i32, [vp, i32, vp, i32]),
        "wvg_true_peak_taps": (i32, [vp]),
        "wvg_true_peak_oversample": (i32, [i64]),
        "wvg_true_peak_tile_frames": (i32, [i32]),
        "wvg_true_peak_ints": (i32, [vp, i64, i32, i32, i32, vp]),
        "wvg_batch_loudness": (i32, [vp, vp]),
        "wvg_batch_file_loudness": (i32, [vp, i32, vp]),
        "wvg_batch_loudness_blocks": (i64, [vp]),
        "wvg_batch_download_loudness_blocks": (i32, [vp, vp, i64]),
        "wvg_loudness_filter": (i32, [i64, vp, ctypes.POINTER(ctypes.c_int32)]),
        "wvg_loudness_weights": (i32, [i32, u32, vp]),
        "wvg_loudness_ints": (i32, [vp, i64, i32, i32, i64, u32, vp, vp, i64]),
        "wvg_loudness_gate": (i32, [vp, i64, vp]),
        "wvg_loudness_run_steps": (i32, []),
        "wvg_batch_loudness_range": (i32, [vp, vp]),
        "wvg_batch_file_loudness_range": (i32, [vp, i32, vp]),
        "wvg_batch_loudness_shorts": (i64, [vp]),
        "wvg_batch_download_loudness_shorts": (i32, [vp, vp, i64]),
        "wvg_loudness_range_ints": (i32, [vp, i64, i32, i32, i64, u32, vp, vp, i64]),
        "wvg_loudness_range_gate": (i32, [vp, i64, vp]),
        "wvg_dsd_pcm_taps": (i32, [vp, ctypes.POINTER(i64), ctypes.POINTER(i64)]),
        "wvg_dsd_pcm_ints": (i32, [vp, i64, i32, vp]),
        "wvg_dsd_pcm_tile_frames": (i32, [i32]),
    }
    for name, (res, args) in sig.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            if os.environ.get("WVG_LIB"):  # an older experiment build (A/B runs): entry points it lacks stay unbound
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


EXPORTED = ("wvg_open", "wvg_close", "wvg_last_error", "wvg_batch_new", "wvg_batch_free", "wvg_batch_add_file",
            "wvg_batch_add_file_at", "wvg_batch_add_files", "wvg_batch_add_files_device", "wvg_batch_file_info", "wvg_batch_file_infos",
            "wvg_batch_add_file_wvc",
            "wvg_batch_framing_stats", "wvg_batch_lane_groups",
            "wvg_batch_upload", "wvg_batch_reset", "wvg_batch_decode", "wvg_batch_sync", "wvg_batch_stream", "wvg_batch_poison", "wvg_batch_set_timing", "wvg_batch_set_kernel",
            "wvg_batch_timed", "wvg_batch_group_times", "wvg_batch_out_ints", "wvg_batch_device_out",
            "wvg_batch_num_blocks", "wvg_batch_bytes_in", "wvg_batch_frames", "wvg_batch_download", "wvg_batch_host_out",
            "wvg_batch_file_result", "wvg_batch_block_status", "wvg_batch_lane_counters", "wvg_batch_file_blocks", "wvg_batch_time", "wvg_decode_file",
            "wvg_probe_file", "wvg_format_samples", "wvg_batch_format", "wvg_batch_pcm_bytes", "wvg_batch_pcm_offset",
            "wvg_batch_device_pcm", "wvg_batch_download_pcm", "wvg_batch_host_pcm", "wvg_batch_download_pcm_async",
            "wvg_batch_wav",
            "wvg_probe_file_streams", "wvg_batch_file_streams", "wvg_interleave_streams", "wvg_interleave_tile_frames",
            "wvg_batch_planar", "wvg_batch_planar_floats", "wvg_batch_file_planar", "wvg_batch_device_planar",
            "wvg_batch_download_planar", "wvg_planar_float", "wvg_planar_tile_frames",
            "wvg_batch_resample", "wvg_batch_resample_floats", "wvg_batch_file_resample", "wvg_batch_device_resampled",
            "wvg_batch_download_resampled", "wvg_resample_filter", "wvg_resample_float", "wvg_resample_tile_frames",
            "wvg_batch_levels", "wvg_batch_file_levels", "wvg_levels_ints", "wvg_levels_tile_frames",
            "wvg_batch_true_peak", "wvg_batch_file_true_peak", "wvg_true_peak_taps", "wvg_true_peak_oversample",
            "wvg_true_peak_tile_frames", "wvg_true_peak_ints",
            "wvg_batch_loudness", "wvg_batch_file_loudness", "wvg_batch_loudness_blocks",
            "wvg_batch_download_loudness_blocks", "wvg_loudness_filter", "wvg_loudness_weights", "wvg_loudness_ints",
            "wvg_loudness_gate", "wvg_loudness_run_steps",
            "wvg_batch_loudness_range", "wvg_batch_file_loudness_range", "wvg_batch_loudness_shorts",
            "wvg_batch_download_loudness_shorts", "wvg_loudness_range_ints", "wvg_loudness_range_gate",
            "wvg_dsd_pcm_taps", "wvg_dsd_pcm_ints", "wvg_dsd_pcm_tile_frames",
            "wvg_stream_open", "wvg_stream_unpack", "wvg_stream_set_sample", "wvg_stream_state", "wvg_stream_close")
# The MD5 entry points, listed apart: tests/test_abi.py's header scan matches names of
# letters and underscores only, so it cannot see a name with a digit in the header and
# its list comparison would fail on one here (tests/test_md5_host.py checks these four
# against the header and the library instead).
EXPORTED_MD5 = ("wvg_batch_md5", "wvg_batch_file_md5", "wvg_probe_file_md5", "wvg_md5_bytes")
