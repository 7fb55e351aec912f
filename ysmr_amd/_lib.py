"""ctypes binding of libysmr_hip.so (include/ysmr_hip.h).

The HIP library is the product: there is no CPU fallback.  If the shared object has not been
built (``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C ysmr_amd/csrc``) every
entry point raises :class:`YsmrLibraryError`.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("YSMR_HIP_LIB") or os.path.join(_HERE, "csrc", "libysmr_hip.so")  # env: tuning builds

YSMR_OK = 0
YSMR_ERR_ARG = 1
YSMR_ERR_STATE = 4
DET_OVERFLOW = 1
DET_ARENA = 2
DET_STALLED = 4
#: ``cv_flavour`` bits (include/ysmr_hip.h): which OpenCV release the a1 / a6 arithmetic follows
CV_DEFAULT, CV_ANGLE_PRE451, CV_GRAY_3X = 0, 1, 2
#: scheduling hint in the same argument: the one-launch link runs on another stream beside the call (YSMR_BESIDE_LINK)
BESIDE_LINK = 4
#: ... and for the one-launch-per-batch link, which holds one compute unit (YSMR_BESIDE_BATCH_LINK)
BESIDE_BATCH_LINK = 8
#: ... and for the two-launch link of large tables (YSMR_BESIDE_SPLIT_LINK): the matrix-pipe threshold kernel on half the units
BESIDE_SPLIT_LINK = 16
#: test hook in a detection workspace's header (include/ysmr_hip.h)
WS_FAULT_OFFSET, WS_FAULT_RESIDUE_STALL = 32, 0xFA17057A


def cv_flavour_of(version):
    """``cv_flavour`` for an OpenCV version string ('3.4.18', '4.5.0', '4.10.0', ...) or None (the default:
    OpenCV >= 4.5.1).  Also accepts the flag value itself."""
    if version is None or version is False:
        return CV_DEFAULT
    if isinstance(version, int):
        return version
    parts = [int("".join(ch for ch in p if ch.isdigit()) or 0) for p in str(version).split(".")[:3]]
    parts += [0] * (3 - len(parts))
    flags = CV_GRAY_3X if parts[0] < 4 else 0
    if tuple(parts) < (4, 5, 1):
        flags |= CV_ANGLE_PRE451
    return flags

#: numpy view of ``struct ysmr_row`` (40 bytes)
ROW_DTYPE = np.dtype([("frame", "<i4"), ("track_id", "<i4"), ("x", "<f8"), ("y", "<f8"),
                      ("w", "<f4"), ("h", "<f4"), ("angle", "<f4"), ("disappeared", "<i4")])

ABI_VERSION = 15   # YSMR_ABI_VERSION of include/ysmr_hip.h these argtypes were written against

EXPORTS = ("ysmr_abi_version", "ysmr_last_error", "ysmr_detect_workspace_bytes", "ysmr_detect_workspace_init",
           "ysmr_threshold_batch", "ysmr_threshold_batch_variant", "ysmr_threshold_timing", "ysmr_threshold_workgroups", "ysmr_mean_threshold_state_bytes", "ysmr_mean_threshold_batch",
           "ysmr_components_batch", "ysmr_detect_batch", "ysmr_gsff_gains", "ysmr_tracker_create", "ysmr_tracker_destroy",
           "ysmr_tracker_reset", "ysmr_tracker_update", "ysmr_tracker_run", "ysmr_tracker_fused", "ysmr_tracker_batched", "ysmr_tracker_link_mode", "ysmr_tracker_prepare", "ysmr_tracker_peek",
           "ysmr_tracker_info", "ysmr_rows_sort_workspace_bytes", "ysmr_rows_sort", "ysmr_rows_csv_bound",
           "ysmr_rows_format_csv", "ysmr_rows_write_csv", "ysmr_rows_write_csv_columns", "ysmr_rows_format_device_workspace_bytes", "ysmr_rows_format_device", "ysmr_rows_format_csv_devicelike", "ysmr_rows_stream_create", "ysmr_rows_stream_push", "ysmr_rows_stream_count", "ysmr_rows_stream_finish", "ysmr_rows_stream_destroy", "ysmr_rows_columns", "ysmr_select_workspace_bytes", "ysmr_select_tracks",
           "ysmr_evaluate_workspace_bytes", "ysmr_evaluate_tracks", "ysmr_atan2_devicelike", "ysmr_unpack_dib_batch", "ysmr_file_read",
           "ysmr_luminosity_batch", "ysmr_luminosity_batch_host", "ysmr_tracker_dimensions", "ysmr_tracker_update3",
           "ysmr_tracker_run3", "ysmr_tracker_peek3", "ysmr_tracker_prepare3", "ysmr_annotate_batch", "ysmr_plot_colormap",
           "ysmr_plot_extent", "ysmr_plot_workspace_bytes", "ysmr_plot_tracks", "ysmr_plot_angle_histogram", "ysmr_plot_wedges",
           "ysmr_mjpeg_workspace_bytes", "ysmr_mjpeg_batch", "ysmr_mjpeg_encode_workspace_bytes", "ysmr_mjpeg_encode_batch", "ysmr_violin_workspace_bytes", "ysmr_violin_stats", "ysmr_plot_violins",
           "ysmr_mjpeg_decode_workspace_bytes", "ysmr_mjpeg_decode_batch",
           "ysmr_mjpeg_decode_sync_workspace_bytes", "ysmr_mjpeg_decode_batch_sync", "ysmr_mjpeg_decode_sync_geometry",
           "ysmr_png_workspace_bytes", "ysmr_png_stream_bytes_max", "ysmr_png_deflate", "ysmr_plot_stamp",
           "ysmr_png_dynamic_workspace_bytes", "ysmr_png_dynamic_stream_bytes_max", "ysmr_png_deflate_dynamic", "ysmr_png_code_lengths",
           "ysmr_view_boxes_batch", "ysmr_view_tracks_batch", "ysmr_view_batch_host", "ysmr_thrview_batch", "ysmr_thrview_batch_host",
           "ysmr_csv_workspace_bytes", "ysmr_csv_index", "ysmr_csv_parse", "ysmr_csv_order_workspace_bytes", "ysmr_csv_order",
           "ysmr_csv_geometry", "ysmr_csv_parse_devicelike",
           "ysmr_table_csv_bound", "ysmr_table_format_workspace_bytes", "ysmr_table_format_device", "ysmr_table_format_geometry",
           "ysmr_table_format_devicelike", "ysmr_fmt_f64_text",
           "ysmr_csv_parse_typed", "ysmr_csv_parse_typed_devicelike", "ysmr_marks_workspace_bytes", "ysmr_marks_build",
           "ysmr_csv_column_kinds", "ysmr_csv_column_kinds_devicelike", "ysmr_xlsx_sheet_bound", "ysmr_xlsx_sheet_workspace_bytes",
           "ysmr_xlsx_sheet_geometry", "ysmr_xlsx_sheet_device", "ysmr_xlsx_sheet_devicelike",
           "ysmr_tiff_decode_workspace_bytes", "ysmr_tiff_decode_batch")

#: bits of ``status_dev`` of ``ysmr_tiff_decode_batch`` (YSMR_TIFFD_*)
TIFFD_BAD_CODE, TIFFD_SHORT, TIFFD_OVERRUN, TIFFD_OLD_LZW, TIFFD_TABLE = 1, 2, 4, 8, 16

#: bits of ``ysmr_csv_column_kinds`` (YSMR_KIND_*): words 0 .. 15 a column each, word 16 the file's
KIND_NOT_INT, KIND_NOT_NUMBER, KIND_EMPTY, KIND_BAD_LINE, KIND_WORDS = 1, 2, 4, 1, 17

#: column types of ``ysmr_table_format_device`` (include/ysmr_hip.h: YSMR_COL_*), by numpy dtype
TABLE_COLUMN_TYPES = {np.dtype(np.uint32): 0, np.dtype(np.int64): 1, np.dtype(np.int32): 2, np.dtype(np.int8): 3, np.dtype(np.float64): 4}
TABLE_MAX_COLUMNS = 16


class TableColumn(ctypes.Structure):
    """``ysmr_table_column``"""
    _fields_ = [("data", ctypes.c_void_p), ("type", ctypes.c_int32), ("reserved", ctypes.c_int32)]

#: ``flags`` of a ``ysmr_csv_field`` (YSMR_CSV_EMPTY_IS_NAN): an empty float64 field is served and is NaN
CSV_EMPTY_IS_NAN = 1


class CsvField(ctypes.Structure):
    """``ysmr_csv_field``"""
    _fields_ = [("data", ctypes.c_void_p), ("type", ctypes.c_int32), ("column", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]

#: numpy view of ``ysmr_mark`` (16 bytes): one track position of one frame of the annotated video
MARK_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("track_id", "<u4"), ("style", "<u4")])

SELECT_OK, SELECT_TOO_SHORT, SELECT_TOO_SHORT_CLEANED, SELECT_NONE = 0, 1, 2, 3


class SelectParams(ctypes.Structure):
    """``struct ysmr_select_params``"""
    _fields_ = [(k, ctypes.c_double) for k in ("area_lo", "area_hi", "area_factor", "q_area", "motility_stop_fraction",
                                               "max_empty_ratio", "ratio_min", "ratio_max", "edge_fraction")] + \
               [(k, ctypes.c_int32) for k in ("min_length_frames", "limit_frames", "limit_exact", "omit_motility",
                                              "max_holes", "max_recursion", "frame_height", "frame_width")]


class SelectSummary(ctypes.Structure):
    """``struct ysmr_select_summary``"""
    _fields_ = [("status", ctypes.c_int32), ("outliers_used", ctypes.c_int32),
                ("rows_before", ctypes.c_longlong), ("tracks_before", ctypes.c_longlong),
                ("rows_after", ctypes.c_longlong), ("tracks_after", ctypes.c_longlong),
                ("area_lo", ctypes.c_double), ("area_hi", ctypes.c_double), ("q1_dist", ctypes.c_double),
                ("q3_dist", ctypes.c_double), ("dist_fence", ctypes.c_double), ("dist_outliers", ctypes.c_longlong),
                ("kick_reasons", ctypes.c_longlong * 9), ("good_tracks", ctypes.c_longlong),
                ("rows_selected", ctypes.c_longlong)]


class EvaluateParams(ctypes.Structure):
    """``struct ysmr_evaluate_params``"""
    _fields_ = [("pixel_per_micrometre", ctypes.c_double), ("fps", ctypes.c_double), ("min_turn_angle", ctypes.c_double),
                ("angle_lag", ctypes.c_int32), ("reach_lag", ctypes.c_int32), ("median_kernel", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class PlotView(ctypes.Structure):
    """``struct ysmr_plot_view``"""
    _fields_ = [(k, ctypes.c_double) for k in ("px", "u0", "v0", "units_per_pixel")] + \
               [(k, ctypes.c_int32) for k in ("mode", "width", "height", "ax_x", "ax_y", "ax_w", "ax_h", "r2_dot", "r2_start",
                                              "n_grid_cols", "n_grid_rows", "bar_x", "bar_y", "bar_w", "bar_h")] + \
               [("grid_cols", ctypes.c_int32 * 32), ("grid_rows", ctypes.c_int32 * 32)]


VIOLIN_GRID, VIOLIN_MAX_CUTS, VIOLIN_MAX_SLOTS = 100, 254, 64

#: numpy view of ``struct ysmr_violin_summary`` (88 bytes)
VIOLIN_SUMMARY_DTYPE = np.dtype([("members", "<i8"), ("values", "<i8")] + [(k, "<f8") for k in (
    "vmin", "vmax", "q25", "q50", "q75", "whisker_lo", "whisker_hi", "mean", "h")])


class ViolinView(ctypes.Structure):
    """``struct ysmr_violin_view``"""
    _fields_ = [("y0", ctypes.c_double), ("units_per_pixel", ctypes.c_double)] + \
               [(k, ctypes.c_int32) for k in ("width", "height", "ax_x", "ax_y", "ax_w", "ax_h", "n_violins", "n_grid_rows",
                                              "line_half", "box_half", "dot_r2", "reserved")] + \
               [("grid_rows", ctypes.c_int32 * 32), ("slot_x", ctypes.c_int32 * 64), ("slot_w", ctypes.c_int32 * 64),
                ("slot_colour", ctypes.c_int32 * 64)]


#: numpy view of ``ysmr_stamp`` (24 bytes): one bitmap of a figure's lettering
STAMP_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"), ("bit_offset", "<u4"), ("colour", "<u4")])


class YsmrLibraryError(RuntimeError):
    pass


class YsmrCapacityError(YsmrLibraryError):
    """A frame held more components than ``max_det`` or the tracker more tracks than ``capacity``."""


_lib = None


def lib():
    """Load (once) and return the ctypes handle with argtypes set."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise YsmrLibraryError(
            f"{LIB_PATH} is missing: build the HIP library first (make -C ysmr_amd/csrc, or "
            "__graft_entry__.build()). ysmr_amd has no CPU fallback.")
    try:
        L = ctypes.CDLL(LIB_PATH)
    except OSError as exc:  # pragma: no cover
        raise YsmrLibraryError(f"cannot load {LIB_PATH}: {exc}") from exc
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.ysmr_abi_version.restype = ci
    if os.environ.get("HIP_FORCE_DEV_KERNARG") == "0":
        # (a launch's first instructions read its arguments: from host memory that is a PCIe round trip per launch --
        # 90 k -> 62 k frames/s with one launch per frame; ROCm's default and this package's is 1)
        import logging
        logging.getLogger("ysmr").warning("HIP_FORCE_DEV_KERNARG=0 is in force: kernel arguments in host memory cost the "
                                          "per-frame link about a third of its rate; unset it or set it to 1")
    if L.ysmr_abi_version() != ABI_VERSION:
        raise YsmrLibraryError(f"{LIB_PATH} has ABI version {L.ysmr_abi_version()}, this host code binds version "
                               f"{ABI_VERSION} (include/ysmr_hip.h): rebuild the library (make -C ysmr_amd/csrc)")
    L.ysmr_last_error.restype = ctypes.c_char_p
    L.ysmr_detect_workspace_bytes.argtypes = [ci, ci, ci, ci]
    L.ysmr_detect_workspace_bytes.restype = ctypes.c_size_t
    L.ysmr_detect_workspace_init.argtypes = [vp, vp, ctypes.c_size_t]
    L.ysmr_threshold_batch.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, ci]
    L.ysmr_threshold_batch_variant.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, ci, ci]
    L.ysmr_threshold_timing.argtypes = [vp, vp]
    L.ysmr_threshold_workgroups.argtypes = [ctypes.c_int]
    L.ysmr_mean_threshold_state_bytes.argtypes = [ci]
    L.ysmr_mean_threshold_state_bytes.restype = ctypes.c_size_t
    L.ysmr_mean_threshold_batch.argtypes = [vp, vp, ci, ci, ci, ci, ci, cd, ci, vp, vp, vp, vp, ci]
    L.ysmr_components_batch.argtypes = [vp, ci, ci, ci, vp, ctypes.c_size_t, vp, vp, vp, vp, vp, vp, ci, vp, ci]
    L.ysmr_detect_batch.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, ctypes.c_size_t, vp, vp, vp,
                                    vp, vp, vp, ci, vp, ci]
    L.ysmr_gsff_gains.argtypes = [cd, ci, cd, ci, vp, vp]
    L.ysmr_tracker_create.argtypes = [cd, cd, ci, cd, ci, ci, ci, ci, vp, ctypes.POINTER(vp)]
    L.ysmr_tracker_destroy.argtypes = [vp]
    L.ysmr_tracker_reset.argtypes = [vp, vp]
    L.ysmr_tracker_update.argtypes = [vp, vp, vp, ci, ci, vp, ctypes.c_int32, vp, vp, vp, vp, vp, vp]
    L.ysmr_tracker_peek.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ysmr_tracker_run.argtypes = [vp, vp, vp, vp, ci, ctypes.c_int32, vp, ctypes.c_int64, vp]
    L.ysmr_tracker_fused.argtypes = [vp]
    L.ysmr_tracker_batched.argtypes = [vp]
    L.ysmr_tracker_link_mode.argtypes = [vp, ci]
    L.ysmr_tracker_prepare.argtypes = [vp, vp, vp, vp, ci, ci]
    L.ysmr_tracker_prepare3.argtypes = [vp, vp, vp, vp, vp, ci, ci]
    L.ysmr_luminosity_batch.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, ci, ci, vp, vp, vp, vp]
    L.ysmr_luminosity_batch_host.argtypes = [vp, ci, ci, ci, ci, vp, vp, ci, ci, vp, vp, vp, vp]
    L.ysmr_tracker_dimensions.argtypes = [vp, ci]
    L.ysmr_tracker_update3.argtypes = [vp, vp, vp, ci, vp, ci, vp, ctypes.c_int32, vp, vp, vp, vp, vp, vp]
    L.ysmr_tracker_run3.argtypes = [vp, vp, vp, vp, vp, ci, ctypes.c_int32, vp, ctypes.c_int64, vp]
    L.ysmr_tracker_peek3.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.ysmr_tracker_info.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                    ctypes.POINTER(ctypes.c_int32)]
    L.ysmr_rows_sort_workspace_bytes.argtypes = [ctypes.c_longlong]
    L.ysmr_rows_sort_workspace_bytes.restype = ctypes.c_size_t
    L.ysmr_rows_sort.argtypes = [vp, vp, ctypes.c_longlong, vp, ctypes.c_size_t, vp]
    L.ysmr_rows_csv_bound.argtypes = [ctypes.c_longlong, ci]
    L.ysmr_rows_csv_bound.restype = ctypes.c_size_t
    L.ysmr_rows_format_csv.argtypes = [vp, ctypes.c_longlong, ci, ci, ci, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    L.ysmr_file_read.argtypes = [ci, vp, ctypes.c_size_t, ctypes.c_longlong, ci]
    L.ysmr_rows_write_csv.argtypes = [vp, ctypes.c_longlong, ci, ci, ci, ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t)]
    L.ysmr_rows_write_csv_columns.argtypes = [vp, ctypes.c_longlong, ci, ci, ci, ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t)] + [vp] * 7
    L.ysmr_rows_format_device_workspace_bytes.argtypes = [ctypes.c_longlong]
    L.ysmr_rows_format_device_workspace_bytes.restype = ctypes.c_size_t
    L.ysmr_rows_format_device.argtypes = [vp, vp, ctypes.c_longlong, ci, ci, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp] + [vp] * 7 + [vp]
    L.ysmr_rows_format_csv_devicelike.argtypes = [vp, ctypes.c_longlong, ci, ci, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), vp,
                                                  ctypes.POINTER(ctypes.c_longlong)]
    L.ysmr_rows_stream_create.argtypes = [ci, ci, ctypes.POINTER(vp)]
    L.ysmr_rows_stream_push.argtypes = [vp, vp, ctypes.c_longlong]
    L.ysmr_rows_stream_count.argtypes = [vp]
    L.ysmr_rows_stream_count.restype = ctypes.c_longlong
    L.ysmr_rows_stream_finish.argtypes = [vp, ci, ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t)] + [vp] * 7
    L.ysmr_rows_stream_destroy.argtypes = [vp]
    L.ysmr_rows_columns.argtypes = [vp, ctypes.c_longlong, ci, vp, vp, vp, vp, vp, vp, vp]
    L.ysmr_select_workspace_bytes.argtypes = [ctypes.c_longlong, ci]
    L.ysmr_select_workspace_bytes.restype = ctypes.c_size_t
    L.ysmr_select_tracks.argtypes = [vp, ctypes.c_longlong, vp, vp, vp, vp, vp, vp, ctypes.POINTER(SelectParams), vp,
                                     ctypes.c_size_t, vp, vp, ctypes.POINTER(SelectSummary)]
    L.ysmr_unpack_dib_batch.argtypes = [vp, vp, ci, ctypes.c_size_t, ci, ci, ci, ci, ci, vp, vp]
    L.ysmr_annotate_batch.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, vp, ci, ctypes.c_size_t, ci]
    L.ysmr_evaluate_workspace_bytes.argtypes = [ctypes.c_longlong]
    L.ysmr_evaluate_workspace_bytes.restype = ctypes.c_size_t
    L.ysmr_evaluate_tracks.argtypes = [vp, ctypes.c_longlong, vp, vp, vp, vp, vp, vp, ctypes.POINTER(EvaluateParams), vp,
                                       ctypes.c_size_t, vp, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_longlong)]
    L.ysmr_atan2_devicelike.argtypes = [vp, vp, ctypes.c_longlong, vp]
    ll = ctypes.c_longlong
    L.ysmr_plot_colormap.argtypes = [vp]
    L.ysmr_plot_extent.argtypes = [vp, ll, vp, vp, vp, ci, cd, vp]
    L.ysmr_plot_workspace_bytes.argtypes = [ll, ll, ci, ci]
    L.ysmr_plot_workspace_bytes.restype = ctypes.c_size_t
    L.ysmr_plot_tracks.argtypes = [vp, ll, vp, vp, vp, ll, vp, ll, ctypes.POINTER(PlotView), vp, ctypes.c_size_t, vp]
    L.ysmr_plot_angle_histogram.argtypes = [vp, ll, vp, vp, vp, vp, ci, ci, vp, vp, ctypes.c_size_t, vp, vp]
    L.ysmr_plot_wedges.argtypes = [vp, ci, ci, ci, ci, ci, vp, vp, ll, vp]
    L.ysmr_mjpeg_workspace_bytes.argtypes = [ci, ci, ci]
    L.ysmr_mjpeg_workspace_bytes.restype = ctypes.c_size_t
    L.ysmr_mjpeg_decode_workspace_bytes.argtypes = [ci, ci, ci, ci, ci]
    L.ysmr_mjpeg_decode_workspace_bytes.restype = ctypes.c_size_t
    L.ysmr_mjpeg_decode_batch.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, vp, ctypes.c_size_t, vp, vp]
    L.ysmr_mjpeg_decode_sync_workspace_bytes.argtypes = [ci, ci, ci, ci, ci, ci]
    L.ysmr_mjpeg_decode_sync_workspace_bytes.restype = ctypes.c_size_t
    L.ysmr_mjpeg_decode_batch_sync.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, ctypes.c_size_t, vp, vp]
    L.ysmr_mjpeg_decode_sync_geometry.argtypes = [ctypes.POINTER(ci), ctypes.POINTER(ci)]
    L.ysmr_mjpeg_decode_sync_geometry.restype = None
    L.ysmr_mjpeg_batch.argtypes = [vp, vp, ci, ci, ci, ci, ctypes.c_size_t, ci, ci, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp, vp]
    L.ysmr_mjpeg_encode_workspace_bytes.argtypes = [ci, ci, ci, ci, ci]
    L.ysmr_mjpeg_encode_workspace_bytes.restype = ctypes.c_size_t
    L.ysmr_mjpeg_encode_batch.argtypes = [vp, vp, ci, ci, ci, ci, ctypes.c_size_t, ci, ci, ci, ci, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp, vp]
    L.ysmr_violin_workspace_bytes.argtypes = [ll, ci, ci]
    L.ysmr_violin_workspace_bytes.restype = ctypes.c_size_t
    L.ysmr_violin_stats.argtypes = [vp, ll, vp, ll, vp, ll, ci, vp, vp, vp, ctypes.c_size_t, vp, vp]
    L.ysmr_plot_violins.argtypes = [vp, ci, vp, vp, ctypes.POINTER(ViolinView), vp, ctypes.c_size_t, vp]
    L.ysmr_png_workspace_bytes.argtypes = [ci, ci]
    L.ysmr_png_workspace_bytes.restype = ctypes.c_size_t
    L.ysmr_png_stream_bytes_max.argtypes = [ci, ci]
    L.ysmr_png_stream_bytes_max.restype = ctypes.c_size_t
    L.ysmr_png_deflate.argtypes = [vp, vp, ci, ci, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp]
    L.ysmr_plot_stamp.argtypes = [vp, vp, ci, ci, vp, ci, vp, ctypes.c_size_t]
    L.ysmr_png_dynamic_workspace_bytes.argtypes = [ci, ci]
    L.ysmr_png_dynamic_workspace_bytes.restype = ctypes.c_size_t
    L.ysmr_png_dynamic_stream_bytes_max.argtypes = [ci, ci]
    L.ysmr_png_dynamic_stream_bytes_max.restype = ctypes.c_size_t
    L.ysmr_png_deflate_dynamic.argtypes = [vp, vp, ci, ci, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp]
    L.ysmr_png_code_lengths.argtypes = [vp, ci, ci, vp]
    L.ysmr_view_boxes_batch.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, ci, vp, ci, ctypes.c_size_t, ci]
    L.ysmr_view_tracks_batch.argtypes = [vp, vp, ctypes.c_int64, vp, vp, ctypes.c_int32, ci, ci, ci, vp, ci, ctypes.c_size_t, ci]
    L.ysmr_view_batch_host.argtypes = [vp, ci, ci, ci, ci, vp, vp, ci, vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, vp, ci,
                                       ctypes.c_size_t, ci]
    L.ysmr_thrview_batch.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, ci, ctypes.c_size_t, ci]
    L.ysmr_thrview_batch_host.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, vp, ci, ctypes.c_size_t, ci]
    L.ysmr_csv_workspace_bytes.argtypes = [ctypes.c_size_t]
    L.ysmr_csv_workspace_bytes.restype = ctypes.c_size_t
    L.ysmr_csv_index.argtypes = [vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp, vp]
    L.ysmr_csv_parse.argtypes = [vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, ci, vp, ll] + [vp] * 7 + [vp]
    L.ysmr_csv_order_workspace_bytes.argtypes = [ll]
    L.ysmr_csv_order_workspace_bytes.restype = ctypes.c_size_t
    L.ysmr_csv_order.argtypes = [vp, ll] + [vp] * 7 + [vp, ctypes.c_size_t] + [vp] * 7
    L.ysmr_csv_geometry.argtypes = [ctypes.POINTER(ci)] * 3
    L.ysmr_csv_geometry.restype = None
    L.ysmr_csv_parse_devicelike.argtypes = [vp, ctypes.c_size_t, ci, vp, ll] + [vp] * 7 + [ctypes.POINTER(ll), ctypes.POINTER(ll),
                                                                                        ctypes.POINTER(ctypes.c_uint32)]
    tc = ctypes.POINTER(TableColumn)
    L.ysmr_table_csv_bound.argtypes = [ll, ci, tc, ctypes.c_size_t]
    L.ysmr_table_csv_bound.restype = ctypes.c_size_t
    L.ysmr_table_format_workspace_bytes.argtypes = [ll, ci, tc]
    L.ysmr_table_format_workspace_bytes.restype = ctypes.c_size_t
    L.ysmr_table_format_device.argtypes = [vp, ll, ci, tc, ctypes.c_char_p, ctypes.c_size_t, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp, vp]
    L.ysmr_table_format_geometry.argtypes = [ctypes.POINTER(ci)] * 2
    L.ysmr_table_format_geometry.restype = None
    L.ysmr_table_format_devicelike.argtypes = [ll, ci, tc, ctypes.c_char_p, ctypes.c_size_t, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                               ctypes.POINTER(ll)]
    L.ysmr_fmt_f64_text.argtypes = [vp, ll, ci, vp, vp]
    cf = ctypes.POINTER(CsvField)
    L.ysmr_csv_parse_typed.argtypes = [vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, ci, ci, cf, ll, vp]
    L.ysmr_csv_parse_typed_devicelike.argtypes = [vp, ctypes.c_size_t, ci, ci, cf, ll, ctypes.POINTER(ll), ctypes.POINTER(ll),
                                                  ctypes.POINTER(ctypes.c_uint32)]
    L.ysmr_marks_workspace_bytes.argtypes = [ll, ci]
    L.ysmr_marks_workspace_bytes.restype = ctypes.c_size_t
    L.ysmr_marks_build.argtypes = [vp, ll] + [vp] * 7 + [ci, ci, ci, vp, ctypes.c_size_t, vp, vp]
    L.ysmr_csv_column_kinds.argtypes = [vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, ci, ll, vp]
    L.ysmr_csv_column_kinds_devicelike.argtypes = [vp, ctypes.c_size_t, ci, vp, ctypes.POINTER(ll), ctypes.POINTER(ctypes.c_uint32)]
    L.ysmr_xlsx_sheet_bound.argtypes = [ll, ci, tc, ll, ci, ctypes.c_size_t, ctypes.c_size_t]
    L.ysmr_xlsx_sheet_bound.restype = ctypes.c_size_t
    L.ysmr_xlsx_sheet_workspace_bytes.argtypes = [ll, ci, tc, ll, ci, ctypes.c_size_t]
    L.ysmr_xlsx_sheet_workspace_bytes.restype = ctypes.c_size_t
    L.ysmr_xlsx_sheet_geometry.argtypes = [ctypes.POINTER(ci)] * 3
    L.ysmr_xlsx_sheet_geometry.restype = None
    L.ysmr_xlsx_sheet_device.argtypes = [vp, ll, ci, tc, ll, ci, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, vp,
                                         ctypes.c_size_t, vp, ctypes.c_size_t, vp, vp]
    L.ysmr_xlsx_sheet_devicelike.argtypes = [ll, ci, tc, ll, ci, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, vp,
                                             ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ll)]
    L.ysmr_tiff_decode_workspace_bytes.argtypes = [ci] * 8 + [ll]
    L.ysmr_tiff_decode_workspace_bytes.restype = ctypes.c_size_t
    L.ysmr_tiff_decode_batch.argtypes = [vp, vp, vp] + [ci] * 8 + [vp, ctypes.c_size_t, vp, vp]
    for name in EXPORTS:
        if name not in ("ysmr_tiff_decode_workspace_bytes", "ysmr_xlsx_sheet_bound", "ysmr_xlsx_sheet_workspace_bytes", "ysmr_xlsx_sheet_geometry", "ysmr_table_csv_bound", "ysmr_table_format_workspace_bytes", "ysmr_table_format_geometry", "ysmr_csv_workspace_bytes", "ysmr_csv_order_workspace_bytes", "ysmr_marks_workspace_bytes", "ysmr_csv_geometry", "ysmr_png_workspace_bytes", "ysmr_png_stream_bytes_max", "ysmr_png_dynamic_workspace_bytes", "ysmr_png_dynamic_stream_bytes_max", "ysmr_mjpeg_decode_sync_workspace_bytes", "ysmr_mjpeg_decode_sync_geometry", "ysmr_mjpeg_decode_workspace_bytes", "ysmr_violin_workspace_bytes", "ysmr_mjpeg_workspace_bytes", "ysmr_mjpeg_encode_workspace_bytes", "ysmr_plot_workspace_bytes", "ysmr_evaluate_workspace_bytes", "ysmr_select_workspace_bytes", "ysmr_last_error", "ysmr_detect_workspace_bytes", "ysmr_abi_version",
                        "ysmr_rows_sort_workspace_bytes", "ysmr_rows_csv_bound", "ysmr_rows_stream_count",
                        "ysmr_mean_threshold_state_bytes"):
            getattr(L, name).restype = ci
    _lib = L
    return L


def check(rc, what):
    """Map a non-zero status to an exception carrying ysmr_last_error()."""
    if rc != YSMR_OK:
        msg = lib().ysmr_last_error().decode("utf-8", "replace")
        raise YsmrLibraryError(f"{what} failed (code {rc}): {msg}")


def stream_ptr(device=None):
    """The current torch HIP stream OF ``device`` as a hipStream_t value (``None``: of the current
    device).  Every entry point that launches work passes the device its buffers live on: the current
    device of a fresh worker is cuda:0 whatever GPU its job was dealt to."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def on(device):
    """Context: make ``device`` the current HIP device (kernels are launched on the current device; a
    stream of another device is an invalid handle there)."""
    import torch
    if torch.cuda.device_count() == 0:      # a host without GPUs: let the first device call report it
        import contextlib
        return contextlib.nullcontext()
    return torch.cuda.device(torch.device(device))


def on_own_device(method):
    """Run a method of an object that has a ``device`` (a Detector, a DeviceTracker, a TrackingPipeline and what hangs on one)
    with that GPU as the current device (the caller's current device is cuda:0 in a fresh worker, whatever GPU its video
    was dealt to)."""
    import functools

    @functools.wraps(method)
    def wrapped(self, *args, **kwargs):
        with on(self.device):
            return method(self, *args, **kwargs)
    return wrapped
