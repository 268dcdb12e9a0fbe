"""Return codes and nl_last_error() strings of the frame-step entries (nlstack_frame.hip, nlstack_frame_pre.hip,
nlstack_frame_stretch.hip, nlstack_frame_rgb.hip) on a machine without a device: every argument check that runs in
front of the device, the order of two faults at once, and NL_ERR_NO_DEVICE for valid arguments.

A characterisation table: EXPECTED was recorded from the library as it was before the entries were split over four
units and must not be regenerated from the code under test.  Every row first sets a known error from another unit
(SENTINEL), so a call that succeeds shows that it leaves the thread's error alone."""
import ctypes as C

import numpy as np
import pytest

from nightlight_amd import capi

# every exported symbol defined outside the four frame units: nlstack_api.hip, nlstack_pass.hip, nlstack_group.hip and
# the host sources (op_stack.cpp, fits_frame.cpp)
ELSEWHERE = {
    "nl_last_error", "nl_device_count", "nl_version", "nl_stack_create", "nl_stack_destroy",
    "nl_stack_upload_frame", "nl_stack_upload_tile", "nl_stack_upload_frame_async", "nl_stack_upload_wait",
    "nl_stack_frames_device_ptr", "nl_stack_device_bytes", "nl_release_cached_memory",
    "nl_fits_parse_header", "nl_fits_write_header", "nl_fits_padded_bytes",
    "nl_stack_attach_device_frames", "nl_stack_attach_device_frames_strided", "nl_stack_frame_stride",
    "nl_stack_fill_synthetic", "nl_stack_download_tile", "nl_stack_download_rows",
    "nl_stack_set_active_frames", "nl_stack_set_weights", "nl_weights_from_scalars",
    "nl_stack_linfit_stage_counts", "nl_stack_run", "nl_stack_run_async", "nl_stack_finish",
    "nl_stack_result_device_ptr", "nl_stack_last_mode", "nl_stack_last_kernel_ms", "nl_stack_last_dominant_kernel_ms",
    "nl_stack_last_kernel_name", "nl_stack_pass_times", "nl_stack_stream", "nl_stack_counters_device_ptr",
    "nl_stack_copy_counters_async", "nl_stack_set_counters_buffer", "nl_stack_order_stream_after",
    "nl_group_tile_rows", "nl_group_create", "nl_group_destroy", "nl_group_size", "nl_group_tile",
    "nl_group_upload_frame", "nl_group_fill_synthetic", "nl_group_set_active_frames", "nl_group_set_weights",
    "nl_group_set_exact", "nl_group_run", "nl_group_last_mode", "nl_group_find_sigmas", "nl_group_accumulate",
    "nl_group_accumulate_finalize", "nl_stack_set_exact", "nl_stack_set_dev_flags", "nl_stack_last_fallback_pixels",
    "nl_stack_last_generic_pixels", "nl_stack_last_pass_protocol", "nl_stack_find_sigmas", "nl_stack_accumulate",
    "nl_stack_accumulate_finalize", "nl_stack_upload_frame_fits", "nl_stack_upload_frame_projected",
    "nl_stack_upload_frame_fits_async", "nl_stack_upload_frame_projected_async", "nl_group_upload_frame_fits",
    "nl_group_upload_frame_projected", "nl_stack_download_result_fits", "nl_fits_decode", "nl_project_bilinear",
    "nl_host_op_stack_apply_json", "nl_host_op_stack_roundtrip_json", "nl_host_set_devices",
    "nl_host_op_stack_batches_apply_json", "nl_group_frame_project_from",
}

SENTINEL = "Invalid weighting mode 7"

W = H = 4
F = np.arange(W * H, dtype=np.float32)            # the 4x4 frame
OUT = np.zeros(3 * W * H, np.float32)
P3 = np.zeros(3 * W * H, np.float32)              # three planes
RAW = np.zeros(8 * W * H, np.uint8)
TAPS3 = np.array([0.25, 0.5, 0.25], np.float32)
TAPS4 = np.array([0.25, 0.25, 0.25, 0.25], np.float32)
TAPS11 = np.full(11, 1.0 / 11.0, np.float32)
MASK = np.array([-1, 0, 1], np.int32)
V3 = np.array([0.0, 0.5, 1.0], np.float32)
STARS = np.zeros(2, capi.STAR_DTYPE)
T6 = np.array([1, 0, 0, 0, 1, 0], np.float32)
PLANES = (C.c_int * 3)(0, 1, 2)
ZERO, ONE = capi.Rgb(0, 0, 0), capi.Rgb(1, 1, 1)

f = capi.fptr
raw = RAW.ctypes.data_as(C.c_void_p)
stars = STARS.ctypes.data_as(C.c_void_p)
mask = MASK.ctypes.data_as(C.POINTER(C.c_int32))


def _i():
    return C.byref(C.c_int(0))


def _i64():
    return C.byref(C.c_int64(0))


def _fl():
    return C.byref(C.c_float(0))


def tone_of(kind, *p):
    return C.byref(capi.Tone(kind, (C.c_float * 3)(*p)))


def chroma_of(kind, *p):
    return C.byref(capi.Chroma(kind, (C.c_float * 4)(*p)))


STAR_ARGS = (0.0, 1.0, 15.0, 5.0, 1.4, 2, 0.0)                   # location ... diff_std
BACK_ARGS = (2, 4.0, 1.5, 0)                                      # grid_size, hfr_factor, sigma, clip
DEBAND_ARGS = (50.0, 2, 3.0, 0.0, 1.0)                            # percentile, window, sigma, location, scale
USM_ARGS = (1.0, 0.5, 0.0, 1.0, 0.0)                              # sigma, gain, min, max, abs_threshold
BALANCE_TAIL = (2, 0.0, 0.0, 0.0, ZERO, ONE, f(V3), f(V3), None)  # block ... report


def _calib(L, *a):
    """nl_calib_create returns a pointer: 0 for the null one"""
    c = L.nl_calib_create(*a)
    if c:
        L.nl_calib_destroy(c)
    return 0 if not c else 1


# (row id, entry, call(L) -> return code)
ROWS = [
    # ---- nlstack_frame.hip ----
    ("frame_stats/null-handle", "nl_stack_frame_stats", lambda L: L.nl_stack_frame_stats(None, 0, _fl(), _fl(), _fl(), None)),
    ("frame_noise/null-handle", "nl_stack_frame_noise", lambda L: L.nl_stack_frame_noise(None, 0, _fl())),
    ("weights_from_noise/null-handle", "nl_stack_weights_from_noise", lambda L: L.nl_stack_weights_from_noise(None, None)),
    ("frame_affine/null-handle", "nl_stack_frame_affine", lambda L: L.nl_stack_frame_affine(None, 0, 1.0, 0.0)),
    ("median_mask/null-input", "nl_median_filter_mask", lambda L: L.nl_median_filter_mask(None, f(OUT), 16, mask, 3, 0)),
    ("median_mask/n-0", "nl_median_filter_mask", lambda L: L.nl_median_filter_mask(f(F), f(OUT), 0, mask, 3, 0)),
    ("median_mask/mask-0", "nl_median_filter_mask", lambda L: L.nl_median_filter_mask(f(F), f(OUT), 16, mask, 0, 0)),
    ("median_mask/valid", "nl_median_filter_mask", lambda L: L.nl_median_filter_mask(f(F), f(OUT), 16, mask, 3, 0)),
    ("median_3x3/null-output", "nl_median_filter_3x3", lambda L: L.nl_median_filter_3x3(f(F), None, W, H, 0)),
    ("median_3x3/width-0", "nl_median_filter_3x3", lambda L: L.nl_median_filter_3x3(f(F), f(OUT), 0, H, 0)),
    ("median_3x3/valid", "nl_median_filter_3x3", lambda L: L.nl_median_filter_3x3(f(F), f(OUT), W, H, 0)),
    ("frame_project_from/null-handles", "nl_stack_frame_project_from",
     lambda L: L.nl_stack_frame_project_from(None, 0, None, 0, f(T6), 0.0)),
    ("project_tile_paths/null-handles", "nl_stack_project_tile_paths",
     lambda L: L.nl_stack_project_tile_paths(None, None, 0, f(T6), _i64(), _i64())),
    # ---- nlstack_frame_pre.hip ----
    ("calib_create/neither", "nl_calib_create", lambda L: _calib(L, 0, None, W, H, None, W, H)),
    ("calib_create/dark-width-0", "nl_calib_create", lambda L: _calib(L, 0, f(F), 0, H, None, W, H)),
    ("calib_create/flat-height-0", "nl_calib_create", lambda L: _calib(L, 0, None, W, H, f(F), W, 0)),
    ("calib_create/dark-flat-mismatch", "nl_calib_create", lambda L: _calib(L, 0, f(F), W, H, f(F), 2, 8)),
    ("calib_create/dark-width-0+mismatch", "nl_calib_create", lambda L: _calib(L, 0, f(F), 0, H, f(F), 2, 8)),
    ("calib_create/valid", "nl_calib_create", lambda L: _calib(L, 0, f(F), W, H, f(F), W, H)),
    ("calib_destroy/null", "nl_calib_destroy", lambda L: L.nl_calib_destroy(None) or 0),
    ("calib_flat_max/null", "nl_calib_flat_max", lambda L: L.nl_calib_flat_max(None, _fl())),
    ("frame_calibrate/null-handle", "nl_stack_frame_calibrate", lambda L: L.nl_stack_frame_calibrate(None, 0, None)),
    ("frame_badpixel/null-handle", "nl_stack_frame_badpixel",
     lambda L: L.nl_stack_frame_badpixel(None, 0, 3.0, 5.0, _i64(), None)),
    ("preprocess_frame/null-input", "nl_preprocess_frame",
     lambda L: L.nl_preprocess_frame(None, 0, None, f(OUT), W, H, 3.0, 5.0, _i64(), None, 0)),
    ("preprocess_frame/width-0", "nl_preprocess_frame",
     lambda L: L.nl_preprocess_frame(None, 0, f(F), f(OUT), 0, H, 3.0, 5.0, _i64(), None, 0)),
    ("preprocess_frame/valid", "nl_preprocess_frame",
     lambda L: L.nl_preprocess_frame(None, 0, f(F), f(OUT), W, H, 3.0, 5.0, _i64(), None, 0)),
    ("debayer_shape/width-0", "nl_debayer_shape", lambda L: L.nl_debayer_shape(0, H, b"R", b"RGGB", _i(), _i())),
    ("debayer_shape/null-output", "nl_debayer_shape", lambda L: L.nl_debayer_shape(W, H, b"R", b"RGGB", None, _i())),
    ("debayer_shape/no-channel", "nl_debayer_shape", lambda L: L.nl_debayer_shape(W, H, b"", b"RGGB", _i(), _i())),
    ("debayer_shape/valid", "nl_debayer_shape", lambda L: L.nl_debayer_shape(W, H, b"R", b"RGGB", _i(), _i())),
    ("debayer_shape/unknown-cfa", "nl_debayer_shape", lambda L: L.nl_debayer_shape(W, H, b"R", b"XYZW", _i(), _i())),
    ("debayer_shape/unknown-channel", "nl_debayer_shape", lambda L: L.nl_debayer_shape(W, H, b"Q", b"RGGB", _i(), _i())),
    ("debayer_shape/unknown-cfa+channel", "nl_debayer_shape", lambda L: L.nl_debayer_shape(W, H, b"Q", b"XYZW", _i(), _i())),
    ("debayer_shape/empty", "nl_debayer_shape", lambda L: L.nl_debayer_shape(1, 1, b"R", b"BGGR", _i(), _i())),
    ("upload_frame_cfa/null-handle", "nl_stack_upload_frame_cfa",
     lambda L: L.nl_stack_upload_frame_cfa(None, 0, f(F), W, H, None, b"R", b"RGGB", 3.0, 5.0, _i64(), None)),
    ("preprocess_frame_cfa/null-input", "nl_preprocess_frame_cfa",
     lambda L: L.nl_preprocess_frame_cfa(None, 0, None, W, H, b"R", b"RGGB", 3.0, 5.0, f(OUT), _i(), _i(), _i64(), None, 0)),
    ("preprocess_frame_cfa/height-0", "nl_preprocess_frame_cfa",
     lambda L: L.nl_preprocess_frame_cfa(None, 0, f(F), W, 0, b"R", b"RGGB", 3.0, 5.0, f(OUT), _i(), _i(), _i64(), None, 0)),
    ("preprocess_frame_cfa/unknown-cfa", "nl_preprocess_frame_cfa",
     lambda L: L.nl_preprocess_frame_cfa(None, 0, f(F), W, H, b"R", b"XYZW", 3.0, 5.0, f(OUT), _i(), _i(), _i64(), None, 0)),
    ("preprocess_frame_cfa/valid", "nl_preprocess_frame_cfa",
     lambda L: L.nl_preprocess_frame_cfa(None, 0, f(F), W, H, b"R", b"RGGB", 3.0, 5.0, f(OUT), _i(), _i(), _i64(), None, 0)),
    ("frame_find_stars/null-handle", "nl_stack_frame_find_stars",
     lambda L: L.nl_stack_frame_find_stars(None, 0, *STAR_ARGS, stars, 2, _i(), None, None)),
    ("result_find_stars/null-handle", "nl_stack_result_find_stars",
     lambda L: L.nl_stack_result_find_stars(None, *STAR_ARGS, stars, 2, _i(), None, None)),
    ("find_stars/null-data", "nl_find_stars", lambda L: L.nl_find_stars(None, W, H, *STAR_ARGS, stars, 2, _i(), None, None, 0)),
    ("find_stars/width-0", "nl_find_stars", lambda L: L.nl_find_stars(f(F), 0, H, *STAR_ARGS, stars, 2, _i(), None, None, 0)),
    ("find_stars/capacity--1", "nl_find_stars", lambda L: L.nl_find_stars(f(F), W, H, *STAR_ARGS, stars, -1, _i(), None, None, 0)),
    ("find_stars/valid", "nl_find_stars", lambda L: L.nl_find_stars(f(F), W, H, *STAR_ARGS, stars, 2, _i(), None, None, 0)),
    ("frame_back_extract/null-handle", "nl_stack_frame_back_extract",
     lambda L: L.nl_stack_frame_back_extract(None, 0, *BACK_ARGS, stars, 2, None, f(OUT), 4, None)),
    ("back_extract/null-data", "nl_back_extract",
     lambda L: L.nl_back_extract(None, W, H, *BACK_ARGS, stars, 2, None, f(OUT), 4, None, 0)),
    ("back_extract/height-0", "nl_back_extract",
     lambda L: L.nl_back_extract(f(F), W, 0, *BACK_ARGS, stars, 2, None, f(OUT), 4, None, 0)),
    ("back_extract/n_stars--1", "nl_back_extract",
     lambda L: L.nl_back_extract(f(F), W, H, *BACK_ARGS, stars, -1, None, f(OUT), 4, None, 0)),
    ("back_extract/valid", "nl_back_extract",
     lambda L: L.nl_back_extract(f(F), W, H, *BACK_ARGS, stars, 2, None, f(OUT), 4, None, 0)),
    ("back_extract/no-grid", "nl_back_extract",
     lambda L: L.nl_back_extract(f(F), W, H, 0, 4.0, 1.5, 0, stars, 2, None, f(OUT), 4, None, 0)),
    ("frame_deband_horiz/null-handle", "nl_stack_frame_deband_horiz",
     lambda L: L.nl_stack_frame_deband_horiz(None, 0, *DEBAND_ARGS, None)),
    ("frame_deband_vert/null-handle", "nl_stack_frame_deband_vert",
     lambda L: L.nl_stack_frame_deband_vert(None, 0, *DEBAND_ARGS, None)),
    ("deband_horiz/null-data", "nl_deband_horiz", lambda L: L.nl_deband_horiz(None, W, H, *DEBAND_ARGS, None, 0)),
    ("deband_horiz/width-0", "nl_deband_horiz", lambda L: L.nl_deband_horiz(f(F), 0, H, *DEBAND_ARGS, None, 0)),
    ("deband_horiz/valid", "nl_deband_horiz", lambda L: L.nl_deband_horiz(f(F), W, H, *DEBAND_ARGS, None, 0)),
    ("deband_horiz/no-op", "nl_deband_horiz", lambda L: L.nl_deband_horiz(f(F), W, H, 0.0, 2, 3.0, 0.0, 1.0, None, 0)),
    ("deband_vert/null-data", "nl_deband_vert", lambda L: L.nl_deband_vert(None, W, H, *DEBAND_ARGS, None, 0)),
    ("deband_vert/height-0", "nl_deband_vert", lambda L: L.nl_deband_vert(f(F), W, 0, *DEBAND_ARGS, None, 0)),
    ("deband_vert/valid", "nl_deband_vert", lambda L: L.nl_deband_vert(f(F), W, H, *DEBAND_ARGS, None, 0)),
    ("bin_shape/width-0", "nl_bin_shape", lambda L: L.nl_bin_shape(0, H, 2, _i(), _i())),
    ("bin_shape/null-output", "nl_bin_shape", lambda L: L.nl_bin_shape(W, H, 2, _i(), None)),
    ("bin_shape/n-1", "nl_bin_shape", lambda L: L.nl_bin_shape(W, H, 1, _i(), _i())),
    ("bin_shape/n-2", "nl_bin_shape", lambda L: L.nl_bin_shape(W, H, 2, _i(), _i())),
    ("bin_shape/empty", "nl_bin_shape", lambda L: L.nl_bin_shape(W, H, 8, _i(), _i())),
    ("frame_bin_from/null-handles", "nl_stack_frame_bin_from", lambda L: L.nl_stack_frame_bin_from(None, 0, None, 0, 2)),
    ("bin_nxn/null-input", "nl_bin_nxn", lambda L: L.nl_bin_nxn(None, W, H, 2, f(OUT), 0)),
    ("bin_nxn/width-0", "nl_bin_nxn", lambda L: L.nl_bin_nxn(f(F), 0, H, 2, f(OUT), 0)),
    ("bin_nxn/empty", "nl_bin_nxn", lambda L: L.nl_bin_nxn(f(F), W, H, 8, f(OUT), 0)),
    ("bin_nxn/valid", "nl_bin_nxn", lambda L: L.nl_bin_nxn(f(F), W, H, 2, f(OUT), 0)),
    # ---- nlstack_frame_stretch.hip ----
    ("gaussian_kernel_1d/capacity--1", "nl_gaussian_kernel_1d", lambda L: L.nl_gaussian_kernel_1d(1.0, f(OUT), -1, _i())),
    ("gaussian_kernel_1d/capacity-no-output", "nl_gaussian_kernel_1d", lambda L: L.nl_gaussian_kernel_1d(1.0, None, 4, _i())),
    ("gaussian_kernel_1d/sigma--1", "nl_gaussian_kernel_1d", lambda L: L.nl_gaussian_kernel_1d(-1.0, f(OUT), 48, _i())),
    ("gaussian_kernel_1d/count-only", "nl_gaussian_kernel_1d", lambda L: L.nl_gaussian_kernel_1d(1.0, None, 0, _i())),
    ("gaussian_kernel_1d/valid", "nl_gaussian_kernel_1d", lambda L: L.nl_gaussian_kernel_1d(1.0, f(OUT), 48, _i())),
    ("blur_tap_paths/even", "nl_blur_tap_paths", lambda L: L.nl_blur_tap_paths(4, _i(), _i())),
    ("blur_tap_paths/n-0", "nl_blur_tap_paths", lambda L: L.nl_blur_tap_paths(0, _i(), _i())),
    ("blur_tap_paths/null-output", "nl_blur_tap_paths", lambda L: L.nl_blur_tap_paths(3, None, _i())),
    ("blur_tap_paths/valid", "nl_blur_tap_paths", lambda L: L.nl_blur_tap_paths(3, _i(), _i())),
    ("frame_gaussian_blur/null-handle", "nl_stack_frame_gaussian_blur", lambda L: L.nl_stack_frame_gaussian_blur(None, 0, 1.0)),
    ("frame_gaussian_blur/null-handle+idx--1", "nl_stack_frame_gaussian_blur",
     lambda L: L.nl_stack_frame_gaussian_blur(None, -1, 1.0)),
    ("frame_unsharp_mask/null-handle", "nl_stack_frame_unsharp_mask", lambda L: L.nl_stack_frame_unsharp_mask(None, 0, *USM_ARGS)),
    ("frame_unsharp_mask/null-handle+idx--1", "nl_stack_frame_unsharp_mask",
     lambda L: L.nl_stack_frame_unsharp_mask(None, -1, *USM_ARGS)),
    ("result_gaussian_blur/null-handle", "nl_stack_result_gaussian_blur", lambda L: L.nl_stack_result_gaussian_blur(None, 1.0)),
    ("result_unsharp_mask/null-handle", "nl_stack_result_unsharp_mask", lambda L: L.nl_stack_result_unsharp_mask(None, *USM_ARGS)),
    ("convolve_separable/null-data", "nl_convolve_separable", lambda L: L.nl_convolve_separable(None, W, H, f(TAPS3), 3, 0)),
    ("convolve_separable/width-0", "nl_convolve_separable", lambda L: L.nl_convolve_separable(f(F), 0, H, f(TAPS3), 3, 0)),
    ("convolve_separable/even-taps", "nl_convolve_separable", lambda L: L.nl_convolve_separable(f(F), W, H, f(TAPS4), 4, 0)),
    ("convolve_separable/null-taps", "nl_convolve_separable", lambda L: L.nl_convolve_separable(f(F), W, H, None, 3, 0)),
    ("convolve_separable/radius-5", "nl_convolve_separable", lambda L: L.nl_convolve_separable(f(F), W, H, f(TAPS11), 11, 0)),
    ("convolve_separable/valid", "nl_convolve_separable", lambda L: L.nl_convolve_separable(f(F), W, H, f(TAPS3), 3, 0)),
    ("gaussian_blur/null-data", "nl_gaussian_blur", lambda L: L.nl_gaussian_blur(None, W, H, 1.0, 0)),
    ("gaussian_blur/height-0", "nl_gaussian_blur", lambda L: L.nl_gaussian_blur(f(F), W, 0, 1.0, 0)),
    ("gaussian_blur/sigma-0", "nl_gaussian_blur", lambda L: L.nl_gaussian_blur(f(F), W, H, 0.0, 0)),
    ("gaussian_blur/sigma--1", "nl_gaussian_blur", lambda L: L.nl_gaussian_blur(f(F), W, H, -1.0, 0)),
    ("gaussian_blur/radius-too-large", "nl_gaussian_blur", lambda L: L.nl_gaussian_blur(f(F), W, H, 8.0, 0)),
    ("gaussian_blur/valid", "nl_gaussian_blur", lambda L: L.nl_gaussian_blur(f(F), W, H, 0.5, 0)),
    ("unsharp_mask/null-output", "nl_unsharp_mask", lambda L: L.nl_unsharp_mask(f(F), None, W, H, 0.5, 0.5, 0.0, 1.0, 0.0, 0)),
    ("unsharp_mask/width-0", "nl_unsharp_mask", lambda L: L.nl_unsharp_mask(f(F), f(OUT), 0, H, 0.5, 0.5, 0.0, 1.0, 0.0, 0)),
    ("unsharp_mask/gain-0", "nl_unsharp_mask", lambda L: L.nl_unsharp_mask(f(F), f(OUT), W, H, 0.5, 0.0, 0.0, 1.0, 0.0, 0)),
    ("unsharp_mask/radius-too-large", "nl_unsharp_mask", lambda L: L.nl_unsharp_mask(f(F), f(OUT), W, H, 8.0, 0.5, 0.0, 1.0, 0.0, 0)),
    ("unsharp_mask/valid", "nl_unsharp_mask", lambda L: L.nl_unsharp_mask(f(F), f(OUT), W, H, 0.5, 0.5, 0.0, 1.0, 0.0, 0)),
    ("frame_tone/null-handle", "nl_stack_frame_tone",
     lambda L: L.nl_stack_frame_tone(None, 0, tone_of(capi.TONE_SCALE_OFFSET, 2.0, 1.0), None, None, None)),
    ("frame_tone/null-handle+idx--1", "nl_stack_frame_tone",
     lambda L: L.nl_stack_frame_tone(None, -1, tone_of(capi.TONE_SCALE_OFFSET, 2.0, 1.0), None, None, None)),
    ("result_tone/null-handle", "nl_stack_result_tone",
     lambda L: L.nl_stack_result_tone(None, tone_of(capi.TONE_SCALE_OFFSET, 2.0, 1.0), None, None, None)),
    ("tone/null-data", "nl_tone", lambda L: L.nl_tone(None, 16, tone_of(capi.TONE_SCALE_OFFSET, 2.0, 1.0), None, None, None, 0)),
    ("tone/n-0", "nl_tone", lambda L: L.nl_tone(f(F), 0, tone_of(capi.TONE_SCALE_OFFSET, 2.0, 1.0), None, None, None, 0)),
    ("tone/null-curve", "nl_tone", lambda L: L.nl_tone(f(F), 16, None, None, None, None, 0)),
    ("tone/unknown-kind", "nl_tone", lambda L: L.nl_tone(f(F), 16, tone_of(99), None, None, None, 0)),
    ("tone/gamma-1-no-stats", "nl_tone", lambda L: L.nl_tone(f(F), 16, tone_of(capi.TONE_GAMMA, 1.0), None, None, None, 0)),
    ("tone/gamma-1-with-stats", "nl_tone", lambda L: L.nl_tone(f(F), 16, tone_of(capi.TONE_GAMMA, 1.0), _fl(), None, None, 0)),
    ("tone/valid", "nl_tone", lambda L: L.nl_tone(f(F), 16, tone_of(capi.TONE_SCALE_OFFSET, 2.0, 1.0), None, None, None, 0)),
    ("frame_export_gray/null-handle", "nl_stack_frame_export_gray",
     lambda L: L.nl_stack_frame_export_gray(None, 0, 0.0, 1.0, 1.0, 16, raw)),
    ("frame_export_gray/null-handle+idx--1", "nl_stack_frame_export_gray",
     lambda L: L.nl_stack_frame_export_gray(None, -1, 0.0, 1.0, 1.0, 16, raw)),
    ("result_export_gray/null-handle", "nl_stack_result_export_gray",
     lambda L: L.nl_stack_result_export_gray(None, 0.0, 1.0, 1.0, 16, raw)),
    ("export_gray/null-data", "nl_export_gray", lambda L: L.nl_export_gray(None, 16, 0.0, 1.0, 1.0, 16, raw, 0)),
    ("export_gray/n-0", "nl_export_gray", lambda L: L.nl_export_gray(f(F), 0, 0.0, 1.0, 1.0, 16, raw, 0)),
    ("export_gray/null-output", "nl_export_gray", lambda L: L.nl_export_gray(f(F), 16, 0.0, 1.0, 1.0, 16, None, 0)),
    ("export_gray/bits-12", "nl_export_gray", lambda L: L.nl_export_gray(f(F), 16, 0.0, 1.0, 1.0, 12, raw, 0)),
    ("export_gray/gamma-0", "nl_export_gray", lambda L: L.nl_export_gray(f(F), 16, 0.0, 1.0, 0.0, 16, raw, 0)),
    ("export_gray/bits-12+gamma-0", "nl_export_gray", lambda L: L.nl_export_gray(f(F), 16, 0.0, 1.0, 0.0, 12, raw, 0)),
    ("export_gray/valid", "nl_export_gray", lambda L: L.nl_export_gray(f(F), 16, 0.0, 1.0, 1.0, 16, raw, 0)),
    # ---- nlstack_frame_rgb.hip ----
    ("rgb_normalization/null", "nl_rgb_normalization", lambda L: L.nl_rgb_normalization(f(V3), None, _fl(), _fl())),
    ("rgb_normalization/valid", "nl_rgb_normalization", lambda L: L.nl_rgb_normalization(f(V3), f(V3), _fl(), _fl())),
    ("rgb_balance_coeffs/null-output", "nl_rgb_balance_coeffs",
     lambda L: L.nl_rgb_balance_coeffs(ZERO, ONE, ZERO, ONE, f(OUT), None)),
    ("rgb_balance_coeffs/valid", "nl_rgb_balance_coeffs",
     lambda L: L.nl_rgb_balance_coeffs(ZERO, ONE, ZERO, ONE, f(OUT), f(OUT))),
    ("frame_combine_from/null-handles", "nl_stack_frame_combine_from",
     lambda L: L.nl_stack_frame_combine_from(None, 0, None, 0, 0.0, 1.0)),
    ("rgb_scale_offset_clamp/null-handle", "nl_stack_rgb_scale_offset_clamp",
     lambda L: L.nl_stack_rgb_scale_offset_clamp(None, PLANES, f(V3), f(V3), None)),
    ("rgb_darkest_block/null-handle", "nl_stack_rgb_darkest_block",
     lambda L: L.nl_stack_rgb_darkest_block(None, PLANES, 2, 0.0, C.byref(capi.Rgb()))),
    ("rgb_mean_star_intensity/null-handle", "nl_stack_rgb_mean_star_intensity",
     lambda L: L.nl_stack_rgb_mean_star_intensity(None, PLANES, stars, 2, 0.0, 0.0, ONE, C.byref(capi.Rgb()))),
    ("stack_rgb_balance/null-handle", "nl_stack_rgb_balance",
     lambda L: L.nl_stack_rgb_balance(None, PLANES, stars, 2, *BALANCE_TAIL)),
    ("rgb_chroma/null-handle", "nl_stack_rgb_chroma",
     lambda L: L.nl_stack_rgb_chroma(None, PLANES, chroma_of(capi.CHROMA_GAMMA, 1.0, 0.0))),
    ("rgb_chroma/null-handle+unknown-kind", "nl_stack_rgb_chroma", lambda L: L.nl_stack_rgb_chroma(None, PLANES, chroma_of(99))),
    ("rgb_export/null-handle", "nl_stack_rgb_export", lambda L: L.nl_stack_rgb_export(None, PLANES, 0.0, 1.0, 1.0, 16, raw)),
    ("rgb_export/null-handle+bits-12", "nl_stack_rgb_export",
     lambda L: L.nl_stack_rgb_export(None, PLANES, 0.0, 1.0, 1.0, 12, raw)),
    ("rgb_balance/null-data", "nl_rgb_balance", lambda L: L.nl_rgb_balance(None, W, H, stars, 2, *BALANCE_TAIL, 0)),
    ("rgb_balance/width-0", "nl_rgb_balance", lambda L: L.nl_rgb_balance(f(P3), 0, H, stars, 2, *BALANCE_TAIL, 0)),
    ("rgb_balance/block-0", "nl_rgb_balance",
     lambda L: L.nl_rgb_balance(f(P3), W, H, stars, 2, 0, 0.0, 0.0, 0.0, ZERO, ONE, f(V3), f(V3), None, 0)),
    ("rgb_balance/valid", "nl_rgb_balance", lambda L: L.nl_rgb_balance(f(P3), W, H, stars, 2, *BALANCE_TAIL, 0)),
    ("export_rgb/null-data", "nl_export_rgb", lambda L: L.nl_export_rgb(None, 16, 0.0, 1.0, 1.0, 16, raw, 0)),
    ("export_rgb/n-0", "nl_export_rgb", lambda L: L.nl_export_rgb(f(P3), 0, 0.0, 1.0, 1.0, 16, raw, 0)),
    ("export_rgb/null-output", "nl_export_rgb", lambda L: L.nl_export_rgb(f(P3), 16, 0.0, 1.0, 1.0, 16, None, 0)),
    ("export_rgb/bits-12", "nl_export_rgb", lambda L: L.nl_export_rgb(f(P3), 16, 0.0, 1.0, 1.0, 12, raw, 0)),
    ("export_rgb/gamma-0", "nl_export_rgb", lambda L: L.nl_export_rgb(f(P3), 16, 0.0, 1.0, 0.0, 16, raw, 0)),
    ("export_rgb/n-0+bits-12", "nl_export_rgb", lambda L: L.nl_export_rgb(f(P3), 0, 0.0, 1.0, 1.0, 12, raw, 0)),
    ("export_rgb/valid", "nl_export_rgb", lambda L: L.nl_export_rgb(f(P3), 16, 0.0, 1.0, 1.0, 16, raw, 0)),
]

NO_DEVICE_TEXT = "no HIP device available (no ROCm-capable device is detected); libnlstack has no CPU path"
NO_DEVICE = (capi.ERR_NO_DEVICE, NO_DEVICE_TEXT)
UNTOUCHED = (capi.OK, SENTINEL)           # the call succeeded and left the thread's error as it was

EXPECTED = {
    "frame_stats/null-handle": (-6, "null handle"),
    "frame_noise/null-handle": (-6, "null handle"),
    "weights_from_noise/null-handle": (-6, "null handle"),
    "frame_affine/null-handle": (-6, "null handle"),
    "median_mask/null-input": (-6, "median_filter_mask: bad argument (mask of 1..32 offsets)"),
    "median_mask/n-0": (-6, "median_filter_mask: bad argument (mask of 1..32 offsets)"),
    "median_mask/mask-0": (-6, "median_filter_mask: bad argument (mask of 1..32 offsets)"),
    "median_mask/valid": NO_DEVICE,
    "median_3x3/null-output": (-6, "median_filter_3x3: bad argument"),
    "median_3x3/width-0": (-6, "median_filter_3x3: bad argument"),
    "median_3x3/valid": NO_DEVICE,
    "frame_project_from/null-handles": (-6, "null handle"),
    "project_tile_paths/null-handles": (-6, "project_tile_paths: null argument"),
    "calib_create/neither": (0, "calib_create: neither a dark nor a flat"),
    "calib_create/dark-width-0": (0, "calib_create: bad master dimensions"),
    "calib_create/flat-height-0": (0, "calib_create: bad master dimensions"),
    "calib_create/dark-flat-mismatch": (0, "dark dimensions [4 4] differ from flat dimensions [2 8]"),
    "calib_create/dark-width-0+mismatch": (0, "calib_create: bad master dimensions"),
    "calib_create/valid": (0, NO_DEVICE_TEXT),
    "calib_destroy/null": UNTOUCHED,
    "calib_flat_max/null": (-6, "calib_flat_max: null argument"),
    "frame_calibrate/null-handle": (-6, "null handle"),
    "frame_badpixel/null-handle": (-6, "null handle"),
    "preprocess_frame/null-input": (-6, "preprocess_frame: bad argument"),
    "preprocess_frame/width-0": (-6, "preprocess_frame: bad argument"),
    "preprocess_frame/valid": NO_DEVICE,
    "debayer_shape/width-0": (-6, "debayer_shape: bad argument"),
    "debayer_shape/null-output": (-6, "debayer_shape: bad argument"),
    "debayer_shape/no-channel": UNTOUCHED,
    "debayer_shape/valid": UNTOUCHED,
    "debayer_shape/unknown-cfa": (-6, "Unknown CFA value XYZW"),
    "debayer_shape/unknown-channel": (-6, "Unknown debayering value Q"),
    "debayer_shape/unknown-cfa+channel": (-6, "Unknown CFA value XYZW"),
    "debayer_shape/empty": (-6, "debayer: 1x1 mosaic with cfa BGGR gives an empty 0x0 image"),
    "upload_frame_cfa/null-handle": NO_DEVICE,
    "preprocess_frame_cfa/null-input": (-6, "preprocess_frame_cfa: bad argument"),
    "preprocess_frame_cfa/height-0": (-6, "preprocess_frame_cfa: bad argument"),
    "preprocess_frame_cfa/unknown-cfa": NO_DEVICE,
    "preprocess_frame_cfa/valid": NO_DEVICE,
    "frame_find_stars/null-handle": (-6, "null handle"),
    "result_find_stars/null-handle": (-6, "null handle"),
    "find_stars/null-data": (-6, "find_stars: bad argument"),
    "find_stars/width-0": (-6, "find_stars: bad argument"),
    "find_stars/capacity--1": NO_DEVICE,
    "find_stars/valid": NO_DEVICE,
    "frame_back_extract/null-handle": (-6, "null handle"),
    "back_extract/null-data": (-6, "back_extract: bad argument"),
    "back_extract/height-0": (-6, "back_extract: bad argument"),
    "back_extract/n_stars--1": NO_DEVICE,
    "back_extract/valid": NO_DEVICE,
    "back_extract/no-grid": NO_DEVICE,
    "frame_deband_horiz/null-handle": (-6, "null handle"),
    "frame_deband_vert/null-handle": (-6, "null handle"),
    "deband_horiz/null-data": (-6, "deband_horiz: bad argument"),
    "deband_horiz/width-0": (-6, "deband_horiz: bad argument"),
    "deband_horiz/valid": NO_DEVICE,
    "deband_horiz/no-op": NO_DEVICE,
    "deband_vert/null-data": (-6, "deband_vert: bad argument"),
    "deband_vert/height-0": (-6, "deband_vert: bad argument"),
    "deband_vert/valid": NO_DEVICE,
    "bin_shape/width-0": (-6, "bin_shape: bad argument"),
    "bin_shape/null-output": (-6, "bin_shape: bad argument"),
    "bin_shape/n-1": UNTOUCHED,
    "bin_shape/n-2": UNTOUCHED,
    "bin_shape/empty": (-6, "NewImageBinNxN (fits.go:163-195): 4x4 binned by 8 gives an empty 0x0 image"),
    "frame_bin_from/null-handles": (-6, "null handle"),
    "bin_nxn/null-input": (-6, "bin_nxn: bad argument"),
    "bin_nxn/width-0": (-6, "bin_nxn: bad argument"),
    "bin_nxn/empty": NO_DEVICE,
    "bin_nxn/valid": NO_DEVICE,
    "gaussian_kernel_1d/capacity--1": (-6, "gaussian_kernel_1d: capacity -1 with an output"),
    "gaussian_kernel_1d/capacity-no-output": (-6, "gaussian_kernel_1d: capacity 4 with no output"),
    "gaussian_kernel_1d/sigma--1": (-6, "gaussian_kernel_1d: GaussianKernel1D (usm.go:41-82) cannot take sigma -1.000000: its radius search (usm.go:47-54) does not end"),
    "gaussian_kernel_1d/count-only": (-6, "gaussian_kernel_1d: sigma 1 gives 3 taps, capacity 0"),
    "gaussian_kernel_1d/valid": UNTOUCHED,
    "blur_tap_paths/even": (-6, "blur_tap_paths: bad argument"),
    "blur_tap_paths/n-0": (-6, "blur_tap_paths: bad argument"),
    "blur_tap_paths/null-output": (-6, "blur_tap_paths: bad argument"),
    "blur_tap_paths/valid": UNTOUCHED,
    "frame_gaussian_blur/null-handle": (-6, "null handle"),
    "frame_gaussian_blur/null-handle+idx--1": (-6, "null handle"),
    "frame_unsharp_mask/null-handle": (-6, "null handle"),
    "frame_unsharp_mask/null-handle+idx--1": (-6, "null handle"),
    "result_gaussian_blur/null-handle": (-6, "null handle"),
    "result_unsharp_mask/null-handle": (-6, "null handle"),
    "convolve_separable/null-data": (-6, "convolve_separable: bad argument"),
    "convolve_separable/width-0": (-6, "convolve_separable: bad argument"),
    "convolve_separable/even-taps": (-6, "convolve_separable: 4 taps: Convolve1DX / Convolve1DY (usm.go:85-114) index kernel[i + k] for i = -k .. k, an odd positive count"),
    "convolve_separable/null-taps": (-6, "convolve_separable: 3 taps: Convolve1DX / Convolve1DY (usm.go:85-114) index kernel[i + k] for i = -k .. k, an odd positive count"),
    "convolve_separable/radius-5": (-6, "convolve_separable: a radius of 5 on a 4x4 frame: one reflect (usm.go:25-33) leaves the range"),
    "convolve_separable/valid": NO_DEVICE,
    "gaussian_blur/null-data": (-6, "gaussian_blur: bad argument"),
    "gaussian_blur/height-0": (-6, "gaussian_blur: bad argument"),
    "gaussian_blur/sigma-0": UNTOUCHED,
    "gaussian_blur/sigma--1": (-6, "gaussian_blur: GaussianKernel1D (usm.go:41-82) cannot take sigma -1.000000: its radius search (usm.go:47-54) does not end"),
    "gaussian_blur/radius-too-large": (-6, "gaussian_blur: a radius of 18 on a 4x4 frame: one reflect (usm.go:25-33) leaves the range"),
    "gaussian_blur/valid": NO_DEVICE,
    "unsharp_mask/null-output": (-6, "unsharp_mask: bad argument"),
    "unsharp_mask/width-0": (-6, "unsharp_mask: bad argument"),
    "unsharp_mask/gain-0": UNTOUCHED,
    "unsharp_mask/radius-too-large": (-6, "unsharp_mask: a radius of 18 on a 4x4 frame: one reflect (usm.go:25-33) leaves the range"),
    "unsharp_mask/valid": NO_DEVICE,
    "frame_tone/null-handle": (-6, "null handle"),
    "frame_tone/null-handle+idx--1": (-6, "null handle"),
    "result_tone/null-handle": (-6, "null handle"),
    "tone/null-data": (-6, "tone: bad argument"),
    "tone/n-0": (-6, "tone: bad argument"),
    "tone/null-curve": (-6, "tone: null curve"),
    "tone/unknown-kind": (-6, "tone: unknown kind 99 (NL_TONE_SCALE_OFFSET ... NL_TONE_SHIFT_BLACK)"),
    "tone/gamma-1-no-stats": UNTOUCHED,
    "tone/gamma-1-with-stats": NO_DEVICE,
    "tone/valid": NO_DEVICE,
    "frame_export_gray/null-handle": (-6, "null handle"),
    "frame_export_gray/null-handle+idx--1": (-6, "null handle"),
    "result_export_gray/null-handle": (-6, "null handle"),
    "export_gray/null-data": (-6, "export_gray: bad argument"),
    "export_gray/n-0": (-6, "export_gray: bad argument"),
    "export_gray/null-output": (-6, "export_gray: null output"),
    "export_gray/bits-12": (-6, "export_gray: 12 bits (8: image.Gray, 16: image.Gray16)"),
    "export_gray/gamma-0": (-6, "export_gray: gamma 0 (tiff16.go:113, writejpg.go:111: a positive number)"),
    "export_gray/bits-12+gamma-0": (-6, "export_gray: 12 bits (8: image.Gray, 16: image.Gray16)"),
    "export_gray/valid": NO_DEVICE,
    "rgb_normalization/null": (-6, "rgb_normalization: null argument"),
    "rgb_normalization/valid": UNTOUCHED,
    "rgb_balance_coeffs/null-output": (-6, "rgb_balance_coeffs: null output"),
    "rgb_balance_coeffs/valid": UNTOUCHED,
    "frame_combine_from/null-handles": NO_DEVICE,
    "rgb_scale_offset_clamp/null-handle": NO_DEVICE,
    "rgb_darkest_block/null-handle": NO_DEVICE,
    "rgb_mean_star_intensity/null-handle": NO_DEVICE,
    "stack_rgb_balance/null-handle": NO_DEVICE,
    "rgb_chroma/null-handle": NO_DEVICE,
    "rgb_chroma/null-handle+unknown-kind": NO_DEVICE,
    "rgb_export/null-handle": NO_DEVICE,
    "rgb_export/null-handle+bits-12": NO_DEVICE,
    "rgb_balance/null-data": (-6, "rgb_balance: bad argument"),
    "rgb_balance/width-0": (-6, "rgb_balance: bad argument"),
    "rgb_balance/block-0": NO_DEVICE,
    "rgb_balance/valid": NO_DEVICE,
    "export_rgb/null-data": (-6, "export_rgb: bad argument"),
    "export_rgb/n-0": (-6, "export_rgb: bad argument"),
    "export_rgb/null-output": (-6, "export_rgb: null output"),
    "export_rgb/bits-12": (-6, "export_rgb: 12 bits (8: image.Gray, 16: image.Gray16)"),
    "export_rgb/gamma-0": (-6, "export_rgb: gamma 0 (tiff16.go:113, writejpg.go:111: a positive number)"),
    "export_rgb/n-0+bits-12": (-6, "export_rgb: bad argument"),
    "export_rgb/valid": NO_DEVICE,
}


def run_row(L, call):
    """(return code, nl_last_error()) of one row, after the sentinel error"""
    bad = C.c_int(-1)
    w = np.zeros(1, np.float32)
    assert L.nl_weights_from_scalars(7, f(w), 1, f(w), C.byref(bad)) == capi.ERR_INVALID_WEIGHTING
    assert L.nl_last_error().decode().startswith(SENTINEL)
    rc = call(L)
    msg = L.nl_last_error().decode("utf-8", "replace")
    return rc, (SENTINEL if msg.startswith(SENTINEL) else msg)


def frame_entries():
    return sorted(set(capi.EXPORTS) - ELSEWHERE)


def test_every_frame_entry_has_a_row():
    assert ELSEWHERE <= set(capi.EXPORTS)
    covered = {entry for _, entry, _ in ROWS}
    assert covered <= set(frame_entries())
    missing = [e for e in frame_entries() if e not in covered]
    assert not missing, "entries of the frame units without a row: %s" % missing
    ids = [rid for rid, _, _ in ROWS]
    assert len(set(ids)) == len(ids) and set(ids) == set(EXPECTED)


def test_codes_and_messages_without_a_device():
    L = capi.load()
    if capi.device_count() > 0:
        pytest.skip("a HIP device is visible: the table holds what a machine without one answers")
    got = {rid: run_row(L, call) for rid, _, call in ROWS}
    wrong = {rid: (got[rid], EXPECTED[rid]) for rid in got if got[rid] != EXPECTED[rid]}
    assert not wrong, "(got, expected) per row: %r" % wrong
