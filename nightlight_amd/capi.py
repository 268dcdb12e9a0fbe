"""ctypes binding of the C ABI in include/nlstack.h (libnlstack.so).

Plumbing only: loads the in-tree HIP library and declares its prototypes.
There is no CPU fallback -- if the library is missing, or no HIP device is
visible, the compute entry points raise NlError.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
# NLSTACK_LIB: another build of the same library (A/B timing of kernel variants)
LIB_PATH = os.environ.get("NLSTACK_LIB") or os.path.join(_PKG, "libnlstack.so")

ST_MEDIAN, ST_MEAN, ST_SIGMA, ST_WINSOR_SIGMA, ST_MAD_SIGMA, ST_LINEAR_FIT, ST_AUTO = range(7)
WEIGHT_NONE, WEIGHT_EXPOSURE, WEIGHT_INVERSE_NOISE, WEIGHT_INVERSE_HFR = range(4)
TONE_SCALE_OFFSET, TONE_NORMALIZE, TONE_GAMMA, TONE_PARTIAL_GAMMA, TONE_MIDTONES, TONE_SHIFT_BLACK = range(6)
CHROMA_GAMMA, CHROMA_NEUTRALIZE, CHROMA_FOR_HUES, ROTATE_HUES = range(4)
LSE_MEAN_STDDEV, LSE_MEDIAN_MAD, LSE_IKSS, LSE_SC_MEDIAN_QN, LSE_HISTOGRAM = range(5)     # stats.go:31-37
LOCSCALE_SAMPLES = 131072
LOCSCALE_MAX_SEEDS = 25
ALIGN_MAX_K = 128

OK = 0
ERR_INVALID_MODE = -1
ERR_MISSING_EXPOSURE = -2
ERR_INVALID_WEIGHTING = -3
ERR_WEIGHTED_MAD = -4
ERR_NO_INPUTS = -5
ERR_INVALID_ARG = -6
ERR_HIP = -7
ERR_TOO_MANY_FRAMES = -8
ERR_NO_DEVICE = -9

# every symbol include/nlstack.h declares (tests check the library exports them)
EXPORTS = [
    "nl_last_error", "nl_device_count", "nl_version",
    "nl_stack_create", "nl_stack_destroy",
    "nl_stack_upload_frame", "nl_stack_upload_tile", "nl_stack_upload_frame_async", "nl_stack_upload_wait", "nl_stack_frames_device_ptr", "nl_stack_device_bytes", "nl_release_cached_memory",
    "nl_fits_parse_header", "nl_fits_write_header", "nl_fits_padded_bytes",
    "nl_stack_attach_device_frames", "nl_stack_attach_device_frames_strided", "nl_stack_frame_stride", "nl_stack_fill_synthetic", "nl_stack_download_tile", "nl_stack_download_rows",
    "nl_stack_set_active_frames", "nl_stack_set_weights", "nl_weights_from_scalars",
    "nl_stack_linfit_stage_counts", "nl_stack_run", "nl_stack_run_async", "nl_stack_finish", "nl_stack_result_device_ptr",
    "nl_stack_last_mode", "nl_stack_last_kernel_ms", "nl_stack_last_dominant_kernel_ms",
    "nl_stack_last_kernel_name", "nl_stack_pass_times", "nl_stack_stream", "nl_stack_counters_device_ptr", "nl_stack_copy_counters_async", "nl_stack_set_counters_buffer", "nl_stack_order_stream_after",
    "nl_group_tile_rows", "nl_group_create", "nl_group_destroy", "nl_group_size", "nl_group_tile",
    "nl_group_upload_frame", "nl_group_fill_synthetic", "nl_group_set_active_frames", "nl_group_set_weights", "nl_group_set_exact",
    "nl_group_run", "nl_group_last_mode", "nl_group_find_sigmas", "nl_group_accumulate",
    "nl_group_accumulate_finalize",
    "nl_stack_set_exact", "nl_stack_set_dev_flags", "nl_stack_last_fallback_pixels", "nl_stack_last_generic_pixels", "nl_stack_last_pass_protocol",
    "nl_stack_find_sigmas", "nl_stack_accumulate", "nl_stack_accumulate_finalize",
    "nl_stack_frame_stats", "nl_stack_frame_noise", "nl_stack_weights_from_noise",
    "nl_median_filter_3x3", "nl_median_filter_mask",
    "nl_stack_upload_frame_fits", "nl_stack_upload_frame_projected", "nl_stack_frame_affine",
    "nl_stack_upload_frame_fits_async", "nl_stack_upload_frame_projected_async",
    "nl_group_upload_frame_fits", "nl_group_upload_frame_projected",
    "nl_stack_download_result_fits", "nl_fits_decode", "nl_project_bilinear",
    "nl_host_op_stack_apply_json", "nl_host_op_stack_roundtrip_json", "nl_host_set_devices",
    "nl_host_op_stack_batches_apply_json",
    "nl_calib_create", "nl_calib_destroy", "nl_calib_flat_max", "nl_preprocess_frame",
    "nl_stack_frame_calibrate", "nl_stack_frame_badpixel",
    "nl_debayer_shape", "nl_preprocess_frame_cfa", "nl_stack_upload_frame_cfa",
    "nl_find_stars", "nl_stack_frame_find_stars", "nl_stack_result_find_stars",
    "nl_back_extract", "nl_stack_frame_back_extract",
    "nl_deband_horiz", "nl_deband_vert", "nl_stack_frame_deband_horiz", "nl_stack_frame_deband_vert",
    "nl_bin_shape", "nl_bin_nxn", "nl_stack_frame_bin_from",
    "nl_gaussian_kernel_1d", "nl_convolve_separable", "nl_gaussian_blur", "nl_unsharp_mask",
    "nl_stack_frame_gaussian_blur", "nl_stack_frame_unsharp_mask", "nl_stack_result_gaussian_blur",
    "nl_stack_result_unsharp_mask", "nl_blur_tap_paths",
    "nl_stack_frame_tone", "nl_stack_result_tone", "nl_tone",
    "nl_stack_frame_export_gray", "nl_stack_result_export_gray", "nl_export_gray",
    "nl_stack_frame_project_from", "nl_group_frame_project_from", "nl_stack_project_tile_paths",
    "nl_rgb_normalization", "nl_stack_frame_combine_from", "nl_stack_rgb_scale_offset_clamp",
    "nl_stack_rgb_darkest_block", "nl_stack_rgb_mean_star_intensity", "nl_rgb_balance_coeffs", "nl_stack_rgb_balance",
    "nl_rgb_balance", "nl_stack_rgb_chroma", "nl_stack_rgb_export", "nl_export_rgb",
]

# every symbol include/nlstack_locscale.h declares (the part of the interface nlstack.h includes)
LOCSCALE_EXPORTS = ["nl_stack_frame_location_scale", "nl_location_scale", "nl_locscale_seeds"]

# every symbol include/nlstack_maps.h declares (likewise)
MAPS_EXPORTS = ["nl_stack_run_maps", "nl_stack_coverage", "nl_stack_last_coverage_ms", "nl_group_run_maps",
                "nl_group_coverage"]

# every symbol include/nlstack_fastmaps.h declares (likewise): the maps pass on the default pass's engines
FASTMAPS_EXPORTS = ["nl_stack_run_maps_fast", "nl_group_run_maps_fast"]

# every symbol include/nlstack_residentmaps.h declares (likewise): the maps pass on the register-resident engines, the
# linear fit's kernels and cascade included
RESIDENTMAPS_EXPORTS = ["nl_stack_run_maps_resident", "nl_group_run_maps_resident"]

# every symbol include/nlstack_deepmaps.h declares (likewise): the maps pass with the LDS-column engines of deep
# (129 ... 512 frames) sigma / winsorized stacks as well
DEEPMAPS_EXPORTS = ["nl_stack_run_maps_deep", "nl_group_run_maps_deep"]

# every symbol include/nlstack_fullmaps.h declares (likewise): the maps pass with the MAD-sigma engines (1 ... 512 frames)
# and the median's default kernels as well
FULLMAPS_EXPORTS = ["nl_stack_run_maps_full", "nl_group_run_maps_full"]

# every symbol include/nlstack_wlinfit.h declares (likewise): the weighted linear-fit pass, an extension
WLINFIT_EXPORTS = ["nl_stack_run_linfit_weighted", "nl_stack_run_linfit_weighted_async", "nl_group_run_linfit_weighted"]

# every symbol include/nlstack_wclip.h declares (likewise): weighted sigma / winsorized clipping whose weights follow
# their frames, an extension
WCLIP_EXPORTS = ["nl_stack_run_clip_weighted", "nl_stack_run_clip_weighted_async", "nl_group_run_clip_weighted"]

# every symbol include/nlstack_wmad.h declares (likewise): weighted MAD-sigma stacking whose weights follow their frames,
# an extension
WMAD_EXPORTS = ["nl_stack_run_mad_weighted", "nl_stack_run_mad_weighted_async", "nl_group_run_mad_weighted"]

# every symbol include/nlstack_deepstack.h declares (likewise): the median and MAD sigma of 513 ... 2048 frames on
# register-resident engines, an extension of depth
DEEPSTACK_EXPORTS = ["nl_stack_run_deepstack", "nl_stack_run_deepstack_async", "nl_group_run_deepstack"]

# every symbol include/nlstack_deepstackmaps.h declares (likewise): the maps pass with the engines of stacks beyond 512
# frames as well -- MAD sigma and the median on 8 / 16 lanes per pixel, sigma / winsorized clipping on the wave-per-pixel replay
DEEPSTACKMAPS_EXPORTS = ["nl_stack_run_maps_deepstack", "nl_group_run_maps_deepstack"]

# every symbol include/nlstack_deepwmad.h declares (likewise): weighted MAD-sigma stacking of 513 ... 2048 frames on the
# 8- / 16-lane engine, an extension of depth
DEEPWMAD_EXPORTS = ["nl_stack_run_mad_weighted_deepstack", "nl_stack_run_mad_weighted_deepstack_async",
                    "nl_group_run_mad_weighted_deepstack"]

# every symbol include/nlstack_align.h declares (likewise)
ALIGN_EXPORTS = ["nl_aligner_create", "nl_aligner_destroy", "nl_aligner_info", "nl_aligner_match",
                 "nl_aligner_match_stars"]

# every symbol include/nlstack_resample.h declares (likewise): bicubic / Lanczos-3 resampling of the resident projection,
# an extension
RESAMPLE_EXPORTS = ["nl_resample_lanczos3_table", "nl_stack_frame_resample_from", "nl_group_frame_resample_from",
                    "nl_stack_resample_tile_paths"]
RS_BILINEAR, RS_BICUBIC, RS_LANCZOS3 = range(3)
RS_PHASES = 1024

# every symbol include/nlstack_drizzle.h declares (likewise): drizzle integration of resident frames onto a finer output
# grid and the rejection step in front of it, an extension
DRIZZLE_EXPORTS = ["nl_drizzle_geometry", "nl_stack_frame_drizzle_from", "nl_stack_drizzle_finalize",
                   "nl_stack_frame_reject_against", "nl_stack_drizzle_tile_paths"]
DZ_TURBO, DZ_POINT = range(2)
DZ_MAX_RADIUS = 3

# every symbol include/nlstack_cfadrizzle.h declares (likewise): CFA drizzle -- a raw Bayer mosaic laid onto one colour
# plane with no debayer in front -- and the resident rejection and bad-pixel steps of a mosaic, an extension
CFADRIZZLE_EXPORTS = ["nl_drizzle_cfa_transform", "nl_stack_frame_drizzle_cfa_from", "nl_stack_frame_reject_against_cfa",
                      "nl_stack_frame_badpixel_cfa"]

# every symbol include/nlstack_sqdrizzle.h declares (likewise): the square drizzle kernel -- the exact overlap of a
# rotated drop with an output pixel -- for mono frames and for one channel of a mosaic, an extension
SQDRIZZLE_EXPORTS = ["nl_drizzle_square_geometry", "nl_stack_frame_drizzle_square_from",
                     "nl_stack_frame_drizzle_square_cfa_from", "nl_stack_drizzle_square_tile_paths"]

# nl_star_t = star.Star (findstars.go:30-37), 24 bytes
STAR_DTYPE = np.dtype([("index", "<i4"), ("value", "<f4"), ("x", "<f4"), ("y", "<f4"), ("mass", "<f4"),
                       ("hfr", "<f4")])
assert STAR_DTYPE.itemsize == 24
# nl_align_triangle_t = star.Triangle (align.go:39-46), 24 bytes; nl_align_candidate_t, 72 bytes
TRIANGLE_DTYPE = np.dtype([("d_ab", "<f4"), ("d_ac", "<f4"), ("d_bc", "<f4"), ("a", "<i4"), ("b", "<i4"), ("c", "<i4")])
CANDIDATE_DTYPE = np.dtype([("dist", "<f4"), ("tri_index", "<i4"), ("ref_tri_index", "<i4"), ("a", "<i4"), ("b", "<i4"),
                            ("c", "<i4"), ("ref_a", "<i4"), ("ref_b", "<i4"), ("ref_c", "<i4"), ("trans", "<f4", (6,)),
                            ("trans_ok", "<i4"), ("num_matches", "<i4"), ("enough", "<i4")])
assert TRIANGLE_DTYPE.itemsize == 24 and CANDIDATE_DTYPE.itemsize == 72




class Background(C.Structure):
    """nl_background_t: what Background.String() prints (background.go:48-52), plus the geometry."""
    _fields_ = [("cells_x", C.c_int32), ("cells_y", C.c_int32), ("outlier_cells", C.c_int32),
                ("spacing_x", C.c_float), ("spacing_y", C.c_float), ("min", C.c_float), ("max", C.c_float)]


class Deband(C.Structure):
    """nl_deband_t: what the debanding operators' log lines print (banding.go:129, :267)."""
    _fields_ = [("threshold", C.c_float), ("lowest", C.c_float), ("highest", C.c_float)]


class LocScale(C.Structure):
    """nl_locscale_t: how an estimate of location and scale came about."""
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("seeds_used", C.c_int32),
                ("draws", C.c_uint32 * LOCSCALE_MAX_SEEDS), ("min", C.c_float), ("max", C.c_float),
                ("epsilon", C.c_float), ("peak_bin", C.c_uint32), ("peak_count", C.c_uint32),
                ("half_width", C.c_uint32)]


class AlignInfo(C.Structure):
    """nl_align_info_t: how a match came about; the three pointers are the caller's optional buffers."""
    _fields_ = [("triangles", C.c_void_p), ("tri_dist", C.POINTER(C.c_float)), ("tri_ref", C.POINTER(C.c_int32)),
                ("tri_capacity", C.c_int32), ("n_picked", C.c_int32), ("n_triangles", C.c_int32),
                ("scale_factor", C.c_float), ("picked", C.c_int32 * ALIGN_MAX_K)]


class Tone(C.Structure):
    """nl_tone_t: one curve of the stretch command, the kind and the pixel function's arguments."""
    _fields_ = [("kind", C.c_int32), ("p", C.c_float * 3)]


class Rgb(C.Structure):
    """nl_rgb_t: fits.RGB (rgb.go:28-32)."""
    _fields_ = [("r", C.c_float), ("g", C.c_float), ("b", C.c_float)]


class RgbBalance(C.Structure):
    """nl_rgb_balance_t: what SetBlackWhitePoints logs."""
    _fields_ = [("alpha1", C.c_float * 3), ("beta1", C.c_float * 3), ("alpha2", C.c_float * 3),
                ("beta2", C.c_float * 3), ("darkest", Rgb), ("stars", Rgb)]


class Chroma(C.Structure):
    """nl_chroma_t: one chroma or hue step of the OpHSL... operators, the kind and the pixel function's arguments."""
    _fields_ = [("kind", C.c_int32), ("p", C.c_float * 4)]


class NlError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("nlstack error %d: %s" % (code, message))
        self.code = code
        self.message = message


REDUCE_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_int64), C.c_void_p)

_lib = None
_f32p = C.POINTER(C.c_float)
_i64p = C.POINTER(C.c_int64)
_intp = C.POINTER(C.c_int)


class FitsHeader(C.Structure):
    """nl_fits_header_t (include/nlstack.h)"""
    _fields_ = [("bitpix", C.c_int32), ("naxis", C.c_int32), ("naxisn", C.c_int32 * 8),
                ("bzero", C.c_float), ("bscale", C.c_float), ("exposure", C.c_float),
                ("pixels", C.c_int64), ("header_bytes", C.c_int64), ("payload_bytes", C.c_int64),
                ("padded_payload_bytes", C.c_int64)]


def load():
    """Load libnlstack.so (built in-tree by __graft_entry__.build())."""
    global _lib
    if _lib is None:
        _lib = open_library(LIB_PATH)
    return _lib


def open_library(path):
    """Open the build of the library at `path` with every prototype declared (load() opens LIB_PATH this way; another
    build can be opened beside it for A/B comparisons in one process)."""
    if not os.path.exists(path):
        raise NlError(ERR_NO_DEVICE, "%s is not built; run "
                      "`python -c 'import __graft_entry__ as g; g.build()'`" % path)
    try:  # if torch is used in this process, let its bundled HIP runtime load first
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the C ABI
        pass
    L = C.CDLL(path)
    vp = C.c_void_p
    L.nl_last_error.restype = C.c_char_p
    L.nl_version.restype = C.c_char_p
    L.nl_device_count.restype = C.c_int
    L.nl_stack_create.argtypes = [C.c_int] * 6
    L.nl_stack_create.restype = vp
    L.nl_stack_destroy.argtypes = [vp]
    L.nl_stack_destroy.restype = None
    L.nl_stack_upload_frame.argtypes = [vp, C.c_int, _f32p]
    L.nl_stack_upload_tile.argtypes = [vp, C.c_int, _f32p]
    L.nl_stack_download_tile.argtypes = [vp, C.c_int, _f32p]
    L.nl_stack_download_rows.argtypes = [vp, C.c_int, C.c_int, C.c_int, _f32p]
    L.nl_stack_frames_device_ptr.argtypes = [vp]
    L.nl_stack_frames_device_ptr.restype = vp
    L.nl_stack_device_bytes.argtypes = [vp]
    L.nl_stack_device_bytes.restype = C.c_int64
    L.nl_fits_parse_header.argtypes = [vp, C.c_int64, C.c_int, C.POINTER(FitsHeader)]
    L.nl_fits_write_header.argtypes = [vp, C.c_int64, C.c_int, C.POINTER(C.c_int32), C.c_float, C.c_float, C.c_float]
    L.nl_fits_write_header.restype = C.c_int64
    L.nl_fits_padded_bytes.argtypes = [C.c_int64]
    L.nl_fits_padded_bytes.restype = C.c_int64
    L.nl_stack_attach_device_frames.argtypes = [vp, vp]
    L.nl_stack_attach_device_frames_strided.argtypes = [vp, vp, C.c_int64]
    L.nl_stack_frame_stride.argtypes = [vp]
    L.nl_stack_frame_stride.restype = C.c_int64
    L.nl_stack_fill_synthetic.argtypes = [vp, C.c_uint64]
    L.nl_stack_set_weights.argtypes = [vp, _f32p]
    L.nl_stack_set_active_frames.argtypes = [vp, C.c_int]
    L.nl_group_set_active_frames.argtypes = [vp, C.c_int]
    L.nl_weights_from_scalars.argtypes = [C.c_int, _f32p, C.c_int, _f32p, _intp]
    L.nl_stack_run.argtypes = [vp, C.c_int, C.c_float, C.c_float, C.c_float, _f32p, _i64p, _i64p]
    L.nl_stack_run_async.argtypes = [vp, C.c_int, C.c_float, C.c_float, C.c_float]
    L.nl_stack_finish.argtypes = [vp, _f32p, _i64p, _i64p]
    L.nl_stack_result_device_ptr.argtypes = [vp]
    L.nl_stack_result_device_ptr.restype = vp
    L.nl_stack_last_mode.argtypes = [vp]
    L.nl_stack_last_kernel_ms.argtypes = [vp]
    L.nl_stack_last_kernel_ms.restype = C.c_float
    L.nl_stack_last_dominant_kernel_ms.argtypes = [vp]
    L.nl_stack_last_dominant_kernel_ms.restype = C.c_float
    L.nl_stack_last_kernel_name.argtypes = [vp]
    L.nl_stack_last_kernel_name.restype = C.c_char_p
    L.nl_stack_set_exact.argtypes = [vp, C.c_int]
    L.nl_stack_set_dev_flags.argtypes = [vp, C.c_uint]
    L.nl_stack_pass_times.argtypes = [vp, C.c_int, _f32p, _f32p]
    L.nl_stack_stream.argtypes = [vp]
    L.nl_stack_stream.restype = vp
    L.nl_stack_counters_device_ptr.argtypes = [vp]
    L.nl_stack_counters_device_ptr.restype = vp
    L.nl_stack_copy_counters_async.argtypes = [vp, vp]
    L.nl_stack_set_counters_buffer.argtypes = [vp, vp]
    L.nl_stack_order_stream_after.argtypes = [vp, vp]
    L.nl_stack_set_counters_buffer.restype = C.c_int
    L.nl_group_tile_rows.argtypes = [C.c_int, C.c_int, C.c_int, _intp, _intp]
    L.nl_group_tile_rows.restype = None
    L.nl_group_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _intp]
    L.nl_group_create.restype = vp
    L.nl_group_destroy.argtypes = [vp]
    L.nl_group_destroy.restype = None
    L.nl_group_size.argtypes = [vp]
    L.nl_group_tile.argtypes = [vp, C.c_int]
    L.nl_group_tile.restype = vp
    L.nl_group_upload_frame.argtypes = [vp, C.c_int, _f32p]
    L.nl_group_fill_synthetic.argtypes = [vp, C.c_uint64]
    L.nl_group_set_weights.argtypes = [vp, _f32p]
    L.nl_group_set_exact.argtypes = [vp, C.c_int]
    L.nl_group_run.argtypes = [vp, C.c_int, C.c_float, C.c_float, C.c_float, _f32p, _i64p, _i64p]
    L.nl_group_last_mode.argtypes = [vp]
    _u16p = C.POINTER(C.c_uint16)
    _maps_args = [vp, C.c_int, C.c_float, C.c_float, C.c_float, _f32p, _i64p, _i64p, _u16p, _u16p]
    for suffix in ("", "_fast", "_resident", "_deep", "_full", "_deepstack"):
        getattr(L, "nl_stack_run_maps" + suffix).argtypes = _maps_args
        getattr(L, "nl_group_run_maps" + suffix).argtypes = _maps_args
    _wlinfit_args = [vp, C.c_float, C.c_float, C.c_float, _f32p, _i64p, _i64p]
    L.nl_stack_run_linfit_weighted.argtypes = _wlinfit_args
    L.nl_group_run_linfit_weighted.argtypes = _wlinfit_args
    L.nl_stack_run_linfit_weighted_async.argtypes = [vp, C.c_float, C.c_float, C.c_float]
    _wclip_args = [vp, C.c_int, C.c_float, C.c_float, C.c_float, _f32p, _i64p, _i64p]
    L.nl_stack_run_clip_weighted.argtypes = _wclip_args
    L.nl_group_run_clip_weighted.argtypes = _wclip_args
    L.nl_stack_run_clip_weighted_async.argtypes = [vp, C.c_int, C.c_float, C.c_float, C.c_float]
    L.nl_stack_run_mad_weighted.argtypes = _wlinfit_args
    L.nl_group_run_mad_weighted.argtypes = _wlinfit_args
    L.nl_stack_run_mad_weighted_async.argtypes = [vp, C.c_float, C.c_float, C.c_float]
    L.nl_stack_run_deepstack.argtypes = _wclip_args
    L.nl_group_run_deepstack.argtypes = _wclip_args
    L.nl_stack_run_deepstack_async.argtypes = [vp, C.c_int, C.c_float, C.c_float, C.c_float]
    L.nl_stack_run_mad_weighted_deepstack.argtypes = _wlinfit_args
    L.nl_group_run_mad_weighted_deepstack.argtypes = _wlinfit_args
    L.nl_stack_run_mad_weighted_deepstack_async.argtypes = [vp, C.c_float, C.c_float, C.c_float]
    L.nl_stack_coverage.argtypes = [vp, _u16p]
    L.nl_group_coverage.argtypes = [vp, _u16p]
    L.nl_stack_last_coverage_ms.argtypes = [vp]
    L.nl_stack_last_coverage_ms.restype = C.c_float
    L.nl_group_find_sigmas.argtypes = [vp, C.c_int, C.c_float, C.c_float, C.c_float, _f32p, _i64p, _i64p,
                                       _f32p, _f32p, _intp]
    L.nl_group_accumulate.argtypes = [vp, C.c_float, C.c_int]
    L.nl_group_accumulate_finalize.argtypes = [vp, C.c_float, _f32p]
    L.nl_stack_last_fallback_pixels.argtypes = [vp]
    L.nl_stack_last_fallback_pixels.restype = C.c_int64
    L.nl_stack_last_generic_pixels.argtypes = [vp]
    L.nl_stack_last_pass_protocol.argtypes = [vp]
    L.nl_stack_last_generic_pixels.restype = C.c_int64
    L.nl_stack_linfit_stage_counts.argtypes = [vp, C.POINTER(C.c_uint), C.c_int]
    L.nl_stack_linfit_stage_counts.restype = C.c_int
    L.nl_stack_find_sigmas.argtypes = [vp, C.c_int, C.c_float, C.c_float, C.c_float, REDUCE_FN,
                                       vp, _f32p, _i64p, _i64p, _f32p, _f32p, _intp]
    L.nl_stack_accumulate.argtypes = [vp, C.c_float, C.c_int]
    L.nl_stack_accumulate_finalize.argtypes = [vp, C.c_float, _f32p]
    L.nl_stack_frame_stats.argtypes = [vp, C.c_int, _f32p, _f32p, _f32p, C.POINTER(C.c_double)]
    L.nl_stack_frame_noise.argtypes = [vp, C.c_int, _f32p]
    _u32p = C.POINTER(C.c_uint32)
    _locscale_args = [C.c_int, C.c_int, _u32p, C.c_int, _f32p, _f32p, _f32p, C.POINTER(LocScale)]
    L.nl_stack_frame_location_scale.argtypes = [vp, C.c_int] + _locscale_args
    L.nl_location_scale.argtypes = [_f32p, C.c_int, C.c_int] + _locscale_args + [C.c_int]
    L.nl_locscale_seeds.argtypes = [C.c_uint64, _u32p, C.c_int]
    _i32p = C.POINTER(C.c_int32)
    L.nl_aligner_create.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int]
    L.nl_aligner_create.restype = vp
    L.nl_aligner_destroy.argtypes = [vp]
    L.nl_aligner_destroy.restype = None
    L.nl_aligner_info.argtypes = [vp, _i32p, C.c_int, _intp, _intp, vp, C.c_int]
    L.nl_aligner_match.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, _intp, _i32p, C.POINTER(AlignInfo)]
    L.nl_aligner_match_stars.argtypes = [vp, _f32p, C.c_int, vp, C.c_int, _i32p, _i32p]
    L.nl_stack_weights_from_noise.argtypes = [vp, _f32p]
    L.nl_median_filter_3x3.argtypes = [_f32p, _f32p, C.c_int, C.c_int, C.c_int]
    L.nl_median_filter_mask.argtypes = [_f32p, _f32p, C.c_int64, C.POINTER(C.c_int32), C.c_int, C.c_int]
    L.nl_stack_upload_frame_async.argtypes = [vp, C.c_int, _f32p]
    L.nl_stack_upload_wait.argtypes = [vp]
    L.nl_stack_upload_frame_fits.argtypes = [vp, C.c_int, vp, C.c_int, C.c_float, C.c_float, C.c_float,
                                             C.c_float, _f32p]
    L.nl_stack_upload_frame_fits_async.argtypes = [vp, C.c_int, vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float]
    L.nl_group_upload_frame_fits.argtypes = [vp, C.c_int, vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float]
    L.nl_stack_upload_frame_projected_async.argtypes = [vp, C.c_int, _f32p, C.c_int, C.c_int, _f32p, C.c_float,
                                                          C.c_float, C.c_float]
    L.nl_group_upload_frame_projected.argtypes = [vp, C.c_int, _f32p, C.c_int, C.c_int, _f32p, C.c_float,
                                                   C.c_float, C.c_float]
    L.nl_stack_upload_frame_projected.argtypes = [vp, C.c_int, _f32p, C.c_int, C.c_int, _f32p, C.c_float,
                                                  C.c_float, C.c_float]
    L.nl_stack_frame_affine.argtypes = [vp, C.c_int, C.c_float, C.c_float]
    L.nl_stack_download_result_fits.argtypes = [vp, vp]
    L.nl_fits_decode.argtypes = [vp, C.c_int, C.c_int64, C.c_float, C.c_float, _f32p, _f32p, C.c_int]
    L.nl_project_bilinear.argtypes = [_f32p, C.c_int, C.c_int, _f32p, C.c_int, C.c_int, _f32p, C.c_float,
                                      C.c_int]
    L.nl_host_op_stack_apply_json.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int,
                                              C.POINTER(_f32p), _f32p, _f32p, C.c_int, C.c_int,
                                              _f32p, _f32p, C.c_char_p, C.c_int, C.c_char_p, C.c_int]
    L.nl_host_op_stack_batches_apply_json.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(_f32p),
                                                      _f32p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, _f32p,
                                                      _intp, C.c_char_p, C.c_int, C.c_char_p, C.c_int]
    L.nl_host_set_devices.argtypes = [_intp, C.c_int]
    L.nl_host_op_stack_roundtrip_json.argtypes = [C.c_char_p]
    L.nl_host_op_stack_roundtrip_json.restype = C.c_char_p
    L.nl_calib_create.argtypes = [C.c_int, _f32p, C.c_int, C.c_int, _f32p, C.c_int, C.c_int]
    L.nl_calib_create.restype = vp
    L.nl_calib_destroy.argtypes = [vp]
    L.nl_calib_destroy.restype = None
    L.nl_calib_flat_max.argtypes = [vp, _f32p]
    L.nl_preprocess_frame.argtypes = [vp, C.c_int, _f32p, _f32p, C.c_int, C.c_int, C.c_float, C.c_float, _i64p,
                                      _f32p, C.c_int]
    L.nl_stack_frame_calibrate.argtypes = [vp, C.c_int, vp]
    L.nl_stack_frame_badpixel.argtypes = [vp, C.c_int, C.c_float, C.c_float, _i64p, _f32p]
    L.nl_debayer_shape.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_char_p, _intp, _intp]
    L.nl_preprocess_frame_cfa.argtypes = [vp, C.c_int, _f32p, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_float,
                                          C.c_float, _f32p, _intp, _intp, _i64p, _f32p, C.c_int]
    L.nl_stack_upload_frame_cfa.argtypes = [vp, C.c_int, _f32p, C.c_int, C.c_int, vp, C.c_char_p, C.c_char_p,
                                            C.c_float, C.c_float, _i64p, _f32p]
    _star_args = [C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_float, vp, C.c_int, _intp,
                  _f32p, _f32p]
    L.nl_find_stars.argtypes = [_f32p, C.c_int, C.c_int] + _star_args + [C.c_int]
    L.nl_stack_frame_find_stars.argtypes = [vp, C.c_int] + _star_args
    L.nl_stack_result_find_stars.argtypes = [vp] + _star_args
    _back_args = [C.c_int, C.c_float, C.c_float, C.c_int, vp, C.c_int, _f32p, _f32p, C.c_int, C.POINTER(Background)]
    L.nl_back_extract.argtypes = [_f32p, C.c_int, C.c_int] + _back_args + [C.c_int]
    L.nl_stack_frame_back_extract.argtypes = [vp, C.c_int] + _back_args
    _deband_args = [C.c_float, C.c_int, C.c_float, C.c_float, C.c_float, C.POINTER(Deband)]
    for name in ("nl_deband_horiz", "nl_deband_vert"):
        getattr(L, name).argtypes = [_f32p, C.c_int, C.c_int] + _deband_args + [C.c_int]
    for name in ("nl_stack_frame_deband_horiz", "nl_stack_frame_deband_vert"):
        getattr(L, name).argtypes = [vp, C.c_int] + _deband_args
    L.nl_bin_shape.argtypes = [C.c_int, C.c_int, C.c_int, _intp, _intp]
    L.nl_bin_nxn.argtypes = [_f32p, C.c_int, C.c_int, C.c_int, _f32p, C.c_int]
    L.nl_stack_frame_bin_from.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int]
    _usm_args = [C.c_float] * 5                          # sigma, gain, min, max, abs_threshold
    L.nl_gaussian_kernel_1d.argtypes = [C.c_float, _f32p, C.c_int, _intp]
    L.nl_convolve_separable.argtypes = [_f32p, C.c_int, C.c_int, _f32p, C.c_int, C.c_int]
    L.nl_gaussian_blur.argtypes = [_f32p, C.c_int, C.c_int, C.c_float, C.c_int]
    L.nl_unsharp_mask.argtypes = [_f32p, _f32p, C.c_int, C.c_int] + _usm_args + [C.c_int]
    L.nl_stack_frame_gaussian_blur.argtypes = [vp, C.c_int, C.c_float]
    L.nl_stack_frame_unsharp_mask.argtypes = [vp, C.c_int] + _usm_args
    L.nl_stack_result_gaussian_blur.argtypes = [vp, C.c_float]
    L.nl_stack_result_unsharp_mask.argtypes = [vp] + _usm_args
    L.nl_blur_tap_paths.argtypes = [C.c_int, _intp, _intp]
    _tone_args = [C.POINTER(Tone), _f32p, _f32p, _f32p]      # the curve, mn, mean, mx
    _gray_args = [C.c_float, C.c_float, C.c_float, C.c_int, vp]     # min, max, gamma, bits, out_host
    L.nl_stack_frame_tone.argtypes = [vp, C.c_int] + _tone_args
    L.nl_stack_result_tone.argtypes = [vp] + _tone_args
    L.nl_tone.argtypes = [_f32p, C.c_int64] + _tone_args + [C.c_int]
    L.nl_stack_frame_export_gray.argtypes = [vp, C.c_int] + _gray_args
    L.nl_stack_result_export_gray.argtypes = [vp] + _gray_args
    L.nl_export_gray.argtypes = [_f32p, C.c_int64] + _gray_args + [C.c_int]
    L.nl_stack_frame_project_from.argtypes = [vp, C.c_int, vp, C.c_int, _f32p, C.c_float]
    L.nl_group_frame_project_from.argtypes = [vp, C.c_int, vp, C.c_int, _f32p, C.c_float]
    L.nl_stack_project_tile_paths.argtypes = [vp, vp, C.c_int, _f32p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.nl_resample_lanczos3_table.argtypes = [_f32p]
    L.nl_stack_frame_resample_from.argtypes = [vp, C.c_int, vp, C.c_int, _f32p, C.c_float, C.c_int, C.c_int]
    L.nl_group_frame_resample_from.argtypes = [vp, C.c_int, vp, C.c_int, _f32p, C.c_float, C.c_int, C.c_int]
    L.nl_stack_resample_tile_paths.argtypes = [vp, vp, C.c_int, _f32p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.nl_drizzle_geometry.argtypes = [_f32p, C.c_float, C.c_float, _f32p, _f32p, _f32p, _intp]
    L.nl_stack_frame_drizzle_from.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, _f32p, C.c_float, C.c_float, C.c_float,
                                              C.c_int, C.c_int]
    L.nl_stack_drizzle_finalize.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float]
    L.nl_stack_frame_reject_against.argtypes = [vp, C.c_int, C.c_int, C.c_float, C.c_float, _i64p, _i64p]
    L.nl_stack_drizzle_tile_paths.argtypes = [vp, vp, C.c_int, _f32p, C.c_float, C.c_float, _i64p, _i64p]
    L.nl_drizzle_cfa_transform.argtypes = [_f32p, C.c_char_p, _f32p]
    L.nl_stack_frame_drizzle_cfa_from.argtypes = L.nl_stack_frame_drizzle_from.argtypes + [C.c_char_p, C.c_char_p]
    L.nl_drizzle_square_geometry.argtypes = [_f32p, C.c_float, C.c_float, _f32p, _f32p, _f32p, _f32p, _intp]
    L.nl_stack_frame_drizzle_square_from.argtypes = L.nl_stack_frame_drizzle_from.argtypes[:-1]
    L.nl_stack_frame_drizzle_square_cfa_from.argtypes = L.nl_stack_frame_drizzle_square_from.argtypes + [C.c_char_p, C.c_char_p]
    L.nl_stack_drizzle_square_tile_paths.argtypes = L.nl_stack_drizzle_tile_paths.argtypes
    L.nl_stack_frame_reject_against_cfa.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_float, C.c_float,
                                                    _i64p, _i64p]
    L.nl_stack_frame_badpixel_cfa.argtypes = [vp, C.c_int, C.c_char_p, C.c_char_p, C.c_float, C.c_float, _i64p, _f32p]
    _planes = C.POINTER(C.c_int)
    # stars, n_stars, block, border, skip_bright, skip_dim, shadows, highlights, loc, scale, report
    _balance_args = [vp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, Rgb, Rgb, _f32p, _f32p, C.POINTER(RgbBalance)]
    L.nl_rgb_normalization.argtypes = [_f32p, _f32p, _f32p, _f32p]
    L.nl_stack_frame_combine_from.argtypes = [vp, C.c_int, vp, C.c_int, C.c_float, C.c_float]
    L.nl_stack_rgb_scale_offset_clamp.argtypes = [vp, _planes, _f32p, _f32p, _f32p]
    L.nl_stack_rgb_darkest_block.argtypes = [vp, _planes, C.c_int, C.c_float, C.POINTER(Rgb)]
    L.nl_stack_rgb_mean_star_intensity.argtypes = [vp, _planes, vp, C.c_int, C.c_float, C.c_float, Rgb, C.POINTER(Rgb)]
    L.nl_rgb_balance_coeffs.argtypes = [Rgb, Rgb, Rgb, Rgb, _f32p, _f32p]
    L.nl_stack_rgb_balance.argtypes = [vp, _planes] + _balance_args
    L.nl_rgb_balance.argtypes = [_f32p, C.c_int, C.c_int] + _balance_args + [C.c_int]
    L.nl_stack_rgb_chroma.argtypes = [vp, _planes, C.POINTER(Chroma)]
    L.nl_stack_rgb_export.argtypes = [vp, _planes] + _gray_args
    L.nl_export_rgb.argtypes = [_f32p, C.c_int64] + _gray_args + [C.c_int]
    return L


def last_error():
    return load().nl_last_error().decode("utf-8", "replace")


def check(rc):
    if rc != OK:
        raise NlError(rc, last_error())
    return rc


def fptr(a):
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(_f32p)


def device_count():
    n = load().nl_device_count()
    return n if n > 0 else 0
