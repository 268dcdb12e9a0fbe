"""nightlight_amd -- MI355X (gfx950) implementation of Nightlight's per-pixel
stacking hot path behind the C ABI in include/nlstack.h.

The product is libnlstack.so (hand-written HIP kernels + C ABI, csrc/); the
Python modules here are plumbing for tests, bench.py and multi-GPU sharding.
"""
from . import capi  # noqa: F401
from .capi import (CHROMA_FOR_HUES, CHROMA_GAMMA, CHROMA_NEUTRALIZE, DZ_MAX_RADIUS, DZ_POINT, DZ_TURBO, LOCSCALE_MAX_SEEDS, LOCSCALE_SAMPLES, LSE_HISTOGRAM, LSE_IKSS,
                   LSE_MEAN_STDDEV, LSE_MEDIAN_MAD, LSE_SC_MEDIAN_QN, NlError, ROTATE_HUES, RS_BICUBIC, RS_BILINEAR, RS_LANCZOS3, RS_PHASES, ST_AUTO, ST_LINEAR_FIT, ST_MAD_SIGMA, ST_MEAN, ST_MEDIAN,  # noqa: F401
                   ST_SIGMA, ST_WINSOR_SIGMA, TONE_GAMMA, TONE_MIDTONES, TONE_NORMALIZE, TONE_PARTIAL_GAMMA,
                   TONE_SCALE_OFFSET, TONE_SHIFT_BLACK, WEIGHT_EXPOSURE, WEIGHT_INVERSE_HFR,
                   WEIGHT_INVERSE_NOISE, WEIGHT_NONE, device_count)
from .stack import (Aligner, Calibration, StackGroup, StackHandle, back_extract, bin_nxn, bin_shape, blur_tap_paths,  # noqa: F401
                    convolve_separable, debayer_shape, drizzle_cfa_transform, drizzle_geometry, drizzle_square_geometry, deband_horiz, deband_vert, export_gray, export_rgb, find_stars, fits_padded_bytes,
                    fits_parse_header, fits_write_header, gaussian_blur, gaussian_kernel_1d, lanczos3_table, location_scale, locscale_seeds,
                    median_filter_3x3,
                    median_filter_mask, preprocess_frame, preprocess_frame_cfa, rgb_balance, rgb_balance_coeffs,
                    rgb_normalization, tone, unsharp_mask, weights_from_scalars)

__version__ = "0.2.0"
