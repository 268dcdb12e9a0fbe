"""Return codes and nl_last_error() strings of the frame-step entries on real handles: the argument checks that a
missing device hides from tests/test_frame_entry_errors.py (indices, "has not run a pass", whole-image steps on a row
tile, plane triples, shapes of a second handle), then one happy path per shared helper.

A characterisation table: EXPECTED was recorded on an MI355X from the library as it was before the entries were split
over four units and must not be regenerated from the code under test (two rows, marked below, pin the one order of
two faults that the split changed).  No row gets past its argument checks."""
import ctypes as C

import numpy as np
import pytest

from nightlight_amd import capi

pytestmark = pytest.mark.gpu

W, H = 8, 6
f = capi.fptr
RAW = np.zeros(8 * W * H, np.uint8)
raw = RAW.ctypes.data_as(C.c_void_p)
OUT = np.zeros(3 * W * H, np.float32)
FRAME = np.arange(W * H, dtype=np.float32)
V3 = np.array([0.0, 0.5, 1.0], np.float32)
T6 = np.array([1, 0, 0, 0, 1, 0], np.float32)
T6_SINGULAR = np.zeros(6, np.float32)
STARS = np.zeros(2, capi.STAR_DTYPE)
STARS["x"], STARS["y"], STARS["hfr"] = 3.0, 3.0, 1.0
BAD_STARS = STARS.copy()
BAD_STARS["hfr"][1] = -1.0
stars = STARS.ctypes.data_as(C.c_void_p)
bad_stars = BAD_STARS.ctypes.data_as(C.c_void_p)
ZERO, ONE = capi.Rgb(0, 0, 0), capi.Rgb(1, 1, 1)

STAR_ARGS = (0.0, 1.0, 15.0, 5.0, 1.4, 2, 0.0)                   # location ... diff_std
BACK_ARGS = (2, 4.0, 1.5, 0)                                      # grid_size, hfr_factor, sigma, clip
DEBAND_ARGS = (50.0, 2, 3.0, 0.0, 1.0)                            # percentile, window, sigma, location, scale
USM_ARGS = (1.0, 0.5, 0.0, 1.0, 0.0)                              # sigma, gain, min, max, abs_threshold


def _i():
    return C.byref(C.c_int(0))


def _i64():
    return C.byref(C.c_int64(0))


def _fl():
    return C.byref(C.c_float(0))


def planes(a, b, c):
    return (C.c_int * 3)(a, b, c)


P012 = planes(0, 1, 2)


def tone_of(kind, *p):
    return C.byref(capi.Tone(kind, (C.c_float * 3)(*p)))


def chroma_of(kind, *p):
    return C.byref(capi.Chroma(kind, (C.c_float * 4)(*p)))


SCALE = (capi.TONE_SCALE_OFFSET, 2.0, 1.0)


def balance(L, h, pl, st, n, block, border):
    return L.nl_stack_rgb_balance(h, pl, st, n, block, border, 0.0, 0.0, ZERO, ONE, f(V3), f(V3), None)


def find_stars(L, h, idx, capacity=2, radius=2):
    return L.nl_stack_frame_find_stars(h, idx, 0.0, 1.0, 15.0, 5.0, 1.4, radius, 0.0, stars, capacity, _i(), None, None)


def back_extract(L, h, idx, n_stars=2, capacity=4):
    return L.nl_stack_frame_back_extract(h, idx, *BACK_ARGS, stars, n_stars, None, f(OUT), capacity, None)


def upload_cfa(L, h, idx, w=W, hh=H, channel=b"R", cfa=b"RGGB", calib=None):
    return L.nl_stack_upload_frame_cfa(h, idx, f(FRAME), w, hh, calib, channel, cfa, 3.0, 5.0, _i64(), None)


class Ctx:
    """A: 3 frames 8x6, whole image, no pass run.  T: 3 frames 8x6, rows [2, 4).  B: 1 frame 4x3, what binning by 2
    gives A's shape.  CAL: dark and flat masters of A's shape."""

    def __init__(self, L):
        self.L = L
        self.A = L.nl_stack_create(3, W, H, 0, H, 0)
        self.T = L.nl_stack_create(3, W, H, 2, 2, 0)
        self.B = L.nl_stack_create(1, W // 2, H // 2, 0, H // 2, 0)
        self.CAL = L.nl_calib_create(0, f(FRAME), W, H, f(FRAME), W, H)
        assert self.A and self.T and self.B and self.CAL, L.nl_last_error()

    def close(self):
        self.L.nl_calib_destroy(self.CAL)
        for h in (self.A, self.T, self.B):
            self.L.nl_stack_destroy(h)


def _per_index(name, call):
    """idx = 3 and idx = -1 of a frame_* entry on A"""
    return [("%s/idx-3" % name, lambda L, c: call(L, c.A, 3)), ("%s/idx--1" % name, lambda L, c: call(L, c.A, -1))]


def _per_planes(name, call):
    return [("%s/planes-0-1-3" % name, lambda L, c: call(L, c.A, planes(0, 1, 3))),
            ("%s/planes--1-1-2" % name, lambda L, c: call(L, c.A, planes(-1, 1, 2))),
            ("%s/planes-0-0-1" % name, lambda L, c: call(L, c.A, planes(0, 0, 1))),
            ("%s/null-planes" % name, lambda L, c: call(L, c.A, None))]


# (row id, call(L, ctx) -> return code)
ROWS = (
    # ---- idx = 3 and idx = -1 on every frame_* entry ----
    _per_index("frame_stats", lambda L, h, i: L.nl_stack_frame_stats(h, i, _fl(), _fl(), _fl(), None))
    + _per_index("frame_noise", lambda L, h, i: L.nl_stack_frame_noise(h, i, _fl()))
    + _per_index("frame_affine", lambda L, h, i: L.nl_stack_frame_affine(h, i, 1.0, 0.0))
    + _per_index("frame_calibrate-null-calib", lambda L, h, i: L.nl_stack_frame_calibrate(h, i, None))
    + _per_index("frame_badpixel", lambda L, h, i: L.nl_stack_frame_badpixel(h, i, 3.0, 5.0, _i64(), None))
    + _per_index("frame_find_stars", lambda L, h, i: find_stars(L, h, i))
    + _per_index("frame_back_extract", lambda L, h, i: back_extract(L, h, i))
    + _per_index("frame_deband_horiz", lambda L, h, i: L.nl_stack_frame_deband_horiz(h, i, *DEBAND_ARGS, None))
    + _per_index("frame_deband_vert", lambda L, h, i: L.nl_stack_frame_deband_vert(h, i, *DEBAND_ARGS, None))
    + _per_index("frame_gaussian_blur", lambda L, h, i: L.nl_stack_frame_gaussian_blur(h, i, 1.0))
    + _per_index("frame_gaussian_blur-sigma-0", lambda L, h, i: L.nl_stack_frame_gaussian_blur(h, i, 0.0))
    + _per_index("frame_unsharp_mask", lambda L, h, i: L.nl_stack_frame_unsharp_mask(h, i, *USM_ARGS))
    + _per_index("frame_tone", lambda L, h, i: L.nl_stack_frame_tone(h, i, tone_of(*SCALE), None, None, None))
    + _per_index("frame_export_gray", lambda L, h, i: L.nl_stack_frame_export_gray(h, i, 0.0, 1.0, 1.0, 16, raw))
    + _per_index("upload_frame_cfa", lambda L, h, i: upload_cfa(L, h, i))
    + _per_index("project_tile_paths", lambda L, h, i: L.nl_stack_project_tile_paths(h, h, i, f(T6), _i64(), _i64()))
    + [
        # (the call's own arguments come before the slot's range)
        ("frame_tone-unknown-kind/idx-3", lambda L, c: L.nl_stack_frame_tone(c.A, 3, tone_of(99), None, None, None)),
        ("frame_export_gray-bits-12/idx-3", lambda L, c: L.nl_stack_frame_export_gray(c.A, 3, 0.0, 1.0, 1.0, 12, raw)),
        # The one pair of faults whose order changed when the entries were split: before, idx < 0 was reported first
        # ("frame_tone: bad index -1", "frame_export_gray: bad index -1").  These two rows are not from the recording.
        ("frame_tone-unknown-kind/idx--1", lambda L, c: L.nl_stack_frame_tone(c.A, -1, tone_of(99), None, None, None)),
        ("frame_export_gray-bits-12/idx--1", lambda L, c: L.nl_stack_frame_export_gray(c.A, -1, 0.0, 1.0, 1.0, 12, raw)),
        ("frame_bin_from/src-idx-3", lambda L, c: L.nl_stack_frame_bin_from(c.B, 0, c.A, 3, 2)),
        ("frame_bin_from/src-idx--1", lambda L, c: L.nl_stack_frame_bin_from(c.B, 0, c.A, -1, 2)),
        ("frame_bin_from/dst-idx-1", lambda L, c: L.nl_stack_frame_bin_from(c.B, 1, c.A, 0, 2)),
        ("frame_bin_from/dst-idx--1", lambda L, c: L.nl_stack_frame_bin_from(c.B, -1, c.A, 0, 2)),
        ("frame_bin_from/src+dst-idx", lambda L, c: L.nl_stack_frame_bin_from(c.B, 1, c.A, 3, 2)),
        ("frame_combine_from/src-idx-3", lambda L, c: L.nl_stack_frame_combine_from(c.A, 0, c.A, 3, 0.0, 1.0)),
        ("frame_combine_from/src-idx--2", lambda L, c: L.nl_stack_frame_combine_from(c.A, 0, c.A, -2, 0.0, 1.0)),
        ("frame_combine_from/src-result-no-pass", lambda L, c: L.nl_stack_frame_combine_from(c.A, 0, c.A, -1, 0.0, 1.0)),
        ("frame_combine_from/dst-idx-3", lambda L, c: L.nl_stack_frame_combine_from(c.A, 3, c.A, 0, 0.0, 1.0)),
        ("frame_combine_from/dst-idx--1", lambda L, c: L.nl_stack_frame_combine_from(c.A, -1, c.A, 0, 0.0, 1.0)),
        ("frame_combine_from/src+dst-idx", lambda L, c: L.nl_stack_frame_combine_from(c.A, 3, c.A, 3, 0.0, 1.0)),
        ("frame_combine_from/null-src", lambda L, c: L.nl_stack_frame_combine_from(c.A, 0, None, 0, 0.0, 1.0)),
        ("frame_project_from/src-idx-3", lambda L, c: L.nl_stack_frame_project_from(c.T, 0, c.A, 3, f(T6), 0.0)),
        ("frame_project_from/src-idx--1", lambda L, c: L.nl_stack_frame_project_from(c.T, 0, c.A, -1, f(T6), 0.0)),
        ("frame_project_from/dst-idx-3", lambda L, c: L.nl_stack_frame_project_from(c.T, 3, c.A, 0, f(T6), 0.0)),
        ("frame_project_from/dst-idx--1", lambda L, c: L.nl_stack_frame_project_from(c.T, -1, c.A, 0, f(T6), 0.0)),
        ("frame_project_from/null-transform", lambda L, c: L.nl_stack_frame_project_from(c.T, 0, c.A, 0, None, 0.0)),
        ("frame_project_from/null-src", lambda L, c: L.nl_stack_frame_project_from(c.T, 0, None, 0, f(T6), 0.0)),
        # ---- every result_* entry before a pass ----
        ("result_find_stars/no-pass",
         lambda L, c: L.nl_stack_result_find_stars(c.A, *STAR_ARGS, stars, 2, _i(), None, None)),
        ("result_gaussian_blur/no-pass", lambda L, c: L.nl_stack_result_gaussian_blur(c.A, 1.0)),
        ("result_unsharp_mask/no-pass", lambda L, c: L.nl_stack_result_unsharp_mask(c.A, *USM_ARGS)),
        ("result_tone/no-pass", lambda L, c: L.nl_stack_result_tone(c.A, tone_of(*SCALE), None, None, None)),
        ("result_tone/no-pass+null-curve", lambda L, c: L.nl_stack_result_tone(c.A, None, None, None, None)),
        ("result_export_gray/no-pass", lambda L, c: L.nl_stack_result_export_gray(c.A, 0.0, 1.0, 1.0, 16, raw)),
        ("result_export_gray/no-pass+gamma-0", lambda L, c: L.nl_stack_result_export_gray(c.A, 0.0, 1.0, 0.0, 16, raw)),
        # ---- every whole-image step on the row tile ----
        ("frame_noise/tile", lambda L, c: L.nl_stack_frame_noise(c.T, 0, _fl())),
        ("frame_noise/tile+idx-3", lambda L, c: L.nl_stack_frame_noise(c.T, 3, _fl())),
        ("frame_noise/null-output", lambda L, c: L.nl_stack_frame_noise(c.A, 0, None)),
        ("weights_from_noise/tile", lambda L, c: L.nl_stack_weights_from_noise(c.T, None)),
        ("frame_badpixel/tile", lambda L, c: L.nl_stack_frame_badpixel(c.T, 0, 3.0, 5.0, _i64(), None)),
        ("frame_badpixel/negative-sigma", lambda L, c: L.nl_stack_frame_badpixel(c.A, 0, -3.0, 5.0, _i64(), None)),
        ("frame_badpixel/tile+negative-sigma", lambda L, c: L.nl_stack_frame_badpixel(c.T, 0, -3.0, 5.0, _i64(), None)),
        ("frame_find_stars/tile", lambda L, c: find_stars(L, c.T, 0)),
        ("frame_find_stars/capacity--1", lambda L, c: find_stars(L, c.A, 0, capacity=-1)),
        ("frame_find_stars/radius-2000", lambda L, c: find_stars(L, c.A, 0, radius=2000)),
        ("frame_find_stars/tile+capacity--1", lambda L, c: find_stars(L, c.T, 0, capacity=-1)),
        ("frame_back_extract/tile", lambda L, c: back_extract(L, c.T, 0)),
        ("frame_back_extract/n_stars--1", lambda L, c: back_extract(L, c.A, 0, n_stars=-1)),
        ("frame_back_extract/capacity--1", lambda L, c: back_extract(L, c.A, 0, capacity=-1)),
        ("frame_back_extract/n_stars--1+capacity--1", lambda L, c: back_extract(L, c.A, 0, n_stars=-1, capacity=-1)),
        ("frame_deband_horiz/tile", lambda L, c: L.nl_stack_frame_deband_horiz(c.T, 0, *DEBAND_ARGS, None)),
        ("frame_deband_vert/tile", lambda L, c: L.nl_stack_frame_deband_vert(c.T, 0, *DEBAND_ARGS, None)),
        ("frame_gaussian_blur/tile", lambda L, c: L.nl_stack_frame_gaussian_blur(c.T, 0, 1.0)),
        ("frame_gaussian_blur/sigma--1", lambda L, c: L.nl_stack_frame_gaussian_blur(c.A, 0, -1.0)),
        ("frame_gaussian_blur/radius-too-large", lambda L, c: L.nl_stack_frame_gaussian_blur(c.A, 0, 8.0)),
        ("frame_unsharp_mask/tile", lambda L, c: L.nl_stack_frame_unsharp_mask(c.T, 0, *USM_ARGS)),
        ("frame_bin_from/src-tile", lambda L, c: L.nl_stack_frame_bin_from(c.B, 0, c.T, 0, 2)),
        ("frame_bin_from/dst-tile", lambda L, c: L.nl_stack_frame_bin_from(c.T, 0, c.A, 0, 1)),
        ("frame_project_from/src-tile", lambda L, c: L.nl_stack_frame_project_from(c.A, 0, c.T, 0, f(T6), 0.0)),
        ("upload_frame_cfa/tile", lambda L, c: upload_cfa(L, c.T, 0)),
        ("rgb_darkest_block/tile", lambda L, c: L.nl_stack_rgb_darkest_block(c.T, P012, 2, 0.0, C.byref(capi.Rgb()))),
        ("rgb_mean_star_intensity/tile",
         lambda L, c: L.nl_stack_rgb_mean_star_intensity(c.T, P012, stars, 2, 0.0, 0.0, ONE, C.byref(capi.Rgb()))),
        ("rgb_balance/tile", lambda L, c: balance(L, c.T, P012, stars, 2, 2, 0.0)),
    ]
    # ---- the plane triples ----
    + _per_planes("rgb_scale_offset_clamp", lambda L, h, pl: L.nl_stack_rgb_scale_offset_clamp(h, pl, f(V3), f(V3), None))
    + _per_planes("rgb_darkest_block", lambda L, h, pl: L.nl_stack_rgb_darkest_block(h, pl, 2, 0.0, C.byref(capi.Rgb())))
    + _per_planes("rgb_mean_star_intensity",
                  lambda L, h, pl: L.nl_stack_rgb_mean_star_intensity(h, pl, stars, 2, 0.0, 0.0, ONE, C.byref(capi.Rgb())))
    + _per_planes("rgb_balance", lambda L, h, pl: balance(L, h, pl, stars, 2, 2, 0.0))
    + _per_planes("rgb_chroma", lambda L, h, pl: L.nl_stack_rgb_chroma(h, pl, chroma_of(capi.CHROMA_GAMMA, 1.0, 0.0)))
    + _per_planes("rgb_export", lambda L, h, pl: L.nl_stack_rgb_export(h, pl, 0.0, 1.0, 1.0, 16, raw))
    + [
        ("rgb_scale_offset_clamp/null-coefficients",
         lambda L, c: L.nl_stack_rgb_scale_offset_clamp(c.A, P012, None, f(V3), None)),
        ("rgb_scale_offset_clamp/planes-0-1-3+null-coefficients",
         lambda L, c: L.nl_stack_rgb_scale_offset_clamp(c.A, planes(0, 1, 3), None, f(V3), None)),
        ("rgb_chroma/null-operation", lambda L, c: L.nl_stack_rgb_chroma(c.A, P012, None)),
        ("rgb_chroma/unknown-kind", lambda L, c: L.nl_stack_rgb_chroma(c.A, P012, chroma_of(99))),
        ("rgb_export/bits-12", lambda L, c: L.nl_stack_rgb_export(c.A, P012, 0.0, 1.0, 1.0, 12, raw)),
        ("rgb_export/gamma-0", lambda L, c: L.nl_stack_rgb_export(c.A, P012, 0.0, 1.0, 0.0, 16, raw)),
        ("rgb_export/null-output", lambda L, c: L.nl_stack_rgb_export(c.A, P012, 0.0, 1.0, 1.0, 16, None)),
        # ---- the projection ----
        ("frame_project_from/in-place", lambda L, c: L.nl_stack_frame_project_from(c.A, 1, c.A, 1, f(T6), 0.0)),
        ("frame_project_from/singular", lambda L, c: L.nl_stack_frame_project_from(c.A, 0, c.A, 1, f(T6_SINGULAR), 0.0)),
        ("project_tile_paths/singular",
         lambda L, c: L.nl_stack_project_tile_paths(c.A, c.A, 1, f(T6_SINGULAR), _i64(), _i64())),
        # ---- a destination of the wrong shape ----
        ("frame_bin_from/wrong-shape", lambda L, c: L.nl_stack_frame_bin_from(c.A, 0, c.A, 1, 2)),
        ("frame_bin_from/empty", lambda L, c: L.nl_stack_frame_bin_from(c.B, 0, c.A, 0, 16)),
        ("frame_combine_from/wrong-shape", lambda L, c: L.nl_stack_frame_combine_from(c.B, 0, c.A, 0, 0.0, 1.0)),
        ("frame_combine_from/tile-of-other-rows", lambda L, c: L.nl_stack_frame_combine_from(c.T, 0, c.A, 0, 0.0, 1.0)),
        ("upload_frame_cfa/wrong-shape", lambda L, c: upload_cfa(L, c.A, 0, w=4, hh=4)),
        ("frame_calibrate/light-differs-from-dark", lambda L, c: L.nl_stack_frame_calibrate(c.B, 0, c.CAL)),
        # ---- block, border and the stars of the colour balance ----
        ("rgb_darkest_block/block-0", lambda L, c: L.nl_stack_rgb_darkest_block(c.A, P012, 0, 0.0, C.byref(capi.Rgb()))),
        ("rgb_darkest_block/border--1", lambda L, c: L.nl_stack_rgb_darkest_block(c.A, P012, 2, -1.0, C.byref(capi.Rgb()))),
        ("rgb_darkest_block/null-output", lambda L, c: L.nl_stack_rgb_darkest_block(c.A, P012, 2, 0.0, None)),
        ("rgb_balance/block-0", lambda L, c: balance(L, c.A, P012, stars, 2, 0, 0.0)),
        ("rgb_balance/border--1", lambda L, c: balance(L, c.A, P012, stars, 2, 2, -1.0)),
        ("rgb_balance/block-0+hfr--1", lambda L, c: balance(L, c.A, P012, bad_stars, 2, 0, 0.0)),
        ("rgb_balance/hfr--1", lambda L, c: balance(L, c.A, P012, bad_stars, 2, 2, 0.0)),
        ("rgb_balance/n_stars--1", lambda L, c: balance(L, c.A, P012, stars, -1, 2, 0.0)),
        ("rgb_balance/null-location",
         lambda L, c: L.nl_stack_rgb_balance(c.A, P012, stars, 2, 2, 0.0, 0.0, 0.0, ZERO, ONE, None, f(V3), None)),
        ("rgb_mean_star_intensity/hfr--1",
         lambda L, c: L.nl_stack_rgb_mean_star_intensity(c.A, P012, bad_stars, 2, 0.0, 0.0, ONE, C.byref(capi.Rgb()))),
        ("rgb_mean_star_intensity/n_stars--1",
         lambda L, c: L.nl_stack_rgb_mean_star_intensity(c.A, P012, stars, -1, 0.0, 0.0, ONE, C.byref(capi.Rgb()))),
        ("rgb_mean_star_intensity/null-output",
         lambda L, c: L.nl_stack_rgb_mean_star_intensity(c.A, P012, stars, 2, 0.0, 0.0, ONE, None)),
        # ---- the colour-camera front ----
        ("upload_frame_cfa/unknown-cfa", lambda L, c: upload_cfa(L, c.A, 0, cfa=b"XYZW")),
        ("upload_frame_cfa/unknown-channel", lambda L, c: upload_cfa(L, c.A, 0, channel=b"Q")),
        ("upload_frame_cfa/unknown-cfa+channel", lambda L, c: upload_cfa(L, c.A, 0, channel=b"Q", cfa=b"XYZW")),
        ("upload_frame_cfa/no-channel", lambda L, c: upload_cfa(L, c.A, 0, channel=b"")),
        ("upload_frame_cfa/null-handle", lambda L, c: upload_cfa(L, None, 0)),
        # ---- host forms whose checks follow the device ----
        ("find_stars/capacity--1",
         lambda L, c: L.nl_find_stars(f(FRAME), W, H, *STAR_ARGS, stars, -1, _i(), None, None, 0)),
        ("back_extract/n_stars--1",
         lambda L, c: L.nl_back_extract(f(FRAME.copy()), W, H, *BACK_ARGS, stars, -1, None, f(OUT), 4, None, 0)),
        ("back_extract/no-grid+n_stars--1",
         lambda L, c: L.nl_back_extract(f(FRAME.copy()), W, H, 0, 4.0, 1.5, 0, stars, -1, None, f(OUT), 4, None, 0)),
        ("bin_nxn/empty", lambda L, c: L.nl_bin_nxn(f(FRAME), W, H, 16, f(OUT), 0)),
        ("preprocess_frame_cfa/unknown-cfa",
         lambda L, c: L.nl_preprocess_frame_cfa(None, 0, f(FRAME), W, H, b"R", b"XYZW", 3.0, 5.0, f(OUT), _i(), _i(),
                                                _i64(), None, 0)),
        ("preprocess_frame/light-differs-from-dark",
         lambda L, c: L.nl_preprocess_frame(c.CAL, 5, f(FRAME), f(OUT), 4, 3, 3.0, 5.0, _i64(), None, 0)),
        ("rgb_balance-host/block-0",
         lambda L, c: L.nl_rgb_balance(f(OUT.copy()), W, H, stars, 2, 0, 0.0, 0.0, 0.0, ZERO, ONE, f(V3), f(V3), None, 0)),
        ("tone-host/unknown-kind", lambda L, c: L.nl_tone(f(FRAME.copy()), W * H, tone_of(99), None, None, None, 0)),
    ]
)

EXPECTED = {
    "frame_stats/idx-3": (-6, "frame_stats: bad index 3"),
    "frame_stats/idx--1": (-6, "frame_stats: bad index -1"),
    "frame_noise/idx-3": (-6, "frame_noise: bad index 3 or null output"),
    "frame_noise/idx--1": (-6, "frame_noise: bad index -1 or null output"),
    "frame_affine/idx-3": (-6, "frame_affine: bad index 3"),
    "frame_affine/idx--1": (-6, "frame_affine: bad index -1"),
    "frame_calibrate-null-calib/idx-3": (-6, "frame_calibrate: bad index 3 or null calibration"),
    "frame_calibrate-null-calib/idx--1": (-6, "frame_calibrate: bad index -1 or null calibration"),
    "frame_badpixel/idx-3": (-6, "frame_badpixel: bad index 3"),
    "frame_badpixel/idx--1": (-6, "frame_badpixel: bad index -1"),
    "frame_find_stars/idx-3": (-6, "frame_find_stars: bad index 3"),
    "frame_find_stars/idx--1": (-6, "frame_find_stars: bad index -1"),
    "frame_back_extract/idx-3": (-6, "frame_back_extract: bad index 3"),
    "frame_back_extract/idx--1": (-6, "frame_back_extract: bad index -1"),
    "frame_deband_horiz/idx-3": (-6, "frame_deband_horiz: bad index 3"),
    "frame_deband_horiz/idx--1": (-6, "frame_deband_horiz: bad index -1"),
    "frame_deband_vert/idx-3": (-6, "frame_deband_vert: bad index 3"),
    "frame_deband_vert/idx--1": (-6, "frame_deband_vert: bad index -1"),
    "frame_gaussian_blur/idx-3": (-6, "frame_gaussian_blur: bad index 3"),
    "frame_gaussian_blur/idx--1": (-6, "frame_gaussian_blur: bad index -1"),
    "frame_gaussian_blur-sigma-0/idx-3": (-6, "frame_gaussian_blur: bad index 3"),
    "frame_gaussian_blur-sigma-0/idx--1": (-6, "frame_gaussian_blur: bad index -1"),
    "frame_unsharp_mask/idx-3": (-6, "frame_unsharp_mask: bad index 3"),
    "frame_unsharp_mask/idx--1": (-6, "frame_unsharp_mask: bad index -1"),
    "frame_tone/idx-3": (-6, "frame_tone: bad index 3"),
    "frame_tone/idx--1": (-6, "frame_tone: bad index -1"),
    "frame_tone-unknown-kind/idx-3": (-6, "frame_tone: unknown kind 99 (NL_TONE_SCALE_OFFSET ... NL_TONE_SHIFT_BLACK)"),
    "frame_export_gray/idx-3": (-6, "frame_export_gray: bad index 3"),
    "frame_export_gray/idx--1": (-6, "frame_export_gray: bad index -1"),
    "frame_export_gray-bits-12/idx-3": (-6, "frame_export_gray: 12 bits (8: image.Gray, 16: image.Gray16)"),
    "upload_frame_cfa/idx-3": (-6, "upload_frame_cfa: bad index 3, null frame or bad raw size 8x6"),
    "upload_frame_cfa/idx--1": (-6, "upload_frame_cfa: bad index -1, null frame or bad raw size 8x6"),
    "project_tile_paths/idx-3": (-6, "project_tile_paths: bad index 3"),
    "project_tile_paths/idx--1": (-6, "project_tile_paths: bad index -1"),
    "frame_tone-unknown-kind/idx--1": (-6, "frame_tone: unknown kind 99 (NL_TONE_SCALE_OFFSET ... NL_TONE_SHIFT_BLACK)"),
    "frame_export_gray-bits-12/idx--1": (-6, "frame_export_gray: 12 bits (8: image.Gray, 16: image.Gray16)"),
    "frame_bin_from/src-idx-3": (-6, "frame_bin_from (source): bad index 3"),
    "frame_bin_from/src-idx--1": (-6, "frame_bin_from (source): bad index -1"),
    "frame_bin_from/dst-idx-1": (-6, "frame_bin_from (destination): bad index 1"),
    "frame_bin_from/dst-idx--1": (-6, "frame_bin_from (destination): bad index -1"),
    "frame_bin_from/src+dst-idx": (-6, "frame_bin_from (source): bad index 3"),
    "frame_combine_from/src-idx-3": (-6, "frame_combine_from (source): bad index 3"),
    "frame_combine_from/src-idx--2": (-6, "frame_combine_from (source): bad index -2"),
    "frame_combine_from/src-result-no-pass": (-6, "frame_combine_from (source): the handle has not run a pass"),
    "frame_combine_from/dst-idx-3": (-6, "frame_combine_from (destination): bad index 3"),
    "frame_combine_from/dst-idx--1": (-6, "frame_combine_from (destination): bad index -1"),
    "frame_combine_from/src+dst-idx": (-6, "frame_combine_from (source): bad index 3"),
    "frame_combine_from/null-src": (-6, "null handle"),
    "frame_project_from/src-idx-3": (-6, "frame_project_from (source): bad index 3"),
    "frame_project_from/src-idx--1": (-6, "frame_project_from (source): bad index -1"),
    "frame_project_from/dst-idx-3": (-6, "frame_project_from (destination): bad index 3"),
    "frame_project_from/dst-idx--1": (-6, "frame_project_from (destination): bad index -1"),
    "frame_project_from/null-transform": (-6, "frame_project_from: null transform"),
    "frame_project_from/null-src": (-6, "null handle"),
    "result_find_stars/no-pass": (-6, "result_find_stars: the handle has not run a pass"),
    "result_gaussian_blur/no-pass": (-6, "result_gaussian_blur: the handle has not run a pass"),
    "result_unsharp_mask/no-pass": (-6, "result_unsharp_mask: the handle has not run a pass"),
    "result_tone/no-pass": (-6, "result_tone: the handle has not run a pass"),
    "result_tone/no-pass+null-curve": (-6, "result_tone: null curve"),
    "result_export_gray/no-pass": (-6, "result_export_gray: the handle has not run a pass"),
    "result_export_gray/no-pass+gamma-0": (-6, "result_export_gray: gamma 0 (tiff16.go:113, writejpg.go:111: a positive number)"),
    "frame_noise/tile": (-6, "frame_noise needs a whole-image handle (3x3 stencil)"),
    "frame_noise/tile+idx-3": (-6, "frame_noise: bad index 3 or null output"),
    "frame_noise/null-output": (-6, "frame_noise: bad index 0 or null output"),
    "weights_from_noise/tile": (-6, "frame_noise needs a whole-image handle (3x3 stencil)"),
    "frame_badpixel/tile": (-6, "frame_badpixel needs a whole-image handle (3x3 stencil, whole-frame std)"),
    "frame_badpixel/negative-sigma": (-6, "frame_badpixel: negative sigma (low -3, high 5)"),
    "frame_badpixel/tile+negative-sigma": (-6, "frame_badpixel: negative sigma (low -3, high 5)"),
    "frame_find_stars/tile": (-6, "frame_find_stars needs a whole-image handle (FindStars indexes the data 1-D)"),
    "frame_find_stars/capacity--1": (-6, "frame_find_stars: capacity -1 with an output"),
    "frame_find_stars/radius-2000": (-6, "frame_find_stars: radius 2000 not in [0, 1024]"),
    "frame_find_stars/tile+capacity--1": (-6, "frame_find_stars: capacity -1 with an output"),
    "frame_back_extract/tile": (-6, "frame_back_extract needs a whole-image handle (the grid spans the whole frame)"),
    "frame_back_extract/n_stars--1": (-6, "frame_back_extract: -1 stars"),
    "frame_back_extract/capacity--1": (-6, "frame_back_extract: capacity -1 with an output"),
    "frame_back_extract/n_stars--1+capacity--1": (-6, "frame_back_extract: -1 stars"),
    "frame_deband_horiz/tile": (-6, "frame_deband_horiz needs a whole-image handle (the window needs every row's percentile)"),
    "frame_deband_vert/tile": (-6, "frame_deband_vert needs a whole-image handle (the window needs every row's percentile)"),
    "frame_gaussian_blur/tile": (-6, "frame_gaussian_blur needs a whole-image handle (the column pass needs every row)"),
    "frame_gaussian_blur/sigma--1": (-6, "frame_gaussian_blur: GaussianKernel1D (usm.go:41-82) cannot take sigma -1.000000: its radius search (usm.go:47-54) does not end"),
    "frame_gaussian_blur/radius-too-large": (-6, "frame_gaussian_blur: a radius of 18 on a 8x6 frame: one reflect (usm.go:25-33) leaves the range"),
    "frame_unsharp_mask/tile": (-6, "frame_unsharp_mask needs a whole-image handle (the column pass needs every row)"),
    "frame_bin_from/src-tile": (-6, "frame_bin_from (source) needs a whole-image handle (a bin spans rows)"),
    "frame_bin_from/dst-tile": (-6, "frame_bin_from (destination) needs a whole-image handle (a bin spans rows)"),
    "frame_project_from/src-tile": (-6, "frame_project_from (source) needs a whole-image handle (a projection reads any row of the source)"),
    "upload_frame_cfa/tile": (-6, "upload_frame_cfa needs a whole-image handle (3x3 stencil, whole-frame std)"),
    "rgb_darkest_block/tile": (-6, "rgb_darkest_block needs a whole-image handle (the blocks span rows)"),
    "rgb_mean_star_intensity/tile": (-6, "rgb_mean_star_intensity needs a whole-image handle (a star's disc spans rows)"),
    "rgb_balance/tile": (-6, "rgb_balance needs a whole-image handle (the blocks span rows)"),
    "rgb_scale_offset_clamp/planes-0-1-3": (-6, "rgb_scale_offset_clamp: bad index 3"),
    "rgb_scale_offset_clamp/planes--1-1-2": (-6, "rgb_scale_offset_clamp: bad index -1"),
    "rgb_scale_offset_clamp/planes-0-0-1": (-6, "rgb_scale_offset_clamp: slot 0 names two planes"),
    "rgb_scale_offset_clamp/null-planes": (-6, "rgb_scale_offset_clamp: null planes"),
    "rgb_darkest_block/planes-0-1-3": (-6, "rgb_darkest_block: bad index 3"),
    "rgb_darkest_block/planes--1-1-2": (-6, "rgb_darkest_block: bad index -1"),
    "rgb_darkest_block/planes-0-0-1": (-6, "rgb_darkest_block: slot 0 names two planes"),
    "rgb_darkest_block/null-planes": (-6, "rgb_darkest_block: null planes"),
    "rgb_mean_star_intensity/planes-0-1-3": (-6, "rgb_mean_star_intensity: bad index 3"),
    "rgb_mean_star_intensity/planes--1-1-2": (-6, "rgb_mean_star_intensity: bad index -1"),
    "rgb_mean_star_intensity/planes-0-0-1": (-6, "rgb_mean_star_intensity: slot 0 names two planes"),
    "rgb_mean_star_intensity/null-planes": (-6, "rgb_mean_star_intensity: null planes"),
    "rgb_balance/planes-0-1-3": (-6, "rgb_balance: bad index 3"),
    "rgb_balance/planes--1-1-2": (-6, "rgb_balance: bad index -1"),
    "rgb_balance/planes-0-0-1": (-6, "rgb_balance: slot 0 names two planes"),
    "rgb_balance/null-planes": (-6, "rgb_balance: null planes"),
    "rgb_chroma/planes-0-1-3": (-6, "rgb_chroma: bad index 3"),
    "rgb_chroma/planes--1-1-2": (-6, "rgb_chroma: bad index -1"),
    "rgb_chroma/planes-0-0-1": (-6, "rgb_chroma: slot 0 names two planes"),
    "rgb_chroma/null-planes": (-6, "rgb_chroma: null planes"),
    "rgb_export/planes-0-1-3": (-6, "rgb_export: bad index 3"),
    "rgb_export/planes--1-1-2": (-6, "rgb_export: bad index -1"),
    "rgb_export/planes-0-0-1": (-6, "rgb_export: slot 0 names two planes"),
    "rgb_export/null-planes": (-6, "rgb_export: null planes"),
    "rgb_scale_offset_clamp/null-coefficients": (-6, "rgb_scale_offset_clamp: null coefficients"),
    "rgb_scale_offset_clamp/planes-0-1-3+null-coefficients": (-6, "rgb_scale_offset_clamp: bad index 3"),
    "rgb_chroma/null-operation": (-6, "rgb_chroma: null operation"),
    "rgb_chroma/unknown-kind": (-6, "rgb_chroma: unknown kind 99 (NL_CHROMA_GAMMA ... NL_ROTATE_HUES)"),
    "rgb_export/bits-12": (-6, "rgb_export: 12 bits (8: image.Gray, 16: image.Gray16)"),
    "rgb_export/gamma-0": (-6, "rgb_export: gamma 0 (tiff16.go:113, writejpg.go:111: a positive number)"),
    "rgb_export/null-output": (-6, "rgb_export: null output"),
    "frame_project_from/in-place": (-6, "frame_project_from: slot 1 of one handle is source and destination (a projection cannot run in place)"),
    "frame_project_from/singular": (-6, "Matrix has no inverse, epsilon=0"),
    "project_tile_paths/singular": (-6, "Matrix has no inverse, epsilon=0"),
    "frame_bin_from/wrong-shape": (-6, "frame_bin_from: 8x6 binned by 2 is 4x3, the destination is 8x6"),
    "frame_bin_from/empty": (-6, "NewImageBinNxN (fits.go:163-195): 8x6 binned by 16 gives an empty 0x0 image"),
    "frame_combine_from/wrong-shape": (-6, "frame_combine_from: source 8x6 rows [0, 6), destination 4x3 rows [0, 3)"),
    "frame_combine_from/tile-of-other-rows": (-6, "frame_combine_from: source 8x6 rows [0, 6), destination 8x6 rows [2, 4)"),
    "upload_frame_cfa/wrong-shape": (-6, "upload_frame_cfa: a 4x4 mosaic debayers to 4x4, the handle is 8x6"),
    "frame_calibrate/light-differs-from-dark": (-6, "0: Light dimensions [4 3] differ from dark dimensions [8 6]"),
    "rgb_darkest_block/block-0": (-6, "rgb_darkest_block: block size 0 (findDarkestBlock, rgb.go:158, divides by it)"),
    "rgb_darkest_block/border--1": (-6, "rgb_darkest_block: border -1 (rgb.go:158-161: the first block would lie below 0)"),
    "rgb_darkest_block/null-output": (-6, "rgb_darkest_block: null output"),
    "rgb_balance/block-0": (-6, "rgb_balance: block size 0 (findDarkestBlock, rgb.go:158, divides by it)"),
    "rgb_balance/border--1": (-6, "rgb_balance: border -1 (rgb.go:158-161: the first block would lie below 0)"),
    "rgb_balance/block-0+hfr--1": (-6, "rgb_balance: block size 0 (findDarkestBlock, rgb.go:158, divides by it)"),
    "rgb_balance/hfr--1": (-6, "rgb_balance: star 1 has HFR -1 (meanStarIntensity, rgb.go:239-240: a disc radius in [0, 1024])"),
    "rgb_balance/n_stars--1": (-6, "rgb_balance: -1 stars"),
    "rgb_balance/null-location": (-6, "rgb_balance: null location or scale"),
    "rgb_mean_star_intensity/hfr--1": (-6, "rgb_mean_star_intensity: star 1 has HFR -1 (meanStarIntensity, rgb.go:239-240: a disc radius in [0, 1024])"),
    "rgb_mean_star_intensity/n_stars--1": (-6, "rgb_mean_star_intensity: -1 stars"),
    "rgb_mean_star_intensity/null-output": (-6, "rgb_mean_star_intensity: null output"),
    "upload_frame_cfa/unknown-cfa": (-6, "Unknown CFA value XYZW"),
    "upload_frame_cfa/unknown-channel": (-6, "Unknown debayering value Q"),
    "upload_frame_cfa/unknown-cfa+channel": (-6, "Unknown CFA value XYZW"),
    "upload_frame_cfa/no-channel": (-6, "upload_frame_cfa needs a channel and a CFA (mono frames: nl_stack_upload_tile, nl_stack_frame_calibrate, nl_stack_frame_badpixel)"),
    "upload_frame_cfa/null-handle": (-6, "null handle"),
    "find_stars/capacity--1": (-6, "find_stars: capacity -1 with an output"),
    "back_extract/n_stars--1": (-6, "back_extract: -1 stars"),
    "back_extract/no-grid+n_stars--1": (-6, "back_extract: -1 stars"),
    "bin_nxn/empty": (-6, "NewImageBinNxN (fits.go:163-195): 8x6 binned by 16 gives an empty 0x0 image"),
    "preprocess_frame_cfa/unknown-cfa": (-6, "Unknown CFA value XYZW"),
    "preprocess_frame/light-differs-from-dark": (-6, "5: Light dimensions [4 3] differ from dark dimensions [8 6]"),
    "rgb_balance-host/block-0": (-6, "rgb_balance: block size 0 (findDarkestBlock, rgb.go:158, divides by it)"),
    "tone-host/unknown-kind": (-6, "tone: unknown kind 99 (NL_TONE_SCALE_OFFSET ... NL_TONE_SHIFT_BLACK)"),
}


def run_row(L, ctx, call):
    """(return code, nl_last_error()) of one row"""
    rc = call(L, ctx)
    return rc, L.nl_last_error().decode("utf-8", "replace")


@pytest.fixture(scope="module")
def ctx(nl):
    c = Ctx(capi.load())
    yield c
    c.close()


def test_codes_and_messages_on_real_handles(ctx):
    ids = [rid for rid, _ in ROWS]
    assert len(set(ids)) == len(ids) and set(ids) == set(EXPECTED)
    got = {rid: run_row(ctx.L, ctx, call) for rid, call in ROWS}
    assert all(rc != capi.OK for rc, _ in got.values()), "a row got past its argument checks"
    wrong = {rid: (got[rid], EXPECTED[rid]) for rid in got if got[rid] != EXPECTED[rid]}
    assert not wrong, "(got, expected) per row: %r" % wrong


def test_frame_stats_happy_path(ctx):
    """resident_target and sum_stat_partials: 0 .. 47 in slot 1 of A"""
    L = ctx.L
    capi.check(L.nl_stack_upload_tile(ctx.A, 1, f(FRAME)))
    mn, mean, mx, var = C.c_float(), C.c_float(), C.c_float(), C.c_double()
    capi.check(L.nl_stack_frame_stats(ctx.A, 1, C.byref(mn), C.byref(mean), C.byref(mx), C.byref(var)))
    assert (mn.value, mean.value, mx.value) == (0.0, 23.5, 47.0)
    assert var.value == (48 * 48 - 1) / 12.0


def test_tone_with_statistics_happy_path(nl):
    """the host-form runner: 2 x + 1 over a 4x4 host frame"""
    out, (mn, mean, mx) = nl.tone(np.arange(16, dtype=np.float32), capi.TONE_SCALE_OFFSET, 2.0, 1.0, stats=True)
    assert np.array_equal(out, 2.0 * np.arange(16, dtype=np.float32) + 1.0)
    assert (mn, mean, mx) == (1.0, 16.0, 31.0)


def test_export_rgb_happy_path(nl):
    """the three-plane runner and the export: 16 pixels, 8 bits"""
    r = np.linspace(0.0, 1.0, 16, dtype=np.float32)
    planar = np.concatenate([r, r[::-1], np.full(16, 0.5, np.float32)])
    got = nl.export_rgb(planar, 0.0, 1.0, gamma=1.0, bits=8)
    want = np.stack([np.floor(planar[16 * c:16 * (c + 1)] * np.float32(255.0)) for c in range(3)]
                    + [np.full(16, 255.0)], axis=1).astype(np.uint8)
    assert got.shape == (16, 4) and np.array_equal(got, want)
