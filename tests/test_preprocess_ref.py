"""Hand-traced known answers for OpCalibrate and OpBadPixel (mono), checked against the CPU
restatement in preprocess_ref.py, and the CPU-side contract of the new entry points: the library
exports them, and without a device they fail with NL_ERR_NO_DEVICE instead of computing on the CPU."""
import ctypes
import os

import numpy as np
import pytest

import preprocess_ref as ref
from util import bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 6x6 frame: background 1..36 row-major, seven hot pixels in three clusters:
#   adjacent pair (1,1)=900 (1,2)=800, diagonal pair (2,4)=700 (3,3)=600, L-shaped triple (3,1)=500 (4,1)=400 (4,2)=300
KAT_W = 6
KAT_HOT = {(1, 1): 900, (1, 2): 800, (2, 4): 700, (3, 3): 600, (3, 1): 500, (4, 1): 400, (4, 2): 300}

# tmp = frame - MedianFilter3x3(frame): border 0, the hot pixels 887 786 682 572 479 368 266, the rest -7..-1;
# sum 4005 -> mean 111.25, std 246.48218.  sigma 1 / 1: exactly the seven hot pixels are bad.
# Sequential MedianFilterSparse, in index order (new values marked *):
#   (1,1) {1 2 3 7 900 800 13 14 15}            -> 13
#   (1,2) {2 3 4 13* 800 10 14 15 16}           -> 13   (one pass: 900 instead of 13* -> 14)
#   (2,4) {10 11 12 16 700 18 600 23 24}        -> 18
#   (3,1) {13 14 15 19 500 21 25 400 300}       -> 21
#   (3,3) {15 16 18* 21 600 23 300 28 29}       -> 23   (one pass: 700 instead of 18* -> 28)
#   (4,1) {19 21* 21 25 400 300 31 32 33}       -> 31   (one pass: 500 instead of 21* -> 32)
#   (4,2) {21* 21 23* 31* 300 28 32 33 34}      -> 31   (one pass -> 34)
KAT_WANT = {(1, 1): 13, (1, 2): 13, (2, 4): 18, (3, 1): 21, (3, 3): 23, (4, 1): 31, (4, 2): 31}


def kat_frame():
    f = np.arange(1, 37, dtype=np.float32).reshape(6, 6)
    for (y, x), v in KAT_HOT.items():
        f[y, x] = v
    return f.reshape(-1)


def kat_want():
    w = kat_frame().reshape(6, 6).copy()
    for (y, x), v in KAT_WANT.items():
        w[y, x] = v
    return w.reshape(-1)


def test_kat_ordered_walk_differs_from_one_pass(oracle):
    frame = kat_frame()
    tmp, mean, std = ref.diff_stats(oracle, frame, KAT_W)
    assert mean == np.float32(111.25)
    assert abs(float(std) - 246.48218) < 1e-4
    assert sorted(ref.bad_pixel_map(tmp, std, 1.0, 1.0).tolist()) == sorted(y * 6 + x for y, x in KAT_HOT)
    out, removed, stats = ref.badpixel(oracle, frame, KAT_W, 1.0, 1.0)
    assert removed == 7 and stats[0] == mean and stats[1] == std
    assert bits_equal(out, kat_want())
    one_pass = ref.badpixel_one_pass(oracle, frame, KAT_W, 1.0, 1.0)
    assert not np.array_equal(out, one_pass)
    assert [one_pass[y * 6 + x] for y, x in ((1, 2), (3, 3), (4, 1), (4, 2))] == [14, 28, 32, 34]


def test_kat_higher_sigma_keeps_the_weaker_pixels(oracle):
    # sigma 2 / 2: hi = 492.96, only 887 786 682 572 are bad; the L triple stays
    out, removed, _ = ref.badpixel(oracle, kat_frame(), KAT_W, 2.0, 2.0)
    assert removed == 4
    want = kat_frame().reshape(6, 6)
    want[1, 1], want[1, 2], want[2, 4], want[3, 3] = 13, 13, 18, 23
    assert bits_equal(out, want.reshape(-1))


def test_sigma_zero_leaves_the_frame(oracle):
    for sl, sh in ((0.0, 5.0), (3.0, 0.0)):
        out, removed, stats = ref.badpixel(oracle, kat_frame(), KAT_W, sl, sh)
        assert removed == 0 and stats is None and bits_equal(out, kat_frame())


def test_one_nan_removes_nothing(oracle):
    frame = kat_frame()
    frame[20] = np.nan
    out, removed, (_, std) = ref.badpixel(oracle, frame, KAT_W, 1.0, 1.0)
    assert np.isnan(std) and removed == 0 and bits_equal(out, frame)


def test_divide_known_answers(oracle):
    a = np.array([10, 10, 10, 10, 10, -4], np.float32)
    b = np.array([2, 0, -1, np.nan, 8, 4], np.float32)
    # bMax = 8 (NaN never becomes the max); b <= 0 keeps a; NaN is not <= 0: 10*8/NaN = NaN
    assert oracle.min_mean_max(b)[2] == np.float32(8)
    got = ref.divide(a, b, 8.0)
    assert bits_equal(got, np.array([40, 10, 10, np.nan, 10, -8], np.float32))
    # (a*bMax)/b in fp32, not a*(bMax/b): 3*7 = 21, 21/3 = 7 exactly, while 7/3*3 = 7.0000005
    assert ref.divide(np.float32([3]), np.float32([3]), 7.0)[0] == np.float32(7)


def test_calibrate_dark_then_flat(oracle):
    light = np.array([110, 60, 30, 20], np.float32)
    dark = np.array([10, 10, 10, 10], np.float32)
    flat = np.array([4, 2, 0, 1], np.float32)
    assert bits_equal(ref.calibrate(oracle, light, dark=dark), light - dark)
    assert bits_equal(ref.calibrate(oracle, light, dark=dark, flat=flat), np.array([100, 100, 20, 40], np.float32))


# ---- the entry points on the CPU side ---------------------------------------------------------------

NEW_SYMBOLS = ["nl_calib_create", "nl_calib_destroy", "nl_calib_flat_max", "nl_preprocess_frame",
               "nl_stack_frame_calibrate", "nl_stack_frame_badpixel"]


def test_library_exports_the_preprocess_entry_points():
    from nightlight_amd import capi
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert [s for s in NEW_SYMBOLS if not hasattr(lib, s)] == []
    assert set(NEW_SYMBOLS) <= set(capi.EXPORTS)
    header = open(os.path.join(ROOT, "include", "nlstack.h")).read()
    assert all(s + "(" in header for s in NEW_SYMBOLS)


def test_preprocess_has_no_cpu_fallback():
    import nightlight_amd as nl
    from nightlight_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a HIP device is visible")
    frame = kat_frame()
    out = np.empty_like(frame)
    rc = capi.load().nl_preprocess_frame(None, 0, capi.fptr(frame), capi.fptr(out), 6, 6, 3.0, 5.0, None, None, 0)
    assert rc == capi.ERR_NO_DEVICE
    with pytest.raises(capi.NlError) as e:
        nl.preprocess_frame(frame, 6, 6)
    assert e.value.code == capi.ERR_NO_DEVICE
    assert not capi.load().nl_calib_create(0, capi.fptr(frame), 6, 6, None, 0, 0)
    assert "no HIP device" in capi.last_error()
    with pytest.raises(capi.NlError) as e:
        nl.Calibration(0, 6, 6, dark=frame)
    assert e.value.code == capi.ERR_NO_DEVICE
