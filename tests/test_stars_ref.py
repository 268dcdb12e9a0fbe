"""Hand-traced known answers for star.FindStars (internal/star/findstars.go), checked against the CPU restatement in
stars_ref.py, and the CPU-side contract of the new entry points: the library exports them, and without a device they
fail with NL_ERR_NO_DEVICE instead of computing on the CPU."""
import ctypes
import math

import numpy as np
import pytest

import stars_ref as ref

f32 = np.float32


def ids(stars):
    return [s[ref.IDX] for s in stars]


def test_row_chain_replace_keep_on_equal_and_sliding_window():
    # radius 2, threshold 1.  Row 0: x=1 (5) opens; x=2 (3) is kept out (5 >= 3); x=3 (7) replaces it; x=4 (7) is
    # kept out on equality; x=5 (2) is kept out only because the window slid to x=3 with the replacement (from x=1 it
    # would be 4 away); x=8 (4) opens a new candidate.  Row 1 starts fresh at x=0 although x=8 of row 0 is near in 1-D.
    data = np.array([0, 5, 3, 7, 7, 2, 0, 0, 4,
                     6, 0, 0, 0, 0, 0, 0, 0, 0], np.float32)
    got = ref.find_bright_pixels(data, 9, f32(1), 2)
    assert ids(got) == [3, 8, 9]
    assert [float(s[ref.VAL]) for s in got] == [7.0, 4.0, 6.0]
    assert [(float(s[ref.X]), float(s[ref.Y])) for s in got] == [(3.0, 0.0), (8.0, 0.0), (0.0, 1.0)]
    assert all(s[ref.MASS] == s[ref.VAL] and s[ref.HFR] == 1 for s in got)


def test_nan_pixel_is_never_a_candidate():
    data = np.array([np.nan, 5, np.nan, 0], np.float32)
    assert ids(ref.find_bright_pixels(data, 4, f32(1), 0)) == [1]


def test_qsort_tie_permutation():
    # masses [1, 2, 2, 2] (labels = index).  Partition of 4, pivot a[1] = 2: swap(0, 3), swap(1, 2), return 1;
    # [:2] = labels 3, 2 -> swapped to 2, 3; [2:] = labels 1, 0 -> unchanged.
    a = [ref.star(i, m, 0, 0, m, 1) for i, m in enumerate([1, 2, 2, 2])]
    ref.qsort_desc(a)
    assert ids(a) == [2, 3, 1, 0]


def test_qsort_two_equal_masses_swap():
    a = [ref.star(7, 1, 0, 0, 3, 1), ref.star(8, 1, 0, 0, 3, 1)]
    ref.qsort_desc(a)
    assert ids(a) == [8, 7]


def test_qsort_nan_pivot_panics():
    a = [ref.star(0, 1, 0, 0, 5, 1), ref.star(1, 1, 0, 0, np.nan, 1), ref.star(2, 1, 0, 0, 4, 1)]
    with pytest.raises(ref.GoPanic):
        ref.qsort_desc(a)


def test_equal_mass_neighbours_across_a_bin_boundary():
    # A at x=255 lies in cell 0, B at x=256 in cell 1; equal masses.  The filter keeps whichever comes first (the
    # other sees it in an adjacent cell); sorting the pair [A, B] swaps it, so B survives.
    a = ref.star(10 * 512 + 255, 9, 255, 10, 9, 1)
    b = ref.star(10 * 512 + 256, 9, 256, 10, 9, 1)
    assert ids(ref.filter_out_overlaps([list(a), list(b)], 512, 256, 3)) == [a[0]]
    assert ids(ref.filter_out_overlaps([list(b), list(a)], 512, 256, 3)) == [b[0]]
    pair = [list(a), list(b)]
    ref.qsort_desc(pair)
    assert ids(ref.filter_out_overlaps(pair, 512, 256, 3)) == [b[0]]


def test_right_edge_spill_into_the_wrong_cell():
    # 512 x 768: xBins 2, yBins 3.  S at x=511.6, y=299: xCell int32(512.1)/256 = 2 = xBins, yCell 1, cell index
    # 2 + 1*2 = 4, which is cell (0, 2).  T at (510.5, 250) lies 49 px away (int32(1.1^2 + 49^2 + 0.5) = 2402 <= 50^2)
    # but searches cells (0..1, 0..1) only: both survive.
    s = ref.star(0, 9, 511.6, 299, 9, 1)
    t = ref.star(1, 8, 510.5, 250, 8, 1)
    assert ids(ref.filter_out_overlaps([s, t], 512, 768, 50)) == [0, 1]
    # in the last cell row the same spill indexes past the grid: the reference panics
    with pytest.raises(ref.GoPanic):
        ref.filter_out_overlaps([ref.star(0, 9, 511.6, 700, 9, 1)], 512, 768, 50)


def test_go_int32_conversion():
    assert ref.go_i32(f32(-0.7)) == 0
    assert ref.go_i32(f32(-1.2)) == -1
    assert ref.go_i32(f32(0.99999994)) == 0
    assert ref.go_i32(float("nan")) == ref.INT32_MIN
    assert ref.go_i32(3e9) == ref.INT32_MIN
    assert ref.go_div(ref.go_i32(float("nan")), 256) == -8388608
    assert ref.go_div(-1, 256) == 0


def test_centroid_negative_delta_truncates_to_zero():
    # 10 x 5, star at (5, 2), radius 1, threshold 0: weights 3 at the star and 7 at (4, 2).  dX = -7/10 = -0.7:
    # X = 5 - 0.7, int32(-0.7 + 0.5) = 0 keeps the index; the second round repeats the window (shift 0).
    data = np.zeros(50, np.float32)
    data[25], data[24] = 3, 7
    out, shifts = ref.shift_to_center_of_mass([ref.star(25, 3, 5, 2, 3, 1)], data, 10, f32(0), 1)
    s = out[0]
    assert s[ref.IDX] == 25 and s[ref.X] == f32(f32(5) + f32(f32(-7) / f32(10))) and s[ref.Y] == 2
    assert s[ref.MASS] == 10 and s[ref.VAL] == 3 and s[ref.HFR] == 0
    assert shifts == 0


def test_centroid_pulled_through_the_row_wrap():
    # 10 x 5, star at (9, 1) (index 19), radius 1, threshold 0.  Its x=+1 neighbour in 1-D is index 20 = (0, 2).
    # Round 1: weights 1 (19) and 1 (20): dX = 0.5, X = 9.5, index 19 + int32(1.0) = 20.
    # Round 2 from 20 = (0, 2): 19 is its x=-1 neighbour: dX = -0.5, X = -0.5, shift (-0.5 - 9.5)^2 = 100.
    # Round 3: the same window, shift 0: done.
    data = np.zeros(50, np.float32)
    data[19], data[20] = 1, 1
    out, shifts = ref.shift_to_center_of_mass([ref.star(19, 1, 9, 1, 1, 1)], data, 10, f32(0), 1)
    s = out[0]
    assert (s[ref.IDX], float(s[ref.X]), float(s[ref.Y]), float(s[ref.MASS])) == (20, -0.5, 2.0, 2.0)
    assert shifts == 0


def test_edge_candidate_median_uses_the_previous_leftover_buffer():
    # 4 x 3, data = 0 .. 11.  Candidate 5 is interior: its gather 0 1 2 4 5 6 8 9 10 is sorted, so the network leaves
    # the buffer as it is.  Candidate 10's mask reaches past the end: it fills slots 0..5 with 5 6 7 9 10 11 and slots
    # 6..8 still hold 8 9 10 -> median 9, diff 1.  Alone (zeroed buffer: 5 6 7 9 10 11 0 0 0) its median is 6, diff 4.
    data = np.arange(12, dtype=np.float32)
    c5, c10 = ref.star(5, 5, 1, 1, 5, 1), ref.star(10, 10, 2, 2, 10, 1)
    assert ids(ref.reject_bad_pixels([c5, c10], data, 4, 2.0, 1.0)) == [5, 10]      # |diff| 1 < 2
    assert ids(ref.reject_bad_pixels([c10], data, 4, 2.0, 1.0)) == []               # |diff| 4
    buf = [f32(v) for v in (5, 6, 7, 9, 10, 11, 8, 9, 10)]
    assert ref.median9_inplace(buf) == 9


def hfr_disc(center):
    # 7 x 7, star at (3, 3), radius 2 (13-pixel disc: distance^2 <= ceil((2 + 1e-8)^2) = 4), location 0:
    # centre `center`, the four distance-1 pixels 1, the four distance-2 pixels 4, the diagonals 0.
    img = np.zeros((7, 7), np.float32)
    img[3, 3] = center
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        img[3 + dy, 3 + dx] = 1
    for dy, dx in ((-2, 0), (2, 0), (0, -2), (0, 2)):
        img[3 + dy, 3 + dx] = 4
    return img.reshape(-1)


def test_hfr_plausibility_at_equality_rejects_and_avg_is_nan():
    # centre 16: moment 4*1 + 4*4*2 = 36, mass 36, HFR 1 -> inner disc distance^2 <= 1: mass 20 over 5 pixels, outer
    # 16 over 8.  starInOut 2: 20*8 = 160 <= 2*16*5 = 160 -> rejected (equality rejects); no star left: avgHFR 0/0.
    data = hfr_disc(16)
    kept, avg = ref.calc_and_filter_hfr([ref.star(24, 16, 3, 3, 0, 0)], data, 7, 2, 0, 2.0)
    assert kept == [] and math.isnan(avg)
    # centre 17: HFR 36/37, inner 21: 168 > 160 -> kept, HFR and mass written
    data = hfr_disc(17)
    kept, avg = ref.calc_and_filter_hfr([ref.star(24, 17, 3, 3, 0, 0)], data, 7, 2, 0, 2.0)
    assert len(kept) == 1 and kept[0][ref.HFR] == f32(f32(36) / f32(37)) and kept[0][ref.MASS] == 37
    assert avg == kept[0][ref.HFR]


def test_radius_zero_finds_no_star():
    data = np.full(100, 10.0, np.float32)
    data[[12, 45, 77]] = [500, 600, 700]
    stars, shifts, avg = ref.find_stars(data, 10, 10.0, 1.0, 15.0, 0.0, 1.4, 0)
    assert stars == [] and shifts == 0 and math.isnan(avg)


def test_nan_pixel_in_a_centroid_window_panics():
    img = np.full((48, 64), 100.0, np.float32)
    img[20, 30], img[20, 31], img[22, 33] = 5000.0, 3000.0, np.nan
    with pytest.raises(ref.GoPanic):
        ref.find_stars(img.reshape(-1), 64, 100.0, 10.0, 15.0, 0.0, 1.4, 16)
    img[22, 33] = 100.0
    stars, _, _ = ref.find_stars(img.reshape(-1), 64, 100.0, 10.0, 15.0, 0.0, 1.4, 16)
    assert ids(stars) == [20 * 64 + 30]


def test_library_exports_the_star_entry_points():
    from nightlight_amd import capi
    lib = ctypes.CDLL(capi.LIB_PATH)
    for sym in ("nl_find_stars", "nl_stack_frame_find_stars", "nl_stack_result_find_stars"):
        assert sym in capi.EXPORTS and hasattr(lib, sym)
    assert capi.STAR_DTYPE.itemsize == 24
    assert capi.STAR_DTYPE.names == ("index", "value", "x", "y", "mass", "hfr")


def test_star_detection_has_no_cpu_fallback():
    from nightlight_amd import capi
    import nightlight_amd as nl
    if capi.device_count() > 0:
        pytest.skip("a device is visible: the no-device contract is checked on CPU-only hosts")
    data = np.full(64, 10.0, np.float32)
    n = ctypes.c_int(-1)
    rc = capi.load().nl_find_stars(capi.fptr(data), 8, 8, 10.0, 1.0, 15.0, 5.0, 1.4, 16, float("nan"), None, 0,
                                   ctypes.byref(n), None, None, 0)
    assert rc == capi.ERR_NO_DEVICE and "no HIP device" in capi.last_error()
    with pytest.raises(capi.NlError) as e:
        nl.find_stars(data, 8, 8, 10.0, 1.0)
    assert e.value.code == capi.ERR_NO_DEVICE
