"""Hand-traced known answers for pre.NewBackground / Subtract (internal/ops/pre/background.go), checked against the CPU
restatement in background_ref.py, and the CPU-side contract of the new entry points: the library exports them, and
without a device they fail with NL_ERR_NO_DEVICE instead of computing on the CPU."""
import ctypes

import numpy as np
import pytest

import background_ref as ref

f32 = np.float32


def stars(*rows):
    from nightlight_amd import capi
    st = np.zeros(len(rows), capi.STAR_DTYPE)
    for i, (x, y, hfr) in enumerate(rows):
        st[i]["x"], st[i]["y"], st[i]["hfr"], st[i]["index"] = x, y, hfr, i
    return st


def test_even_count_median_averages_the_two_middle_values(oracle):
    # [1, 2, 3, 10]: median 2.5; |v - 2.5| = [1.5, .5, .5, 7.5] -> MAD 1; bound 2.5 + 1.5*1.4826 = 4.72; trimmed
    # [1, 2, 3] -> 2
    assert ref.fit_cell(np.array([10, 1, 3, 2], np.float32), 1.5, oracle) == f32(2.0)
    assert ref.select_median(np.array([4, 1, 3, 2], np.float32), oracle)[0] == f32(2.5)


def test_pixel_exactly_on_the_disc_is_masked():
    # star at (2, 2), HFR 0.5, factor 4: hfrSq = 0.25*4*4 = 4; (4, 2) has distSq 4 -> masked; (4, 3) has 5 -> kept
    img = np.arange(36, dtype=np.float32).reshape(6, 6)
    s = stars((2.0, 2.0, 0.5))
    got = ref.gather(img, (0, 6, 0, 6), [(f32(2), f32(2), ref.hfr_sq(s[0], 4.0))])
    assert img[2, 4] not in got and img[3, 4] in got
    assert got.size == 36 - 13


def test_star_binned_only_into_the_cells_its_sample_points_hit():
    # 64 x 64, g 32: 2 x 2 cells of spacing 32, hfr*f = 1.  A star at (30, 10) samples x = 29, 30, 31: cell 0 only;
    # one at (31.5, 10) samples x = 32.5 too: cells 0 and 1.
    s = stars((30.0, 10.0, 0.25), (31.5, 10.0, 0.25))
    bins = ref.bin_stars(s, 2, 2, f32(32), f32(32), 4.0)
    assert bins[0] == [0, 1] and bins[1] == [1] and bins[2] == [] and bins[3] == []
    # star 1's disc (hfrSq 1) holds one pixel of cell 1, (32, 10) at distSq 0.25 ((32, 9) has 1.25): masked there
    img = np.zeros((64, 64), np.float32)
    e1 = [(f32(31.5), f32(10), ref.hfr_sq(s[1], 4.0))]
    assert ref.gather(img, (32, 64, 0, 32), e1).size == 32 * 32 - 1
    # a disc wider than a cell: hfr*f = 70 over cells of 32 samples x = 0, 70, 140 (cells 0, 2, 4) and y = -60, 10, 80
    # (cells 0, 0, 2), so cell (1, 0) lists no star and its pixel (50, 10), 20 from the centre, stays in
    big = stars((70.0, 10.0, 17.5))
    bins = ref.bin_stars(big, 10, 10, f32(32), f32(32), 4.0)
    assert [c for c in range(100) if bins[c]] == [0, 2, 4, 20, 22, 24]
    img = np.zeros((320, 320), np.float32)
    img[10, 50] = 5.0
    assert 5.0 in ref.gather(img, (32, 64, 0, 32), [])
    assert 5.0 not in ref.gather(img, (32, 64, 0, 32), [(f32(70), f32(10), ref.hfr_sq(big[0], 4.0))])


def test_nan_hfr_star_lands_in_cell_zero_and_repeats():
    # hfr NaN: every sample point is NaN -> int32 MinInt32 -> cell 0; s != s, so all nine appends happen
    s = stars((50.0, 50.0, np.nan))
    bins = ref.bin_stars(s, 2, 2, f32(32), f32(32), 4.0)
    assert bins[0] == [0] * 9 and bins[3] == []
    assert ref.go_i32(f32(np.nan)) == ref.INT32_MIN and ref.go_i32(f32(3e9)) == ref.INT32_MIN
    assert ref.go_i32(f32(-2.7)) == -2


def test_clip_interpolates_in_place_and_counts_outliers():
    # 3 x 3 grid; clip 1 removes the 9 at the centre; its 8 neighbours [1..8] -> median 4.5
    cells = [f32(v) for v in (1, 2, 3, 4, 9, 5, 6, 7, 8)]
    assert ref.clip(cells, 3, 3, 1) == 1
    assert cells[4] == f32(4.5)
    # clip 2 removes 9 and 8 (bottom right); in raster order the centre sees 7 valid neighbours -> waits for 7;
    # the corner (3 neighbours: 5, 7, and the NaN centre) fills at neighbors = 2 after the centre did at 7
    cells = [f32(v) for v in (1, 2, 3, 4, 9, 5, 6, 7, 8)]
    assert ref.clip(cells, 3, 3, 2) == 2
    assert cells[4] == f32(4)                      # median of [1, 2, 3, 4, 5, 6, 7]
    assert cells[8] == f32(5)                      # median of [4, 5, 7] after the centre became 4


def test_gauss3x3_at_a_corner():
    cells = [f32(v) for v in (1, 2, 3, 4)]
    got = ref.gauss3x3(cells, 2, 2)
    w0, w1, w2 = ref.GAUSS
    s = f32(f32(f32(f32(0) + f32(1 * w0)) + f32(2 * w1)) + f32(f32(3) * w1))
    s = f32(s + f32(f32(4) * w2))
    ws = f32(f32(f32(f32(w0 + w1) + w1)) + w2)
    assert got[0] == f32(s / ws)


def test_subtract_tables_with_border_extrapolation():
    # width 70, g 32: 2 cells of spacing 35.  destXl = int32(-18) = -18, destXh = int32(18) = 18, span 1/36
    xl, xr = ref.axis_table(70, f32(35), 2)
    assert xr[0] < 0                             # left border: xl shifted to 0, xr outside [0, 1]
    assert xl[-1] == 0 and xr[-1] > 1            # right border: xh = 2 shifted back, xr > 1
    assert set(xl.tolist()) == {0}
    assert xr[17] == f32(f32(-1) + f32(f32(35) * f32(f32(1) / f32(36))))


def test_deviation_1_flat_plateau_empties_the_trimmed_set(oracle):
    with pytest.raises(ref.GoPanic):
        ref.fit_cell(np.full(16, 3, np.float32), 1.5, oracle)


def test_deviation_1_grid_one_cell_tall_indexes_cells_minus_one(oracle):
    with pytest.raises(ref.GoPanic):
        ref.back_extract(np.ones(96 * 20, np.float32) + np.arange(96 * 20, dtype=np.float32) % 5, 96, 20, None, 32,
                         oracle)


def test_deviation_1_nan_pivot_panics():
    a = [f32(1), f32(np.nan), f32(2)]
    with pytest.raises(ref.GoPanic):
        ref.qselect(a, 2)


def test_deviation_2_grid_larger_than_twice_the_image(oracle):
    with pytest.raises(ref.GoPanic):
        ref.back_extract(np.ones(64, np.float32), 8, 8, None, 32, oracle)


def test_deviation_3_clip_of_every_cell_hangs():
    with pytest.raises(ref.GoHang):
        ref.clip([f32(v) for v in range(9)], 3, 3, 9)


def test_nan_cell_takes_the_literal_path(oracle):
    data = np.arange(64 * 64, dtype=np.float32) % 97 + 100
    data[5] = np.nan
    out, bg, cells, info = ref.back_extract(data, 64, 64, None, 32, oracle)
    assert info["cells_x"] == 2 and not np.isnan(cells).any()


def test_library_exports_the_background_entry_points():
    from nightlight_amd import capi
    lib = ctypes.CDLL(capi.LIB_PATH)
    for sym in ("nl_back_extract", "nl_stack_frame_back_extract"):
        assert sym in capi.EXPORTS and hasattr(lib, sym)
    assert ctypes.sizeof(capi.Background) == 28


def test_background_extraction_has_no_cpu_fallback():
    from nightlight_amd import capi
    import nightlight_amd as nl
    if capi.device_count() > 0:
        pytest.skip("a device is visible: the no-device contract is checked on CPU-only hosts")
    data = np.full(64 * 64, 10.0, np.float32)
    rc = capi.load().nl_back_extract(capi.fptr(data), 64, 64, 32, 4.0, 1.5, 0, None, 0, None, None, 0, None, 0)
    assert rc == capi.ERR_NO_DEVICE and "no HIP device" in capi.last_error()
    with pytest.raises(capi.NlError) as e:
        nl.back_extract(data, 64, 64, None, 32)
    assert e.value.code == capi.ERR_NO_DEVICE
