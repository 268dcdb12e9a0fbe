"""The restatement in deband_ref.py against hand-traced cases of OpDebandHoriz / OpDebandVert (banding.go:61-270) and
NewImageBinNxN (fits.go:163-195).  CPU only."""
import numpy as np
import pytest

import deband_ref as ref

f32 = np.float32
INF = f32(np.inf)
NAN = f32(np.nan)

# 4 x 3 frame, P = 50: n = 4 samples per row, k = int(4 * 50 * 0.01) = 2, the second smallest of each row
#   row 0: 1 2 3 4    -> 2
#   row 1: 8 4 6 2    -> 4
#   row 2: 16 8 4 12  -> 8
FRAME = np.array([1, 2, 3, 4, 8, 4, 6, 2, 16, 8, 4, 12], np.float32)


def test_horiz_4x3_window_2(oracle):
    # windowRows = 2, windowRows >> 1 = 1
    #   row 0: start -1 -> missing -1, window [2 4].  fixWindowEdge: left [2], right [4]: medians 2 and 4, mean 3,
    #          center 0.5 * (1 + 1) = 1, slope 2; i = 1: offset (1 - 2) - 1 = -2, window[1] = 3 + 2 * -2 = -1.
    #          Median of [2 -1] (even: upper 2, lower -1) = 0.5; factor 0.5 / 2 = 0.25
    #   row 1: start 0, window [2 4], median 3, factor 3 / 4 = 0.75
    #   row 2: start 1, window [4 8], median 6, factor 6 / 8 = 0.75
    out, info = ref.deband_horiz(FRAME, 4, 3, 50, 2, 0, 0, 0, oracle)
    want = np.array([.25, .5, .75, 1, 6, 3, 4.5, 1.5, 12, 6, 3, 9], np.float32)
    assert np.array_equal(out, want)
    assert info["threshold"] == np.finfo(np.float32).max
    assert info["lowest"] == f32(0.25) and info["highest"] == f32(0.75)


def test_factors_window_3_both_edges(oracle):
    # percentiles [2 4 8], windowRows = 3, windowRows >> 1 = 1; left [2] -> 2, right [4 8] -> 6, mean 4, center 1.5,
    # slope 4 / 1.5
    slope = f32(f32(4) / f32(1.5))
    #   row 0: missing -1: i = 2, offset (2 - 3) - 1.5 = -2.5: window [2 4 4 + slope * -2.5], median 2, factor 1
    w = np.array([2, 4, 8], np.float32)
    ref.fix_window_edge(w, -1, oracle)
    assert np.array_equal(w, np.array([2, 4, f32(4) + f32(slope * f32(-2.5))], np.float32)) and w[2] < -2.6
    #   row 2: end 4 > 3: missing 1, start 0: i = 0, offset (0 + 3) - 1.5 = 1.5: window [4 + slope * 1.5  4  8] = [8 4 8],
    #          median 8, factor 1
    w = np.array([2, 4, 8], np.float32)
    ref.fix_window_edge(w, 1, oracle)
    assert np.array_equal(w, np.array([8, 4, 8], np.float32))
    #   row 1: the whole window [2 4 8], median 4, factor 1
    fac, lowest, highest = ref.factors(np.array([2, 4, 8], np.float32), 3, oracle)
    assert np.array_equal(fac, np.ones(3, np.float32)) and lowest == 1 and highest == 1
    # a window beyond the axis is the axis
    assert np.array_equal(ref.factors(np.array([2, 4, 8], np.float32), 4096, oracle)[0], fac)


def test_vert_is_horiz_of_the_transpose(oracle):
    t = np.ascontiguousarray(FRAME.reshape(3, 4).T).reshape(-1)           # 3 x 4: the columns are FRAME's rows
    out, info = ref.deband_vert(t, 3, 4, 50, 2, 0, 0, 0, oracle)
    want, winfo = ref.deband_horiz(FRAME, 4, 3, 50, 2, 0, 0, 0, oracle)
    assert np.array_equal(out.reshape(4, 3).T.reshape(-1), want) and info == winfo


def test_rank(oracle):
    line = np.array([3, 1, 2, 5], np.float32)
    big = ref.MAX_FLOAT32
    assert ref.line_percentile(line, big, f32(0.001), oracle) == 1      # k = int(4 * 0.001 * 0.01) = 0: the minimum
    assert ref.line_percentile(line, big, f32(25), oracle) == 1         # k = 1
    assert ref.line_percentile(line, big, f32(50), oracle) == 2         # k = 2
    assert ref.line_percentile(line, big, f32(99.99), oracle) == 3      # k = int(3.9996) = 3 = n - 1
    assert ref.go_int(NAN) == -2 ** 63 and ref.go_int(f32(3.99)) == 3


def test_even_window_takes_the_average(oracle):
    fac, lowest, highest = ref.factors(np.array([1, 3, 3, 3, 3, 7], np.float32), 2, oracle)
    # row 2: window [3 3] -> 3, factor 1; row 1: window [1 3] -> 2, factor 2 / 3; row 5: window [3 7] -> 5, factor 5 / 7
    assert fac[2] == 1 and fac[1] == f32(f32(2) / f32(3)) and fac[5] == f32(f32(5) / f32(7))
    # row 0: missing -1, window [1 3] -> [1  2 + 2 * -2] = [1 -2], median -0.5, factor -0.5
    assert fac[0] == f32(-0.5) and lowest == f32(-0.5) and highest == 1


def test_threshold(oracle):
    line = np.array([INF, 1, -INF, 2, NAN], np.float32)
    # sigma 0: MaxFloat32 drops +Inf and NaN, keeps -Inf: samples [1 -Inf 2], k = int(1.5) = 1
    t = ref.threshold_of(0, 5, 7)
    assert t == ref.MAX_FLOAT32
    assert ref.line_percentile(line, t, f32(50), oracle) == -INF
    assert ref.line_percentile(line, t, f32(99), oracle) == 1            # k = int(2.97) = 2
    # sigma 3: location + sigma * scale in fp32
    assert ref.threshold_of(3, 1, f32(0.25)) == f32(1.75)
    assert ref.line_percentile(np.array([1, 2, 3, 9], np.float32), f32(3), f32(99), oracle) == 2   # [1 2 3], k = 2


def test_threshold_99_of_two(oracle):
    # samples [1 -Inf]: k = int(2 * 99 * 0.01) = 1, the minimum
    assert ref.line_percentile(np.array([INF, 1, -INF, 2], np.float32), f32(1.75), f32(99), oracle) == -INF


def test_guards(oracle):
    for p, window in ((0, 2), (100, 2), (-1, 2), (50, 0), (50, -3)):
        out, info = ref.deband_horiz(FRAME, 4, 3, p, window, 3, 2, 1, oracle)
        assert np.array_equal(out, FRAME)
        assert info == dict(threshold=f32(5), lowest=f32(1), highest=f32(0))
    for p in (0, 100, 150):
        out, info = ref.deband_vert(FRAME, 4, 3, p, 0, 0, 0, 0, oracle)
        assert np.array_equal(out, FRAME) and info["lowest"] == 1 and info["highest"] == 0


def test_panics(oracle):
    frame = FRAME.copy()
    frame[4:8] = NAN                                         # a row with no sample
    with pytest.raises(ref.GoPanic):
        ref.deband_horiz(frame, 4, 3, 50, 2, 0, 0, 0, oracle)
    with pytest.raises(ref.GoPanic):                         # a row entirely above the threshold
        ref.deband_horiz(FRAME, 4, 3, 50, 2, 1, 2, 1, oracle)
    with pytest.raises(ref.GoPanic):                         # a NaN threshold passes nothing
        ref.deband_vert(FRAME, 4, 3, 50, 2, 1, NAN, 1, oracle)
    for window in (0, -1):                                   # vert has no window guard
        with pytest.raises(ref.GoPanic):
            ref.deband_vert(FRAME, 4, 3, 50, window, 0, 0, 0, oracle)
    with pytest.raises(ref.GoPanic):                         # fixWindowEdge of one element: an empty left half
        ref.fix_window_edge(np.array([1], np.float32), 1, oracle)


def test_zero_percentile_divides(oracle):
    frame = np.array([0, 0, 0, 1, 1, 1], np.float32)                      # 3 x 2: percentiles [0 1]
    out, info = ref.deband_horiz(frame, 3, 2, 50, 1, 0, 0, 0, oracle)
    # window 1: the median is the row's own percentile: 0 / 0 = NaN moves neither bound, 1 / 1 = 1
    assert np.isnan(out[:3]).all() and np.array_equal(out[3:], frame[3:])
    assert info["lowest"] == 1 and info["highest"] == 1


def test_bin_5x5_by_2_shows_the_summation_order():
    big = 1e8
    # 2 x 2 blocks, summed over yoff then xoff from 0 in fp32 (1e8 + 1 == 1e8):
    #   [1e8 1 / -1e8 1]: ((1e8 + 1) - 1e8) + 1 = 1     -> 0.25  (column first: (1e8 - 1e8) + 1 + 1 = 2)
    #   [1 1e8 / 1 -1e8]: ((1 + 1e8) + 1) - 1e8 = 0     -> 0
    #   [1 2 / 3 4]: 10                                  -> 2.5
    #   [NaN 1 / 1 1]                                    -> NaN
    # the fifth column and row are dropped
    img = np.array([[big, 1, 1, big, 7e8],
                    [-big, 1, 1, -big, 7e8],
                    [1, 2, NAN, 1, 7e8],
                    [3, 4, 1, 1, 7e8],
                    [7e8, 7e8, 7e8, 7e8, 7e8]], np.float32)
    out, ow, oh = ref.bin_nxn(img.reshape(-1), 5, 5, 2)
    assert (ow, oh) == (2, 2)
    assert np.array_equal(out[:3], np.array([0.25, 0, 2.5], np.float32)) and np.isnan(out[3])
    # n <= 1 is OpBin's no-op; n = 5 is the whole frame; n = 6 leaves nothing
    same, ow, oh = ref.bin_nxn(img.reshape(-1), 5, 5, 1)
    assert (ow, oh) == (5, 5) and np.array_equal(same, img.reshape(-1), equal_nan=True)
    assert ref.bin_shape(5, 5, 5) == (1, 1) and ref.bin_shape(5, 5, 6) == (0, 0) and ref.bin_shape(67, 29, 3) == (22, 9)
