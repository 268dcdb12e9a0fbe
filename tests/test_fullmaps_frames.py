"""CPU, oracle only: the frames of the full maps tests (tests/fullmaps_frames.py) are worth testing with.  The GPU tests
(tests/test_gpu_fullmaps.py) compare the MAD maps pass with the oracle pixel by pixel; these are the conditions of their
inputs: something is rejected on both sides, sample counts of both parities occur, a few pixels have no finite median (the
exact list), and from 114 frames on a good share of the tile -- but less than half -- has fewer than 114 samples (the
hand-over list of stack_mad_bitonic_kernel).

Depths 1 and 2 cannot reject: with one sample the bounds are the sample itself, with two the MAD is half their distance
and the bounds lie 1.4826 * 3 / 2 distances outside them.  There the totals must be 0 / 0, and are asserted to be."""
import numpy as np
import pytest

import fullmaps_frames as full
from nightlight_amd import capi

MAD = capi.ST_MAD_SIGMA


@pytest.mark.parametrize("n", full.DEPTHS)
def test_the_frames_hold_what_the_gpu_tests_need(oracle, n):
    fr = full.frames_of(n)
    assert fr.shape == (n, full.P) and full.P % 64 != 0
    t = full.truth(oracle, n, MAD)
    med, count = full.medians_of(fr)
    assert np.array_equal(count, t.coverage)
    print("n %d: totals %d / %d, %d pixels reject something, sample counts %d ... %d"
          % (n, t.clip_low, t.clip_high, int(((t.reject_low + t.reject_high) > 0).sum()), count.min(), count.max()))
    # both totals are positive wherever the arithmetic can reject at all
    if n >= 3:
        assert t.clip_low > 0 and t.clip_high > 0
    else:
        assert (t.clip_low, t.clip_high) == (0, 0)
    assert np.all(t.reject_low.astype(np.int64) + t.reject_high <= t.coverage)
    # both parities of the sample count
    if n >= 2:
        assert (count[count > 0] & 1).any() and not (count[count > 0] & 1).all()
    # the NaN borders grow with the frame index
    img = np.isnan(fr).reshape(n, full.H, full.W)
    widths = [int(img[i, full.BORDER_ROWS:, :].all(0)[:full.BORDER_COLUMNS + 1].sum()) for i in range(n)]
    assert widths == sorted(widths) and widths[-1] == full.BORDER_COLUMNS * (n - 1) // n
    # one pixel without data
    assert count[full.NO_DATA] == 0 and t.result[full.NO_DATA] == np.float32(full.REF_LOC)
    assert t.reject_low[full.NO_DATA] == 0 and t.reject_high[full.NO_DATA] == 0
    # the pixels without a finite median: exactly the four, at least 3 and at most 2 % of the tile, at least half of
    # their samples infinite, both signs
    undefined = np.flatnonzero((count > 0) & ~np.isfinite(med))
    assert tuple(undefined) == full.INF_PIXELS
    assert 3 <= undefined.size <= 0.02 * full.P
    for p in undefined:
        assert 2 * int(np.isinf(fr[:, p]).sum()) >= count[p] > 0
        assert med[p] == np.float32(full.INF_RESULT[p]) == t.result[p]
        assert t.reject_low[p] == 0 and t.reject_high[p] == 0
    assert {float(med[p]) for p in undefined} == {np.inf, -np.inf}
    # no other pixel holds an infinity
    others = np.ones(full.P, bool)
    others[undefined] = False
    assert not np.isinf(fr[:, others]).any()


@pytest.mark.parametrize("n", [114, 120, 128])
def test_the_bitonic_kernel_hands_over_a_good_share(n):
    _, count = full.medians_of(full.frames_of(n))
    narrow = (count > 0) & (count < full.BITONIC_MIN_SAMPLES)
    print("n %d: %d of %d pixels have fewer than %d samples" % (n, int(narrow.sum()), full.P, full.BITONIC_MIN_SAMPLES))
    assert 60 <= narrow.sum() < full.P // 2
    assert narrow[full.NARROW_NEG_INF] and not narrow[list(full.INF_PIXELS[:3])].any()


def test_the_oracle_is_not_asked_where_the_reference_is_undefined(oracle):
    """where it is defined on a pixel without a finite median -- a single infinite sample; a finite sample and +Inf -- the
    oracle gives what fullmaps_frames.truth takes from arithmetic: nothing rejected, the infinity"""
    for column, want in (([np.inf], np.inf), ([-np.inf], -np.inf), ([1000.0, np.inf], np.inf)):
        fr = np.array(column, np.float32).reshape(-1, 1)
        rc, res, cl, ch, _ = oracle.stack_apply(MAD, fr, None, 3.0, 3.0, full.REF_LOC)
        assert rc == 0 and (cl, ch) == (0, 0) and res[0] == np.float32(want)
