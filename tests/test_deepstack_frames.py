"""CPU, oracle only: the frames of the deep-pass tests (tests/deepstack_frames.py) are worth testing with, and the
tolerance of the GPU tests (tests/test_gpu_deepstack.py) has room.

The GPU tests compare the deep MAD pass with the oracle pixel by pixel: totals count for count, the result within
util.RTOL.  These are the conditions of their inputs -- both parities of the sample count, pixels with far fewer samples
than frames and pixels with all of them, the four pixels without a finite median and the one without data where the
module says, something rejected on both sides, at both sigma pairs where both are run -- and the measurement behind the tolerance: the
oracle's result (a sequential fp32 sum of up to 2048 values around 1000) against the fp64 mean of the same survivors
stays within RTOL / 2 at every finite pixel of every depth, so a GPU result that misses RTOL misses it by itself."""
import numpy as np
import pytest

import deepstack_frames as deep
from nightlight_amd import capi
from util import RTOL, bits_equal

MAD = capi.ST_MAD_SIGMA


@pytest.mark.parametrize("n", deep.DEPTHS)
def test_the_frames_hold_what_the_gpu_tests_need(oracle, n):
    fr = deep.frames_of(n)
    assert fr.shape == (n, deep.P) and deep.P % 32 != 0 and deep.P % 16 != 0
    assert deep.lanes_of(n) == (8 if n <= 1024 else 16) and n > deep.lanes_of(n) * deep.LANE_SAMPLES // 2
    t = deep.truth(oracle, n, MAD)
    med, count = deep.medians_of(fr)
    assert np.array_equal(count, t.coverage)
    print("n %d: totals %d / %d, sample counts %d ... %d" % (n, t.clip_low, t.clip_high, count.min(), count.max()))
    # something is rejected on both sides; at both sigma pairs where the GPU tests run both, and the pairs give different maps
    assert t.clip_low > 0 and t.clip_high > 0
    if n in deep.TIGHT_DEPTHS:
        tight = deep.truth(oracle, n, MAD, sigmas=deep.TIGHT)
        print("n %d: totals at %.1f / %.1f: %d / %d" % ((n,) + deep.TIGHT + (tight.clip_low, tight.clip_high)))
        assert tight.clip_low > t.clip_low and tight.clip_high > t.clip_high
        assert not np.array_equal(tight.reject_low, t.reject_low) and not np.array_equal(tight.reject_high, t.reject_high)
    # both parities of the sample count; pixels with all samples, pixels with far fewer samples than frames
    assert (count[count > 0] & 1).any() and not (count[count > 0] & 1).all()
    assert count.max() == n and 0 < count[count > 0].min() < n // 4
    # one pixel without data
    assert count[deep.NO_DATA] == 0 and t.result[deep.NO_DATA] == np.float32(deep.REF_LOC)
    assert t.reject_low[deep.NO_DATA] == 0 and t.reject_high[deep.NO_DATA] == 0
    # the pixels without a finite median: exactly the four, both signs, nothing rejected
    undefined = np.flatnonzero((count > 0) & ~np.isfinite(med))
    assert tuple(undefined) == deep.INF_PIXELS
    for p in undefined:
        assert 2 * int(np.isinf(fr[:, p]).sum()) >= count[p] > 0
        assert med[p] == np.float32(deep.INF_RESULT[p]) == t.result[p]
        assert t.reject_low[p] == 0 and t.reject_high[p] == 0
    assert {float(med[p]) for p in undefined} == {np.inf, -np.inf}
    others = np.ones(deep.P, bool)
    others[undefined] = False
    assert not np.isinf(fr[:, others]).any()


@pytest.mark.parametrize("n", deep.DEPTHS)
def test_the_whole_image_truth_is_the_pixel_by_pixel_truth(oracle, n):
    """deepstack_frames.whole_truth, one oracle call per image, against truth's 943: MAD sigma bit for bit and count for
    count; the median bit for bit against the reference's median restated in numpy (medians_of; the infinite ones included)"""
    t, w = deep.truth(oracle, n, MAD), deep.whole_truth(oracle, n, MAD)
    assert bits_equal(w.result, t.result) and (w.clip_low, w.clip_high) == (t.clip_low, t.clip_high)
    med, count = deep.medians_of(deep.frames_of(n))
    want = np.where(count > 0, med, np.float32(deep.REF_LOC)).astype(np.float32)
    m = deep.whole_truth(oracle, n, capi.ST_MEDIAN)
    assert bits_equal(m.result, want) and (m.clip_low, m.clip_high) == (0, 0)


def test_the_deepest_stack_has_narrow_and_full_pixels():
    """2048 frames on 16 lanes: a pixel with fewer than 1025 samples (more than half of the 2048 positions are pads) and a
    pixel with every sample"""
    _, count = deep.medians_of(deep.frames_of(2048))
    assert ((count > 0) & (count < 1025)).any() and (count == 2048).any()


@pytest.mark.parametrize("n", deep.DEPTHS)
def test_the_tolerance_has_room(oracle, n):
    """the oracle's MAD result against the fp64 mean of the same survivors: within RTOL / 2 at every finite pixel"""
    worst = 0.0
    for sigmas in (deep.SIGMAS, deep.TIGHT) if n in deep.TIGHT_DEPTHS else (deep.SIGMAS,):
        t = deep.truth(oracle, n, MAD, sigmas=sigmas)
        mean, low, high = deep.survivor_means(n, sigmas)
        finite = ~np.isnan(mean)
        assert finite.sum() == deep.P - 1 - len(deep.INF_PIXELS)
        # the same survivors: the restatement rejects what the oracle rejects, count for count
        assert np.array_equal(low[finite], t.reject_low[finite]) and np.array_equal(high[finite], t.reject_high[finite])
        rel = np.abs(t.result[finite].astype(np.float64) - mean[finite]) / np.abs(mean[finite])
        worst = max(worst, float(rel.max()))
    print("n %d: the oracle's fp32 sum is within %.3g relative of the fp64 mean (RTOL / 2 = %.3g)" % (n, worst, RTOL / 2))
    assert worst <= RTOL / 2
