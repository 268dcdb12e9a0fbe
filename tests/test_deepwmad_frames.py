"""CPU, numpy only: the weights and truths of the deep weighted MAD-sigma tests (tests/deepwmad_frames.py) are worth testing
with.  The GPU tests (tests/test_gpu_deepwmad.py) compare the pass with wmad_ref.mad_clip bit for bit; here are the
conditions of that comparison: distinct weights up to the deepest stack; the restatement rejects what the unweighted
deep-pass truth rejects, count for count; the frames hold the four pixels without a finite median and the one without
data, which the streaming engine hands over; and the weights MATTER -- the weighted result differs from the unweighted mean
of the same survivors by more than 1e-4 relative at half or more of the pixels, a hundred times the rounding of either
sum, so a kernel that drops the weights or pairs frames with their neighbours' cannot pass."""
import numpy as np
import pytest

import deepstack_frames as deep
import deepwmad_frames as dw

# totals of mad_clip at kappa 3 / 3 and, where the GPU tests run them, 1.2 / 1.2
TOTALS = {513: (6521, 13010), 1024: (13462, 25950), 2048: (26654, 52273)}
TIGHT_TOTALS = {1024: (97911, 105002), 2048: (197467, 210443)}


def test_weights_are_distinct_and_bounded():
    w = dw.weights_of(2048)
    assert w.dtype == np.float32 and w.shape == (2048,)
    assert np.unique(w).size == 2048
    assert w.min() >= np.float32(0.25) and w.max() <= np.float32(1.0) and w[0] == np.float32(1.0)
    # a prefix of the deepest set, and no monotone run the frame order could hide behind
    assert np.array_equal(dw.weights_of(513), w[:513])
    assert (np.diff(w) > 0).any() and (np.diff(w) < 0).any()


@pytest.mark.parametrize("n", deep.DEPTHS)
def test_the_truth_holds_what_the_gpu_tests_need(n):
    t = dw.truth(n)
    mean, low, high = deep.survivor_means(n)
    others = np.ones(deep.P, bool)
    others[list(deep.INF_PIXELS)] = False
    # the rejection ignores the weights: the counts of the unweighted restatement, outside the pixels without a finite median
    assert np.array_equal(t.clip_low[others], low[others]) and np.array_equal(t.clip_high[others], high[others])
    assert tuple(np.flatnonzero(t.degenerate)) == deep.INF_PIXELS and int(t.degenerate.sum()) == 4
    assert tuple(np.flatnonzero(t.n == 0)) == (deep.NO_DATA,)
    assert dw.handed_over(t) == 5
    assert np.all(t.clip_low[list(deep.INF_PIXELS)] == 0) and np.all(t.clip_high[list(deep.INF_PIXELS)] == 0)
    assert t.result[deep.NO_DATA] == np.float32(deep.REF_LOC)
    for p in deep.INF_PIXELS:
        assert t.result[p] == np.float32(deep.INF_RESULT[p])
    cl, ch = dw.totals(t)
    assert cl > 0 and ch > 0
    # the weights matter
    finite = ~np.isnan(mean)
    assert finite.sum() == deep.P - 5
    rel = np.abs(t.result[finite].astype(np.float64) - mean[finite]) / np.abs(mean[finite])
    differing = int((rel > 1e-4).sum())
    print("n %d: totals %d / %d, %d of %d pixels differ from the unweighted survivor mean by more than 1e-4" %
          (n, cl, ch, differing, finite.sum()))
    assert 2 * differing >= finite.sum()
    if n in TOTALS:
        assert (cl, ch) == TOTALS[n]
    # ... and differ from equal weights only in the result
    if n == 700:
        flat = dw.truth(n, weights=np.ones(n, np.float32))
        assert np.array_equal(flat.clip_low, t.clip_low) and np.array_equal(flat.clip_high, t.clip_high)
        assert np.allclose(flat.result[finite], mean[finite], rtol=1e-5, atol=0)


@pytest.mark.parametrize("n", sorted(TIGHT_TOTALS))
def test_the_tight_sigmas_reject_more(n):
    t, tight = dw.truth(n), dw.truth(n, dw.TIGHT)
    assert dw.totals(tight) == TIGHT_TOTALS[n]
    assert dw.totals(tight)[0] > dw.totals(t)[0] and dw.totals(tight)[1] > dw.totals(t)[1]
    assert dw.handed_over(tight) == 5
