"""CPU: tests/wlinfit_ref.py, the checker of the weighted linear-fit pass (include/nlstack_wlinfit.h), held to the CPU
oracle wherever the oracle has something to say, and to hand-computed pixels where it has not.

(a) rejection: per pixel, the checker's counters and its unweighted ymean are the oracle's StackLinearFit, bit for bit;
(b) arithmetic: at a sigma that rejects nothing its result is the oracle's StackMeanWeighted, bit for bit;
(c) with all weights 1 its result is the oracle's unweighted fit within the rounding of two sequential fp32 sums;
(d) - (f) which frames: SURVEY K6 with exact integer arithmetic, a literal pixel whose group of equal samples the
rejection splits, and a loop that ends through n < 3 with rejections in its last sweep."""
import numpy as np
import pytest

import wlinfit_ref as ref
from nightlight_amd import capi
from util import bits_equal

F = np.float32
ALL = ref.CASES + [ref.ADVERSARIAL]
IDS = [c.name for c in ALL]


def oracle_per_pixel(oracle, frames, kappa):
    """(result, clip_low, clip_high) of the oracle's StackLinearFit, one call per pixel (as tests/rejmap_ref.py)"""
    n, p = frames.shape
    columns = np.ascontiguousarray(frames.T)
    result, low, high = np.empty(p, F), np.zeros(p, np.int64), np.zeros(p, np.int64)
    for i in range(p):
        rc, res, cl, ch, _ = oracle.stack_apply(capi.ST_LINEAR_FIT, columns[i].reshape(n, 1), None, kappa, kappa, ref.REF_LOC)
        assert rc == 0
        result[i], low[i], high[i] = res[0], cl, ch
    return result, low, high


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_a_rejection_is_the_oracles_linear_fit(oracle, case):
    t = ref.truth(case)
    result, low, high = oracle_per_pixel(oracle, np.asarray(ref.make_frames(case)), case.kappa)
    assert np.array_equal(t.clip_low, low) and np.array_equal(t.clip_high, high)
    assert bits_equal(t.ymean, result)
    # ... and the whole-image call gives the same totals
    rc, _, cl, ch, _ = oracle.stack_apply(capi.ST_LINEAR_FIT, np.asarray(ref.make_frames(case)), None, case.kappa, case.kappa,
                                          ref.REF_LOC)
    assert rc == 0 and (cl, ch) == (int(low.sum()), int(high.sum()))


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_b_without_rejection_the_result_is_the_oracles_weighted_mean(oracle, case):
    t = ref.truth(case, kappa=1e30)
    assert not t.clip_low.any() and not t.clip_high.any() and not (t.runs > 1).any()
    rc, mean, _, _, _ = oracle.stack_apply(capi.ST_MEAN, np.asarray(ref.make_frames(case)), ref.weights_of(case.frames),
                                           0.0, 0.0, ref.REF_LOC)
    assert rc == 0
    assert bits_equal(t.result, mean)


@pytest.mark.parametrize("case", ref.CASES, ids=[c.name for c in ref.CASES])
def test_c_unit_weights_give_the_unweighted_fit_within_rounding(oracle, case):
    """num = the sequential fp32 sum of the m survivors in frame order, den = m exactly; the oracle's ymean = their
    sequential fp32 sum in sorted order / m.  Each sum is off its exact value by at most (m - 1) 2^-24 sum|v|, each
    division by 2^-24 of its quotient: |difference| <= 2 m 2^-24 mean|v|."""
    t = ref.truth(case, weights=np.ones(case.frames, F))
    frames = np.asarray(ref.make_frames(case)).T
    m = t.member.sum(1)
    some = m > 0
    mean_abs = np.where(t.member, np.abs(frames.astype(np.float64)), 0.0).sum(1)[some] / m[some]
    bound = 2.0 * m[some] * 2.0 ** -24 * mean_abs
    diff = np.abs(t.result[some].astype(np.float64) - t.ymean[some].astype(np.float64))
    assert np.all(np.isfinite(diff)) and np.all(diff <= bound)
    assert case.frames < 7 or (m[some] < t.n[some]).any()           # (the bound was put to work: something was rejected)


K6 = [10, 11, 9, 10, 12, 8, 10, 11, 9, 10, 10, 11, 9, 10, 200, 10, 10, 9, 11, 10, 10, 12, 8, 10, 10]


def test_d_survey_k6_with_integer_weights(oracle):
    """the 200 in frame 14 is rejected (high 1), the unweighted result is 10.  Small integer weights make
    every product and sum exact in fp32: the expected value is ONE rounded division.  The outlier's weight is the
    largest, so keeping it, or dropping another frame for it, shows."""
    w = np.array([(3 * k) % 7 + 1 for k in range(25)], F)
    w[14] = 9
    t = ref.fit(np.array(K6, F).reshape(25, 1), w, 2.75, 2.75)
    assert (int(t.clip_low[0]), int(t.clip_high[0])) == (0, 1) and t.ymean[0] == F(10)
    assert np.flatnonzero(~t.member[0]).tolist() == [14]
    num = sum(int(K6[k]) * int(w[k]) for k in range(25) if k != 14)
    den = sum(int(w[k]) for k in range(25) if k != 14)
    assert num < 2 ** 24 and den < 2 ** 24
    assert t.result[0] == F(num) / F(den)
    assert t.result[0] != F(num + 200 * 9) / F(den + 9)


# found by a search on the CPU (integer samples, sigma 1.5): frames 5, 7 and 10 hold 101; the fit rejects the upper two
# sorted positions of that group together with the 108s and the 109, so of the three equal samples the LOWEST frame
# index stays
SPLIT = [100, 100, 100, 99, 108, 101, 108, 101, 109, 100, 101, 99]
SPLIT_W = [1, 6, 4, 2, 7, 5, 3, 1, 6, 4, 2, 7]
SPLIT_K = [0, 1, 2, 3, 5, 9, 11]


def test_e_a_split_group_of_equal_samples_keeps_its_lower_frame_indices(oracle):
    t = ref.fit(np.array(SPLIT, F).reshape(12, 1), np.array(SPLIT_W, F), 1.5, 1.5)
    assert np.flatnonzero(t.member[0]).tolist() == SPLIT_K
    assert (int(t.clip_low[0]), int(t.clip_high[0])) == (2, 3)
    assert bool(t.split[0]) and int(t.runs[0]) == 1 and bool(t.handover[0])
    num, den = sum(SPLIT[k] * SPLIT_W[k] for k in SPLIT_K), sum(SPLIT_W[k] for k in SPLIT_K)
    assert (num, den) == (2896, 29) and t.result[0] == F(num) / F(den)
    # the weights tell the three 101s apart: keeping frame 7 or 10 instead of 5 gives another value
    for other in (7, 10):
        k = [x for x in SPLIT_K if x != 5] + [other]
        assert F(sum(SPLIT[x] * SPLIT_W[x] for x in k)) / F(sum(SPLIT_W[x] for x in k)) != t.result[0]
    rc, res, cl, ch, _ = oracle.stack_apply(capi.ST_LINEAR_FIT, np.array(SPLIT, F).reshape(12, 1), None, 1.5, 1.5, 0.0)
    assert rc == 0 and (cl, ch) == (2, 3) and bits_equal(res, t.ymean)


def test_f_a_loop_that_ends_through_n_below_3_keeps_the_set_before_its_last_sweep(oracle):
    """Two samples, 0 and 10 (the third frame is NaN): the reference's slope is 2/3 of the exact one (divisor n + 1,
    SURVEY Q5), so both residuals are 10/6 and at sigma 0.1 both samples are rejected -- in the sweep that ends the loop
    because n < 3.  The reference returns the mean of BOTH; K is both frames, the result (0 * 1 + 10 * 3) / 4."""
    frames = np.array([0.0, np.nan, 10.0], F).reshape(3, 1)
    t = ref.fit(frames, np.array([1, 5, 3], F), 0.1, 0.1)
    assert (int(t.clip_low[0]), int(t.clip_high[0])) == (1, 1)
    assert t.member[0].tolist() == [True, False, True] and t.ymean[0] == F(5) and t.result[0] == F(7.5)
    rc, res, cl, ch, _ = oracle.stack_apply(capi.ST_LINEAR_FIT, frames, None, 0.1, 0.1, 0.0)
    assert rc == 0 and (cl, ch) == (1, 1) and res[0] == F(5)


def test_the_cases_keep_the_register_engine_in_charge():
    """generic cases: at most 10 % of the pixels go to the column kernel; the adversarial case: at least 25 %, and a
    pixel of every kind"""
    for case in ref.CASES:
        t = ref.truth(case)
        assert t.handover.mean() <= 0.10, case.name
        p = case.width * case.height
        assert t.n[p // 2] == 0 and t.n[p // 2 + 7] == 1 and (case.frames < 2 or t.n[p // 2 + 9] == 2)
        assert np.isnan(np.asarray(ref.make_frames(case))).any(1).all() or case.frames < 3       # per-frame borders
    t = ref.truth(ref.ADVERSARIAL)
    assert t.handover.mean() >= 0.25
    assert t.too_many.any() and t.split.any() and t.inf.any()
    assert ref.kernel_name(ref.BY_FRAMES[65]) == "stack_linfit_weighted_kernel<96>"
    assert ref.kernel_name(ref.BY_FRAMES[200]) == ref.COLUMN_KERNEL
