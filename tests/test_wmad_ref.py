"""CPU: tests/wmad_ref.py, the checker of the weighted MAD-sigma pass whose weights follow their frames
(include/nlstack_wmad.h), held to the CPU oracle wherever the oracle has something to say, and to hand-computed pixels
where it has not.

(a) rejection: per pixel, the checker's two counts are those of the oracle's unweighted MAD sigma, and the whole-image
    totals agree;
(b) arithmetic: at a sigma that rejects nothing its result is the oracle's StackMeanWeighted, bit for bit;
(c) with every weight 0.5 the result is the oracle's unweighted MAD-sigma result within the rounding of a reordered sum;
(d) literal pixels: the hand-traced one of the definition, MAD 0, a sample on a bound, sigma 0, two sigmas, zero weights;
(e) a median that is not finite: the bounds reject nothing whatever the second median comes to.

The oracle is NOT called on pixels without a finite median: its second quickselect runs over Inf - Inf there, which is
as undefined as the reference's (it may leave the array).  (e) checks the claim by arithmetic instead."""
import numpy as np
import pytest

import wmad_ref as ref
from nightlight_amd import capi
from util import bits_equal

F = np.float32
ALL = ref.CASES + ref.ADVERSARIAL
IDS = [c.name for c in ALL]

assert ref.ST_MAD == capi.ST_MAD_SIGMA


def oracle_per_pixel(oracle, frames, sigmas, pixels):
    """(result, clip_low, clip_high) of the oracle's unweighted MAD sigma, one call per pixel (as tests/rejmap_ref.py)"""
    n, p = frames.shape
    columns = np.ascontiguousarray(frames.T)
    result, low, high = np.empty(len(pixels), F), np.zeros(len(pixels), np.int64), np.zeros(len(pixels), np.int64)
    for at, i in enumerate(pixels):
        rc, res, cl, ch, _ = oracle.stack_apply(capi.ST_MAD_SIGMA, columns[i].reshape(n, 1), None, sigmas[0], sigmas[1], ref.REF_LOC)
        assert rc == 0
        result[at], low[at], high[at] = res[0], cl, ch
    return result, low, high


def sigma_sets(case):
    return ref.ADVERSARIAL_SIGMAS if case in ref.ADVERSARIAL else [(case.kappa, case.kappa)]


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_a_counts_are_the_oracles_unweighted_mad_counts(oracle, case):
    frames = np.asarray(ref.make_frames(case))
    for sigmas in sigma_sets(case):
        t = ref.truth(case, sigmas=sigmas)
        pixels = np.flatnonzero(~t.degenerate)
        _, low, high = oracle_per_pixel(oracle, frames, sigmas, pixels)
        assert np.array_equal(t.clip_low[pixels], low) and np.array_equal(t.clip_high[pixels], high), sigmas
        assert not t.clip_low[t.degenerate].any() and not t.clip_high[t.degenerate].any()
        if not t.degenerate.any():
            rc, _, cl, ch, _ = oracle.stack_apply(capi.ST_MAD_SIGMA, frames, None, sigmas[0], sigmas[1], ref.REF_LOC)
            assert rc == 0 and (cl, ch) == (int(low.sum()), int(high.sum()))
    p = case.width * case.height
    assert t.n[p // 2] == 0 and t.result[p // 2] == F(ref.REF_LOC) and t.n[p // 2 + 7] == 1
    assert case.frames < 2 or t.n[p // 2 + 9] == 2
    if case in ref.CASES and case.frames >= 8:
        assert (t.clip_high > 0).mean() > 0.1 and t.clip_low.any()                  # (the counts were put to work)
        assert (t.n & 1).any() and not (t.n & 1).all() and not t.degenerate.any()   # odd and even n


@pytest.mark.parametrize("case", ref.CASES, ids=[c.name for c in ref.CASES])
def test_b_without_rejection_the_result_is_the_oracles_weighted_mean(oracle, case):
    t = ref.truth(case, sigmas=(1e30, 1e30))
    assert not t.clip_low.any() and not t.clip_high.any() and np.array_equal(t.member.sum(1), t.n)
    rc, mean, _, _, _ = oracle.stack_apply(capi.ST_MEAN, np.asarray(ref.make_frames(case)), ref.weights_of(case.frames),
                                           0.0, 0.0, ref.REF_LOC)
    assert rc == 0
    assert bits_equal(t.result, mean)


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_c_equal_weights_give_the_oracles_result_within_rounding(oracle, case):
    """Every weight 0.5: the products v * 0.5 are exact and den = m / 2 exactly, so the checker (frame order, then one
    division) and the oracle (the order two quickselects and the clip swaps left, then a division by m) sum the same m
    numbers, up to the exact factor 0.5, in two orders.  Each sequential fp32 sum is off its exact value by at most
    (m - 1) 2^-24 sum|v|, each division by 2^-24 of its quotient: |difference| <= 2 m 2^-24 mean|v| (the argument of
    tests/test_wclip_ref.py (c))."""
    half = np.full(case.frames, 0.5, F)
    frames = np.asarray(ref.make_frames(case))
    t = ref.truth(case, weights=half)
    inf = (np.isinf(frames.T) & ~np.isnan(frames.T)).any(1)
    pixels = np.flatnonzero((t.n > 0) & ~inf)
    want, _, _ = oracle_per_pixel(oracle, frames, (case.kappa, case.kappa), pixels)
    m = t.member.sum(1)[pixels]
    assert (m > 0).all()                 # (the median itself is never rejected at a sigma >= 0)
    mean_abs = np.where(t.member, np.abs(frames.T.astype(np.float64)), 0.0).sum(1)[pixels] / m
    bound = 2.0 * m * 2.0 ** -24 * mean_abs
    diff = np.abs(t.result[pixels].astype(np.float64) - want.astype(np.float64))
    assert np.all(np.isfinite(diff)) and np.all(diff <= bound)
    assert case.frames < 8 or (m < t.n[pixels]).any()           # (the bound was put to work: something was rejected)


def one_pixel(values, weights, sigma_low, sigma_high):
    return ref.mad_clip(np.array(values, F).reshape(len(values), 1), np.array(weights, F), sigma_low, sigma_high)


def test_d_the_hand_traced_pixel(oracle):
    """[1, 2, 3, 4, 100], weights [1, 2, 3, 4, 5], sigma 3: median 3, deviations [2, 1, 0, 1, 97], MAD 1, bounds
    3 -/+ 3 * 1.4826 = -1.4478 / 7.4478, the 100 goes high, (1 + 4 + 9 + 16) / (1 + 2 + 3 + 4) = 30 / 10 = 3 exactly"""
    v = [1, 2, 3, 4, 100]
    t = one_pixel(v, [1, 2, 3, 4, 5], 3.0, 3.0)
    assert abs(float(t.lo[0]) + 1.4478) < 1e-5 and abs(float(t.hi[0]) - 7.4478) < 1e-5
    assert (int(t.clip_low[0]), int(t.clip_high[0])) == (0, 1)
    assert t.member[0].tolist() == [True, True, True, True, False]
    assert t.result[0] == F(3)
    rc, _, cl, ch, _ = oracle.stack_apply(capi.ST_MAD_SIGMA, np.array(v, F).reshape(5, 1), None, 3.0, 3.0, 0.0)
    assert rc == 0 and (cl, ch) == (0, 1)


def test_d_mad_zero_keeps_only_the_median_value(oracle):
    """seven 10s, one 9.5, one 12: MAD 0, both bounds ARE the median; a sample equal to a bound is kept"""
    v = [10, 10, 9.5, 10, 10, 12, 10, 10, 10]
    w = [3, 7, 1, 2, 5, 6, 4, 1, 2]
    t = one_pixel(v, w, 3.0, 3.0)
    assert t.lo[0] == F(10) and t.hi[0] == F(10)
    assert (int(t.clip_low[0]), int(t.clip_high[0])) == (1, 1)
    assert t.member[0].tolist() == [x == 10 for x in v] and t.result[0] == F(10)
    rc, _, cl, ch, _ = oracle.stack_apply(capi.ST_MAD_SIGMA, np.array(v, F).reshape(len(v), 1), None, 3.0, 3.0, 0.0)
    assert rc == 0 and (cl, ch) == (1, 1)


def test_d_a_sample_on_a_bound_is_kept(oracle):
    """c = 4 * 1.4826f.  [-c, -2, 0, 2, c]: median 0, deviations [c, 2, 0, 2, c], MAD 2, sd = 2 * 1.4826f and, at sigma 2,
    t = 4 * 1.4826f -- both products are exact (powers of two) -- so the bounds are -c and c themselves: the two samples
    ON the bounds are kept, and one ulp further out they are not"""
    c = F(4) * F(1.4826)
    w = [1, 2, 3, 4, 5]
    t = one_pixel([-c, -2, 0, 2, c], w, 2.0, 2.0)
    assert t.lo[0] == -c and t.hi[0] == c
    assert (int(t.clip_low[0]), int(t.clip_high[0])) == (0, 0) and t.member[0].all()
    out = np.nextafter(c, F(np.inf), dtype=F)
    v = [-out, -2, 0, 2, out]
    t = one_pixel(v, w, 2.0, 2.0)
    assert t.lo[0] == -c and t.hi[0] == c
    assert (int(t.clip_low[0]), int(t.clip_high[0])) == (1, 1) and t.member[0].tolist() == [False, True, True, True, False]
    rc, _, cl, ch, _ = oracle.stack_apply(capi.ST_MAD_SIGMA, np.array(v, F).reshape(5, 1), None, 2.0, 2.0, 0.0)
    assert rc == 0 and (cl, ch) == (1, 1)


def test_d_sigma_zero():
    """[0, 2, 4, 6, 8] at sigma 0: both bounds are the median, the 4 alone is kept"""
    t = one_pixel([0, 2, 4, 6, 8], [1, 1, 5, 1, 1], 0.0, 0.0)
    assert t.lo[0] == F(4) and t.hi[0] == F(4)
    assert (int(t.clip_low[0]), int(t.clip_high[0])) == (2, 2) and t.member[0].tolist() == [False, False, True, False, False]
    assert t.result[0] == F(4)


def test_d_different_sigmas_low_and_high(oracle):
    """[1, 2, 3, 4, 5, 6, 7], median 4, MAD 2, sd 2.9652: sigma_low 0.5 -> lo 2.5174 (1 and 2 go), sigma_high 1 -> hi
    6.9652 (7 goes)"""
    v = [1, 2, 3, 4, 5, 6, 7]
    w = [1, 2, 4, 8, 16, 32, 64]
    t = one_pixel(v, w, 0.5, 1.0)
    assert (int(t.clip_low[0]), int(t.clip_high[0])) == (2, 1)
    assert t.member[0].tolist() == [False, False, True, True, True, True, False]
    assert t.result[0] == F(3 * 4 + 4 * 8 + 5 * 16 + 6 * 32) / F(4 + 8 + 16 + 32)          # integers: one rounding
    rc, _, cl, ch, _ = oracle.stack_apply(capi.ST_MAD_SIGMA, np.array(v, F).reshape(7, 1), None, 0.5, 1.0, 0.0)
    assert rc == 0 and (cl, ch) == (2, 1)


def test_d_zero_weights():
    """a zero weight takes its frame out of the sum; every survivor's weight zero: 0 / 0, a NaN result"""
    t = one_pixel([1, 2, 3, 4, 100], [1, 0, 3, 4, 5], 3.0, 3.0)
    assert t.result[0] == F(1 + 9 + 16) / F(8)
    t = one_pixel([1, 2, 3, 4, 100], [0, 0, 0, 0, 5], 3.0, 3.0)
    assert (int(t.clip_low[0]), int(t.clip_high[0])) == (0, 1) and np.isnan(t.result[0])


@pytest.mark.parametrize("median", [np.inf, -np.inf, np.nan])
@pytest.mark.parametrize("sigmas", [(0.0, 0.0), (1.0, 1.0), (3.0, 0.5), (0.0, 2.0), (1e30, 1e30)], ids=lambda s: "%g,%g" % s)
def test_e_without_a_finite_median_the_bounds_reject_nothing(median, sigmas):
    """Definition, point 5.  The deviations of such a pixel are |v - median|: Inf for a finite sample and for the other
    infinity, NaN for the median's own infinity, NaN throughout for a NaN median.  The column kernel's second selection
    returns an element of that column, or half the sum of two: Inf or NaN, whichever order it leaves.  With either,
    and every sigma >= 0, the fp32 bounds reject no sample."""
    samples = np.array([-np.inf, -3e38, -1.0, 0.0, 1000.0, 3e38, np.inf], F)
    with np.errstate(all="ignore"):
        for mad in (F(np.inf), F(np.nan)):
            sd = mad * F(1.4826)
            lo, hi = F(median) - F(sigmas[0]) * sd, F(median) + F(sigmas[1]) * sd
            assert not (samples < lo).any() and not (samples > hi).any()
    # ... and the checker takes exactly that
    column = {np.inf: [np.inf, 1.0, np.inf, np.inf, 7.0], -np.inf: [-np.inf, 1.0, -np.inf, -np.inf, 7.0]}.get(median, [np.inf, -np.inf, -np.inf, np.inf])
    t = one_pixel(column, np.arange(1, len(column) + 1), *sigmas)
    assert t.degenerate[0] and (int(t.clip_low[0]), int(t.clip_high[0])) == (0, 0) and t.member[0].all()
    assert np.isnan(t.result[0]) if np.isnan(median) else t.result[0] == F(median)


def test_e_the_adversarial_pixels_are_what_they_are_named():
    for case in ref.ADVERSARIAL:
        t = ref.truth(case, sigmas=(1.0, 1.0))
        f = np.asarray(ref.make_frames(case))
        assert not t.degenerate[ref.PX_FEW_POS_INF] and np.isposinf(f[:, ref.PX_FEW_POS_INF]).any()
        assert not t.degenerate[ref.PX_FEW_NEG_INF] and np.isneginf(f[:, ref.PX_FEW_NEG_INF]).any()
        assert t.clip_high[ref.PX_FEW_POS_INF] >= np.isposinf(f[:, ref.PX_FEW_POS_INF]).sum()
        assert t.clip_low[ref.PX_FEW_NEG_INF] >= np.isneginf(f[:, ref.PX_FEW_NEG_INF]).sum()
        assert t.degenerate[[ref.PX_MOST_POS_INF, ref.PX_MOST_NEG_INF, ref.PX_HALF_HALF]].all() and t.degenerate.sum() == 3
        assert np.isnan(t.result[ref.PX_HALF_HALF])                      # -Inf * w + Inf * w


def test_the_cases_are_what_the_issue_asks_for():
    assert [c.frames for c in ref.CASES] == [1, 2, 8, 9, 16, 17, 64, 65, 112, 113, 114, 127, 128, 129, 256, 257, 512, 513]
    assert [c.frames for c in ref.ADVERSARIAL] == [24, 128, 200]
    assert ref.ADVERSARIAL_SIGMAS == [(0.0, 0.0), (1.0, 1.0), (3.0, 0.5)]
    assert all((c.width, c.height) == (61, 37) for c in ALL) and 61 * 37 % 4 and 61 * 37 % 64 and 61 * 37 % 256
    for case in ref.CASES:
        f = np.asarray(ref.make_frames(case))
        assert not np.isinf(f).any()
        t = ref.truth(case)
        if ref.BITONIC_MIN <= case.frames <= ref.REGISTER_MAX:
            # pixels the selection kernel hands to the generic list: n < 114 inside a stack of 114 ... 128 frames
            assert ((t.n > 2) & (t.n < ref.BITONIC_MIN)).sum() >= 10
    assert ref.kernel_name(8) == "stack_mad_fast_kernel<8, true>" and ref.kernel_name(9) == "stack_mad_fast_kernel<16, true>"
    assert ref.kernel_name(65) == "stack_mad_fast_kernel<80, true>" and ref.kernel_name(113) == "stack_mad_fast_kernel<128, true>"
    assert ref.kernel_name(114) == ref.kernel_name(128) == "stack_mad_bitonic_kernel<true>"
    assert ref.kernel_name(129) == ref.kernel_name(512) == "stack_clip_weighted_kernel<1, true>"
    assert ref.kernel_name(200, vec=True) == "stack_clip_weighted_kernel<4, true>"
    assert ref.kernel_name(513) == ref.kernel_name(24, exact=True) == "stack_exact_kernel<mad,follow>"
