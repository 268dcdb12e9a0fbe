"""CPU: tests/wclip_ref.py, the checker of the weighted clip pass whose weights follow their frames
(include/nlstack_wclip.h), held to the CPU oracle wherever the oracle has something to say, and to hand-computed pixels
where it has not.

(a) rejection: per pixel, the checker's two counts are those of the oracle's sigma / winsorized modes, unweighted and
    weighted, and the whole-image totals agree;
(b) arithmetic: at a sigma that rejects nothing its result is the oracle's StackMeanWeighted, bit for bit;
(c) with every weight 0.5 the pairing of weights and frames cannot matter: the result is the oracle's WEIGHTED sigma /
    winsorized result within the rounding of a reordered sum -- which pins K to the set after the last sweep;
(d) a literal pixel, [1, 2, 3, 100] with weights [1, 2, 4, 8]: exactly 17 / 7, rounded once;
(e) equal samples on both sides of a bound share one fate."""
import numpy as np
import pytest

import wclip_ref as ref
from nightlight_amd import capi
from util import bits_equal

F = np.float32
ALL = ref.CASES + [ref.ADVERSARIAL]
IDS = [c.name for c in ALL]
WITH_PADDED = ALL + [ref.PADDED]                 # (b), (c): one oracle call per case, so the 512 x 512 case is in
PADDED_IDS = [c.name for c in WITH_PADDED]
MODE_IDS = {ref.ST_SIGMA: "sigma", ref.ST_WINSOR: "winsor"}

assert (ref.ST_SIGMA, ref.ST_WINSOR) == (capi.ST_SIGMA, capi.ST_WINSOR_SIGMA)


def oracle_per_pixel(oracle, mode, frames, weights, sigmas, pixels=None):
    """(result, clip_low, clip_high) of the oracle's mode, one call per pixel (as tests/rejmap_ref.py)"""
    n, p = frames.shape
    pixels = range(p) if pixels is None else pixels
    columns = np.ascontiguousarray(frames.T)
    result, low, high = np.empty(len(pixels), F), np.zeros(len(pixels), np.int64), np.zeros(len(pixels), np.int64)
    for at, i in enumerate(pixels):
        rc, res, cl, ch, _ = oracle.stack_apply(mode, columns[i].reshape(n, 1), weights, sigmas[0], sigmas[1], ref.REF_LOC)
        assert rc == 0
        result[at], low[at], high[at] = res[0], cl, ch
    return result, low, high


def sigma_sets(case):
    return ref.ADVERSARIAL_SIGMAS if case is ref.ADVERSARIAL else [(case.kappa, case.kappa)]


@pytest.mark.parametrize("mode", ref.MODES, ids=MODE_IDS.get)
@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_a_rejection_is_the_oracles_unweighted_and_weighted(oracle, case, mode):
    frames = np.asarray(ref.make_frames(case))
    for sigmas in sigma_sets(case):
        t = ref.truth(case, mode, sigmas=sigmas)
        for weights in (None, ref.weights_of(case.frames)):
            _, low, high = oracle_per_pixel(oracle, mode, frames, weights, sigmas)
            assert np.array_equal(t.clip_low, low) and np.array_equal(t.clip_high, high), (sigmas, weights is None)
            rc, _, cl, ch, _ = oracle.stack_apply(mode, frames, weights, sigmas[0], sigmas[1], ref.REF_LOC)
            assert rc == 0 and (cl, ch) == (int(low.sum()), int(high.sum()))
    p = case.width * case.height
    assert t.n[p // 2] == 0 and t.result[p // 2] == F(ref.REF_LOC) and t.n[p // 2 + 7] == 1
    assert case.frames < 2 or t.n[p // 2 + 9] == 2


def test_a_nine_frames_under_rejection(oracle):
    """plain sigma at 2.5 on 9 frames: per pixel, and something is rejected in at least a quarter of the pixels"""
    case, mode = ref.NINE_SIGMA, ref.ST_SIGMA
    frames = np.asarray(ref.make_frames(case))
    t = ref.truth(case, mode)
    for weights in (None, ref.weights_of(case.frames)):
        _, low, high = oracle_per_pixel(oracle, mode, frames, weights, (case.kappa, case.kappa))
        assert np.array_equal(t.clip_low, low) and np.array_equal(t.clip_high, high)
    assert ((t.clip_low + t.clip_high) > 0).mean() >= 0.25


@pytest.mark.parametrize("mode", ref.MODES, ids=MODE_IDS.get)
def test_a_padded_case_totals_and_a_sample_of_its_pixels(oracle, mode):
    """24 frames of 512 x 512.  A DEPARTURE from "per pixel on every case", for run time (a per-pixel oracle call costs
    about 20 us; four passes over 262 144 pixels would take this test beyond a minute): the whole-image totals of the
    weighted pass, and every 97th pixel (2 703 of them) on its own, unweighted.  The 61 x 37 cases above are per pixel."""
    case = ref.PADDED
    frames = np.asarray(ref.make_frames(case))
    t = ref.truth(case, mode)
    rc, _, cl, ch, _ = oracle.stack_apply(mode, frames, ref.weights_of(case.frames), case.kappa, case.kappa, ref.REF_LOC)
    assert rc == 0 and (cl, ch) == (int(t.clip_low.sum()), int(t.clip_high.sum()))
    pixels = list(range(0, frames.shape[1], 97))
    _, low, high = oracle_per_pixel(oracle, mode, frames, None, (case.kappa, case.kappa), pixels)
    assert np.array_equal(t.clip_low[pixels], low) and np.array_equal(t.clip_high[pixels], high)


@pytest.mark.parametrize("mode", ref.MODES, ids=MODE_IDS.get)
@pytest.mark.parametrize("case", WITH_PADDED, ids=PADDED_IDS)
def test_b_without_rejection_the_result_is_the_oracles_weighted_mean(oracle, case, mode):
    t = ref.truth(case, mode, sigmas=(1e30, 1e30))
    assert not t.clip_low.any() and not t.clip_high.any() and np.array_equal(t.member.sum(1), t.n)
    rc, mean, _, _, _ = oracle.stack_apply(capi.ST_MEAN, np.asarray(ref.make_frames(case)), ref.weights_of(case.frames),
                                           0.0, 0.0, ref.REF_LOC)
    assert rc == 0
    assert bits_equal(t.result, mean)


@pytest.mark.parametrize("mode", ref.MODES, ids=MODE_IDS.get)
@pytest.mark.parametrize("case", WITH_PADDED, ids=PADDED_IDS)
def test_c_equal_weights_give_the_oracles_weighted_result_within_rounding(oracle, case, mode):
    """Every weight 0.5: the products v * 0.5 are exact and den = m / 2 exactly in either order, so the checker (frame
    order) and the oracle (Hoare's order) sum the same m numbers in two orders.  Each sequential fp32 sum is off its
    exact value by at most (m - 1) 2^-24 sum|v| / 2, each division by 2^-24 of its quotient:
    |difference| <= 2 m 2^-24 mean|v| (the argument of tests/test_wlinfit_ref.py (c))."""
    half = np.full(case.frames, 0.5, F)
    frames = np.asarray(ref.make_frames(case))
    t = ref.truth(case, mode, weights=half)
    rc, want, _, _, _ = oracle.stack_apply(mode, frames, half, case.kappa, case.kappa, ref.REF_LOC)
    assert rc == 0
    m = t.member.sum(1)
    some = (m > 0) & ~t.inf
    mean_abs = np.where(t.member, np.abs(frames.T.astype(np.float64)), 0.0).sum(1)[some] / m[some]
    bound = 2.0 * m[some] * 2.0 ** -24 * mean_abs
    diff = np.abs(t.result[some].astype(np.float64) - want[some].astype(np.float64))
    assert np.all(np.isfinite(diff)) and np.all(diff <= bound)
    assert bits_equal(t.result[t.n == 0], want[t.n == 0])
    # (the bound was put to work: something was rejected)
    # (9 frames at sigma 3: plain sigma clipping can reject nothing there, see wclip_ref._kappa)
    assert case.frames < 5 or (case.frames == 9 and mode == ref.ST_SIGMA) or (m[some] < t.n[some]).any()
    if case is ref.ADVERSARIAL:
        # the pixel whose loop ends through len <= 1 is among the compared ones: K is what is left AFTER the last sweep
        # (the 1000 alone), not the three samples whose mean the unweighted modes return
        px = ref.LEN_LE_1_PIXEL
        assert some[px] and t.n[px] == 3 and m[px] == 1 and t.rounds[px] == 1
        assert t.result[px] == F(1000) and want[px] == F(1000)
        rc, plain, _, _, _ = oracle.stack_apply(mode, np.ascontiguousarray(frames[:, px:px + 1]), None, case.kappa, case.kappa, ref.REF_LOC)
        assert rc == 0 and abs(float(plain[0]) - 3001.0 / 3.0) < 1e-3


@pytest.mark.parametrize("mode", ref.MODES, ids=MODE_IDS.get)
def test_d_a_literal_pixel_is_seventeen_sevenths(oracle, mode):
    frames = np.array([1, 2, 3, 100], F).reshape(4, 1)
    t = ref.clip(frames, np.array([1, 2, 4, 8], F), mode, 2.0, 2.0)
    assert (int(t.clip_low[0]), int(t.clip_high[0])) == (0, 1)
    assert t.member[0].tolist() == [True, True, True, False]
    assert t.result[0] == F(17) / F(7)                  # (1 * 1 + 2 * 2 + 3 * 4) / (1 + 2 + 4): integers, one rounding
    assert t.result[0] != F(817) / F(15)                # ... and not with the 100 and its weight
    rc, _, cl, ch, _ = oracle.stack_apply(mode, frames, None, 2.0, 2.0, 0.0)
    assert rc == 0 and (cl, ch) == (0, 1)


@pytest.mark.parametrize("mode", ref.MODES, ids=MODE_IDS.get)
def test_e_equal_samples_share_their_fate(oracle, mode):
    """two 5s, seven 10s, two 15s: median 10, standard deviation 3.0; at sigma 1.5 the bounds lie between the groups,
    so both 5s go low, both 15s go high and every 10 stays, whatever order the samples are in"""
    v = [10, 15, 5, 10, 10, 5, 10, 15, 10, 10, 10]
    w = [3, 7, 1, 2, 5, 6, 4, 1, 2, 3, 7]
    frames = np.array(v, F).reshape(len(v), 1)
    t = ref.clip(frames, np.array(w, F), mode, 1.5, 1.5)
    assert (int(t.clip_low[0]), int(t.clip_high[0])) == (2, 2)
    assert t.member[0].tolist() == [x == 10 for x in v]
    num, den = sum(x * y for x, y in zip(v, w) if x == 10), sum(y for x, y in zip(v, w) if x == 10)
    assert t.result[0] == F(num) / F(den) == F(10)
    rc, _, cl, ch, _ = oracle.stack_apply(mode, frames, np.array(w, F), 1.5, 1.5, 0.0)
    assert rc == 0 and (cl, ch) == (2, 2)


def test_the_cases_are_what_the_issue_asks_for():
    assert [c.frames for c in ref.CASES] == [1, 2, 5, 8, 9, 16, 17, 24, 32, 33, 48, 64, 65, 100, 128, 129, 200, 512]
    for case in ref.CASES + [ref.PADDED]:
        p = case.width * case.height
        assert (case.width, case.height) == ((512, 512) if case is ref.PADDED else (61, 37))
        f = np.asarray(ref.make_frames(case))
        nan_share = np.isnan(f).mean(0)
        # under 2 % of the pixels miss more than a quarter of their samples.  (Not asserted for 1 and 2 frames, where it
        # cannot hold: a single NaN already is more than a quarter, and 1 % of the samples are NaN.)
        assert (nan_share > 0.25).mean() < 0.02 or case.frames <= 2, case.name
        assert not np.isinf(f).any()
    assert 61 * 37 % 4 and 61 * 37 % 64 and 61 * 37 % 256
    w = ref.weights_of(128)
    assert 3.5 < w.max() / w.min() <= 4.0
    assert ref.kernel_name(ref.BY_FRAMES[8], ref.ST_SIGMA) == "stack_exact_kernel<sigma,follow>"
    assert ref.kernel_name(ref.BY_FRAMES[9], ref.ST_WINSOR) == "stack_clip_weighted_kernel<1>"
    assert ref.kernel_name(ref.PADDED, ref.ST_SIGMA) == "stack_clip_weighted_kernel<4>"
