"""Location and scale on the device (nl_stack_frame_location_scale, nl_location_scale) against the restatement
(locscale_ref.py), bit for bit given the seeds: location, scale and every integer of nl_locscale_t.  The inputs and
what the restatement makes of them: locscale_cases.py (test_locscale_ref.py checks them on the CPU)."""
import numpy as np
import pytest

import locscale_cases as lc
import locscale_ref as ref

pytestmark = pytest.mark.gpu

f32 = np.float32
INTS = ("iterations", "converged", "seeds_used", "draws", "peak_bin", "peak_count", "half_width")


# estimator 0 against the sequential reference: both are fp32 roundings of fp64 sums that differ by the order of their
# terms only (about 1e-12 relative over a megapixel), so at most one fp32 ulp apart
ONE_ULP = 2.0 ** -23


def bits(v):
    return np.asarray(v, np.float32).view(np.uint32).tolist()


def check(got, want, what):
    """got: (location, scale, info) of the device; want: lc.expected's ("ok", location, scale, info)"""
    assert want[0] == lc.OK
    print(what, "device", got[0], got[1], "restatement", want[1], want[2])
    assert bits([got[0], got[1]]) == bits([want[1], want[2]]), (what, got[:2], want[1:3])
    for name in INTS:
        assert got[2][name] == want[3][name], (what, name, got[2][name], want[3][name])
    assert bits([got[2]["min"], got[2]["max"], got[2]["epsilon"]]) == bits([want[3]["min"], want[3]["max"], want[3]["epsilon"]])


def run_slot(nl, case, st=None, idx=0):
    name, estimator, num_samples, key, min_max, _ = case
    width, height, d = lc.frame(name)
    if st is not None:
        return st.frame_location_scale(idx, estimator, lc.seeds_of(key), num_samples, min_max)
    with nl.StackHandle(1, width, height) as own:
        own.upload_frame(0, d)
        return own.frame_location_scale(0, estimator, lc.seeds_of(key), num_samples, min_max)


def expect_mean_stddev(st, idx, got):
    """Estimator 0 is the existing reductions: the bits nl_stack_frame_stats gives on the same pixels."""
    mn, mean, mx, var = st.frame_stats(idx)
    assert bits([got[0], got[1]]) == bits([mean, f32(np.sqrt(var))])
    assert bits([got[2]["min"], got[2]["max"]]) == bits([mn, mx])
    assert got[2]["seeds_used"] == 0 and got[2]["iterations"] == 0


@pytest.mark.parametrize("case", lc.FORMS, ids=lc.case_id)
def test_every_estimator_on_a_slot_on_the_result_and_through_the_host_form(nl, oracle, case):
    name, estimator, num_samples, key, min_max, _ = case
    width, height, d = lc.frame(name)
    seeds = lc.seeds_of(key)
    other = (d * f32(0.5)).astype(np.float32)
    with nl.StackHandle(2, width, height) as st:
        st.upload_frames([other, d])
        got = st.frame_location_scale(1, estimator, seeds, num_samples, min_max)
        if estimator == ref.LSE_MEAN_STDDEV:
            expect_mean_stddev(st, 1, got)
        else:
            check(got, lc.expected(case), "slot")
        # the last pass's result: the mean of the two slots, whatever its bits are
        result, _, _ = st.run(nl.ST_MEAN)
        got = st.frame_location_scale(-1, estimator, seeds, num_samples, min_max)
        if estimator == ref.LSE_MEAN_STDDEV:
            want = ref.location_scale(result, estimator, oracle)
            assert bits([got[2]["min"], got[2]["max"]]) == bits([want[2]["min"], want[2]["max"]])
            assert abs(float(got[0]) - float(want[0])) <= ONE_ULP * abs(float(want[0]))
            assert abs(float(got[1]) - float(want[1])) <= ONE_ULP * abs(float(want[1]))
        else:
            check(got, lc.expected_on(case, result), "result")
    got = nl.location_scale(d, width, height, estimator, seeds, num_samples, min_max)
    if estimator == ref.LSE_MEAN_STDDEV:
        want = lc.expected(case)
        assert bits([got[2]["min"], got[2]["max"]]) == bits([want[3]["min"], want[3]["max"]])
        assert abs(float(got[0]) - float(want[1])) <= ONE_ULP * abs(float(want[1]))
        assert abs(float(got[1]) - float(want[2])) <= ONE_ULP * abs(float(want[2]))
    else:
        check(got, lc.expected(case), "host form")


def test_result_form_needs_a_pass(nl):
    from nightlight_amd import capi
    width, height, d = lc.frame("sky37")
    with nl.StackHandle(1, width, height) as st:
        st.upload_frame(0, d)
        with pytest.raises(capi.NlError) as e:
            st.frame_location_scale(-1, ref.LSE_HISTOGRAM)
        assert e.value.code == capi.ERR_INVALID_ARG and "has not run a pass" in e.value.message


@pytest.mark.parametrize("case", lc.COUNTS + lc.CONTENTS, ids=lc.case_id)
def test_sample_counts_and_contents(nl, case):
    name, estimator = case[0], case[1]
    width, height, d = lc.frame(name)
    with nl.StackHandle(1, width, height) as st:
        st.upload_frame(0, d)
        got = run_slot(nl, case, st)
        if estimator == ref.LSE_MEAN_STDDEV:
            expect_mean_stddev(st, 0, got)
            if name.startswith(("ties", "constant")):           # sums of small integers are exact in any order
                check(got, lc.expected(case), "slot")
        else:
            check(got, lc.expected(case), "slot")


def test_reference_sample_count_on_a_megapixel_frame(nl):
    """NL_LOCSCALE_SAMPLES, once: the restatement's literal loops take seconds at this size."""
    assert lc.FULL[2] == nl.LOCSCALE_SAMPLES == 131072
    check(run_slot(nl, lc.FULL), lc.expected(lc.FULL), "slot")


def test_cached_min_max_changes_epsilon_and_the_iterations(nl):
    width, height, d = lc.frame(lc.WIDE_EPSILON[0])
    with nl.StackHandle(1, width, height) as st:
        st.upload_frame(0, d)
        wide, plain = run_slot(nl, lc.WIDE_EPSILON, st), run_slot(nl, lc.PLAIN_EPSILON, st)
        check(wide, lc.expected(lc.WIDE_EPSILON), "cached min / max")
        check(plain, lc.expected(lc.PLAIN_EPSILON), "the frame's min / max")
        assert wide[2]["iterations"] < plain[2]["iterations"]
        zero = run_slot(nl, lc.ZERO_EPSILON, st)
        check(zero, lc.expected(lc.ZERO_EPSILON), "epsilon 0")
        assert (zero[2]["iterations"], zero[2]["converged"]) == (11, 0)       # ended by i >= 10


def test_bounded_call_that_needs_another_round_of_the_stream(nl):
    got = run_slot(nl, lc.SECOND_ROUND)
    check(got, lc.expected(lc.SECOND_ROUND), "second round")
    s = lc.SECOND_ROUND[2]
    assert got[2]["draws"][2] > s + s // 4 + 64 and got[2]["draws"][3] > 2 * s + s // 2 + 64


def test_draw_budget_is_an_error_and_the_handle_stays_usable(nl):
    from nightlight_amd import capi
    assert lc.expected(lc.OVER_BUDGET) == (lc.BUDGET,)
    name, estimator, num_samples, key, _, _ = lc.OVER_BUDGET
    width, height, d = lc.frame(name)
    good = lc._case("sky256", ref.LSE_SC_MEDIAN_QN, 1000, 13)
    with nl.StackHandle(2, width, height) as st:
        st.upload_frames([d, lc.frame("sky256")[2]])
        with pytest.raises(capi.NlError) as e:
            st.frame_location_scale(0, estimator, lc.seeds_of(key), num_samples)
        assert e.value.code == capi.ERR_INVALID_ARG
        assert "FastApproxBoundedMedian" in e.value.message and "fewer than 1 in 16 draws within [" in e.value.message
        check(run_slot(nl, good, st, 1), lc.expected(good), "after the budget error")


@pytest.mark.parametrize("case", lc.NAN_SAMPLED + lc.BAD_BIN, ids=lc.case_id)
def test_nan_samples_and_bad_bins_are_errors(nl, case):
    from nightlight_amd import capi
    assert lc.expected(case) == (case[5],)
    with pytest.raises(capi.NlError) as e:
        run_slot(nl, case)
    assert e.value.code == capi.ERR_INVALID_ARG
    if case[5] == lc.NAN:
        assert "NaN among the samples" in e.value.message and "FastApproxMedian" in e.value.message
    else:
        assert "HistogramScaleLoc" in e.value.message and "outside [0, 4096)" in e.value.message


def test_nan_pixels_that_no_unbounded_call_samples(nl):
    """The bounded calls draw NaN pixels in every role (test_locscale_ref.py asserts so) and no sample is NaN; with
    another key a bounded Qn keeps a pair whose d1 is NaN, which is the NaN error of that call."""
    from nightlight_amd import capi
    for case in lc.nan_missed():
        check(run_slot(nl, case), lc.expected(case), lc.case_id(case))
    with pytest.raises(capi.NlError) as e:
        run_slot(nl, lc.nan_from_bounded_qn())
    assert e.value.code == capi.ERR_INVALID_ARG
    assert "FastApproxBoundedQn" in e.value.message and "NaN among the samples" in e.value.message


def test_estimator_1_ignores_a_cached_min_max(nl):
    got = run_slot(nl, lc.MAD_IGNORES_MIN_MAX)
    check(got, lc.expected(lc.MAD_IGNORES_MIN_MAX), "median / MAD with min_max")
    assert (got[2]["min"], got[2]["max"]) == (0, 0)


def test_row_tiles_and_tiny_frames_are_errors(nl):
    from nightlight_amd import capi
    width, height, d = lc.frame("sky37")
    with nl.StackHandle(1, width, height, row0=4, rows=8) as st:
        st.upload_frame(0, d)
        with pytest.raises(capi.NlError) as e:
            st.frame_location_scale(0, ref.LSE_HISTOGRAM)
        assert e.value.code == capi.ERR_INVALID_ARG and "whole-image handle" in e.value.message
    with pytest.raises(capi.NlError) as e:
        nl.location_scale(np.ones(1, np.float32), 1, 1, ref.LSE_MEDIAN_MAD, lc.seeds_of(1), 4)
    assert e.value.code == capi.ERR_INVALID_ARG and "1 pixels" in e.value.message


def test_estimate_feeds_star_detection_and_a_tone_curve(nl):
    """End to end on a resident frame: the device's estimate handed to FindStars and to a tone curve gives what the
    restatement's location and scale give."""
    case = lc.END_TO_END
    width, height, d = lc.frame(case[0])
    _, want_loc, want_scale, _ = lc.expected(case)
    outs = []
    for source in ("device", "restatement"):
        with nl.StackHandle(1, width, height) as st:
            st.upload_frame(0, d)
            if source == "device":
                loc, scale, _ = run_slot(nl, case, st)
            else:
                loc, scale = want_loc, want_scale
            stars, shifts, hfr = st.frame_find_stars(0, loc, scale, bp_sigma=0.0)
            st.frame_tone(0, nl.TONE_SHIFT_BLACK, loc, f32(0.1) * scale)
            outs.append((stars, bits([shifts]), st.download_tile(0)))
    assert len(outs[0][0]) > 0
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1] == outs[1][1]
    assert np.array_equal(outs[0][2].view(np.uint32), outs[1][2].view(np.uint32))
