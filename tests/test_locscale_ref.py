"""CPU checks of the location / scale restatement (locscale_ref.py) that the GPU tests compare against, of the inputs
those tests use (locscale_cases.py), and of what the library's entries decide without a device."""
import ctypes as C

import numpy as np
import pytest

import locscale_cases as lc
import locscale_ref as ref

f32 = np.float32

# eight pixels and bounds [9, 13] that leave out pixels 2 and 6
HAND = [10.0, 12.0, 50.0, 11.0, 9.5, 13.0, -40.0, 10.5]
HAND_SEED = 2463534242


def test_xorshift_known_answers():
    rng = ref.RNG(1)
    assert [rng.uint32() for _ in range(5)] == [270369, 67634689, 2647435461, 307599695, 2398689233]
    rng = ref.RNG(1)
    assert [rng.uint32n(1073) for _ in range(5)] == [0, 16, 661, 76, 599]
    assert rng.draws == 5


def test_hand_trace_unbounded_qn(oracle):
    # Uint32n(7) of the draws of HAND_SEED: 1 4 3 3 5 0 2 1 ...; pairs (i1, i2) = (2, 1) (4, 1) (6, 0) (3, 0):
    # |50 - 12|, |9.5 - 12|, |-40 - 10|, |11 - 10| = 38, 2.5, 50, 1; rank (4 >> 2) + 1 = 2 is 2.5
    qn, draws = ref.fast_approx_qn(HAND, 4, HAND_SEED, oracle)
    assert draws == 8
    assert qn == f32(f32(2.5) * f32(2.21914))


def test_hand_trace_bounded_qn_with_both_rejections(oracle):
    # draw 0: i1 = 2 (50) fails the first test.  draws 1, 2: i1 = 5 (13), i2 = 2 (50) fails the second test.
    # draws 3, 4: (4, 3) |9.5 - 11| = 1.5.  draws 5, 6: (1, 0) |12 - 10| = 2.  draws 7, 8: i1 = 2, twice.
    # draws 9, 10: (5, 1) |13 - 12| = 1.  draw 11: i1 = 6 (-40).  draws 12, 13: (5, 4) |13 - 9.5| = 3.5.
    # rank 2 of {1.5, 2, 1, 3.5} is 1.5
    qn, draws = ref.fast_approx_bounded_qn(HAND, 9.0, 13.0, 4, HAND_SEED, oracle)
    assert draws == 14
    assert qn == f32(f32(1.5) * f32(2.21914))


def test_hand_trace_medians(oracle):
    # Uint32n(8) of the first draws: 1 4 3 3: 12, 9.5, 11, 11; the median of an even count is 0.5 * (11 + 11)
    rng = ref.RNG(HAND_SEED)
    assert [rng.uint32n(8) for _ in range(4)] == [1, 4, 3, 3]
    assert ref.fast_approx_median(HAND, 4, HAND_SEED, oracle) == (f32(11.0), 4)
    assert ref.fast_approx_bounded_median(HAND, 9.0, 13.0, 4, HAND_SEED, oracle) == (f32(11.0), 4)
    # MAD around 10: |12 - 10|, |9.5 - 10|, 1, 1 -> 0.5 * (1 + 1) * 1.4826
    assert ref.fast_approx_mad(HAND, 10.0, 4, HAND_SEED, oracle) == (f32(f32(1.0) * f32(1.4826)), 4)


def test_bounded_calls_give_up_at_the_budget(oracle):
    with pytest.raises(ref.LocScaleError) as e:
        ref.fast_approx_bounded_median(HAND, 100.0, 200.0, 4, 1, oracle)
    assert e.value.kind == "budget"
    with pytest.raises(ref.LocScaleError) as e:
        ref.fast_approx_bounded_qn(HAND, float("nan"), float("nan"), 4, 1, oracle)
    assert e.value.kind == "budget"


def test_histogram_constant_frame(oracle):
    loc, scale, info = ref.location_scale(np.full(100, 3.25, np.float32), ref.LSE_HISTOGRAM, oracle)
    assert (loc, scale) == (f32(3.25), f32(0)) and info["peak_count"] == 0


def test_histogram_two_spikes(oracle):
    # min 0, max 4095: valueToBin 1, bin = value.  600 pixels at 1000, 398 at 1200; the threshold is
    # uint32(1000 * 0.6827) = 682, reached when the interval takes in bin 1200 at i = 200
    d = np.array([0.0, 4095.0] + [1000.0] * 600 + [1200.0] * 398, np.float32)
    loc, scale, info = ref.location_scale(d, ref.LSE_HISTOGRAM, oracle)
    assert (info["peak_bin"], info["peak_count"], info["half_width"]) == (1000, 600, 200)
    assert (loc, scale) == (f32(1000.0), f32(200.5))


def test_histogram_stops_at_the_interval_limit(oracle):
    # the peak at bin 3 holds 400 of 1000 pixels, the rest lies far away: the cumulation runs i = 1 .. 3 = peakBin
    # and ends below the threshold with scale 0.5 * 7
    d = np.array([0.0, 4095.0] + [3.0] * 400 + [2000.0] * 299 + [3000.0] * 299, np.float32)
    loc, scale, info = ref.location_scale(d, ref.LSE_HISTOGRAM, oracle)
    assert (info["peak_bin"], info["peak_count"], info["half_width"]) == (3, 400, 3)
    assert (loc, scale) == (f32(3.0), f32(3.5))


def test_histogram_bin_out_of_range(oracle):
    d = np.array([0.0, 1.0, np.nan, 2.0], np.float32)
    with pytest.raises(ref.LocScaleError) as e:
        ref.location_scale(d, ref.LSE_HISTOGRAM, oracle, min_max_cached=(0.0, 2.0))
    assert e.value.kind == "bin"


def test_estimator_3_recovers_a_gaussian_sky(oracle):
    """The restatement, not the device: mean 1000, sigma 30, 1 % bright outliers, 4096 samples, ten seeds."""
    d = lc.sky(256, 256, seed=99)
    for key in range(10):
        loc, scale, info = ref.location_scale(d, ref.LSE_SC_MEDIAN_QN, oracle, lc.seeds_of(1000 + key), 4096)
        assert abs(float(loc) - 1000.0) <= 3.0, (key, loc)
        assert abs(float(scale) - 30.0) <= 0.15 * 30.0, (key, scale)
        assert 1 <= info["iterations"] <= 11 and info["seeds_used"] == 3 + 2 * info["iterations"]


@pytest.mark.parametrize("case", lc.all_cases(), ids=lc.case_id)
def test_gpu_inputs_stay_far_inside_the_draw_budget(case):
    """Every input of the GPU tests: the outcome the case names, and each bounded call under a quarter of its budget
    (16 x num_samples draws for the median, 32 x for Qn) -- but for the one case that is there to exceed it."""
    _, estimator, num_samples, _, _, outcome = case
    got = lc.expected(case)
    assert got[0] == outcome
    if outcome != lc.OK or estimator != ref.LSE_SC_MEDIAN_QN:
        return
    info = got[3]
    assert info["seeds_used"] == 3 + 2 * info["iterations"]
    for i in range(info["iterations"]):
        assert num_samples <= info["draws"][2 + 2 * i] < ref.BUDGET_MEDIAN * num_samples // 4, (i, info["draws"])
        assert 2 * num_samples <= info["draws"][3 + 2 * i] < ref.BUDGET_QN * num_samples // 4, (i, info["draws"])


def test_gpu_inputs_take_the_paths_they_are_there_for(oracle):
    wide, plain, zero = lc.expected(lc.WIDE_EPSILON)[3], lc.expected(lc.PLAIN_EPSILON)[3], lc.expected(lc.ZERO_EPSILON)[3]
    assert wide["epsilon"] > plain["epsilon"] and wide["iterations"] < plain["iterations"]
    assert (zero["epsilon"], zero["iterations"], zero["converged"]) == (f32(0), 11, 0)
    # a second round: more draws than the first round of 1.25 S (median) or 2.5 S (Qn) holds
    second = lc.expected(lc.SECOND_ROUND)[3]
    s = lc.SECOND_ROUND[2]
    assert second["draws"][2] > s + s // 4 + 64 and second["draws"][3] > 2 * s + s // 2 + 64
    const = lc.expected(lc._case("constant37", ref.LSE_SC_MEDIAN_QN, 1000, 33))
    assert const[1:3] == (f32(42.5), f32(0)) and (const[3]["iterations"], const[3]["converged"]) == (1, 1)
    # the frames with NaN pixels whose samples hold none: the bounded calls drew NaN pixels all the same, at 64 samples
    # in every role (rejected by the median; as d1, which passes stats.go:458; as d2, rejected at :462)
    one, few = (lc.expected(c)[3]["nan_drawn"] for c in lc.nan_missed())
    assert one["median"] + one["first"] + one["second"] > 0
    assert few["median"] > 0 and few["first"] > 0 and few["second"] > 0 and lc.nan_missed()[1][2] == 64
    # ... and the key for which a bounded Qn keeps a pair whose d1 is NaN
    with pytest.raises(ref.LocScaleError) as e:
        name, estimator, num_samples, key, _, _ = lc.nan_from_bounded_qn()
        ref.location_scale(lc.frame(name)[2], estimator, oracle, lc.seeds_of(key), num_samples)
    assert e.value.kind == "nan" and str(e.value).startswith("FastApproxBoundedQn:") and e.value.info["nan_drawn"]["first"] > 0
    mad = lc.expected(lc.MAD_IGNORES_MIN_MAX)
    assert mad[1:3] == lc.expected(lc._case("sky37", ref.LSE_MEDIAN_MAD, 1000, 11))[1:3] and (mad[3]["min"], mad[3]["max"]) == (0, 0)


# ---- what the library decides without a device ---------------------------------------------------------------------

def _host_call(estimator, num_samples, seeds, n_seeds=None):
    from nightlight_amd import capi
    lib = capi.load()
    frame = np.ones(64, np.float32)
    seeds = np.ascontiguousarray(seeds, np.uint32)
    loc, scale = C.c_float(), C.c_float()
    rc = lib.nl_location_scale(capi.fptr(frame), 8, 8, estimator, num_samples,
                               seeds.ctypes.data_as(C.POINTER(C.c_uint32)), seeds.size if n_seeds is None else n_seeds,
                               None, C.byref(loc), C.byref(scale), None, 0)
    return rc, capi.last_error()


def test_argument_errors_need_no_device():
    from nightlight_amd import capi
    good = lc.seeds_of(1)
    rc, msg = _host_call(capi.LSE_IKSS, 1000, good)
    assert rc == capi.ERR_INVALID_ARG and "LSEIKSS" in msg and "not implemented on the device" in msg
    rc, msg = _host_call(capi.LSE_SC_MEDIAN_QN, 3, good)
    assert rc == capi.ERR_INVALID_ARG and "3 samples" in msg
    rc, msg = _host_call(capi.LSE_SC_MEDIAN_QN, 1000, good[:24])
    assert rc == capi.ERR_INVALID_ARG and "24 seeds" in msg
    rc, msg = _host_call(capi.LSE_MEDIAN_MAD, 1000, good[:1])
    assert rc == capi.ERR_INVALID_ARG and "1 seeds" in msg
    zero = good.copy()
    zero[7] = 0
    rc, msg = _host_call(capi.LSE_SC_MEDIAN_QN, 1000, zero)
    assert rc == capi.ERR_INVALID_ARG and "seed 7 is zero" in msg
    rc, msg = _host_call(5, 1000, good)
    assert rc == capi.ERR_INVALID_ARG and "unknown estimator 5" in msg


def test_locscale_seeds_are_deterministic_and_nonzero():
    import nightlight_amd as nl
    a, b = nl.locscale_seeds(12345), nl.locscale_seeds(12345)
    assert a.dtype == np.uint32 and a.size == nl.LOCSCALE_MAX_SEEDS and np.array_equal(a, b)
    assert not np.array_equal(a, nl.locscale_seeds(12346))
    for key in (0, 1, 2 ** 64 - 1, 0x9e3779b97f4a7c15):
        got = nl.locscale_seeds(key, 1000)
        assert np.all(got != 0) and np.array_equal(got, ref.splitmix_seeds(key, 1000))
    assert nl.locscale_seeds(7, 0).size == 0
