"""CPU restatement of Stats.Location() / Scale(): updateLocationScale (internal/stats/stats.go:225-244) with
FastApproxMedian (:336-345), FastApproxBoundedMedian (:349-364), FastApproxMAD (:401-410), FastApproxQn (:436-447),
FastApproxBoundedQn (:450-472), FastApproxSigmaClippedMedianAndQn (:477-499) and HistogramScaleLoc (:640-688), in
fp32 throughout, and of the generator behind them, valyala/fastrand v1.1.0: xorshift32 (13, 17, 5) with
Uint32n(m) = uint32(uint64(x) * uint64(m) >> 32), from a seed the caller passes where the reference takes one from the
clock (one fresh RNG, hence one seed, per sampling call).

Every select goes through the oracle's literal C QSelect*.  The sampling loops run literally, one draw at a time; the
fp32 arithmetic on what they gathered is numpy's.  Beside the results it returns what nl_locscale_t reports.  Where the
reference panics or computes on NaN samples, LocScaleError("nan" / "bin" / ...) is raised; the one deviation of the
library is restated too: a bounded call gives up with LocScaleError("budget") after 16 (median) or 32 (Qn) times
num_samples draws, where the reference would go on drawing."""
import numpy as np

f32 = np.float32

LSE_MEAN_STDDEV, LSE_MEDIAN_MAD, LSE_IKSS, LSE_SC_MEDIAN_QN, LSE_HISTOGRAM = range(5)
NUM_SAMPLES = 128 * 1024            # :226
MAX_SEEDS = 25
NUM_BINS = 4096                     # :241
BUDGET_MEDIAN, BUDGET_QN = 16, 32   # times num_samples


class LocScaleError(Exception):
    def __init__(self, kind, message):
        Exception.__init__(self, message)
        self.kind = kind


class RNG:
    """fastrand.RNG with its state set to `seed` (nonzero: a zero state is replaced from the clock)."""

    def __init__(self, seed):
        assert 0 < int(seed) < 2 ** 32
        self.x = int(seed)
        self.draws = 0

    def uint32(self):
        x = self.x
        x ^= (x << 13) & 0xffffffff
        x ^= x >> 17
        x ^= (x << 5) & 0xffffffff
        self.x = x
        self.draws += 1
        return x

    def uint32n(self, m):
        return (self.uint32() * int(m)) >> 32


def splitmix_seeds(key, n):
    """nl_locscale_seeds: the high halves of splitmix64's outputs from `key`, zeros skipped."""
    mask = 2 ** 64 - 1
    x = int(key) & mask
    out = []
    while len(out) < n:
        x = (x + 0x9e3779b97f4a7c15) & mask
        z = x
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & mask
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & mask
        z ^= z >> 31
        if z >> 32:
            out.append(z >> 32)
    return np.array(out, np.uint32)


def _select_median(samples, oracle, site):
    samples = np.asarray(samples, np.float32)
    if np.isnan(samples).any():
        raise LocScaleError("nan", "%s: NaN among the samples (QSelectFloat32 requires NaN-free input)" % site)
    return f32(oracle.qselect_median(samples)[0])


def _select_first_quartile(samples, oracle, site):
    samples = np.asarray(samples, np.float32)
    if np.isnan(samples).any():
        raise LocScaleError("nan", "%s: NaN among the samples (QSelectFloat32 requires NaN-free input)" % site)
    return f32(oracle.qselect(samples, (samples.size >> 2) + 1)[0])       # qsort.go:61-63


def _abs_diff(a, b):
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(a, np.float32) - np.asarray(b, np.float32))


def fast_approx_median(data, num_samples, seed, oracle):
    """:336-345 -> (median, draws)"""
    rng = RNG(seed)
    n = len(data)
    samples = [data[rng.uint32n(n)] for _ in range(num_samples)]
    return _select_median(samples, oracle, "FastApproxMedian"), rng.draws


def fast_approx_mad(data, location, num_samples, seed, oracle):
    """:401-410 -> (mad, draws)"""
    rng = RNG(seed)
    n = len(data)
    samples = _abs_diff([data[rng.uint32n(n)] for _ in range(num_samples)], f32(location))
    return f32(_select_median(samples, oracle, "FastApproxMAD") * f32(1.4826)), rng.draws


def fast_approx_qn(data, num_samples, seed, oracle):
    """:436-447 -> (qn, draws)"""
    rng = RNG(seed)
    n = len(data)
    d1, d2 = [], []
    for _ in range(num_samples):
        index1 = 1 + rng.uint32n(n - 1)
        index2 = rng.uint32n(index1)
        d1.append(data[index1])
        d2.append(data[index2])
    samples = _abs_diff(d1, d2)
    return f32(_select_first_quartile(samples, oracle, "FastApproxQn") * f32(2.21914)), rng.draws


def fast_approx_bounded_median(data, low, high, num_samples, seed, oracle, nan_drawn=None):
    """:349-364 -> (median, draws); nan_drawn (a dict) counts the NaN pixels the call drew, as "median" """
    rng = RNG(seed)
    n = len(data)
    budget = BUDGET_MEDIAN * num_samples
    samples = []
    for _ in range(num_samples):
        while True:
            if rng.draws >= budget:
                raise LocScaleError("budget", "FastApproxBoundedMedian: fewer than 1 in 16 draws within [%r, %r]" % (low, high))
            d = data[rng.uint32n(n)]
            if d != d and nan_drawn is not None:
                nan_drawn["median"] += 1
            if d >= low and d <= high:
                break
        samples.append(d)
    return _select_median(samples, oracle, "FastApproxBoundedMedian"), rng.draws


def fast_approx_bounded_qn(data, low, high, num_samples, seed, oracle, nan_drawn=None):
    """:450-472 -> (qn, draws); nan_drawn (a dict) counts the NaN pixels the call drew: "first" as d1 (they pass :458),
    "second" as d2 (rejected at :462)"""
    rng = RNG(seed)
    n = len(data)
    budget = BUDGET_QN * num_samples
    s1, s2 = [], []
    for _ in range(num_samples):
        while True:
            if rng.draws >= budget:
                raise LocScaleError("budget", "FastApproxBoundedQn: fewer than 1 in 16 draws within [%r, %r]" % (low, high))
            index1 = 1 + rng.uint32n(n - 1)
            d1 = data[index1]
            if d1 != d1 and nan_drawn is not None:
                nan_drawn["first"] += 1
            if d1 < low or d1 > high:
                continue
            if rng.draws >= budget:
                raise LocScaleError("budget", "FastApproxBoundedQn: fewer than 1 in 16 draws within [%r, %r]" % (low, high))
            d2 = data[rng.uint32n(index1)]
            if d2 != d2 and nan_drawn is not None:
                nan_drawn["second"] += 1
            if d2 >= low and d2 <= high:
                break
        s1.append(d1)
        s2.append(d2)
    samples = _abs_diff(s1, s2)
    return f32(_select_first_quartile(samples, oracle, "FastApproxBoundedQn") * f32(2.21914)), rng.draws


def min_max(data):
    """calcMinMeanMaxPureGo's min and max (:264-277): a comparison with NaN is false."""
    data = np.asarray(data, np.float32).reshape(-1)
    if np.isnan(data[0]):
        return f32(np.nan), f32(np.nan)
    return f32(np.fmin.reduce(data)), f32(np.fmax.reduce(data))


def sigma_clipped_median_and_qn(data, sigma_low, sigma_high, epsilon, num_samples, seeds, oracle, info):
    """:477-499 -> (location, scale); info gains iterations, converged, seeds_used, draws"""
    draws = info["draws"]
    sigma_low, epsilon = f32(sigma_low), f32(epsilon)

    nan_drawn = info.setdefault("nan_drawn", dict(median=0, first=0, second=0))

    def call(fn, *args, **kw):
        k = info["seeds_used"]
        value, used = fn(*args, num_samples, int(seeds[k]), oracle, **kw)
        draws[k] = used
        info["seeds_used"] = k + 1
        return value

    location = call(fast_approx_median, data)
    scale = call(fast_approx_qn, data)
    i = 0
    while True:
        with np.errstate(all="ignore"):
            low = f32(location - f32(sigma_low * scale))
            high = f32(location + f32(sigma_low * scale))      # (sigmaLow on both sides, :483-484)
        new_location = call(fast_approx_bounded_median, data, float(low), float(high), nan_drawn=nan_drawn)
        new_scale = f32(call(fast_approx_bounded_qn, data, float(low), float(high), nan_drawn=nan_drawn) * f32(1.134))
        info["iterations"] = i + 1
        with np.errstate(all="ignore"):
            delta = f32(abs(float(f32(new_location - location))) + abs(float(f32(new_scale - scale))))
        converged = bool(delta <= epsilon)
        if converged or i >= 10:
            info["converged"] = 1 if converged else 0
            scale = call(fast_approx_qn, data)
            return location, scale
        location, scale = new_location, new_scale
        i += 1


def go_uint32(v):
    """uint32(float32) on amd64 (CVTTSS2SQ, then the low 32 bits); None where the index that follows panics."""
    v = f32(v)
    if not (v > f32(-1.0) and v < f32(NUM_BINS)):
        return None
    return int(v)


def histogram_scale_loc(data, mn, mx, info, num_bins=NUM_BINS):
    """:640-688 -> (loc, scale); info gains peak_bin, peak_count, half_width"""
    data = np.asarray(data, np.float32).reshape(-1)
    mn, mx = f32(mn), f32(mx)
    if mn == mx:
        return mn, f32(0)
    with np.errstate(all="ignore"):
        value_to_bin = f32(f32(num_bins - 1) / f32(mx - mn))
        t = (data - mn) * value_to_bin + f32(0.5)
    assert t.dtype == np.float32
    if not np.all((t > f32(-1.0)) & (t < f32(num_bins))):
        raise LocScaleError("bin", "HistogramScaleLoc: index out of range [0, %d)" % num_bins)
    bins = np.bincount(t.astype(np.int64), minlength=num_bins)
    peak_bin, peak_count = 0, 0
    for b in range(1, num_bins - 1):
        if bins[b] > peak_count:
            peak_bin, peak_count = b, int(bins[b])
    loc = f32(mn + f32(f32(peak_bin) / value_to_bin))
    sigma_threshold = int(f32(f32(data.size) * f32(0.6827)))
    interval_limit = min(peak_bin, num_bins - 1 - peak_bin)
    cum = peak_count
    scale = f32(f32(0.5) * f32(1.0) / value_to_bin)
    reached = 0
    if cum < sigma_threshold:
        for i in range(1, interval_limit + 1):
            cum = cum + int(bins[peak_bin - i]) + int(bins[peak_bin + i])
            scale = f32(f32(f32(0.5) * f32(2 * i + 1)) / value_to_bin)
            reached = i
            if cum >= sigma_threshold:
                break
    info.update(peak_bin=peak_bin, peak_count=peak_count, half_width=reached)
    return loc, scale


def location_scale(data, estimator, oracle, seeds=None, num_samples=NUM_SAMPLES, min_max_cached=None):
    """updateLocationScale (:225-244) with LSEstimator = estimator -> (location, scale, info): info as nl_locscale_t."""
    arr = np.ascontiguousarray(data, np.float32).reshape(-1)
    info = dict(iterations=0, converged=0, seeds_used=0, draws=[0] * MAX_SEEDS, min=f32(0), max=f32(0), epsilon=f32(0),
                peak_bin=0, peak_count=0, half_width=0)
    if estimator == LSE_MEAN_STDDEV:
        info["min"], mean, info["max"] = oracle.min_mean_max(arr)
        return f32(mean), f32(np.sqrt(oracle.variance(arr, mean))), info
    if estimator != LSE_MEDIAN_MAD:
        info["min"], info["max"] = min_max(arr) if min_max_cached is None else (f32(min_max_cached[0]), f32(min_max_cached[1]))
    if estimator == LSE_HISTOGRAM:
        loc, scale = histogram_scale_loc(arr, info["min"], info["max"], info)
        return loc, scale, info
    values = arr.tolist()               # exact: every fp32 is an fp64, and the compares agree
    if estimator == LSE_MEDIAN_MAD:
        loc, info["draws"][0] = fast_approx_median(values, num_samples, int(seeds[0]), oracle)
        info["seeds_used"] = 1
        scale, info["draws"][1] = fast_approx_mad(values, loc, num_samples, int(seeds[1]), oracle)
        info["seeds_used"] = 2
        return loc, scale, info
    assert estimator == LSE_SC_MEDIAN_QN
    with np.errstate(all="ignore"):
        info["epsilon"] = f32(f32(info["max"] - info["min"]) / f32(65535.0))
    try:
        loc, scale = sigma_clipped_median_and_qn(values, 2, 2, info["epsilon"], num_samples, seeds, oracle, info)
    except LocScaleError as e:
        e.info = info                   # what had happened up to the failing call
        raise
    return loc, scale, info
