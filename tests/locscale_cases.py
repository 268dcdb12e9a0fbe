"""The inputs of the location / scale tests (test_gpu_locscale.py) and what the restatement (locscale_ref.py) makes of
them, computed once per process.  test_locscale_ref.py asserts on the CPU that every case stays far inside the draw
budget of its bounded calls; the GPU tests compare the device with `expected` bit for bit."""
import functools

import numpy as np

import locscale_ref as ref

f32 = np.float32
OK, NAN, BUDGET, BIN = "ok", "nan", "budget", "bin"


def seeds_of(key, n=ref.MAX_SEEDS):
    return ref.splitmix_seeds(key, n)


# ---- frames --------------------------------------------------------------------------------------------------------

def sky(width, height, seed=1):
    """Gaussian sky (mean 1000, sigma 30) with 1 % bright outliers."""
    rng = np.random.default_rng(seed)
    n = width * height
    d = rng.normal(1000.0, 30.0, n)
    out = rng.random(n) < 0.01
    d[out] += rng.uniform(500.0, 20000.0, int(out.sum()))
    return d.astype(np.float32)


def ties(width, height, seed=2):
    """Many exactly tied values: the integers 0 .. 15."""
    return np.random.default_rng(seed).integers(0, 16, width * height).astype(np.float32)


def negative(width, height, seed=3):
    """Negative and positive values around -5, some of them -0.0 and +0.0 (never the selected rank of the median)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(-5.0, 20.0, width * height).astype(np.float32)
    d[::97] = f32(-0.0)
    d[1::193] = f32(0.0)
    return d


def constant(width, height):
    return np.full(width * height, 42.5, np.float32)


def nan_border(width, height, seed=4):
    """The sky with a NaN border of about 5 % of the pixels."""
    img = sky(width, height, seed).reshape(height, width)
    b = max(1, int(round(0.0127 * min(width, height))))
    img[:b] = img[-b:] = np.nan
    img[:, :b] = img[:, -b:] = np.nan
    return img.reshape(-1)


def nan_sparse(width, height, seed=9):
    """The sky with 0.3 % NaN pixels strewn over it: few enough that the unbounded calls of a small estimate can miss
    them all, enough that its bounded calls draw some."""
    rng = np.random.default_rng(seed)
    d = sky(width, height, seed)
    d[rng.random(d.size) < 0.003] = np.nan
    return d


def single_nan(width, height, seed=5):
    d = sky(width, height, seed)
    d[12345 % d.size] = np.nan
    return d


def core_and_plateau(width, height, seed=6):
    """55 % of the pixels in a tight core (sigma 1 around 1000), the rest spread evenly over [0, 60000): the bounds
    location +- 2 scale then hold little more than the core, so a bounded call needs a second round of the stream."""
    rng = np.random.default_rng(seed)
    n = width * height
    d = rng.normal(1000.0, 1.0, n)
    wide = rng.random(n) >= 0.55
    d[wide] = rng.uniform(0.0, 60000.0, int(wide.sum()))
    return d.astype(np.float32)


def spikes(width, height, seed=7):
    """45 % exactly 0, 45 % exactly 2, 10 % distinct values in (0.5, 1.5): the median is one of the distinct values,
    more than a quarter of the pair differences is 0, so the first scale is 0 and the bounds hold one pixel."""
    rng = np.random.default_rng(seed)
    n = width * height
    u = rng.random(n)
    d = np.where(u < 0.45, 0.0, 2.0)
    mid = u >= 0.9
    d[mid] = rng.permutation(int(mid.sum())) / float(mid.sum()) + 0.5
    return d.astype(np.float32)


def star_field(width, height, seed=8):
    """Sky (mean 1000, sigma 10) with forty Gaussian stars."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    img = 1000.0 + 10.0 * rng.standard_normal((height, width))
    for _ in range(40):
        x0, y0 = rng.uniform(8, width - 9), rng.uniform(8, height - 9)
        sigma = rng.uniform(1.0, 2.5)
        img += 10.0 ** rng.uniform(2.5, 4.0) * np.exp(-((xx - x0) ** 2 + (yy - y0) ** 2) / (2.0 * sigma * sigma))
    return img.astype(np.float32).reshape(-1)


FRAMES = {
    "sky37": (37, 29, lambda: sky(37, 29)),
    "sky256": (256, 256, lambda: sky(256, 256)),
    "sky1024": (1024, 1024, lambda: sky(1024, 1024, 11)),
    "ties37": (37, 29, lambda: ties(37, 29)),
    "ties256": (256, 256, lambda: ties(256, 256)),
    "negative256": (256, 256, lambda: negative(256, 256)),
    "constant37": (37, 29, lambda: constant(37, 29)),
    "nanborder256": (256, 256, lambda: nan_border(256, 256)),
    "singlenan256": (256, 256, lambda: single_nan(256, 256)),
    "nansparse256": (256, 256, lambda: nan_sparse(256, 256)),
    "plateau256": (256, 256, lambda: core_and_plateau(256, 256)),
    "spikes256": (256, 256, lambda: spikes(256, 256)),
    "stars256": (256, 256, lambda: star_field(256, 256)),
}


@functools.lru_cache(maxsize=None)
def frame(name):
    width, height, make = FRAMES[name]
    d = make()
    d.setflags(write=False)
    return width, height, d


# ---- cases: (frame, estimator, num_samples, seed key, min_max, outcome) -----------------------------------------------

E0, E1, E3, E4 = ref.LSE_MEAN_STDDEV, ref.LSE_MEDIAN_MAD, ref.LSE_SC_MEDIAN_QN, ref.LSE_HISTOGRAM


def _case(frame_name, estimator, num_samples=1000, key=1, min_max=None, outcome=OK):
    return (frame_name, estimator, num_samples, key, min_max, outcome)


# every estimator on the odd-sized and the 256 x 256 sky (on a slot, on the result, through the host form)
FORMS = [_case(f, e, 1000, 10 + e) for f in ("sky37", "sky256") for e in (E0, E1, E3, E4)]
# the sample counts: even, odd (another median branch, another quartile rank), 4096
COUNTS = [_case(f, e, s, 20 + s) for f in ("sky37", "ties256") for e in (E1, E3) for s in (1000, 1001, 4096)]
# the contents
CONTENTS = ([_case(f, e, 1000, 30 + e) for f in ("ties37", "negative256", "constant37") for e in (E0, E1, E3, E4)] +
            [_case("ties256", E4, 1000, 34), _case("sky1024", E0), _case("sky1024", E4)])
# the 1024 x 1024 frame with the reference's own sample count, once
FULL = _case("sky1024", E3, ref.NUM_SAMPLES, 40)
# a cached min / max that changes epsilon, hence the iteration count; epsilon 0 ends by i >= 10
WIDE_EPSILON = _case("sky256", E3, 4096, 50, (0.0, 6.5e6))
PLAIN_EPSILON = _case("sky256", E3, 4096, 50)
ZERO_EPSILON = _case("sky256", E3, 1000, 51, (0.0, 0.0))
# a bounded call that needs another round of the stream; the budget error
SECOND_ROUND = _case("plateau256", E3, 1000, 60)
OVER_BUDGET = _case("spikes256", E3, 1000, 61, None, BUDGET)
# NaN: sampled by an unbounded call; a histogram bin out of range (a NaN pixel, a stale min / max)
NAN_SAMPLED = [_case("nanborder256", E3, 1000, 70, None, NAN), _case("nanborder256", E1, 1000, 71, None, NAN)]
BAD_BIN = [_case("singlenan256", E4, 1000, 72, None, BIN), _case("sky256", E4, 1000, 73, (1000.0, 1100.0), BIN)]


# estimator 1 reads neither Min() nor Max(): a cached pair changes nothing and is not reported
MAD_IGNORES_MIN_MAX = _case("sky37", E1, 1000, 11, (1.0, 2.0))

# the estimate that feeds star detection and a tone curve
END_TO_END = _case("stars256", E3, 1000, 90)


NAN_FEW_SAMPLES = 64


def _quarter(info, num_samples):
    bounded = [(info["draws"][2 + 2 * i], info["draws"][3 + 2 * i]) for i in range(info["iterations"])]
    return all(m < ref.BUDGET_MEDIAN * num_samples // 4 and q < ref.BUDGET_QN * num_samples // 4 for m, q in bounded)


def _search(frame_name, num_samples, start, accept):
    """The first key from `start` on whose estimate accept(info, error kind or None, failing site or None) takes."""
    from oracle import oracle
    _, _, d = frame(frame_name)
    for key in range(start, start + 4000):
        try:
            info, kind, site = ref.location_scale(d, E3, oracle, seeds_of(key), num_samples)[2], None, None
        except ref.LocScaleError as e:
            info, kind, site = e.info, e.kind, str(e).split(":")[0]
        if accept(info, kind, site):
            return key
    raise AssertionError("no key in %d .. %d on %s" % (start, start + 4000, frame_name))


@functools.lru_cache(maxsize=None)
def nan_missed():
    """Estimator 3 on frames with NaN pixels, with seeds for which no sample of any call is NaN: the single NaN pixel at
    1000 samples, and the strewn NaN pixels at 64 samples with a key for which the bounded calls draw NaN pixels in
    every role -- the bounded median rejects one, the bounded Qn meets one as d1 (it passes :458; its pair is then
    dropped because d2 is out of bounds) and one as d2 (rejected at :462) -- far inside the budget."""
    def every_role(info, kind, site):
        n = info["nan_drawn"]
        return kind is None and n["median"] > 0 and n["first"] > 0 and n["second"] > 0 and _quarter(info, NAN_FEW_SAMPLES)
    return [_case("singlenan256", E3, 1000, _search("singlenan256", 1000, 80, lambda info, kind, site: kind is None)),
            _case("nansparse256", E3, NAN_FEW_SAMPLES, _search("nansparse256", NAN_FEW_SAMPLES, 300, every_role))]


@functools.lru_cache(maxsize=None)
def nan_from_bounded_qn():
    """... and a key for which the unbounded calls miss the NaN pixels but a bounded Qn keeps a pair whose d1 is NaN:
    the NaN error of a bounded call."""
    return _case("nansparse256", E3, NAN_FEW_SAMPLES,
                 _search("nansparse256", NAN_FEW_SAMPLES, 300,
                         lambda info, kind, site: kind == NAN and site == "FastApproxBoundedQn"), None, NAN)


def all_cases():
    return (FORMS + COUNTS + CONTENTS + [FULL, WIDE_EPSILON, PLAIN_EPSILON, ZERO_EPSILON, SECOND_ROUND, OVER_BUDGET,
             END_TO_END] +
            NAN_SAMPLED + BAD_BIN + nan_missed() + [nan_from_bounded_qn(), MAD_IGNORES_MIN_MAX])


def case_id(case):
    name, estimator, num_samples, key, min_max, outcome = case
    return "%s-e%d-s%d-k%d%s-%s" % (name, estimator, num_samples, key, "" if min_max is None else "-mm", outcome)


@functools.lru_cache(maxsize=None)
def expected(case):
    """The restatement on the case's frame: ("ok", location, scale, info) or (the kind of its LocScaleError,)."""
    return expected_on(case, None)


def expected_on(case, data):
    """... on `data` instead of the case's own frame (the result of a pass)"""
    from oracle import oracle
    name, estimator, num_samples, key, min_max, _ = case
    if data is None:
        data = frame(name)[2]
    try:
        loc, scale, info = ref.location_scale(data, estimator, oracle, seeds_of(key), num_samples, min_max)
    except ref.LocScaleError as e:
        return (e.kind,)
    return (OK, loc, scale, info)
