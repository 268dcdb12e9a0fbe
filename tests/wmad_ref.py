"""Checker of the weighted MAD-sigma pass whose weights follow their frames (include/nlstack_wmad.h): the header's
definition restated in numpy, fp32.

The pass is an extension -- the reference panics on MAD sigma with weights (stack.go:185) -- so there is no oracle for
its result.  The rejection IS the reference's StackMADSigma, though, and tests/test_wmad_ref.py holds this restatement to
the CPU oracle: its per-pixel counts to the oracle's unweighted MAD sigma, its result at a sigma that rejects nothing to
StackMeanWeighted bit for bit, and its result under equal weights to the oracle's MAD-sigma result within the rounding
of a reordered sum.

Both medians are order statistics, so a sort per pixel serves (no replay of Hoare's permutation); every array operation
below is ONE fp32 operation per pixel (numpy rounds float32 op float32 to float32).  The sum is a loop over the frames
with explicit float32 multiplies and adds.

A pixel whose median is not finite (definition, point 5): the deviations hold Inf - Inf, what the second median comes to
depends on the order the column kernel's selection leaves, and for sigmas >= 0 it does not matter -- it is Inf or NaN
either way and the bounds reject nothing.  The checker takes exactly that: K is every sample, both counts are 0; it
refuses negative sigmas on such pixels.

Inputs and cases are shared by the CPU self-check and the GPU tests; every truth is computed once per process and
returned read-only."""
import collections
import functools

import numpy as np

import wclip_ref

F = np.float32
KAPPA = 3.0
REF_LOC = 123.0
ST_MAD = 4
COLUMN_KERNEL = "stack_exact_kernel<mad,follow>"
WIDTH, HEIGHT = wclip_ref.WIDTH, wclip_ref.HEIGHT
weights_of = wclip_ref.weights_of

# what a pixel's pass leaves: result (the definition), the two counts, member[p, k] = frame k is in K, n = samples
# gathered, lo / hi = the bounds (NaN where the median is not finite), degenerate = the median is not finite
Mad = collections.namedtuple("Mad", "result clip_low clip_high member n lo hi degenerate")


def _median(s, n):
    """QSelectMedianFloat32 (qsort.go:68-82) of the first n entries of every sorted row of s: k = (n>>1)+1, the k-th
    smallest for odd n, 0.5f * ((k-1)-th + k-th) for even n.  Rows with n == 0: garbage."""
    rows = np.arange(s.shape[0])
    k = (n >> 1) + 1
    upper = s[rows, np.maximum(k - 1, 0)]
    lower = s[rows, np.maximum(k - 2, 0)]
    with np.errstate(all="ignore"):
        even = F(0.5) * (lower + upper)
    assert even.dtype == F
    return np.where((n & 1) == 0, even, upper).astype(F)


def mad_clip(frames, weights, sigma_low=KAPPA, sigma_high=KAPPA, ref_loc=REF_LOC):
    """frames [N, P] float32, weights [N] float32 -> Mad, arrays over the P pixels"""
    frames = np.ascontiguousarray(frames, F)
    w = np.ascontiguousarray(weights, F)
    N, P = frames.shape
    sl, sh = F(sigma_low), F(sigma_high)
    cols = np.ascontiguousarray(frames.T)                        # [P, N], frame order
    valid = ~np.isnan(cols)
    n = valid.sum(1)
    with np.errstate(all="ignore"):
        # (np.sort puts NaN last: the first n entries of a row are its samples, ascending)
        median = _median(np.sort(cols, axis=1), n)
        degenerate = (n > 0) & ~np.isfinite(median)
        d = cols - median[:, None]
        d = np.where(d < 0, -d, d)
        assert d.dtype == F
        mad = _median(np.sort(np.where(valid, d, F(np.nan)), axis=1), n)
        sd = mad * F(1.4826)
        t_lo, t_hi = sl * sd, sh * sd
        lo, hi = median - t_lo, median + t_hi                    # two roundings per bound
        assert lo.dtype == F and hi.dtype == F
        if degenerate.any():
            assert sigma_low >= 0 and sigma_high >= 0, "a pixel without a finite median: non-negative sigmas only"
            lo = np.where(degenerate, F(np.nan), lo)
            hi = np.where(degenerate, F(np.nan), hi)
        low = valid & (cols < lo[:, None])
        high = valid & ~low & (cols > hi[:, None])
        member = valid & ~low & ~high
        # StackMeanWeighted's arithmetic (stack.go:343-364) over K, in frame order
        num, den = np.zeros(P, F), np.zeros(P, F)
        for k in range(N):
            sel = member[:, k]
            num = np.where(sel, num + cols[:, k] * w[k], num)
            den = np.where(sel, den + w[k], den)
        assert num.dtype == F and den.dtype == F
        result = np.where(n > 0, num / den, F(ref_loc)).astype(F)
    out = Mad(result, low.sum(1), high.sum(1), member, n, lo, hi, degenerate)
    for a in out:
        a.setflags(write=False)
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------
# 61 x 37 = 2257 pixels: no multiple of 256, of 64 or of 4
Case = collections.namedtuple("Case", "name frames width height kappa")

# every count is a boundary in the code: network sizes (8, 16; 64 / 65: the bitonic merge of the deviations), the
# selection kernel from 114 frames, two lanes per pixel from 129, four from 257, the column kernel from 513
FRAME_COUNTS = (1, 2, 8, 9, 16, 17, 64, 65, 112, 113, 114, 127, 128, 129, 256, 257, 512, 513)
BITONIC_MIN = 114         # frames (and samples of a pixel) from which stack_mad_bitonic_kernel takes a stack (a pixel)
REGISTER_MAX, STREAM_MAX = 128, 512


def _case(n):
    return Case("mad-%dx%dx%d" % (n, WIDTH, HEIGHT), n, WIDTH, HEIGHT, KAPPA)


CASES = [_case(n) for n in FRAME_COUNTS]
BY_FRAMES = {c.frames: c for c in CASES}
C130, C200 = _case(130), _case(200)                       # active-frame walks; the padded stride
ADVERSARIAL = [Case("adversarial-%dx%dx%d" % (n, WIDTH, HEIGHT), n, WIDTH, HEIGHT, 1.0) for n in (24, 128, 200)]
ADVERSARIAL_SIGMAS = [(0.0, 0.0), (1.0, 1.0), (3.0, 0.5)]
# adversarial pixels: minority infinities (finite median), then medians +Inf, -Inf and NaN
PX_FEW_POS_INF, PX_FEW_NEG_INF, PX_MOST_POS_INF, PX_MOST_NEG_INF, PX_HALF_HALF = (5 * WIDTH + 3 + i for i in range(5))


def engine(n_active, exact=False):
    return "column" if exact or n_active > STREAM_MAX else "register" if n_active <= REGISTER_MAX else "streaming"


def kernel_name(n_active, vec=False, exact=False):
    """nl_stack_last_kernel_name of the pass over n_active frames.  vec: the frame stride is a multiple of 4 floats (the
    streaming kernel then takes four pixels per lane)"""
    e = engine(n_active, exact)
    if e == "column":
        return COLUMN_KERNEL
    if e == "streaming":
        return "stack_clip_weighted_kernel<%d, true>" % (4 if vec else 1)
    if n_active >= BITONIC_MIN:
        return "stack_mad_bitonic_kernel<true>"
    return "stack_mad_fast_kernel<%d, true>" % [c for c in (8, 16, 32, 48, 64, 80, 96, 112, 128) if c >= n_active][0]


def handed_over(t, n_active, exact=False):
    """the exact number of pixels the engine hands to the column kernel: the register engines those without a finite
    median, the streaming engine those and the pixels without a sample (no round on record); the column kernel none"""
    e = engine(n_active, exact)
    if e == "column":
        return 0
    return int((t.degenerate | (t.n == 0)).sum()) if e == "streaming" else int(t.degenerate.sum())


@functools.lru_cache(maxsize=None)
def make_frames(case):
    """[n, width * height] float32, read-only.  Generic cases: wclip_ref's generator -- 1000 + 20 N(0, 1), a few bright
    samples and one cold sample per pixel, 1 % NaN, 1.5 % of the pixels with a third of their samples NaN (odd and even
    n; n < 114 inside a stack of 114 frames or more), pixels without data, with one and with two samples.  The
    adversarial cases: integer samples 1000 + round(2.5 N(0, 1)) -- ties at the bounds --, pixels with a few infinite
    samples (finite median), with most samples +Inf, most -Inf, and half -Inf / half +Inf (median NaN)."""
    n, w, h = case.frames, case.width, case.height
    p = w * h
    adversarial = case.name.startswith("adversarial")
    rng = np.random.default_rng(7300 + 10 * n + (1 if adversarial else 0))
    if adversarial:
        f = (1000.0 + np.round(2.5 * rng.standard_normal((n, p)))).astype(F)
        f[rng.random((n, p)) < 0.01] = np.nan
        f[::7, PX_FEW_POS_INF] = F(np.inf)
        f[1::5, PX_FEW_NEG_INF] = F(-np.inf)
        f[: n // 2 + 2, PX_MOST_POS_INF] = F(np.inf)
        f[n // 3:, PX_MOST_NEG_INF] = F(-np.inf)
        f[:, PX_HALF_HALF] = np.where(np.arange(n) % 2 == 0, F(-np.inf), F(np.inf))        # n is even: median NaN
    else:
        f = (1000.0 + 20.0 * rng.standard_normal((n, p))).astype(F)
        share = 0.02 + 0.03 * rng.random(p)
        f[wclip_ref._at_most(rng.random((n, p)) < share[None, :], wclip_ref.MAX_BRIGHT)] += F(400.0)
        f[wclip_ref._at_most(rng.random((n, p)) < 0.005, 1)] -= F(300.0)
        f[wclip_ref._at_most(rng.random((n, p)) < 0.01, 1)] = np.nan
        holes = rng.random(p) < 0.015
        f[np.ix_(rng.random(n) < 0.34, holes)] = np.nan
    wclip_ref._special_pixels(f)
    f.setflags(write=False)
    return f


_truths = {}


def truth(case, n_active=None, sigmas=None, weights=None):
    """The Mad of `case` over its first n_active frames (default: all), computed once; weights default to weights_of"""
    key = (case, n_active, sigmas, None if weights is None else weights.tobytes())
    if key not in _truths:
        n = case.frames if n_active is None else n_active
        sl, sh = (case.kappa, case.kappa) if sigmas is None else sigmas
        _truths[key] = mad_clip(make_frames(case)[:n], weights_of(n) if weights is None else weights, sl, sh, REF_LOC)
    return _truths[key]
