"""Checker of the weighted linear-fit pass (include/nlstack_wlinfit.h): the header's definition restated in numpy, fp32.

The pass is an extension -- the reference's StackLinearFit takes no weights -- so there is no oracle for its result.
The rejection loop IS the reference's, though: tests/test_wlinfit_ref.py holds this restatement's counters and its
unweighted ymean to the CPU oracle's StackLinearFit bit for bit on every case, its result at a sigma that rejects
nothing to the oracle's StackMeanWeighted, and the frames it keeps to hand-computed pixels.

Vectorised over the pixels: every array operation below is ONE fp32 operation per pixel (numpy rounds float32 op
float32 to float32), the loops run over the sorted positions, so each pixel's sums are sequential in the reference's
order.  A dead position adds +0, as skipping it does (an accumulator that starts at +0 never becomes -0).  The square
root is taken in fp64 and then cast (stats.go:259).

Inputs and cases are shared by the CPU self-check and the GPU tests; every truth is computed once per process and
returned read-only."""
import collections
import functools

import numpy as np

F = np.float32
KAPPA = 2.75
REF_LOC = 123.0
K_RUNS = 4                # runs of survivors the register engine takes (kWlfRuns, stack_linfit_weighted.hip)
REGISTER_CLASSES = (8, 16, 32, 48, 64, 96, 128)
COLUMN_KERNEL = "stack_exact_kernel<linfit,weighted>"

# what a pixel's fit leaves: result (the definition), ymean (what the unweighted reference returns), the two counters,
# member[p, k] = frame k is in K, runs = maximal runs of live sorted positions in S, and why the register engine hands
# the pixel over (too_many runs, a tie group split by a run's end, a +-Inf sample); handover = any of the three
Fit = collections.namedtuple("Fit", "result ymean clip_low clip_high member runs too_many split inf handover n")


@functools.lru_cache(maxsize=None)
def _xstat(n_max):
    """MeanStdDev of xs = 0 .. m-1 (stats.go:246-261) for m = 0 .. n_max, sequential fp32"""
    mean, sd = np.zeros(n_max + 1, F), np.zeros(n_max + 1, F)
    for m in range(1, n_max + 1):
        s = F(0)
        for i in range(m):
            s = F(s + F(i))
        mu = F(s / F(m))
        v = F(0)
        for i in range(m):
            d = F(F(i) - mu)
            v = F(v + F(d * d))
        mean[m], sd[m] = mu, F(np.sqrt(np.float64(F(v / F(m)))))
    return mean, sd


def fit(frames, weights, sigma_low=KAPPA, sigma_high=KAPPA, ref_loc=REF_LOC):
    """frames [N, P] float32, weights [N] float32 -> Fit, arrays over the P pixels"""
    frames = np.ascontiguousarray(frames, F)
    w = np.ascontiguousarray(weights, F)
    N, P = frames.shape
    sl, sh = F(sigma_low), F(sigma_high)
    cols = np.ascontiguousarray(frames.T)                        # [P, N]
    valid = ~np.isnan(cols)
    n = valid.sum(1)
    # (value ascending, frame index ascending); +0 == -0; NaN behind everything, +Inf included
    order = np.argsort(cols, axis=1, kind="stable")
    v = np.take_along_axis(cols, order, axis=1)
    pos = np.arange(N)[None, :]
    live = pos < n[:, None]
    xmean, xsd_t = _xstat(N)
    active = n > 0
    S = live.copy()
    ymean = np.full(P, F(ref_loc), F)
    c_lo, c_hi = np.zeros(P, np.int64), np.zeros(P, np.int64)
    zero = F(0)
    with np.errstate(all="ignore"):
        while active.any():
            m = live.sum(1)
            fm = m.astype(F)
            xm, xsd = xmean[np.maximum(m, 1)], xsd_t[np.maximum(m, 1)]
            s = np.zeros(P, F)
            for k in range(N):
                s = s + np.where(live[:, k], v[:, k], zero)
            ym = s / fm
            vs, corr, fi = np.zeros(P, F), np.zeros(P, F), np.zeros(P, F)
            for k in range(N):
                lk = live[:, k]
                dy = v[:, k] - ym
                vs = vs + np.where(lk, dy * dy, zero)
                corr = corr + np.where(lk, (fi - xm) * dy, zero)
                fi = fi + lk.astype(F)
            ysd = np.sqrt((vs / fm).astype(np.float64)).astype(F)
            den = (xsd * ysd) * (fm + F(1))
            corr = corr / den
            slope = (corr * ysd) / xsd
            icpt = ym - slope * xm
            sg, fi = np.zeros(P, F), np.zeros(P, F)
            for k in range(N):
                lk = live[:, k]
                lin = fi * slope + icpt
                sg = sg + np.where(lk, np.abs(v[:, k] - lin), zero)
                fi = fi + lk.astype(F)
            sg = sg / fm
            lb, hb = sl * sg, sh * sg
            fi = np.zeros(P, F)
            low, high = np.zeros((P, N), bool), np.zeros((P, N), bool)
            for k in range(N):
                lk = live[:, k]
                lin = fi * slope + icpt
                low[:, k] = lk & ((lin - v[:, k]) > lb)
                high[:, k] = lk & ~low[:, k] & ((v[:, k] - lin) > hb)
                fi = fi + lk.astype(F)
            for a in (s, ym, vs, corr, ysd, den, slope, icpt, sg, lb, hb):
                assert a.dtype == F
            n_lo, n_hi = low.sum(1), high.sum(1)
            c_lo += np.where(active, n_lo, 0)
            c_hi += np.where(active, n_hi, 0)
            done = active & ((n_lo + n_hi == 0) | (m < 3))
            S[done] = live[done]                                 # the positions of the LAST regression
            ymean[done] = ym[done]
            go_on = active & ~done
            live[go_on] &= ~(low[go_on] | high[go_on])
            active = go_on
    # K: the frames at the positions of S
    member = np.zeros((P, N), bool)
    np.put_along_axis(member, order, S, axis=1)
    member &= (n > 0)[:, None]
    num, den = np.zeros(P, F), np.zeros(P, F)
    with np.errstate(all="ignore"):
        for k in range(N):
            sel = member[:, k]
            num = np.where(sel, num + cols[:, k] * w[k], num)
            den = np.where(sel, den + w[k], den)
        assert num.dtype == F and den.dtype == F
        result = np.where(n > 0, num / den, F(ref_loc)).astype(F)
    Sn = S & (n > 0)[:, None]
    before = np.concatenate([np.zeros((P, 1), bool), Sn[:, :-1]], axis=1)
    after = np.concatenate([Sn[:, 1:], np.zeros((P, 1), bool)], axis=1)
    first, last = Sn & ~before, Sn & ~after
    runs = first.sum(1)
    same_below = np.concatenate([np.zeros((P, 1), bool), v[:, 1:] == v[:, :-1]], axis=1)           # v[k-1] == v[k]
    same_above = np.concatenate([(v[:, 1:] == v[:, :-1]) & (pos[:, 1:] < n[:, None]), np.zeros((P, 1), bool)], axis=1)
    split = ((first & same_below) | (last & same_above)).any(1)
    too_many = runs > K_RUNS
    inf = (np.isinf(cols) & valid).any(1)
    out = Fit(result, ymean, c_lo, c_hi, member, runs, too_many, split, inf, too_many | split | inf, n)
    for a in out:
        a.setflags(write=False)
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------
# 41 x 23 = 943 pixels: three full 256-thread workgroups and a partial one, no multiple of 64; the deep stacks 23 x 13 = 299
Case = collections.namedtuple("Case", "name frames width height engine kappa")


def _case(n, engine):
    w, h = (41, 23) if n < 96 else (23, 13)
    return Case("%s-%dx%dx%d" % (engine, n, w, h), n, w, h, engine, KAPPA)


CASES = [_case(n, "register") for n in (1, 2, 3, 7, 24, 33, 64, 65, 96, 128)] + [_case(n, "column") for n in (129, 200)]
ADVERSARIAL = Case("adversarial-24x41x23", 24, 41, 23, "register", 1.0)
BY_FRAMES = {c.frames: c for c in CASES}


def kernel_name(case, n_active=None):
    n = case.frames if n_active is None else n_active
    if case.engine == "column":
        return COLUMN_KERNEL
    return "stack_linfit_weighted_kernel<%d>" % [c for c in REGISTER_CLASSES if c >= n][0]


def weights_of(n):
    """1 / (1 + 4 s_k) of distinct per-frame scalars s_k in [0.1, 1.0]: what inverse-noise weighting makes of noises"""
    s = F(0.1) + F(0.9) * ((np.arange(n) * 37 % 211).astype(F) / F(210))
    assert np.unique(s).size == n
    return (F(1) / (F(1) + F(4) * s)).astype(F)


def _special_pixels(f):
    """per-frame NaN borders, one pixel without data, pixels with one and with two samples"""
    n, h, w = f.shape
    for k in range(n):
        f[k, :k % 3, :] = np.nan                       # 0 .. 2 rows at the top
        if k * 5 % 4:
            f[k, :, w - k * 5 % 4:] = np.nan           # 0 .. 3 columns on the right
    flat = f.reshape(n, h * w)
    p = h * w
    flat[:, p // 2] = np.nan                           # no data
    flat[:, p // 2 + 7] = np.nan                       # a single sample
    flat[n // 2, p // 2 + 7] = F(987.5)
    if n >= 2:
        flat[:, p // 2 + 9] = np.nan                   # two samples
        flat[0, p // 2 + 9] = F(1001.5)
        flat[n - 1, p // 2 + 9] = F(1010.25)


# A pixel whose last regression runs over FIVE runs of sorted positions, found by a search on the CPU.  At sigma 1 a fit
# ends with nothing left to reject only when all residuals are equal in magnitude; 965, 977, 999, 1001, 1023, 1035 are
# built so (1000 + 12 (r - 2.5) +- 5: the slope the reference computes for them, 6/7 of the exact one, leaves +-5
# everywhere), the other 18 samples were drawn until they die around those six without touching them.
FIVE_RUNS = [921, 996, 947, 1093, 999, 976, 1050, 1035, 1083, 965, 1006, 990, 1023, 1012, 1007, 1003, 1036, 1006, 1034, 944,
             977, 1001, 973, 989]


@functools.lru_cache(maxsize=None)
def make_frames(case):
    """[n, width * height] float32, read-only.  Generic cases: 1000 + 20 N(0, 1), 3 % of the samples + 400 (bright
    outliers), 3 % NaN.  The adversarial case: integer-valued samples 1000 + round(2.5 N(0, 1)) -- groups of equal
    samples everywhere -- and a few pixels with a +Inf or a -Inf sample."""
    n, w, h = case.frames, case.width, case.height
    rng = np.random.default_rng(7000 + 10 * n + (1 if case is ADVERSARIAL else 0))
    p = w * h
    if case is ADVERSARIAL:
        f = (1000.0 + np.round(2.5 * rng.standard_normal((n, p)))).astype(F)
    else:
        f = (1000.0 + 20.0 * rng.standard_normal((n, p))).astype(F)
        f[rng.random((n, p)) < 0.03] += F(400.0)
    f[rng.random((n, p)) < 0.03] = np.nan
    _special_pixels(f.reshape(n, h, w))
    if case is ADVERSARIAL:
        for i, px in enumerate(range(5 * w + 3, 5 * w + 11)):
            f[(3 * i) % n, px] = F(np.inf) if i % 2 == 0 else F(-np.inf)
        f[:, 7 * w + 5] = np.array(FIVE_RUNS, F)
    f.setflags(write=False)
    return f


_truths = {}


def truth(case, n_active=None, kappa=None, weights=None):
    """The Fit of `case` over its first n_active frames (default: all), computed once; weights default to weights_of"""
    key = (case, n_active, kappa, None if weights is None else weights.tobytes())
    if key not in _truths:
        n = case.frames if n_active is None else n_active
        k = case.kappa if kappa is None else kappa
        frames = make_frames(case)[:n]
        _truths[key] = fit(frames, weights_of(n) if weights is None else weights, k, k, REF_LOC)
    return _truths[key]
