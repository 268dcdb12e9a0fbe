"""Checker of the weighted clip pass whose weights follow their frames (include/nlstack_wclip.h): the header's definition
restated in numpy, fp32.

The pass is an extension -- the reference multiplies a survivor by whichever weight Hoare's permutation left in its slot
-- so there is no oracle for its result.  The rejection loop IS the reference's, though, and tests/test_wclip_ref.py
holds this restatement to the CPU oracle: its per-pixel counts to StackSigma / StackWinsorSigma (unweighted and
weighted), its result at a sigma that rejects nothing to StackMeanWeighted bit for bit, and its result under equal
weights to the oracle's weighted modes within the rounding of a reordered sum.

Vectorised over the pixels: every array operation below is ONE fp32 operation per pixel (numpy rounds float32 op float32
to float32).  MeanStdDev (stats.go:246-261) sums in the order QSelectMedianFloat32 and the clip swaps left the samples in,
and a clip decision can hinge on the last bit of that sum, so the restatement keeps every pixel's samples in the
reference's order: Hoare's partition (qsort.go:94-126) and the swap-with-last sweep (stack.go:411-424) run in lockstep
over the pixels, one pointer move per step.  The square root is taken in fp64 and then cast (stats.go:259).

Which FRAMES survive is then a matter of values alone (the definition, step 2): every round's bounds are applied to the
frames in frame order, and the result is StackMeanWeighted's arithmetic over the frames still in.

Inputs and cases are shared by the CPU self-check and the GPU tests; every truth is computed once per process and
returned read-only."""
import collections
import functools

import numpy as np

F = np.float32
KAPPA = 3.0
REF_LOC = 123.0
ST_SIGMA, ST_WINSOR = 2, 3
BOUND_ROUNDS = 8          # rounds of thresholds the decision pass records per pixel (kBoundRounds, stack_kernels.h)
COLUMN_MAX = 8            # frames up to which the column kernel takes the whole tile (no zonal kernel below 9)
COLUMN_KERNEL = {ST_SIGMA: "stack_exact_kernel<sigma,follow>", ST_WINSOR: "stack_exact_kernel<winsor,follow>"}

# what a pixel's pass leaves: result (the definition), the two counts, member[p, k] = frame k is in K, n = samples
# gathered, rounds = removal sweeps run, inf = the pixel has an infinite sample, must_hand_over = the streaming engine
# cannot have a complete record for it (no sample; more rounds than the record holds; truth() adds zone_overflow)
Clip = collections.namedtuple("Clip", "result clip_low clip_high member n rounds inf must_hand_over")


def _hoare_select(g, m, k, on):
    """QSelectFloat32 (qsort.go:94-126) on the rows `on` of g [P, N] with lengths m and 1-based ranks k, in place and in
    lockstep: returns the selected values (rows that are off: garbage)"""
    P = g.shape[0]
    rows = np.arange(P)
    left = np.zeros(P, np.int64)
    right = np.where(on, m - 1, 0)
    k = k.copy()
    outer = on & (left < right)
    while outer.any():
        pivot = g[rows, (left + right) >> 1]
        l, r = left - 1, right + 1
        part = outer.copy()
        while part.any():
            scan = part.copy()
            while scan.any():
                l = np.where(scan, l + 1, l)
                scan &= ~(g[rows, np.maximum(l, 0)] >= pivot)
            scan = part.copy()
            while scan.any():
                r = np.where(scan, r - 1, r)
                scan &= ~(g[rows, np.maximum(r, 0)] <= pivot)
            part &= l < r
            i = np.nonzero(part)[0]
            a, b = g[i, l[i]].copy(), g[i, r[i]].copy()
            g[i, l[i]], g[i, r[i]] = b, a
        offset = r - left + 1
        lower = outer & (k <= offset)
        upper = outer & ~lower
        right = np.where(lower, r, right)
        left = np.where(upper, r + 1, left)
        k = np.where(upper, k - offset, k)
        outer = on & (left < right)
    return g[rows, left]


def _select_median(g, m, on):
    """QSelectMedianFloat32 (qsort.go:68-82)"""
    k = (m >> 1) + 1
    upper = _hoare_select(g, m, k, on)
    pos = np.arange(g.shape[1])[None, :]
    with np.errstate(all="ignore"):
        lower = np.where(pos < (k - 1)[:, None], g, F(-np.inf)).max(1)          # (a maximum rounds nothing)
        even = F(0.5) * (lower + upper)
    return np.where((m & 1) == 0, even, upper).astype(F)


def _mean_stddev(x, m):
    """MeanStdDev (stats.go:246-261) of the first m entries of every row of x, sequential fp32"""
    P, N = x.shape
    fm = m.astype(F)
    s = np.zeros(P, F)
    for i in range(int(m.max(initial=0))):
        s = np.where(i < m, s + x[:, i], s)
    mean = s / fm
    v = np.zeros(P, F)
    for i in range(int(m.max(initial=0))):
        d = x[:, i] - mean
        v = np.where(i < m, v + d * d, v)
    v = v / fm
    assert s.dtype == F and mean.dtype == F and v.dtype == F
    return mean, np.sqrt(v.astype(np.float64)).astype(F)


def _winsorized_stddev(g, m, median, sd):
    """stack.go:646-672: clamp a copy to median -/+ 1.5 sd, sd = 1.134 * stddev(copy), until nothing moved or sd
    changed by at most 0.05 %.  (Only the pixels still in the loop are carried along.)"""
    out = sd.copy()
    ids = np.arange(g.shape[0])
    wz, m, median, sd = g.copy(), m, median, sd
    pos = np.arange(g.shape[1])[None, :]
    while ids.size:
        live = pos < m[:, None]
        t = F(1.5) * sd
        lo, hi = median - t, median + t
        below = live & (wz < lo[:, None])
        above = live & ~below & (wz > hi[:, None])
        wz = np.where(below, lo[:, None], np.where(above, hi[:, None], wz))
        changed = below.sum(1) + above.sum(1)
        _, new = _mean_stddev(wz, m)
        new = F(1.134) * new
        factor = np.abs(new - sd) / sd
        assert new.dtype == F and factor.dtype == F
        out[ids] = new
        go = ~((changed == 0) | (factor <= F(0.0005)))
        ids, wz, m, median, sd = ids[go], wz[go], m[go], median[go], new[go]
    return out


def _clip_sweep(g, m, lo, hi, on):
    """stack.go:411-424, the swap-with-last sweep, in lockstep: returns the new lengths and the two counts"""
    P = g.shape[0]
    rows = np.arange(P)
    m = m.copy()
    j = np.zeros(P, np.int64)
    n_lo, n_hi = np.zeros(P, np.int64), np.zeros(P, np.int64)
    go = on & (j < m)
    while go.any():
        x = g[rows, np.minimum(j, g.shape[1] - 1)]
        low = go & (x < lo)
        high = go & ~low & (x > hi)
        out = low | high
        m = np.where(out, m - 1, m)
        i = np.nonzero(out)[0]
        g[i, j[i]] = g[i, m[i]]
        n_lo += low
        n_hi += high
        j = np.where(go & ~out, j + 1, j)
        go = on & (j < m)
    return m, n_lo, n_hi


def clip(frames, weights, mode, sigma_low=KAPPA, sigma_high=KAPPA, ref_loc=REF_LOC):
    """frames [N, P] float32, weights [N] float32, mode ST_SIGMA / ST_WINSOR -> Clip, arrays over the P pixels"""
    assert mode in (ST_SIGMA, ST_WINSOR)
    frames = np.ascontiguousarray(frames, F)
    w = np.ascontiguousarray(weights, F)
    N, P = frames.shape
    sl, sh = F(sigma_low), F(sigma_high)
    cols = np.ascontiguousarray(frames.T)                        # [P, N], frame order
    valid = ~np.isnan(cols)
    n = valid.sum(1)
    # gather (stack.go:380-387): frame order, NaN dropped
    order = np.argsort(~valid, axis=1, kind="stable")
    g = np.take_along_axis(cols, order, axis=1)
    member = valid.copy()
    c_lo, c_hi = np.zeros(P, np.int64), np.zeros(P, np.int64)
    rounds = np.zeros(P, np.int64)
    # (only the pixels whose loop is still running are carried along: ids names them)
    ids = np.nonzero(n > 0)[0]
    g, m, colsa, memb = g[ids], n[ids], cols[ids], valid[ids]
    with np.errstate(all="ignore"):
        while ids.size:
            on = np.ones(ids.size, bool)
            median = _select_median(g, m, on)
            _, sd = _mean_stddev(g, m)
            if mode == ST_WINSOR:
                sd = _winsorized_stddev(g, m, median, sd)
            lo, hi = median - sl * sd, median + sh * sd
            assert lo.dtype == F and hi.dtype == F
            m_new, n_lo, n_hi = _clip_sweep(g, m, lo, hi, on)
            # the same predicates on the frames, in frame order: equal samples share their fate
            f_lo = memb & (colsa < lo[:, None])
            f_hi = memb & ~f_lo & (colsa > hi[:, None])
            assert np.array_equal(f_lo.sum(1), n_lo) and np.array_equal(f_hi.sum(1), n_hi)
            memb &= ~(f_lo | f_hi)
            assert np.array_equal(memb.sum(1), m_new)
            c_lo[ids] += n_lo
            c_hi[ids] += n_hi
            rounds[ids] += 1
            member[ids] = memb
            go = ~((m_new == m) | (m_new <= 1))
            ids, g, m, colsa, memb = ids[go], g[go], m_new[go], colsa[go], memb[go]
        # StackMeanWeighted's arithmetic (stack.go:343-364) over K, in frame order
        num, den = np.zeros(P, F), np.zeros(P, F)
        for k in range(N):
            sel = member[:, k]
            num = np.where(sel, num + cols[:, k] * w[k], num)
            den = np.where(sel, den + w[k], den)
        assert num.dtype == F and den.dtype == F
        result = np.where(n > 0, num / den, F(ref_loc)).astype(F)
    inf = (np.isinf(cols) & valid).any(1)
    out = Clip(result, c_lo, c_hi, member, n, rounds, inf, (n == 0) | (rounds > BOUND_ROUNDS))
    for a in out:
        a.setflags(write=False)
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------
# 61 x 37 = 2257 pixels: no multiple of 256, of 64 or of 4.  One more case, 24 frames of 512 x 512, has the padded stride
# (and with it 16-byte loads: four pixels per lane).
Case = collections.namedtuple("Case", "name frames width height engine kappa")
WIDTH, HEIGHT = 61, 37


def _engine(n):
    return "column" if n <= COLUMN_MAX else "shallow" if n <= 32 else "register" if n <= 128 else "lds-column"


def _kappa(n):
    """No sample of n lies further than (n - 1) / sqrt(n) standard deviations from the mean, so a sigma of 3 rejects
    nothing in plain sigma clipping up to 10 frames: the column kernel's cases (up to 8 frames) run at 1.5.  The 9-frame
    case stays at 3 -- winsorized clipping rejects in half of its pixels there -- and NINE_SIGMA runs plain sigma at 2.5."""
    return 1.5 if n <= COLUMN_MAX else KAPPA


def _case(n, w=WIDTH, h=HEIGHT):
    return Case("%s-%dx%dx%d" % (_engine(n), n, w, h), n, w, h, _engine(n), _kappa(n))


FRAME_COUNTS = (1, 2, 5, 8, 9, 16, 17, 24, 32, 33, 48, 64, 65, 100, 128, 129, 200, 512)
CASES = [_case(n) for n in FRAME_COUNTS]
PADDED = _case(24, 512, 512)
# 9 frames, plain sigma at 2.5: the padded 16-position decision kernel under rejection (a sample goes in a third of the
# pixels).  Sigma only: its zones hold 4 positions a side, 2 of the low ones padding, and winsorized clipping at 2.5
# would overflow them in 9 % of the pixels before a single undecidable one.
NINE_SIGMA = Case("shallow-9x61x37-sigma2.5", 9, WIDTH, HEIGHT, "shallow", 2.5)
ADVERSARIAL = Case("adversarial-24x61x37", 24, WIDTH, HEIGHT, "shallow", 1.0)
BY_FRAMES = {c.frames: c for c in CASES}
MODES = (ST_SIGMA, ST_WINSOR)
LEN_LE_1_PIXEL = 11 * WIDTH + 4          # adversarial case: the loop ends through len <= 1


def kernel_name(case, mode, n_active=None, vec=None):
    """nl_stack_last_kernel_name of the pass: the column kernel up to 8 frames, else the streaming kernel -- four pixels
    per lane where the frame stride is a multiple of 4 floats (the padded stride of large tiles), else one"""
    n = case.frames if n_active is None else n_active
    if n <= COLUMN_MAX:
        return COLUMN_KERNEL[mode]
    if vec is None:
        vec = case.width * case.height >= (1 << 18)
    return "stack_clip_weighted_kernel<%d>" % (4 if vec else 1)


def weights_of(n):
    """noise-like weights spread over a factor of 4: 1 / (1 + 3 s_k) of distinct per-frame scalars s_k in [0, 1]"""
    s = ((np.arange(n) * 37 % 521).astype(F) / F(520))
    assert np.unique(s).size == n
    return (F(1) / (F(1) + F(3) * s)).astype(F)


def _special_pixels(flat):
    """fixed pixels without data, with one and with two samples"""
    n, p = flat.shape
    flat[:, p // 2] = np.nan                           # no data
    flat[:, p // 2 + 7] = np.nan                       # a single sample
    flat[n // 2, p // 2 + 7] = F(987.5)
    if n >= 2:
        flat[:, p // 2 + 9] = np.nan                   # two samples
        flat[0, p // 2 + 9] = F(1001.5)
        flat[n - 1, p // 2 + 9] = F(1010.25)


# Outliers per pixel: a property of the cases.  The decision kernels keep what may be clipped in ZONES of sorted positions
# -- 8 a side from the 48-position network on, 4 below -- and a stack just above a network size (17, 33, 65, 100 frames)
# has only 3 or 4 samples in its high zone; a pixel that clips as many on one side as its zone holds has no round on
# record and goes to the column kernel (zone_overflow below predicts which).  The cases are to exercise the streaming
# engine, so a pixel has at most MAX_BRIGHT bright samples, one cold sample and one NaN -- a pixel crossed by two trails
# --, drawn at 2 - 5 % (0.5 %, 1 %) per sample.  Up to 40 frames that is 2 - 5 % bright samples per pixel; from 128 frames
# on the cap makes it less (2 of 128 = 1.6 %, 2 of 512 = 0.4 %).  Beside these, 1.5 % of the pixels miss a third of their
# samples: those are meant to go to the column kernel.
MAX_BRIGHT = 2


def _at_most(mask, most):
    """mask [n, p] with at most `most` True per pixel: the first ones in frame order stay"""
    return mask & (np.cumsum(mask, axis=0) <= most)


def zone_overflow(case, mode, t, n_active=None):
    """Pixels of a 9 ... 128-frame stack that the register-resident decision kernel cannot keep in its zones
    (stack_fast_sigma_impl.hpp: zone widths KZ / KP, lo_pads of the padding at the bottom): no sample, too few samples
    to reach the high zone, or as many clips on one side as its zone holds.  They have no round on record."""
    n_fr = case.frames if n_active is None else n_active
    if not COLUMN_MAX < n_fr <= 128:
        return np.zeros(t.n.size, bool)
    ns = [c for c in (16, 24, 32, 48, 64, 80, 96, 112, 128) if c >= n_fr][0]
    tight = ns == n_fr
    kz = 8 if ns >= 48 else 4
    kp = 0 if tight else kz
    zl, zh = kz, ns - kz - kp
    lo_pads = 0 if tight else min(max(kz // 2 + 1 - (n_fr - zh), 0), kz // 2 if kz == 4 else kz // 2 - 1)
    b = lo_pads + t.n
    return (t.n == 0) | ~(b > zh) | (lo_pads + t.clip_low >= zl) | (b - t.clip_high <= zh)


@functools.lru_cache(maxsize=None)
def make_frames(case):
    """[n, width * height] float32, read-only.  Generic cases: 1000 + 20 N(0, 1); per pixel 2 - 5 % of the samples + 400
    (bright outliers, at most MAX_BRIGHT of them), 0.5 % - 300 (cold ones, at most one); 1 % NaN (at most one), and 1.5 %
    of the pixels with a third of their samples NaN.  The adversarial case: integer-valued samples 1000 + round(2.5 N(0, 1)) -- groups of
    equal samples on both sides of every bound --, pixels with a +Inf or a -Inf sample, one pixel that ends through
    len <= 1; it is run at sigma 1 and with negative sigmas (ADVERSARIAL_SIGMAS)."""
    n, w, h = case.frames, case.width, case.height
    p = w * h
    rng = np.random.default_rng(9100 + 10 * n + (1 if case is ADVERSARIAL else 0) + (2 if p > 4096 else 0))
    if case is ADVERSARIAL:
        f = (1000.0 + np.round(2.5 * rng.standard_normal((n, p)))).astype(F)
        f[rng.random((n, p)) < 0.01] = np.nan
        for i, px in enumerate(range(5 * w + 3, 5 * w + 11)):
            f[(3 * i) % n, px] = F(np.inf) if i % 2 == 0 else F(-np.inf)
        # 990, 1000, 1011: median 1000, standard deviation 8.58 about the mean 1000.33 -- at sigma 1 the first sweep
        # removes 990 and 1011 and the loop ends through len <= 1.  K is the 1000 alone; the mean BEFORE that sweep, which
        # the unweighted modes return, is 1000.33
        f[:, LEN_LE_1_PIXEL] = np.nan
        f[3, LEN_LE_1_PIXEL], f[9, LEN_LE_1_PIXEL], f[17, LEN_LE_1_PIXEL] = F(990.0), F(1000.0), F(1011.0)
    else:
        f = (1000.0 + 20.0 * rng.standard_normal((n, p))).astype(F)
        share = 0.02 + 0.03 * rng.random(p)
        f[_at_most(rng.random((n, p)) < share[None, :], MAX_BRIGHT)] += F(400.0)
        f[_at_most(rng.random((n, p)) < 0.005, 1)] -= F(300.0)
        f[_at_most(rng.random((n, p)) < 0.01, 1)] = np.nan
        holes = rng.random(p) < 0.015
        f[np.ix_(rng.random(n) < 0.34, holes)] = np.nan
    _special_pixels(f)
    f.setflags(write=False)
    return f


# the adversarial case is run at sigma 1 and, for bounds that cross, at negative sigmas: (sigma_low, sigma_high)
ADVERSARIAL_SIGMAS = [(1.0, 1.0), (-0.25, -0.5), (-0.5, 1.0)]


_truths = {}


def truth(case, mode, n_active=None, sigmas=None, weights=None):
    """The Clip of `case` over its first n_active frames (default: all), computed once; weights default to weights_of"""
    key = (case, mode, n_active, sigmas, None if weights is None else weights.tobytes())
    if key not in _truths:
        n = case.frames if n_active is None else n_active
        sl, sh = (case.kappa, case.kappa) if sigmas is None else sigmas
        frames = make_frames(case)[:n]
        t = clip(frames, weights_of(n) if weights is None else weights, mode, sl, sh, REF_LOC)
        must = t.must_hand_over | zone_overflow(case, mode, t, n)
        must.setflags(write=False)
        _truths[key] = t._replace(must_hand_over=must)
    return _truths[key]
