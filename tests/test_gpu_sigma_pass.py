"""GPU: the clipping pass of the zonal plain-sigma kernel on pixels built to sit on its edges -- zones clipped to 7 and
8 samples per side, samples on and next to a clip bound, the median read at both ends of its window, odd and even
survivor counts, infinite samples, NaN-bordered waves, negative kappa -- at 16 / 32 / 64 / 100 / 128 frames (stacks
of exactly a network size run the TIGHT instantiation, 100 frames the padded one).  Bar, against the CPU oracle:
clip counters equal, values within 1e-5 relative (NaN where the oracle has NaN)."""
import numpy as np
import pytest

from util import describe_mismatch

pytestmark = pytest.mark.gpu

RTOL = 1e-5
F32 = np.float32


def close_values(a, b, rtol=RTOL):
    a = np.asarray(a, F32)
    b = np.asarray(b, F32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a) & (a != b)
    return bool(np.all(np.abs(a[ok].astype(np.float64) - b[ok]) <= rtol * np.abs(b[ok].astype(np.float64))))


def gaussian(rng, n, loc=1000.0, scale=30.0):
    return (loc + scale * rng.standard_normal(n)).astype(F32)


def with_outliers(rng, n, k_lo, k_hi):
    """k_lo samples far below the bulk and k_hi far above it (distinct values: the zone is clipped k per side)"""
    c = gaussian(rng, n)
    pos = rng.permutation(n)
    c[pos[:k_lo]] = F32(1000.0 - 600.0) - F32(13.0) * np.arange(k_lo, dtype=F32)
    c[pos[k_lo:k_lo + k_hi]] = F32(1000.0 + 600.0) + F32(17.0) * np.arange(k_hi, dtype=F32)
    return c


def first_bound(col, kappa):
    """the reference's low bound median - kappa * std of col, in float64 (close to, not equal to, its fp32 value)"""
    x = np.sort(col.astype(np.float64))
    m = len(x)
    med = x[m // 2] if m % 2 else 0.5 * (x[m // 2 - 1] + x[m // 2])
    return med - kappa * x.std()


def bound_scan(rng, n, kappa, ulps=8, far=None):
    """columns whose one low sample walks across the low bound in single ulps: the value that solves
    x = bound(column with x) -- found in float64 -- and its neighbours +-ulps in fp32.  The bulk is a shuffled even
    grid (no sample beyond 1.8 sigma), so whether the walking sample is clipped is decided by that bound alone.
    far: one more sample that far above the bulk -- clipped in the first round, the scan then meets the bound of the
    second"""
    base = (1000.0 + 30.0 * rng.permutation(np.linspace(-1.0, 1.0, n))).astype(F32)
    x = F32(first_bound(base[1:] if far else base, kappa))
    for _ in range(200):
        base[0] = x
        x = F32(0.5 * (float(x) + first_bound(np.delete(base, 1) if far else base, kappa)))
    cols = []
    v = x
    for _ in range(ulps):
        v = np.nextafter(v, F32(-np.inf))
    for _ in range(2 * ulps + 1):
        c = base.copy()
        c[0] = v
        if far:
            c[1] = F32(far)
        cols.append(c)
        v = np.nextafter(v, F32(np.inf))
    return cols


def edge_columns(n, seed):
    rng = np.random.default_rng(seed)
    cols = []
    for _ in range(8):
        cols.append(gaussian(rng, n))
    kz = 8 if n >= 48 else 4          # zone width of the network this stack runs on
    for k in sorted({kz - 1, kz, 1, 2, 3}):
        # k clips per side, on one side only (the median window's ends: a = 0 with the high zone nearly empty, and
        # the low zone nearly full with b = NS) and on both; 1 / 2 / 3 give odd and even survivor counts
        if 2 * k + 2 > n // 2:
            continue
        for _ in range(3):
            cols.append(with_outliers(rng, n, k, 0))
            cols.append(with_outliers(rng, n, 0, k))
            cols.append(with_outliers(rng, n, k, k))
            cols.append(with_outliers(rng, n, k, k - 1))
    cols += bound_scan(rng, n, 2.0)
    # a second clipping pass that meets a bound: a far outlier first, then a sample next to the bound of round 2
    cols += bound_scan(rng, n, 2.0, ulps=3, far=5000.0)
    # infinite samples
    for inf in (np.inf, -np.inf):
        c = gaussian(rng, n)
        c[3] = F32(inf)
        cols.append(c)
    c = gaussian(rng, n)
    c[2], c[5] = F32(np.inf), F32(-np.inf)
    cols.append(c)
    # missing samples: a few (the zonal pass), more than a zone holds (the generic pass), all
    for n_nan in (1, 3, kz, kz + 1, n - 1, n):
        c = gaussian(rng, n)
        c[rng.permutation(n)[:n_nan]] = np.nan
        cols.append(c)
    # ties on the median and inside the zones
    c = np.full(n, F32(1000.0))
    c[: n // 3] = F32(990.0)
    cols.append(c)
    c = with_outliers(rng, n, 3, 3)
    c[:4] = F32(400.0)
    cols.append(c)
    return cols


def stack_of(cols, n):
    """(n, 64 * rows) frames, one pixel per column, padded to whole waves with Gaussian pixels; a NaN border (a
    whole wave of pixels missing from some frames) at the end"""
    rng = np.random.default_rng(n)
    per = 64
    rows = (len(cols) + per - 1) // per + 1
    p = rows * per
    frames = np.empty((n, p), F32)
    for i in range(p):
        frames[:, i] = cols[i] if i < len(cols) else gaussian(rng, n)
    frames[: max(1, n // 10), (rows - 1) * per:] = np.nan        # last wave: NaN-bordered frames
    return frames, per, rows


def run(nl, oracle, frames, width, height, sl, sh):
    n = frames.shape[0]
    with nl.StackHandle(n, width, height) as st:
        st.upload_frames(frames)
        st.set_exact(False)
        got, cl, ch = st.run(2, sl, sh, 0.0)
    rc, want, wl, wh, _ = oracle.stack_apply(2, frames, None, sl, sh, 0.0, num_cpu=4)
    assert rc == 0
    return got, (cl, ch), want, (wl, wh)


@pytest.mark.parametrize("n", [16, 32, 64, 100, 128])
@pytest.mark.parametrize("kappa", [(2.0, 2.0), (2.75, 1.5), (1.0, 3.0)])
def test_sigma_pass_edges(nl, oracle, n, kappa):
    frames, width, height = stack_of(edge_columns(n, 7000 + n), n)
    got, gc, want, wc = run(nl, oracle, frames, width, height, *kappa)
    assert gc == wc, "n=%d kappa=%r clip counters %r vs oracle %r" % (n, kappa, gc, wc)
    assert close_values(got, want), "n=%d kappa=%r: %s" % (n, kappa, describe_mismatch(got, want))


@pytest.mark.parametrize("n", [16, 32, 64, 100, 128])
@pytest.mark.parametrize("kappa", [(-0.5, 2.0), (2.0, -0.5), (-0.25, -0.25)])
def test_sigma_pass_negative_kappa(nl, oracle, n, kappa):
    # inverted bounds: the reference's "low first" order decides, and the pass hands such pixels to the exact replay
    frames, width, height = stack_of(edge_columns(n, 7100 + n), n)
    got, gc, want, wc = run(nl, oracle, frames, width, height, *kappa)
    assert gc == wc, "n=%d kappa=%r clip counters %r vs oracle %r" % (n, kappa, gc, wc)
    assert close_values(got, want), "n=%d kappa=%r: %s" % (n, kappa, describe_mismatch(got, want))


@pytest.mark.parametrize("n", [16, 32, 64, 100, 128])
def test_sigma_pass_bound_scan_crosses(nl, oracle, n):
    # the scan really straddles the bound: within each scan the oracle clips the low end and keeps the high end
    rng = np.random.default_rng(7200 + n)
    cols = bound_scan(rng, n, 2.0, ulps=8) + bound_scan(rng, n, 2.0, ulps=8, far=5000.0)
    frames, width, height = stack_of(cols, n)
    got, gc, want, wc = run(nl, oracle, frames, width, height, 2.0, 2.0)
    assert gc == wc, "n=%d clip counters %r vs oracle %r" % (n, gc, wc)
    assert close_values(got, want), "n=%d: %s" % (n, describe_mismatch(got, want))
    one = np.zeros((n, 1), F32)
    clipped = []
    for c in cols:
        one[:, 0] = c
        rc, _, lo, _, _ = oracle.stack_apply(2, one, None, 2.0, 2.0, 0.0, num_cpu=1)
        assert rc == 0
        clipped.append(lo)
    for scan in (clipped[:17], clipped[17:]):
        assert scan[0] > scan[-1], "n=%d: the scan does not cross the bound (%r)" % (n, scan)
