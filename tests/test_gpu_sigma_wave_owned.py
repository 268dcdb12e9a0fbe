"""GPU: the wave-owned form of the zonal plain-sigma kernel -- at exactly 128 frames a wave of
the dominant kernel shares nothing with its neighbours: no LDS, no barrier, its own reservation on the hand-over lists,
its own addition to the clip totals, at any number of waves per workgroup.  What that changes is who books what
where, so the stacks here are about bookkeeping: pixel counts that leave a wave ragged or nearly empty, totals that come from many per-wave
additions (and waves that add nothing), waves that all hand pixels over -- to the capacity of the generic list --,
undecidable pixels in several waves, passes repeated on one handle (plain protocol first, fused afterwards), and the
fast maps pass, which runs the same body from its own launcher.
Bar, through the C ABI against the CPU oracle: clip counters equal, values within 1e-5 relative (NaN where the oracle
has NaN)."""
import numpy as np
import pytest

from util import describe_mismatch

pytestmark = pytest.mark.gpu

RTOL = 1e-5
F32 = np.float32
N = 128
WAVE = 64
KAPPA = 3.0
KERNEL = "stack_sigma_fast_kernel<128, true, false, true,"
NO_SHARED_HINTS = 512          # developer switch: a handle starts without the list lengths of earlier handles


def close_values(a, b, rtol=RTOL):
    a = np.asarray(a, F32)
    b = np.asarray(b, F32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a) & (a != b)
    return bool(np.all(np.abs(a[ok].astype(np.float64) - b[ok]) <= rtol * np.abs(b[ok].astype(np.float64))))


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def gaussian(rng, width, height):
    return (1000.0 + 30.0 * rng.standard_normal((N, height, width))).astype(F32)


def bulk(rng, width, height):
    """Gaussian frames with far outliers now and then: several clipping passes, every sample finite"""
    f = gaussian(rng, width, height)
    f[rng.random(f.shape) < 0.01] += F32(900.0)
    f[rng.random(f.shape) < 0.005] -= F32(700.0)
    return f


def grid(rng, width, height):
    """every pixel a shuffled even grid, no sample beyond 1.8 sigma: at kappa 3 nothing is clipped that is not planted,
    and the grid stays unclipped when up to 20 of its samples are taken away"""
    f = np.empty((N, height, width), F32)
    col = (1000.0 + 30.0 * np.linspace(-1.0, 1.0, N)).astype(F32)
    for y in range(height):
        for x in range(width):
            f[:, y, x] = rng.permutation(col)
    return f


def plant(rng, f, y, x, k_lo, k_hi):
    pos = rng.permutation(N)
    f[pos[:k_lo], y, x] = F32(300.0) - F32(13.0) * np.arange(k_lo, dtype=F32)
    f[pos[k_lo:k_lo + k_hi], y, x] = F32(1700.0) + F32(17.0) * np.arange(k_hi, dtype=F32)


def drop(rng, f, y, x, k):
    f[rng.permutation(N)[:k], y, x] = np.nan


def first_bound(col, kappa):
    """the reference's low bound median - kappa * std of col, in float64 (close to, not equal to, its fp32 value)"""
    x = np.sort(col.astype(np.float64))
    m = len(x)
    med = x[m // 2] if m % 2 else 0.5 * (x[m // 2 - 1] + x[m // 2])
    return med - kappa * x.std()


def bound_scan(rng, kappa, ulps=8):
    """columns whose one low sample walks across the first round's low bound in single ulps (the construction of
    test_gpu_sigma_pass.py): the value that solves x = bound(column with x), found in float64, and its neighbours"""
    base = (1000.0 + 30.0 * rng.permutation(np.linspace(-1.0, 1.0, N))).astype(F32)
    x = F32(first_bound(base, kappa))
    for _ in range(200):
        base[0] = x
        x = F32(0.5 * (float(x) + first_bound(base, kappa)))
    v = x
    for _ in range(ulps):
        v = np.nextafter(v, F32(-np.inf))
    cols = []
    for _ in range(2 * ulps + 1):
        c = base.copy()
        c[0] = v
        cols.append(c)
        v = np.nextafter(v, F32(np.inf))
    return cols


# ---- the stacks: name -> (frames (N, height, width), facts) -------------------------------------------------------------
def tiny_clean(rng):
    return gaussian(rng, 5, 7), {}


def tiny_outliers(rng):
    return bulk(rng, 5, 7), {"clips": True}


def ragged_clean(rng):
    return gaussian(rng, 67, 3), {}


def ragged_outliers(rng):
    return bulk(rng, 67, 3), {"clips": True}


def planted(rng):
    # 40 waves (a row is a wave), ten workgroups of old.  Odd rows: a few pixels with planted outliers; even rows: none,
    # those waves add nothing to the totals
    f = grid(rng, WAVE, 40)
    lo = hi = 0
    for y in range(1, 40, 2):
        for x in rng.permutation(WAVE)[: 1 + y % 5]:
            k_lo, k_hi = int(rng.integers(0, 4)), int(rng.integers(1, 4))
            plant(rng, f, y, x, k_lo, k_hi)
            lo += k_lo
            hi += k_hi
    return f, {"clips": True, "counters": (lo, hi)}


def nan_columns(rng):
    # the first two columns miss 9 ... 20 samples per pixel in every row: every wave hands two pixels over, four
    # consecutive waves -- one workgroup of old -- among them; a few planted outliers elsewhere
    f = grid(rng, WAVE, 8)
    for y in range(8):
        for x in (0, 1):
            drop(rng, f, y, x, 9 + (3 * y + 5 * x) % 12)
        plant(rng, f, y, 7 + y, 2, 1)
    return f, {"clips": True, "counters": (16, 8), "generic": 16}


def all_handed_over(rng):
    # every pixel misses 9 ... 20 samples: the generic list is as long as the tile (its capacity)
    f = bulk(rng, WAVE, 4)
    for y in range(4):
        for x in range(WAVE):
            drop(rng, f, y, x, 9 + (x + 7 * y) % 12)
    return f, {"clips": True, "generic": 4 * WAVE}


def no_data_pixel(rng):
    f = bulk(rng, WAVE, 3)
    f[:, 1, 17] = np.nan                   # no sample at all
    drop(rng, f, 2, 40, N - 1)             # a single one
    return f, {"clips": True}


def undecidable(rng):
    # two scans across the first round's bound, in waves 0 and 2 (kappa 2, as in test_gpu_sigma_pass.py)
    f = grid(rng, WAVE, 4)
    for y, x0 in ((0, 3), (2, 40)):
        for i, c in enumerate(bound_scan(rng, 2.0)):
            f[:, y, x0 + i] = c
    return f, {"kappa": 2.0, "clips": True, "fallback": 2}


STACKS = {"tiny_clean": tiny_clean, "tiny_outliers": tiny_outliers, "ragged_clean": ragged_clean,
          "ragged_outliers": ragged_outliers, "planted": planted, "nan_columns": nan_columns,
          "all_handed_over": all_handed_over, "no_data_pixel": no_data_pixel, "undecidable": undecidable}
_cache = {}


def stack(oracle, kind):
    """(flat frames, width, height, facts, oracle's (result, low, high)): built and solved once, read-only"""
    if kind not in _cache:
        rng = np.random.default_rng(15000 + sorted(STACKS).index(kind))
        frames, facts = STACKS[kind](rng)
        _, height, width = frames.shape
        flat = np.ascontiguousarray(frames.reshape(N, height * width))
        k = facts.get("kappa", KAPPA)
        rc, want, wl, wh, _ = oracle.stack_apply(2, flat, None, k, k, 0.0, num_cpu=4)
        assert rc == 0
        flat.setflags(write=False)
        want.setflags(write=False)
        _cache[kind] = (flat, width, height, facts, (want, int(wl), int(wh)))
    return _cache[kind]


@pytest.mark.parametrize("kind", sorted(STACKS))
def test_wave_owned_pass_equals_the_oracle(nl, oracle, kind):
    flat, width, height, facts, (want, wl, wh) = stack(oracle, kind)
    k = facts.get("kappa", KAPPA)
    with nl.StackHandle(N, width, height) as st:
        st.upload_frames(flat)
        st.set_exact(False)
        got, cl, ch = st.run(2, k, k, 0.0)
        kernel, generic, fallback = st.last_kernel_name, st.last_generic_pixels, st.last_fallback_pixels
    print("%-16s %dx%d counters %r oracle %r generic list %d exact list %d on %s"
          % (kind, width, height, (cl, ch), (wl, wh), generic, fallback, kernel))
    assert kernel.startswith(KERNEL), "%s ran on %s" % (kind, kernel)
    if "counters" in facts:
        assert (wl, wh) == facts["counters"], "%s: the oracle clips %r, planted %r" % (kind, (wl, wh), facts["counters"])
    if facts.get("clips"):
        assert wl + wh > 0, "%s: nothing is clipped" % kind
    assert (cl, ch) == (wl, wh), "%s clip counters %r vs oracle %r" % (kind, (cl, ch), (wl, wh))
    assert close_values(got, want), "%s: %s" % (kind, describe_mismatch(got, want))
    if "generic" in facts:
        assert generic == facts["generic"], "%s: generic list of %d pixels, planted %d" % (kind, generic, facts["generic"])
    if "fallback" in facts:
        assert fallback >= facts["fallback"], "%s: exact list of %d pixels" % (kind, fallback)


def test_three_passes_on_one_handle_equal_a_fresh_handle(nl, oracle):
    rng = np.random.default_rng(15100)
    frames = bulk(rng, WAVE, 40)
    frames[: N // 10, :2, :] = np.nan                      # (a NaN border: some pixels go through the generic list)
    flat = np.ascontiguousarray(frames.reshape(N, 40 * WAVE))
    rc, want, wl, wh, _ = oracle.stack_apply(2, flat, None, KAPPA, KAPPA, 0.0, num_cpu=4)
    assert rc == 0

    def passes(count):
        runs = []
        with nl.StackHandle(N, WAVE, 40) as st:
            st.upload_frames(flat)
            st.set_dev_flags(NO_SHARED_HINTS)
            for _ in range(count):
                got, cl, ch = st.run(2, KAPPA, KAPPA, 0.0)
                runs.append((got.view(np.uint32).copy(), (cl, ch), st.last_pass_protocol & 1, st.last_fallback_pixels,
                             st.last_generic_pixels, st.last_kernel_name))
        return runs

    three, fresh = passes(3), passes(1)
    print("protocols %r exact lists %r generic lists %r" % ([r[2] for r in three], [r[3] for r in three], [r[4] for r in three]))
    assert all(r[5].startswith(KERNEL) for r in three + fresh)
    assert [r[2] for r in three] == [0, 1, 1] and fresh[0][2] == 0, "the first pass of a handle is plain, the later ones fused"
    for r in three + fresh:
        assert r[1] == (wl, wh), "clip counters %r vs oracle %r" % (r[1], (wl, wh))
        assert np.array_equal(r[0], three[0][0]), describe_mismatch(r[0].view(F32), three[0][0].view(F32))
        assert r[3:5] == three[0][3:5]
    assert close_values(three[0][0].view(F32), want), describe_mismatch(three[0][0].view(F32), want)


def test_fast_maps_pass_runs_the_wave_owned_twin(nl, oracle):
    flat, width, height, facts, (want, wl, wh) = stack(oracle, "nan_columns")
    with nl.StackHandle(N, width, height) as st:
        st.upload_frames(flat)
        out, cl, ch, low, high = st.run_maps(2, KAPPA, KAPPA, 0.0, fast=True)
        kernel, generic = st.last_kernel_name, st.last_generic_pixels
        ref_out, rl, rh, ref_low, ref_high = st.run_maps(2, KAPPA, KAPPA, 0.0, fast=False)
    print("fast maps on %s: counters %r, column kernel %r, generic list %d" % (kernel, (cl, ch), (rl, rh), generic))
    assert kernel.startswith(KERNEL) and kernel.endswith("maps>"), kernel
    assert close_values(ref_out, want) and (rl, rh) == (wl, wh)
    assert (cl, ch) == (rl, rh) == facts["counters"]
    assert np.array_equal(low, ref_low) and np.array_equal(high, ref_high)
    assert (int(low.astype(np.int64).sum()), int(high.astype(np.int64).sum())) == (cl, ch)
    assert close_values(out, ref_out), describe_mismatch(out, ref_out)
    assert generic == facts["generic"]
