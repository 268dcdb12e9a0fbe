"""GPU: the per-lane lookups of the wave-owned zonal plain-sigma kernel.  At exactly 128 frames
a clipping pass of the loop finds its zone sums (tables indexed by a = clipped low samples and by NS - b = clipped high
and missing samples) and the two ranks of its median (indexed by floor((a + b) / 2)) in LDS rows that every lane fills
once behind the sort and reads at its own index; the peeled first pass of a clean wave reads registers.  What can go
wrong is an index, a row or a column, so the stacks here are about which entry a lane reads: lanes beyond the tile,
every table index on either side, indices that change from round to round, every median position with odd and even
survivor counts, neighbouring waves of one workgroup with very different columns, passes repeated on one handle, and
the fast maps pass, which runs the same body from its own launcher.
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
KAPPA = 2.5                    # (the planted stacks: 14 equal outliers of 128 sit at 3.02 sigma -- at 2.5 they go at once)
KERNEL = "stack_sigma_fast_kernel<128, true, false, true,"
NO_SHARED_HINTS = 512          # developer switch: a handle starts without the list lengths of earlier handles
SPAN = 30.0                    # the bulk of a planted column: an even grid over 1000 -/+ SPAN (sigma = 17.4, ends at 1.72 sigma)


def close_values(a, b, rtol=RTOL):
    a = np.asarray(a, F32)
    b = np.asarray(b, F32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a) & (a != b)
    return bool(np.all(np.abs(a[ok].astype(np.float64) - b[ok]) <= rtol * np.abs(b[ok].astype(np.float64))))


def grid(rng, width, height):
    """every pixel a shuffled even grid: at kappa 2.5 nothing of it is clipped, with or without a few samples taken away"""
    f = np.empty((N, height, width), F32)
    col = (1000.0 + SPAN * np.linspace(-1.0, 1.0, N)).astype(F32)
    for y in range(height):
        for x in range(width):
            f[:, y, x] = rng.permutation(col)
    return f


def plant(rng, f, y, x, lows, highs, nans=0):
    """replace samples of pixel (x, y), at random frames, by the given distances below / above 1000 and by NaNs"""
    pos = rng.permutation(N)
    k, m = len(lows), len(highs)
    f[pos[:k], y, x] = F32(1000.0) - np.asarray(lows, F32)
    f[pos[k:k + m], y, x] = F32(1000.0) + np.asarray(highs, F32)
    f[pos[k + m:k + m + nans], y, x] = np.nan


def rounds_of(col, kappa):
    """the clipping rounds of one column in float64 (median -/+ kappa * population sigma, the reference's rule; far from
    its fp32 rounding in every stack here): [(clipped low, clipped high)] per round that clips"""
    x = np.sort(col[~np.isnan(col)].astype(np.float64))
    out = []
    while x.size > 1:
        m = x.size
        med = x[m // 2] if m % 2 else 0.5 * (x[m // 2 - 1] + x[m // 2])
        s = x.std()
        lo, hi = int((x < med - kappa * s).sum()), int((x > med + kappa * s).sum())
        if lo + hi == 0:
            break
        out.append((lo, hi))
        x = x[lo:m - hi]
    return out


# ---- the stacks: name -> (frames (N, height, width), facts) -------------------------------------------------------------
def tiny(rng):
    # one partial wave, clean: the peeled first pass, then the loop at whatever was clipped
    f = grid(rng, 5, 7)
    lo = hi = 0
    for y in range(7):
        for x in range(5):
            k, m = (x + y) % 4, (2 * x + y) % 3
            plant(rng, f, y, x, [700.0] * k, [700.0] * m)
            lo, hi = lo + k, hi + m
    return f, {"counters": (lo, hi)}


def tiny_nan(rng):
    # the same with a NaN in one pixel: the wave is not clean and runs its first pass in the loop as well
    # (a sample of the grid: what is clipped stays what was planted)
    f, facts = tiny(rng)
    f[np.flatnonzero(np.abs(f[:, 2, 1] - F32(1000.0)) <= F32(SPAN))[0], 2, 1] = np.nan
    return f, facts


def every_table_index(rng):
    # pixel (i, j): i % 8 low and j high outliers, all gone in the first round: the second pass reads every a in 0 ... 7
    # and every NS - b in 0 ... 7
    f = grid(rng, WAVE, 8)
    lo = hi = 0
    for j in range(8):
        for i in range(WAVE):
            plant(rng, f, j, i, [700.0] * (i % 8), [700.0] * j)
            assert rounds_of(f[:, j, i], KAPPA) == ([(i % 8, j)] if i % 8 + j else [])
            lo, hi = lo + i % 8, hi + j
    return f, {"counters": (lo, hi)}


def graded(rng):
    # three grades of outliers, 0 ... 2 of each per side: the far ones go in round 1, the middle ones in round 2, the near
    # ones in round 3 -- a and b move in the rounds the loop runs, to entries the first pass did not read
    f = grid(rng, WAVE, 4)
    lo = hi = 0
    most = 0
    for y in range(4):
        for x in range(WAVE):
            p = y * WAVE + x
            kl = [p % 3, (p // 3) % 3, (p // 9) % 3]
            kh = [(p // 27) % 3, (p // 81) % 3, (p + y) % 3]
            lows = [5000.0] * kl[0] + [400.0] * kl[1] + [80.0] * kl[2]
            highs = [5000.0] * kh[0] + [400.0] * kh[1] + [80.0] * kh[2]
            plant(rng, f, y, x, lows, highs)
            want = [(a, b) for a, b in zip(kl, kh) if a + b]
            assert rounds_of(f[:, y, x], KAPPA) == want, (p, want)
            most = max(most, len(want))
            lo, hi = lo + sum(kl), hi + sum(kh)
    assert most == 3
    return f, {"counters": (lo, hi)}


def every_median_position(rng):
    # one row of 256 pixels: 0 ... 8 NaNs and 0 ... 7 low / 0 ... 3 high outliers per pixel -- floor((a + b) / 2) takes every
    # value of its range, the survivor count both parities (8 NaNs, or NaNs and high clips that empty the high zone:
    # the pixel goes through the generic list)
    f = grid(rng, 256, 1)
    lo = hi = 0
    seen = set()
    for p in range(256):
        nn, k, m = p % 9, (p // 9) % 8, (p // 72) % 4
        plant(rng, f, 0, p, [700.0] * k, [700.0] * m, nans=nn)
        assert rounds_of(f[:, 0, p], KAPPA) == ([(k, m)] if k + m else [])
        a, b = k, N - nn - m
        if b > N - 8:
            seen.add(((a + b) // 2, (b - a) % 2))
        lo, hi = lo + k, hi + m
    assert {s[0] for s in seen} == set(range(60, 68)) and len(seen) >= 14, sorted(seen)
    return f, {"counters": (lo, hi), "generic": True}


def slices(rng):
    # 67 x 3 = 201 pixels, one workgroup of four waves whose columns have nothing in common: constant 1, constant 1000,
    # a ramp over the frames with outliers, a grid at 1e6.  One NaN per wave: no wave is clean, every lane reads its zone
    # sums and its median from LDS in its first pass already -- a lane that read a neighbour's rows would be far off
    f = np.empty((N, 3, 67), F32)
    flat = f.reshape(N, 201)
    ramp = (500.0 + 3.0 * np.arange(N)).astype(F32)
    for p in range(201):
        w = p // WAVE
        if w == 0:
            flat[:, p] = F32(1.0)
        elif w == 1:
            flat[:, p] = F32(1000.0)
        elif w == 2:
            col = rng.permutation(ramp)
            col[:p % 4] = F32(-40000.0)
            col[4:4 + p % 3] = F32(90000.0)
            flat[:, p] = col
        else:
            flat[:, p] = rng.permutation((1.0e6 + 100.0 * np.linspace(-1.0, 1.0, N)).astype(F32))
    for w in range(4):
        flat[(7 * w) % N, min(w * WAVE + 5 + w, 200)] = np.nan
    return f, {"clips": True}


STACKS = {"tiny": tiny, "tiny_nan": tiny_nan, "every_table_index": every_table_index, "graded": graded,
          "every_median_position": every_median_position, "slices": slices}
_cache = {}


def stack(oracle, kind):
    """(flat frames, width, height, facts, oracle's (result, low, high)): built and solved once, read-only"""
    if kind not in _cache:
        rng = np.random.default_rng(16000 + sorted(STACKS).index(kind))
        frames, facts = STACKS[kind](rng)
        _, height, width = frames.shape
        flat = np.ascontiguousarray(frames.reshape(N, height * width))
        rc, want, wl, wh, _ = oracle.stack_apply(2, flat, None, KAPPA, KAPPA, 0.0, num_cpu=4)
        assert rc == 0
        flat.setflags(write=False)
        want.setflags(write=False)
        _cache[kind] = (flat, width, height, facts, (want, int(wl), int(wh)))
    return _cache[kind]


@pytest.mark.parametrize("kind", sorted(STACKS))
def test_lookup_pass_equals_the_oracle(nl, oracle, kind):
    flat, width, height, facts, (want, wl, wh) = stack(oracle, kind)
    with nl.StackHandle(N, width, height) as st:
        st.upload_frames(flat)
        st.set_exact(False)
        got, cl, ch = st.run(2, KAPPA, KAPPA, 0.0)
        kernel, generic, fallback = st.last_kernel_name, st.last_generic_pixels, st.last_fallback_pixels
    print("%-22s %dx%d counters %r oracle %r generic list %d exact list %d on %s"
          % (kind, width, height, (cl, ch), (wl, wh), generic, fallback, kernel))
    assert kernel.startswith(KERNEL), "%s ran on %s" % (kind, kernel)
    if "counters" in facts:
        assert (wl, wh) == facts["counters"], "%s: the oracle clips %r, planted %r" % (kind, (wl, wh), facts["counters"])
    assert wl + wh > 0, "%s: nothing is clipped" % kind
    assert (cl, ch) == (wl, wh), "%s clip counters %r vs oracle %r" % (kind, (cl, ch), (wl, wh))
    assert close_values(got, want), "%s: %s" % (kind, describe_mismatch(got, want))
    if not facts.get("generic"):
        assert generic == 0, "%s: %d pixels left the kernel under test for the generic pass" % (kind, generic)


def test_three_passes_on_one_handle_equal_a_fresh_handle(nl, oracle):
    flat, width, height, _, (want, wl, wh) = stack(oracle, "graded")

    def passes(count):
        runs = []
        with nl.StackHandle(N, width, height) as st:
            st.upload_frames(flat)
            st.set_dev_flags(NO_SHARED_HINTS)
            for _ in range(count):
                got, cl, ch = st.run(2, KAPPA, KAPPA, 0.0)
                runs.append((got.view(np.uint32).copy(), (cl, ch), st.last_fallback_pixels, st.last_generic_pixels,
                             st.last_kernel_name))
        return runs

    three, fresh = passes(3), passes(1)
    assert all(r[4].startswith(KERNEL) for r in three + fresh)
    for r in three + fresh:
        assert r[1] == (wl, wh), "clip counters %r vs oracle %r" % (r[1], (wl, wh))
        assert np.array_equal(r[0], three[0][0]), describe_mismatch(r[0].view(F32), three[0][0].view(F32))
        assert r[2:4] == three[0][2:4]
    assert close_values(three[0][0].view(F32), want), describe_mismatch(three[0][0].view(F32), want)


def test_fast_maps_pass_runs_the_lookup_twin(nl, oracle):
    flat, width, height, facts, (want, wl, wh) = stack(oracle, "every_table_index")
    with nl.StackHandle(N, width, height) as st:
        st.upload_frames(flat)
        out, cl, ch, low, high = st.run_maps(2, KAPPA, KAPPA, 0.0, fast=True)
        kernel = st.last_kernel_name
        ref_out, rl, rh, ref_low, ref_high = st.run_maps(2, KAPPA, KAPPA, 0.0, fast=False)
    print("fast maps on %s: counters %r, column kernel %r" % (kernel, (cl, ch), (rl, rh)))
    assert kernel.startswith(KERNEL) and kernel.endswith("maps>"), kernel
    assert close_values(ref_out, want) and (rl, rh) == (wl, wh)
    assert (cl, ch) == (rl, rh) == facts["counters"]
    assert np.array_equal(low, ref_low) and np.array_equal(high, ref_high)
    # pixel (i, j) of the stack holds i % 8 low and j high planted outliers
    assert np.array_equal(np.asarray(low).reshape(height, width), np.tile(np.arange(width) % 8, (height, 1)))
    assert np.array_equal(np.asarray(high).reshape(height, width), np.tile(np.arange(height)[:, None], (1, width)))
    assert close_values(out, ref_out), describe_mismatch(out, ref_out)
