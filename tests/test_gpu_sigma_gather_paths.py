"""GPU: the paths a wave of the zonal plain-sigma kernel can take through its gather and its first clipping pass, at the
frame counts that decide between them -- 128 frames (a stack of exactly the largest network size: the gather from a
running descriptor base, and a clean wave takes the peeled first pass with its constant positions), 112 frames (exactly
a network size as well, but every wave in the loop and the gather clamped per position), 127 and 113 frames (one frame
short of the 128-position network and one above the 112-position one: running base up to position 112, clamped gather
behind it, padding at both ends, every wave in the loop).  Stacks: clean (every wave clean); one NaN in one pixel of an otherwise clean wave (that wave
alone leaves the peeled pass); a NaN-bordered tile; pixels whose first-pass median sits at either end of the median
window (no sample missing / as many missing as the high zone still holds a survivor for, and one more: generic pass).
Bar, through the C ABI against the CPU oracle: clip counters equal, values within 1e-5 relative (NaN where the oracle
has NaN)."""
import numpy as np
import pytest

from util import describe_mismatch

pytestmark = pytest.mark.gpu

RTOL = 1e-5
F32 = np.float32
WAVE = 64
FRAMES = [128, 127, 113, 112]


def close_values(a, b, rtol=RTOL):
    a = np.asarray(a, F32)
    b = np.asarray(b, F32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a) & (a != b)
    return bool(np.all(np.abs(a[ok].astype(np.float64) - b[ok]) <= rtol * np.abs(b[ok].astype(np.float64))))


def bulk(rng, n, width, height):
    """Gaussian frames with a few far outliers per pixel column now and then: several clipping passes, every sample
    finite"""
    f = (1000.0 + 30.0 * rng.standard_normal((n, height, width))).astype(F32)
    hot = rng.random((n, height, width)) < 0.01
    f[hot] += F32(900.0)
    cold = rng.random((n, height, width)) < 0.005
    f[cold] -= F32(700.0)
    return f


def clean_stack(rng, n):
    return bulk(rng, n, WAVE, 12)


def one_nan_stack(rng, n):
    f = bulk(rng, n, WAVE, 12)
    f[n // 3, 5, 17] = np.nan                  # one sample of one pixel: wave 5 takes the NaN count, the others do not
    return f


def nan_border_stack(rng, n):
    # frames shifted against the reference leave NaN borders: rows at the top / bottom and columns at the sides, in
    # different frames (up to 12 missing samples per pixel in the corners: zonal pass, generic pass)
    f = bulk(rng, n, WAVE, 16)
    f[: n // 20, :2, :] = np.nan
    f[n // 20: n // 10, -3:, :] = np.nan
    f[n // 2: n // 2 + 5, :, :4] = np.nan
    f[-3:, :, -5:] = np.nan
    return f


def median_ends_stack(rng, n):
    # first-pass median = position lo_pads + n_valid / 2 of the sorted column.  Top end of the window: nothing missing
    # (rows 0 - 1, clean waves).  Bottom end: as many samples missing as still leave a survivor in the high zone --
    # the zone starts at position 120 of the 128 a stack of exactly 128 frames sorts, at 104 of 112, and at 112 for
    # the padded stacks, whose padding shifts the count -- so every count from 0 to 18 occurs, as whole waves (rows
    # 2 - 20: wave-uniform) and mixed within a wave (rows 21 - 23); the counts beyond the zone go to the generic pass.
    f = bulk(rng, n, WAVE, 24)
    for m in range(19):
        for x in range(WAVE):
            f[rng.permutation(n)[:m], 2 + m, x] = np.nan
    for y in (21, 22, 23):
        for x in range(WAVE):
            f[rng.permutation(n)[: (x + y) % 19], y, x] = np.nan
    return f


STACKS = {"clean": clean_stack, "one_nan": one_nan_stack, "nan_border": nan_border_stack, "median_ends": median_ends_stack}


@pytest.mark.parametrize("n", FRAMES)
@pytest.mark.parametrize("kind", sorted(STACKS))
def test_sigma_gather_paths(nl, oracle, n, kind):
    rng = np.random.default_rng(8000 + 10 * n + sorted(STACKS).index(kind))
    frames = STACKS[kind](rng, n)
    _, height, width = frames.shape
    flat = np.ascontiguousarray(frames.reshape(n, height * width))
    with nl.StackHandle(n, width, height) as st:
        st.upload_frames(flat)
        st.set_exact(False)
        got, cl, ch = st.run(2, 3.0, 3.0, 0.0)
        kernel = st.last_kernel_name
    rc, want, wl, wh, _ = oracle.stack_apply(2, flat, None, 3.0, 3.0, 0.0, num_cpu=4)
    assert rc == 0
    # (positions, zonal, plain sigma, TIGHT = the stack has exactly as many frames as the network positions)
    expect = "stack_sigma_fast_kernel<%d, true, false, %s," % (112 if n == 112 else 128, "true" if n in (112, 128) else "false")
    assert kernel.startswith(expect), "n=%d %s ran on %s, not on %s ...>" % (n, kind, kernel, expect)
    assert cl + ch > 0, "n=%d %s: nothing was clipped (the stack does not exercise a clipping pass)" % (n, kind)
    print("n=%d %-11s kernel %s counters %r oracle %r" % (n, kind, kernel, (cl, ch), (wl, wh)))
    assert (cl, ch) == (wl, wh), "n=%d %s clip counters %r vs oracle %r" % (n, kind, (cl, ch), (wl, wh))
    assert close_values(got, want), "n=%d %s: %s" % (n, kind, describe_mismatch(got, want))
