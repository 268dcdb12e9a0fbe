"""Frames and truths for the tests of the full maps pass (include/nlstack_fullmaps.h), shared by the CPU check of the
frames themselves (tests/test_fullmaps_frames.py) and the GPU tests (tests/test_gpu_fullmaps.py).  In the form of
tests/deepmaps_frames.py; the image is 41 x 23 = 943 pixels, no multiple of the 64, 128 or 256 pixels of a workgroup.

What the frames hold, at every depth n:
  * a sky 1000 + 20 N(0, 1) with outliers on both sides (+400, -300), at rates that fall as 1 / n down to 3 % / 1.5 %;
  * NaN borders that grow with the frame index (frame i misses its 6 i // n left columns and its 4 i // n top rows), so
    the sample count of a pixel falls towards the corner: both parities occur, and from 114 frames on the border pixels
    have fewer than 114 samples -- the hand-over list of stack_mad_bitonic_kernel; a few random NaN beside them;
  * one pixel without data;
  * four pixels whose median is not finite, each with at least half of its samples infinite: mostly +Inf, mostly -Inf,
    all but one +Inf, and a -Inf pixel that also misses every fifth frame (a narrow pixel from 114 frames on).

The truth is the CPU oracle called pixel by pixel (rejmap_ref.per_pixel), held to its whole-image totals, EXCEPT at the four
pixels without a finite median.  There the reference is not defined: the deviations hold Inf - Inf = NaN, its second
quickselect (qsort.go:94-126) takes a NaN pivot and runs off the array -- the reference panics, the oracle reads past its
buffer (tests/test_wmad_ref.py says the same and does not call it either).  What every defined order of that selection
gives is arithmetic, not a choice: the second median is Inf or NaN, so is sigma * mad * 1.4826 for sigma > 0; with a median
of +Inf the bounds are (Inf - Inf or NaN, Inf or NaN), with -Inf (-Inf or NaN, NaN): no sample is below the one or above the
other, nothing is rejected, and the mean of samples that hold infinities of one sign is that infinity.  So the truth
there is 0 / 0 and +Inf or -Inf, whose bit patterns are unique, and the oracle sees those pixels as pixels without data.
Every array is computed once per process and returned read-only."""
import numpy as np

import rejmap_ref as ref

SIGMAS = (3.0, 3.0)
TIGHT = (1.2, 1.2)
REF_LOC = 123.0
W, H = 41, 23
P = W * H
NO_DATA = 9 * W + 20                         # the pixel without data, clear of the borders
POS_INF, NEG_INF, MOST_POS_INF, NARROW_NEG_INF = (9 * W + 31 + i for i in range(4))
INF_PIXELS = (POS_INF, NEG_INF, MOST_POS_INF, NARROW_NEG_INF)
INF_RESULT = {POS_INF: np.inf, NEG_INF: -np.inf, MOST_POS_INF: np.inf, NARROW_NEG_INF: -np.inf}
BORDER_COLUMNS, BORDER_ROWS = 6, 4           # the borders reach so far in the last frame
# every network size of stack_mad_fast_kernel, both sides of the second-sort / fused-bitonic split at 64, both sides of
# stack_mad_bitonic_kernel's threshold (113 | 114), both lane counts of stack_mad_ml_kernel (256 | 257)
DEPTHS = (1, 2, 8, 9, 16, 33, 48, 64, 65, 80, 97, 113, 114, 120, 128, 129, 200, 256, 257, 400, 512)
BITONIC_MIN_SAMPLES = 114                    # stack_mad_bitonic_kernel hands on the pixels with fewer samples

_frames, _truths = {}, {}


def frames_of(n):
    """[n, P] float32, read-only"""
    if n not in _frames:
        rng = np.random.default_rng(7000 * n + W)
        f = (1000.0 + 20.0 * rng.standard_normal((n, P))).astype(np.float32)
        u = rng.random((n, P))
        hot, cold = max(0.03, 1.5 / n), max(0.015, 1.0 / n)
        f[u < hot] += np.float32(400.0)
        f[(u >= hot) & (u < hot + cold)] -= np.float32(300.0)
        f[rng.random((n, P)) < 0.2 / n] = np.nan
        img = f.reshape(n, H, W)
        for i in range(n):
            img[i, :, :BORDER_COLUMNS * i // n] = np.nan
            img[i, :BORDER_ROWS * i // n, :] = np.nan
        f[:, NO_DATA] = np.nan
        half = n - n // 2                                # at least half of n
        f[:, INF_PIXELS] = (1000.0 + 20.0 * rng.standard_normal((n, 4))).astype(np.float32)
        f[:half, POS_INF] = np.inf
        f[n - half:, NEG_INF] = -np.inf
        f[min(1, n - 1):, MOST_POS_INF] = np.inf
        present = np.flatnonzero(np.arange(n) % 5 != 0) if n >= 5 else np.arange(n)
        f[np.setdiff1d(np.arange(n), present), NARROW_NEG_INF] = np.nan
        f[present[:present.size - present.size // 2], NARROW_NEG_INF] = -np.inf
        f.setflags(write=False)
        _frames[n] = f
    return _frames[n]


def medians_of(frames):
    """the reference's median of every pixel (qsort.go:68-82: odd n the middle, even n 0.5 * (lower + upper)), NaN = no sample"""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.sort(frames.T.astype(np.float32), axis=1)              # NaN sorts last
        n = (~np.isnan(s)).sum(1)
        at = np.arange(s.shape[0])
        upper, lower = s[at, np.minimum(n >> 1, s.shape[1] - 1)], s[at, np.maximum((n >> 1) - 1, 0)]
        med = np.where(n & 1, upper, np.float32(0.5) * (lower + upper)).astype(np.float32)
    med[n == 0] = np.nan
    return med, n


def truth(oracle, n, mode, n_active=None, sigmas=SIGMAS):
    """rejmap_ref.Truth of frames_of(n)[:n_active] (the head of this file: the oracle pixel by pixel, arithmetic where the
    median is not finite); computed once"""
    key = (n, mode, n_active, sigmas)
    if key not in _truths:
        fr = np.ascontiguousarray(frames_of(n)[:n if n_active is None else n_active])
        med, count = medians_of(fr)
        undefined = np.flatnonzero((count > 0) & ~np.isfinite(med))
        seen = fr.copy()
        seen[:, undefined] = np.nan
        result, low, high = ref.per_pixel(oracle, mode, seen, None, sigmas[0], sigmas[1], REF_LOC)
        rc, _, cl, ch, _ = oracle.stack_apply(mode, seen, None, sigmas[0], sigmas[1], REF_LOC)
        assert rc == 0 and (cl, ch) == (int(low.sum()), int(high.sum()))
        assert low.max(initial=0) <= 65535 and high.max(initial=0) <= 65535
        for p in undefined:
            inf = fr[np.isinf(fr[:, p]), p]
            assert inf.size * 2 >= count[p] and np.all(inf == inf[0]), "pixel %d: infinities of one sign only" % p
            result[p] = inf[0]
        t = ref.Truth(result, int(cl), int(ch), low.astype(np.uint16), high.astype(np.uint16),
                      (~np.isnan(fr)).sum(0).astype(np.uint16))
        for a in (t.result, t.reject_low, t.reject_high, t.coverage):
            a.setflags(write=False)
        _truths[key] = t
    return _truths[key]
