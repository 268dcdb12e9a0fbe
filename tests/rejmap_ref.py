"""Truth for the per-pixel rejection and coverage maps (include/nlstack_maps.h), from the CPU oracle as it is.

The oracle, like the reference, returns two totals per call.  Called on ONE pixel -- frames[:, i:i+1] -- the totals are
that pixel's own counts and the result is that pixel's result: the reference treats every pixel on its own, so the
per-pixel results are the whole-image result bit for bit and the counts sum to the whole-image totals
(tests/test_rejmap_ref.py holds the checker to that).  Coverage is numpy's count of samples that are not NaN.

Inputs and cases are shared by the CPU self-check and the GPU tests; every truth is computed once per process and
returned read-only."""
import collections
import functools

import numpy as np

SIGMA_LOW, SIGMA_HIGH = 2.0, 2.5
REF_LOC = 123.0

# (name, frames, width, height, mode, weighted): N = 24 takes every mode at 64 pixels per wave on a pixel count that
# is no multiple of 64; the deeper stacks take the narrower waves of exact_plan (160 KiB of LDS: N = 130 sorts 256
# padded slots; N = 330 with two columns 32 lanes; N = 700 pads to 1024 slots, 32 lanes, and with two columns 16)
Case = collections.namedtuple("Case", "name frames width height mode weighted")
MODE_NAMES = {0: "median", 1: "mean", 2: "sigma", 3: "winsor", 4: "mad", 5: "linearfit"}


def _case(n, w, h, mode, weighted=False):
    return Case("%s%s-%dx%dx%d" % (MODE_NAMES[mode], "-weighted" if weighted else "", n, w, h), n, w, h, mode, weighted)


CASES = ([_case(24, 41, 23, m) for m in range(6)] + [_case(24, 41, 23, 2, True), _case(24, 41, 23, 3, True)] +
         [_case(130, 24, 16, 2), _case(130, 24, 16, 5)] +
         [_case(330, 16, 8, 2, True), _case(330, 16, 8, 4)] +
         [_case(700, 16, 8, 5), _case(700, 16, 8, 4)] +
         [_case(2100, 6, 3, 5)])                    # 4096 padded slots: 4 pixels per wave
CLIPPING = [c for c in CASES if c.mode >= 2]


def weights_of(n):
    return (0.25 + 0.75 * ((np.arange(n) * 37 % 101) / 100.0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def make_frames(n, width, height):
    """[n, width * height] float32, read-only: 1000 + 20 N(0, 1); 3 % of the samples +400, 1 % -300, 5 % NaN; one pixel
    without data, one with a single sample, one whose samples are all the same, and one image column of ones."""
    rng = np.random.default_rng(1000 * n + width)
    p = width * height
    f = (1000.0 + 20.0 * rng.standard_normal((n, p))).astype(np.float32)
    u = rng.random((n, p))
    f[u < 0.03] += np.float32(400.0)
    f[(u >= 0.03) & (u < 0.04)] -= np.float32(300.0)
    f[rng.random((n, p)) < 0.05] = np.nan
    f[:, 3] = np.nan                                   # no data
    f[:, p - 2] = np.nan                               # a single sample
    f[n // 2, p - 2] = np.float32(987.5)
    f[:, width + 1] = np.float32(1003.25)              # a constant column of samples
    f.reshape(n, height, width)[:, :, 5] = np.float32(1.0)      # a constant image column
    f.setflags(write=False)
    return f


Truth = collections.namedtuple("Truth", "result clip_low clip_high reject_low reject_high coverage")


def per_pixel(oracle, mode, frames, weights, sigma_low=SIGMA_LOW, sigma_high=SIGMA_HIGH, ref_loc=REF_LOC):
    """(result, reject_low, reject_high): one oracle call per pixel"""
    n, p = frames.shape
    columns = np.ascontiguousarray(frames.T)           # [p, n]: a pixel's samples are one contiguous row
    result = np.empty(p, np.float32)
    low, high = np.zeros(p, np.int64), np.zeros(p, np.int64)
    for i in range(p):
        rc, res, cl, ch, _ = oracle.stack_apply(mode, columns[i].reshape(n, 1), weights, sigma_low, sigma_high, ref_loc)
        assert rc == 0
        result[i], low[i], high[i] = res[0], cl, ch
    return result, low, high


_truths = {}


def truth(oracle, case, n_active=None):
    """The maps of `case` over its first n_active frames (default: all), computed once."""
    key = (case, n_active)
    if key not in _truths:
        n = case.frames if n_active is None else n_active
        frames = np.ascontiguousarray(make_frames(case.frames, case.width, case.height)[:n])
        weights = weights_of(n) if case.weighted else None
        result, low, high = per_pixel(oracle, case.mode, frames, weights)
        assert low.max(initial=0) <= 65535 and high.max(initial=0) <= 65535
        t = Truth(result, int(low.sum()), int(high.sum()), low.astype(np.uint16), high.astype(np.uint16),
                  (~np.isnan(frames)).sum(0).astype(np.uint16))
        for a in (t.result, t.reject_low, t.reject_high, t.coverage):
            a.setflags(write=False)
        _truths[key] = t
    return _truths[key]
