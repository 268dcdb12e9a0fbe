"""Frames and truths for the tests of the deep pass (include/nlstack_deepstack.h: the median and MAD sigma of
513 ... 2048 frames on 8 or 16 lanes per pixel), shared by the CPU check of the frames themselves
(tests/test_deepstack_frames.py) and the GPU tests (tests/test_gpu_deepstack.py).

The frames are those of tests/fullmaps_frames.py, which work at any depth: frames_of(n) and truth(oracle, n, mode) are used
as they are, with everything the head of that file says about the four pixels without a finite median.  The image is
41 x 23 = 943 pixels, no multiple of the 32 or 16 pixels a workgroup takes at 8 or 16 lanes per pixel.  The depths are
both ends of both lane counts and something in between, odd and even; the NaN borders that grow with the frame index
give both parities of the per-pixel sample count and pixels with far fewer samples than frames (a sixth of them in
the corner).

survivor_means(n): the fp64 mean of the survivors of the MAD rejection as the header defines it, from numpy alone -- what
the oracle's sequential fp32 sum and the kernels' per-lane fp32 sums are both roundings of.  Every array is computed once
per process and returned read-only."""
import collections

import numpy as np

from fullmaps_frames import (INF_PIXELS, INF_RESULT, NO_DATA, P, REF_LOC, SIGMAS, TIGHT, H, W,  # noqa: F401
                             frames_of, medians_of, truth)

DEPTHS = (513, 700, 1023, 1024, 1025, 1500, 2047, 2048)
TIGHT_DEPTHS = (700, 1500)                  # one depth per lane count also runs the second sigma pair
LANE_SAMPLES = 128


def lanes_of(n):
    """lanes per pixel of the deep kernels at n active frames"""
    assert 512 < n <= 2048
    return 8 if n <= 8 * LANE_SAMPLES else 16


Whole = collections.namedtuple("Whole", "result clip_low clip_high")
_wholes, _means = {}, {}


def whole_truth(oracle, n, mode, sigmas=SIGMAS):
    """(result, clip_low, clip_high) of frames_of(n) from ONE call of the oracle over the whole image -- what
    truth(oracle, n, mode) gives without its per-pixel counts (tests/test_deepstack_frames.py holds the two to each other),
    at a thousandth of its oracle calls: the GPU tests that need no per-pixel counts use this one.  The four pixels
    without a finite median are treated as truth treats them (the head of tests/fullmaps_frames.py): hidden from the
    oracle, their result the infinity arithmetic gives, nothing rejected."""
    key = (n, mode, sigmas)
    if key not in _wholes:
        fr = frames_of(n)
        med, count = medians_of(fr)
        undefined = np.flatnonzero((count > 0) & ~np.isfinite(med))
        seen = fr.copy()
        seen[:, undefined] = np.nan
        rc, result, cl, ch, _ = oracle.stack_apply(mode, seen, None, sigmas[0], sigmas[1], REF_LOC)
        assert rc == 0
        result = np.array(result, np.float32)
        for p in undefined:
            inf = fr[np.isinf(fr[:, p]), p]
            assert inf.size * 2 >= count[p] and np.all(inf == inf[0]), "pixel %d: infinities of one sign only" % p
            result[p] = inf[0]
        result.setflags(write=False)
        _wholes[key] = Whole(result, int(cl), int(ch))
    return _wholes[key]


def survivor_means(n, sigmas=SIGMAS):
    """(mean, low, high): per pixel the fp64 mean of the samples the MAD rejection keeps, and its two counts -- the header's
    definition in fp32 (median; d = |v - median|; mad; sd = mad * 1.4826f; lo = median - sigma_low * sd,
    hi = median + sigma_high * sd; v < lo low, else v > hi high).  NaN mean where the median is not finite or no sample
    exists."""
    key = (n, sigmas)
    if key not in _means:
        fr = frames_of(n)
        med, count = medians_of(fr)
        with np.errstate(invalid="ignore", over="ignore"):
            dev = np.abs(fr - med[None, :]).astype(np.float32)
            mad, _ = medians_of(dev)
            sd = (mad * np.float32(1.4826)).astype(np.float32)
            lo = (med - (np.float32(sigmas[0]) * sd).astype(np.float32)).astype(np.float32)
            hi = (med + (np.float32(sigmas[1]) * sd).astype(np.float32)).astype(np.float32)
            present = ~np.isnan(fr)
            below = present & (fr < lo[None, :])
            above = present & ~below & (fr > hi[None, :])
            keep = present & ~below & ~above
            mean = np.where(keep, fr.astype(np.float64), 0.0).sum(0) / keep.sum(0)
        mean[(count == 0) | ~np.isfinite(med)] = np.nan
        out = (mean, below.sum(0), above.sum(0))
        for a in out:
            a.setflags(write=False)
        _means[key] = out
    return _means[key]
