"""Frames and truths for the tests of the deep maps pass (include/nlstack_deepmaps.h), shared by the CPU check of the
frames themselves (tests/test_deepmaps_frames.py) and the GPU tests (tests/test_gpu_deepmaps.py).

rejmap_ref.make_frames would send nearly every pixel of a 129 ... 512-frame stack past the dominant kernel: 5 % NaN is 26
missing samples of 512 where its columns take 15 or 23, 3 % outliers is 15 high clips in one round where the sigma
columns read 8 ranks per side and pass.  So the rates here scale as 1 / n: per pixel about two samples of +400, one of
-300 and four NaN, whatever the depth.  The image is 41 x 23 = 943 pixels, no multiple of the 32 or 64 pixels of a
workgroup.  Every array is computed once per process and returned read-only."""
import numpy as np

import maps_cases

SIGMAS = (3.0, 3.0)
TIGHT = (1.2, 1.2)                           # nearly every pixel clips more than the columns hold: the generic pass
REF_LOC = 123.0
W, H = 41, 23
P = W * H
NO_DATA = 3                                  # rejmap_ref.make_frames: the pixel without data
SINGLE = P - 2                               # ... with a single sample
CONSTANT = W + 1                             # ... whose samples are all the same
HALF_NAN = slice(220, 280)                   # the upper half of the frames is NaN: the generic list
HEAVY = slice(300, 320)                      # 20 samples of +400
INF_PIXELS = (400, 401, 402)                 # +Inf, +Inf, -Inf in one sample each: the exact list

_frames, _truths = {}, {}


def frames_of(n):
    """[n, P] float32, read-only"""
    if n not in _frames:
        rng = np.random.default_rng(5000 * n + W)
        f = (1000.0 + 20.0 * rng.standard_normal((n, P))).astype(np.float32)
        u = rng.random((n, P))
        f[u < 2.0 / n] += np.float32(400.0)
        f[(u >= 2.0 / n) & (u < 3.0 / n)] -= np.float32(300.0)
        f[rng.random((n, P)) < 4.0 / n] = np.nan
        f[:, NO_DATA] = np.nan
        f[:, SINGLE] = np.nan
        f[n // 2, SINGLE] = np.float32(987.5)
        f[:, CONSTANT] = np.float32(1003.25)
        f.reshape(n, H, W)[:, :, 5] = np.float32(1.0)              # a constant image column
        f[n // 2:, HALF_NAN] = np.nan
        k = min(20, n)
        f[:k, HEAVY] = (1400.0 + 20.0 * rng.standard_normal((k, HEAVY.stop - HEAVY.start))).astype(np.float32)
        f[1, INF_PIXELS[0]] = np.inf
        f[2, INF_PIXELS[1]] = np.inf
        f[0, INF_PIXELS[2]] = -np.inf
        f.setflags(write=False)
        _frames[n] = f
    return _frames[n]


def truth(oracle, n, mode, n_active=None, sigmas=SIGMAS):
    """rejmap_ref.Truth of frames_of(n)[:n_active]: the oracle pixel by pixel, held to its whole-image totals"""
    key = (n, mode, n_active, sigmas)
    if key not in _truths:
        fr = np.ascontiguousarray(frames_of(n)[:n if n_active is None else n_active])
        _truths[key] = maps_cases.truth_of(oracle, mode, fr, sigmas, REF_LOC)
    return _truths[key]
