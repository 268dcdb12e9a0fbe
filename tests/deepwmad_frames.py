"""Weights and truths for the tests of the deep weighted MAD-sigma pass (include/nlstack_deepwmad.h: nl_stack_run_mad_weighted
of 513 ... 2048 frames on the 8- / 16-lane engine), shared by the CPU check (tests/test_deepwmad_frames.py) and the GPU
tests (tests/test_gpu_deepwmad.py).  The frames are those of tests/deepstack_frames.py; the truth is tests/wmad_ref.py's
restatement of the header's definition (mad_clip), which works at any depth.

Weights.  wclip_ref.weights_of asserts distinct scalars and breaks above 521 frames, and rejmap_ref.weights_of(2048) has 101
distinct values: a kernel that pairs a frame with another frame's weight could pass under either.  weights_of(n) here is
1 / (1 + 3 s_k) with s_k = (1237 k mod 4099) / 4098, k = 0 ... n-1: 4099 is prime, so the s_k are distinct for n <= 4099,
they jump about the frame index instead of rising with it, and the weights lie in [0.25, 1].  Every array is computed once
per process and returned read-only."""
import numpy as np

import deepstack_frames as deep
import wmad_ref

SIGMAS, TIGHT, REF_LOC = deep.SIGMAS, deep.TIGHT, deep.REF_LOC
DEPTHS = deep.DEPTHS
STREAMING_KERNEL = "stack_clip_weighted_kernel<"

_weights, _truths = {}, {}


def weights_of(n):
    """[n] float32, read-only: n distinct weights in [0.25, 1]"""
    if n not in _weights:
        assert 0 < n <= 4099
        s = ((1237 * np.arange(n, dtype=np.int64)) % 4099).astype(np.float64) / 4098.0
        w = (1.0 / (1.0 + 3.0 * s)).astype(np.float32)
        w.setflags(write=False)
        _weights[n] = w
    return _weights[n]


def truth(n, sigmas=SIGMAS, weights=None):
    """wmad_ref.Mad of deepstack_frames.frames_of(n) under weights_of(n) (or `weights`); computed once"""
    key = (n, sigmas, None if weights is None else weights.tobytes())
    if key not in _truths:
        _truths[key] = wmad_ref.mad_clip(deep.frames_of(n), weights_of(n) if weights is None else weights,
                                         sigmas[0], sigmas[1], REF_LOC)
    return _truths[key]


def totals(t, rows=slice(None)):
    return int(t.clip_low[rows].sum()), int(t.clip_high[rows].sum())


def handed_over(t):
    """pixels the streaming engine hands to the column kernel: those without a finite median and those without a sample"""
    return int((t.degenerate | (t.n == 0)).sum())
