"""What the GPU tests of the maps passes share (tests/test_gpu_rejmap.py, test_gpu_fastmaps.py, test_gpu_residentmaps.py,
test_gpu_deepmaps.py): the frames with pixels for both hand-over paths, their truths from the CPU oracle called pixel by
pixel (tests/rejmap_ref.py), and the comparisons of what a maps pass returns with a truth.  A plain module as
tests/deepmaps_frames.py, which holds the frames of the deep stacks.  The image is 41 x 23 = 943 pixels: three full
workgroups and a partial one, no multiple of 64.  Every array is computed once per process and returned read-only."""
import numpy as np

import rejmap_ref as ref
from util import RTOL, bits_equal, close_values

SIGMA_LOW, SIGMA_HIGH = 2.0, 2.5
TIGHT = (1.2, 1.2)
REF_LOC = 123.0
W, H = 41, 23
P = W * H
NO_DATA = 3                                  # rejmap_ref.make_frames: the pixel without data
HALF_NAN = slice(220, 280)                   # the upper half of the frames is NaN: an aligned frame's border (generic pass)
HEAVY = slice(300, 320)                      # 10 samples of +400: more clipped than a zone of 8 holds (generic pass)
INF_PIXELS = (400, 401, 402)                 # +Inf, +Inf, -Inf in one sample each: the exact list

_frames, _truths = {}, {}


def frames_of(n):
    """[n, P] float32, read-only: rejmap_ref's frames of n with the hand-over pixels added"""
    if n not in _frames:
        f = ref.make_frames(n, W, H).copy()
        rng = np.random.default_rng(77 + n)
        f[n // 2:, HALF_NAN] = np.nan
        k = min(10, n)
        f[:k, HEAVY] = (1400.0 + 20.0 * rng.standard_normal((k, HEAVY.stop - HEAVY.start))).astype(np.float32)
        f[1, INF_PIXELS[0]] = np.inf
        f[2, INF_PIXELS[1]] = np.inf
        f[0, INF_PIXELS[2]] = -np.inf
        f.setflags(write=False)
        _frames[n] = f
    return _frames[n]


def truth_of(oracle, mode, frames, sigmas, ref_loc=REF_LOC):
    """rejmap_ref.Truth of unweighted `frames`: the oracle pixel by pixel, held to its whole-image totals; read-only"""
    result, low, high = ref.per_pixel(oracle, mode, frames, None, sigmas[0], sigmas[1], ref_loc)
    rc, _, cl, ch, _ = oracle.stack_apply(mode, frames, None, sigmas[0], sigmas[1], ref_loc)
    assert rc == 0 and (cl, ch) == (int(low.sum()), int(high.sum()))
    assert low.max(initial=0) <= 65535 and high.max(initial=0) <= 65535
    t = ref.Truth(result, int(cl), int(ch), low.astype(np.uint16), high.astype(np.uint16),
                  (~np.isnan(frames)).sum(0).astype(np.uint16))
    for a in (t.result, t.reject_low, t.reject_high, t.coverage):
        a.setflags(write=False)
    return t


def truth(oracle, n, mode, n_active=None, sigmas=(SIGMA_LOW, SIGMA_HIGH)):
    """the maps of frames_of(n)[:n_active]; computed once"""
    key = (n, mode, n_active, sigmas)
    if key not in _truths:
        _truths[key] = truth_of(oracle, mode, np.ascontiguousarray(frames_of(n)[:n if n_active is None else n_active]), sigmas)
    return _truths[key]


def open_handle(nl, n, row0=0, rows=None, frames=frames_of):
    st = nl.StackHandle(n, W, H, row0=row0, rows=rows)
    st.upload_frames(frames(n))
    return st


def _assert_counts(got, t, rows):
    """both maps count for count, the totals their sums, no pixel with more rejections than samples"""
    _, cl, ch, low, high = got
    assert low.dtype == np.uint16 and high.dtype == np.uint16
    assert np.array_equal(low[rows], t.reject_low[rows]) and np.array_equal(high[rows], t.reject_high[rows])
    assert (cl, ch) == (int(low[rows].astype(np.int64).sum()), int(high[rows].astype(np.int64).sum()))
    assert (cl, ch) == (int(t.reject_low[rows].astype(np.int64).sum()), int(t.reject_high[rows].astype(np.int64).sum()))
    assert np.all(low[rows].astype(np.int64) + high[rows] <= t.coverage[rows])


def assert_exact_maps(got, t, rows=slice(None)):
    """got: what a maps pass returned on bit-exact kernels (the column kernel, the linear fit's); t: the truth; rows: the
    pixels to compare.  Bit for bit, count for count."""
    _assert_counts(got, t, rows)
    assert bits_equal(got[0][rows], t.result[rows])


def assert_fast_maps(got, t, rows=slice(None)):
    """... on the register-resident sigma engines: the result is the default pass's (util.RTOL), bit-exact on the pixels
    the exact kernel replays and on the pixel without data (whole-image indices of frames_of)"""
    _assert_counts(got, t, rows)
    out = got[0]
    assert close_values(out[rows], t.result[rows], RTOL)
    exact = np.zeros(P, bool)
    exact[list(INF_PIXELS) + [NO_DATA]] = True
    assert bits_equal(out[rows][exact[rows]], t.result[rows][exact[rows]])


def assert_deep_maps(got, t, rows=slice(None)):
    """... on the LDS-column sigma engines (the frames of deepmaps_frames): maps and totals count for count, the result
    within RTOL; the pixels that must be bit-exact are the caller's to name"""
    _assert_counts(got, t, rows)
    assert close_values(got[0][rows], t.result[rows], RTOL), ref_mismatch(got[0][rows], t.result[rows])


def ref_mismatch(got, want):
    ok = ~np.isnan(want) & (want != got)
    rel = np.abs(got[ok].astype(np.float64) - want[ok]) / np.abs(want[ok].astype(np.float64))
    return "%d pixels differ, largest relative difference %g" % (int(ok.sum()), rel.max(initial=0.0))


def is_fast_maps_name(name):
    return "stack_sigma_fast_kernel" in name and "maps" in name


def is_linfit_maps_name(name, n):
    return ("stack_linfit_fast_kernel" if n <= 128 else "stack_linfit_ml_kernel") in name and "maps" in name


def is_deep_maps_name(name):
    return "stack_sigma_mlz_kernel" in name and "maps" in name
