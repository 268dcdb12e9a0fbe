"""GPU: the full maps pass (include/nlstack_fullmaps.h) -- nl_stack_run_maps_full / nl_group_run_maps_full -- on the frames
of tests/fullmaps_frames.py, whose conditions tests/test_fullmaps_frames.py asserts on the CPU.  MAD sigma runs the three
MAD kernels of the default pass in their MAPS instantiations: the maps and totals are compared with the oracle called
pixel by pixel, count for count; the result is the default pass's (within RTOL of the oracle, bit-equal to run() on a fresh
handle; bit-exact where the column kernel replays a pixel -- the four without a finite median -- and where a pixel has no
data).  The median runs its default kernels and gives zero maps.  Everything else is the pass of nl_stack_run_maps_deep.

Each pixel's word is written by one of up to three kernels -- the dominant kernel, from 114 frames on the finisher of the
bitonic kernel's hand-over list, the column kernel over the exact list -- so the cases insist on the lengths of the two
lists, and passes with different sigmas run in turn on one handle.  Every truth is computed once per key."""
import ctypes as C

import numpy as np
import pytest

import fullmaps_frames as full
import maps_cases as cases
import rejmap_ref as ref
from maps_cases import assert_deep_maps as assert_maps, ref_mismatch
from nightlight_amd import capi
from util import RTOL, bits_equal, close_values

pytestmark = pytest.mark.gpu

W, H, P = full.W, full.H, full.P
SIGMAS, TIGHT, REF_LOC = full.SIGMAS, full.TIGHT, full.REF_LOC
MAD, MEDIAN = capi.ST_MAD_SIGMA, capi.ST_MEDIAN
NO_SHARED_HINTS = 512       # developer switch: no list-length hints from earlier handles of the same geometry
COLUMN_MAD = "stack_exact_kernel<mad,maps>"


def open_handle(nl, n, row0=0, rows=None):
    return cases.open_handle(nl, n, row0, rows, frames=full.frames_of)


def full_pass(st, mode=MAD, sigmas=SIGMAS, **kw):
    return st.run_maps_full(mode, sigmas[0], sigmas[1], REF_LOC, **kw)


def is_mad_maps_name(name):
    return "stack_mad_" in name and "maps" in name


def expected_name(n):
    if n > 128:
        return "stack_mad_ml_kernel<%d, maps>" % (2 if n <= 256 else 4)
    if n >= 114:
        return "stack_mad_bitonic_kernel<maps>"
    return "stack_mad_fast_kernel<%d, maps>" % next(c for c in (8, 16, 32, 48, 64, 80, 96, 112, 128) if n <= c)


@pytest.mark.parametrize("n", full.DEPTHS)
def test_every_depth_equals_the_oracle_pixel_by_pixel(nl, oracle, n):
    t = full.truth(oracle, n, MAD)
    with open_handle(nl, n) as st:
        got = full_pass(st)
        name, protocol = st.last_kernel_name, st.last_pass_protocol
        fallback, generic = st.last_fallback_pixels, st.last_generic_pixels
        assert st.last_mode == MAD
    print("n %d: %s, generic list %d, exact list %d of %d pixels, totals %d / %d"
          % (n, name, generic, fallback, P, got[1], got[2]))
    assert_maps(got, t)
    assert (got[1], got[2]) == (t.clip_low, t.clip_high)
    for p in full.INF_PIXELS + (full.NO_DATA,):
        assert bits_equal(got[0][p:p + 1], t.result[p:p + 1]), p
        assert got[3][p] == 0 and got[4][p] == 0
    assert got[0][full.NO_DATA] == np.float32(REF_LOC) and t.coverage[full.NO_DATA] == 0
    assert is_mad_maps_name(name), name
    assert name == expected_name(n)
    assert protocol == 0
    assert fallback >= 3
    if 114 <= n <= 128:
        assert generic >= 60
        assert generic + fallback < P // 2


@pytest.mark.parametrize("n", [16, 128, 300])
def test_agrees_with_the_column_pass_and_the_default_pass(nl, oracle, n):
    with open_handle(nl, n) as st:
        got = full_pass(st)
        assert is_mad_maps_name(st.last_kernel_name)
        col = st.run_maps(MAD, SIGMAS[0], SIGMAS[1], REF_LOC)
        assert st.last_kernel_name == COLUMN_MAD
    assert np.array_equal(got[3], col[3]) and np.array_equal(got[4], col[4]) and (got[1], got[2]) == (col[1], col[2])
    assert close_values(got[0], col[0], RTOL), ref_mismatch(got[0], col[0])
    assert got[1] > 0 and got[2] > 0
    # the default pass on a fresh handle: the same kernels without the store, the same arithmetic
    with open_handle(nl, n) as st:
        st.set_dev_flags(NO_SHARED_HINTS)
        out, cl, ch = st.run(MAD, SIGMAS[0], SIGMAS[1], REF_LOC)
        assert st.last_kernel_name.startswith("stack_mad_") and "maps" not in st.last_kernel_name
    assert (cl, ch) == (got[1], got[2])
    assert bits_equal(out, got[0]), ref_mismatch(got[0], out)


@pytest.mark.parametrize("n", [120, 300])
def test_nothing_stale_and_nothing_twice(nl, oracle, n):
    """kappa 3 / 3, then 1.2 / 1.2, then 3 / 3 on one handle, a column pass and a default pass in between: each pass
    equals its own truth; with the host maps preset and no result asked for, every word is still written"""
    t, tight = full.truth(oracle, n, MAD), full.truth(oracle, n, MAD, sigmas=TIGHT)
    assert not np.array_equal(tight.reject_low, t.reject_low) and not np.array_equal(tight.reject_high, t.reject_high)
    L = capi.load()
    u16p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16))
    with open_handle(nl, n) as st:
        assert_maps(full_pass(st), t)
        assert_maps(full_pass(st, MAD, TIGHT), tight)
        assert is_mad_maps_name(st.last_kernel_name)
        assert_maps(full_pass(st), t)
        cases.assert_exact_maps(st.run_maps(MAD, TIGHT[0], TIGHT[1], REF_LOC), tight)      # the column pass in between
        assert st.last_kernel_name == COLUMN_MAD
        _, cl, ch = st.run(MAD, TIGHT[0], TIGHT[1], REF_LOC)                                   # ... and a default pass
        assert (cl, ch) == (tight.clip_low, tight.clip_high) and "maps" not in st.last_kernel_name
        low, high = np.full(P, 0xABCD, np.uint16), np.full(P, 0x1234, np.uint16)
        cl, ch = C.c_int64(-1), C.c_int64(-1)
        capi.check(L.nl_stack_run_maps_full(st._h, MAD, SIGMAS[0], SIGMAS[1], REF_LOC, None, C.byref(cl), C.byref(ch),
                                            u16p(low), u16p(high)))
        assert is_mad_maps_name(st.last_kernel_name)
        assert np.array_equal(low, t.reject_low) and np.array_equal(high, t.reject_high)
        assert (cl.value, ch.value) == (t.clip_low, t.clip_high)
        assert close_values(st.result_tile(), t.result, RTOL)


@pytest.mark.parametrize("n", [16, 128, 300])
def test_the_median_runs_its_own_kernels_and_zeroes_the_maps(nl, n):
    low, high = np.full(P, 7, np.uint16), np.full(P, 9, np.uint16)
    with open_handle(nl, n) as st:
        full_pass(st)                                    # a MAD maps pass first: its words must not show through
        got = full_pass(st, MEDIAN, reject_low=low, reject_high=high)
        name = st.last_kernel_name
        assert st.last_pass_protocol == 0 and st.last_mode == MEDIAN
        out, cl, ch = st.run(MEDIAN, SIGMAS[0], SIGMAS[1], REF_LOC)
        assert st.last_kernel_name == name
    print("n %d: %s" % (n, name))
    assert name.startswith("stack_median_fast_kernel" if n <= 128 else "stack_median_ml_kernel") and "stack_exact_kernel" not in name
    assert (got[1], got[2]) == (0, 0) == (cl, ch)
    assert got[3] is low and got[4] is high and not low.any() and not high.any()
    assert bits_equal(got[0], out)


def test_tile_handle_writes_only_its_rows(nl, oracle):
    n, row0, rows = 120, 5, 13                                   # rows 5 ... 17 of the 23
    t = full.truth(oracle, n, MAD)
    inside = slice(row0 * W, (row0 + rows) * W)
    assert inside.start <= full.NO_DATA and full.INF_PIXELS[-1] < inside.stop
    out = np.full(P, np.float32(-7.5))
    low, high = np.full(P, 0xABCD, np.uint16), np.full(P, 0x1234, np.uint16)
    with open_handle(nl, n, row0=row0, rows=rows) as st:
        got = full_pass(st, out=out, reject_low=low, reject_high=high)
        assert got[0] is out and got[3] is low and got[4] is high
        assert st.last_kernel_name == "stack_mad_bitonic_kernel<maps>"
        assert st.last_fallback_pixels >= 3 and st.last_generic_pixels >= 60
    assert_maps(got, t, inside)
    for a, fill in ((out, np.float32(-7.5)), (low, 0xABCD), (high, 0x1234)):
        assert np.all(a[:inside.start] == fill) and np.all(a[inside.stop:] == fill)


@pytest.mark.parametrize("n", [120, 300])
def test_two_tile_group_equals_the_single_handle(nl, oracle, n):
    t = full.truth(oracle, n, MAD)
    with open_handle(nl, n) as st:
        single = full_pass(st)
    with nl.StackGroup(n, W, H, devices=[0, 0]) as g:
        assert g.size == 2
        split = [g.tile(i).rows for i in range(2)]
        assert sum(split) == H and split[0] != split[1]          # 23 rows: an uneven split
        g.upload_frames(full.frames_of(n))
        got = g.run_maps_full(MAD, SIGMAS[0], SIGMAS[1], REF_LOC)
        assert all(is_mad_maps_name(g.tile(i).last_kernel_name) for i in range(2))
        med = g.run_maps_full(MEDIAN, SIGMAS[0], SIGMAS[1], REF_LOC)
        assert all("stack_median_" in g.tile(i).last_kernel_name for i in range(2))
    assert_maps(got, t)
    assert (got[1], got[2]) == (t.clip_low, t.clip_high) == (single[1], single[2])
    assert bits_equal(got[0], single[0]) and np.array_equal(got[3], single[3]) and np.array_equal(got[4], single[4])
    assert (med[1], med[2]) == (0, 0) and not med[3].any() and not med[4].any()


@pytest.mark.parametrize("what", ["forced-exact", "513-frames", "deep-entry"])
def test_fall_throughs_run_the_column_kernel(nl, what):
    """what the MAD engines do not take is the column kernel's pass, with the maps of nl_stack_run_maps"""
    if what == "513-frames":
        st = nl.StackHandle(513, 16, 8)
        st.upload_frames(ref.make_frames(513, 16, 8))
    else:
        st = open_handle(nl, 48)
    with st:
        if what == "forced-exact":
            st.set_exact(1)
        entry = st.run_maps_deep if what == "deep-entry" else st.run_maps_full
        got = entry(MAD, SIGMAS[0], SIGMAS[1], REF_LOC)
        assert st.last_kernel_name == COLUMN_MAD and st.last_pass_protocol == 0
        col = st.run_maps(MAD, SIGMAS[0], SIGMAS[1], REF_LOC)
        assert st.last_kernel_name == COLUMN_MAD
    assert bits_equal(got[0], col[0]) and (got[1], got[2]) == (col[1], col[2])
    assert np.array_equal(got[3], col[3]) and np.array_equal(got[4], col[4])
    assert got[1] > 0 and got[2] > 0


def test_weights_are_refused_and_the_handle_stays_usable(nl, oracle):
    n = 48
    with open_handle(nl, n) as st:
        st.set_weights(ref.weights_of(n))
        with pytest.raises(capi.NlError) as e:
            full_pass(st)
        assert e.value.code == capi.ERR_WEIGHTED_MAD and "MADSigma" in e.value.message
        with pytest.raises(capi.NlError) as e2:
            full_pass(st, 9)
        assert e2.value.code == capi.ERR_INVALID_MODE
        st.set_weights(None)
        assert_maps(full_pass(st), full.truth(oracle, n, MAD))
        assert st.last_kernel_name == "stack_mad_fast_kernel<48, maps>"


@pytest.mark.parametrize("what", ["sigma-48", "sigma-200", "linearfit-48", "linearfit-200", "mean-48"])
def test_the_other_modes_are_the_deep_pass(nl, what):
    """the kernel name and the results of run_maps_deep on the same handle (frames without an infinite sample)"""
    mode = {"sigma": capi.ST_SIGMA, "linearfit": capi.ST_LINEAR_FIT, "mean": capi.ST_MEAN}[what.split("-")[0]]
    n = int(what.split("-")[1])
    with cases.open_handle(nl, n) as st:
        got = full_pass(st, mode)
        name, protocol = st.last_kernel_name, st.last_pass_protocol
        deep = st.run_maps_deep(mode, SIGMAS[0], SIGMAS[1], REF_LOC)
        assert st.last_kernel_name == name and st.last_pass_protocol == protocol == 0
    print("%s: %s" % (what, name))
    if mode != capi.ST_MEAN:
        assert "maps" in name and "stack_exact_kernel" not in name and got[1] + got[2] > 0
    assert bits_equal(got[0], deep[0]) and (got[1], got[2]) == (deep[1], deep[2])
    assert np.array_equal(got[3], deep[3]) and np.array_equal(got[4], deep[4])


def default_pass(st):
    out, cl, ch = st.run(MAD, SIGMAS[0], SIGMAS[1], REF_LOC)
    return (out.view(np.uint32).copy(), (cl, ch), st.last_kernel_name, st.last_pass_protocol,
            st.last_fallback_pixels, st.last_generic_pixels)


@pytest.mark.parametrize("n", [64, 128, 300])
def test_a_full_maps_pass_leaves_default_passes_as_they_were(nl, oracle, n):
    """a default MAD pass behind a full maps pass is the same pass of a fresh handle that never ran one: result bits, totals,
    kernel name, protocol and both list lengths"""
    t = full.truth(oracle, n, MAD)
    with open_handle(nl, n) as st:
        st.set_dev_flags(NO_SHARED_HINTS)
        fresh = [default_pass(st), default_pass(st)]
    with open_handle(nl, n) as st:
        st.set_dev_flags(NO_SHARED_HINTS)
        assert_maps(full_pass(st), t)
        assert st.last_pass_protocol == 0 and is_mad_maps_name(st.last_kernel_name)
        after = [default_pass(st)]
        assert_maps(full_pass(st, MAD, TIGHT), full.truth(oracle, n, MAD, sigmas=TIGHT))
        after.append(default_pass(st))
    for k in range(2):
        assert np.array_equal(fresh[k][0], after[k][0]) and fresh[k][1:] == after[k][1:], k
        assert fresh[k][1] == (t.clip_low, t.clip_high)
        assert fresh[k][2].startswith("stack_mad_") and "maps" not in fresh[k][2] and fresh[k][3] == 0
