"""GPU: the fast maps pass (include/nlstack_fastmaps.h) -- nl_stack_run_maps_fast / nl_group_run_maps_fast -- against
the CPU oracle called pixel by pixel (tests/rejmap_ref.py).  The maps and totals are exact equalities; the result is the
default pass's (util.RTOL), bit-exact on the pixels the exact kernel replays and on the pixel without data.  The frames
are those of tests/rejmap_ref.py with what sends pixels down the two hand-over paths: a block with half of its frames
missing and a block that clips more than a zone holds (generic pass), infinite samples (exact replay): tests/maps_cases.py
has them, their truths and the comparisons.  The image is 41 x 23 = 943 pixels: three full workgroups and a partial one,
no multiple of 64.  Every truth is computed once."""
import ctypes as C

import numpy as np
import pytest

import rejmap_ref as ref
from maps_cases import (H, HALF_NAN, INF_PIXELS, NO_DATA, P, REF_LOC, SIGMA_HIGH, SIGMA_LOW, W, assert_exact_maps,
                        assert_fast_maps, frames_of, is_fast_maps_name, open_handle, truth)
from nightlight_amd import capi
from util import RTOL, bits_equal, close_values

pytestmark = pytest.mark.gpu

FRAME_COUNTS = [5, 16, 17, 24, 33, 48, 64, 65, 100, 112, 127, 128]
MODES = [capi.ST_SIGMA, capi.ST_WINSOR_SIGMA]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", FRAME_COUNTS)
def test_every_network_equals_the_oracle_pixel_by_pixel(nl, oracle, n, mode):
    t = truth(oracle, n, mode)
    with open_handle(nl, n) as st:
        got = st.run_maps(mode, SIGMA_LOW, SIGMA_HIGH, REF_LOC, fast=True)
        name, protocol = st.last_kernel_name, st.last_pass_protocol
        fallback, generic = st.last_fallback_pixels, st.last_generic_pixels
        assert st.last_mode == mode
    print("n %d mode %d: %s, exact list %d, generic list %d, totals %d / %d" % (n, mode, name, fallback, generic, got[1], got[2]))
    assert_fast_maps(got, t)
    assert (got[1], got[2]) == (t.clip_low, t.clip_high)
    assert got[0][NO_DATA] == np.float32(REF_LOC) and got[3][NO_DATA] == 0 and got[4][NO_DATA] == 0 and t.coverage[NO_DATA] == 0
    assert is_fast_maps_name(name), name
    assert protocol == 0
    assert fallback >= 3
    if n >= 16:
        assert generic > 0


def test_no_stale_words(nl, oracle):
    n, mode = 24, capi.ST_SIGMA
    tight, t = truth(oracle, n, mode, sigmas=(1.2, 1.2)), truth(oracle, n, mode)
    assert not np.array_equal(tight.reject_low, t.reject_low) and not np.array_equal(tight.reject_high, t.reject_high)
    with open_handle(nl, n) as st:
        assert_fast_maps(st.run_maps(mode, 1.2, 1.2, REF_LOC, fast=True), tight)
        assert_fast_maps(st.run_maps(mode, SIGMA_LOW, SIGMA_HIGH, REF_LOC, fast=True), t)
        # column pass then fast pass, fast pass then column pass: each is its own truth
        assert_exact_maps(st.run_maps(mode, 1.2, 1.2, REF_LOC), tight)
        assert st.last_kernel_name == "stack_exact_kernel<sigma,maps>"
        assert_fast_maps(st.run_maps(mode, SIGMA_LOW, SIGMA_HIGH, REF_LOC, fast=True), t)
        assert is_fast_maps_name(st.last_kernel_name)
        assert_fast_maps(st.run_maps(mode, 1.2, 1.2, REF_LOC, fast=True), tight)
        assert_exact_maps(st.run_maps(mode, SIGMA_LOW, SIGMA_HIGH, REF_LOC), t)


@pytest.mark.parametrize("mode", MODES)
def test_active_frames_are_respected(nl, oracle, mode):
    with open_handle(nl, 128) as st:
        st.set_active_frames(100)
        assert_fast_maps(st.run_maps(mode, SIGMA_LOW, SIGMA_HIGH, REF_LOC, fast=True), truth(oracle, 128, mode, 100))
        assert is_fast_maps_name(st.last_kernel_name) and "<112," in st.last_kernel_name
        st.set_active_frames(128)
        assert_fast_maps(st.run_maps(mode, SIGMA_LOW, SIGMA_HIGH, REF_LOC, fast=True), truth(oracle, 128, mode))
        assert is_fast_maps_name(st.last_kernel_name) and "<128," in st.last_kernel_name


def test_tile_handle_writes_only_its_rows(nl, oracle):
    n, mode, row0, rows = 24, capi.ST_SIGMA, 5, 9
    t = truth(oracle, n, mode)
    inside = slice(row0 * W, (row0 + rows) * W)
    assert inside.start <= HALF_NAN.start and INF_PIXELS[-1] < inside.stop          # both hand-over paths inside the tile
    out = np.full(P, np.float32(-7.5))
    low, high = np.full(P, 0xABCD, np.uint16), np.full(P, 0x1234, np.uint16)
    with nl.StackHandle(n, W, H, row0=row0, rows=rows) as st:
        st.upload_frames(frames_of(n))
        got = st.run_maps(mode, SIGMA_LOW, SIGMA_HIGH, REF_LOC, out=out, reject_low=low, reject_high=high, fast=True)
        assert got[0] is out and got[3] is low and got[4] is high
        assert is_fast_maps_name(st.last_kernel_name)
    # (the exact pixels of assert_fast_maps are whole-image indices: compare the tile's rows by hand)
    assert np.array_equal(low[inside], t.reject_low[inside]) and np.array_equal(high[inside], t.reject_high[inside])
    assert (got[1], got[2]) == (int(t.reject_low[inside].astype(np.int64).sum()), int(t.reject_high[inside].astype(np.int64).sum()))
    assert close_values(out[inside], t.result[inside], RTOL)
    assert bits_equal(out[list(INF_PIXELS)], t.result[list(INF_PIXELS)])
    for a, fill in ((out, np.float32(-7.5)), (low, 0xABCD), (high, 0x1234)):
        assert np.all(a[:inside.start] == fill) and np.all(a[inside.stop:] == fill)


@pytest.mark.parametrize("parallel_finish", ["0", "1"])
@pytest.mark.parametrize("mode", MODES)
def test_three_tile_group_equals_the_single_handle(nl, oracle, monkeypatch, mode, parallel_finish):
    monkeypatch.setenv("NL_GROUP_PARALLEL_FINISH", parallel_finish)      # the tiles finished in turn / on worker threads
    n = 24
    t = truth(oracle, n, mode)
    with nl.StackGroup(n, W, H, devices=[0, 0, 0]) as g:
        assert g.size == 3
        g.upload_frames(frames_of(n))
        got = g.run_maps(mode, SIGMA_LOW, SIGMA_HIGH, REF_LOC, fast=True)
        assert_fast_maps(got, t)
        assert (got[1], got[2]) == (t.clip_low, t.clip_high)
        assert "maps" in g.tile(1).last_kernel_name and is_fast_maps_name(g.tile(1).last_kernel_name)


def default_pass(st, mode):
    out, cl, ch = st.run(mode, SIGMA_LOW, SIGMA_HIGH, REF_LOC)
    return (out.view(np.uint32).copy(), (cl, ch), st.last_kernel_name, st.last_pass_protocol, st.last_fallback_pixels,
            st.last_generic_pixels)


@pytest.mark.parametrize("n", [24, 128])
@pytest.mark.parametrize("mode", MODES)
def test_a_fast_maps_pass_leaves_default_passes_as_they_were(nl, oracle, mode, n):
    """default pass, default pass, fast maps pass, default pass: the second and the fourth agree in result bits, totals,
    kernel, protocol and both list lengths (the form of test_a_maps_pass_leaves_default_passes_as_they_were: a handle's
    FIRST pass has no list lengths to go by, so one default pass runs in front)."""
    t = truth(oracle, n, mode)
    with open_handle(nl, n) as st:
        default_pass(st, mode)
        before = default_pass(st, mode)
        assert_fast_maps(st.run_maps(mode, SIGMA_LOW, SIGMA_HIGH, REF_LOC, fast=True), t)
        assert st.last_pass_protocol == 0 and is_fast_maps_name(st.last_kernel_name)
        after = default_pass(st, mode)
        assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
        assert before[1] == (t.clip_low, t.clip_high) and "maps" not in after[2] and not after[2].startswith("stack_exact_kernel")
        # and the other way round: the fast maps pass is the same behind default passes as on a fresh handle
        assert_fast_maps(st.run_maps(mode, SIGMA_LOW, SIGMA_HIGH, REF_LOC, fast=True), t)


def both_ways(st, mode):
    fast = st.run_maps(mode, SIGMA_LOW, SIGMA_HIGH, REF_LOC, fast=True)
    fast_name = st.last_kernel_name
    column = st.run_maps(mode, SIGMA_LOW, SIGMA_HIGH, REF_LOC)
    assert st.last_kernel_name == fast_name
    assert bits_equal(fast[0], column[0]) and (fast[1], fast[2]) == (column[1], column[2])
    assert np.array_equal(fast[3], column[3]) and np.array_equal(fast[4], column[4])
    return fast, fast_name


@pytest.mark.parametrize("what", ["sigma-weighted", "mad", "linearfit", "median", "sigma-130", "sigma-forced-exact"])
def test_everything_else_runs_the_column_pass(nl, what):
    mode = {"mad": capi.ST_MAD_SIGMA, "linearfit": capi.ST_LINEAR_FIT, "median": capi.ST_MEDIAN}.get(what, capi.ST_SIGMA)
    if what == "sigma-130":
        st = nl.StackHandle(130, 24, 16)
        st.upload_frames(ref.make_frames(130, 24, 16))
    else:
        st = open_handle(nl, 24)
    with st:
        if what == "sigma-weighted":
            st.set_weights(ref.weights_of(24))
        if what == "sigma-forced-exact":
            st.set_exact(1)
        got, name = both_ways(st, mode)
    assert name == "stack_exact_kernel<%s%s,maps>" % (ref.MODE_NAMES[mode], ",weighted" if what == "sigma-weighted" else "")
    if mode != capi.ST_MEDIAN:
        assert got[1] + got[2] > 0


def test_mean_and_refusals(nl, oracle):
    n = 24
    rc, want, _, _, _ = oracle.stack_apply(capi.ST_MEAN, np.ascontiguousarray(frames_of(n)), None, SIGMA_LOW, SIGMA_HIGH, REF_LOC)
    assert rc == 0
    low, high = np.full(P, 7, np.uint16), np.full(P, 9, np.uint16)
    with open_handle(nl, n) as st:
        got = st.run_maps(capi.ST_MEAN, SIGMA_LOW, SIGMA_HIGH, REF_LOC, reject_low=low, reject_high=high, fast=True)
        assert st.last_kernel_name == "stack_mean_vec4_kernel"
        assert bits_equal(got[0], want) and (got[1], got[2]) == (0, 0)
        assert not low.any() and not high.any()
        st.set_weights(ref.weights_of(n))
        with pytest.raises(capi.NlError) as e:
            st.run_maps(capi.ST_MAD_SIGMA, SIGMA_LOW, SIGMA_HIGH, REF_LOC, fast=True)
        assert e.value.code == capi.ERR_WEIGHTED_MAD and "MADSigma" in e.value.message
        with pytest.raises(capi.NlError) as e:
            st.run_maps(9, SIGMA_LOW, SIGMA_HIGH, REF_LOC, fast=True)
        assert e.value.code == capi.ERR_INVALID_MODE
        st.set_weights(None)                     # the handle is settled: the next pass is as any other
        assert_fast_maps(st.run_maps(capi.ST_SIGMA, SIGMA_LOW, SIGMA_HIGH, REF_LOC, fast=True), truth(oracle, n, capi.ST_SIGMA))
        assert is_fast_maps_name(st.last_kernel_name)


def test_null_host_pointers(nl, oracle):
    """any of the host pointers may be NULL: nothing is written, the result stays on the device"""
    n, mode = 24, capi.ST_SIGMA
    t = truth(oracle, n, mode)
    L = capi.load()
    high = np.zeros(P, np.uint16)
    with open_handle(nl, n) as st:
        capi.check(L.nl_stack_run_maps_fast(st._h, mode, SIGMA_LOW, SIGMA_HIGH, REF_LOC, None, None, None, None, None))
        assert is_fast_maps_name(st.last_kernel_name)
        assert close_values(st.result_tile(), t.result, RTOL)
        ch = C.c_int64(-1)
        capi.check(L.nl_stack_run_maps_fast(st._h, mode, SIGMA_LOW, SIGMA_HIGH, REF_LOC, None, None, C.byref(ch), None,
                                            high.ctypes.data_as(C.POINTER(C.c_uint16))))
        assert ch.value == t.clip_high and np.array_equal(high, t.reject_high)
