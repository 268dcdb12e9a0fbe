"""GPU: the resident maps pass (include/nlstack_residentmaps.h) -- nl_stack_run_maps_resident /
nl_group_run_maps_resident -- against the CPU oracle called pixel by pixel (tests/rejmap_ref.py).  For the linear fit
everything is an exact equality: both kernels are bit-exact, so the result is compared bit for bit, the maps count for
count.  The frames are those of tests/test_gpu_fastmaps.py (tests/maps_cases.py): rejmap_ref's with a
block whose upper half of the frames is missing, a block with ten samples of +400, and three infinite samples, which go
to the exact list.  The image is 41 x 23 = 943 pixels: three full workgroups and a partial one, no multiple of 64.
Every truth is computed once per key.

What is particular to this pass is that a pixel's word of the map is built across the stages of the linear fit's
cascade -- stored by the first stage, added to by the later ones -- so the tests insist that the cascade really ran
(nl_stack_linfit_stage_counts), and run passes with different sigmas in turn on one handle: a word that survived from
an earlier pass, or one that was added to twice, would show."""
import ctypes as C

import numpy as np
import pytest

import maps_cases as cases
import rejmap_ref as ref
from maps_cases import (H, HALF_NAN, INF_PIXELS, NO_DATA, P, REF_LOC, SIGMA_HIGH, SIGMA_LOW, TIGHT, W, assert_exact_maps,
                        frames_of, is_fast_maps_name, is_linfit_maps_name, open_handle)
from nightlight_amd import capi
from util import RTOL, bits_equal, close_values

pytestmark = pytest.mark.gpu

LINFIT = capi.ST_LINEAR_FIT
# every with_class size of the one-lane kernel and both sides of each boundary (8 | 16 | 32 | 48 | 64 | 96 | 128; the
# parked 128 class from 97), both lane counts of the multi-lane kernel (2 up to 256 frames, then 4)
ONE_LANE = [5, 8, 9, 16, 17, 24, 32, 33, 48, 49, 64, 65, 96, 97, 112, 128]
MULTI_LANE = [129, 200, 257, 300]


def truth(oracle, n, mode=LINFIT, n_active=None, sigmas=(SIGMA_LOW, SIGMA_HIGH)):
    return cases.truth(oracle, n, mode, n_active, sigmas)


def resident(st, sigmas=(SIGMA_LOW, SIGMA_HIGH), mode=LINFIT, **kw):
    return st.run_maps_resident(mode, sigmas[0], sigmas[1], REF_LOC, **kw)


def column(st, sigmas=(SIGMA_LOW, SIGMA_HIGH), mode=LINFIT):
    return st.run_maps(mode, sigmas[0], sigmas[1], REF_LOC)


@pytest.mark.parametrize("n", ONE_LANE + MULTI_LANE)
def test_every_class_equals_the_oracle_pixel_by_pixel(nl, oracle, n):
    t = truth(oracle, n)
    with open_handle(nl, n) as st:
        got = resident(st)
        name, protocol, fallback = st.last_kernel_name, st.last_pass_protocol, st.last_fallback_pixels
        counts = st.linfit_stage_counts
        assert st.last_mode == LINFIT
    print("n %d: %s, exact list %d, stages %r, totals %d / %d" % (n, name, fallback, counts, got[1], got[2]))
    assert_exact_maps(got, t)
    assert (got[1], got[2]) == (t.clip_low, t.clip_high)
    assert got[0][NO_DATA] == np.float32(REF_LOC) and got[3][NO_DATA] == 0 and got[4][NO_DATA] == 0 and t.coverage[NO_DATA] == 0
    assert is_linfit_maps_name(name, n), name
    assert protocol == 0
    assert fallback >= 3
    # the cascade really ran: pixels went past the first / second / third stage, so their words were added to
    assert len(counts) >= 3
    if n >= 16:
        assert counts[0] > 0
    if n >= 24:
        assert counts[1] > 0
    if n >= 48:
        assert counts[2] > 0


@pytest.mark.parametrize("n", [24, 128, 200])
def test_agrees_with_the_column_pass_bit_for_bit(nl, oracle, n):
    with open_handle(nl, n) as st:
        res = resident(st)
        assert is_linfit_maps_name(st.last_kernel_name, n)
        col = column(st)
        assert st.last_kernel_name == "stack_exact_kernel<linearfit,maps>"
    assert bits_equal(res[0], col[0]) and (res[1], res[2]) == (col[1], col[2])
    assert np.array_equal(res[3], col[3]) and np.array_equal(res[4], col[4])
    assert res[1] + res[2] > 0


def test_no_stale_or_double_counted_words(nl, oracle):
    """Later stages load, add and store: a word an earlier pass left -- resident or column -- must never be what they add to"""
    n = 64
    tight, t = truth(oracle, n, sigmas=TIGHT), truth(oracle, n)
    assert not np.array_equal(tight.reject_low, t.reject_low) and not np.array_equal(tight.reject_high, t.reject_high)
    with open_handle(nl, n) as st:
        assert_exact_maps(resident(st, TIGHT), tight)
        assert st.linfit_stage_counts[0] > 0
        assert_exact_maps(resident(st), t)
        assert_exact_maps(column(st, TIGHT), tight)
        assert st.last_kernel_name == "stack_exact_kernel<linearfit,maps>"
        assert_exact_maps(resident(st), t)
        assert is_linfit_maps_name(st.last_kernel_name, n) and st.linfit_stage_counts[2] > 0
        assert_exact_maps(resident(st, TIGHT), tight)
        assert_exact_maps(column(st), t)


def test_active_frames_are_respected(nl, oracle):
    with open_handle(nl, 128) as st:
        st.set_active_frames(100)
        assert_exact_maps(resident(st), truth(oracle, 128, n_active=100))
        assert is_linfit_maps_name(st.last_kernel_name, 100) and "<128," in st.last_kernel_name
        st.set_active_frames(40)
        assert_exact_maps(resident(st), truth(oracle, 128, n_active=40))
        assert is_linfit_maps_name(st.last_kernel_name, 40) and "<48," in st.last_kernel_name


def test_tile_handle_writes_only_its_rows(nl, oracle):
    n, row0, rows = 48, 5, 9
    t = truth(oracle, n)
    inside = slice(row0 * W, (row0 + rows) * W)
    assert inside.start <= HALF_NAN.start and INF_PIXELS[-1] < inside.stop          # the exact list inside the tile
    out = np.full(P, np.float32(-7.5))
    low, high = np.full(P, 0xABCD, np.uint16), np.full(P, 0x1234, np.uint16)
    with nl.StackHandle(n, W, H, row0=row0, rows=rows) as st:
        st.upload_frames(frames_of(n))
        got = resident(st, out=out, reject_low=low, reject_high=high)
        assert got[0] is out and got[3] is low and got[4] is high
        assert is_linfit_maps_name(st.last_kernel_name, n)
    assert_exact_maps(got, t, inside)
    for a, fill in ((out, np.float32(-7.5)), (low, 0xABCD), (high, 0x1234)):
        assert np.all(a[:inside.start] == fill) and np.all(a[inside.stop:] == fill)


@pytest.mark.parametrize("parallel_finish", ["0", "1"])
def test_three_tile_group_equals_the_single_handle(nl, oracle, monkeypatch, parallel_finish):
    monkeypatch.setenv("NL_GROUP_PARALLEL_FINISH", parallel_finish)      # the tiles finished in turn / on worker threads
    n = 48
    t = truth(oracle, n)
    with open_handle(nl, n) as st:
        single = resident(st)
    with nl.StackGroup(n, W, H, devices=[0, 0, 0]) as g:
        assert g.size == 3
        g.upload_frames(frames_of(n))
        got = g.run_maps_resident(LINFIT, SIGMA_LOW, SIGMA_HIGH, REF_LOC)
        assert is_linfit_maps_name(g.tile(1).last_kernel_name, n)
    assert_exact_maps(got, t)
    assert (got[1], got[2]) == (t.clip_low, t.clip_high) == (single[1], single[2])
    assert bits_equal(got[0], single[0]) and np.array_equal(got[3], single[3]) and np.array_equal(got[4], single[4])


def default_pass(st):
    out, cl, ch = st.run(LINFIT, SIGMA_LOW, SIGMA_HIGH, REF_LOC)
    return (out.view(np.uint32).copy(), (cl, ch), st.last_kernel_name, st.last_pass_protocol, st.last_fallback_pixels,
            st.linfit_stage_counts)


@pytest.mark.parametrize("n", [24, 128])
def test_a_resident_maps_pass_leaves_default_passes_as_they_were(nl, oracle, n):
    """default, default, resident maps, default: the second and the fourth agree in result bits, totals, kernel name,
    protocol, exact-list length and stage counts"""
    t = truth(oracle, n)
    with open_handle(nl, n) as st:
        default_pass(st)
        before = default_pass(st)
        assert_exact_maps(resident(st), t)
        assert st.last_pass_protocol == 0 and is_linfit_maps_name(st.last_kernel_name, n)
        maps_counts = st.linfit_stage_counts
        after = default_pass(st)
    assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
    assert before[1] == (t.clip_low, t.clip_high) and bits_equal(before[0].view(np.float32), t.result)
    assert "stack_linfit_fast_kernel" in after[2] and "maps" not in after[2]
    assert maps_counts == before[5]                 # the same cascade: stage for stage the same pixels


@pytest.mark.parametrize("mode", [capi.ST_SIGMA, capi.ST_WINSOR_SIGMA])
def test_sigma_and_winsorized_run_the_fast_maps_pass(nl, mode):
    with open_handle(nl, 24) as st:
        fast = st.run_maps(mode, SIGMA_LOW, SIGMA_HIGH, REF_LOC, fast=True)
        fast_name = st.last_kernel_name
        res = resident(st, mode=mode)
        assert st.last_kernel_name == fast_name and is_fast_maps_name(fast_name)
        assert st.last_pass_protocol == 0
    assert np.array_equal(res[3], fast[3]) and np.array_equal(res[4], fast[4]) and (res[1], res[2]) == (fast[1], fast[2])
    assert close_values(res[0], fast[0], RTOL)
    assert res[1] + res[2] > 0


@pytest.mark.parametrize("what", ["median", "mad", "sigma-130", "linearfit-forced-exact", "sigma-forced-exact",
                                  "sigma-weighted", "winsor-weighted"])
def test_everything_else_runs_the_column_pass(nl, what):
    mode = {"median": capi.ST_MEDIAN, "mad": capi.ST_MAD_SIGMA, "linearfit-forced-exact": LINFIT,
            "winsor-weighted": capi.ST_WINSOR_SIGMA}.get(what, capi.ST_SIGMA)
    if what == "sigma-130":
        st = nl.StackHandle(130, 24, 16)
        st.upload_frames(ref.make_frames(130, 24, 16))
    else:
        st = open_handle(nl, 24)
    weighted = what.endswith("-weighted")
    with st:
        if weighted:
            st.set_weights(ref.weights_of(24))
        if what.endswith("-forced-exact"):
            st.set_exact(1)
        res = resident(st, mode=mode)
        res_name = st.last_kernel_name
        col = column(st, mode=mode)
        assert st.last_kernel_name == res_name
    assert res_name == "stack_exact_kernel<%s%s,maps>" % (ref.MODE_NAMES[mode], ",weighted" if weighted else "")
    assert bits_equal(res[0], col[0]) and (res[1], res[2]) == (col[1], col[2])
    assert np.array_equal(res[3], col[3]) and np.array_equal(res[4], col[4])
    if mode != capi.ST_MEDIAN:
        assert res[1] + res[2] > 0


def test_weights_on_the_handle_are_dropped_by_the_linear_fit(nl, oracle):
    """as through nl_stack_run and nl_stack_run_maps (stack.go:158): the unweighted fit, here on the resident engine"""
    n = 24
    t = truth(oracle, n)
    with open_handle(nl, n) as st:
        st.set_weights(ref.weights_of(n))
        res = resident(st)
        assert is_linfit_maps_name(st.last_kernel_name, n)
        col = column(st)
        assert st.last_kernel_name == "stack_exact_kernel<linearfit,maps>"
    assert_exact_maps(res, t)
    assert_exact_maps(col, t)


def test_mean_and_refusals(nl, oracle):
    n = 24
    rc, want, _, _, _ = oracle.stack_apply(capi.ST_MEAN, np.ascontiguousarray(frames_of(n)), None, SIGMA_LOW, SIGMA_HIGH, REF_LOC)
    assert rc == 0
    low, high = np.full(P, 7, np.uint16), np.full(P, 9, np.uint16)
    with open_handle(nl, n) as st:
        got = resident(st, mode=capi.ST_MEAN, reject_low=low, reject_high=high)
        assert st.last_kernel_name == "stack_mean_vec4_kernel"
        assert bits_equal(got[0], want) and (got[1], got[2]) == (0, 0)
        assert not low.any() and not high.any()
        st.set_weights(ref.weights_of(n))
        codes = []
        for entry in (st.run_maps_resident, st.run_maps):
            with pytest.raises(capi.NlError) as e:
                entry(capi.ST_MAD_SIGMA, SIGMA_LOW, SIGMA_HIGH, REF_LOC)
            assert e.value.code == capi.ERR_WEIGHTED_MAD and "MADSigma" in e.value.message
            with pytest.raises(capi.NlError) as e2:
                entry(9, SIGMA_LOW, SIGMA_HIGH, REF_LOC)
            assert e2.value.code == capi.ERR_INVALID_MODE
            codes.append((e.value.code, e.value.message, e2.value.code, e2.value.message))
        assert codes[0] == codes[1]
        st.set_weights(None)                     # the handle is settled: the next pass is as any other
        assert_exact_maps(resident(st), truth(oracle, n))
        assert is_linfit_maps_name(st.last_kernel_name, n)


def test_null_host_pointers(nl, oracle):
    """any of the host pointers may be NULL: nothing is written, the result stays on the device"""
    n = 24
    t = truth(oracle, n)
    L = capi.load()
    high = np.zeros(P, np.uint16)
    with open_handle(nl, n) as st:
        capi.check(L.nl_stack_run_maps_resident(st._h, LINFIT, SIGMA_LOW, SIGMA_HIGH, REF_LOC, None, None, None, None, None))
        assert is_linfit_maps_name(st.last_kernel_name, n)
        assert bits_equal(st.result_tile(), t.result)
        ch = C.c_int64(-1)
        capi.check(L.nl_stack_run_maps_resident(st._h, LINFIT, SIGMA_LOW, SIGMA_HIGH, REF_LOC, None, None, C.byref(ch), None,
                                                high.ctypes.data_as(C.POINTER(C.c_uint16))))
        assert ch.value == t.clip_high and np.array_equal(high, t.reject_high)
