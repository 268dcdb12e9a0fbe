"""GPU: the per-pixel rejection maps of a maps pass and the coverage map (include/nlstack_maps.h) against the CPU oracle
called pixel by pixel (tests/rejmap_ref.py; tests/test_rejmap_ref.py holds that checker to the whole-image oracle).
Every comparison is exact equality: result bits, totals, both maps, coverage.  The shapes take every lane width of
exact_plan (64 / 32 / 16 / 4 pixels per wave) on pixel counts that are no multiple of it or of 64; the handle cases
are a shorter active frame count, a row tile writing into pre-filled whole-image buffers, a three-tile group on one
device, NULL host pointers, the weighted-MAD refusal, and a maps pass between two default passes."""
import ctypes as C

import numpy as np
import pytest

import rejmap_ref as ref
from maps_cases import assert_exact_maps as assert_maps
from nightlight_amd import capi
from util import bits_equal

pytestmark = pytest.mark.gpu

SL, SH, LOC = ref.SIGMA_LOW, ref.SIGMA_HIGH, ref.REF_LOC
N24 = {c.name: c for c in ref.CASES if c.frames == 24}
SIGMA24, MEAN24, MAD24 = N24["sigma-24x41x23"], N24["mean-24x41x23"], N24["mad-24x41x23"]


def open_handle(nl, case, row0=0, rows=None):
    st = nl.StackHandle(case.frames, case.width, case.height, row0=row0, rows=rows)
    st.upload_frames(ref.make_frames(case.frames, case.width, case.height))
    if case.weighted:
        st.set_weights(ref.weights_of(case.frames))
    return st


@pytest.mark.parametrize("case", ref.CASES, ids=[c.name for c in ref.CASES])
def test_maps_equal_the_oracle_pixel_by_pixel(nl, oracle, case):
    t = ref.truth(oracle, case)
    with open_handle(nl, case) as st:
        got = st.run_maps(case.mode, SL, SH, LOC)
        assert_maps(got, t)
        assert (got[1], got[2]) == (t.clip_low, t.clip_high)
        assert st.last_mode == case.mode
        name = st.last_kernel_name
        cov = st.coverage()
        assert st.last_kernel_name == name and st.last_mode == case.mode         # coverage is no pass
        assert st.last_coverage_ms > 0
    if case.mode == capi.ST_MEAN:
        assert name.startswith("stack_mean") and not got[3].any() and not got[4].any()
    else:
        assert name == "stack_exact_kernel<%s%s,maps>" % (ref.MODE_NAMES[case.mode], ",weighted" if case.weighted else "")
    if case.mode == capi.ST_MEDIAN:
        assert not got[3].any() and not got[4].any()
    assert cov.dtype == np.uint16 and np.array_equal(cov, t.coverage)
    assert np.all(got[3].astype(np.int64) + got[4] <= cov)
    assert got[3][3] == 0 and got[4][3] == 0 and cov[3] == 0 and got[0][3] == np.float32(LOC)       # the pixel without data


def test_active_frames_are_respected(nl, oracle):
    case, n = SIGMA24, 17
    t = ref.truth(oracle, case, n)
    with open_handle(nl, case) as st:
        st.set_active_frames(n)
        assert_maps(st.run_maps(case.mode, SL, SH, LOC), t)
        assert np.array_equal(st.coverage(), t.coverage)
        st.set_active_frames(case.frames)
        assert_maps(st.run_maps(case.mode, SL, SH, LOC), ref.truth(oracle, case))
        assert np.array_equal(st.coverage(), ref.truth(oracle, case).coverage)


def test_tile_handle_writes_only_its_rows(nl, oracle):
    case, row0, rows = SIGMA24, 5, 9
    t = ref.truth(oracle, case)
    p, w = case.width * case.height, case.width
    inside = slice(row0 * w, (row0 + rows) * w)
    out = np.full(p, np.float32(-7.5))
    low, high, cov = np.full(p, 0xABCD, np.uint16), np.full(p, 0x1234, np.uint16), np.full(p, 0x5555, np.uint16)
    with open_handle(nl, case, row0, rows) as st:
        got = st.run_maps(case.mode, SL, SH, LOC, out=out, reject_low=low, reject_high=high)
        assert got[0] is out and got[3] is low and got[4] is high
        assert_maps(got, t, inside)
        assert st.coverage(out=cov) is cov
    assert np.array_equal(cov[inside], t.coverage[inside])
    for a, fill in ((out, np.float32(-7.5)), (low, 0xABCD), (high, 0x1234), (cov, 0x5555)):
        assert np.all(a[:inside.start] == fill) and np.all(a[inside.stop:] == fill)


@pytest.mark.parametrize("parallel_finish", ["0", "1"])
@pytest.mark.parametrize("case", [SIGMA24, N24["winsor-weighted-24x41x23"]], ids=lambda c: c.name)
def test_three_tile_group_equals_the_single_handle(nl, oracle, monkeypatch, case, parallel_finish):
    monkeypatch.setenv("NL_GROUP_PARALLEL_FINISH", parallel_finish)      # the tiles finished in turn / on worker threads
    t = ref.truth(oracle, case)
    with nl.StackGroup(case.frames, case.width, case.height, devices=[0, 0, 0]) as g:
        assert g.size == 3
        g.upload_frames(ref.make_frames(case.frames, case.width, case.height))
        if case.weighted:
            g.set_weights(ref.weights_of(case.frames))
        got = g.run_maps(case.mode, SL, SH, LOC)
        assert_maps(got, t)
        assert (got[1], got[2]) == (t.clip_low, t.clip_high)
        assert np.array_equal(g.coverage(), t.coverage)
        assert g.tile(1).last_kernel_name.endswith(",maps>")


def test_mean_gives_zero_maps_and_the_mean(nl, oracle):
    t = ref.truth(oracle, MEAN24)
    low, high = np.full(t.result.size, 7, np.uint16), np.full(t.result.size, 9, np.uint16)
    with open_handle(nl, MEAN24) as st:
        got = st.run_maps(capi.ST_MEAN, SL, SH, LOC, reject_low=low, reject_high=high)
        assert st.last_kernel_name == "stack_mean_vec4_kernel"
    assert bits_equal(got[0], t.result) and (got[1], got[2]) == (0, 0)
    assert not low.any() and not high.any()


def test_null_host_pointers(nl, oracle):
    """any of the host pointers may be NULL: nothing is written, the result stays on the device"""
    case = SIGMA24
    t = ref.truth(oracle, case)
    L = capi.load()
    high = np.zeros(t.result.size, np.uint16)
    with open_handle(nl, case) as st:
        capi.check(L.nl_stack_run_maps(st._h, case.mode, SL, SH, LOC, None, None, None, None, None))
        assert bits_equal(st.result_tile(), t.result)
        ch = C.c_int64(-1)
        capi.check(L.nl_stack_run_maps(st._h, case.mode, SL, SH, LOC, None, None, C.byref(ch), None,
                                       high.ctypes.data_as(C.POINTER(C.c_uint16))))
        assert ch.value == t.clip_high and np.array_equal(high, t.reject_high)
        assert L.nl_stack_coverage(st._h, None) == capi.ERR_INVALID_ARG
        assert capi.last_error() == "coverage: null output"


def test_weighted_mad_and_invalid_mode_are_refused(nl, oracle):
    t = ref.truth(oracle, MAD24)
    with open_handle(nl, MAD24) as st:
        st.set_weights(ref.weights_of(MAD24.frames))
        with pytest.raises(capi.NlError) as e:
            st.run_maps(capi.ST_MAD_SIGMA, SL, SH, LOC)
        assert e.value.code == capi.ERR_WEIGHTED_MAD
        with pytest.raises(capi.NlError) as e:
            st.run_maps(9, SL, SH, LOC)
        assert e.value.code == capi.ERR_INVALID_MODE
        st.set_weights(None)                     # the handle is settled: the next pass is as any other
        assert_maps(st.run_maps(capi.ST_MAD_SIGMA, SL, SH, LOC), t)
    with nl.StackGroup(MAD24.frames, MAD24.width, MAD24.height, devices=[0, 0, 0]) as g:
        g.upload_frames(ref.make_frames(MAD24.frames, MAD24.width, MAD24.height))
        g.set_weights(ref.weights_of(MAD24.frames))
        with pytest.raises(capi.NlError) as e:
            g.run_maps(capi.ST_MAD_SIGMA, SL, SH, LOC)
        assert e.value.code == capi.ERR_WEIGHTED_MAD and "MADSigma" in e.value.message
        g.set_weights(None)
        assert_maps(g.run_maps(capi.ST_MAD_SIGMA, SL, SH, LOC), t)


def default_pass(st, mode):
    out, cl, ch = st.run(mode, SL, SH, LOC)
    return out.view(np.uint32).copy(), (cl, ch), st.last_kernel_name, st.last_pass_protocol


@pytest.mark.parametrize("mode", [capi.ST_SIGMA, capi.ST_WINSOR_SIGMA, capi.ST_LINEAR_FIT])
def test_a_maps_pass_leaves_default_passes_as_they_were(nl, oracle, mode):
    """default pass, maps pass, default pass: the two default passes agree in result bits, totals, kernel and protocol.
    (A handle's FIRST pass has no list lengths to go by and may run another protocol than its later ones -- with or
    without a maps pass in between, and depending on what the process ran before -- so one default pass runs in front
    of the three; the maps pass must also not have forced the bit-exact kernels on what follows.)"""
    case = [c for c in N24.values() if c.mode == mode and not c.weighted][0]
    t = ref.truth(oracle, case)
    with open_handle(nl, case) as st:
        default_pass(st, mode)
        before = default_pass(st, mode)
        assert_maps(st.run_maps(mode, SL, SH, LOC), t)
        assert st.last_pass_protocol == 0
        after = default_pass(st, mode)
        assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
        assert before[1] == (t.clip_low, t.clip_high) and "maps" not in after[2] and not after[2].startswith("stack_exact_kernel")
        # and the other way round: the maps pass is the same behind default passes as on a fresh handle
        assert_maps(st.run_maps(mode, SL, SH, LOC), t)
