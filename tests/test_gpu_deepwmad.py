"""GPU: the deep weighted MAD-sigma pass (include/nlstack_deepwmad.h) -- nl_stack_run_mad_weighted_deepstack, its _async form
and nl_group_run_mad_weighted_deepstack -- on the frames of tests/deepstack_frames.py under the 2048 distinct weights of
tests/deepwmad_frames.py, whose conditions tests/test_deepwmad_frames.py asserts on the CPU.

The definition is nlstack_wmad.h's: every comparison with its restatement (wmad_ref.mad_clip) and with run_mad_weighted,
the column pass beyond 512 frames, is equality of bits and of counts.  513 ... 1024 frames run the record-only MAD kernel on
8 lanes per pixel, 1025 ... 2048 on 16, then the streaming kernel; the pixels it hands to the column kernel are the four
without a finite median and the one without data -- wmad_ref.handed_over's prediction for the streaming engine of
129 ... 512 frames (tests/test_gpu_wmad.py), which is the same engine behind another record kernel.  Every truth is
computed once per key."""
import numpy as np
import pytest

import deepstack_frames as deep
import deepwmad_frames as dw
import maps_cases as cases
import rejmap_ref as ref
import wmad_ref
from maps_cases import ref_mismatch
from nightlight_amd import capi
from util import RTOL, bits_equal, close_values

pytestmark = pytest.mark.gpu

W, H, P = deep.W, deep.H, deep.P
SIGMAS, TIGHT, REF_LOC = dw.SIGMAS, dw.TIGHT, dw.REF_LOC
MAD = capi.ST_MAD_SIGMA
NO_SHARED_HINTS = 512
COLUMN = wmad_ref.COLUMN_KERNEL


def open_handle(nl, n, row0=0, rows=None, weights=True):
    st = cases.open_handle(nl, n, row0, rows, frames=deep.frames_of)
    if weights:
        st.set_weights(dw.weights_of(n))
    return st


def deep_pass(st, sigmas=SIGMAS, **kw):
    return st.run_mad_weighted_deepstack(sigmas[0], sigmas[1], REF_LOC, **kw)


def is_streaming_name(name):
    return name.startswith(dw.STREAMING_KERNEL) and name.endswith(", true>")


def assert_pass(got, t, rows=slice(0, P)):
    out, cl, ch = got
    assert bits_equal(out[rows], t.result[rows]), ref_mismatch(out[rows], t.result[rows])
    assert (cl, ch) == dw.totals(t, rows)


@pytest.mark.parametrize("n", deep.DEPTHS)
def test_result_totals_kernel_and_handover_at_every_depth(nl, n):
    t = dw.truth(n)
    assert dw.handed_over(t) == 5 == wmad_ref.handed_over(t, 512)       # (the streaming engine's prediction)
    with open_handle(nl, n) as st:
        got = deep_pass(st)
        name, handed, protocol = st.last_kernel_name, st.last_fallback_pixels, st.last_pass_protocol
        assert st.last_mode == MAD
        column = st.run_mad_weighted(SIGMAS[0], SIGMAS[1], REF_LOC) if n in deep.TIGHT_DEPTHS else None
        assert column is None or (st.last_kernel_name == COLUMN and st.last_fallback_pixels == 0)
    print("n %d: %s, handed over %d, totals %d / %d" % (n, name, handed, got[1], got[2]))
    assert_pass(got, t)
    assert got[0][deep.NO_DATA] == np.float32(REF_LOC)
    assert is_streaming_name(name) and protocol == 0
    assert handed == 5
    if column is not None:
        assert bits_equal(got[0], column[0]), ref_mismatch(got[0], column[0])
        assert (got[1], got[2]) == (column[1], column[2])


def test_equal_weights_give_the_unweighted_pass(nl):
    n = 700
    with open_handle(nl, n, weights=False) as st:
        plain = st.run_deepstack(MAD, SIGMAS[0], SIGMAS[1], REF_LOC)
        st.set_weights(np.ones(n, np.float32))
        got = deep_pass(st)
        assert is_streaming_name(st.last_kernel_name)
    assert (got[1], got[2]) == (plain[1], plain[2]) and got[1] > 0 and got[2] > 0
    assert close_values(got[0], plain[0], RTOL), ref_mismatch(got[0], plain[0])


def test_async_form_is_finished_by_finish(nl):
    n = 700
    t = dw.truth(n)
    with open_handle(nl, n) as st:
        st.run_mad_weighted_deepstack_async(SIGMAS[0], SIGMAS[1], REF_LOC)
        out = np.zeros(P, np.float32)
        cl, ch = st.finish(out)
        whole, dominant = st.pass_times()
        assert is_streaming_name(st.last_kernel_name) and st.last_mode == MAD and 0 < dominant <= whole
        assert_pass((out, cl, ch), t)
        # ... and with the result left on the device, for the nl_stack_result_* steps
        none, cl, ch = deep_pass(st, fetch=False)
        assert none is None
        assert_pass((st.result_tile(), cl, ch), t)


def test_tile_handle_writes_only_its_rows(nl):
    n, row0, rows = 700, 5, 13                                   # rows 5 ... 17 of the 23
    t = dw.truth(n)
    inside = slice(row0 * W, (row0 + rows) * W)
    assert inside.start <= deep.NO_DATA and deep.INF_PIXELS[-1] < inside.stop
    with open_handle(nl, n, row0=row0, rows=rows) as st:
        out = np.full(P, np.float32(-7.5))
        got = deep_pass(st, out=out)
        assert got[0] is out and is_streaming_name(st.last_kernel_name) and st.last_fallback_pixels == 5
    assert_pass(got, t, inside)
    assert np.all(out[:inside.start] == np.float32(-7.5)) and np.all(out[inside.stop:] == np.float32(-7.5))


@pytest.mark.parametrize("n", deep.TIGHT_DEPTHS)
def test_two_tile_group_equals_the_single_handle(nl, n):
    t = dw.truth(n)
    with nl.StackGroup(n, W, H, devices=[0, 0]) as g:
        assert g.size == 2
        split = [g.tile(i).rows for i in range(2)]
        assert sum(split) == H and split[0] != split[1]          # 23 rows: an uneven split
        g.upload_frames(deep.frames_of(n))
        with pytest.raises(capi.NlError) as e:
            g.run_mad_weighted_deepstack(SIGMAS[0], SIGMAS[1], REF_LOC)
        assert e.value.code == capi.ERR_INVALID_ARG and "nl_stack_set_weights" in e.value.message
        g.set_weights(dw.weights_of(n))
        got = g.run_mad_weighted_deepstack(SIGMAS[0], SIGMAS[1], REF_LOC)
        assert all(is_streaming_name(g.tile(i).last_kernel_name) and g.tile(i).last_mode == MAD for i in range(2))
    assert_pass(got, t)


@pytest.mark.parametrize("n", deep.TIGHT_DEPTHS)
def test_nothing_stale(nl, n):
    """kappa 3 / 3, then 1.2 / 1.2, then 3 / 3 on one handle, a column pass and a default pass in between"""
    t, tight = dw.truth(n), dw.truth(n, TIGHT)
    assert dw.totals(tight) != dw.totals(t)
    with open_handle(nl, n) as st:
        assert_pass(deep_pass(st), t)
        assert_pass(deep_pass(st, TIGHT), tight)
        assert is_streaming_name(st.last_kernel_name) and st.last_fallback_pixels == 5
        assert_pass(st.run_mad_weighted(TIGHT[0], TIGHT[1], REF_LOC), tight)                  # the column pass in between
        assert st.last_kernel_name == COLUMN
        med, _, _ = st.run(capi.ST_MEDIAN, SIGMAS[0], SIGMAS[1], REF_LOC)                      # ... and a default pass
        assert st.last_mode == capi.ST_MEDIAN
        assert_pass(deep_pass(st), t)
        assert is_streaming_name(st.last_kernel_name) and st.last_fallback_pixels == 5 and st.last_pass_protocol == 0
        # the weights are read anew: other weights, another result, the same counters
        st.set_weights(np.ones(n, np.float32))
        flat = deep_pass(st)
        assert (flat[1], flat[2]) == dw.totals(t) and not bits_equal(flat[0], t.result)


def test_a_handle_without_weights_is_refused_as_run_mad_weighted_refuses_it(nl):
    n = 700
    with open_handle(nl, n, weights=False) as st:
        st.run(capi.ST_MEDIAN, 0.0, 0.0, REF_LOC)
        seen = []
        for call in (st.run_mad_weighted, st.run_mad_weighted_deepstack, st.run_mad_weighted_async,
                     st.run_mad_weighted_deepstack_async):
            with pytest.raises(capi.NlError) as e:
                call(SIGMAS[0], SIGMAS[1], REF_LOC)
            seen.append((e.value.code, e.value.message))
        assert seen[0][0] == capi.ERR_INVALID_ARG and "nl_stack_set_weights" in seen[0][1]
        assert seen[1] == seen[0] and seen[3] == seen[2] == seen[0]
        st.set_weights(dw.weights_of(n))                       # the handle is settled: the next pass is as any other
        assert_pass(deep_pass(st), dw.truth(n))


def fall_through_handle(nl, what):
    if what == "2049-frames":
        st = nl.StackHandle(2049, 16, 8)
        st.upload_frames(ref.make_frames(2049, 16, 8))
        st.set_weights(dw.weights_of(2049))
    elif what == "forced-exact-700":
        st = open_handle(nl, 700)
        st.set_exact(1)
    else:
        st = open_handle(nl, 400)
    st.set_dev_flags(NO_SHARED_HINTS)
    return st


@pytest.mark.parametrize("what", ["400-frames", "2049-frames", "forced-exact-700"])
def test_fall_throughs_are_run_mad_weighted(nl, what):
    """what the deep engine does not take is run_mad_weighted's pass, each entry on a fresh handle: result bits, totals, kernel
    name, protocol and the number of pixels handed over"""
    seen = {}
    for entry in ("run_mad_weighted", "run_mad_weighted_deepstack"):
        with fall_through_handle(nl, what) as st:
            out, cl, ch = getattr(st, entry)(SIGMAS[0], SIGMAS[1], REF_LOC)
            assert st.last_mode == MAD
            seen[entry] = (out.view(np.uint32).copy(), (cl, ch), st.last_kernel_name, st.last_pass_protocol,
                           st.last_fallback_pixels)
    base, got = seen["run_mad_weighted"], seen["run_mad_weighted_deepstack"]
    print("%s: %s, totals %r, handed over %d" % (what, base[2], base[1], base[4]))
    assert np.array_equal(got[0], base[0]) and got[1:] == base[1:]
    assert base[2] == COLUMN if what != "400-frames" else is_streaming_name(base[2])      # (400: the 129 ... 512 engine)
    assert base[1][0] + base[1][1] > 0
