"""GPU: the deep pass (include/nlstack_deepstack.h) -- nl_stack_run_deepstack / nl_group_run_deepstack -- on the frames of
tests/deepstack_frames.py, whose conditions and whose room for the tolerance tests/test_deepstack_frames.py asserts on the
CPU.  513 ... 1024 frames run the median and MAD-sigma kernels on 8 lanes per pixel, 1025 ... 2048 on 16.

The median is an order statistic: bit-equal to the oracle and to run(ST_MEDIAN) on the same handle, which keeps its
wave-per-pixel kernel.  A wrong cross-lane partner in any merge level gives wrong medians at once, at every depth.  MAD
sigma: the totals equal the oracle's count for count, the result is within RTOL of it (a mean of the same survivors in
another order of summation), bit-equal where the column kernel replays a pixel -- the four without a finite median -- and
where a pixel has no data.  Everything the engines do not take is run's pass on the same handle, kernel name and bits.
Every truth is computed once per key."""
import numpy as np
import pytest

import deepstack_frames as deep
import maps_cases as cases
import rejmap_ref as ref
from maps_cases import ref_mismatch
from nightlight_amd import capi
from util import RTOL, bits_equal, close_values

pytestmark = pytest.mark.gpu

W, H, P = deep.W, deep.H, deep.P
SIGMAS, TIGHT, REF_LOC = deep.SIGMAS, deep.TIGHT, deep.REF_LOC
MAD, MEDIAN = capi.ST_MAD_SIGMA, capi.ST_MEDIAN
NO_SHARED_HINTS = 512       # developer switch: no list-length hints from earlier handles of the same geometry
COOP_MEDIAN, COLUMN_MAD = "stack_median_coop_kernel", "stack_exact_kernel<mad>"
SPECIAL = deep.INF_PIXELS + (deep.NO_DATA,)


def open_handle(nl, n, row0=0, rows=None):
    return cases.open_handle(nl, n, row0, rows, frames=deep.frames_of)


def deep_pass(st, mode, sigmas=SIGMAS, **kw):
    return st.run_deepstack(mode, sigmas[0], sigmas[1], REF_LOC, **kw)


def default_pass(st, mode, sigmas=SIGMAS, **kw):
    return st.run(mode, sigmas[0], sigmas[1], REF_LOC, **kw)


def median_name(n):
    return "stack_median_ml_kernel<%d>" % deep.lanes_of(n)


def mad_name(n):
    return "stack_mad_ml_kernel<%d>" % deep.lanes_of(n)


def assert_mad(got, t, rows=None):
    """totals count for count, the result within RTOL, bit-equal at the pixels of the exact list and without data; `rows`:
    a tile's pixels (t is then the pixel-by-pixel truth with its maps)"""
    out, cl, ch = got
    if rows is None:
        assert (cl, ch) == (t.clip_low, t.clip_high)
        rows = slice(0, P)
    else:
        assert (cl, ch) == (int(t.reject_low[rows].astype(np.int64).sum()), int(t.reject_high[rows].astype(np.int64).sum()))
    assert close_values(out[rows], t.result[rows], RTOL), ref_mismatch(out[rows], t.result[rows])
    for p in SPECIAL:
        if rows.start <= p < rows.stop:
            assert bits_equal(out[p:p + 1], t.result[p:p + 1]), p


@pytest.mark.parametrize("n", deep.DEPTHS)
def test_median_is_bit_equal_at_every_depth(nl, oracle, n):
    t = deep.whole_truth(oracle, n, MEDIAN)
    with open_handle(nl, n) as st:
        out, cl, ch = deep_pass(st, MEDIAN)
        name, protocol = st.last_kernel_name, st.last_pass_protocol
        assert st.last_mode == MEDIAN
        base, bl, bh = default_pass(st, MEDIAN)
        assert st.last_kernel_name == COOP_MEDIAN
    print("n %d: %s" % (n, name))
    assert name == median_name(n) and protocol == 0
    assert (cl, ch) == (0, 0) == (bl, bh)
    assert bits_equal(out, t.result), ref_mismatch(out, t.result)
    assert bits_equal(out, base), ref_mismatch(out, base)
    assert out[deep.NO_DATA] == np.float32(REF_LOC)


@pytest.mark.parametrize("n", deep.DEPTHS)
def test_mad_equals_the_oracle_at_every_depth(nl, oracle, n):
    t = deep.whole_truth(oracle, n, MAD)
    with open_handle(nl, n) as st:
        got = deep_pass(st, MAD)
        name, protocol, fallback = st.last_kernel_name, st.last_pass_protocol, st.last_fallback_pixels
        assert st.last_mode == MAD
        base = default_pass(st, MAD)
        assert st.last_kernel_name == COLUMN_MAD
    ok = ~np.isnan(t.result) & np.isfinite(t.result) & (t.result != 0)
    worst = float(np.max(np.abs(got[0][ok].astype(np.float64) - t.result[ok]) / np.abs(t.result[ok].astype(np.float64))))
    print("n %d: %s, exact list %d of %d pixels, totals %d / %d, result within %.3g relative of the oracle (RTOL %.3g)"
          % (n, name, fallback, P, got[1], got[2], worst, RTOL))
    assert (got[1], got[2]) == (t.clip_low, t.clip_high) == (base[1], base[2])
    assert_mad(got, t)
    assert got[0][deep.NO_DATA] == np.float32(REF_LOC)
    assert name == mad_name(n) and protocol == 0
    assert fallback == len(deep.INF_PIXELS) == 4
    for p in SPECIAL:
        assert bits_equal(got[0][p:p + 1], base[0][p:p + 1]), p


@pytest.mark.parametrize("n", deep.TIGHT_DEPTHS)
def test_nothing_stale(nl, oracle, n):
    """kappa 3 / 3, then 1.2 / 1.2, then 3 / 3 on one handle, a default pass in between: each pass equals its own truth"""
    t, tight = deep.whole_truth(oracle, n, MAD), deep.whole_truth(oracle, n, MAD, sigmas=TIGHT)
    assert (tight.clip_low, tight.clip_high) != (t.clip_low, t.clip_high)
    with open_handle(nl, n) as st:
        assert_mad(deep_pass(st, MAD), t)
        assert_mad(deep_pass(st, MAD, TIGHT), tight)
        assert st.last_kernel_name == mad_name(n)
        _, cl, ch = default_pass(st, MAD, TIGHT)
        assert (cl, ch) == (tight.clip_low, tight.clip_high) and st.last_kernel_name == COLUMN_MAD
        assert_mad(deep_pass(st, MAD), t)
        assert st.last_kernel_name == mad_name(n) and st.last_fallback_pixels == 4
        med = deep_pass(st, MEDIAN)
        assert bits_equal(med[0], deep.whole_truth(oracle, n, MEDIAN).result) and (med[1], med[2]) == (0, 0)
        # ... and with the result left on the device, for the nl_stack_result_* steps
        none, cl, ch = deep_pass(st, MAD, TIGHT, fetch=False)
        assert none is None
        assert_mad((st.result_tile(), cl, ch), tight)


def observed(st, mode):
    out, cl, ch = default_pass(st, mode)
    return (out.view(np.uint32).copy(), (cl, ch), st.last_kernel_name, st.last_pass_protocol,
            st.last_fallback_pixels, st.last_generic_pixels)


@pytest.mark.parametrize("n", [700, 1500])
def test_deep_passes_leave_default_passes_as_they_were(nl, n):
    """a default MAD pass and a default median pass behind deep passes are the passes of a fresh handle that never ran one:
    result bits, totals, kernel name, protocol and both list lengths"""
    with open_handle(nl, n) as st:
        st.set_dev_flags(NO_SHARED_HINTS)
        fresh = [observed(st, MAD), observed(st, MEDIAN), observed(st, MAD)]
    with open_handle(nl, n) as st:
        st.set_dev_flags(NO_SHARED_HINTS)
        deep_pass(st, MAD)
        assert st.last_kernel_name == mad_name(n)
        after = [observed(st, MAD)]
        deep_pass(st, MEDIAN)
        assert st.last_kernel_name == median_name(n)
        after.append(observed(st, MEDIAN))
        deep_pass(st, MAD, TIGHT)
        after.append(observed(st, MAD))
    for k in range(3):
        assert np.array_equal(fresh[k][0], after[k][0]) and fresh[k][1:] == after[k][1:], k
    assert fresh[0][2] == COLUMN_MAD and fresh[1][2] == COOP_MEDIAN and fresh[0][3] == 0


def test_the_lane_count_follows_the_active_frames(nl):
    n = 1100
    with open_handle(nl, n) as st:
        for active, lanes in ((1000, 8), (1100, 16)):
            st.set_active_frames(active)
            med, count = deep.medians_of(deep.frames_of(n)[:active])
            listed = int(((count > 0) & ~np.isfinite(med)).sum())          # (fewer frames: fewer medians are infinite)
            assert 3 <= listed <= 4
            out, cl, ch = deep_pass(st, MEDIAN)
            assert st.last_kernel_name == "stack_median_ml_kernel<%d>" % lanes
            base, _, _ = default_pass(st, MEDIAN)
            assert st.last_kernel_name == COOP_MEDIAN and bits_equal(out, base), active
            got = deep_pass(st, MAD)
            assert st.last_kernel_name == "stack_mad_ml_kernel<%d>" % lanes and st.last_fallback_pixels == listed
            base = default_pass(st, MAD)
            assert st.last_kernel_name == COLUMN_MAD and (got[1], got[2]) == (base[1], base[2]) and got[1] > 0 and got[2] > 0
            # (the column kernel is the bit-exact replay of the reference: RTOL against it is RTOL against the oracle)
            assert close_values(got[0], base[0], RTOL), ref_mismatch(got[0], base[0])
        st.set_active_frames(400)
        for mode in (MEDIAN, MAD):
            got = deep_pass(st, mode)
            name = st.last_kernel_name
            base = default_pass(st, mode)
            assert st.last_kernel_name == name and "<4" in name, name
            assert bits_equal(got[0], base[0]) and got[1:] == base[1:]


def fall_through_handle(nl, what):
    if what == "2049-frames":
        st = nl.StackHandle(2049, 16, 8)
        st.upload_frames(ref.make_frames(2049, 16, 8))
    elif what == "forced-exact-700":
        st = open_handle(nl, 700)
        st.set_exact(1)
    else:
        st = cases.open_handle(nl, int(what.split("-")[1]))
    st.set_dev_flags(NO_SHARED_HINTS)
    return st


@pytest.mark.parametrize("what", ["2049-frames", "sigma-300", "sigma-600", "linearfit-600", "forced-exact-700"])
def test_fall_throughs_are_the_default_pass(nl, what):
    """What the deep engines do not take is run's pass in every observable respect: two passes through each entry, each on
    a fresh handle (the second pass of a sigma stack sizes its grids and picks its protocol from what the first left) --
    result bits, totals, kernel name, protocol and both list lengths, pass by pass"""
    modes = {"sigma": (capi.ST_SIGMA,), "linearfit": (capi.ST_LINEAR_FIT,)}.get(what.split("-")[0], (MEDIAN, MAD))
    for mode in modes:
        seen = {}
        for entry in ("run", "run_deepstack"):
            with fall_through_handle(nl, what) as st:
                seen[entry] = []
                for _ in range(2):
                    out, cl, ch = getattr(st, entry)(mode, SIGMAS[0], SIGMAS[1], REF_LOC)
                    assert st.last_mode == mode
                    seen[entry].append((out.view(np.uint32).copy(), (cl, ch), st.last_kernel_name, st.last_pass_protocol,
                                        st.last_fallback_pixels, st.last_generic_pixels))
        for k in range(2):
            base, got = seen["run"][k], seen["run_deepstack"][k]
            print("%s, mode %d, pass %d: %s, protocol %d" % (what, mode, k, base[2], base[3]))
            assert np.array_equal(got[0], base[0]) and got[1:] == base[1:], k
            assert "_ml_kernel<8>" not in base[2] and "_ml_kernel<16>" not in base[2]
            if mode != MEDIAN:
                assert base[1][0] + base[1][1] > 0


def test_weighted_mad_is_refused_and_the_median_ignores_weights(nl, oracle):
    n = 700
    t = deep.whole_truth(oracle, n, MAD)
    with open_handle(nl, n) as st:
        plain = deep_pass(st, MEDIAN)
        st.set_weights(ref.weights_of(n))
        with pytest.raises(capi.NlError) as e:
            deep_pass(st, MAD)
        assert e.value.code == capi.ERR_WEIGHTED_MAD and "MADSigma" in e.value.message
        with pytest.raises(capi.NlError) as e2:
            deep_pass(st, 9)
        assert e2.value.code == capi.ERR_INVALID_MODE
        weighted = deep_pass(st, MEDIAN)
        assert st.last_kernel_name == median_name(n) and bits_equal(weighted[0], plain[0])
        st.set_weights(None)
        assert_mad(deep_pass(st, MAD), t)
        assert st.last_kernel_name == mad_name(n)


def test_async_form_is_finished_by_finish(nl, oracle):
    n = 700
    t = deep.whole_truth(oracle, n, MAD)
    with open_handle(nl, n) as st:
        st.run_deepstack_async(MAD, SIGMAS[0], SIGMAS[1], REF_LOC)
        out = np.zeros(P, np.float32)
        cl, ch = st.finish(out)
        whole, dominant = st.pass_times()
        assert st.last_kernel_name == mad_name(n) and st.last_mode == MAD and 0 < dominant <= whole
    assert_mad((out, cl, ch), t)


def test_tile_handle_writes_only_its_rows(nl, oracle):
    n, row0, rows = 700, 5, 13                                   # rows 5 ... 17 of the 23
    t = deep.truth(oracle, n, MAD)
    inside = slice(row0 * W, (row0 + rows) * W)
    assert inside.start <= deep.NO_DATA and deep.INF_PIXELS[-1] < inside.stop
    with open_handle(nl, n, row0=row0, rows=rows) as st:
        out = np.full(P, np.float32(-7.5))
        got = deep_pass(st, MAD, out=out)
        assert got[0] is out and st.last_kernel_name == mad_name(n) and st.last_fallback_pixels == 4
        assert_mad(got, t, inside)
        assert np.all(out[:inside.start] == np.float32(-7.5)) and np.all(out[inside.stop:] == np.float32(-7.5))
        out = np.full(P, np.float32(-7.5))
        med = deep_pass(st, MEDIAN, out=out)
        assert st.last_kernel_name == median_name(n)
        assert bits_equal(med[0][inside], deep.whole_truth(oracle, n, MEDIAN).result[inside])
        assert np.all(out[:inside.start] == np.float32(-7.5)) and np.all(out[inside.stop:] == np.float32(-7.5))


@pytest.mark.parametrize("n", [700, 1500])
def test_two_tile_group_equals_the_single_handle(nl, n):
    with open_handle(nl, n) as st:
        single_med, single_mad = deep_pass(st, MEDIAN), deep_pass(st, MAD)
    with nl.StackGroup(n, W, H, devices=[0, 0]) as g:
        assert g.size == 2
        split = [g.tile(i).rows for i in range(2)]
        assert sum(split) == H and split[0] != split[1]          # 23 rows: an uneven split
        g.upload_frames(deep.frames_of(n))
        med = g.run_deepstack(MEDIAN, SIGMAS[0], SIGMAS[1], REF_LOC)
        assert all(g.tile(i).last_kernel_name == median_name(n) for i in range(2))
        mad = g.run_deepstack(MAD, SIGMAS[0], SIGMAS[1], REF_LOC)
        assert all(g.tile(i).last_kernel_name == mad_name(n) for i in range(2))
    assert bits_equal(med[0], single_med[0]) and (med[1], med[2]) == (0, 0)
    assert (mad[1], mad[2]) == (single_mad[1], single_mad[2]) and mad[1] > 0 and mad[2] > 0
    assert bits_equal(mad[0], single_mad[0]), ref_mismatch(mad[0], single_mad[0])
