"""GPU: the weighted MAD-sigma pass whose weights follow their frames (include/nlstack_wmad.h, an extension) against the
fp32 restatement of its definition (tests/wmad_ref.py; tests/test_wmad_ref.py pins that checker to the CPU oracle).
Every comparison is equality of bits: the result, the two totals (also against run(ST_MAD_SIGMA) on the same handle with
the weights removed), the kernel's name, and the number of pixels handed to the column kernel -- an equality with the
checker's prediction, so that the column kernel cannot quietly do another engine's work.  1 ... 113 frames run the
register-resident kernel of the network size, 114 ... 128 the selection kernel, 129 ... 512 the record-only multi-lane
kernel and the streaming kernel, 513 the column kernel.

The one place where "equal" is not "equal bits": a result that is NaN by the definition (an empty K at sigma 0, an
infinite sample in K) -- the sign and payload of the NaN a division makes are the hardware's, so the adversarial cases
compare NaN with NaN and everything else bit for bit.  The generic cases have no NaN result and compare bits
throughout."""
import numpy as np
import pytest

import wmad_ref as ref
from nightlight_amd import capi
from util import bits_equal

pytestmark = pytest.mark.gpu

LOC = ref.REF_LOC
MAD = capi.ST_MAD_SIGMA
C24, C128, C200 = ref.ADVERSARIAL


def open_handle(nl, case, n=None, row0=0, rows=None, weights=True):
    n = case.frames if n is None else n
    st = nl.StackHandle(n, case.width, case.height, row0=row0, rows=rows)
    st.upload_frames(ref.make_frames(case)[:n])
    if weights:
        st.set_weights(ref.weights_of(n))
    return st


def totals(t, rows=slice(None)):
    return int(t.clip_low[rows].sum()), int(t.clip_high[rows].sum())


def bits_equal_or_both_nan(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and bits_equal(got[~nan], want[~nan])


def check_pass(st, case, t, n_active=None, sigmas=None, equal=bits_equal, vec=False, exact=False):
    """one pass on `st` equals the truth `t` in bits and totals, runs the predicted kernel and hands over exactly the
    predicted number of pixels; returns the result"""
    n = case.frames if n_active is None else n_active
    sl, sh = (case.kappa, case.kappa) if sigmas is None else sigmas
    out, cl, ch = st.run_mad_weighted(sl, sh, LOC)
    name, handed = st.last_kernel_name, st.last_fallback_pixels
    print("%s (%d active) sigmas %r: totals %r, kernel %s, handed over %d of %d (predicted %d)"
          % (case.name, n, (sl, sh), (cl, ch), name, handed, t.result.size, ref.handed_over(t, n, exact)))
    assert equal(out, t.result)
    assert (cl, ch) == totals(t)
    assert st.last_mode == MAD
    assert name == ref.kernel_name(n, vec, exact)
    assert handed == ref.handed_over(t, n, exact)
    return out


@pytest.mark.parametrize("case", ref.CASES, ids=[c.name for c in ref.CASES])
def test_result_totals_kernel_and_handover(nl, case):
    t = ref.truth(case)
    assert not np.isnan(t.result).any()
    with open_handle(nl, case) as st:
        out = check_pass(st, case, t)
        # the rejection ignores the weights: the same totals from the unweighted MAD pass on the same handle
        st.set_weights(None)
        _, cl, ch = st.run(MAD, case.kappa, case.kappa, LOC)
        assert (cl, ch) == totals(t)
        # ... and with weights the default entry keeps refusing the mode
        st.set_weights(ref.weights_of(case.frames))
        with pytest.raises(capi.NlError) as e:
            st.run(MAD, case.kappa, case.kappa, LOC)
        assert e.value.code == capi.ERR_WEIGHTED_MAD
    p = case.width * case.height
    assert t.n[p // 2] == 0 and out[p // 2] == np.float32(LOC)          # the pixel without data
    assert t.n[p // 2 + 7] == 1
    if case.frames >= 2:
        assert t.n[p // 2 + 9] == 2


@pytest.mark.parametrize("sigmas", ref.ADVERSARIAL_SIGMAS, ids=lambda s: "%g,%g" % s)
@pytest.mark.parametrize("case", ref.ADVERSARIAL, ids=lambda c: c.name)
def test_adversarial_case(nl, case, sigmas):
    """integer samples with ties at the bounds, minority infinities, and the three pixels without a finite median
    (+Inf, -Inf, NaN), which the column kernel takes"""
    t = ref.truth(case, sigmas=sigmas)
    assert t.degenerate.sum() == 3
    with open_handle(nl, case) as st:
        out = check_pass(st, case, t, sigmas=sigmas, equal=bits_equal_or_both_nan)
        st.set_weights(None)
        _, cl, ch = st.run(MAD, sigmas[0], sigmas[1], LOC)
        assert (cl, ch) == totals(t)
    assert out[ref.PX_MOST_POS_INF] == np.float32(np.inf) and out[ref.PX_MOST_NEG_INF] == np.float32(-np.inf)
    assert np.isnan(out[ref.PX_HALF_HALF])
    assert np.isfinite(out[ref.PX_FEW_POS_INF]) and np.isfinite(out[ref.PX_FEW_NEG_INF])


@pytest.mark.parametrize("case", [ref.BY_FRAMES[17], ref.BY_FRAMES[128], ref.BY_FRAMES[257], C24, C200], ids=lambda c: c.name)
def test_forced_column_engine_equals_the_default_engine(nl, case):
    t = ref.truth(case)
    equal = bits_equal_or_both_nan if case in ref.ADVERSARIAL else bits_equal
    with open_handle(nl, case) as st:
        default = check_pass(st, case, t, equal=equal)
        st.set_exact(1)
        forced = check_pass(st, case, t, equal=equal, exact=True)
        assert st.last_kernel_name == ref.COLUMN_KERNEL and st.last_fallback_pixels == 0
        assert equal(default, forced)
        st.set_exact(0)
        check_pass(st, case, t, equal=equal)


def test_four_pixels_per_lane_and_the_tail(nl, monkeypatch):
    """a frame stride of 2257 + 3 floats: 16-byte loads, four pixels per lane, and one tail pixel for the scalar kernel"""
    monkeypatch.setenv("NL_STRIDE_PAD", "3")
    for case in (ref.C200, C200):
        equal = bits_equal_or_both_nan if case in ref.ADVERSARIAL else bits_equal
        with open_handle(nl, case) as st:
            check_pass(st, case, ref.truth(case), vec=True, equal=equal)


def test_active_frames_each_equal_a_fresh_handle(nl):
    case = ref.C130
    with open_handle(nl, case, weights=False) as st:
        for n in (128, 130, 114, 113):
            t = ref.truth(case, n)
            st.set_active_frames(n)
            st.set_weights(ref.weights_of(n))
            out = check_pass(st, case, t, n)
            with open_handle(nl, case, n) as fresh:
                assert bits_equal(out, check_pass(fresh, case, t, n))


@pytest.mark.parametrize("case", [ref.BY_FRAMES[17], ref.BY_FRAMES[128], ref.C200], ids=lambda c: c.name)
def test_pass_history(nl, case):
    """default sigma pass, this pass, default sigma pass: the two default passes agree bit for bit with their counters,
    kernel and protocol, and last_mode says MAD in between"""
    t = ref.truth(case)
    other = (2.5, 3.5)

    def default_pass(st):
        out, cl, ch = st.run(capi.ST_SIGMA, other[0], other[1], LOC)
        assert st.last_mode == capi.ST_SIGMA
        return out.view(np.uint32).copy(), (cl, ch), st.last_kernel_name, st.last_pass_protocol

    for weights in (None, ref.weights_of(case.frames)):
        with open_handle(nl, case, weights=False) as st:
            st.set_weights(weights)
            default_pass(st)                              # (a handle's first pass has no list lengths to go by)
            before = default_pass(st)
            st.set_weights(ref.weights_of(case.frames))
            check_pass(st, case, t)
            assert st.last_pass_protocol == 0 and st.last_mode == MAD
            st.set_weights(weights)
            after = default_pass(st)
            assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]


def test_weights_async_and_the_resident_result(nl):
    case = ref.BY_FRAMES[64]
    t = ref.truth(case)
    with open_handle(nl, case, weights=False) as st:
        st.run(capi.ST_MEAN, 0.0, 0.0, LOC)
        for call in (st.run_mad_weighted, st.run_mad_weighted_async):
            with pytest.raises(capi.NlError) as e:
                call(case.kappa, case.kappa, LOC)
            assert e.value.code == capi.ERR_INVALID_ARG
            assert "nl_stack_set_weights" in e.value.message and "nl_stack_run with NL_ST_MAD_SIGMA" in e.value.message
        st.set_weights(ref.weights_of(case.frames))               # the handle is settled: the next pass is as any other
        sync = check_pass(st, case, t)
        st.run(capi.ST_MEAN, 0.0, 0.0, LOC)                       # another result in between
        st.run_mad_weighted_async(case.kappa, case.kappa, LOC)
        out = np.zeros(t.result.size, np.float32)
        assert st.finish(out) == totals(t)
        assert bits_equal(out, sync) and st.last_mode == MAD
        p_ms, d_ms = st.pass_times(0)
        assert p_ms > 0 and d_ms > 0
        st.run(capi.ST_MEAN, 0.0, 0.0, LOC)
        got, cl, ch = st.run_mad_weighted(case.kappa, case.kappa, LOC, fetch=False)
        assert got is None and (cl, ch) == totals(t)
        assert bits_equal(st.result_tile(), t.result)


def test_a_sigma_that_rejects_nothing_gives_the_weighted_mean(nl):
    for case in (ref.BY_FRAMES[128], ref.BY_FRAMES[256]):
        t = ref.truth(case, sigmas=(1e30, 1e30))
        with open_handle(nl, case) as st:
            out = check_pass(st, case, t, sigmas=(1e30, 1e30))
            mean, _, _ = st.run(capi.ST_MEAN, 0.0, 0.0, LOC)
            assert totals(t) == (0, 0) and bits_equal(out, mean)


def test_two_tile_group_equals_the_checker(nl):
    case = ref.BY_FRAMES[65]
    t = ref.truth(case)
    with nl.StackGroup(case.frames, case.width, case.height, devices=[0, 0]) as g:
        assert g.size == 2 and [g.tile_rows(i) for i in range(2)] == [(0, 19), (19, 18)]     # (the group's own split of 37 rows)
        g.upload_frames(ref.make_frames(case))
        with pytest.raises(capi.NlError) as e:
            g.run_mad_weighted(case.kappa, case.kappa, LOC)
        assert e.value.code == capi.ERR_INVALID_ARG and "nl_stack_set_weights" in e.value.message
        g.set_weights(ref.weights_of(case.frames))
        out, cl, ch = g.run_mad_weighted(case.kappa, case.kappa, LOC)
        assert bits_equal(out, t.result) and (cl, ch) == totals(t)
        assert g.tile(1).last_kernel_name == ref.kernel_name(case.frames) and g.tile(1).last_mode == MAD


def test_two_tile_handles_of_20_and_17_rows(nl):
    """rows 20 + 17 on one device, each handle writing its own rows of one image: the rows, and the summed totals"""
    case = ref.BY_FRAMES[129]
    t = ref.truth(case)
    w = case.width
    out = np.full(w * case.height, np.float32(-7.5))
    low = high = 0
    for row0, rows in ((0, 20), (20, 17)):
        with open_handle(nl, case, row0=row0, rows=rows) as st:
            got, cl, ch = st.run_mad_weighted(case.kappa, case.kappa, LOC, out=out)
            assert got is out and (cl, ch) == totals(t, slice(row0 * w, (row0 + rows) * w))
            assert np.all(out[(row0 + rows) * w:] == np.float32(-7.5)) or row0 > 0
            low, high = low + cl, high + ch
    assert bits_equal(out, t.result) and (low, high) == totals(t)


def test_host_operator_takes_the_switch(nl):
    """OpStack with mode 4, exposure weighting and weightsFollowFrames: the checker's bits under the operator's weights
    and the log line; without the switch the same JSON keeps failing as the reference does"""
    from nightlight_amd import operator as op
    case = ref.BY_FRAMES[16]
    frames = np.asarray(ref.make_frames(case))
    exposure = np.linspace(10, 80, case.frames).astype(np.float32)
    w = nl.weights_from_scalars(nl.WEIGHT_EXPOSURE, exposure)
    t = ref.truth(case, sigmas=(2.75, 2.75), weights=w)
    spec = '{"type":"stack","mode":4,"weighting":1%s}'
    out, _, log = op.op_stack_apply_json(spec % ',"weightsFollowFrames":true', list(frames), case.width, case.height,
                                         exposure=exposure)
    some = t.n > 0                                               # (the operator's RefFrameLoc is 0, the checker's 123)
    assert bits_equal(out[some], t.result[some]) and np.all(out[~some] == 0) and (~some).any()
    assert "stacking mode 4" in log and "Clipped low %d " % totals(t)[0] in log and " high %d " % totals(t)[1] in log
    with pytest.raises(op.OperatorError) as e:
        op.op_stack_apply_json(spec % "", list(frames), case.width, case.height, exposure=exposure)
    assert "MADSigma stacking with weights is still unimplemented" in str(e.value)
