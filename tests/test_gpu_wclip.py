"""GPU: the weighted clip pass whose weights follow their frames (include/nlstack_wclip.h, an extension) against the
fp32 restatement of its definition (tests/wclip_ref.py; tests/test_wclip_ref.py pins that checker to the CPU oracle).
Every comparison of results is equality of bits: the result, the two totals (also against run(mode) with weights on the
same handle), the kernel's name, and bounds on the number of pixels the streaming engine hands to the column kernel -- at
least the pixels that cannot have a complete record, at most 10 % on the generic cases, so that the column kernel cannot
quietly do the streaming kernel's work.  1 ... 8 frames run the column kernel alone, 9 ... 32 the shallow decision
kernels, 33 ... 128 the register decision pass, 129 ... 512 the LDS-column one.

The one place where "equal" is not "equal bits": a result that is NaN by the definition (an empty K: 0 / 0; an infinite
sample) -- the sign and payload of the NaN a division makes are the hardware's, so the adversarial case compares NaN
with NaN and everything else bit for bit.  The generic cases have no NaN result and compare bits throughout."""
import numpy as np
import pytest

import wclip_ref as ref
from nightlight_amd import capi
from util import bits_equal

pytestmark = pytest.mark.gpu

LOC = ref.REF_LOC
MODE_IDS = {ref.ST_SIGMA: "sigma", ref.ST_WINSOR: "winsor"}
GENERIC = ref.CASES + [ref.PADDED]
C24, C128, C200 = ref.BY_FRAMES[24], ref.BY_FRAMES[128], ref.BY_FRAMES[200]
both_modes = pytest.mark.parametrize("mode", ref.MODES, ids=MODE_IDS.get)


def open_handle(nl, case, row0=0, rows=None, weights=True):
    st = nl.StackHandle(case.frames, case.width, case.height, row0=row0, rows=rows)
    st.upload_frames(ref.make_frames(case))
    if weights:
        st.set_weights(ref.weights_of(case.frames))
    return st


def totals(t, rows=slice(None)):
    return int(t.clip_low[rows].sum()), int(t.clip_high[rows].sum())


def bits_equal_or_both_nan(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and bits_equal(got[~nan], want[~nan])


def check_pass(st, case, mode, t, sigmas=None, equal=bits_equal):
    """one pass on `st` equals the truth `t` in bits and totals; returns (result, kernel name, pixels handed over)"""
    sl, sh = (case.kappa, case.kappa) if sigmas is None else sigmas
    out, cl, ch = st.run_clip_weighted(mode, sl, sh, LOC)
    name, handed = st.last_kernel_name, st.last_fallback_pixels
    print("%s %s: totals %r, kernel %s, handed over %d of %d (%.2f %%; at least %d)"
          % (case.name, MODE_IDS[mode], (cl, ch), name, handed, t.result.size, 100.0 * handed / t.result.size,
             int(t.must_hand_over.sum())))
    assert equal(out, t.result)
    assert (cl, ch) == totals(t)
    assert st.last_mode == mode
    return out, name, handed


GENERIC_RUNS = [(c, m) for c in GENERIC for m in ref.MODES] + [(ref.NINE_SIGMA, ref.ST_SIGMA)]


@pytest.mark.parametrize("case,mode", GENERIC_RUNS, ids=["%s-%s" % (c.name, MODE_IDS[m]) for c, m in GENERIC_RUNS])
def test_result_totals_kernel_and_handover(nl, case, mode):
    t = ref.truth(case, mode)
    assert not np.isnan(t.result).any()
    with open_handle(nl, case) as st:
        out, name, handed = check_pass(st, case, mode, t)
        assert name == ref.kernel_name(case, mode)
        if case.engine == "column":
            assert handed == 0                          # the column kernel took the whole tile: nothing was handed over
        else:
            assert handed >= int(t.must_hand_over.sum())
            assert handed <= 0.10 * t.result.size       # the column kernel cannot hide the streaming engine
        # the rejection ignores the weights: the same totals from the parity pass with weights on the same handle
        _, cl, ch = st.run(mode, case.kappa, case.kappa, LOC)
        assert (cl, ch) == totals(t)
    p = case.width * case.height
    assert t.n[p // 2] == 0 and out[p // 2] == np.float32(LOC)          # the pixel without data
    assert t.n[p // 2 + 7] == 1
    if case.frames >= 2:
        assert t.n[p // 2 + 9] == 2


@both_modes
@pytest.mark.parametrize("sigmas", ref.ADVERSARIAL_SIGMAS, ids=lambda s: "%g,%g" % s)
def test_adversarial_case(nl, mode, sigmas):
    """integer samples at sigma 1, +-Inf samples, the pixel that ends through len <= 1, crossing bounds: no cap on what is
    handed over"""
    case = ref.ADVERSARIAL
    t = ref.truth(case, mode, sigmas=sigmas)
    with open_handle(nl, case) as st:
        out, name, handed = check_pass(st, case, mode, t, sigmas, equal=bits_equal_or_both_nan)
        assert name == ref.kernel_name(case, mode) and handed >= int(t.must_hand_over.sum())
        _, cl, ch = st.run(mode, sigmas[0], sigmas[1], LOC)
        assert (cl, ch) == totals(t)
    if sigmas == (1.0, 1.0):
        # K is what is left AFTER the last sweep, the 1000 alone (1000 * w / w), not the three samples' 1000.33
        px = ref.LEN_LE_1_PIXEL
        assert t.member[px].sum() == 1 and abs(float(out[px]) - 1000.0) < 1e-3


@both_modes
@pytest.mark.parametrize("case", [C24, C128, C200], ids=lambda c: c.name)
def test_forced_column_engine_equals_the_default_engine(nl, case, mode):
    t = ref.truth(case, mode)
    with open_handle(nl, case) as st:
        default, name, _ = check_pass(st, case, mode, t)
        st.set_exact(1)
        forced, forced_name, handed = check_pass(st, case, mode, t)
        assert bits_equal(default, forced)
        assert name.startswith("stack_clip_weighted_kernel<") and forced_name == ref.COLUMN_KERNEL[mode] and handed == 0
        st.set_exact(0)
        assert check_pass(st, case, mode, t)[1] == name


@both_modes
@pytest.mark.parametrize("case", [C128, C200], ids=lambda c: c.name)
def test_four_pixels_per_lane_and_the_tail(nl, monkeypatch, case, mode):
    """a frame stride of 2257 + 3 floats: 16-byte loads, four pixels per lane, and one tail pixel for the scalar kernel"""
    monkeypatch.setenv("NL_STRIDE_PAD", "3")
    t = ref.truth(case, mode)
    with open_handle(nl, case) as st:
        _, name, handed = check_pass(st, case, mode, t)
        assert name == ref.kernel_name(case, mode, vec=True) and handed <= 0.10 * t.result.size


@both_modes
def test_a_sigma_that_rejects_nothing_gives_the_weighted_mean(nl, mode):
    case = C128
    t = ref.truth(case, mode, sigmas=(1e30, 1e30))
    with open_handle(nl, case) as st:
        out, _, _ = check_pass(st, case, mode, t, (1e30, 1e30))
        mean, cl, ch = st.run(capi.ST_MEAN, 0.0, 0.0, LOC)
        assert (cl, ch) == (0, 0) and totals(t) == (0, 0)
        assert bits_equal(out, mean)


@both_modes
def test_active_frames_are_respected(nl, mode):
    case, n = C24, 17
    t = ref.truth(case, mode, n)
    with open_handle(nl, case, weights=False) as st:
        st.set_active_frames(n)
        st.set_weights(ref.weights_of(n))
        _, name, _ = check_pass(st, case, mode, t)
        assert name == ref.kernel_name(case, mode, n)
        st.set_active_frames(5)                       # ... down to the column kernel's depths
        st.set_weights(ref.weights_of(5))
        _, name, handed = check_pass(st, case, mode, ref.truth(case, mode, 5))
        assert name == ref.COLUMN_KERNEL[mode] and handed == 0


def test_tile_handle_writes_only_its_rows(nl):
    case, mode, row0, rows = C24, ref.ST_WINSOR, 5, 9
    t = ref.truth(case, mode)
    p, w = case.width * case.height, case.width
    inside = slice(row0 * w, (row0 + rows) * w)
    out = np.full(p, np.float32(-7.5))
    with open_handle(nl, case, row0, rows) as st:
        got, cl, ch = st.run_clip_weighted(mode, case.kappa, case.kappa, LOC, out=out)
        assert got is out
    assert bits_equal(out[inside], t.result[inside]) and (cl, ch) == totals(t, inside)
    assert np.all(out[:inside.start] == np.float32(-7.5)) and np.all(out[inside.stop:] == np.float32(-7.5))


@both_modes
def test_two_tile_group_equals_the_single_handle(nl, mode):
    case = C24
    t = ref.truth(case, mode)
    with nl.StackGroup(case.frames, case.width, case.height, devices=[0, 0]) as g:
        assert g.size == 2
        g.upload_frames(ref.make_frames(case))
        with pytest.raises(capi.NlError) as e:
            g.run_clip_weighted(mode, case.kappa, case.kappa, LOC)
        assert e.value.code == capi.ERR_INVALID_ARG and "nl_stack_run" in e.value.message
        g.set_weights(ref.weights_of(case.frames))
        out, cl, ch = g.run_clip_weighted(mode, case.kappa, case.kappa, LOC)
        assert bits_equal(out, t.result) and (cl, ch) == totals(t)
        assert g.tile(1).last_kernel_name == ref.kernel_name(case, mode)


def test_auto_mode_result_on_the_device_and_async_finish(nl):
    case = C24                                                   # 24 frames: auto resolves to winsorized sigma
    t = ref.truth(case, ref.ST_WINSOR)
    with open_handle(nl, case) as st:
        got, cl, ch = st.run_clip_weighted(capi.ST_AUTO, case.kappa, case.kappa, LOC, fetch=False)
        assert got is None and (cl, ch) == totals(t) and st.last_mode == capi.ST_WINSOR_SIGMA
        assert bits_equal(st.result_tile(), t.result)
        st.run(capi.ST_MEAN, 0.0, 0.0, LOC)                      # another result in between
        st.run_clip_weighted_async(capi.ST_AUTO, case.kappa, case.kappa, LOC)
        out = np.zeros(t.result.size, np.float32)
        assert st.finish(out) == totals(t)
        assert bits_equal(out, t.result)
        p_ms, d_ms = st.pass_times(0)
        assert p_ms > 0 and d_ms > 0
        st.set_active_frames(9)                                  # 9 frames: auto resolves to sigma
        st.set_weights(ref.weights_of(9))
        st.run_clip_weighted(capi.ST_AUTO, 1.5, 1.5, LOC)
        assert st.last_mode == capi.ST_SIGMA
    with open_handle(nl, ref.BY_FRAMES[33]) as st:               # 33 frames: auto resolves to the linear fit
        with pytest.raises(capi.NlError) as e:
            st.run_clip_weighted(capi.ST_AUTO, 3.0, 3.0, LOC)
        assert e.value.code == capi.ERR_INVALID_MODE and "neither NL_ST_SIGMA nor NL_ST_WINSOR_SIGMA" in e.value.message


def test_without_weights_the_call_names_the_unweighted_one(nl):
    case, mode = C24, ref.ST_SIGMA
    t = ref.truth(case, mode)
    with open_handle(nl, case, weights=False) as st:
        st.run(capi.ST_MEAN, 0.0, 0.0, LOC)
        with pytest.raises(capi.NlError) as e:
            st.run_clip_weighted(mode, case.kappa, case.kappa, LOC)
        assert e.value.code == capi.ERR_INVALID_ARG
        assert "nl_stack_run" in e.value.message and "nl_stack_set_weights" in e.value.message
        with pytest.raises(capi.NlError):
            st.run_clip_weighted_async(mode, case.kappa, case.kappa, LOC)
        st.set_weights(ref.weights_of(case.frames))              # the handle is settled: the next pass is as any other
        check_pass(st, case, mode, t)
        st.set_weights(None)
        with pytest.raises(capi.NlError):
            st.run_clip_weighted(mode, case.kappa, case.kappa, LOC)


@both_modes
@pytest.mark.parametrize("case", [C24, C128], ids=lambda c: c.name)
def test_pass_history(nl, oracle, case, mode):
    """default unweighted and weighted passes at other sigmas, in front of and behind the new pass: each keeps its own
    truth -- the counters the oracle's, the weighted default pass the oracle's bits, the unweighted one its own bits of
    before -- and the new pass, run twice between them, keeps its own"""
    frames = np.asarray(ref.make_frames(case))
    w = ref.weights_of(case.frames)
    t = ref.truth(case, mode)
    other = (2.5, 3.5)

    def default_pass(st, weights):
        st.set_weights(weights)
        out, cl, ch = st.run(mode, other[0], other[1], LOC)
        rc, want, wl, wh, _ = oracle.stack_apply(mode, frames, weights, other[0], other[1], LOC)
        assert rc == 0 and (cl, ch) == (wl, wh)
        if weights is not None:
            assert bits_equal(out, want)
        return out.view(np.uint32).copy(), st.last_kernel_name, st.last_pass_protocol

    with open_handle(nl, case, weights=False) as st:
        default_pass(st, None)                       # (a handle's first pass has no list lengths to go by)
        plain = default_pass(st, None)
        weighted = default_pass(st, w)
        name = check_pass(st, case, mode, t)[1]
        assert st.last_pass_protocol == 0
        again = default_pass(st, w)
        assert np.array_equal(again[0], weighted[0]) and again[1:] == weighted[1:]
        assert check_pass(st, case, mode, t)[1] == name
        after = default_pass(st, None)
        assert np.array_equal(plain[0], after[0]) and plain[1:] == after[1:]
        st.set_weights(w)
        check_pass(st, case, mode, t)


def test_host_operator_takes_the_switch(nl):
    """OpStack with weightsFollowFrames: exposure weighting, auto mode at 9 frames (sigma) -- the checker's bits under the
    operator's weights; without the switch the same JSON gives the parity result, which differs"""
    from nightlight_amd import operator as op
    case = ref.BY_FRAMES[9]
    frames = np.asarray(ref.make_frames(case))
    exposure = np.linspace(10, 80, case.frames).astype(np.float32)
    w = nl.weights_from_scalars(nl.WEIGHT_EXPOSURE, exposure)
    t = ref.truth(case, ref.ST_SIGMA, sigmas=(1.5, 1.5), weights=w)
    spec = '{"type":"stack","weighting":1,"sigmaLow":1.5,"sigmaHigh":1.5%s}'
    out, _, log = op.op_stack_apply_json(spec % ',"weightsFollowFrames":true', list(frames), case.width, case.height,
                                         exposure=exposure)
    some = t.n > 0                                               # (the operator's RefFrameLoc is 0, the checker's 123)
    assert bits_equal(out[some], t.result[some]) and np.all(out[~some] == 0) and (~some).any()
    assert "stacking mode 2" in log and "Clipped low %d " % totals(t)[0] in log and " high %d " % totals(t)[1] in log
    parity, _, parity_log = op.op_stack_apply_json(spec % "", list(frames), case.width, case.height, exposure=exposure)
    assert "Clipped low %d " % totals(t)[0] in parity_log and not bits_equal(parity[some], t.result[some])
    # a mode the switch does not apply to is left alone
    mean_on, _, _ = op.op_stack_apply_json('{"type":"stack","mode":1,"weighting":1,"weightsFollowFrames":true}',
                                           list(frames), case.width, case.height, exposure=exposure)
    mean_off, _, _ = op.op_stack_apply_json('{"type":"stack","mode":1,"weighting":1}', list(frames), case.width,
                                            case.height, exposure=exposure)
    assert bits_equal(mean_on, mean_off)
