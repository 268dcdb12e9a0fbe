"""GPU: the weighted linear-fit pass (include/nlstack_wlinfit.h, an extension) against the fp32 restatement of its
definition (tests/wlinfit_ref.py; tests/test_wlinfit_ref.py pins that checker to the CPU oracle).  Every comparison is
equality of bits: the result, the two totals (also against run(ST_LINEAR_FIT) on the same handle), the kernel's name,
and the number of pixels the register engine hands to the column kernel -- predicted by the checker, so the column
kernel cannot quietly do the register engine's work.  1 ... 128 frames run the register engine, 129 and 200 the column
kernel; the adversarial case (integer samples, sigma 1, +-Inf) hands over most of its pixels for every reason there is.

Figures of the cases (CPU, tests/wlinfit_ref.py): predicted hand-over share of the generic cases 0 % up to 33 frames,
0.2 % at 64, 0.6 % at 65, 1.7 % at 96, 5.4 % at 128 frames; adversarial case about 90 %."""
import numpy as np
import pytest

import wlinfit_ref as ref
from nightlight_amd import capi
from util import bits_equal

pytestmark = pytest.mark.gpu

LOC = ref.REF_LOC
C24, C128 = ref.BY_FRAMES[24], ref.BY_FRAMES[128]


def open_handle(nl, case, row0=0, rows=None, weights=True):
    st = nl.StackHandle(case.frames, case.width, case.height, row0=row0, rows=rows)
    st.upload_frames(ref.make_frames(case))
    if weights:
        st.set_weights(ref.weights_of(case.frames))
    return st


def totals(t, rows=slice(None)):
    return int(t.clip_low[rows].sum()), int(t.clip_high[rows].sum())


def check_pass(st, case, t, kappa=None):
    """one weighted pass on `st` equals the truth `t` in bits, totals, kernel and hand-over count"""
    k = case.kappa if kappa is None else kappa
    out, cl, ch = st.run_linfit_weighted(k, k, LOC)
    name, handed = st.last_kernel_name, st.last_fallback_pixels
    print("%s: totals %r, kernel %s, handed over %d of %d (predicted %d)"
          % (case.name, (cl, ch), name, handed, t.result.size, int(t.handover.sum())))
    assert bits_equal(out, t.result)
    assert (cl, ch) == totals(t)
    assert st.last_mode == capi.ST_LINEAR_FIT
    return out, name, handed


@pytest.mark.parametrize("case", ref.CASES, ids=[c.name for c in ref.CASES])
def test_result_totals_kernel_and_handover_equal_the_checker(nl, case):
    t = ref.truth(case)
    with open_handle(nl, case) as st:
        out, name, handed = check_pass(st, case, t)
        assert name == ref.kernel_name(case)
        if case.engine == "register":
            assert handed == int(t.handover.sum())
            assert t.handover.mean() <= 0.10            # the column kernel cannot hide the register engine
        else:
            assert handed == 0                          # the column kernel took the whole tile: nothing was handed over
        # the rejection is the unweighted fit's: the same totals from the default pass on the same handle
        _, cl, ch = st.run(capi.ST_LINEAR_FIT, case.kappa, case.kappa, LOC)
        assert (cl, ch) == totals(t)
    p = case.width * case.height
    assert t.n[p // 2] == 0 and out[p // 2] == np.float32(LOC)          # the pixel without data
    assert t.n[p // 2 + 7] == 1
    if case.frames >= 2:
        assert t.n[p // 2 + 9] == 2


def test_adversarial_case_hands_over_for_every_reason(nl):
    case = ref.ADVERSARIAL
    t = ref.truth(case)
    assert t.handover.mean() >= 0.25
    assert t.too_many.any() and t.split.any() and t.inf.any()
    with open_handle(nl, case) as st:
        _, name, handed = check_pass(st, case, t)
        assert name == ref.kernel_name(case) and handed == int(t.handover.sum())
        _, cl, ch = st.run(capi.ST_LINEAR_FIT, case.kappa, case.kappa, LOC)
        assert (cl, ch) == totals(t)


@pytest.mark.parametrize("case", [C24, C128], ids=lambda c: c.name)
def test_forced_column_engine_equals_the_default_engine(nl, case):
    t = ref.truth(case)
    with open_handle(nl, case) as st:
        default, name, _ = check_pass(st, case, t)
        st.set_exact(1)
        forced, forced_name, handed = check_pass(st, case, t)
        assert bits_equal(default, forced)
        assert name.startswith("stack_linfit_weighted_kernel<") and forced_name == ref.COLUMN_KERNEL and handed == 0
        st.set_exact(0)
        assert check_pass(st, case, t)[1] == name


def test_a_sigma_that_rejects_nothing_gives_the_weighted_mean(nl):
    case = C128
    t = ref.truth(case, kappa=1e30)
    with open_handle(nl, case) as st:
        out, _, _ = check_pass(st, case, t, kappa=1e30)
        mean, cl, ch = st.run(capi.ST_MEAN, 0.0, 0.0, LOC)
        assert (cl, ch) == (0, 0) and totals(t) == (0, 0)
        assert bits_equal(out, mean)


def test_active_frames_are_respected(nl):
    case, n = C24, 17
    t = ref.truth(case, n)
    with open_handle(nl, case, weights=False) as st:
        st.set_active_frames(n)
        st.set_weights(ref.weights_of(n))
        _, name, handed = check_pass(st, case, t)
        assert name == ref.kernel_name(case, n) and handed == int(t.handover.sum())


def test_tile_handle_writes_only_its_rows(nl):
    case, row0, rows = C24, 5, 9
    t = ref.truth(case)
    p, w = case.width * case.height, case.width
    inside = slice(row0 * w, (row0 + rows) * w)
    out = np.full(p, np.float32(-7.5))
    with open_handle(nl, case, row0, rows) as st:
        got, cl, ch = st.run_linfit_weighted(case.kappa, case.kappa, LOC, out=out)
        assert got is out and st.last_fallback_pixels == int(t.handover[inside].sum())
    assert bits_equal(out[inside], t.result[inside]) and (cl, ch) == totals(t, inside)
    assert np.all(out[:inside.start] == np.float32(-7.5)) and np.all(out[inside.stop:] == np.float32(-7.5))


@pytest.mark.parametrize("parallel_finish", ["0", "1"])
def test_three_tile_group_equals_the_single_handle(nl, monkeypatch, parallel_finish):
    monkeypatch.setenv("NL_GROUP_PARALLEL_FINISH", parallel_finish)
    case = C24
    t = ref.truth(case)
    with nl.StackGroup(case.frames, case.width, case.height, devices=[0, 0, 0]) as g:
        assert g.size == 3
        g.upload_frames(ref.make_frames(case))
        with pytest.raises(capi.NlError) as e:
            g.run_linfit_weighted(case.kappa, case.kappa, LOC)
        assert e.value.code == capi.ERR_INVALID_ARG and "NL_ST_LINEAR_FIT" in e.value.message
        g.set_weights(ref.weights_of(case.frames))
        out, cl, ch = g.run_linfit_weighted(case.kappa, case.kappa, LOC)
        assert bits_equal(out, t.result) and (cl, ch) == totals(t)
        assert g.tile(1).last_kernel_name == ref.kernel_name(case)


def test_result_stays_on_the_device_and_async_finish(nl):
    case = C24
    t = ref.truth(case)
    with open_handle(nl, case) as st:
        got, cl, ch = st.run_linfit_weighted(case.kappa, case.kappa, LOC, fetch=False)
        assert got is None and (cl, ch) == totals(t)
        assert bits_equal(st.result_tile(), t.result)
        st.run(capi.ST_MEAN, 0.0, 0.0, LOC)                      # another result in between
        st.run_linfit_weighted_async(case.kappa, case.kappa, LOC)
        out = np.zeros(t.result.size, np.float32)
        assert st.finish(out) == totals(t)
        assert bits_equal(out, t.result)
        p_ms, d_ms = st.pass_times(0)
        assert p_ms > 0 and d_ms > 0


def test_without_weights_the_call_names_the_unweighted_one(nl):
    case = C24
    t = ref.truth(case)
    with open_handle(nl, case, weights=False) as st:
        st.run(capi.ST_MEAN, 0.0, 0.0, LOC)
        with pytest.raises(capi.NlError) as e:
            st.run_linfit_weighted(case.kappa, case.kappa, LOC)
        assert e.value.code == capi.ERR_INVALID_ARG
        assert "nl_stack_run with NL_ST_LINEAR_FIT" in e.value.message and "nl_stack_set_weights" in e.value.message
        with pytest.raises(capi.NlError):
            st.run_linfit_weighted_async(case.kappa, case.kappa, LOC)
        st.set_weights(ref.weights_of(case.frames))              # the handle is settled: the next pass is as any other
        check_pass(st, case, t)
        st.set_weights(None)
        with pytest.raises(capi.NlError):
            st.run_linfit_weighted(case.kappa, case.kappa, LOC)


def default_pass(st, mode, k):
    out, cl, ch = st.run(mode, k, k, LOC)
    return out.view(np.uint32).copy(), (cl, ch), st.last_kernel_name, st.last_pass_protocol


@pytest.mark.parametrize("mode", [capi.ST_LINEAR_FIT, capi.ST_SIGMA])
def test_a_weighted_pass_leaves_default_passes_as_they_were(nl, mode):
    """default pass, weighted linear-fit pass, default pass: the two default passes agree in result bits, totals,
    kernel and protocol -- around the default linear fit and around a default sigma pass.  (One default pass runs in
    front of the three: a handle's first pass has no list lengths to go by, tests/test_gpu_rejmap.py.)"""
    case = C24
    t = ref.truth(case)
    with open_handle(nl, case, weights=False) as st:
        default_pass(st, mode, case.kappa)
        before = default_pass(st, mode, case.kappa)
        st.set_weights(ref.weights_of(case.frames))
        check_pass(st, case, t)
        assert st.last_pass_protocol == 0
        st.set_weights(None)
        after = default_pass(st, mode, case.kappa)
        assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
        assert not after[2].startswith("stack_exact_kernel") and "weighted" not in after[2]
        if mode == capi.ST_LINEAR_FIT:
            assert before[1] == totals(t)


def test_the_default_linear_fit_still_ignores_the_weights(nl):
    case = C24
    with open_handle(nl, case, weights=False) as st:
        plain = default_pass(st, capi.ST_LINEAR_FIT, case.kappa)
        st.set_weights(ref.weights_of(case.frames))
        weighted = default_pass(st, capi.ST_LINEAR_FIT, case.kappa)
        assert np.array_equal(plain[0], weighted[0]) and plain[1:3] == weighted[1:3]
        assert weighted[2].startswith("stack_linfit_fast_kernel<")
    assert bits_equal(plain[0].view(np.float32), ref.truth(case).ymean)
