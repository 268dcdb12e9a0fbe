"""GPU: the deep maps pass (include/nlstack_deepmaps.h) -- nl_stack_run_maps_deep / nl_group_run_maps_deep -- against the
CPU oracle called pixel by pixel (rejmap_ref.per_pixel) on the frames of tests/deepmaps_frames.py, which
tests/test_deepmaps_frames.py holds to keeping at least 85 % of the pixels inside the dominant kernel's columns.  The maps
and totals are compared count for count; the result is the default pass's (same kernels, same arithmetic: within RTOL of
the oracle, bit-exact where the column kernel replays a pixel or a pixel has no data).  The image is 41 x 23 = 943
pixels: no multiple of the 32 or 64 pixels of a workgroup.  Every truth is computed once per key.

What is particular to this pass is that each pixel's word is written by one of three kernels -- the dominant kernel of the
frame-count class, the generic kernel over its hand-over list, the column kernel over the exact list -- so every case
insists that all three really ran and that the dominant kernel kept more than half of the pixels, and passes with
different sigmas run in turn on one handle: a word that no kernel wrote, or one left by an earlier pass, would show.

497 frames are the depth at which that last demand bites: they run the class of 512, the stack that fills its lanes,
whose default layout takes 15 missing samples (MlzLayout::PADS) -- and 497 frames are 15 short of 512 already, so with that
layout every pixel with one NaN among its samples goes to the generic pass (measured: 904 + 5 of the 943 pixels; these
frames give a pixel four NaN on average).  A maps pass of 241 ... 255 or 497 ... 511 frames therefore runs the class's second
layout (ROOMY: 23 missing samples, launch_mlz_classes), with which 105 + 4 pixels are handed over at 497 frames."""
import ctypes as C

import numpy as np
import pytest

import deepmaps_frames as deep
import maps_cases as cases
import rejmap_ref as ref
from maps_cases import assert_deep_maps as assert_maps, is_deep_maps_name, ref_mismatch
from nightlight_amd import capi
from util import RTOL, bits_equal, close_values

pytestmark = pytest.mark.gpu

W, H, P = deep.W, deep.H, deep.P
SIGMAS, TIGHT, REF_LOC = deep.SIGMAS, deep.TIGHT, deep.REF_LOC
MODES = {"sigma": capi.ST_SIGMA, "winsor": capi.ST_WINSOR_SIGMA}
LINFIT = capi.ST_LINEAR_FIT
NO_SHARED_HINTS = 512       # developer switch: no list-length hints from earlier handles of the same geometry
# every boundary of the frame-count classes' dispatch: the first deep stack, both sides of a class boundary with two
# lanes (144 | 145), a class with pads (200), both sides of the stack that fills two lanes (255, 256 | 257: four lanes),
# classes of four lanes with and without pads (272, 300, 400), the last class before the selection front end and the
# class that runs it (496 | 497, 511), the stack that fills four lanes (512)
DEPTHS = [129, 144, 145, 200, 255, 256, 257, 272, 300, 400, 496, 497, 511, 512]


def open_handle(nl, n, row0=0, rows=None):
    return cases.open_handle(nl, n, row0, rows, frames=deep.frames_of)


def deep_pass(st, mode, sigmas=SIGMAS, **kw):
    return st.run_maps_deep(mode, sigmas[0], sigmas[1], REF_LOC, **kw)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("n", DEPTHS)
def test_every_class_equals_the_oracle_pixel_by_pixel(nl, oracle, n, mode):
    t = deep.truth(oracle, n, MODES[mode])
    with open_handle(nl, n) as st:
        got = deep_pass(st, MODES[mode])
        name, protocol = st.last_kernel_name, st.last_pass_protocol
        fallback, generic = st.last_fallback_pixels, st.last_generic_pixels
        assert st.last_mode == MODES[mode]
    print("n %d %s: %s, generic list %d, exact list %d of %d pixels, totals %d / %d"
          % (n, mode, name, generic, fallback, P, got[1], got[2]))
    assert_maps(got, t)
    assert (got[1], got[2]) == (t.clip_low, t.clip_high)
    for p in deep.INF_PIXELS + (deep.NO_DATA,):
        assert bits_equal(got[0][p:p + 1], t.result[p:p + 1]), p
    assert got[0][deep.NO_DATA] == np.float32(REF_LOC) and got[3][deep.NO_DATA] == 0 and got[4][deep.NO_DATA] == 0
    assert t.coverage[deep.NO_DATA] == 0
    assert is_deep_maps_name(name), name
    lanes, ntop = (2 if n <= 256 else 4), (n + 15) // 16 * 16
    assert name == "stack_sigma_mlz_kernel<%d, %s, %d, 0, maps>" % (lanes, "true" if mode == "winsor" else "false", ntop)
    assert protocol == 0
    # all three kernels ran: the exact replay (the infinite samples), the generic pass (the half-empty pixels), and the
    # dominant kernel kept more than half of the tile
    assert fallback >= 3
    assert generic >= 60
    assert generic + fallback < P // 2


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("n", [200, 400])
def test_agrees_with_the_column_pass_and_the_default_pass(nl, oracle, n, mode):
    m = MODES[mode]
    with open_handle(nl, n) as st:
        got = deep_pass(st, m)
        assert is_deep_maps_name(st.last_kernel_name)
        col = st.run_maps(m, SIGMAS[0], SIGMAS[1], REF_LOC)
        assert st.last_kernel_name == "stack_exact_kernel<%s,maps>" % ref.MODE_NAMES[m]
    assert np.array_equal(got[3], col[3]) and np.array_equal(got[4], col[4]) and (got[1], got[2]) == (col[1], col[2])
    assert close_values(got[0], col[0], RTOL)
    assert got[1] > 0 and got[2] > 0
    # the default pass on a fresh handle: the same kernels without the store, the same arithmetic
    with open_handle(nl, n) as st:
        st.set_dev_flags(NO_SHARED_HINTS)
        out, cl, ch = st.run(m, SIGMAS[0], SIGMAS[1], REF_LOC)
        assert st.last_kernel_name.startswith("stack_sigma_mlz_kernel<") and "maps" not in st.last_kernel_name
    assert (cl, ch) == (got[1], got[2])
    assert bits_equal(out, got[0]), ref_mismatch(got[0], out)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_nothing_stale_and_nothing_twice(nl, oracle, mode):
    """kappa 3 / 3, then 1.2 / 1.2 (nearly every pixel goes to the generic pass), then 3 / 3 on one handle: each pass
    equals its own truth; with the maps preset and no result asked for, every word is written"""
    n, m = 300, MODES[mode]
    t, tight = deep.truth(oracle, n, m), deep.truth(oracle, n, m, sigmas=TIGHT)
    assert not np.array_equal(tight.reject_low, t.reject_low) and not np.array_equal(tight.reject_high, t.reject_high)
    L = capi.load()
    with open_handle(nl, n) as st:
        assert_maps(deep_pass(st, m), t)
        lists = (st.last_generic_pixels, st.last_fallback_pixels)
        assert_maps(deep_pass(st, m, TIGHT), tight)
        assert is_deep_maps_name(st.last_kernel_name)
        # (a pixel the generic pass cannot decide is on both lists)
        print("%s: generic / exact list %d / %d pixels at 3 / 3, %d / %d at 1.2 / 1.2"
              % ((mode,) + lists + (st.last_generic_pixels, st.last_fallback_pixels)))
        assert st.last_generic_pixels > P // 2
        assert_maps(deep_pass(st, m), t)
        assert_maps(st.run_maps(m, TIGHT[0], TIGHT[1], REF_LOC), tight)          # the column pass in between
        low, high = np.full(P, 0xABCD, np.uint16), np.full(P, 0x1234, np.uint16)
        cl, ch = C.c_int64(-1), C.c_int64(-1)
        capi.check(L.nl_stack_run_maps_deep(st._h, m, SIGMAS[0], SIGMAS[1], REF_LOC, None, C.byref(cl), C.byref(ch),
                                            low.ctypes.data_as(C.POINTER(C.c_uint16)), high.ctypes.data_as(C.POINTER(C.c_uint16))))
        assert is_deep_maps_name(st.last_kernel_name)
        assert np.array_equal(low, t.reject_low) and np.array_equal(high, t.reject_high)
        assert (cl.value, ch.value) == (t.clip_low, t.clip_high)
        assert close_values(st.result_tile(), t.result, RTOL)


def test_null_host_pointers(nl, oracle):
    """each of the five host pointers may be NULL: nothing is written there, the result stays on the device"""
    n, m = 300, capi.ST_SIGMA
    t = deep.truth(oracle, n, m)
    L = capi.load()
    u16p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16))
    with open_handle(nl, n) as st:
        capi.check(L.nl_stack_run_maps_deep(st._h, m, SIGMAS[0], SIGMAS[1], REF_LOC, None, None, None, None, None))
        assert is_deep_maps_name(st.last_kernel_name)
        assert close_values(st.result_tile(), t.result, RTOL)
        for missing in range(5):
            out, low, high = np.zeros(P, np.float32), np.zeros(P, np.uint16), np.zeros(P, np.uint16)
            cl, ch = C.c_int64(-1), C.c_int64(-1)
            args = [capi.fptr(out), C.byref(cl), C.byref(ch), u16p(low), u16p(high)]
            args[missing] = None
            capi.check(L.nl_stack_run_maps_deep(st._h, m, SIGMAS[0], SIGMAS[1], REF_LOC, *args))
            assert missing == 0 or close_values(out, t.result, RTOL)
            assert missing == 1 or cl.value == t.clip_low
            assert missing == 2 or ch.value == t.clip_high
            assert missing == 3 or np.array_equal(low, t.reject_low)
            assert missing == 4 or np.array_equal(high, t.reject_high)
            assert (missing != 0 or not out.any()) and (missing != 1 or cl.value == -1) and (missing != 2 or ch.value == -1)
            assert (missing != 3 or not low.any()) and (missing != 4 or not high.any())


@pytest.mark.parametrize("mode", sorted(MODES))
def test_active_frames_are_respected(nl, oracle, mode):
    m = MODES[mode]
    winsor = "true" if mode == "winsor" else "false"
    with open_handle(nl, 300) as st:
        st.set_active_frames(256)
        assert_maps(deep_pass(st, m), deep.truth(oracle, 300, m, n_active=256))
        assert st.last_kernel_name == "stack_sigma_mlz_kernel<2, %s, 256, 0, maps>" % winsor
        st.set_active_frames(130)
        assert_maps(deep_pass(st, m), deep.truth(oracle, 300, m, n_active=130))
        assert st.last_kernel_name == "stack_sigma_mlz_kernel<2, %s, 144, 0, maps>" % winsor
        # 128 active frames: the register-resident engine, as the resident entry runs it
        st.set_active_frames(128)
        got = deep_pass(st, m)
        name = st.last_kernel_name
        assert "stack_sigma_fast_kernel" in name and "maps" in name
        assert_maps(got, deep.truth(oracle, 300, m, n_active=128))
        res = st.run_maps_resident(m, SIGMAS[0], SIGMAS[1], REF_LOC)
        assert st.last_kernel_name == name
        assert bits_equal(res[0], got[0]) and np.array_equal(res[3], got[3]) and np.array_equal(res[4], got[4])
        st.set_active_frames(300)
        assert_maps(deep_pass(st, m), deep.truth(oracle, 300, m))
        assert st.last_kernel_name == "stack_sigma_mlz_kernel<4, %s, 304, 0, maps>" % winsor


def test_tile_handle_writes_only_its_rows(nl, oracle):
    n, row0, rows, m = 300, 5, 13, capi.ST_SIGMA                 # rows 5 ... 17 of the 23
    t = deep.truth(oracle, n, m)
    inside = slice(row0 * W, (row0 + rows) * W)
    assert inside.start <= deep.HALF_NAN.start and deep.INF_PIXELS[-1] < inside.stop      # both lists inside the tile
    out = np.full(P, np.float32(-7.5))
    low, high = np.full(P, 0xABCD, np.uint16), np.full(P, 0x1234, np.uint16)
    with open_handle(nl, n, row0=row0, rows=rows) as st:
        got = deep_pass(st, m, out=out, reject_low=low, reject_high=high)
        assert got[0] is out and got[3] is low and got[4] is high
        assert is_deep_maps_name(st.last_kernel_name)
        assert st.last_fallback_pixels >= 3 and st.last_generic_pixels >= 60
    assert_maps(got, t, inside)
    for a, fill in ((out, np.float32(-7.5)), (low, 0xABCD), (high, 0x1234)):
        assert np.all(a[:inside.start] == fill) and np.all(a[inside.stop:] == fill)


@pytest.mark.parametrize("parallel_finish", ["0", "1"])
def test_three_tile_group_equals_the_single_handle(nl, oracle, monkeypatch, parallel_finish):
    monkeypatch.setenv("NL_GROUP_PARALLEL_FINISH", parallel_finish)      # the tiles finished in turn / on worker threads
    n, m = 300, capi.ST_WINSOR_SIGMA
    t = deep.truth(oracle, n, m)
    with open_handle(nl, n) as st:
        single = deep_pass(st, m)
    with nl.StackGroup(n, W, H, devices=[0, 0, 0]) as g:
        assert g.size == 3
        g.upload_frames(deep.frames_of(n))
        got = g.run_maps_deep(m, SIGMAS[0], SIGMAS[1], REF_LOC)
        assert all(is_deep_maps_name(g.tile(i).last_kernel_name) for i in range(3))
    assert_maps(got, t)
    assert (got[1], got[2]) == (t.clip_low, t.clip_high) == (single[1], single[2])
    assert bits_equal(got[0], single[0]) and np.array_equal(got[3], single[3]) and np.array_equal(got[4], single[4])


@pytest.mark.parametrize("what", ["median", "mad", "sigma-weighted", "winsor-weighted", "sigma-forced-exact",
                                  "linearfit-24", "linearfit-200", "sigma-24"])
def test_everything_else_is_the_resident_pass(nl, what):
    """the kernel name and the results of run_maps_resident on the same handle"""
    mode = {"median": capi.ST_MEDIAN, "mad": capi.ST_MAD_SIGMA, "winsor-weighted": capi.ST_WINSOR_SIGMA,
            "linearfit-24": LINFIT, "linearfit-200": LINFIT}.get(what, capi.ST_SIGMA)
    n = 24 if what.endswith("-24") else 200
    with open_handle(nl, n) as st:
        if what.endswith("-weighted"):
            st.set_weights(ref.weights_of(n))
        if what.endswith("-forced-exact"):
            st.set_exact(1)
        got = deep_pass(st, mode)
        name, protocol = st.last_kernel_name, st.last_pass_protocol
        res = st.run_maps_resident(mode, SIGMAS[0], SIGMAS[1], REF_LOC)
        assert st.last_kernel_name == name and st.last_pass_protocol == protocol == 0
    print("%s: %s" % (what, name))
    if what.startswith("linearfit"):
        assert ("stack_linfit_fast_kernel" if n <= 128 else "stack_linfit_ml_kernel") in name and "maps" in name
    elif what == "sigma-24":
        assert "stack_sigma_fast_kernel" in name and "maps" in name
    else:
        assert name == "stack_exact_kernel<%s%s,maps>" % (ref.MODE_NAMES[mode], ",weighted" if what.endswith("-weighted") else "")
    assert bits_equal(got[0], res[0]) and (got[1], got[2]) == (res[1], res[2])
    assert np.array_equal(got[3], res[3]) and np.array_equal(got[4], res[4])
    if mode != capi.ST_MEDIAN:
        assert got[1] + got[2] > 0


def test_mean_and_refusals(nl, oracle):
    n = 200
    rc, want, _, _, _ = oracle.stack_apply(capi.ST_MEAN, np.ascontiguousarray(deep.frames_of(n)), None, SIGMAS[0], SIGMAS[1], REF_LOC)
    assert rc == 0
    low, high = np.full(P, 7, np.uint16), np.full(P, 9, np.uint16)
    with open_handle(nl, n) as st:
        got = deep_pass(st, capi.ST_MEAN, reject_low=low, reject_high=high)
        assert st.last_kernel_name == "stack_mean_vec4_kernel"
        assert bits_equal(got[0], want) and (got[1], got[2]) == (0, 0)
        assert not low.any() and not high.any()
        st.set_weights(ref.weights_of(n))
        codes = []
        for entry in (st.run_maps_deep, st.run_maps_resident):
            with pytest.raises(capi.NlError) as e:
                entry(capi.ST_MAD_SIGMA, SIGMAS[0], SIGMAS[1], REF_LOC)
            assert e.value.code == capi.ERR_WEIGHTED_MAD and "MADSigma" in e.value.message
            with pytest.raises(capi.NlError) as e2:
                entry(9, SIGMAS[0], SIGMAS[1], REF_LOC)
            assert e2.value.code == capi.ERR_INVALID_MODE
            codes.append((e.value.code, e.value.message, e2.value.code, e2.value.message))
        assert codes[0] == codes[1]
        st.set_weights(None)                     # the handle is settled: the next pass is as any other
        assert_maps(deep_pass(st, capi.ST_SIGMA), deep.truth(oracle, n, capi.ST_SIGMA))
        assert is_deep_maps_name(st.last_kernel_name)


def default_pass(st, mode):
    out, cl, ch = st.run(mode, SIGMAS[0], SIGMAS[1], REF_LOC)
    return out.view(np.uint32).copy(), (cl, ch), st.last_kernel_name, st.last_pass_protocol


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("n", [200, 512])
def test_a_deep_maps_pass_leaves_default_passes_as_they_were(nl, oracle, n, mode):
    """a default run behind a deep maps pass -- as a handle's first default pass, and as its second, which has the first
    one's list lengths to go by -- is the same run of a fresh handle that never ran a maps pass: result bits, totals,
    kernel name and protocol"""
    m = MODES[mode]
    t = deep.truth(oracle, n, m)
    with open_handle(nl, n) as st:
        st.set_dev_flags(NO_SHARED_HINTS)
        fresh = [default_pass(st, m), default_pass(st, m)]
    with open_handle(nl, n) as st:
        st.set_dev_flags(NO_SHARED_HINTS)
        assert_maps(deep_pass(st, m), t)
        assert st.last_pass_protocol == 0 and is_deep_maps_name(st.last_kernel_name)
        after = [default_pass(st, m)]
        assert_maps(deep_pass(st, m), t)
        after.append(default_pass(st, m))
    print("n %d %s: protocols of the two default passes %r" % (n, mode, [f[3] for f in fresh]))
    for k in range(2):
        assert np.array_equal(fresh[k][0], after[k][0]) and fresh[k][1:] == after[k][1:], k
        assert fresh[k][1] == (t.clip_low, t.clip_high)
        assert fresh[k][2].startswith("stack_sigma_mlz_kernel<") and "maps" not in fresh[k][2]
