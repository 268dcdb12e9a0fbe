"""GPU: the deep-stack maps pass (include/nlstack_deepstackmaps.h) -- nl_stack_run_maps_deepstack /
nl_group_run_maps_deepstack -- beyond 512 frames.

MAD sigma and the median run on the frames of tests/deepstack_frames.py (41 x 23 pixels, every lane class and merge level
of the 8- and 16-lane kernels).  The MAD maps are counts of decisions that rest on two medians: equal to the restatement
of the definition (deepstack_frames.survivor_means) and to the column pass count for count, the totals their sums and the
oracle's; the result is run_deepstack's bit for bit, the same kernel with one more store.  Sigma and winsorized clipping run
the wave-per-pixel replay with its per-pixel counts: result bits, both maps and totals equal run_maps' (the column kernel,
the other replay of the reference) on the same handle, the totals one whole-image oracle call.  Everything the engines
do not take is run_maps_full's pass in every observable respect.  Every truth is computed once per key."""
import numpy as np
import pytest

import deepstack_frames as deep
import maps_cases as cases
import rejmap_ref as ref
from maps_cases import ref_mismatch
from nightlight_amd import capi
from util import bits_equal

pytestmark = pytest.mark.gpu

W, H, P = deep.W, deep.H, deep.P
SIGMAS, TIGHT, REF_LOC = deep.SIGMAS, deep.TIGHT, deep.REF_LOC
CLIP_SIGMAS = (cases.SIGMA_LOW, cases.SIGMA_HIGH)            # 2.0 / 2.5, the sigma / winsorized cases
MAD, MEDIAN, SIGMA, WINSOR = capi.ST_MAD_SIGMA, capi.ST_MEDIAN, capi.ST_SIGMA, capi.ST_WINSOR_SIGMA
NO_SHARED_HINTS = 512       # developer switch: no list-length hints from earlier handles of the same geometry
COLUMN_MAD_MAPS = "stack_exact_kernel<mad,maps>"
LISTED = list(deep.INF_PIXELS)


def open_handle(nl, n, row0=0, rows=None):
    return cases.open_handle(nl, n, row0, rows, frames=deep.frames_of)


def maps_pass(st, mode=MAD, sigmas=SIGMAS, **kw):
    return st.run_maps_deepstack(mode, sigmas[0], sigmas[1], REF_LOC, **kw)


def is_mad_maps_name(name, n):
    return name == "stack_mad_ml_kernel<%d, maps>" % deep.lanes_of(n)


def assert_mad_maps(got, n, sigmas=SIGMAS, rows=slice(0, P)):
    """both maps equal the restatement's counts outside the exact list, are zero on it and at the pixel without data; the
    totals are the maps' sums"""
    _, cl, ch, low, high = got
    _, want_low, want_high = deep.survivor_means(n, sigmas)
    assert low.dtype == np.uint16 and high.dtype == np.uint16
    keep = np.zeros(P, bool)
    keep[rows] = True
    keep[LISTED] = False
    assert np.array_equal(low[keep], want_low[keep]) and np.array_equal(high[keep], want_high[keep])
    for p in LISTED + [deep.NO_DATA]:
        if rows.start <= p < rows.stop:
            assert low[p] == 0 and high[p] == 0, p
    assert (cl, ch) == (int(low[rows].astype(np.int64).sum()), int(high[rows].astype(np.int64).sum()))


@pytest.mark.parametrize("n", deep.DEPTHS)
def test_mad_maps_at_every_depth(nl, oracle, n):
    t = deep.whole_truth(oracle, n, MAD)
    with open_handle(nl, n) as st:
        got = maps_pass(st)
        name, protocol, fallback = st.last_kernel_name, st.last_pass_protocol, st.last_fallback_pixels
        assert st.last_mode == MAD
        plain = st.run_deepstack(MAD, SIGMAS[0], SIGMAS[1], REF_LOC)
        assert st.last_kernel_name == "stack_mad_ml_kernel<%d>" % deep.lanes_of(n)
        column = st.run_maps(MAD, SIGMAS[0], SIGMAS[1], REF_LOC) if n in deep.TIGHT_DEPTHS else None
        assert column is None or st.last_kernel_name == COLUMN_MAD_MAPS
    print("n %d: %s, exact list %d, totals %d / %d" % (n, name, fallback, got[1], got[2]))
    assert_mad_maps(got, n)
    assert (got[1], got[2]) == (t.clip_low, t.clip_high) == (plain[1], plain[2])
    assert bits_equal(got[0], plain[0]), ref_mismatch(got[0], plain[0])
    assert got[0][deep.NO_DATA] == np.float32(REF_LOC)
    assert name.startswith("stack_mad_ml_kernel<8" if n <= 1024 else "stack_mad_ml_kernel<16") and "maps" in name
    assert is_mad_maps_name(name, n)
    assert fallback == len(deep.INF_PIXELS) == 4 and protocol == 0
    if column is not None:
        assert np.array_equal(got[3], column[3]) and np.array_equal(got[4], column[4])
        assert (got[1], got[2]) == (column[1], column[2])


@pytest.mark.parametrize("n", deep.TIGHT_DEPTHS)
def test_the_median_runs_its_deep_kernel_and_zeroes_the_maps(nl, n):
    low, high = np.full(P, 7, np.uint16), np.full(P, 9, np.uint16)
    with open_handle(nl, n) as st:
        maps_pass(st)                                    # a MAD maps pass first: its words must not show through
        got = maps_pass(st, MEDIAN, reject_low=low, reject_high=high)
        name = st.last_kernel_name
        assert st.last_pass_protocol == 0 and st.last_mode == MEDIAN
        out, cl, ch = st.run(MEDIAN, SIGMAS[0], SIGMAS[1], REF_LOC)
    assert name == "stack_median_ml_kernel<%d>" % deep.lanes_of(n)
    assert (got[1], got[2]) == (0, 0) == (cl, ch)
    assert got[3] is low and got[4] is high and not low.any() and not high.any()
    assert bits_equal(got[0], out), ref_mismatch(got[0], out)


# ---- sigma / winsorized clipping beyond 512 frames: the wave-per-pixel replay with its per-pixel counts ----------------
def clip_handle(nl, what):
    if what == "rejmap-513x64x16":
        st = nl.StackHandle(513, 64, 16)                 # 1024 pixels: four per work item where the stride allows them
        frames = ref.make_frames(513, 64, 16)
    else:
        n = int(what.split("-")[1])                      # 943 pixels: one pixel per work item
        st, frames = cases.open_handle(nl, n), cases.frames_of(n)
        return st, frames
    st.upload_frames(frames)
    return st, frames


# the oracle's totals at kappa 2.0 / 2.5, one whole-image call each
CLIP_TOTALS = {("cases-513", SIGMA): (23907, 18875), ("cases-513", WINSOR): (19519, 17293),
               ("cases-1100", SIGMA): (51223, 40756), ("cases-1100", WINSOR): (41976, 37248),
               ("rejmap-513x64x16", SIGMA): (26435, 21290), ("rejmap-513x64x16", WINSOR): (21704, 19583)}


@pytest.mark.parametrize("mode", [SIGMA, WINSOR], ids=["sigma", "winsor"])
@pytest.mark.parametrize("what", ["cases-513", "cases-1100", "rejmap-513x64x16"])
def test_sigma_and_winsor_maps_beyond_512_frames(nl, oracle, what, mode):
    st, frames = clip_handle(nl, what)
    with st:
        got = maps_pass(st, mode, CLIP_SIGMAS)
        name, protocol = st.last_kernel_name, st.last_pass_protocol
        assert st.last_mode == mode
        column = st.run_maps(mode, CLIP_SIGMAS[0], CLIP_SIGMAS[1], REF_LOC)
        assert st.last_kernel_name.startswith("stack_exact_kernel<") and "maps" in st.last_kernel_name
    rc, _, cl, ch, _ = oracle.stack_apply(mode, frames, None, CLIP_SIGMAS[0], CLIP_SIGMAS[1], REF_LOC)
    assert rc == 0
    print("%s, mode %d: %s, totals %d / %d" % (what, mode, name, got[1], got[2]))
    assert name.startswith("stack_sigma_coop_kernel<") and "maps" in name and protocol == 0
    if what.startswith("cases"):
        assert name == "stack_sigma_coop_kernel<%s, false, 1, 2, maps>" % ("true" if mode == WINSOR else "false")
    assert bits_equal(got[0], column[0]), ref_mismatch(got[0], column[0])
    assert np.array_equal(got[3], column[3]) and np.array_equal(got[4], column[4])
    assert (got[1], got[2]) == (column[1], column[2]) == (int(cl), int(ch)) == CLIP_TOTALS[what, mode]
    assert (got[1], got[2]) == (int(got[3].astype(np.int64).sum()), int(got[4].astype(np.int64).sum()))
    assert got[1] > 0 and got[2] > 0
    coverage = (~np.isnan(frames)).sum(0)
    assert np.all(got[3].astype(np.int64) + got[4] <= coverage)
    empty = np.flatnonzero(coverage == 0)
    assert empty.size >= 1 and np.all(got[0][empty] == np.float32(REF_LOC)) and not got[3][empty].any() and not got[4][empty].any()


# ---- the pass among other passes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", deep.TIGHT_DEPTHS)
def test_nothing_stale(nl, oracle, n):
    """kappa 3 / 3, then 1.2 / 1.2, then 3 / 3 on one handle, a column pass and a default pass in between: each pass has its
    own maps"""
    t, tight = deep.whole_truth(oracle, n, MAD), deep.whole_truth(oracle, n, MAD, sigmas=TIGHT)
    assert (tight.clip_low, tight.clip_high) != (t.clip_low, t.clip_high)
    with open_handle(nl, n) as st:
        first = maps_pass(st)
        assert_mad_maps(first, n)
        second = maps_pass(st, MAD, TIGHT)
        assert_mad_maps(second, n, TIGHT)
        assert (second[1], second[2]) == (tight.clip_low, tight.clip_high) and is_mad_maps_name(st.last_kernel_name, n)
        column = st.run_maps(MAD, TIGHT[0], TIGHT[1], REF_LOC)                                # the column pass in between
        assert st.last_kernel_name == COLUMN_MAD_MAPS
        assert np.array_equal(column[3], second[3]) and np.array_equal(column[4], second[4])
        _, cl, ch = st.run(MAD, TIGHT[0], TIGHT[1], REF_LOC)                                   # ... and a default pass
        assert (cl, ch) == (tight.clip_low, tight.clip_high) and "maps" not in st.last_kernel_name
        third = maps_pass(st)
        assert_mad_maps(third, n)
        assert (third[1], third[2]) == (t.clip_low, t.clip_high) and is_mad_maps_name(st.last_kernel_name, n)
        assert bits_equal(third[0], first[0]) and np.array_equal(third[3], first[3]) and np.array_equal(third[4], first[4])


def test_tile_handle_writes_only_its_rows(nl):
    n, row0, rows = 700, 5, 13                                   # rows 5 ... 17 of the 23
    inside = slice(row0 * W, (row0 + rows) * W)
    assert inside.start <= deep.NO_DATA and deep.INF_PIXELS[-1] < inside.stop
    out = np.full(P, np.float32(-7.5))
    low, high = np.full(P, 0xABCD, np.uint16), np.full(P, 0x1234, np.uint16)
    with open_handle(nl, n, row0=row0, rows=rows) as st:
        got = maps_pass(st, out=out, reject_low=low, reject_high=high)
        assert got[0] is out and got[3] is low and got[4] is high
        assert is_mad_maps_name(st.last_kernel_name, n) and st.last_fallback_pixels == 4
        plain = st.run_deepstack(MAD, SIGMAS[0], SIGMAS[1], REF_LOC)
    assert_mad_maps(got, n, rows=inside)
    assert bits_equal(out[inside], plain[0][inside]) and (got[1], got[2]) == (plain[1], plain[2])
    for a, fill in ((out, np.float32(-7.5)), (low, 0xABCD), (high, 0x1234)):
        assert np.all(a[:inside.start] == fill) and np.all(a[inside.stop:] == fill)


@pytest.mark.parametrize("n", deep.TIGHT_DEPTHS)
def test_two_tile_group_equals_the_single_handle(nl, n):
    with open_handle(nl, n) as st:
        single = maps_pass(st)
    with nl.StackGroup(n, W, H, devices=[0, 0]) as g:
        assert g.size == 2
        split = [g.tile(i).rows for i in range(2)]
        assert sum(split) == H and split[0] != split[1]          # 23 rows: an uneven split
        g.upload_frames(deep.frames_of(n))
        got = g.run_maps_deepstack(MAD, SIGMAS[0], SIGMAS[1], REF_LOC)
        assert all(is_mad_maps_name(g.tile(i).last_kernel_name, n) for i in range(2))
        med = g.run_maps_deepstack(MEDIAN, SIGMAS[0], SIGMAS[1], REF_LOC)
        assert all(g.tile(i).last_kernel_name == "stack_median_ml_kernel<%d>" % deep.lanes_of(n) for i in range(2))
    assert_mad_maps(got, n)
    assert (got[1], got[2]) == (single[1], single[2]) and got[1] > 0 and got[2] > 0
    assert bits_equal(got[0], single[0]) and np.array_equal(got[3], single[3]) and np.array_equal(got[4], single[4])
    assert (med[1], med[2]) == (0, 0) and not med[3].any() and not med[4].any()


def observed(st, mode, sigmas):
    out, cl, ch = st.run(mode, sigmas[0], sigmas[1], REF_LOC)
    return (out.view(np.uint32).copy(), (cl, ch), st.last_kernel_name, st.last_pass_protocol,
            st.last_fallback_pixels, st.last_generic_pixels)


@pytest.mark.parametrize("what", ["mad-700", "mad-1500", "sigma-600"])
def test_default_passes_behind_the_new_passes_are_those_of_a_fresh_handle(nl, what):
    """result bits, totals, kernel name, protocol and both list lengths of default passes, with and without maps passes of
    this tier in front of them"""
    n = int(what.split("-")[1])
    if what.startswith("mad"):
        opener, walk, sig = open_handle, (MAD, MEDIAN, MAD), SIGMAS
    else:
        opener, walk, sig = cases.open_handle, (SIGMA, WINSOR, SIGMA), CLIP_SIGMAS
    with opener(nl, n) as st:
        st.set_dev_flags(NO_SHARED_HINTS)
        fresh = [observed(st, mode, sig) for mode in walk]
    with opener(nl, n) as st:
        st.set_dev_flags(NO_SHARED_HINTS)
        after = []
        for k, mode in enumerate(walk):
            maps_pass(st, mode, TIGHT if k == 2 else sig)
            assert st.last_pass_protocol == 0
            assert "maps" in st.last_kernel_name or mode == MEDIAN, st.last_kernel_name
            assert "stack_exact_kernel" not in st.last_kernel_name
            after.append(observed(st, mode, sig))
    for k in range(3):
        assert np.array_equal(fresh[k][0], after[k][0]) and fresh[k][1:] == after[k][1:], k
        assert "maps" not in fresh[k][2]


def fall_through_handle(nl, what):
    weights = None
    if what == "mad-2049":
        st = nl.StackHandle(2049, 16, 8)
        st.upload_frames(ref.make_frames(2049, 16, 8))
    elif what == "mad-400":
        st = open_handle(nl, 400)
    elif what == "mad-700-forced-exact":
        st = open_handle(nl, 700)
        st.set_exact(1)
    else:
        st = cases.open_handle(nl, 600)
        weights = ref.weights_of(600) if what == "sigma-600-weighted" else None
    st.set_weights(weights)
    st.set_dev_flags(NO_SHARED_HINTS)
    return st


@pytest.mark.parametrize("what", ["mad-400", "linearfit-600", "sigma-600-weighted", "mad-700-forced-exact", "mad-2049"])
def test_fall_throughs_equal_run_maps_full(nl, what):
    """what the engines of this tier do not take is run_maps_full's pass in every observable respect, each entry on a fresh
    handle: result bits, totals, both maps, kernel name, protocol and both list lengths"""
    mode = {"mad": MAD, "linearfit": capi.ST_LINEAR_FIT, "sigma": SIGMA}[what.split("-")[0]]
    seen = {}
    for entry in ("run_maps_full", "run_maps_deepstack"):
        with fall_through_handle(nl, what) as st:
            out, cl, ch, low, high = getattr(st, entry)(mode, SIGMAS[0], SIGMAS[1], REF_LOC)
            assert st.last_mode == mode
            seen[entry] = (out.view(np.uint32).copy(), low, high, (cl, ch), st.last_kernel_name, st.last_pass_protocol,
                           st.last_fallback_pixels, st.last_generic_pixels)
    base, got = seen["run_maps_full"], seen["run_maps_deepstack"]
    print("%s: %s, protocol %d, totals %r" % (what, base[4], base[5], base[3]))
    assert all(np.array_equal(got[k], base[k]) for k in range(3)) and got[3:] == base[3:]
    assert "_ml_kernel<8" not in base[4] and "_ml_kernel<16" not in base[4] and "coop" not in base[4]
    assert base[3][0] + base[3][1] > 0 and "maps" in base[4]


def test_weighted_mad_is_refused_and_the_handle_stays_usable(nl):
    n = 700
    with open_handle(nl, n) as st:
        st.set_weights(ref.weights_of(n))
        with pytest.raises(capi.NlError) as e:
            maps_pass(st)
        assert e.value.code == capi.ERR_WEIGHTED_MAD and "MADSigma" in e.value.message
        with pytest.raises(capi.NlError) as e2:
            maps_pass(st, 9)
        assert e2.value.code == capi.ERR_INVALID_MODE
        st.set_weights(None)
        assert_mad_maps(maps_pass(st), n)
        assert is_mad_maps_name(st.last_kernel_name, n)
