"""GPU: which kernel, protocol and engine every pass entry lands on, pinned row by row.

The launchers of the stack kernels take one nl::Form (stack_kernels.h: Plain, Maps, Follow, Record) and select_engine hands
every pass kind its engine.  That was a host-side refactor, and ROWS below is its fence: the table was RECORDED FROM THE
PARENT BUILD (commit a715147, before the refactor) by running these very rows, one fresh handle and one pass each, and every
later build must give the same last_kernel_name, last_pass_protocol and "the exact list was used" for each of them.  Results
are not compared here: test_gpu_rejmap / fastmaps / residentmaps / deepmaps / fullmaps / wlinfit / wclip / wmad do that
against the oracle.

A row is (entry, mode, active frames, weights, set_exact) -> (kernel name, protocol, fallback pixels > 0).  The image is
41 x 23 = 943 pixels; the frames are those of maps_cases (up to 128 frames) and deepmaps_frames (beyond), which hold pixels
for the generic list and three for the exact list.  The depths reach every launcher in every form: 7 the generic-only
network, 24 zonal, 100 stack_mad_fast_kernel<112>, 120 the bitonic MAD kernel and its finisher, 200 two lanes per pixel,
300 four.  Every handle runs without the process-wide list-length hints, so a row does not depend on the rows before it."""
import numpy as np
import pytest

import deepmaps_frames as deep
import maps_cases as cases
from nightlight_amd import capi

pytestmark = pytest.mark.gpu

W, H = cases.W, cases.H
REF_LOC = cases.REF_LOC
NO_SHARED_HINTS = 512       # developer switch: no list-length hints from earlier handles of the same geometry
MEDIAN, SIGMA, WINSOR, MAD, LINFIT = capi.ST_MEDIAN, capi.ST_SIGMA, capi.ST_WINSOR_SIGMA, capi.ST_MAD_SIGMA, capi.ST_LINEAR_FIT


def frames_and_sigmas(n):
    return (cases.frames_of(n), (cases.SIGMA_LOW, cases.SIGMA_HIGH)) if n <= 128 else (deep.frames_of(n), deep.SIGMAS)


def run_entry(st, entry, mode, sigmas):
    lo, hi = sigmas
    if entry == "run":
        return st.run(mode, lo, hi, REF_LOC)
    if entry == "run_maps":
        return st.run_maps(mode, lo, hi, REF_LOC)
    if entry == "run_maps_fast":
        return st.run_maps(mode, lo, hi, REF_LOC, fast=True)
    if entry in ("run_maps_resident", "run_maps_deep", "run_maps_full"):
        return getattr(st, entry)(mode, lo, hi, REF_LOC)
    if entry == "run_clip_weighted":
        return st.run_clip_weighted(mode, lo, hi, REF_LOC)
    assert entry in ("run_linfit_weighted", "run_mad_weighted")
    return getattr(st, entry)(lo, hi, REF_LOC)


def observe(nl, entry, mode, n, weights, exact):
    """one fresh handle, one pass: (kernel name, protocol, fallback pixels > 0)"""
    frames, sigmas = frames_and_sigmas(n)
    with nl.StackHandle(n, W, H) as st:
        st.set_dev_flags(NO_SHARED_HINTS)
        st.upload_frames(frames)
        if weights:
            st.set_weights(np.linspace(0.5, 1.5, n, dtype=np.float32))
        if exact:
            st.set_exact(1)
        run_entry(st, entry, mode, sigmas)
        return st.last_kernel_name, st.last_pass_protocol, st.last_fallback_pixels > 0


# recorded from the parent build (see above): entry, mode, frames, weights, set_exact, kernel name, protocol, exact list used
ROWS = [
    # the default pass, unweighted
    ("run", 0, 7, 0, 0, "stack_median_fast_kernel<8, false>", 0, False),
    ("run", 0, 24, 0, 0, "stack_median_fast_kernel<32, true>", 0, False),
    ("run", 0, 100, 0, 0, "stack_median_fast_kernel<112, true>", 0, False),
    ("run", 0, 120, 0, 0, "stack_median_fast_kernel<128, true>", 0, False),
    ("run", 0, 200, 0, 0, "stack_median_ml_kernel<2>", 0, False),
    ("run", 0, 300, 0, 0, "stack_median_ml_kernel<4>", 0, False),
    ("run", 2, 7, 0, 0, "stack_sigma_fast_kernel<8, false, false, false, false, false>", 0, True),
    ("run", 2, 24, 0, 0, "stack_sigma_fast_kernel<24, true, false, true, false, false>", 0, True),
    ("run", 2, 100, 0, 0, "stack_sigma_fast_kernel<112, true, false, false, false, false>", 0, True),
    ("run", 2, 120, 0, 0, "stack_sigma_fast_kernel<128, true, false, false, false, false>", 0, True),
    ("run", 2, 200, 0, 0, "stack_sigma_mlz_kernel<2, false, 208, 0>", 0, True),
    ("run", 2, 300, 0, 0, "stack_sigma_mlz_kernel<4, false, 304, 0>", 0, True),
    ("run", 3, 7, 0, 0, "stack_sigma_fast_kernel<8, false, true, false, false, false>", 0, True),
    ("run", 3, 24, 0, 0, "stack_sigma_fast_kernel<24, true, true, true, false, false>", 0, True),
    ("run", 3, 100, 0, 0, "stack_sigma_fast_kernel<112, true, true, false, false, false>", 0, True),
    ("run", 3, 120, 0, 0, "stack_sigma_fast_kernel<128, true, true, false, false, false>", 0, True),
    ("run", 3, 200, 0, 0, "stack_sigma_mlz_kernel<2, true, 208, 0>", 0, True),
    ("run", 3, 300, 0, 0, "stack_sigma_mlz_kernel<4, true, 304, 0>", 0, True),
    ("run", 4, 7, 0, 0, "stack_mad_fast_kernel<8>", 0, False),
    ("run", 4, 24, 0, 0, "stack_mad_fast_kernel<32>", 0, False),
    ("run", 4, 100, 0, 0, "stack_mad_fast_kernel<112>", 0, False),
    ("run", 4, 120, 0, 0, "stack_mad_bitonic_kernel", 0, False),
    ("run", 4, 200, 0, 0, "stack_mad_ml_kernel<2>", 0, False),
    ("run", 4, 300, 0, 0, "stack_mad_ml_kernel<4>", 0, False),
    ("run", 5, 7, 0, 0, "stack_linfit_fast_kernel<8, false>", 0, True),
    ("run", 5, 24, 0, 0, "stack_linfit_fast_kernel<32, false>", 0, True),
    ("run", 5, 100, 0, 0, "stack_linfit_fast_kernel<128, false>", 0, True),
    ("run", 5, 120, 0, 0, "stack_linfit_fast_kernel<128, false>", 0, True),
    ("run", 5, 200, 0, 0, "stack_linfit_ml_kernel<2, false>", 0, True),
    ("run", 5, 300, 0, 0, "stack_linfit_ml_kernel<4, false>", 0, True),
    # ... weighted: the tile replay, the decision pass and the wave-per-pixel replay
    ("run", 2, 7, 1, 0, "stack_sigma_tile_kernel<sigma,weighted>", 0, False),
    ("run", 2, 24, 1, 0, "stack_sigma_tile_kernel<sigma,weighted>", 0, False),
    ("run", 2, 100, 1, 0, "stack_sigma_coop_kernel<false, true, 1, 2>", 0, False),
    ("run", 2, 200, 1, 0, "stack_sigma_coop_kernel<false, true, 1, 2>", 0, False),
    ("run", 3, 7, 1, 0, "stack_sigma_tile_kernel<winsor,weighted>", 0, False),
    ("run", 3, 24, 1, 0, "stack_sigma_tile_kernel<winsor,weighted>", 0, False),
    ("run", 3, 100, 1, 0, "stack_sigma_coop_kernel<true, true, 1, 2>", 0, False),
    ("run", 3, 200, 1, 0, "stack_sigma_coop_kernel<true, true, 1, 2>", 0, False),
    # the five maps tiers
    ("run_maps", 0, 24, 0, 0, "stack_exact_kernel<median,maps>", 0, False),
    ("run_maps", 2, 24, 0, 0, "stack_exact_kernel<sigma,maps>", 0, False),
    ("run_maps", 3, 24, 0, 0, "stack_exact_kernel<winsor,maps>", 0, False),
    ("run_maps", 4, 24, 0, 0, "stack_exact_kernel<mad,maps>", 0, False),
    ("run_maps", 5, 24, 0, 0, "stack_exact_kernel<linearfit,maps>", 0, False),
    ("run_maps", 2, 24, 1, 0, "stack_exact_kernel<sigma,weighted,maps>", 0, False),
    ("run_maps_fast", 2, 7, 0, 0, "stack_sigma_fast_kernel<8, false, false, false, false, false, maps>", 0, True),
    ("run_maps_fast", 2, 24, 0, 0, "stack_sigma_fast_kernel<24, true, false, true, false, false, maps>", 0, True),
    ("run_maps_fast", 2, 100, 0, 0, "stack_sigma_fast_kernel<112, true, false, false, false, false, maps>", 0, True),
    ("run_maps_fast", 2, 120, 0, 0, "stack_sigma_fast_kernel<128, true, false, false, false, false, maps>", 0, True),
    ("run_maps_fast", 2, 200, 0, 0, "stack_exact_kernel<sigma,maps>", 0, False),
    ("run_maps_fast", 2, 300, 0, 0, "stack_exact_kernel<sigma,maps>", 0, False),
    ("run_maps_fast", 3, 7, 0, 0, "stack_sigma_fast_kernel<8, false, true, false, false, false, maps>", 0, True),
    ("run_maps_fast", 3, 24, 0, 0, "stack_sigma_fast_kernel<24, true, true, true, false, false, maps>", 0, True),
    ("run_maps_fast", 3, 100, 0, 0, "stack_sigma_fast_kernel<112, true, true, false, false, false, maps>", 0, True),
    ("run_maps_fast", 3, 120, 0, 0, "stack_sigma_fast_kernel<128, true, true, false, false, false, maps>", 0, True),
    ("run_maps_fast", 3, 200, 0, 0, "stack_exact_kernel<winsor,maps>", 0, False),
    ("run_maps_fast", 3, 300, 0, 0, "stack_exact_kernel<winsor,maps>", 0, False),
    ("run_maps_fast", 5, 24, 0, 0, "stack_exact_kernel<linearfit,maps>", 0, False),
    ("run_maps_resident", 5, 7, 0, 0, "stack_linfit_fast_kernel<8, false, maps>", 0, True),
    ("run_maps_resident", 5, 24, 0, 0, "stack_linfit_fast_kernel<32, false, maps>", 0, True),
    ("run_maps_resident", 5, 100, 0, 0, "stack_linfit_fast_kernel<128, false, maps>", 0, True),
    ("run_maps_resident", 5, 120, 0, 0, "stack_linfit_fast_kernel<128, false, maps>", 0, True),
    ("run_maps_resident", 5, 200, 0, 0, "stack_linfit_ml_kernel<2, false, maps>", 0, True),
    ("run_maps_resident", 5, 300, 0, 0, "stack_linfit_ml_kernel<4, false, maps>", 0, True),
    ("run_maps_resident", 2, 24, 0, 0, "stack_sigma_fast_kernel<24, true, false, true, false, false, maps>", 0, True),
    ("run_maps_deep", 2, 24, 0, 0, "stack_sigma_fast_kernel<24, true, false, true, false, false, maps>", 0, True),
    ("run_maps_deep", 2, 200, 0, 0, "stack_sigma_mlz_kernel<2, false, 208, 0, maps>", 0, True),
    ("run_maps_deep", 2, 300, 0, 0, "stack_sigma_mlz_kernel<4, false, 304, 0, maps>", 0, True),
    ("run_maps_deep", 3, 24, 0, 0, "stack_sigma_fast_kernel<24, true, true, true, false, false, maps>", 0, True),
    ("run_maps_deep", 3, 200, 0, 0, "stack_sigma_mlz_kernel<2, true, 208, 0, maps>", 0, True),
    ("run_maps_deep", 3, 300, 0, 0, "stack_sigma_mlz_kernel<4, true, 304, 0, maps>", 0, True),
    ("run_maps_deep", 4, 120, 0, 0, "stack_exact_kernel<mad,maps>", 0, False),
    ("run_maps_full", 4, 7, 0, 0, "stack_mad_fast_kernel<8, maps>", 0, False),
    ("run_maps_full", 4, 24, 0, 0, "stack_mad_fast_kernel<32, maps>", 0, False),
    ("run_maps_full", 4, 100, 0, 0, "stack_mad_fast_kernel<112, maps>", 0, False),
    ("run_maps_full", 4, 120, 0, 0, "stack_mad_bitonic_kernel<maps>", 0, False),
    ("run_maps_full", 4, 200, 0, 0, "stack_mad_ml_kernel<2, maps>", 0, False),
    ("run_maps_full", 4, 300, 0, 0, "stack_mad_ml_kernel<4, maps>", 0, False),
    ("run_maps_full", 0, 24, 0, 0, "stack_median_fast_kernel<32, true>", 0, False),
    ("run_maps_full", 0, 200, 0, 0, "stack_median_ml_kernel<2>", 0, False),
    ("run_maps_full", 2, 24, 0, 0, "stack_sigma_fast_kernel<24, true, false, true, false, false, maps>", 0, True),
    ("run_maps_full", 2, 300, 0, 0, "stack_sigma_mlz_kernel<4, false, 304, 0, maps>", 0, True),
    ("run_maps_full", 3, 300, 0, 0, "stack_sigma_mlz_kernel<4, true, 304, 0, maps>", 0, True),
    ("run_maps_full", 5, 100, 0, 0, "stack_linfit_fast_kernel<128, false, maps>", 0, True),
    ("run_maps_full", 5, 300, 0, 0, "stack_linfit_ml_kernel<4, false, maps>", 0, True),
    # the three weighted entries
    ("run_linfit_weighted", 5, 7, 1, 0, "stack_linfit_weighted_kernel<8>", 0, True),
    ("run_linfit_weighted", 5, 24, 1, 0, "stack_linfit_weighted_kernel<32>", 0, True),
    ("run_linfit_weighted", 5, 100, 1, 0, "stack_linfit_weighted_kernel<128>", 0, True),
    ("run_linfit_weighted", 5, 120, 1, 0, "stack_linfit_weighted_kernel<128>", 0, True),
    ("run_linfit_weighted", 5, 200, 1, 0, "stack_exact_kernel<linfit,weighted>", 0, False),
    ("run_linfit_weighted", 5, 300, 1, 0, "stack_exact_kernel<linfit,weighted>", 0, False),
    ("run_clip_weighted", 2, 7, 1, 0, "stack_exact_kernel<sigma,follow>", 0, False),
    ("run_clip_weighted", 2, 24, 1, 0, "stack_clip_weighted_kernel<1>", 0, True),
    ("run_clip_weighted", 2, 100, 1, 0, "stack_clip_weighted_kernel<1>", 0, True),
    ("run_clip_weighted", 2, 200, 1, 0, "stack_clip_weighted_kernel<1>", 0, True),
    ("run_clip_weighted", 3, 7, 1, 0, "stack_exact_kernel<winsor,follow>", 0, False),
    ("run_clip_weighted", 3, 24, 1, 0, "stack_clip_weighted_kernel<1>", 0, True),
    ("run_clip_weighted", 3, 100, 1, 0, "stack_clip_weighted_kernel<1>", 0, True),
    ("run_clip_weighted", 3, 200, 1, 0, "stack_clip_weighted_kernel<1>", 0, True),
    ("run_mad_weighted", 4, 7, 1, 0, "stack_mad_fast_kernel<8, true>", 0, False),
    ("run_mad_weighted", 4, 24, 1, 0, "stack_mad_fast_kernel<32, true>", 0, False),
    ("run_mad_weighted", 4, 100, 1, 0, "stack_mad_fast_kernel<112, true>", 0, False),
    ("run_mad_weighted", 4, 120, 1, 0, "stack_mad_bitonic_kernel<true>", 0, False),
    ("run_mad_weighted", 4, 200, 1, 0, "stack_clip_weighted_kernel<1, true>", 0, True),
    ("run_mad_weighted", 4, 300, 1, 0, "stack_clip_weighted_kernel<1, true>", 0, True),
    # ... behind set_exact(1): the column kernel over the whole tile
    ("run_linfit_weighted", 5, 24, 1, 1, "stack_exact_kernel<linfit,weighted>", 0, False),
    ("run_clip_weighted", 2, 24, 1, 1, "stack_exact_kernel<sigma,follow>", 0, False),
    ("run_mad_weighted", 4, 24, 1, 1, "stack_exact_kernel<mad,follow>", 0, False),
]


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "%s-m%d-n%d%s%s" % (r[0], r[1], r[2], "-w" if r[3] else "", "-exact" if r[4] else ""))
def test_entry_lands_on_the_parents_kernel_protocol_and_engine(nl, row):
    entry, mode, n, weights, exact, name, protocol, listed = row
    assert observe(nl, entry, mode, n, weights, exact) == (name, protocol, listed)


# recorded from the parent build as well: code and full message of the three refusals
REFUSALS = [
    ("run_linfit_weighted", 5, -6, "run_linfit_weighted: the handle has no weights (nl_stack_set_weights); "
                                   "the unweighted fit is nl_stack_run with NL_ST_LINEAR_FIT"),
    ("run_clip_weighted", 2, -6, "run_clip_weighted: the handle has no weights (nl_stack_set_weights); the unweighted pass is nl_stack_run"),
    ("run_mad_weighted", 4, -6, "run_mad_weighted: the handle has no weights (nl_stack_set_weights); "
                                "the unweighted pass is nl_stack_run with NL_ST_MAD_SIGMA"),
]


@pytest.mark.parametrize("refusal", REFUSALS, ids=lambda r: r[0])
def test_weighted_entries_refuse_a_handle_without_weights(nl, refusal):
    entry, mode, code, message = refusal
    with nl.StackHandle(7, W, H) as st:
        st.upload_frames(cases.frames_of(7))
        with pytest.raises(capi.NlError) as err:
            run_entry(st, entry, mode, (cases.SIGMA_LOW, cases.SIGMA_HIGH))
    assert (err.value.code, err.value.message) == (code, message)
