"""Pins drizzle_ref.py, the numpy restatement of include/nlstack_drizzle.h, by hand: cases whose planes are known
without it, the order of the sums, and the completeness of the candidate window -- for every transform any drizzle test
uses, the windowed gather takes exactly the contributions a gather over all source pixels takes.  No device."""
import itertools

import numpy as np
import pytest

import drizzle_ref as ref

f32 = np.float32
IDENTITY = np.array([1, 0, 0, 0, 1, 0], f32)


def test_identity_scale_1_is_the_frame_times_its_weight():
    src = ref.source(7, 5, 1, holes=False)
    w = f32(0.625)
    s, t = ref.accumulate(src, IDENTITY, 1.0, 1.0, 7, 5, weight=w)
    assert ref.geometry(IDENTITY, 1.0, 1.0)[3] == 2
    assert np.array_equal(s.view(np.uint32), (src * w).view(np.uint32)) and np.all(t == w)


def test_identity_scale_2_covers_2x2_outputs_with_area_1():
    src = ref.source(5, 3, 2, holes=False)
    s, t = ref.accumulate(src, IDENTITY, 2.0, 1.0, 10, 6, weight=3.0)
    assert np.all(t == f32(3.0)) and np.array_equal(s, np.repeat(np.repeat(src, 2, 0), 2, 1) * f32(3.0))
    got = {}
    ref.accumulate(src, IDENTITY, 2.0, 1.0, 10, 6, contributions=got)
    assert len(got) == 4 * src.size and all(wa == 1 for wa in got.values())
    assert all((r // 2, c // 2) == (j, i) for j, i, r, c in got)


def test_identity_scale_2_pixfrac_half_gives_area_a_quarter_on_four_outputs():
    src = ref.source(5, 3, 3, holes=False)
    got = {}
    s, t = ref.accumulate(src, IDENTITY, 2.0, 0.5, 10, 6, contributions=got)
    assert len(got) == 4 * src.size and all(wa == f32(0.25) for wa in got.values())
    assert np.all(t == f32(0.25)) and np.array_equal(s, np.repeat(np.repeat(src, 2, 0), 2, 1) * f32(0.25))


def test_nan_is_skipped_and_inf_takes_part():
    src = np.ones((3, 5), f32)
    src[1, 1], src[1, 3] = np.nan, np.inf
    s, t = ref.accumulate(src, IDENTITY, 1.0, 1.0, 5, 3)
    assert s[1, 1] == 0 and t[1, 1] == 0 and s[1, 3] == np.inf and t[1, 3] == 1
    assert np.all(np.delete(s.reshape(-1), [6, 8]) == 1)
    # a drop of Inf beside a pixel it does not overlap leaves that pixel alone (no Inf * 0)
    assert np.isfinite(s[1, 2]) and np.isfinite(s[1, 4])


def test_first_ignores_stale_slots_and_accumulate_adds_to_them():
    a, b = ref.source(5, 3, 4, holes=False), ref.source(5, 3, 5, holes=False)
    stale = np.full((3, 5), np.nan, f32)
    s1, t1 = ref.accumulate(a, IDENTITY, 1.0, 1.0, 5, 3, sum_plane=stale, wgt_plane=stale, first=True, weight=2.0)
    assert np.array_equal(s1, a * f32(2.0)) and np.all(t1 == 2)
    s2, t2 = ref.accumulate(b, IDENTITY, 1.0, 1.0, 5, 3, sum_plane=s1, wgt_plane=t1, first=False, weight=0.5)
    assert np.array_equal(s2, a * f32(2.0) + b * f32(0.5)) and np.all(t2 == f32(2.5))
    s3, _ = ref.accumulate(b, IDENTITY, 1.0, 1.0, 5, 3, sum_plane=stale, wgt_plane=stale, first=False)
    assert np.all(np.isnan(s3))


def test_three_contributions_are_summed_in_candidate_order():
    # three source columns per output column: output pixel 0 collects the drops of source columns 0, 1, 2; the values
    # are chosen so that the sum depends on the order (big + small - big in fp32)
    t3 = np.array([1.0 / 3.0, 0, 0, 0, 1, 0], f32)                   # source column i -> reference i / 3
    assert ref.geometry(t3, 1.0, 1.0)[3] == 3
    areas = {}
    ref.accumulate(np.ones((1, 6), f32), t3, 1.0, 1.0, 2, 1, contributions=areas)
    wa = [areas[(0, i, 0, 0)] for i in range(3)]
    src = np.array([[f32(1e8) / wa[0], f32(1.0) / wa[1], f32(-1e8) / wa[2], 5.0, 6.0, 7.0]], f32)
    got = {}
    s, t = ref.accumulate(src, t3, 1.0, 1.0, 2, 1, contributions=got)
    mine = sorted((i, wa) for (j, i, r, c), wa in got.items() if c == 0)
    assert [i for i, _ in mine] == [0, 1, 2]
    in_order = f32(0)
    for i, wa in mine:
        in_order = f32(in_order + f32(src[0, i] * wa))
    other = f32(f32(f32(src[0, 0] * mine[0][1]) + f32(src[0, 2] * mine[2][1])) + f32(src[0, 1] * mine[1][1]))
    assert s[0, 0] == in_order and in_order != other


def test_point_lays_every_finite_pixel_that_lands_on_exactly_one_output():
    w = f32(0.75)
    for name, make in ref.TRANSFORMS.items():
        src = ref.source(23, 17, 6)
        trans = make(23, 17)
        F, G, hw, R = ref.geometry(trans, 2.0, 0.7)
        got = {}
        s, t = ref.accumulate(src, trans, 2.0, 0.7, 46, 34, weight=w, kernel=ref.POINT, contributions=got)
        jj, ii = np.mgrid[0:17, 0:23].astype(f32)
        u, v = F[0] * ii + F[1] * jj + F[2], F[3] * ii + F[4] * jj + F[5]
        lands = (np.floor(u + f32(0.5)) >= 0) & (np.floor(u + f32(0.5)) < 46) & (np.floor(v + f32(0.5)) >= 0) & \
                (np.floor(v + f32(0.5)) < 34) & ~np.isnan(src)
        assert len(got) == int(lands.sum()), name
        assert float(t.astype(np.float64).sum()) == float(w) * int(lands.sum()), name      # (0.75 n is exact)


def test_a_constant_frame_finalizes_to_the_constant_where_weight_landed():
    # (a power of two: every product and sum is the weight plane's, scaled, so the quotient is exact)
    src = np.full((17, 23), 4.0, f32)
    for name, make in ref.TRANSFORMS.items():
        s, t = ref.accumulate(src, make(23, 17), 2.0, 0.7, 46, 34, weight=1.0)
        out = ref.finalize(s, t, 0.0, -1.0)
        assert np.all(out[t > 0] == 4.0), name
        assert np.all(out[~(t > 0)] == -1.0) and (name == "all-out") == (not np.any(t > 0))
    assert np.array_equal(ref.finalize([1, 2, 3, 4], [2, 0, np.nan, 0.25], 0.25, -7.0), np.array([0.5, -7, -7, -7], f32))


def test_reject_against():
    v = np.array([1, 5, -3, np.nan, 2, 2.5, 0.5], f32)
    m = np.array([1, 1, 1, 1, np.nan, 1, 1], f32)
    out, lo, hi = ref.reject_against(v, m, 1.0, 1.5)
    assert (lo, hi) == (1, 1) and ref.same(out, [1, np.nan, np.nan, np.nan, 2, 2.5, 0.5])
    assert np.array_equal(out[[0, 4, 5, 6]].view(np.uint32), v[[0, 4, 5, 6]].view(np.uint32))


# ---- completeness of the window ------------------------------------------------------------------------------------------

SOURCES = [(5, 3), (23, 17)]
SCALES = [1.0, 1.5, 2.0, 3.0]
PIXFRACS = [0.5, 0.7, 0.9, 1.0]


def _window_cases():
    cases = []
    for (w, h), (name, make) in itertools.product(SOURCES, ref.TRANSFORMS.items()):
        for k, (S, p) in enumerate(itertools.product(SCALES, PIXFRACS)):
            # every scale and pixfrac with every transform and source, a third of the products each
            if (k + len(name) + w) % 3 == 0:
                cases.append(("%dx%d-%s-S%g-p%g" % (w, h, name, S, p), w, h, make(w, h), S, p))
    for deg, mag in itertools.product((0, 13, 30, 45, 90, 180), (0.97, 1.0, 1.02)):
        for w, h in SOURCES:
            S, p = SCALES[(deg + w) % 4], PIXFRACS[(deg // 13 + h) % 4]
            cases.append(("%dx%d-rot%d-m%g-S%g-p%g" % (w, h, deg, mag, S, p), w, h,
                          ref.rotation(w, h, deg, mag, 0.31, -0.17), S, p))
    # the shapes and pixfracs the device tests use, on the small sources
    for cid, name, (w, h), _, S, p, _ in ref.gpu_cases():
        if name in ref.TRANSFORMS:
            cases.append(("gpu-" + cid, 23, 17, ref.TRANSFORMS[name](23, 17), S, p))
    name, make, S, p = ref.R3
    cases += [("%dx%d-%s" % (w, h, name), w, h, make(w, h), S, p) for w, h in SOURCES]
    name, make, S, p = ref.R1
    cases += [("%dx%d-%s" % (w, h, name), w, h, make(w, h), S, p) for w, h in SOURCES]
    return cases


WINDOW_CASES = _window_cases()


@pytest.mark.parametrize("case", WINDOW_CASES, ids=[c[0] for c in WINDOW_CASES])
def test_the_window_holds_every_contribution(case):
    _, w, h, trans, S, p = case
    ow, oh = int(round(S * w)), int(round(S * h))
    src = ref.source(w, h, 11)
    for kernel in (ref.TURBO, ref.POINT):
        win, brute = {}, {}
        s, t = ref.accumulate(src, trans, S, p, ow, oh, weight=1.25, kernel=kernel, contributions=win)
        sb, tb = ref.accumulate_brute(src, trans, S, p, ow, oh, weight=1.25, kernel=kernel, contributions=brute)
        assert win.keys() == brute.keys() and all(win[k] == brute[k] for k in win)
        assert ref.same(s, sb) and ref.same(t, tb)


def test_the_radius_3_case_and_the_radius_4_case():
    name, make, S, p = ref.R3
    assert ref.geometry(make(67, 35), S, p)[3] == 3
    # (R is a bound, not the least radius: a window of 0 loses contributions, what a window of 1 loses depends on the turn)
    src = ref.source(23, 17, 12, holes=False)
    full, short = {}, {}
    ref.accumulate(src, make(23, 17), S, p, 23, 17, contributions=full)
    ref.accumulate(src, make(23, 17), S, p, 23, 17, radius=0, contributions=short)
    assert len(short) < len(full) and short.items() <= full.items()
    name, make, S, p = ref.R4
    with pytest.raises(ref.GeometryError, match="radius 4"):
        ref.geometry(make(67, 35), S, p)


def test_the_radii_of_the_cases_are_1_to_3():
    radii = {ref.geometry(trans, S, p)[3] for _, _, _, _, S, p, trans in ref.gpu_cases()}
    assert radii == {1, 2, 3}, radii
