"""Pins sqdrizzle_ref.py, the numpy restatement of include/nlstack_sqdrizzle.h, by hand: cases whose planes are known
without it (the identity, the diamond of a 45 degree turn magnified by sqrt 2, whose coordinates are all exact in fp32),
the order of the sums, every area against a float64 polygon clip, the area a whole drop lays down, and the completeness
of the candidate window -- for every transform any square drizzle test uses, the windowed gather takes exactly the
contributions a gather over all source pixels takes.  No device.

The yardstick of an area is the float64 clip of the polygon whose corners are the definition's own x_k, y_k (fp32 values):
it judges the edge arithmetic, not the rounding of u and vv, which belongs to the definition as it does for NL_DZ_TURBO
(half an ulp of a coordinate of 300 is 1.5e-5; against the geometry carried in float64 throughout the same areas differ
by up to 3.5e-5).

Measured here (the maxima over the 221 888 candidates of all device cases): |ar - exact| 1.57e-7 against the bar 2^-20;
the largest area taken where the exact overlap is zero 0; over 38 039 drops that lie whole inside the grid, the sum of a
drop's areas against p^2 |det F| 2.95e-7 against the bar 1e-5."""
import itertools

import numpy as np
import pytest

import drizzle_ref as ref
import sqdrizzle_ref as sq

f32 = np.float32
IDENTITY = np.array([1, 0, 0, 0, 1, 0], f32)
DIAMOND = np.array([1, -1, 3, 1, 1, -3], f32)              # a turn of 45 degrees magnified by sqrt 2; (3, 3) stays
MIRRORED = np.array([1, 1, -3, 1, -1, 3], f32)             # the same drop with det < 0; (3, 3) stays
AREA_BAR = 2.0 ** -20
DROP_BAR = 1e-5


def test_identity_scale_1_is_the_frame_times_its_weight():
    src = ref.source(7, 5, 1, holes=False)
    w = f32(0.625)
    got = {}
    s, t = sq.accumulate_square(src, IDENTITY, 1.0, 1.0, 7, 5, weight=w, contributions=got)
    assert sq.geometry_square(IDENTITY, 1.0, 1.0)[4] == 2
    assert np.array_equal(s.view(np.uint32), (src * w).view(np.uint32)) and np.all(t == w)
    assert len(got) == src.size and all((j, i) == (r, c) and wa == w for (j, i, r, c), wa in got.items())


def test_identity_scale_2_covers_2x2_outputs_with_area_1():
    src = ref.source(5, 3, 2, holes=False)
    got = {}
    s, t = sq.accumulate_square(src, IDENTITY, 2.0, 1.0, 10, 6, weight=3.0, contributions=got)
    assert np.all(t == f32(3.0)) and np.array_equal(s, np.repeat(np.repeat(src, 2, 0), 2, 1) * f32(3.0))
    assert len(got) == 4 * src.size and all(wa == 3 for wa in got.values())
    assert all((r // 2, c // 2) == (j, i) for j, i, r, c in got)


def test_identity_scale_2_pixfrac_half_gives_area_a_quarter_on_four_outputs():
    src = ref.source(5, 3, 3, holes=False)
    got = {}
    s, t = sq.accumulate_square(src, IDENTITY, 2.0, 0.5, 10, 6, contributions=got)
    assert len(got) == 4 * src.size and all(wa == f32(0.25) for wa in got.values())
    assert np.all(t == f32(0.25)) and np.array_equal(s, np.repeat(np.repeat(src, 2, 0), 2, 1) * f32(0.25))


def _areas_of_pixel_3_3(trans):
    got = {}
    sq.accumulate_square(np.ones((7, 7), f32), trans, 1.0, 1.0, 7, 7, contributions=got)
    return {(r - 3, c - 3): wa for (j, i, r, c), wa in got.items() if (j, i) == (3, 3)}


def test_the_diamond_lays_1_on_its_own_pixel_and_a_quarter_on_each_edge_neighbour():
    F, G, corners, box, R = sq.geometry_square(DIAMOND, 1.0, 1.0)
    assert np.array_equal(F, DIAMOND) and np.array_equal(box, [1, 1])
    assert np.array_equal(corners, [[0, -1], [-1, 0], [0, 1], [1, 0]])                    # the diamond |x| + |y| <= 1
    mine = _areas_of_pixel_3_3(DIAMOND)
    quarter = f32(0.25)
    assert mine == {(0, 0): f32(1.0), (-1, 0): quarter, (1, 0): quarter, (0, -1): quarter, (0, 1): quarter}
    for key in ((-1, -1), (-1, 1), (1, -1), (1, 1)):                                      # the diagonal neighbours
        assert key not in mine
    # what the kernel is for: the turbo drop of the same call is the square of side sqrt 2 around (3, 3) and puts
    # weight on the diagonal neighbours, and other numbers on the rest
    turbo = {}
    ref.accumulate(np.ones((7, 7), f32), DIAMOND, 1.0, 1.0, 7, 7, contributions=turbo)
    turbo = {(r - 3, c - 3): wa for (j, i, r, c), wa in turbo.items() if (j, i) == (3, 3)}
    assert turbo[(0, 0)] == 1 and (1, 1) in turbo and turbo[(1, 1)] > 0.04
    assert abs(float(turbo[(0, 1)]) - 0.2071) < 1e-3 and turbo[(0, 1)] != mine[(0, 1)]
    assert abs(sum(float(v) for v in turbo.values()) - 2.0) < 1e-6 and sum(float(v) for v in mine.values()) == 2.0


def test_the_mirrored_transform_gives_the_same_areas():
    F, G, corners, box, R = sq.geometry_square(MIRRORED, 1.0, 1.0)
    assert F[0] * F[4] - F[1] * F[3] < 0
    # the reversed order: the same diamond walked so that the edge sum is positive
    assert np.array_equal(corners, [[0, 1], [1, 0], [0, -1], [-1, 0]])
    assert _areas_of_pixel_3_3(MIRRORED) == _areas_of_pixel_3_3(DIAMOND)
    flip = ref.TRANSFORMS["flip"](7, 5)
    src = ref.source(7, 5, 4, holes=False)
    s, t = sq.accumulate_square(src, flip, 1.0, 1.0, 7, 5)
    assert np.all(t[1:] > 0.999) and np.all(t >= 0)


def test_contributions_are_summed_in_candidate_order():
    # three source columns per output column (the form of test_drizzle_ref.py): output pixel 1 collects the drops of
    # source columns 2, 3 and 4, whose sides meet on its borders (a fourth may add an area of rounding size: its value
    # is 0); the values are chosen so that the sum depends on the order (big + small - big in fp32)
    t3 = np.array([1.0 / 3.0, 0, 0, 0, 1, 0], f32)
    assert sq.geometry_square(t3, 1.0, 1.0)[4] == 3
    areas = {}
    sq.accumulate_square(np.ones((1, 9), f32), t3, 1.0, 1.0, 3, 1, contributions=areas)
    mine = [(i, wa) for (j, i, r, c), wa in areas.items() if c == 1]                      # in the order taken
    cols = [i for i, wa in mine if wa > 0.3]
    assert cols == [2, 3, 4] and [i for i, _ in mine] == sorted(i for i, _ in mine)
    wa = dict(mine)
    src = np.zeros((1, 9), f32)
    src[0, 2], src[0, 3], src[0, 4] = f32(1e8) / wa[2], f32(1.0) / wa[3], f32(-1e8) / wa[4]
    s, t = sq.accumulate_square(src, t3, 1.0, 1.0, 3, 1)
    in_order = f32(0)
    for i, a in mine:
        in_order = f32(in_order + f32(src[0, i] * a))
    other = f32(f32(f32(src[0, 2] * wa[2]) + f32(src[0, 4] * wa[4])) + f32(src[0, 3] * wa[3]))
    assert s[0, 1] == in_order and in_order != other


def test_nan_is_skipped_and_inf_takes_part():
    src = np.ones((3, 5), f32)
    src[1, 1], src[1, 3] = np.nan, np.inf
    s, t = sq.accumulate_square(src, IDENTITY, 1.0, 1.0, 5, 3)
    assert s[1, 1] == 0 and t[1, 1] == 0 and s[1, 3] == np.inf and t[1, 3] == 1
    assert np.all(np.delete(s.reshape(-1), [6, 8]) == 1)
    assert np.isfinite(s[1, 2]) and np.isfinite(s[1, 4])


def test_first_ignores_stale_slots_and_accumulate_adds_to_them():
    a, b = ref.source(5, 3, 4, holes=False), ref.source(5, 3, 5, holes=False)
    stale = np.full((3, 5), np.nan, f32)
    s1, t1 = sq.accumulate_square(a, IDENTITY, 1.0, 1.0, 5, 3, sum_plane=stale, wgt_plane=stale, first=True, weight=2.0)
    assert np.array_equal(s1, a * f32(2.0)) and np.all(t1 == 2)
    s2, t2 = sq.accumulate_square(b, IDENTITY, 1.0, 1.0, 5, 3, sum_plane=s1, wgt_plane=t1, first=False, weight=0.5)
    assert np.array_equal(s2, a * f32(2.0) + b * f32(0.5)) and np.all(t2 == f32(2.5))
    s3, _ = sq.accumulate_square(b, IDENTITY, 1.0, 1.0, 5, 3, sum_plane=stale, wgt_plane=stale, first=False)
    assert np.all(np.isnan(s3))


# ---- the areas against the float64 clip ---------------------------------------------------------------------------------

def test_exact_overlap_by_hand():
    assert sq.exact_overlap([(0, 0), (1, 0), (1, 1), (0, 1)]) == 1.0
    assert sq.exact_overlap([(0.5, -0.5), (1.5, 0.5), (0.5, 1.5), (-0.5, 0.5)]) == 1.0   # the diamond around the pixel
    assert sq.exact_overlap([(1.5, -0.5), (2.5, 0.5), (1.5, 1.5), (0.5, 0.5)]) == 0.25   # around its neighbour
    assert sq.exact_overlap([(1.5, 0.5), (0.5, 1.5), (1.5, 2.5), (2.5, 1.5)]) == 0.0     # the diagonal one, clockwise
    assert sq.exact_overlap([(0.25, 0.25), (0.75, 0.25), (0.75, 0.5), (0.25, 0.5)]) == 0.125
    assert sq.exact_overlap([(2, 2), (3, 2), (3, 3), (2, 3)]) == 0.0


def _area_errors(case):
    """over every candidate of every pixel of a device case: (worst |ar - exact| over the candidates in the bounding
    box, the largest ar taken where the exact overlap is zero, worst |sum of a drop's areas - p^2 |det F|| over the
    drops that lie whole inside the grid, how many candidates, how many such drops)"""
    _, _, (w, h), (ow, oh), S, p, trans = case
    F, G, corners, box, R = sq.geometry_square(trans, S, p)
    px, py, xc, yc = ref._centres(G, ow, 0, oh)
    xi, yi = xc.astype(np.int64), yc.astype(np.int64)
    F64 = F.astype(np.float64)
    cols, rows = np.broadcast_to(px, xc.shape).astype(np.float64), np.broadcast_to(py, xc.shape).astype(np.float64)
    worst = stray = 0.0
    n = 0
    total = np.zeros((h, w))
    for dj, di in itertools.product(range(-R, R + 1), repeat=2):
        j, i = yi + dj, xi + di
        take, _, ar = sq._candidate(F, corners, box, i.astype(f32), j.astype(f32), px, py, 1.0)
        inside = (i >= 0) & (i < w) & (j >= 0) & (j < h)
        u, vv = F64[0] * i + F64[1] * j + F64[2], F64[3] * i + F64[4] * j + F64[5]
        boxed = (np.abs(u - cols) < 0.5 + float(box[0])) & (np.abs(vv - rows) < 0.5 + float(box[1]))
        m = (boxed | take) & inside
        if not m.any():
            continue
        exact = sq.exact_overlap(sq.drop_polygon(F, corners, i[m].astype(f32), j[m].astype(f32), cols[m].astype(f32),
                                                 rows[m].astype(f32)))
        got = np.where(take[m], ar[m].astype(np.float64), 0.0)
        worst = max(worst, float(np.abs(got - exact).max()))
        stray = max(stray, float(got[exact == 0.0].max(initial=0.0)))
        np.add.at(total, (j[m], i[m]), got)
        n += int(m.sum())
    want = float(f32(p)) ** 2 * abs(F64[0] * F64[4] - F64[1] * F64[3])
    reach = 1.0 + float(max(box))
    jj, ii = np.mgrid[0:h, 0:w].astype(np.float64)
    u, vv = F64[0] * ii + F64[1] * jj + F64[2], F64[3] * ii + F64[4] * jj + F64[5]
    interior = (u >= reach) & (u <= ow - 1 - reach) & (vv >= reach) & (vv <= oh - 1 - reach)
    drops = np.abs(total[interior] - want)
    return worst, stray, float(drops.max(initial=0.0)), n, int(interior.sum())


AREA_CASES = sq.gpu_cases()                                # every device case, the two turns included


def test_every_area_against_the_float64_clip():
    worst = stray = drop = 0.0
    n = drops = 0
    for case in AREA_CASES:
        a, b, c, k, m = _area_errors(case)
        worst, stray, drop, n, drops = max(worst, a), max(stray, b), max(drop, c), n + k, drops + m
    print("candidates %d: worst |ar - exact| %.3g (bar %.3g), largest area where the exact overlap is zero %.3g; "
          "interior drops %d: worst |sum - p^2 |det F|| %.3g (bar %.3g)" % (n, worst, AREA_BAR, stray, drops, drop, DROP_BAR))
    assert n > 100000 and drops > 5000
    assert worst <= AREA_BAR
    assert stray <= AREA_BAR
    assert drop <= DROP_BAR


# ---- completeness of the window ------------------------------------------------------------------------------------------

SOURCES = [(5, 3), (23, 17)]
SCALES = [1.0, 1.5, 2.0, 3.0]
PIXFRACS = [0.5, 0.7, 0.9, 1.0]


def _window_cases():
    cases = []
    for (w, h), (name, make) in itertools.product(SOURCES, ref.TRANSFORMS.items()):
        for k, (S, p) in enumerate(itertools.product(SCALES, PIXFRACS)):
            if (k + len(name) + w) % 6 == 0:
                cases.append(("%dx%d-%s-S%g-p%g" % (w, h, name, S, p), w, h, make(w, h), S, p))
    for deg, mag in itertools.product((0, 13, 30, 45, 90, 180), (0.97, 1.02)):
        w, h = SOURCES[1]
        S, p = SCALES[(deg + w) % 4], PIXFRACS[(deg // 13 + h) % 4]
        cases.append(("%dx%d-rot%d-m%g-S%g-p%g" % (w, h, deg, mag, S, p), w, h, ref.rotation(w, h, deg, mag, 0.31, -0.17), S, p))
    # every transform, scale and pixfrac the device tests use, on the small source
    for cid, name, (w, h), _, S, p, _ in ref.gpu_cases():
        if name in ref.TRANSFORMS and (w, h) != (150, 20):
            cases.append(("gpu-" + cid, 23, 17, ref.TRANSFORMS[name](23, 17), S, p))
    for cid, name, _, _, S, p, _ in sq.turn_cases():
        cases.append(("gpu-" + cid, 23, 17, ref.rotation(23, 17, float(name[3:]), 0.99, -0.2, 0.45), S, p))
    for name, make, S, p in (ref.R3, ref.R1):
        cases.append(("23x17-%s" % name, 23, 17, make(23, 17), S, p))
    cases += [("7x7-diamond", 7, 7, DIAMOND, 1.0, 1.0), ("7x7-mirrored", 7, 7, MIRRORED, 1.0, 1.0)]
    return cases


WINDOW_CASES = _window_cases()


@pytest.mark.parametrize("case", WINDOW_CASES, ids=[c[0] for c in WINDOW_CASES])
def test_the_window_holds_every_contribution(case):
    _, w, h, trans, S, p = case
    ow, oh = int(round(S * w)), int(round(S * h))
    src = ref.source(w, h, 11)
    win, brute = {}, {}
    s, t = sq.accumulate_square(src, trans, S, p, ow, oh, weight=1.25, contributions=win)
    sb, tb = sq.accumulate_square_brute(src, trans, S, p, ow, oh, weight=1.25, contributions=brute)
    assert win.keys() == brute.keys() and all(win[k] == brute[k] for k in win)
    assert ref.same(s, sb) and ref.same(t, tb)


def test_the_radii_of_the_cases_are_1_to_3():
    assert {sq.geometry_square(c[3], c[4], c[5])[4] for c in WINDOW_CASES} == {1, 2, 3}
    assert {sq.geometry_square(trans, S, p)[4] for _, _, _, _, S, p, trans in sq.gpu_cases()} == {1, 2, 3}


def test_a_rotated_drop_reaches_further_than_turbos():
    name, make, S, p = sq.R4_SQUARE
    trans = make(67, 35)
    assert ref.geometry(trans, S, p)[3] == 3
    with pytest.raises(ref.GeometryError, match="radius 4"):
        sq.geometry_square(trans, S, p)
    name, make, S, p = ref.R3
    assert sq.geometry_square(make(67, 35), S, p)[4] == 3
    # (R is a bound, not the least radius: a window of 0 loses contributions)
    src = ref.source(23, 17, 12, holes=False)
    full, short = {}, {}
    sq.accumulate_square(src, make(23, 17), S, p, 23, 17, contributions=full)
    sq.accumulate_square(src, make(23, 17), S, p, 23, 17, radius=0, contributions=short)
    assert len(short) < len(full) and short.items() <= full.items()


def test_the_radius_4_case_of_the_turbo_drizzle_raises_here_too():
    name, make, S, p = ref.R4
    with pytest.raises(ref.GeometryError, match="radius"):
        sq.geometry_square(make(67, 35), S, p)


def test_the_cfa_form_is_the_mono_form_of_the_masked_copy():
    import cfadrizzle_ref as cref
    src = ref.source(7, 5, 13)
    trans = ref.TRANSFORMS["rot30"](7, 5)
    for ch, cfa in cref.PAIRS:
        s, t = sq.accumulate_square_cfa(src, trans, 2.0, 0.7, 14, 10, ch, cfa, weight=1.5)
        sm, tm = sq.accumulate_square(cref.masked(src, ch, cfa), trans, 2.0, 0.7, 14, 10, weight=1.5)
        assert ref.same(s, sm) and ref.same(t, tm) and np.any(t > 0)
