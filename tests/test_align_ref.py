"""tests/align_ref.py against itself and against hand-traced values: on every case of tests/align_cases.py the
reference's kd-trees and the brute-force search with the documented tie rules agree in every bit, which is what lets
the device search by brute force; and the corners of the restated functions."""
import numpy as np
import pytest

import align_cases
import align_ref
from align_ref import F


def bits(a):
    return np.asarray(a, F).view(np.uint32)


@pytest.mark.parametrize("name", list(align_cases.CASES))
def test_kdtree_and_brute_force_agree_in_every_bit_and_no_case_has_a_tie(name):
    kd, brute = align_cases.reference(name), align_cases.reference(name, "brute")
    assert align_ref.compare(kd, brute) == []
    assert brute["ties"] == 0                                  # a condition of the case, not a tolerance
    assert len(kd["dist"]) == min(align_cases.CASES[name][0], len(kd["tri_dist"])) > 0
    assert np.all(np.diff(kd["dist"]) > 0)                     # every shortlist position is decided by the distances


def test_no_case_is_left_out():
    """the cases the device is compared on are these, all of them (tests/test_gpu_align.py takes the same table)"""
    assert len(align_cases.CASES) == 14
    shapes = {name: (len(align_cases.aligner(name).tri_dist), len(align_cases.reference(name)["tri_dist"]))
              for name in ("k3-three-stars", "k15-455-triangles", "k16-560-triangles", "k50-300-stars")}
    assert shapes == {"k3-three-stars": (1, 1), "k15-455-triangles": (455, 455), "k16-560-triangles": (560, 560),
                      "k50-300-stars": (19600, 19600)}
    assert len(align_cases.reference("k50-60-stars")["picked"]) < 50 < len(align_cases.frames("k50-60-stars")[2])
    assert len(align_cases.frames("fewer-stars-than-k")[2]) < align_cases.CASES["fewer-stars-than-k"][0]
    assert align_cases.reference("binned-frame")["scale_factor"] == 2.0


@pytest.mark.parametrize("name", ["k8-12-stars", "k16-560-triangles", "65-ref-stars"])
def test_the_stepped_search_is_the_recursive_one(name):
    a, ref = align_cases.aligner(name), align_cases.reference(name)
    for tree, queries in ((a.ref_tri_3dt, ref["tri_dist"]),
                          (a.stars_2dt, np.stack(align_cases.frames(name)[2:4], axis=1))):
        got, want = tree.nearest_neighbor(queries), tree.nearest_neighbor_recursive(queries)
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[2]), bits(want[2]))
        assert np.array_equal(bits(got[1]), bits(want[1]))


def test_kdtree_layout_of_seven_points():
    """kdtree2.go:31-59 by hand: Make sorts by x and keeps the median as the root, makeY sorts either side by y"""
    pts = [(2, 3), (5, 4), (9, 6), (4, 7), (8, 1), (7, 2), (1, 9)]
    tree = align_ref.KDTree(pts)
    # by x: (1,9) (2,3) (4,7) | (5,4) | (7,2) (8,1) (9,6); left by y: (2,3) | (4,7) | (1,9); right by y: (8,1) | (7,2) | (9,6)
    assert tree.pts.tolist() == [[2, 3], [4, 7], [1, 9], [5, 4], [8, 1], [7, 2], [9, 6]]
    assert tree.payload.tolist() == [0, 3, 6, 1, 4, 5, 2]
    index, point, dsq = tree.nearest_neighbor([(9, 2), (0, 0), (5, 4)])
    assert index.tolist() == [4, 0, 1] and dsq.tolist() == [2.0, 13.0, 0.0] and point.tolist() == [[8, 1], [2, 3], [5, 4]]


# four stars with integer coordinates and the light frame shifted by (1, 2): every number below was traced by hand
# from align.go.  Sides: 01 = 10, 02 = 25, 03 = 40, 12 = sqrt(325), 13 = sqrt(1060), 23 = sqrt(1665).
HAND_X, HAND_Y = np.array([0, 6, 24, 0], F), np.array([0, 8, 7, 40], F)


def test_hand_traced_case_of_four_stars():
    a = align_ref.RefAligner(100, 100, HAND_X, HAND_Y, 4)       # minLength = 5: nothing is skipped
    r325, r1060, r1665 = [F(np.sqrt(np.float64(v))) for v in (325, 1060, 1665)]
    assert a.picked.tolist() == [0, 1, 2, 3]
    # per unordered triple the one order with dAB < dAC < dBC: B joins the shortest and the longest side
    assert a.tri_abc.tolist() == [[0, 2, 3], [1, 0, 2], [1, 0, 3], [1, 2, 3]]
    assert np.array_equal(bits(a.tri_dist), bits([[25, 40, r1665], [10, r325, 25], [10, r1060, 40], [r325, r1060, r1665]]))
    for path in ("kdtree", "brute"):
        out = a.align(100, HAND_X + F(1), HAND_Y + F(2), path)
        assert out["scale_factor"] == 1.0 and out["tri_abc"].tolist() == a.tri_abc.tolist()
        assert np.array_equal(bits(out["tri_dist"]), bits(a.tri_dist))       # a shift of integers is exact
        assert out["match_dist"].tolist() == [0, 0, 0, 0] and out["match_ref"].tolist() == [0, 1, 2, 3]
        assert out["tri_index"].tolist() == [0, 1, 2, 3]                      # equal distances: (dist, tri index)
        assert out["abc"].tolist() == a.tri_abc.tolist() == out["ref_abc"].tolist()
        # candidate 0, p1 p2 p3 = (1,2) (25,9) (1,42) -> (0,0) (24,7) (0,40): den = 7*0 - 24*40 = -960,
        # a = (0*7 - 24*40) / -960 = 1, b = (24 - 1*24) / 7 = 0, c = 0 - 1 - 0 = -1, d = (40*7 - 7*40) / -960 = -0,
        # e = (7 - -0*24) / 7 = 1, f = 0 - -0*1 - 1*2 = -2
        assert out["trans"].tolist() == [[1, 0, -1, 0, 1, -2]] * 4
        assert out["trans_ok"].tolist() == [1] * 4 and out["num_matches"].tolist() == [4] * 4
        assert out["enough"].tolist() == [1] * 4 and out["ref_index"].tolist() == [[0, 1, 2, 3]] * 4
        assert out["ties"] == 3                                                # four equal distances: three pairs


def test_pick_skips_a_star_closer_than_min_length():
    x, y = np.array([10, 13, 13, 50, 10], F), np.array([10, 14, 13.9, 10, 14.9], F)
    # minLength 5: star 1 is exactly 5 away (kept: dAB < minLength is strict), star 2 closer, star 4 within 5 of star 1
    assert align_ref.pick_brightest_distant(x, y, F(5), 4).tolist() == [0, 1, 3]
    assert align_ref.pick_brightest_distant(x, y, F(5), 2).tolist() == [0, 1]
    assert align_ref.pick_brightest_distant(x, y, F(0), 9).tolist() == [0, 1, 2, 3, 4]
    assert align_ref.RefAligner(100, 100, x, y, 4).min_length == 5.0          # float32(naxisn[1]) * (1/20)


def test_transform_with_a_level_first_side_is_divide_by_zero():
    """p2.Y == p1.Y: b and e divide by zero.  a = float32(13 / 11) times 11 is not 13, the numerator of b is what the
    rounding left, and b is Inf, which NewTransform2D rejects"""
    assert F(13) - (F(-91) / F(-77)) * F(11) != 0
    trans, ok = align_ref.new_transform_2d((0, 0), (11, 0), (3, 7), (0, 0), (13, 0), (3, 7))
    assert not ok and trans.tolist() == [0] * 6


def test_zero_over_zero_gives_a_nan_transform_that_passes_and_matches_nothing():
    """the same triangle on both sides: the numerators are 0 too, 0 / 0 = NaN, and IsInf lets NaN through"""
    trans, ok = align_ref.new_transform_2d((0, 0), (10, 0), (3, 7), (0, 0), (10, 0), (3, 7))
    assert ok and trans[0] == 1 and np.isnan(trans[1]) and np.isnan(trans[2]) and np.isnan(trans[4])
    a = align_ref.RefAligner(100, 100, HAND_X, HAND_Y, 4)
    for path in ("kdtree", "brute"):
        ref_index, counts, _ = a.match_stars([trans, [1, 0, 0, 0, 1, 0]], HAND_X, HAND_Y, path)
        assert ref_index.tolist() == [[-1] * 4, [0, 1, 2, 3]] and counts.tolist() == [0, 4]


def test_the_eight_pixel_boundary_is_strict():
    ref_x, ref_y, x, y, want = align_cases.lattice_case()
    assert F(49) + align_cases.ROOT_14 * align_cases.ROOT_14 == 63.0
    a = align_ref.RefAligner(align_cases.WIDTH, align_cases.HEIGHT, ref_x, ref_y, 8)
    for path in ("kdtree", "brute"):
        ref_index, counts, ties = a.match_stars([1, 0, 0, 0, 1, 0], x, y, path)
        assert ref_index[0].tolist() == want.tolist() and counts.tolist() == [int((want >= 0).sum())] and ties == 0
    _, dsq, _ = align_ref.brute_nearest(np.stack([ref_x, ref_y], axis=1), np.stack([x, y], axis=1))
    assert dsq[[1, 3]].tolist() == [64.0, 63.0] and want[[1, 3]].tolist() == [-1, 0]


def test_brute_force_holds_the_tie_rules():
    """two reference stars at one distance from a projected star: the lowest index; a frame identical to the
    reference: every dist is 0 and the shortlist is in triangle order"""
    a = align_ref.RefAligner(100, 100, np.array([30, 20, 50], F), np.array([10, 10, 40], F), 3)
    ref_index, _, ties = a.match_stars([1, 0, 0, 0, 1, 0], np.array([25], F), np.array([10], F), "brute")
    assert ref_index.tolist() == [[0]] and ties == 1
    ref_x, ref_y = align_cases.frames("k8-12-stars")[:2]
    out = align_cases.aligner("k8-12-stars").align(align_cases.WIDTH, ref_x, ref_y, "brute")
    assert not out["dist"].any() and out["tri_index"].tolist() == list(range(8)) and out["ties"] >= 8
