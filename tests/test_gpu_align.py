"""The alignment entries on the device against tests/align_ref.py's kd-tree path, everything with array_equal: the
triangles in order, every triangle's nearest reference triangle, the candidates field by field with the bits of dist
and trans, ref_index and the counts.  The cases are those of tests/align_cases.py, which tests/test_align_ref.py
holds free of ties; the one tie case is compared with the brute-force path and its stated tie rules."""
import threading

import numpy as np
import pytest

import align_cases
import align_ref
from nightlight_amd import Aligner, NlError, capi

pytestmark = pytest.mark.gpu

IDENTITY = np.array([1, 0, 0, 0, 1, 0], np.float32)


def stars_of(x, y):
    s = np.zeros(len(x), capi.STAR_DTYPE)
    s["x"], s["y"] = x, y
    s["index"] = np.arange(len(x))
    return s


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_triangles_equal(tris, dist, abc, what):
    assert len(tris) == len(dist), what
    got = np.stack([tris["d_ab"], tris["d_ac"], tris["d_bc"]], axis=1).reshape(-1, 3)
    assert np.array_equal(bits(got), bits(dist)), what
    assert np.array_equal(np.stack([tris["a"], tris["b"], tris["c"]], axis=1).reshape(-1, 3), abc), what


def assert_match_equal(got, want):
    """(candidates, ref_index, info) of Aligner.match against a result of align_ref's align()"""
    cands, ref_index, info = got
    assert np.array_equal(info["picked"], want["picked"])
    assert info["n_picked"] == len(want["picked"]) and info["n_triangles"] == len(want["tri_dist"])
    assert bits(info["scale_factor"]) == bits(want["scale_factor"])
    assert_triangles_equal(info["triangles"], want["tri_dist"], want["tri_abc"], "the frame's triangles")
    assert np.array_equal(bits(info["tri_dist"]), bits(want["match_dist"]))
    assert np.array_equal(info["tri_ref"], want["match_ref"])
    assert len(cands) == len(want["dist"])
    assert np.array_equal(bits(cands["dist"]), bits(want["dist"]))
    for field, key in (("tri_index", "tri_index"), ("ref_tri_index", "ref_tri_index"), ("trans_ok", "trans_ok"),
                       ("num_matches", "num_matches"), ("enough", "enough")):
        assert np.array_equal(cands[field], want[key]), field
    assert np.array_equal(np.stack([cands["a"], cands["b"], cands["c"]], axis=1).reshape(-1, 3), want["abc"])
    assert np.array_equal(np.stack([cands["ref_a"], cands["ref_b"], cands["ref_c"]], axis=1).reshape(-1, 3),
                          want["ref_abc"])
    assert np.array_equal(bits(cands["trans"]), bits(want["trans"]))
    assert ref_index.shape == want["ref_index"].shape and np.array_equal(ref_index, want["ref_index"])


def device_aligner(name):
    ref_x, ref_y = align_cases.frames(name)[:2]
    return Aligner(align_cases.WIDTH, align_cases.HEIGHT, stars_of(ref_x, ref_y), k=align_cases.CASES[name][0])


@pytest.mark.parametrize("name", list(align_cases.CASES))
def test_match_is_the_reference_in_every_bit(name):
    _, _, x, y, frame_width = align_cases.frames(name)
    ref, want = align_cases.aligner(name), align_cases.reference(name)
    with device_aligner(name) as a:
        picked, tris = a.info()
        assert np.array_equal(picked, ref.picked)
        assert_triangles_equal(tris, ref.tri_dist, ref.tri_abc, "the reference's triangles")
        assert_match_equal(a.match(frame_width, stars_of(x, y), triangles=True), want)


def test_three_stars_give_one_candidate_and_two_give_none():
    name = "k3-three-stars"
    _, _, x, y, frame_width = align_cases.frames(name)
    with device_aligner(name) as a:
        cands, ref_index, info = a.match(frame_width, stars_of(x, y))
        assert len(cands) == 1 < a.k and info["n_triangles"] == 1 and ref_index.shape == (1, 3)
        # fewer than three stars: no triangle, no candidate, no error (the zero transform and MaxFloat32)
        cands, ref_index, info = a.match(frame_width, stars_of(x[:2], y[:2]))
        assert len(cands) == 0 and info["n_picked"] == 2 and info["n_triangles"] == 0 and ref_index.shape == (0, 2)


def test_a_reference_without_triangles():
    """one reference star: matching stars works, a frame without triangles gives no candidate, one with triangles is
    the reference's panic"""
    _, _, x, y, frame_width = align_cases.frames("k8-12-stars")
    ref = align_ref.RefAligner(align_cases.WIDTH, align_cases.HEIGHT, x[:1], y[:1], 8)
    with Aligner(align_cases.WIDTH, align_cases.HEIGHT, stars_of(x[:1], y[:1]), k=8) as a:
        picked, tris = a.info()
        assert picked.tolist() == [0] and len(tris) == 0
        got = a.match_stars(IDENTITY, stars_of(x, y))
        want = ref.match_stars(IDENTITY, x, y)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[1].tolist() == [1]
        assert len(a.match(frame_width, stars_of(x[:2], y[:2]))[0]) == 0
        with pytest.raises(NlError, match="56 triangles against a reference with none") as err:
            a.match(frame_width, stars_of(x, y))
        assert err.value.code == capi.ERR_INVALID_ARG


def test_the_eight_pixel_boundary_is_strict():
    ref_x, ref_y, x, y, want = align_cases.lattice_case()
    with Aligner(align_cases.WIDTH, align_cases.HEIGHT, stars_of(ref_x, ref_y), k=8) as a:
        ref_index, counts = a.match_stars(IDENTITY, stars_of(x, y))
        assert ref_index.tolist() == [want.tolist()]           # dsq exactly 64: unmatched; 63: matched
        assert counts.tolist() == [int((want >= 0).sum())]


@pytest.mark.parametrize("name", ["63-ref-stars", "64-ref-stars", "65-ref-stars", "1025-ref-stars"])
def test_match_stars_for_one_and_for_k_transforms_with_a_nan_among_them(name):
    _, _, x, y, _ = align_cases.frames(name)
    ref, want = align_cases.aligner(name), align_cases.reference(name)
    transforms = want["trans"].copy()
    transforms[1, 1] = np.nan                                  # a NaN transform matches nothing
    with device_aligner(name) as a:
        assert len(transforms) == a.k
        for t in (transforms[:1], transforms):
            got = a.match_stars(t, stars_of(x, y))
            expect = ref.match_stars(t, x, y)
            assert np.array_equal(got[0], expect[0]) and np.array_equal(got[1], expect[1])
        assert got[1][1] == 0 and (got[0][1] == -1).all() and got[1][0] == want["num_matches"][0] > 0
        assert np.array_equal(got[0][0], want["ref_index"][0])


def test_ties_follow_the_stated_rules():
    """two reference stars equidistant from a projected star: the lowest index; a frame identical to the reference:
    every dist is 0 and the shortlist is ordered by triangle index -- the brute-force path's rules"""
    ref_x, ref_y = np.array([30, 20, 50], np.float32), np.array([10, 10, 40], np.float32)
    with Aligner(100, 100, stars_of(ref_x, ref_y), k=3) as a:
        ref_index, counts = a.match_stars(IDENTITY, stars_of([25.0], [10.0]))
        assert ref_index.tolist() == [[0]] and counts.tolist() == [1]
    name = "k16-560-triangles"                                  # two chunks of reference triangles: ties across them too
    ref_x, ref_y = align_cases.frames(name)[:2]
    want = align_cases.aligner(name).align(align_cases.WIDTH, ref_x, ref_y, "brute")
    assert not want["dist"].any() and want["tri_index"].tolist() == list(range(16)) and want["ties"] > 0
    with device_aligner(name) as a:
        assert_match_equal(a.match(align_cases.WIDTH, stars_of(ref_x, ref_y), triangles=True), want)


def test_one_aligner_matched_from_four_threads_at_once():
    name = "k15-455-triangles"
    _, _, x, y, frame_width = align_cases.frames(name)
    frames = [stars_of(x + np.float32(0.25 * i), y - np.float32(0.5 * i)) for i in range(4)]
    with device_aligner(name) as a:
        serial = [a.match(frame_width, f, triangles=True) for f in frames]
        assert_match_equal(serial[0], align_cases.reference(name))
        rounds, got, errors = 3, {}, []
        barrier = threading.Barrier(len(frames))

        def work(i):
            try:
                for r in range(rounds):
                    barrier.wait()
                    got[i, r] = a.match(frame_width, frames[i], triangles=True)
            except Exception as e:                             # pragma: no cover - reported below
                errors.append(e)
                barrier.abort()

        threads = [threading.Thread(target=work, args=(i,)) for i in range(len(frames))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for (i, _), (cands, ref_index, info) in got.items():
            assert cands.tobytes() == serial[i][0].tobytes() and np.array_equal(ref_index, serial[i][1])
            assert info["triangles"].tobytes() == serial[i][2]["triangles"].tobytes()
            assert np.array_equal(bits(info["tri_dist"]), bits(serial[i][2]["tri_dist"]))
