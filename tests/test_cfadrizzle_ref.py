"""Pins cfadrizzle_ref.py, the restatement of include/nlstack_cfadrizzle.h, by hand: channel membership, planes that are
known without it, the order of the sums, the transform of the mosaic -- and the strided walk of the kernel
(drizzle_cfa.hip): for every transform the device test uses, a numpy walk strided as the kernel strides takes the same
contributions, per output pixel in the same order, as the full window over the masked mosaic.  No device."""
import numpy as np
import pytest

import bayer_ref
import cfadrizzle_ref as cref
import drizzle_ref as ref

f32 = np.float32
IDENTITY = np.array([1, 0, 0, 0, 1, 0], f32)


# ---- membership --------------------------------------------------------------------------------------------------------

def _by_definition(w, h, channel, cfa):
    xo, yo = bayer_ref.offsets(cfa)
    jj, ii = np.mgrid[0:h, 0:w]
    dx, dy = ii - xo, jj - yo
    inside = (ii >= xo) & (jj >= yo)
    if channel == "R":
        return inside & (dx % 2 == 0) & (dy % 2 == 0)
    if channel == "B":
        return inside & (dx % 2 == 1) & (dy % 2 == 1)
    return inside & ((dx + dy) % 2 == 1)


@pytest.mark.parametrize("w, h", [(6, 4), (7, 5)])
def test_masks_are_the_definition_s_disjoint_and_cover_the_pattern(w, h):
    for cfa in cref.CFAS:
        xo, yo = bayer_ref.offsets(cfa)
        masks = {ch: cref.channel_mask(w, h, ch, cfa) for ch in cref.CHANNELS}
        for ch in cref.CHANNELS:
            assert np.array_equal(masks[ch], _by_definition(w, h, ch, cfa)), (ch, cfa)
            assert np.array_equal(cref.channel_mask(w, h, ch.lower(), cfa.lower()), masks[ch])
        total = masks["R"].astype(int) + masks["G"] + masks["B"]
        jj, ii = np.mgrid[0:h, 0:w]
        assert np.array_equal(total, ((ii >= xo) & (jj >= yo)).astype(int)), cfa
        pw, ph = w - xo, h - yo                                               # the pattern's own extent
        counts = {ch: int(masks[ch].sum()) for ch in cref.CHANNELS}
        assert counts["R"] == ((pw + 1) // 2) * ((ph + 1) // 2)
        assert counts["B"] == (pw // 2) * (ph // 2)
        assert counts["G"] == pw * ph - counts["R"] - counts["B"]


def test_mask_counts_pinned_by_hand():
    # 6x4: RGGB has 6 R, 12 G, 6 B; BGGR (offsets 1, 1) is a 5x3 pattern: 6 R, 7 G, 2 B
    assert [int(cref.channel_mask(6, 4, ch, "RGGB").sum()) for ch in "RGB"] == [6, 12, 6]
    assert [int(cref.channel_mask(6, 4, ch, "BGGR").sum()) for ch in "RGB"] == [6, 7, 2]
    # 7x5: RGGB 12 R, 17 G, 6 B; GRBG (offset 1, 0) is a 6x5 pattern: 9 R, 15 G, 6 B
    assert [int(cref.channel_mask(7, 5, ch, "RGGB").sum()) for ch in "RGB"] == [12, 17, 6]
    assert [int(cref.channel_mask(7, 5, ch, "GRBG").sum()) for ch in "RGB"] == [9, 15, 6]


# ---- hand checks -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfa", cref.CFAS)
def test_flat_colours_land_on_their_own_plane_only(cfa):
    w, h, weight = 7, 5, f32(0.625)
    mosaic = np.zeros((h, w), f32)
    for value, ch in ((1.0, "R"), (2.0, "G"), (3.0, "B")):
        mosaic[cref.channel_mask(w, h, ch, cfa)] = value
    for value, ch in ((1.0, "R"), (2.0, "G"), (3.0, "B")):
        s, t = cref.accumulate_cfa(mosaic, IDENTITY, 1.0, 1.0, w, h, ch, cfa, weight=weight)
        mask = cref.channel_mask(w, h, ch, cfa)
        assert np.all(t[mask] == weight) and np.all(t[~mask] == 0)
        out = ref.finalize(s, t, 0.0, -1.0)
        assert np.all(out[t > 0] == f32(value)) and np.all(out[~(t > 0)] == -1.0)


def test_two_frames_an_odd_shift_apart_fill_complementary_pixels_of_r():
    w, h = 8, 6
    a, b = ref.source(w, h, 1, holes=False), ref.source(w, h, 2, holes=False)
    shift = np.array([1, 0, 1, 0, 1, 0], f32)                                 # one column to the right
    s, t = cref.accumulate_cfa(a, IDENTITY, 1.0, 1.0, w, h, "R", "RGGB", first=True)
    first = t > 0
    s, t = cref.accumulate_cfa(b, shift, 1.0, 1.0, w, h, "R", "RGGB", sum_plane=s, wgt_plane=t, first=False)
    second = (t > 0) & ~first
    assert np.array_equal(first, cref.channel_mask(w, h, "R", "RGGB"))
    want = np.zeros((h, w), bool)
    want[0::2, 1::2] = True                                                   # R columns 0, 2, .. moved to 1, 3, ..
    assert np.array_equal(second, want) and np.all(t[first | second] == 1) and not np.any(first & second)
    assert np.array_equal(s[second], b[0::2, 0::2][:, :w // 2].reshape(-1))


def test_contributions_of_one_channel_are_summed_in_candidate_order():
    # source pixel (i, j) -> reference (i / 3, j / 3): output pixel (1, 1) collects the drops of columns and rows 2, 3, 4,
    # of which (2, 2), (4, 2), (2, 4), (4, 4) are R; the values make the sum depend on the order (big + small - big)
    t3 = np.array([1.0 / 3.0, 0, 0, 0, 1.0 / 3.0, 0], f32)
    assert ref.geometry(t3, 1.0, 1.0)[3] == 3
    areas = {}
    cref.accumulate_cfa(np.ones((8, 8), f32), t3, 1.0, 1.0, 2, 2, "R", "RGGB", contributions=areas)
    mine = sorted((j, i) for (j, i, r, c) in areas if (r, c) == (1, 1))       # rows outer, columns inner
    assert mine == [(2, 2), (2, 4), (4, 2), (4, 4)]
    wa = [areas[(j, i, 1, 1)] for j, i in mine]
    src = np.full((8, 8), 12345.0, f32)                                       # the other channels: never taken
    values = [f32(1e8) / wa[0], f32(1.0) / wa[1], f32(-1e8) / wa[2], f32(0.0)]
    for (j, i), v in zip(mine, values):
        src[j, i] = v
    s, _ = cref.accumulate_cfa(src, t3, 1.0, 1.0, 2, 2, "R", "RGGB")
    in_order = f32(0)
    for v, a in zip(values, wa):
        in_order = f32(in_order + f32(v * a))
    other = f32(f32(f32(values[0] * wa[0]) + f32(values[2] * wa[2])) + f32(values[1] * wa[1]))
    assert s[1, 1] == in_order and in_order != other
    ss, _ = cref.accumulate_strided(src, t3, 1.0, 1.0, 2, 2, "R", "RGGB")
    assert ss[1, 1] == in_order


def test_reject_against_cfa_touches_the_channel_only():
    w, h = 6, 4
    v = np.arange(w * h, dtype=f32).reshape(h, w)
    m = v.copy()
    m[0, 0] -= 5          # R, high
    m[0, 1] -= 5          # G: another channel, kept
    m[2, 2] += 5          # R, low
    m[2, 4] = np.nan      # R against NaN: kept
    out, lo, hi = cref.reject_against_cfa(v, m, "R", "RGGB", 1.0, 1.0)
    assert (lo, hi) == (1, 1)
    gone = np.zeros((h, w), bool)
    gone[0, 0] = gone[2, 2] = True
    assert np.all(np.isnan(out[gone])) and np.array_equal(out[~gone].view(np.uint32), v[~gone].view(np.uint32))


# ---- the strided walk --------------------------------------------------------------------------------------------------

def _walk_cases():
    """every transform the device test uses (with its scale and pixfrac) on a small odd and a small even mosaic, the 12
    pairs in rotation; `half-out` and the frame's edges make the window start negative"""
    seen, out = set(), []
    for k, (case, ch, cfa) in enumerate(cref.rotation_cases() + cref.pair_cases()):
        _, name, _, _, S, p, _ = case
        if name in ref.TRANSFORMS:
            make = ref.TRANSFORMS[name]
        else:
            make = {ref.R3[0]: ref.R3[1], ref.R1[0]: ref.R1[1]}[name]
        if (name, S, p, ch, cfa) in seen:
            continue
        seen.add((name, S, p, ch, cfa))
        w, h = ((23, 17), (12, 10))[k % 2]
        out.append(("%dx%d-%s-S%g-p%g-%s-%s" % (w, h, name, S, p, ch, cfa), w, h, make(w, h), S, p, ch, cfa))
    return out


WALK_CASES = _walk_cases()


@pytest.mark.parametrize("case", WALK_CASES, ids=[c[0] for c in WALK_CASES])
def test_the_strided_walk_takes_the_masked_window_s_contributions_in_its_order(case):
    _, w, h, trans, S, p, ch, cfa = case
    ow, oh = int(round(S * w)), int(round(S * h))
    src = ref.source(w, h, 13)
    for kernel in (ref.TURBO, ref.POINT):
        full, walk = {}, {}
        s, t = cref.accumulate_cfa(src, trans, S, p, ow, oh, ch, cfa, weight=1.25, kernel=kernel, contributions=full)
        ss, ts = cref.accumulate_strided(src, trans, S, p, ow, oh, ch, cfa, weight=1.25, kernel=kernel, contributions=walk)
        assert full.keys() == walk.keys()
        a, b = cref.per_pixel(full), cref.per_pixel(walk)
        assert a.keys() == b.keys() and all(a[k] == b[k] for k in a)          # same keys and weights, same order
        assert ref.same(s, ss) and ref.same(t, ts)
        mask = cref.channel_mask(w, h, ch, cfa)
        assert all(mask[j, i] for j, i, _, _ in full)


def test_the_walk_cases_reach_every_radius_class_and_negative_window_starts():
    radii = {ref.geometry(c[3], c[4], c[5])[3] for c in WALK_CASES}
    assert radii == {1, 2, 3}
    assert {(c[6], c[7]) for c in WALK_CASES} == set(cref.PAIRS)
    _, w, h, trans, S, p, ch, cfa = next(c for c in WALK_CASES if "half-out" in c[0])
    F, G, hw, R = ref.geometry(trans, S, p)
    _, _, xc, _ = ref._centres(G, int(round(S * w)), 0, int(round(S * h)))
    assert np.nanmin(xc) - R < 0


# ---- the transform -----------------------------------------------------------------------------------------------------

def test_cfa_transform_is_the_composition_of_the_affine_maps():
    rng = np.random.default_rng(3)
    for cfa in cref.CFAS:
        xo, yo = bayer_ref.offsets(cfa)
        for trans in (ref.rotation(67, 35, 30.0, 1.01, 0.3, -0.4), ref.TRANSFORMS["shift"](1, 1), ref.TRANSFORMS["flip"](67, 35)):
            raw = cref.cfa_transform_double(trans, cfa)
            a, b, c, d, e, f = [float(v) for v in trans]
            for i, j in rng.integers(-5, 80, (20, 2)):
                x, y = float(i - xo), float(j - yo)                           # the plane's pixel of mosaic pixel (i, j)
                want = (a * x + b * y + c, d * x + e * y + f)
                got = (raw[0] * i + raw[1] * j + raw[2], raw[3] * i + raw[4] * j + raw[5])
                assert np.allclose(got, want, rtol=0, atol=1e-9)
            assert np.array_equal(cref.cfa_transform(trans, cfa), raw.astype(f32))


@pytest.mark.parametrize("cfa", cref.CFAS)
def test_a_star_lands_where_the_debayered_frame_had_it(cfa):
    # a star at plane pixel (x, y) is at mosaic pixel (x + xo, y + yo); the plane's transform moves plane (x, y) to
    # reference (x + 3, y + 2), so the mosaic's transform must move the mosaic pixel there too
    xo, yo = bayer_ref.offsets(cfa)
    w, h = 12, 10
    plane_trans = np.array([1, 0, 3, 0, 1, 2], f32)
    x, y = 4, 4                                                               # even: an R pixel of the pattern
    mosaic = np.zeros((h, w), f32)
    mosaic[y + yo, x + xo] = 7.0
    assert cref.channel_mask(w, h, "R", cfa)[y + yo, x + xo]
    s, t = cref.accumulate_cfa(mosaic, cref.cfa_transform(plane_trans, cfa), 1.0, 1.0, 20, 16, "R", cfa)
    assert s[y + 2, x + 3] == 7.0 and t[y + 2, x + 3] == 1.0 and np.count_nonzero(s) == 1
