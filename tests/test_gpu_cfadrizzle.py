"""GPU parity of the CFA drizzle (include/nlstack_cfadrizzle.h, an extension: the header is the contract) against its
restatement cfadrizzle_ref.py -- the mono restatement drizzle_ref.py on a copy of the mosaic whose other pixels are NaN
-- which test_cfadrizzle_ref.py pins by hand: bit equality throughout, any NaN equal to any NaN.

The kernel (drizzle_cfa.hip) walks only the channel's positions of each window; the tile shape, the staging and
developer switch 32768 are the mono kernel's, so every case runs on both tile paths and nl_stack_drizzle_tile_paths
answers for it.  The planes lie in a buffer of random bits, padding included (test_gpu_drizzle.py's Planes): after
every call only the planes the call names have changed.  The resident bad-pixel step is held against
bayer_ref.correct as test_gpu_bayer.py holds the upload's."""
import numpy as np
import pytest

import bayer_ref
import cfadrizzle_ref as cref
import drizzle_ref as ref
from test_gpu_bayer import mosaic
from test_gpu_drizzle import DIRECT, WEIGHTS, Planes, dithered

pytestmark = pytest.mark.gpu

f32 = np.float32
CASES = cref.rotation_cases() + cref.pair_cases()


def restated(case, channel, cfa, kernel, row0=0, rows=None):
    """the (sum, wgt) planes after each of the three frames of a case"""
    _, _, (w, h), (ow, oh), S, p, trans = case
    out, s, t = [], None, None
    for k in range(3):
        s, t = cref.accumulate_cfa(ref.source(w, h, 20 + k), dithered(trans, k), S, p, ow, oh, channel, cfa, sum_plane=s,
                                   wgt_plane=t, weight=WEIGHTS[k], first=k == 0, kernel=kernel, row0=row0, rows=rows)
        out.append((s, t))
    return out


@pytest.mark.parametrize("entry", CASES, ids=[cref.case_id(e) for e in CASES])
def test_cfa_drizzle_matches_the_restatement_on_both_paths(nl, entry):
    case, channel, cfa = entry
    cid, name, (w, h), (ow, oh), S, p, trans = case
    tiles = -(-ow // 256) * -(-oh // 16)
    SUM, WGT = 2, 0
    with nl.StackHandle(3, w, h) as src:
        for k in range(3):
            src.upload_tile(k, ref.source(w, h, 20 + k))
        for kernel in (nl.DZ_TURBO, nl.DZ_POINT):
            want = restated(case, channel, cfa, kernel)
            assert name == "all-out" or any(np.any(t > 0) for _, t in want)
            for flags in (0, DIRECT):
                with Planes(nl, ow, oh) as dst:
                    dst.st.set_dev_flags(flags)
                    for k in range(3):
                        t_k = dithered(trans, k)
                        staged, direct = dst.st.drizzle_tile_paths(src, k, t_k, S, p)
                        assert staged + direct == tiles and (staged == 0 or not flags)
                        if not flags:
                            assert name not in ("identity", "shift", "flip") or direct == 0
                        dst.st.frame_drizzle_cfa_from(SUM, WGT, src, k, t_k, S, channel, cfa, pixfrac=p,
                                                      weight=WEIGHTS[k], first=k == 0, kernel=kernel)
                        got = dst.read((SUM, WGT))
                        assert ref.same(got[SUM], want[k][0]), (kernel, flags, k, "sum")
                        assert ref.same(got[WGT], want[k][1]), (kernel, flags, k, "wgt")
        for k in range(3):                                                    # the source is only read
            assert ref.same(src.download_tile(k), ref.source(w, h, 20 + k))


@pytest.mark.parametrize("name, channel, cfa", [("rot30", "G", "GRBG"), ("half-out", "B", "GBRG")])
def test_a_row_tile_makes_its_own_rows_of_the_whole_image(nl, name, channel, cfa):
    (w, h), (ow, oh), S = ref.SHAPES[3]
    case = (name, name, (w, h), (ow, oh), S, 0.7, ref.TRANSFORMS[name](w, h))
    whole = restated(case, channel, cfa, ref.TURBO)
    with nl.StackHandle(3, w, h) as src:
        for k in range(3):
            src.upload_tile(k, ref.source(w, h, 20 + k))
        for row0, rows in ((0, 13), (13, 27)):
            for flags in (0, DIRECT):
                with Planes(nl, ow, oh, row0=row0, rows=rows) as dst:
                    dst.st.set_dev_flags(flags)
                    for k in range(3):
                        staged, direct = dst.st.drizzle_tile_paths(src, k, dithered(case[6], k), S, 0.7)
                        assert staged + direct == 2 * -(-rows // 16)
                        dst.st.frame_drizzle_cfa_from(1, 3, src, k, dithered(case[6], k), S, channel, cfa, pixfrac=0.7,
                                                      weight=WEIGHTS[k], first=k == 0)
                        got = dst.read((1, 3))
                        for plane, slot in ((0, 1), (1, 3)):
                            assert ref.same(got[slot], whole[k][plane][row0:row0 + rows])


CROSS = [(ref.R1, (201, 105), "R", "BGGR"), (("shift-S2-p0.7", ref.TRANSFORMS["shift"], 2.0, 0.7), (134, 70), "G", "RGGB"),
         (("rot30-S2-p1", ref.TRANSFORMS["rot30"], 2.0, 1.0), (134, 70), "B", "GRBG"), (ref.R3, (67, 35), "G", "GBRG")]


@pytest.mark.parametrize("spec, out_shape, channel, cfa", CROSS, ids=[c[0][0] for c in CROSS])
def test_the_cfa_entry_equals_the_mono_entry_on_a_host_masked_copy(nl, spec, out_shape, channel, cfa):
    _, make, S, p = spec
    (w, h), (ow, oh) = (67, 35), out_shape
    trans = make(w, h)
    with nl.StackHandle(2, w, h) as src, nl.StackHandle(4, ow, oh) as dst:
        raw = ref.source(w, h, 31)
        src.upload_tile(0, raw)
        src.upload_tile(1, cref.masked(raw, channel, cfa))
        for kernel in (nl.DZ_TURBO, nl.DZ_POINT):
            dst.frame_drizzle_cfa_from(0, 1, src, 0, trans, S, channel, cfa, pixfrac=p, weight=1.5, first=True, kernel=kernel)
            dst.frame_drizzle_from(2, 3, src, 1, trans, S, p, weight=1.5, first=True, kernel=kernel)
            assert np.any(dst.download_tile(1) > 0)
            assert ref.same(dst.download_tile(0), dst.download_tile(2)) and ref.same(dst.download_tile(1), dst.download_tile(3))


def test_the_cross_check_reaches_every_radius():
    assert {ref.geometry(c[0][1](67, 35), c[0][2], c[0][3])[3] for c in CROSS} == {1, 2, 3}


def test_reject_against_cfa_counts_survivors_and_other_channels(nl):
    w, h = 53, 19
    rng = np.random.default_rng(6)
    m = rng.standard_normal((h, w)).astype(f32)
    v = (m + 0.4 * rng.standard_normal((h, w))).astype(f32)
    fv, fm = v.reshape(-1), m.reshape(-1)
    fv[::9] = np.nan
    fm[4::9] = np.nan
    fv[1::31] = np.inf
    fv[2::37] = -np.inf
    fm[3::41] = np.inf
    fv[5::43] = -0.0
    fv[7::9] = fm[7::9] + f32(0.5)                                            # on the threshold or a rounding beside it
    for k, (low, high) in enumerate(((0.5, 0.5), (0.0, 1.0), (0.25, 0.0), (np.inf, np.inf))):
        for channel, cfa in (cref.PAIRS[3 * k], cref.PAIRS[3 * k + 1], cref.PAIRS[3 * k + 2]):
            want, n_low, n_high = cref.reject_against_cfa(v, m, channel, cfa, low, high)
            mask = cref.channel_mask(w, h, channel, cfa).reshape(-1)
            with Planes(nl, w, h) as p:
                p.put(0, v)
                p.put(2, m)
                assert p.st.frame_reject_against_cfa(0, 2, channel, cfa, low, high) == (n_low, n_high)
                got = p.read((0,))[0]
                gone = np.isnan(want.reshape(-1)) & ~np.isnan(fv)
                assert int(gone.sum()) == n_low + n_high and (n_low > 0 and n_high > 0 or low == np.inf)
                assert not np.any(gone & ~mask)
                assert ref.same(got, want) and np.array_equal(got.view(np.uint32)[~gone], fv.view(np.uint32)[~gone])
    with Planes(nl, w, h) as p:                                               # a frame against itself: nothing goes
        p.put(1, v)
        assert p.st.frame_reject_against_cfa(1, 1, "G", "RGGB", 0.0, 0.0) == (0, 0)
        assert np.array_equal(p.read(())[1].view(np.uint32), fv.view(np.uint32))


def test_reject_against_cfa_on_a_row_tile_takes_the_image_s_rows(nl):
    w, h, row0, rows = 21, 16, 5, 7
    rng = np.random.default_rng(7)
    m = rng.standard_normal((h, w)).astype(f32)
    v = (m + rng.standard_normal((h, w))).astype(f32)
    want, _, _ = cref.reject_against_cfa(v, m, "B", "GBRG", 0.5, 0.5)
    part = want[row0:row0 + rows]
    gone = np.isnan(part) & ~np.isnan(v[row0:row0 + rows])
    with Planes(nl, w, h, row0=row0, rows=rows) as p:
        p.put(0, v[row0:row0 + rows])
        p.put(1, m[row0:row0 + rows])
        n_low, n_high = p.st.frame_reject_against_cfa(0, 1, "B", "GBRG", 0.5, 0.5)
        assert n_low + n_high == int(gone.sum()) > 0
        assert ref.same(p.read((0,))[0], part)


@pytest.mark.parametrize("w, h, cfa", [(16, 12, "RGGB"), (16, 12, "BGGR"), (67, 35, "RGGB"), (67, 35, "BGGR"), (67, 35, "GRBG")])
def test_badpixel_cfa_is_the_reference_s_correction_in_place(nl, oracle, w, h, cfa):
    raw = mosaic(w, h, seed=w + len(cfa) + ord(cfa[0]))
    raw[(h // 2) * w + w // 2] += f32(40000.0)
    raw[(h // 2 + 1) * w + w // 2 - 3] += f32(40000.0)
    raw[(h // 2 - 2) * w + w // 2 + 2] += f32(40000.0)
    with Planes(nl, w, h, n=3) as p:
        p.put(1, raw)
        # the zero-sigma no-op: nothing runs
        for sl, sh in ((0.0, 5.0), (3.0, 0.0)):
            removed, stats = p.st.frame_badpixel_cfa(1, "R", cfa, sl, sh)
            assert removed == 0 and np.isnan(stats[0]) and np.isnan(stats[1])
            assert np.array_equal(p.read(())[1].view(np.uint32), raw.view(np.uint32))
        # the three channels in sequence on one slot; the neighbouring slots and the padding keep their bits
        want, total = raw, 0
        for channel in ("R", "G", "B"):
            want, removed, (mean, std) = bayer_ref.correct(oracle, want, w, channel, cfa, 3.0, 5.0)
            got_removed, got_stats = p.st.frame_badpixel_cfa(1, channel, cfa, 3.0, 5.0)
            assert got_removed == removed, (channel, got_removed, removed)
            assert ref.same(got_stats, [mean, std]), (channel, got_stats, (mean, std))
            assert ref.same(p.read((1,))[1], want), channel
            total += removed
        assert total > 0
        # a negative sigma is the reference's
        want, removed, (mean, std) = bayer_ref.correct(oracle, want, w, "G", cfa, -0.5, 5.0)
        got_removed, got_stats = p.st.frame_badpixel_cfa(1, "g", cfa.lower(), -0.5, 5.0)
        assert got_removed == removed and ref.same(got_stats, [mean, std]) and ref.same(p.read((1,))[1], want)


def test_upload_badpixel_drizzle_finalize_end_to_end(nl, oracle):
    w, h, S, p, cfa = 67, 35, 2.0, 0.7, "GRBG"
    ow, oh = 134, 70
    hot = ((10, 20), (11, 31), (20, 12))                                      # (row, column) of each frame's hot pixel
    frames = []
    for k, (r, c) in enumerate(hot):
        f = mosaic(w, h, seed=300 + k)
        f[r * w + c] += f32(50000.0)
        frames.append(f)
    # alignment is estimated on the debayered planes: their dithered shifts, moved to the mosaic's grid
    plane_trans = [np.array([1, 0, dx, 0, 1, dy], f32) for dx, dy in ((0.0, 0.0), (1.25, -0.5), (-0.5, 1.75))]
    raw_trans = [nl.drizzle_cfa_transform(t, cfa) for t in plane_trans]
    for t, pt in zip(raw_trans, plane_trans):
        assert np.array_equal(t, cref.cfa_transform(pt, cfa))

    # the restatement of the chain
    clean, removed_want = [], []
    for f in frames:
        counts = []
        for channel in ("R", "G", "B"):
            f, removed, _ = bayer_ref.correct(oracle, f, w, channel, cfa, 3.0, 5.0)
            counts.append(removed)
        clean.append(f.reshape(h, w))
        removed_want.append(counts)
    assert all(sum(c) > 0 for c in removed_want)
    for k, (r, c) in enumerate(hot):
        assert clean[k][r, c] < 10000.0                                       # the hot pixel is gone
    want = {}
    for channel in ("R", "G", "B"):
        s = t = None
        for k in range(3):
            s, t = cref.accumulate_cfa(clean[k], raw_trans[k], S, p, ow, oh, channel, cfa, sum_plane=s, wgt_plane=t,
                                       first=k == 0)
        want[channel] = (s, t, ref.finalize(s, t, 0.0, np.nan))

    with nl.StackHandle(3, w, h) as raw, nl.StackHandle(9, ow, oh) as dz:
        for k in range(3):
            raw.upload_tile(k, frames[k])
            got = [raw.frame_badpixel_cfa(k, channel, cfa, 3.0, 5.0)[0] for channel in ("R", "G", "B")]
            assert got == removed_want[k]
            assert ref.same(raw.download_tile(k), clean[k])
        for n, channel in enumerate(("R", "G", "B")):
            SUM, WGT, OUT = 3 * n, 3 * n + 1, 3 * n + 2
            for k in range(3):
                dz.frame_drizzle_cfa_from(SUM, WGT, raw, k, raw_trans[k], S, channel, cfa, pixfrac=p, first=k == 0)
            dz.drizzle_finalize(SUM, WGT, OUT)
            s, t, out = want[channel]
            assert ref.same(dz.download_tile(SUM), s) and ref.same(dz.download_tile(WGT), t)
            got = dz.download_tile(OUT)
            assert ref.same(got, out)
            assert np.isfinite(got).any() and np.nanmax(got) < 10000.0        # no hot pixel reached the plane


def test_error_messages_that_need_a_device(nl):
    from nightlight_amd import capi
    w, h = 40, 24
    ident = [1, 0, 0, 0, 1, 0]
    before = ref.source(w, h, 9)
    with nl.StackHandle(2, w, h) as src, nl.StackHandle(3, 2 * w, 2 * h) as dst, \
            nl.StackHandle(2, w, h, row0=8, rows=8) as tile, nl.StackHandle(3, 2 * w, 2 * h) as lender:
        src.upload_tile(0, before)
        src.upload_tile(1, before)
        for k in range(3):
            dst.upload_tile(k, np.full(4 * w * h, k, f32))

        def refused(call, words):
            with pytest.raises(capi.NlError) as e:
                call()
            assert e.value.code == capi.ERR_INVALID_ARG and words in str(e.value), str(e.value)
            for k in range(3):
                assert np.all(dst.download_tile(k) == k)
            assert ref.same(src.download_tile(0), before) and ref.same(src.download_tile(1), before)

        def from_(sum_idx, wgt_idx, s, idx, trans=ident, scale=2.0, channel="R", cfa="RGGB"):
            return lambda: dst.frame_drizzle_cfa_from(sum_idx, wgt_idx, s, idx, trans, scale, channel, cfa)

        refused(from_(0, 1, tile, 0), "frame_drizzle_cfa_from (source) needs a whole-image handle")
        refused(from_(1, 1, src, 0), "frame_drizzle_cfa_from: slot 1 is both the sum and the weight plane")
        refused(from_(0, 1, src, 2), "frame_drizzle_cfa_from (source): bad index 2")
        refused(from_(3, 1, src, 0), "frame_drizzle_cfa_from (sum plane): bad index 3")
        refused(from_(0, -1, src, 0), "frame_drizzle_cfa_from (weight plane): bad index -1")
        refused(from_(0, 1, dst, 1), "source and destination")
        refused(from_(0, 1, src, 0, ref.R4[1](w, h), 1.0), "window radius 4")
        refused(from_(0, 1, src, 0, cfa="RGBG"), "Unknown CFA value RGBG")
        refused(from_(0, 1, src, 0, channel="L"), "Unknown debayering value L")
        refused(from_(0, 1, src, 0, channel=""), "frame_drizzle_cfa_from needs a channel and a CFA")
        refused(lambda: src.frame_reject_against_cfa(2, 0, "R", "RGGB", 1.0, 1.0), "frame_reject_against_cfa: bad index 2")
        refused(lambda: src.frame_reject_against_cfa(0, 5, "R", "RGGB", 1.0, 1.0), "frame_reject_against_cfa (model): bad index 5")
        refused(lambda: src.frame_reject_against_cfa(0, 1, "R", "XXXX", 1.0, 1.0), "Unknown CFA value XXXX")
        refused(lambda: src.frame_badpixel_cfa(2, "R", "RGGB"), "frame_badpixel_cfa: bad index 2")
        refused(lambda: src.frame_badpixel_cfa(0, "R", "XXXX"), "Unknown CFA value XXXX")
        refused(lambda: src.frame_badpixel_cfa(0, "Q", "RGGB"), "Unknown debayering value Q")
        refused(lambda: src.frame_badpixel_cfa(0, "", "RGGB"), "frame_badpixel_cfa needs a channel and a CFA")
        refused(lambda: tile.frame_badpixel_cfa(0, "R", "RGGB"), "frame_badpixel_cfa needs a whole-image handle")
        dst.attach_device_frames(lender.frames_device_ptr(), lender.frame_stride())
        try:
            with pytest.raises(capi.NlError) as e:
                dst.frame_drizzle_cfa_from(0, 1, src, 0, ident, 2.0, "R", "RGGB")
            assert e.value.code == capi.ERR_INVALID_ARG and "attached, not owned" in str(e.value)
        finally:
            dst.attach_device_frames(None)
        # two slots of one handle beside the source's: fine
        with nl.StackHandle(3, w, h) as one:
            one.upload_tile(2, before)
            one.frame_drizzle_cfa_from(0, 1, one, 2, ident, 1.0, "G", "BGGR", first=True)
            s, t = cref.accumulate_cfa(before, ident, 1.0, 1.0, w, h, "G", "BGGR")
            assert ref.same(one.download_tile(0), s) and ref.same(one.download_tile(1), t)
            assert ref.same(one.download_tile(2), before)
