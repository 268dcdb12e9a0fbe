"""GPU parity of the square drizzle (include/nlstack_sqdrizzle.h, an extension: the header is the contract) against its
numpy restatement sqdrizzle_ref.py, which test_sqdrizzle_ref.py pins by hand: bit equality throughout, any NaN equal to
any NaN.

The kernels (drizzle_square.hip) are the walks of the turbo drizzle with another weight per candidate, so the tests are
test_gpu_drizzle.py's and test_gpu_cfadrizzle.py's under the new entries: every case on both tile paths (developer switch
32768, nl_stack_drizzle_square_tile_paths says which tiles took which) and in both candidate forms (developer switch
262144: the edges of every candidate), the planes inside a buffer of random bits (test_gpu_drizzle.py's Planes), a
row-tile destination, the 12 channel x CFA pairs, the CFA entry against the mono entry on a host-masked copy, and one
chain from the stack to the finished image."""
import numpy as np
import pytest

import cfadrizzle_ref as cref
import drizzle_ref as ref
import sqdrizzle_ref as sq
from test_gpu_drizzle import DIRECT, WEIGHTS, Planes, dithered

pytestmark = pytest.mark.gpu

f32 = np.float32
EVERY = 262144
CASES = sq.gpu_cases()
CFA_CASES = cref.pair_cases()


def restated(case, row0=0, rows=None, pair=None):
    """the (sum, wgt) planes after each of the three frames of a case (of the channel and CFA in pair)"""
    _, _, (w, h), (ow, oh), S, p, trans = case
    out, s, t = [], None, None
    for k in range(3):
        src = ref.source(w, h, 20 + k)
        kw = dict(sum_plane=s, wgt_plane=t, weight=WEIGHTS[k], first=k == 0, row0=row0, rows=rows)
        if pair is None:
            s, t = sq.accumulate_square(src, dithered(trans, k), S, p, ow, oh, **kw)
        else:
            s, t = sq.accumulate_square_cfa(src, dithered(trans, k), S, p, ow, oh, pair[0], pair[1], **kw)
        out.append((s, t))
    return out


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_square_drizzle_matches_the_restatement_on_both_paths_in_both_forms(nl, case):
    cid, name, (w, h), (ow, oh), S, p, trans = case
    tiles = -(-ow // 256) * -(-oh // 16)
    SUM, WGT = 2, 0
    want = restated(case)
    assert name == "all-out" or any(np.any(t > 0) for _, t in want)
    with nl.StackHandle(3, w, h) as src:
        for k in range(3):
            src.upload_tile(k, ref.source(w, h, 20 + k))                      # NaN, +Inf and -Inf among them
        for flags in (0, DIRECT, EVERY, EVERY | DIRECT):
            with Planes(nl, ow, oh) as dst:
                dst.st.set_dev_flags(flags)
                for k in range(3):
                    t_k = dithered(trans, k)
                    staged, direct = dst.st.drizzle_square_tile_paths(src, k, t_k, S, p)
                    assert staged + direct == tiles and (staged == 0 or not flags & DIRECT)
                    if not flags & DIRECT:
                        assert name != "all-out" or staged == 0               # all out: no candidate, no box
                        assert name not in ("identity", "shift", "flip") or direct == 0
                    dst.st.frame_drizzle_square_from(SUM, WGT, src, k, t_k, S, p, weight=WEIGHTS[k], first=k == 0)
                    got = dst.read((SUM, WGT))
                    assert ref.same(got[SUM], want[k][0]), (flags, k, "sum")
                    assert ref.same(got[WGT], want[k][1]), (flags, k, "wgt")
        for k in range(3):                                                    # the source is only read
            assert ref.same(src.download_tile(k), ref.source(w, h, 20 + k))


def test_the_cases_reach_every_radius():
    assert {sq.geometry_square(c[6], c[4], c[5])[4] for c in CASES} == {1, 2, 3}


@pytest.mark.parametrize("name", ["rot30", "half-out"])
def test_a_row_tile_makes_its_own_rows_of_the_whole_image(nl, name):
    (w, h), (ow, oh), S = ref.SHAPES[3]
    case = (name, name, (w, h), (ow, oh), S, 0.7, ref.TRANSFORMS[name](w, h))
    whole = restated(case)
    with nl.StackHandle(3, w, h) as src:
        for k in range(3):
            src.upload_tile(k, ref.source(w, h, 20 + k))
        for row0, rows in ((0, 13), (13, 27)):
            part = restated(case, row0, rows)
            for flags in (0, DIRECT):
                with Planes(nl, ow, oh, row0=row0, rows=rows) as dst:
                    dst.st.set_dev_flags(flags)
                    for k in range(3):
                        staged, direct = dst.st.drizzle_square_tile_paths(src, k, dithered(case[6], k), S, 0.7)
                        assert staged + direct == 2 * -(-rows // 16)
                        dst.st.frame_drizzle_square_from(1, 3, src, k, dithered(case[6], k), S, 0.7, weight=WEIGHTS[k],
                                                         first=k == 0)
                        got = dst.read((1, 3))
                        for plane, slot in ((0, 1), (1, 3)):
                            assert ref.same(got[slot], part[k][plane])
                            assert ref.same(got[slot], whole[k][plane][row0:row0 + rows])


@pytest.mark.parametrize("entry", CFA_CASES, ids=[cref.case_id(e) for e in CFA_CASES])
def test_cfa_square_drizzle_matches_the_restatement_on_both_paths(nl, entry):
    case, channel, cfa = entry
    cid, name, (w, h), (ow, oh), S, p, trans = case
    tiles = -(-ow // 256) * -(-oh // 16)
    SUM, WGT = 2, 0
    want = restated(case, pair=(channel, cfa))
    assert any(np.any(t > 0) for _, t in want)
    with nl.StackHandle(3, w, h) as src:
        for k in range(3):
            src.upload_tile(k, ref.source(w, h, 20 + k))
        for flags in (0, DIRECT, EVERY):
            with Planes(nl, ow, oh) as dst:
                dst.st.set_dev_flags(flags)
                for k in range(3):
                    t_k = dithered(trans, k)
                    staged, direct = dst.st.drizzle_square_tile_paths(src, k, t_k, S, p)
                    assert staged + direct == tiles and (staged == 0 or not flags & DIRECT)
                    dst.st.frame_drizzle_square_cfa_from(SUM, WGT, src, k, t_k, S, channel, cfa, pixfrac=p,
                                                         weight=WEIGHTS[k], first=k == 0)
                    got = dst.read((SUM, WGT))
                    assert ref.same(got[SUM], want[k][0]), (flags, k, "sum")
                    assert ref.same(got[WGT], want[k][1]), (flags, k, "wgt")


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
        for flags in (0, EVERY):
            dst.set_dev_flags(flags)
            dst.frame_drizzle_square_cfa_from(0, 1, src, 0, trans, S, channel, cfa, pixfrac=p, weight=1.5, first=True)
            dst.frame_drizzle_square_from(2, 3, src, 1, trans, S, p, weight=1.5, first=True)
            assert np.any(dst.download_tile(1) > 0)
            assert ref.same(dst.download_tile(0), dst.download_tile(2)) and ref.same(dst.download_tile(1), dst.download_tile(3))
            s, t = sq.accumulate_square_cfa(raw, trans, S, p, ow, oh, channel, cfa, weight=1.5)
            assert ref.same(dst.download_tile(0), s) and ref.same(dst.download_tile(1), t)


def test_the_cross_check_reaches_every_radius():
    assert {sq.geometry_square(c[0][1](67, 35), c[0][2], c[0][3])[4] for c in CROSS} == {1, 2, 3}


def chain_frames():
    """three frames of one smooth sky under small turns and shifts, an outlier in each: (frames, transforms)"""
    w, h = 48, 32
    rng = np.random.default_rng(8)
    transs = [ref.rotation(w, h, deg, 1.0, dx, dy) for deg, dx, dy in ((0.0, 0.0, 0.0), (2.0, 1.3, -0.6), (-3.0, -0.8, 1.1))]
    jj, ii = np.mgrid[0:h, 0:w].astype(np.float64)
    frames = []
    for k, t in enumerate(transs):
        t = t.astype(np.float64)
        x, y = t[0] * ii + t[1] * jj + t[2], t[3] * ii + t[4] * jj + t[5]     # where the pixel lies on the reference grid
        f = (1.0 + 0.5 * np.sin(x / 5.0) * np.cos(y / 7.0) + 0.01 * rng.standard_normal((h, w))).astype(f32)
        f[12 + k, 20 + 3 * k] += f32(10.0) if k != 1 else f32(-10.0)          # one outlier each
        frames.append(f)
    return frames, transs


def invert(t):
    a, b, c, d, e, f = [float(v) for v in t]
    det = a * e - b * d
    return np.array([e / det, -b / det, (b * f - c * e) / det, -d / det, a / det, (c * d - a * f) / det], f32)


def test_stack_blot_reject_square_drizzle_finalize_end_to_end(nl, oracle):
    w, h, S, p = 48, 32, 2.0, 0.7
    ow, oh = 96, 64
    frames, transs = chain_frames()
    blots = [invert(t) for t in transs]
    low = high = 0.5

    # the restatement: the oracle's projection and median, then sqdrizzle_ref
    aligned = []
    for k in range(3):
        rc, a = oracle.project_bilinear(frames[k].reshape(-1), w, h, w, h, transs[k], np.nan)
        assert rc == 0
        aligned.append(a)
    rc, model, _, _, _ = oracle.stack_apply(nl.ST_MEDIAN, np.stack(aligned), None, 3.0, 3.0)
    assert rc == 0
    s = t = None
    counts = []
    for k in range(3):
        rc, blot = oracle.project_bilinear(model, w, h, w, h, blots[k], np.nan)
        assert rc == 0
        kept, n_low, n_high = ref.reject_against(frames[k].reshape(-1), blot, low, high)
        counts.append((n_low, n_high))
        s, t = sq.accumulate_square(kept.reshape(h, w), transs[k], S, p, ow, oh, sum_plane=s, wgt_plane=t, first=k == 0)
    want = ref.finalize(s, t, 0.0, np.nan)
    # (each frame's outlier, and one pixel of the second frame on the border, where the stack ends beside it)
    assert counts == [(0, 1), (1, 1), (0, 1)]

    with nl.StackHandle(2, w, h) as staging, nl.StackHandle(3, w, h) as stack, nl.StackHandle(3, ow, oh) as dz:
        for k in range(3):
            staging.upload_tile(0, frames[k])
            stack.frame_project_from(k, staging, 0, transs[k], np.nan)
        stack.set_exact(True)
        got_model, _, _ = stack.run(nl.ST_MEDIAN, 3.0, 3.0)
        assert ref.same(got_model, model)
        stack.upload_tile(0, got_model)                                       # the finished stack as a slot to blot from
        for k in range(3):
            staging.upload_tile(0, frames[k])
            staging.frame_project_from(1, stack, 0, blots[k], np.nan)         # blot
            assert staging.frame_reject_against(0, 1, low, high) == counts[k]
            dz.frame_drizzle_square_from(0, 1, staging, 0, transs[k], S, p, first=k == 0)
        assert ref.same(dz.download_tile(0), s) and ref.same(dz.download_tile(1), t)
        dz.drizzle_finalize(0, 1, 2)
        got = dz.download_tile(2)
        assert ref.same(got, want)
        # the outliers are gone: the drizzle of the cleaned frames stays within the sky's range
        assert np.nanmax(got) < 2.0 and np.nanmin(got) > 0.0 and np.isfinite(got).mean() > 0.9


def test_error_messages_that_need_a_device(nl):
    from nightlight_amd import capi
    w, h = 40, 24
    ident = [1, 0, 0, 0, 1, 0]
    before = ref.source(w, h, 9)
    with nl.StackHandle(2, w, h) as src, nl.StackHandle(3, 2 * w, 2 * h) as dst, \
            nl.StackHandle(1, w, h, row0=8, rows=8) as tile, nl.StackHandle(3, 2 * w, 2 * h) as lender:
        src.upload_tile(0, before)
        for k in range(3):
            dst.upload_tile(k, np.full(4 * w * h, k, f32))

        def mono(s, t, source, idx, trans=ident, scale=2.0):
            return lambda: dst.frame_drizzle_square_from(s, t, source, idx, trans, scale)

        def cfa(s, t, source, idx, trans=ident, scale=2.0):
            return lambda: dst.frame_drizzle_square_cfa_from(s, t, source, idx, trans, scale, "G", "GRBG")

        def refused(call, words):
            with pytest.raises(capi.NlError) as e:
                call()
            assert e.value.code == capi.ERR_INVALID_ARG and words in str(e.value), str(e.value)
            for k in range(3):
                assert np.all(dst.download_tile(k) == k)

        for form, who in ((mono, "frame_drizzle_square_from"), (cfa, "frame_drizzle_square_cfa_from")):
            refused(form(0, 1, tile, 0), "whole-image")                                            # a row-tile source
            refused(form(1, 1, src, 0), who + ": slot 1 is both the sum and the weight plane")
            refused(form(0, 1, src, 2), who + " (source): bad index 2")
            refused(form(3, 1, src, 0), who + " (sum plane): bad index 3")
            refused(form(0, -1, src, 0), who + " (weight plane): bad index -1")
            refused(form(0, 1, dst, 1), "source and destination")
            refused(form(2, 0, dst, 2), "source and destination")
            refused(form(0, 1, src, 0, sq.R4_SQUARE[1](w, h), 1.0), who + ": window radius 4")
        with pytest.raises(capi.NlError) as e:
            dst.drizzle_square_tile_paths(src, 2, ident, 2.0)
        assert "drizzle_square_tile_paths: bad index 2" in str(e.value)
        dst.attach_device_frames(lender.frames_device_ptr(), lender.frame_stride())
        try:
            with pytest.raises(capi.NlError) as e:
                dst.frame_drizzle_square_from(0, 1, src, 0, ident, 2.0)
            assert e.value.code == capi.ERR_INVALID_ARG and "attached, not owned" in str(e.value)
        finally:
            dst.attach_device_frames(None)
        if nl.device_count() > 1:
            with nl.StackHandle(2, 2 * w, 2 * h, device=1) as far:
                with pytest.raises(capi.NlError) as e:
                    far.frame_drizzle_square_from(0, 1, src, 0, ident, 2.0)
                assert "source on device 0, destination on device 1" in str(e.value)
        # two slots of one handle beside the source's: fine (a handle of the output's size drizzles into itself)
        with nl.StackHandle(3, w, h) as one:
            one.upload_tile(2, before)
            one.frame_drizzle_square_from(0, 1, one, 2, ident, 1.0, first=True)
            s, t = sq.accumulate_square(before, ident, 1.0, 1.0, w, h)
            assert ref.same(one.download_tile(0), s) and ref.same(one.download_tile(1), t)
            assert ref.same(one.download_tile(2), before)
