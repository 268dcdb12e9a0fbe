"""GPU parity of the drizzle integration (include/nlstack_drizzle.h, an extension: the header is the contract) against
its numpy restatement drizzle_ref.py, which test_drizzle_ref.py pins by hand: bit equality throughout, any NaN equal to
any NaN.

The kernel (drizzle.hip) makes 256 x 16 tiles of the output grid; a tile either stages its candidate box in LDS or
reads global memory.  Every case runs on both paths -- as the kernel chooses, and with developer switch 32768 (no tile
stages) -- and the two must give the same bits; nl_stack_drizzle_tile_paths says which tiles took which.  300 x 40 is
two tile columns and three tile rows.  The planes lie in the handle's own buffer, filled with random bits slot by slot
and padding included (a second handle lent the same memory, one row of `stride` pixels per slot, reads and writes it):
after every call only the planes the call names have changed."""
import numpy as np
import pytest

import drizzle_ref as ref

pytestmark = pytest.mark.gpu

f32 = np.float32
DIRECT = 32768
CASES = ref.gpu_cases()
WEIGHTS = (1.0, 0.5, 2.25)
DITHER = ((0.0, 0.0), (0.25, -0.5), (-0.4, 0.3))


class Planes:
    """n slots of random bits, padding included, in the owned buffer of a w x h handle (or a row tile of it)"""

    def __init__(self, nl, w, h, row0=0, rows=None, n=4, seed=3):
        self.st = nl.StackHandle(n, w, h, row0=row0, rows=rows, device=0)
        self.n, self.npix, self.stride = n, self.st.tile_pixels, self.st.frame_stride()
        self.view = nl.StackHandle(n, self.stride, 1, device=0)
        self.view.attach_device_frames(self.st.frames_device_ptr(), self.stride)
        self.before = np.random.default_rng(seed).integers(0, 2 ** 32, (n, self.stride), dtype=np.uint32)
        for k in range(n):
            self.view.upload_tile(k, self.before[k].view(f32))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.view.attach_device_frames(None)
        self.view.close()
        self.st.close()

    def put(self, k, data):
        self.before[k, :self.npix] = np.asarray(data, f32).reshape(-1).view(np.uint32)
        self.view.upload_tile(k, self.before[k].view(f32))

    def read(self, written):
        """every slot's pixels as (n, npix) float32, after asserting that no word outside the slots in `written`
        changed since the last read"""
        after = np.stack([self.view.download_tile(k).view(np.uint32) for k in range(self.n)])
        keep = np.ones(after.shape, bool)
        for k in written:
            keep[k, :self.npix] = False
        assert np.array_equal(after[keep], self.before[keep]), "a word outside the written planes changed"
        self.before = after.copy()
        return after[:, :self.npix].view(f32)


def dithered(trans, k):
    t = np.array(trans, f32)
    t[2] += f32(DITHER[k][0])
    t[5] += f32(DITHER[k][1])
    return t


def restated(case, kernel, row0=0, rows=None):
    """the (sum, wgt) planes after each of the three frames of a case"""
    _, _, (w, h), (ow, oh), S, p, trans = case
    out, s, t = [], None, None
    for k in range(3):
        s, t = ref.accumulate(ref.source(w, h, 20 + k), dithered(trans, k), S, p, ow, oh, sum_plane=s, wgt_plane=t,
                              weight=WEIGHTS[k], first=k == 0, kernel=kernel, row0=row0, rows=rows)
        out.append((s, t))
    return out


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_drizzle_matches_the_restatement_on_both_paths(nl, case):
    cid, name, (w, h), (ow, oh), S, p, trans = case
    tiles = -(-ow // 256) * -(-oh // 16)
    SUM, WGT = 2, 0
    with nl.StackHandle(3, w, h) as src:
        for k in range(3):
            src.upload_tile(k, ref.source(w, h, 20 + k))
        for kernel in (nl.DZ_TURBO, nl.DZ_POINT):
            want = restated(case, kernel)
            assert name == "all-out" or any(np.any(t > 0) for _, t in want)
            for flags in (0, DIRECT):
                with Planes(nl, ow, oh) as dst:
                    dst.st.set_dev_flags(flags)
                    for k in range(3):
                        t_k = dithered(trans, k)
                        staged, direct = dst.st.drizzle_tile_paths(src, k, t_k, S, p)
                        assert staged + direct == tiles and (staged == 0 or not flags)
                        if not flags:
                            print("%s frame %d: tiles staged %d direct %d" % (cid, k, staged, direct))
                            assert name != "all-out" or staged == 0               # all out: no candidate, no box
                            assert name not in ("identity", "shift", "flip") or direct == 0
                        dst.st.frame_drizzle_from(SUM, WGT, src, k, t_k, S, p, weight=WEIGHTS[k], first=k == 0,
                                                  kernel=kernel)
                        got = dst.read((SUM, WGT))
                        assert ref.same(got[SUM], want[k][0]), (kernel, flags, k, "sum")
                        assert ref.same(got[WGT], want[k][1]), (kernel, flags, k, "wgt")
            for k in range(3):                                                # the source is only read
                assert ref.same(src.download_tile(k), ref.source(w, h, 20 + k))


@pytest.mark.parametrize("name", ["rot30", "half-out"])
def test_a_row_tile_makes_its_own_rows_of_the_whole_image(nl, name):
    (w, h), (ow, oh), S = ref.SHAPES[3]
    case = (name, name, (w, h), (ow, oh), S, 0.7, ref.TRANSFORMS[name](w, h))
    whole = restated(case, ref.TURBO)
    with nl.StackHandle(3, w, h) as src:
        for k in range(3):
            src.upload_tile(k, ref.source(w, h, 20 + k))
        for row0, rows in ((0, 13), (13, 27)):
            part = restated(case, ref.TURBO, row0, rows)
            for flags in (0, DIRECT):
                with Planes(nl, ow, oh, row0=row0, rows=rows) as dst:
                    dst.st.set_dev_flags(flags)
                    for k in range(3):
                        staged, direct = dst.st.drizzle_tile_paths(src, k, dithered(case[6], k), S, 0.7)
                        assert staged + direct == 2 * -(-rows // 16)
                        dst.st.frame_drizzle_from(1, 3, src, k, dithered(case[6], k), S, 0.7, weight=WEIGHTS[k], first=k == 0)
                        got = dst.read((1, 3))
                        for plane, slot in ((0, 1), (1, 3)):
                            assert ref.same(got[slot], part[k][plane])
                            assert ref.same(got[slot], whole[k][plane][row0:row0 + rows])


def test_finalize_with_aliased_slots_min_weight_and_nan_weights(nl):
    w, h = 37, 11
    rng = np.random.default_rng(5)
    s = rng.standard_normal(w * h).astype(f32)
    t = rng.random(w * h).astype(f32)
    t[::7] = 0.0
    t[3::11] = np.nan
    t[5::13] = -1.0
    t[6::17] = np.inf
    s[2::19] = np.inf
    s[4::23] = np.nan
    for min_weight, empty in ((0.0, np.nan), (0.25, -7.5), (-2.0, 0.0)):
        want = ref.finalize(s, t, min_weight, empty)
        for S, T, O in ((0, 1, 2), (0, 1, 0), (0, 1, 1), (3, 0, 3)):
            with Planes(nl, w, h) as p:
                p.put(S, s)
                p.put(T, t)
                p.st.drizzle_finalize(S, T, O, min_weight, empty)
                got = p.read((O,))
                assert ref.same(got[O], want), (min_weight, S, T, O)
    # sum and weight in one slot: the quotient of a plane by itself
    with Planes(nl, w, h) as p:
        p.put(1, t)
        p.st.drizzle_finalize(1, 1, 1, 0.0, -1.0)
        assert ref.same(p.read((1,))[1], ref.finalize(t, t, 0.0, -1.0))


def test_reject_against_counts_and_survivors_keep_their_bits(nl):
    w, h = 53, 19
    rng = np.random.default_rng(6)
    m = rng.standard_normal(w * h).astype(f32)
    v = (m + 0.4 * rng.standard_normal(w * h)).astype(f32)
    v[::9] = np.nan
    m[4::9] = np.nan
    v[1::31] = np.inf
    v[2::37] = -np.inf
    m[3::41] = np.inf
    v[5::43] = -0.0
    v[6::47] = f32(1e-42)                                                     # a subnormal
    v[7::9] = m[7::9] + f32(0.5)                                              # on the threshold or a rounding beside it
    for low, high in ((0.5, 0.5), (0.0, 1.0), (0.25, 0.0), (np.inf, np.inf)):
        want, n_low, n_high = ref.reject_against(v, m, low, high)
        with Planes(nl, w, h) as p:
            p.put(0, v)
            p.put(2, m)
            assert p.st.frame_reject_against(0, 2, low, high) == (n_low, n_high)
            got = p.read((0,))[0]
            gone = np.isnan(want) & ~np.isnan(v)
            assert int(gone.sum()) == n_low + n_high and (n_low > 0 and n_high > 0 or low == np.inf)
            assert ref.same(got, want) and np.array_equal(got.view(np.uint32)[~gone], v.view(np.uint32)[~gone])
    with Planes(nl, w, h) as p:                                               # a frame against itself: nothing goes
        p.put(1, v)
        assert p.st.frame_reject_against(1, 1, 0.0, 0.0) == (0, 0)
        assert np.array_equal(p.read(())[1].view(np.uint32), v.view(np.uint32))


def test_stack_blot_reject_drizzle_finalize_end_to_end(nl, oracle):
    w, h, S, p = 48, 32, 2.0, 0.7
    ow, oh = 96, 64
    rng = np.random.default_rng(8)
    yy, xx = np.mgrid[0:h + 8, 0:w + 8].astype(np.float64)
    sky = (1.0 + 0.5 * np.sin(xx / 5.0) * np.cos(yy / 7.0)).astype(f32)
    shifts = ((0, 0), (2, 1), (1, 3))                                         # whole pixels: the frames are cut-outs of one sky
    transs = [np.array([1, 0, dx, 0, 1, dy], f32) for dx, dy in shifts]
    blots = [np.array([1, 0, -dx, 0, 1, -dy], f32) for dx, dy in shifts]
    frames = []
    for k, (dx, dy) in enumerate(shifts):
        f = sky[4 + dy:4 + dy + h, 4 + dx:4 + dx + w] + (0.01 * rng.standard_normal((h, w))).astype(f32)
        f[10 + k, 20 + 2 * k] += f32(10.0) if k != 1 else f32(-10.0)           # one outlier each
        frames.append(f.astype(f32))
    low = high = 0.5

    # the restatement: the oracle's projection and median, then drizzle_ref
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
        s, t = ref.accumulate(kept.reshape(h, w), transs[k], S, p, ow, oh, sum_plane=s, wgt_plane=t, first=k == 0)
    want = ref.finalize(s, t, 0.0, np.nan)
    assert counts == [(0, 1), (1, 0), (0, 1)]

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
            dz.frame_drizzle_from(0, 1, staging, 0, transs[k], S, p, first=k == 0)
        assert ref.same(dz.download_tile(0), s) and ref.same(dz.download_tile(1), t)
        dz.drizzle_finalize(0, 1, 2)
        got = dz.download_tile(2)
        assert ref.same(got, want)
        # the outliers are gone: the drizzle of the cleaned frames stays within the sky's range
        assert np.nanmax(got) < 2.0 and np.nanmin(got) > 0.0 and np.isfinite(got).mean() > 0.9
        mn, mean, mx, _ = dz.frame_stats(1)                                   # the weight map is a slot like any other
        assert (mn, mx) == (t.min(), t.max()) and mx > 0.0


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

        def refused(call, words):
            with pytest.raises(capi.NlError) as e:
                call()
            assert e.value.code == capi.ERR_INVALID_ARG and words in str(e.value), str(e.value)
            for k in range(3):
                assert np.all(dst.download_tile(k) == k)

        refused(lambda: dst.frame_drizzle_from(0, 1, tile, 0, ident, 2.0), "whole-image")          # a row-tile source
        refused(lambda: dst.frame_drizzle_from(1, 1, src, 0, ident, 2.0), "slot 1 is both the sum and the weight plane")
        refused(lambda: dst.frame_drizzle_from(0, 1, src, 2, ident, 2.0), "(source): bad index 2")
        refused(lambda: dst.frame_drizzle_from(3, 1, src, 0, ident, 2.0), "(sum plane): bad index 3")
        refused(lambda: dst.frame_drizzle_from(0, -1, src, 0, ident, 2.0), "(weight plane): bad index -1")
        refused(lambda: dst.frame_drizzle_from(0, 1, dst, 1, ident, 2.0), "source and destination")
        refused(lambda: dst.frame_drizzle_from(2, 0, dst, 2, ident, 2.0), "source and destination")
        refused(lambda: dst.drizzle_finalize(0, 1, 3), "drizzle_finalize (result): bad index 3")
        refused(lambda: dst.drizzle_finalize(0, -1, 2), "drizzle_finalize (weight plane): bad index -1")
        refused(lambda: dst.frame_reject_against(3, 0, 1.0, 1.0), "frame_reject_against: bad index 3")
        refused(lambda: dst.frame_reject_against(0, 5, 1.0, 1.0), "frame_reject_against (model): bad index 5")
        refused(lambda: dst.frame_drizzle_from(0, 1, src, 0, ref.R4[1](w, h), 1.0), "window radius 4")
        with pytest.raises(capi.NlError) as e:
            dst.drizzle_tile_paths(src, 2, ident, 2.0)
        assert "drizzle_tile_paths: bad index 2" in str(e.value)
        dst.attach_device_frames(lender.frames_device_ptr(), lender.frame_stride())
        try:
            with pytest.raises(capi.NlError) as e:
                dst.frame_drizzle_from(0, 1, src, 0, ident, 2.0)
            assert e.value.code == capi.ERR_INVALID_ARG and "attached, not owned" in str(e.value)
        finally:
            dst.attach_device_frames(None)
        if nl.device_count() > 1:
            with nl.StackHandle(2, 2 * w, 2 * h, device=1) as far:
                with pytest.raises(capi.NlError) as e:
                    far.frame_drizzle_from(0, 1, src, 0, ident, 2.0)
                assert "source on device 0, destination on device 1" in str(e.value)
        # two slots of one handle beside the source's: fine (a handle of the output's size drizzles into itself)
        with nl.StackHandle(3, w, h) as one:
            one.upload_tile(2, before)
            one.frame_drizzle_from(0, 1, one, 2, ident, 1.0, first=True)
            s, t = ref.accumulate(before, ident, 1.0, 1.0, w, h)
            assert ref.same(one.download_tile(0), s) and ref.same(one.download_tile(1), t)
            assert ref.same(one.download_tile(2), before)
