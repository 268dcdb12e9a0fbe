"""GPU parity of the colour steps of the rgb / lrgb command -- nl_stack_frame_combine_from, nl_stack_rgb_* and the host
forms nl_rgb_balance / nl_export_rgb -- against the CPU restatement in colour_ref.py, on the inputs defined there.

Bars.  Everything without a power is bit for bit the restatement's: any NaN equals any NaN, the sign of a zero counts.
The two powers (NL_CHROMA_GAMMA, the export with gamma != 1) are bit-exact outside tone_ref.near_boundary (at most 1e-3
of a frame, test_colour_ref.py holds the inputs to that) and within one fp32 ulp / one count inside it.  The planes sit
in a buffer of the test's own filled with random bits, at the handle's stride: after every call only the plane the
reference writes has changed.  Everything runs in this one pytest process."""
import numpy as np
import pytest

import colour_ref as ref
import tone_ref

pytestmark = pytest.mark.gpu

f32 = np.float32
WHOLE = [s for s in ref.SHAPES]
SHADOWS, HIGHLIGHTS = (0.05, 0.06, 0.07), (0.9, 0.95, 1.0)
LOC, SCALE = (0.45, 0.5, 0.55), (0.1, 0.12, 0.09)
DEV_COLOUR_DIRECT = 131072


def bits(a):
    return np.asarray(a, np.float32).reshape(-1).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def first_diff(a, b):
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    bad = np.flatnonzero(~((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))
    return "%d differ, first at %d: %r vs %r" % (bad.size, bad[0], a[bad[0]], b[bad[0]]) if bad.size else "equal"


def ordered(a):
    i = bits(a).astype(np.int64)
    return np.where(i & 0x80000000, 0x80000000 - i, i)


class Rig:
    """Five slots of random bits in a buffer of the test's own; slots planes[c] hold data[c]."""

    def __init__(self, nl, w, h, data, planes=(1, 2, 3), row0=0, rows=None):
        import torch
        self.st = nl.StackHandle(5, w, h, row0=row0, rows=rows, device=0)
        self.npix, self.planes, self.stride = self.st.tile_pixels, planes, self.st.frame_stride()
        self.before = np.random.default_rng(3).integers(0, 2 ** 32, 5 * self.stride, dtype=np.uint32)
        for c in range(3):
            self.before[planes[c] * self.stride:planes[c] * self.stride + self.npix] = bits(data[c])
        self.buf = torch.from_numpy(self.before.view(np.int32).copy()).to("cuda:0")
        self.st.attach_device_frames(self.buf.data_ptr(), self.stride)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.st.attach_device_frames(None)
        self.st.close()

    def read(self, written):
        """the three planes as (3, npix) float32, after asserting that nothing but the planes in `written` (channel
        numbers) changed since the last read"""
        after = self.buf.cpu().numpy().view(np.uint32)
        keep = np.ones(after.size, bool)
        for c in written:
            keep[self.planes[c] * self.stride:self.planes[c] * self.stride + self.npix] = False
        assert np.array_equal(after[keep], self.before[keep]), "a word outside the written planes changed"
        self.before = after.copy()
        return np.stack([after[self.planes[c] * self.stride:self.planes[c] * self.stride + self.npix].view(np.float32)
                         for c in range(3)])


def err(nl, call, *needles):
    with pytest.raises(nl.NlError) as e:
        call()
    assert e.value.code == nl.capi.ERR_INVALID_ARG, e.value
    for n in needles:
        assert n in str(e.value), e.value


@pytest.mark.parametrize("w,h", ref.SHAPES)
def test_combine(nl, w, h):
    sky, plain = ref.planes("sky", w, h), ref.planes("plain", w, h)
    mn, mult = ref.normalization([0.1, 0.05, 0.2], [0.9, 1.5, 0.7])
    with nl.StackHandle(2, w, h, device=0) as src, nl.StackHandle(3, w, h, device=0) as dst:
        err(nl, lambda: dst.frame_combine_from(0, src, -1, mn, mult), "frame_combine_from", "has not run a pass")
        src.upload_frames([sky[0], plain[1]])
        dst.upload_frames([plain[0], plain[1], plain[2]])
        dst.frame_combine_from(1, src, 0, mn, mult)
        assert same(dst.download_tile(1), ref.combine(sky[0], mn, mult)), first_diff(dst.download_tile(1), ref.combine(sky[0], mn, mult))
        assert same(dst.download_tile(0), plain[0]) and same(dst.download_tile(2), plain[2]) and same(src.download_tile(0), sky[0])
        dst.frame_combine_from(2, dst, 2, mn, mult)                              # in place
        assert same(dst.download_tile(2), ref.combine(plain[2], mn, mult))
        res, _, _ = src.run(nl.ST_MEAN, 3.0, 3.0)                                # a real pass, then its result
        dst.frame_combine_from(0, src, -1, mn, mult)
        assert same(dst.download_tile(0), ref.combine(res, mn, mult))
        assert same(src.download_rows(-1, 0, h), res)
        err(nl, lambda: dst.frame_combine_from(3, src, 0, mn, mult), "frame_combine_from (destination)", "bad index 3")
        err(nl, lambda: dst.frame_combine_from(0, src, 2, mn, mult), "frame_combine_from (source)", "bad index 2")
        err(nl, lambda: dst.frame_combine_from(0, src, -2, mn, mult), "frame_combine_from (source)", "bad index -2")
    with nl.StackHandle(1, w + 1, h, device=0) as other, nl.StackHandle(1, w, h, device=0) as dst:
        err(nl, lambda: dst.frame_combine_from(0, other, 0, mn, mult), "frame_combine_from: source %dx%d" % (w + 1, h))


@pytest.mark.parametrize("w,h", ref.SHAPES)
def test_clamp_and_its_statistics(nl, w, h):
    alpha, beta = (1.7, -1.0, 0.5), (-0.3, 1.2, 0.25)
    for name in ("sky", "plain"):
        data = ref.planes(name, w, h)
        want = ref.scale_offset_clamp(data, alpha, beta)
        with Rig(nl, w, h, data, planes=(3, 1, 2)) as rig:
            stats = rig.st.rgb_scale_offset_clamp(rig.planes, alpha, beta, stats=True)
            got = rig.read({0, 1, 2})
            assert same(got, want), "%s: %s" % (name, first_diff(got, want))
            for c in range(3):
                after = rig.st.frame_stats(rig.planes[c], variance=False)
                assert np.array_equal(bits(stats[c]), bits(np.array(after[:3], np.float32))), (name, c, stats[c], after)
            if name == "plain":
                assert np.array_equal(stats[:, 0], want.min(axis=1)) and np.array_equal(stats[:, 2], want.max(axis=1))
        with Rig(nl, w, h, data) as rig:                                          # without statistics: the same pixels
            assert rig.st.rgb_scale_offset_clamp(rig.planes, alpha, beta) is None
            assert same(rig.read({0, 1, 2}), want)


def darkest_cases(w, h):
    cases = [(b, border) for b in ref.BLOCKS for border in ref.BORDERS]
    cases += [(max(w, h) + 1, 0.0), (5, 0.1), (7, 0.0)]                           # no block at all; no divisor of the size
    if min(w, h) >= 128:
        cases += [(128, 0.0), (100, 0.1)]                                         # a strip staged in several chunks
    return cases


@pytest.mark.parametrize("w,h", ref.SHAPES)
def test_darkest_block(nl, w, h):
    for name in ("sky", "plain"):
        data = ref.planes(name, w, h)
        with Rig(nl, w, h, data) as rig:
            for block, border in darkest_cases(w, h):
                want = ref.darkest_block(data, w, h, block, border)
                got = rig.st.rgb_darkest_block(rig.planes, block, border)
                assert same(got, want), "%s block %d border %g: %r vs %r" % (name, block, border, got, want)
                if block > max(w, h):
                    assert np.array_equal(got, [ref.FMAX] * 3)
            rig.st.set_dev_flags(DEV_COLOUR_DIRECT)                               # ... and without the LDS
            for block, border in darkest_cases(w, h)[::3]:
                assert same(rig.st.rgb_darkest_block(rig.planes, block, border), ref.darkest_block(data, w, h, block, border))
            rig.st.set_dev_flags(0)
            rig.read(set())
    if (w, h) == (512, 512):
        assert ref.darkest_block(ref.planes("plain", w, h), w, h, 16, 0.1)[0] < 0.5


@pytest.mark.parametrize("w,h", ref.SHAPES)
def test_mean_star_intensity(nl, w, h):
    stars = ref.stars(w, h)
    for name, clip in (("sky", (0.9, 0.95, 2.0)), ("plain", (0.8, 0.9, 0.85)), ("plain", (0.0, 1.0, 1.0))):
        data = ref.planes(name, w, h)
        with Rig(nl, w, h, data) as rig:
            for skip_bright, skip_dim in ref.SKIPS:
                want = ref.mean_star_intensity(data, w, h, stars, skip_bright, skip_dim, clip)
                got = rig.st.rgb_mean_star_intensity(rig.planes, stars, skip_bright, skip_dim, clip)
                assert same(got, want), "%s skips %g %g: %r vs %r" % (name, skip_bright, skip_dim, got, want)
            assert np.array_equal(bits(rig.st.rgb_mean_star_intensity(rig.planes, None, 0.0, 0.0, clip)), [0, 0, 0])
            assert np.array_equal(bits(rig.st.rgb_mean_star_intensity(rig.planes, stars, 0.6, 0.6, clip)), [0, 0, 0])
            rig.read(set())
    assert np.isnan(ref.mean_star_intensity(ref.planes("plain", w, h), w, h, stars, 0.0, 0.0, (0.0, 1.0, 1.0))).all()


@pytest.mark.parametrize("w,h", ref.SHAPES)
def test_chroma_and_hue_steps(nl, w, h):
    steps = [(ref.CHROMA_NEUTRALIZE, (0.2, 0.3), 1), (ref.CHROMA_NEUTRALIZE, (np.nan, 0.3), 1),
             (ref.CHROMA_FOR_HUES, (295.0, 30.0, 0.5), 1), (ref.CHROMA_FOR_HUES, (100.0, 300.0, 4.0), 1),
             (ref.CHROMA_FOR_HUES, (np.nan, 300.0, 4.0), 1), (ref.ROTATE_HUES, (90.0, 200.0, -30.0, 0.2), 0),
             (ref.ROTATE_HUES, (300.0, 60.0, 45.0, 0.0), 0)]
    for name in ("sky", "plain"):
        data = ref.hcl(name, w, h)
        with Rig(nl, w, h, data) as rig:
            cur = data
            for kind, p, written in steps:                                        # each step on the result of the last
                want = ref.chroma(cur, kind, *p)
                rig.st.rgb_chroma(rig.planes, kind, *p)
                cur = rig.read({written})
                assert same(cur, want), "%s kind %d %r: %s" % (name, kind, p, first_diff(cur, want))
                if w * h >= 225 and not np.isnan(p[0]):
                    assert not np.array_equal(bits(cur), bits(data))
        for g, thr in ref.CHROMA_GAMMAS:
            with Rig(nl, w, h, data) as rig:
                touched, power = ref.chroma_gamma_parts(data, g, thr)
                near = touched & tone_ref.near_boundary(power)
                want = ref.chroma(data, ref.CHROMA_GAMMA, g, thr)
                rig.st.rgb_chroma(rig.planes, ref.CHROMA_GAMMA, g, thr)
                got = rig.read({1})
                assert np.array_equal(bits(got[1])[~touched], bits(data[1])[~touched])          # NaN payloads included
                assert same(got[1][~near], want[1][~near]), "%s gamma %g: %s" % (name, g, first_diff(got[1][~near], want[1][~near]))
                if near.any():
                    assert np.isfinite(got[1][near]).all() and (np.abs(ordered(got[1][near]) - ordered(want[1][near])) <= 1).all()


@pytest.mark.parametrize("w,h", ref.SHAPES)
def test_export(nl, w, h):
    for name in ("sky", "plain"):
        data = ref.planes(name, w, h)
        with Rig(nl, w, h, data, planes=(2, 3, 1)) as rig:
            for mn, mx, gamma, nbits in ref.EXPORTS:
                got = rig.st.rgb_export(rig.planes, mn, mx, gamma, nbits)
                want = ref.export_rgb(data, mn, mx, gamma, nbits)
                assert got.shape == want.shape == (w * h, 4)
                near = np.zeros((w * h, 4), bool)
                for c in range(3):
                    gray, gamma_inv = tone_ref.export_parts(data[c], mn, mx, gamma)
                    if gamma_inv != 1.0:
                        near[:, c] = tone_ref.near_boundary(tone_ref._pow32(gray, gamma_inv)[1])
                diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
                what = "%s export [%g, %g] gamma %g, %d bits" % (name, mn, mx, gamma, nbits)
                assert (diff[~near] == 0).all(), "%s: %d counts differ" % (what, np.count_nonzero(diff[~near]))
                assert (diff[near] <= 1).all(), what
                if gamma == 1.0:
                    assert not near.any()
                    raw = ref.rgba64_bytes(want) if nbits == 16 else want.astype(np.uint8).tobytes()
                    assert got.tobytes() == raw, what
                host = nl.export_rgb(data, mn, mx, gamma, nbits)
                assert host.dtype == got.dtype and np.array_equal(host, got), what
            rig.read(set())


def test_rgba64_byte_order(nl):
    counts = np.array([[0x0102, 0x1234, 0xfffe], [0x00ff, 0xff00, 0x8001]], np.uint16)
    data = ((counts.T.astype(np.float64) + 0.5) / 65535.0).astype(np.float32)
    got = nl.export_rgb(data, 0.0, 1.0, 1.0, 16)
    assert got.dtype == np.dtype(">u2")
    assert got.tobytes() == b"\x01\x02\x12\x34\xff\xfe\xff\xff" b"\x00\xff\xff\x00\x80\x01\xff\xff"
    # the same floats as 8-bit counts: (0xfffe + 0.5) / 65535 * 255 = 254.99 -> 254, (0xff00 + 0.5) ... = 254.01 -> 254
    assert ref.export_rgb(data, 0.0, 1.0, 1.0, 8).tolist() == [[1, 0x12, 0xfe, 255], [0, 0xfe, 0x7f, 255]]
    assert nl.export_rgb(data, 0.0, 1.0, 1.0, 8).tobytes() == bytes([1, 0x12, 0xfe, 255, 0, 0xfe, 0x7f, 255])


@pytest.mark.parametrize("w,h", ref.SHAPES)
def test_balance(nl, w, h):
    stars = ref.stars(w, h)
    block = 2 if w < 15 else 8
    args = (stars, block, 0.1, 0.1, 0.1, SHADOWS, HIGHLIGHTS, LOC, SCALE)
    for name in ("plain", "sky"):
        data = ref.planes(name, w, h)
        with Rig(nl, w, h, data) as rig:
            rep = rig.st.rgb_balance(rig.planes, *args)
            got = rig.read({0, 1, 2})
        host, host_rep = nl.rgb_balance(data, w, h, *args)
        assert same(host, got), "%s: resident and host forms differ: %s" % (name, first_diff(host, got))
        for k in rep:
            assert same(rep[k], host_rep[k]), (name, k)
        if name == "plain":
            want, want_rep = ref.set_black_white_points(data, w, h, *args)
            assert same(got, want), first_diff(got, want)
            for k in want_rep:
                assert same(rep[k], want_rep[k]), (k, rep[k], want_rep[k])
            assert np.isfinite(rep["alpha1"]).all() and not np.array_equal(bits(got), bits(data))


def test_row_tile_handles(nl):
    w, h, row0, rows = 67, 64, 13, 30
    data = ref.hcl("sky", w, h)
    tile = data[:, row0 * w:(row0 + rows) * w]
    alpha, beta = (1.7, -1.0, 0.5), (-0.3, 1.2, 0.25)
    with nl.StackHandle(3, w, h, row0=row0, rows=rows, device=0) as st, \
            nl.StackHandle(1, w, h, row0=row0, rows=rows, device=0) as src:
        planes = (0, 1, 2)
        st.upload_frames(list(data))
        src.upload_frame(0, data[1])
        counts = st.rgb_export(planes, 0.0, 1.0, 1.0, 8)
        assert counts.shape == (rows * w, 4) and np.array_equal(counts, ref.export_rgb(tile, 0.0, 1.0, 1.0, 8))
        st.rgb_chroma(planes, ref.CHROMA_FOR_HUES, 295.0, 30.0, 0.5)
        want = ref.chroma(tile, ref.CHROMA_FOR_HUES, 295.0, 30.0, 0.5)
        assert all(same(st.download_tile(c), want[c]) for c in range(3))
        stats = st.rgb_scale_offset_clamp(planes, alpha, beta, stats=True)
        want = ref.scale_offset_clamp(want, alpha, beta)
        for c in range(3):
            assert same(st.download_tile(c), want[c])
            assert np.array_equal(bits(stats[c]), bits(np.array(st.frame_stats(c, variance=False)[:3], np.float32)))
        st.frame_combine_from(2, src, 0, 0.25, 2.0)
        assert same(st.download_tile(2), ref.combine(tile[1], 0.25, 2.0))
        rgb = (0.9, 0.9, 0.9)
        for call in (lambda: st.rgb_darkest_block(planes, 4, 0.0),
                     lambda: st.rgb_mean_star_intensity(planes, ref.stars(w, h), 0.0, 0.0, rgb),
                     lambda: st.rgb_balance(planes, ref.stars(w, h), 4, 0.0, 0.0, 0.0, rgb, rgb, LOC, SCALE)):
            err(nl, call, "rgb_", "needs a whole-image handle")
    with nl.StackHandle(1, w, h, device=0) as whole, nl.StackHandle(1, w, h, row0=row0, rows=rows, device=0) as part:
        err(nl, lambda: part.frame_combine_from(0, whole, 0, 0.0, 1.0), "frame_combine_from: source")


def test_errors_by_message(nl):
    import ctypes as C
    w, h = 64, 48
    data = ref.planes("plain", w, h)
    stars = ref.stars(w, h).copy()
    rgb = (0.9, 0.9, 0.9)
    with nl.StackHandle(3, w, h, device=0) as st:
        st.upload_frames(list(data))
        p = (0, 1, 2)
        one = np.ones(3, np.float32)
        lib, hd = st._lib, st._h
        planes = (C.c_int * 3)(0, 1, 2)
        out = nl.capi.Rgb()
        bad_hfr, neg_hfr, big_hfr = stars.copy(), stars.copy(), stars.copy()
        bad_hfr["hfr"][5], neg_hfr["hfr"][5], big_hfr["hfr"][5] = np.nan, -1.0, 1400.0
        cases = [
            (lambda: st.rgb_scale_offset_clamp((0, 1, 3), one, one), ("rgb_scale_offset_clamp", "bad index 3")),
            (lambda: st.rgb_scale_offset_clamp((0, 1, 1), one, one), ("rgb_scale_offset_clamp", "slot 1 names two planes")),
            (lambda: st.rgb_scale_offset_clamp((-1, 1, 2), one, one), ("rgb_scale_offset_clamp", "bad index -1")),
            (lambda: nl.capi.check(lib.nl_stack_rgb_scale_offset_clamp(hd, None, nl.capi.fptr(one), nl.capi.fptr(one), None)),
             ("rgb_scale_offset_clamp", "null planes")),
            (lambda: nl.capi.check(lib.nl_stack_rgb_scale_offset_clamp(hd, planes, None, nl.capi.fptr(one), None)),
             ("rgb_scale_offset_clamp", "null coefficients")),
            (lambda: st.rgb_darkest_block(p, 0, 0.0), ("rgb_darkest_block", "block size 0")),
            (lambda: st.rgb_darkest_block(p, 4, -0.1), ("rgb_darkest_block", "border")),
            (lambda: st.rgb_darkest_block(p, 4, np.nan), ("rgb_darkest_block", "border")),
            (lambda: st.rgb_darkest_block(p, 4, 1e30), ("rgb_darkest_block", "border")),
            (lambda: nl.capi.check(lib.nl_stack_rgb_darkest_block(hd, planes, 4, 0.0, None)), ("rgb_darkest_block", "null output")),
            (lambda: st.rgb_mean_star_intensity(p, bad_hfr, 0.0, 0.0, rgb), ("rgb_mean_star_intensity", "star 5 has HFR")),
            (lambda: st.rgb_mean_star_intensity(p, neg_hfr, 0.0, 0.0, rgb), ("rgb_mean_star_intensity", "star 5 has HFR")),
            (lambda: st.rgb_mean_star_intensity(p, big_hfr, 0.0, 0.0, rgb), ("rgb_mean_star_intensity", "star 5 has HFR")),
            (lambda: st.rgb_mean_star_intensity(p, stars, -0.5, 0.0, rgb), ("rgb_mean_star_intensity", "select stars")),
            (lambda: st.rgb_mean_star_intensity(p, stars, 0.0, -0.5, rgb), ("rgb_mean_star_intensity", "select stars")),
            (lambda: nl.capi.check(lib.nl_stack_rgb_mean_star_intensity(hd, planes, None, 3, 0.0, 0.0, out, C.byref(out))),
             ("rgb_mean_star_intensity", "3 stars")),
            (lambda: st.rgb_balance(p, stars, 0, 0.0, 0.0, 0.0, rgb, rgb, LOC, SCALE), ("rgb_balance", "block size 0")),
            (lambda: st.rgb_chroma(p, 4, 1.0), ("rgb_chroma", "unknown kind 4")),
            (lambda: st.rgb_chroma(p, -1, 1.0), ("rgb_chroma", "unknown kind -1")),
            (lambda: nl.capi.check(lib.nl_stack_rgb_chroma(hd, planes, None)), ("rgb_chroma", "null operation")),
            (lambda: st.rgb_export(p, 0.0, 1.0, 1.0, 12), ("rgb_export", "12 bits")),
            (lambda: st.rgb_export(p, 0.0, 1.0, 0.0, 16), ("rgb_export", "gamma")),
            (lambda: st.rgb_export(p, 0.0, 1.0, np.nan, 16), ("rgb_export", "gamma")),
            (lambda: nl.capi.check(lib.nl_stack_rgb_export(hd, planes, 0.0, 1.0, 1.0, 16, None)), ("rgb_export", "null output")),
            (lambda: nl.export_rgb(data, 0.0, 1.0, -1.0, 8), ("export_rgb", "gamma")),
        ]
        for call, needles in cases:
            err(nl, call, *needles)
        # a star with a bad HFR outside the selected range is never looked at
        assert np.isfinite(st.rgb_mean_star_intensity(p, bad_hfr, 0.25, 0.0, rgb)).all()
        for c in range(3):                                                        # ... and nothing was written
            assert np.array_equal(bits(st.download_tile(c)), bits(data[c]))


def test_one_chain_from_three_stacks_to_rgba64(nl):
    """three stacked channels, the common normalisation from their statistics, combine x 3 from the passes' results,
    balance and a 16-bit export, against the restatement end to end"""
    w, h = 261, 70
    rng = np.random.default_rng(21)
    stars = ref.stars(w, h)
    results, mins, maxs = [], [], []
    with nl.StackHandle(3, w, h, device=0) as rgb:
        chans = [nl.StackHandle(3, w, h, device=0) for _ in range(3)]
        try:
            for c, st in enumerate(chans):
                st.upload_frames([(900.0 + 100.0 * c + 40.0 * rng.standard_normal(w * h)).astype(np.float32) for _ in range(3)])
                res, _, _ = st.run(nl.ST_MEAN, 3.0, 3.0)
                mn, _, mx = st.result_tone(nl.TONE_GAMMA, 1.0, stats=True)       # the no-op fills the statistics
                assert mn == res.min() and mx == res.max()
                results.append(res)
                mins.append(mn)
                maxs.append(mx)
            mn, mult = nl.rgb_normalization(mins, maxs)
            for c, st in enumerate(chans):
                rgb.frame_combine_from(c, st, -1, mn, mult)
        finally:
            for st in chans:
                st.close()
        want = np.stack([ref.combine(results[c], *ref.normalization(mins, maxs)) for c in range(3)])
        assert all(same(rgb.download_tile(c), want[c]) for c in range(3))
        loc = [f32(np.median(want[c])) for c in range(3)]
        scale = [f32(np.std(want[c])) for c in range(3)]
        args = (stars, 16, 0.1, 0.0, 0.75, SHADOWS, HIGHLIGHTS, loc, scale)
        rep = rgb.rgb_balance((0, 1, 2), *args)
        want, want_rep = ref.set_black_white_points(want, w, h, *args)
        for k in want_rep:
            assert same(rep[k], want_rep[k]), (k, rep[k], want_rep[k])
        assert all(same(rgb.download_tile(c), want[c]) for c in range(3))
        got = rgb.rgb_export((0, 1, 2), 0.0, 1.0, 1.0, 16)
        assert got.tobytes() == ref.rgba64_bytes(ref.export_rgb(want, 0.0, 1.0, 1.0, 16))
        assert got[:, :3].max() > 30000 and (got[:, 3] == 65535).all()
