"""GPU parity of the tone curves and the gray export -- nl_tone, nl_export_gray and the resident forms
nl_stack_frame_* / nl_stack_result_* -- against the CPU restatement in tone_ref.py, on the inputs defined there.

Bars.  Curves without a power (scale-offset, normalize, midtones, shift-black, the pixels partial gamma leaves alone):
the bits of every pixel equal the restatement's; any NaN equals any NaN, the sign of a zero counts.  Powers: the same
outside tone_ref.near_boundary (at most 1e-3 of a frame, test_tone_ref.py holds the inputs to that), at most one fp32
ulp inside it -- neither Go's pow nor the device's is correctly rounded -- and special values exact everywhere.  The ulp
is the narrowed power's, float32(pow(...)).  Gamma stores that.  Partial gamma stores from + power * rescale2, two more
roundings, which can turn one ulp of the power into two of the pixel (sky 512 x 512, g 0.5, [0.25, 0.95], pixel 67904:
the power 0x3eabebbc / ...bd gives the pixel 0x3ef85836 / ...38), so there the pixel has to be, bit for bit, what the
reference's expression makes of a power at most one ulp from the restatement's.  Export:
counts equal outside near_boundary, within one count inside, exactly equal when gamma == 1.  Statistics: the bits
nl_stack_frame_stats returns on the slot afterwards.  Everything runs in this one pytest process."""
import numpy as np
import pytest

import tone_ref as ref

pytestmark = pytest.mark.gpu

f32 = np.float32
# (kind, arguments) without a power
PLAIN_CURVES = [(ref.SCALE_OFFSET, (1.7, -0.3)), (ref.SCALE_OFFSET, (-1.0, 0.0)), (ref.NORMALIZE, (0.05, 0.9)),
                (ref.NORMALIZE, (0.5, 0.5)), (ref.MIDTONES, (0.25, 0.1)), (ref.MIDTONES, (0.012, 0.09)),
                (ref.SHIFT_BLACK, (0.3, 0.1)), (ref.SHIFT_BLACK, (1.5, 0.5))]
# one of every kind for the statistics and the resident forms
EVERY_KIND = [(ref.SCALE_OFFSET, (1.7, -0.3)), (ref.NORMALIZE, (0.05, 0.9)), (ref.GAMMA, (2.2,)),
              (ref.PARTIAL_GAMMA, (0.25, 0.95, 1.5)), (ref.MIDTONES, (0.25, 0.1)), (ref.SHIFT_BLACK, (0.3, 0.1))]


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
    """fp32 bits as integers in the order of the values: neighbours differ by 1"""
    i = bits(a).astype(np.int64)
    return np.where(i & 0x80000000, 0x80000000 - i, i)


def assert_power(got, want, near, what):
    """bits equal outside `near`; inside it at most one ulp, finite and non-zero on both sides"""
    assert same(got[~near], want[~near]), "%s: %s" % (what, first_diff(got[~near], want[~near]))
    if near.any():
        g, w = got[near], want[near]
        assert np.isfinite(g).all() and np.isfinite(w).all(), what
        assert (np.abs(ordered(g) - ordered(w)) <= 1).all(), "%s: more than one ulp at a boundary" % what


def assert_partial_gamma(got, want, near, p, lo, hi, what):
    """bits equal outside `near`; inside it the pixel is from + q * rescale2 for a q at most one ulp from float32(p)"""
    assert same(got[~near], want[~near]), "%s: %s" % (what, first_diff(got[~near], want[~near]))
    if near.any():
        p32 = p[near].astype(np.float32)
        assert np.isfinite(p32).all() and np.isfinite(got[near]).all(), what
        allowed = [bits(ref.partial_gamma_of_power(q, lo, hi))
                   for q in (np.nextafter(p32, f32(-np.inf)), p32, np.nextafter(p32, f32(np.inf)))]
        ok = (bits(got[near]) == allowed[0]) | (bits(got[near]) == allowed[1]) | (bits(got[near]) == allowed[2])
        assert ok.all(), "%s: a power more than one ulp from the restatement's at a boundary" % what


@pytest.mark.parametrize("w,h", ref.SHAPES)
def test_curves_without_a_power(nl, w, h):
    for name, data in (("sky", ref.sky(w, h)), ("plain", ref.plain(w, h))):
        for kind, p in PLAIN_CURVES:
            got = nl.tone(data, kind, *p)
            want = ref.tone(data, kind, *p)
            assert same(got, want), "%s, kind %d %r: %s" % (name, kind, p, first_diff(got, want))


@pytest.mark.parametrize("w,h", ref.SHAPES)
def test_gamma(nl, w, h):
    for name, data in (("sky", ref.sky(w, h)), ("plain", ref.plain(w, h))):
        for g in ref.GAMMAS:
            want, p = ref._pow32(data, ref.gamma_exponent(g))
            assert_power(nl.tone(data, ref.GAMMA, g), want, ref.near_boundary(p), "%s gamma %g" % (name, g))


@pytest.mark.parametrize("w,h", ref.SHAPES)
def test_partial_gamma(nl, w, h):
    for name, data in (("sky", ref.sky(w, h)), ("plain", ref.plain(w, h))):
        for g in ref.GAMMAS:
            for lo, hi in ref.PARTIAL_RANGES:
                touched, _, p = ref.partial_gamma_parts(data, lo, hi, g)
                got = nl.tone(data, ref.PARTIAL_GAMMA, lo, hi, g)
                what = "%s partial gamma %g [%g, %g]" % (name, g, lo, hi)
                assert np.array_equal(bits(got)[~touched], bits(data)[~touched]), what      # NaN payloads included
                assert_partial_gamma(got, ref.partial_gamma(data, lo, hi, g), touched & ref.near_boundary(p), p, lo, hi, what)
                if data.size >= 225:
                    assert touched.any() == (lo < hi)


@pytest.mark.parametrize("w,h", ref.SHAPES)
def test_export_gray(nl, w, h):
    for name, data in (("sky", ref.sky(w, h)), ("plain", ref.plain(w, h))):
        for mn, mx, gamma, nbits in ref.EXPORTS:
            got = nl.export_gray(data, mn, mx, gamma, nbits)
            want = ref.export_gray(data, mn, mx, gamma, nbits)
            assert got.size == want.size == data.size
            gray, gamma_inv = ref.export_parts(data, mn, mx, gamma)
            near = ref.near_boundary(ref._pow32(gray, gamma_inv)[1]) if gamma_inv != 1.0 else np.zeros(data.size, bool)
            what = "%s export [%g, %g] gamma %g, %d bits" % (name, mn, mx, gamma, nbits)
            diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
            assert (diff[~near] == 0).all(), "%s: %d counts differ" % (what, np.count_nonzero(diff[~near]))
            assert (diff[near] <= 1).all(), what


def test_export_byte_order(nl):
    # counts 0x0102, 0x1234, 0xfffe ...: distinct high and low bytes, high byte first in memory
    counts = np.array([0x0102, 0x1234, 0xfffe, 0x00ff, 0xff00, 0x8001, 0x7f80], np.uint16)
    data = ((counts.astype(np.float64) + 0.5) / 65535.0).astype(np.float32)
    assert np.array_equal(ref.export_gray(data, 0.0, 1.0, 1.0, 16), counts)
    got = nl.export_gray(data, 0.0, 1.0, 1.0, 16)
    assert got.dtype == np.dtype(">u2") and np.array_equal(got.astype(np.uint16), counts)
    assert got.tobytes() == b"\x01\x02\x12\x34\xff\xfe\x00\xff\xff\x00\x80\x01\x7f\x80"
    assert nl.export_gray(data, 0.0, 1.0, 1.0, 8).tobytes() == bytes(ref.export_gray(data, 0.0, 1.0, 1.0, 8))


def stats_bits(t):
    return [int(bits(np.array([v], np.float32))[0]) for v in t[:3]]


def stats_frames():
    w, h = 261, 70
    nan0 = ref.plain(w, h).copy()
    nan0[0] = np.nan
    return [("sky", w, h, ref.sky(w, h)), ("plain", w, h, ref.plain(w, h)), ("tail", 15, 15, ref.plain(15, 15)),
            ("no quad", 1, 3, ref.plain(1, 3)), ("all NaN", w, h, np.full(w * h, np.nan, np.float32)),
            ("element 0 NaN", w, h, nan0), ("second sweep",) + ref.STATS_SHAPE + (ref.plain(*ref.STATS_SHAPE),)]


@pytest.mark.parametrize("name,w,h,data", stats_frames(), ids=[f[0] for f in stats_frames()])
def test_fused_statistics_are_frame_stats_bits(nl, name, w, h, data):
    kinds = EVERY_KIND + [(ref.GAMMA, (1.0,))]                 # ... and the no-op, which fills them too
    with nl.StackHandle(2, w, h, device=0) as st:
        for kind, p in kinds:
            st.upload_frame(0, data)
            st.upload_frame(1, data)
            got = st.frame_tone(0, kind, *p, stats=True)
            after = st.frame_stats(0, variance=False)
            assert stats_bits(got) == stats_bits(after), "%s, kind %d: %r vs %r" % (name, kind, got, after[:3])
            # with the outputs NULL: the same pixels
            assert st.frame_tone(1, kind, *p) is None
            assert np.array_equal(bits(st.download_tile(0)), bits(st.download_tile(1))), (name, kind)
            if name == "plain":                                # ... and they are the transformed slot's
                dev = st.download_tile(0)
                assert np.isfinite(dev).all() and got[0] == dev.min() and got[2] == dev.max()
                assert abs(float(got[1]) - float(np.mean(dev, dtype=np.float64))) <= 1e-6 * abs(float(got[1]))


def test_only_one_statistic_asked_for(nl):
    w, h = 67, 35
    data = ref.plain(w, h)
    t = nl.capi.Tone(ref.SHIFT_BLACK, (0.3, 0.1, 0.0))
    import ctypes as C
    with nl.StackHandle(1, w, h, device=0) as st:
        st.upload_frame(0, data)
        mx = C.c_float(-1.0)
        nl.capi.check(st._lib.nl_stack_frame_tone(st._h, 0, C.byref(t), None, None, C.byref(mx)))
        assert f32(mx.value) == st.frame_stats(0, variance=False)[2] == ref.shift_black(data, 0.3, 0.1).max()


@pytest.mark.parametrize("w,h", [(67, 35), (512, 512)])
def test_resident_slot_equals_host_and_touches_nothing_else(nl, w, h):
    """Slots at the handle's stride (padded for 512 x 512) in a buffer of this test's own filled with random bits:
    after a curve on slot 1 only that slot's w * h floats have changed, and they are the host form's."""
    import torch
    npix = w * h
    data = ref.sky(w, h)
    with nl.StackHandle(3, w, h, device=0) as st:
        stride = st.frame_stride()
        assert (stride > npix) == (w == 512)
        rng = np.random.default_rng(3)
        before = rng.integers(0, 2 ** 32, 3 * stride, dtype=np.uint32)
        for kind, p in EVERY_KIND:
            before[stride:stride + npix] = data.view(np.uint32)
            buf = torch.from_numpy(before.view(np.int32).copy()).to("cuda:0")
            st.attach_device_frames(buf.data_ptr(), stride)
            st.frame_tone(1, kind, *p, stats=(kind % 2 == 0))
            after = buf.cpu().numpy().view(np.uint32)
            want = nl.tone(data, kind, *p)
            assert np.array_equal(after[stride:stride + npix], bits(want)), kind
            changed = np.flatnonzero(after != before)
            assert changed.size and changed.min() >= stride and changed.max() < stride + npix
            counts = st.frame_export_gray(1, 0.0, 1.0, 2.2, 16)
            assert np.array_equal(counts, nl.export_gray(want, 0.0, 1.0, 2.2, 16))
            assert np.array_equal(buf.cpu().numpy().view(np.uint32), after)         # the export writes no frame
            st.attach_device_frames(None)


def test_result_forms(nl):
    w, h = 261, 70
    frames = [ref.plain(w, h), ref.sky(w, h)]
    with nl.StackHandle(2, w, h, device=0) as st:
        for call in (lambda: st.result_tone(ref.GAMMA, 2.2), lambda: st.result_tone(ref.GAMMA, 1.0, stats=True),
                     lambda: st.result_export_gray(0.0, 1.0)):
            with pytest.raises(nl.NlError) as e:              # before any pass
                call()
            assert e.value.code == nl.capi.ERR_INVALID_ARG and "has not run a pass" in str(e.value)
        st.upload_frames(frames)
        res, _, _ = st.run(nl.ST_MEAN, 3.0, 3.0)
        for kind, p in EVERY_KIND:
            got_stats = st.result_tone(kind, *p, stats=True)
            want, want_stats = nl.tone(res, kind, *p, stats=True)
            res = st.download_rows(-1, 0, h)
            assert np.array_equal(bits(res), bits(want)), kind
            assert stats_bits(got_stats) == stats_bits(want_stats)
        assert np.array_equal(st.result_export_gray(0.0, 1.0, 2.2, 8), nl.export_gray(res, 0.0, 1.0, 2.2, 8))
        for i in range(2):                                    # the frames stay
            assert same(st.download_tile(i), frames[i])


def test_row_tile_handle_transforms_its_tile_only(nl):
    w, h, row0, rows = 67, 64, 13, 30
    data = ref.sky(w, h)
    tile = data[row0 * w:(row0 + rows) * w]
    with nl.StackHandle(2, w, h, row0=row0, rows=rows, device=0) as st:
        st.upload_frame(0, data)
        st.upload_frame(1, data)
        got = st.frame_tone(0, ref.MIDTONES, 0.25, 0.1, stats=True)
        assert same(st.download_tile(0), ref.midtones(tile, 0.25, 0.1))
        assert stats_bits(got) == stats_bits(st.frame_stats(0, variance=False))
        assert same(st.download_tile(1), tile)
        counts = st.frame_export_gray(1, 0.0, 1.0, 1.0, 16)
        assert counts.size == rows * w and np.array_equal(counts, ref.export_gray(tile, 0.0, 1.0, 1.0, 16))
        st.run(nl.ST_MEAN, 3.0, 3.0)
        before = st.download_rows(-1, 0, rows)
        st.result_tone(ref.SCALE_OFFSET, 2.0, 1.0)
        assert same(st.download_rows(-1, 0, rows), ref.scale_offset(before, 2.0, 1.0))


def test_guards_leave_every_bit(nl):
    w, h = 67, 35
    data = ref.sky(w, h)
    out, stats = nl.tone(data, ref.GAMMA, 1.0, stats=True)
    assert np.array_equal(bits(out), bits(data))
    with nl.StackHandle(1, w, h, device=0) as st:
        st.upload_frame(0, data)
        assert st.frame_tone(0, ref.GAMMA, 1.0) is None
        assert stats_bits(st.frame_tone(0, ref.GAMMA, 1.0, stats=True)) == stats_bits(st.frame_stats(0, False)) == stats_bits(stats)
        assert np.array_equal(bits(st.download_tile(0)), bits(data))
        # partial gamma has no guard of its own: g == 1 computes from + dd * rescale2, which rounds
        st.frame_tone(0, ref.PARTIAL_GAMMA, 0.25, 0.95, 1.0)
        assert same(st.download_tile(0), ref.partial_gamma(data, 0.25, 0.95, 1.0))


def test_errors_on_a_handle(nl):
    import ctypes as C
    with nl.StackHandle(1, 64, 64, device=0) as st:
        st.fill_synthetic(seed=3)
        before = st.download_tile(0)
        out = np.empty(64 * 64 * 2, np.uint8)
        calls = [lambda: st.frame_tone(1, ref.GAMMA, 2.0), lambda: st.frame_tone(-1, ref.GAMMA, 2.0),
                 lambda: st.frame_tone(0, 6, 2.0), lambda: st.frame_tone(0, -1, 2.0, stats=True),
                 lambda: st.frame_export_gray(1, 0.0, 1.0), lambda: st.frame_export_gray(-1, 0.0, 1.0),
                 lambda: st.frame_export_gray(0, 0.0, 1.0, bits=12), lambda: st.frame_export_gray(0, 0.0, 1.0, gamma=0.0),
                 lambda: st.frame_export_gray(0, 0.0, 1.0, gamma=-2.0), lambda: st.frame_export_gray(0, 0.0, 1.0, gamma=np.nan),
                 lambda: nl.capi.check(st._lib.nl_stack_frame_tone(st._h, 0, None, None, None, None)),
                 lambda: nl.capi.check(st._lib.nl_stack_frame_export_gray(st._h, 0, 0.0, 1.0, 1.0, 16, None))]
        for call in calls:
            with pytest.raises(nl.NlError) as e:
                call()
            assert e.value.code == nl.capi.ERR_INVALID_ARG and "frame_" in str(e.value), e.value
        assert np.array_equal(bits(st.download_tile(0)), bits(before))
        assert out.size == st.frame_export_gray(0, 0.0, 1.0).nbytes


def test_one_chain_on_the_result(nl):
    """normalize, shift-black, gamma 2.2, unsharp mask and a 16-bit export on a stacked result, each step's min / max
    from the previous step's fused statistics, against the same chain through the host forms."""
    w, h = 261, 70
    rng = np.random.default_rng(9)
    frames = [(900.0 + 40.0 * rng.standard_normal(w * h)).astype(np.float32) for _ in range(3)]
    with nl.StackHandle(3, w, h, device=0) as st:
        st.upload_frames(frames)
        host, _, _ = st.run(nl.ST_MEAN, 3.0, 3.0)
        lo, hi = f32(host.min()), f32(host.max())
        mn, mean, mx = st.result_tone(ref.NORMALIZE, lo, hi, stats=True)
        host, hs = nl.tone(host, ref.NORMALIZE, lo, hi, stats=True)
        assert stats_bits(hs) == stats_bits((mn, mean, mx)) and mn == 0.0 and 0.99 < mx <= 1.0
        mn, mean, mx = st.result_tone(ref.SHIFT_BLACK, mean, mean / f32(2), stats=True)
        host, hs = nl.tone(host, ref.SHIFT_BLACK, hs[1], hs[1] / f32(2), stats=True)
        assert stats_bits(hs) == stats_bits((mn, mean, mx))
        mn, mean, mx = st.result_tone(ref.GAMMA, 2.2, stats=True)
        host, hs = nl.tone(host, ref.GAMMA, 2.2, stats=True)
        assert stats_bits(hs) == stats_bits((mn, mean, mx))
        st.result_unsharp_mask(1.5, 1.0, mn, mx, mean)
        host = nl.unsharp_mask(host, w, h, 1.5, 1.0, hs[0], hs[2], hs[1])
        got = st.result_export_gray(mn, mx, 1.0, 16)
        assert np.array_equal(bits(st.download_rows(-1, 0, h)), bits(host))
        assert np.array_equal(got, nl.export_gray(host, hs[0], hs[2], 1.0, 16))
        assert got.max() > 60000 and got.min() == 0
