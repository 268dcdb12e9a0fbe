"""The restatement in tone_ref.py against vectors worked out by hand from the reference's expressions
(internal/fits/pixelops.go, tiff16.go, writejpg.go), the cap on rounding-boundary pixels that the inputs of
test_gpu_tone.py must meet, and what the new entry points do without a device.  CPU only."""
import math

import numpy as np
import pytest

import tone_ref as ref

f32 = np.float32


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def test_scale_offset_and_normalize():
    d = np.array([0.5, -0.0, np.nan, np.inf], np.float32)
    assert same(ref.scale_offset(d, 2.0, 0.25), [1.25, 0.25, np.nan, np.inf])
    assert same(ref.scale_offset(d[:2], -1.0, 0.0), [-0.5, 0.0])           # -0 * -1 = +0, + 0 = +0
    # Normalize: scale = 1 / (3 - 1) = 0.5, offset = -1 * 0.5
    assert same(ref.normalize(np.array([1, 2, 3, 5], np.float32), 1.0, 3.0), [0, 0.5, 1, 2])
    # max == min: scale = +Inf, offset = -Inf; d > 0 gives Inf - Inf, d < 0 gives -Inf, d == 0 gives 0 * Inf
    assert ref.normalize_constants(0.5, 0.5) == (f32(np.inf), f32(-np.inf))
    assert same(ref.normalize(np.array([0.5, 2, -1, 0], np.float32), 0.5, 0.5), [np.nan, np.nan, -np.inf, np.nan])
    # min == max == 0: offset = -0 * Inf = NaN
    assert np.isnan(ref.normalize(np.array([1, -1], np.float32), 0.0, 0.0)).all()


def test_gamma_special_cases():
    d = np.array([0.25, 0.0, -0.0, 1.0, -0.25, np.nan, np.inf, 4.0], np.float32)
    assert ref.gamma_exponent(2.0) == 0.5 and ref.gamma_exponent(3.0) == float(f32(1) / f32(3))    # fp32, then widened
    assert same(ref.gamma(d, 2.0), [0.5, 0, 0, 1, np.nan, np.nan, np.inf, 2])
    # g == 0: an exponent of +Inf; g < 0: a negative power, +-0 gives +Inf
    assert ref.gamma_exponent(0.0) == np.inf
    assert same(ref.gamma(d, 0.0), [0, 0, 0, 1, 0, np.nan, np.inf, np.inf])
    assert same(ref.gamma(d, -2.0), [2, np.inf, np.inf, 1, np.nan, np.nan, 0, 0.5])
    assert same(ref.gamma(d, 0.5), [0.0625, 0, 0, 1, 0.0625, np.nan, np.inf, 16])


def test_partial_gamma_leaves_the_ends_and_everything_outside():
    d = np.array([0.25, 0.75, 0.5, 0.1, 0.9, np.nan, -0.0, np.inf], np.float32)
    out = ref.partial_gamma(d, 0.25, 0.75, 2.0)
    # d == from and d == to are untouched; 0.5: dd = 0.25 * 2, from + float32(sqrt(0.5)) * 0.5
    mid = f32(0.25) + f32(f32(math.sqrt(0.5)) * f32(0.5))
    assert same(out, [0.25, 0.75, mid, 0.1, 0.9, np.nan, -0.0, np.inf])
    nan_in = np.array([np.nan], np.float32)
    nan_in.view(np.uint32)[0] = 0x7fc12345                                # a NaN keeps its payload
    assert bits(ref.partial_gamma(nan_in, 0.25, 0.75, 2.0))[0] == 0x7fc12345
    assert np.array_equal(bits(ref.partial_gamma(d, 0.75, 0.25, 2.0)), bits(d))     # from > to: no pixel qualifies


def test_midtones_by_hand():
    # mid 0.25, black 0.5: clipLow = 0.5 * -0.75 / (-0.5 * 0.5 - 0.25) = 0.75, scaler = 1 / 0.25 = 4
    assert ref.midtones_constants(0.25, 0.5) == (f32(0.75), f32(4))
    d = np.array([0.25, 0.5, 1.0, 2.0, np.nan], np.float32)
    #  0.25: -0.1875 / -0.375 = 0.5 < clipLow -> 0 -> (0 - 0.75) * 4;   0.5: 0.75, inside -> 0;   1: 1 -> 1;
    #  2: -1.5 / -1.25 = 1.2 > 1 -> 1 -> 1;   NaN falls through both tests
    assert same(ref.midtones(d, 0.25, 0.5), [-3, 0, 1, 1, np.nan])
    # black 0: clipLow = -0 / -0.25 = +0, scaler 1; a negative value is clipped to 0
    assert ref.midtones_constants(0.25, 0.0) == (f32(0), f32(1))
    assert same(ref.midtones(np.array([0.5, -0.25, 2.0], np.float32), 0.25, 0.0), [0.75, 0, 1])


def test_shift_black_is_go_s_max():
    # before 0.5, after 0: black = -0.5 / -1 = 0.5, scale = 2
    assert ref.shift_black_constants(0.5, 0.0) == (f32(0.5), f32(2))
    out = ref.shift_black(np.array([0.75, 0.5, 0.25, np.nan, np.inf, -np.inf], np.float32), 0.5, 0.0)
    assert same(out, [0.5, 0, 0, np.nan, np.inf, 0]) and bits(out)[2] == 0         # a negative product gives +0
    # before 1.5, after 0.5: black = -1 / -0.5 = 2, scale = 1 / (1 - 2) = -1; d == 2: +0 * -1 = -0, and Max(0, -0) = +0
    assert ref.shift_black_constants(1.5, 0.5) == (f32(2), f32(-1))
    out = ref.shift_black(np.array([2.0, 1.0, 3.0], np.float32), 1.5, 0.5)
    assert same(out, [0, 1, 0]) and bits(out)[0] == 0


def test_export_counts_by_hand():
    d = np.array([0.0, 1.0, 0.5, np.nan, -1.0, 2.0, np.inf, -np.inf, 0.25], np.float32)
    assert list(ref.export_gray(d, 0.0, 1.0, 1.0, 16)) == [0, 65535, 32767, 0, 0, 65535, 65535, 0, 16383]
    assert list(ref.export_gray(d, 0.0, 1.0, 1.0, 8)) == [0, 255, 127, 0, 0, 255, 255, 0, 63]
    # gamma 2: sqrt, then truncation: sqrt(0.25) * 65535 = 32767.5
    assert list(ref.export_gray(d, 0.0, 1.0, 2.0, 16)) == [0, 65535, 46340, 0, 0, 65535, 65535, 0, 32767]
    # min == max: scale = +Inf; d == min gives 0 * Inf = NaN -> 0, above 1, below 0
    assert list(ref.export_gray(np.array([0.5, 0.6, 0.4], np.float32), 0.5, 0.5, 1.0, 16)) == [0, 65535, 0]
    # the bytes of 0x1234 in image.Gray16.Pix: high byte first
    assert ref.export_gray(np.array([0x1234 / 65535 + 1e-6], np.float32), 0, 1, 1.0, 16).astype(">u2").tobytes() == b"\x12\x34"


def test_near_boundary_marks_ties_and_nothing_else():
    f64 = np.float64
    a = np.float32(0.7)
    b = np.nextafter(a, f32(1))
    mid = (f64(a) + f64(b)) / 2
    ulp = np.spacing(mid)
    p = np.array([mid, mid + 60 * ulp, mid - 60 * ulp, mid + 70 * ulp, f64(a), f64(b), 0.0, np.inf, np.nan, 3.5e38])
    assert list(ref.near_boundary(p)) == [True, True, True, False, False, False, False, False, False, False]
    # exact squares tie exactly: 4097^2 = 2^24 + 8193 needs 25 bits
    x = f32(4097.0) * f32(2.0) ** -24
    assert ref.near_boundary(np.array([f64(x) * f64(x)]))[0]


def test_the_gpu_tests_inputs_meet_the_cap():
    """At most 1e-3 of a frame's pixels may lie near a rounding boundary, in every power test_gpu_tone.py compares:
    the looser bar those pixels get must not be able to swallow a wrong kernel."""
    cases = 0
    for what, pixels, near in ref.power_cases():
        assert near.sum() <= 1e-3 * pixels, "%s: %d of %d pixels near a boundary" % (what, near.sum(), pixels)
        cases += 1
    assert cases == len(ref.SHAPES) * 2 * (len(ref.GAMMAS) * (1 + len(ref.PARTIAL_RANGES)) + 4)


def test_inputs_hold_what_the_kernels_must_survive():
    for w, h in ref.SHAPES[1:]:
        data = ref.sky(w, h)
        assert np.isnan(data).any() and np.isinf(data).any() and (data < 0).any() and (data > 1).any()
        assert (bits(data) == 0x80000000).any()
        assert np.isfinite(ref.plain(w, h)).all()


@pytest.fixture(scope="module")
def nl():
    import nightlight_amd
    nightlight_amd.capi.load()
    return nightlight_amd


def test_argument_errors_need_no_device(nl):
    frame = np.linspace(0, 1, 16, dtype=np.float32)
    for call in (lambda: nl.tone(frame, 6, 1.0), lambda: nl.tone(frame, -1, 1.0),
                 lambda: nl.export_gray(frame, 0, 1, 1.0, bits=12), lambda: nl.export_gray(frame, 0, 1, 0.0),
                 lambda: nl.export_gray(frame, 0, 1, -1.0), lambda: nl.export_gray(frame, 0, 1, np.nan)):
        with pytest.raises(nl.NlError) as e:
            call()
        assert e.value.code == nl.capi.ERR_INVALID_ARG, e.value
    lib = nl.capi.load()
    assert lib.nl_tone(nl.capi.fptr(frame.copy()), 16, None, None, None, None, 0) == nl.capi.ERR_INVALID_ARG
    assert "null curve" in nl.capi.last_error()
    assert lib.nl_export_gray(nl.capi.fptr(frame), 16, 0.0, 1.0, 1.0, 16, None, 0) == nl.capi.ERR_INVALID_ARG
    assert "null output" in nl.capi.last_error()
    # OpGamma's own guard with no statistics asked for: nothing to compute, no device needed
    assert np.array_equal(bits(nl.tone(frame, nl.TONE_GAMMA, 1.0)), bits(frame))


def test_tone_and_export_have_no_cpu_fallback(nl):
    if nl.capi.device_count() > 0:
        pytest.skip("a device is visible: the no-device contract is checked on CPU-only hosts")
    frame = np.linspace(0, 1, 16, dtype=np.float32)
    calls = [lambda k=k, p=p: nl.tone(frame, k, *p)
             for k, p in ((nl.TONE_SCALE_OFFSET, (2.0, 0.0)), (nl.TONE_NORMALIZE, (0.0, 1.0)), (nl.TONE_GAMMA, (2.0,)),
                          (nl.TONE_PARTIAL_GAMMA, (0.2, 0.8, 2.0)), (nl.TONE_MIDTONES, (0.25, 0.1)),
                          (nl.TONE_SHIFT_BLACK, (0.5, 0.1)))]
    calls += [lambda: nl.tone(frame, nl.TONE_GAMMA, 1.0, stats=True), lambda: nl.export_gray(frame, 0, 1, 1.0, 16),
              lambda: nl.export_gray(frame, 0, 1, 2.2, 8)]
    for call in calls:
        before = frame.copy()
        with pytest.raises(nl.NlError) as e:
            call()
        assert e.value.code == nl.capi.ERR_NO_DEVICE and "no HIP device" in str(e.value)
        assert np.array_equal(frame, before)
