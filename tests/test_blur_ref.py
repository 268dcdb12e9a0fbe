"""The restatement in blur_ref.py against what the reference's own tests pin (internal/ops/stretch/usm_test.go): the
taps of TestGaussianKernel1D (tests/golden/gaussian_kernel_1d.json) and the properties of TestGaussFilter2D and
TestUnsharpMask; then nl_gaussian_kernel_1d against the restatement bit for bit, and the deviations that need no
device.  CPU only."""
import json
import os

import numpy as np
import pytest

import blur_ref as ref

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gaussian_kernel_1d.json")
TAP_COUNTS = {0.215: 1, 0.3: 1, 1: 3, 1.5: 5, 2: 9, 3: 13, 10: 45, 50: 231}


@pytest.fixture(scope="module")
def nl():
    import nightlight_amd
    nightlight_amd.capi.load()
    return nightlight_amd


def test_taps_meet_the_reference_s_vectors():
    golden = json.load(open(GOLDEN))
    eps = golden["epsilon"]
    assert eps == 1e-5 and [c["sigma"] for c in golden["cases"]] == [1.0, 2.0, 3.0]
    for case in golden["cases"]:
        kernel = ref.gaussian_kernel_1d(case["sigma"])
        want = np.array(case["kernel"], np.float32)
        assert kernel.dtype == np.float32 and kernel.size == want.size
        total = f32(0)
        for got, exp in zip(kernel, want):
            assert abs(float(f32(got - exp))) <= eps, (case["sigma"], got, exp)
            total = f32(total + got)
        assert abs(float(f32(total - f32(1)))) <= eps


def footprint(dim, k):
    inside = np.zeros((dim, dim), bool)
    inside[dim // 2 - k:dim // 2 + k + 1, dim // 2 - k:dim // 2 + k + 1] = True
    # the reference leaves column width/2 - kHalfSize - 1 of the footprint's rows unchecked (usm_test.go:101, :107)
    unchecked = np.zeros((dim, dim), bool)
    unchecked[dim // 2 - k:dim // 2 + k + 1, dim // 2 - k - 1] = True
    return inside, unchecked


@pytest.mark.parametrize("dim", [15, 31, 63])
@pytest.mark.parametrize("sigma", [1.0, 2.0, 3.0])
def test_gauss_filter_2d_properties(dim, sigma):
    # TestGaussFilter2D (usm_test.go:54-135)
    peak = f32(9.99)
    sharp = np.zeros(dim * dim, np.float32)
    sharp[dim * (dim // 2) + dim // 2] = peak
    kernel = ref.gaussian_kernel_1d(sigma)
    k = kernel.size // 2
    blur = ref.convolve_separable(sharp, dim, kernel).reshape(dim, dim)
    inside, unchecked = footprint(dim, k)
    assert (blur[~inside & ~unchecked] == 0).all()
    assert (blur[inside] > 0).all() and (blur[inside] < peak).all()
    total = f32(0)
    for v in blur.reshape(-1):                   # the reference's fp32 running sum, row-major
        total = f32(total + v)
    assert abs(float(f32(total - peak))) <= 1e-5
    assert np.array_equal(ref.gaussian_blur(sharp, dim, sigma).reshape(dim, dim), blur)


@pytest.mark.parametrize("sigma", [1.0, 2.0, 3.0])
def test_unsharp_mask_properties(sigma):
    # TestUnsharpMask (usm_test.go:137-228): dim 15, background 10, peak 15, gain 1, min 0, max 20, threshold 0
    dim, back, peak, hi = 15, f32(10), f32(15), f32(20)
    sharp = np.full(dim * dim, back, np.float32)
    sharp[dim * (dim // 2) + dim // 2] = peak
    out = ref.unsharp_mask(sharp, dim, sigma, 1.0, 0, hi, 0).reshape(dim, dim)
    k = ref.gaussian_kernel_1d(sigma).size // 2
    inside, unchecked = footprint(dim, k)
    outside = ~inside & ~unchecked
    assert (np.abs((out[outside] - back).astype(np.float64)) <= 1e-5).all()
    centre = np.zeros((dim, dim), bool)
    centre[dim // 2, dim // 2] = True
    assert out[dim // 2, dim // 2] > peak and out[dim // 2, dim // 2] <= hi
    assert (out[inside & ~centre] > 0).all() and (out[inside & ~centre] <= hi).all()


def test_unsharp_mask_order_of_the_tests():
    # d < absThreshold copies; r < min before r > max, so min > max ends at max; NaN falls through every test
    d = np.array([1, 5, 5, np.nan, 5], np.float32)
    b = np.array([0, 0, 9, 1, np.nan], np.float32)
    out = ref.apply_unsharp_mask(d, b, 1.0, 7, 3, 2)
    #   1 < 2: 1;   5 + 5 = 10 -> (10 < 7 no) 10 > 3: 3;   5 - 4 = 1 -> 1 < 7: 7 -> 7 > 3: 3;   NaN;   NaN
    assert np.array_equal(out[:3], np.array([1, 3, 3], np.float32)) and np.isnan(out[3:]).all()
    assert np.array_equal(ref.apply_unsharp_mask(d[:3], b[:3], 1.0, 0, 20, np.nan), np.array([2, 10, 1], np.float32))


def test_convolution_order_and_sign_of_zero():
    # 0 + (-0 * tap) = +0: an all -0 frame comes out +0; and the taps are taken in ascending order, not mirrored
    neg = np.full(12, -0.0, np.float32)
    out = ref.convolve_separable(neg, 4, np.array([0.25, 0.5, 0.25], np.float32))
    assert (out.view(np.uint32) == 0).all()
    row = np.array([1, 2, 4, 8], np.float32)
    taps = np.array([1, 10, 100], np.float32)    # out[x] = data[x-1] + 10 data[x] + 100 data[x+1], edges reflected
    assert np.array_equal(ref.convolve_1d_x(row, 4, taps), np.array([211, 421, 842, 884], np.float32))
    assert np.array_equal(ref.convolve_1d_y(row, 1, taps), np.array([211, 421, 842, 884], np.float32))


@pytest.mark.parametrize("sigma", sorted(TAP_COUNTS))
def test_library_taps_are_the_restatement_s_bits(nl, sigma):
    want = ref.gaussian_kernel_1d(sigma)
    got = nl.gaussian_kernel_1d(sigma)
    assert got.size == want.size == TAP_COUNTS[sigma]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def invalid(nl, call, *args, **kw):
    with pytest.raises(nl.NlError) as e:
        call(*args, **kw)
    assert e.value.code == nl.capi.ERR_INVALID_ARG, e.value
    return str(e.value)


def test_deviations_without_a_device(nl):
    frame = np.ones(64, np.float32)
    # 1: a sigma the reference cannot handle
    for sigma in (np.nan, -1.0, np.inf, 0.0, 0.2, 0.1, 1e-30):
        assert "usm.go" in invalid(nl, nl.gaussian_kernel_1d, sigma)
        with pytest.raises(ref.GoPanic):
            ref.gaussian_kernel_1d(sigma)
    assert "usm.go" in invalid(nl, nl.gaussian_kernel_1d, 1e9)              # the bounded radius search
    for sigma in (np.nan, -1.0, np.inf, 0.2):
        assert "usm.go" in invalid(nl, nl.gaussian_blur, frame, 8, 8, sigma)
        assert "usm.go" in invalid(nl, nl.unsharp_mask, frame, 8, 8, sigma, 1.0, 0.0, 1.0, 0.0)
    # 3: an even or non-positive number of taps
    for n in (0, 2, 4):
        assert "usm.go" in invalid(nl, nl.convolve_separable, frame, 8, 8, np.ones(n, np.float32))
    # 4: less room than taps; the count still comes back
    assert "13 taps" in invalid(nl, nl.gaussian_kernel_1d, 3.0, capacity=12)
    assert nl.gaussian_kernel_1d(3.0, capacity=13).size == 13 and nl.gaussian_kernel_1d(3.0, capacity=99).size == 13
    # 2 needs no device either: a radius above the width or the height
    assert "reflect" in invalid(nl, nl.gaussian_blur, np.ones(40, np.float32), 5, 8, 3.0)
    assert "reflect" in invalid(nl, nl.convolve_separable, np.ones(40, np.float32), 8, 5, np.ones(13, np.float32))


def test_guards_need_no_device(nl):
    frame = np.arange(64, dtype=np.float32)
    assert np.array_equal(nl.gaussian_blur(frame, 8, 8, 0.0), frame)
    assert np.array_equal(nl.unsharp_mask(frame, 8, 8, 0.0, 1.0, 0.0, 1.0, 0.0), frame)
    assert np.array_equal(nl.unsharp_mask(frame, 8, 8, 1.5, 0.0, 0.0, 1.0, 0.0), frame)
    assert nl.blur_tap_paths(9) == (True, True) and nl.blur_tap_paths(57) == (True, False)
    assert nl.blur_tap_paths(81) == (False, False)
