"""GPU parity of the Gaussian blur and the unsharp mask -- nl_convolve_separable, nl_gaussian_blur, nl_unsharp_mask and
the resident forms nl_stack_frame_* / nl_stack_result_* -- against the CPU restatement in blur_ref.py.

Bar: the bits of every pixel equal the restatement's given the same taps (the library's own, which test_blur_ref.py
compares with the restatement's bit for bit); any NaN equals any NaN, the sign of a zero counts.  Everything runs in
this one pytest process."""
import functools

import numpy as np
import pytest

import blur_ref as ref

pytestmark = pytest.mark.gpu

f32 = np.float32
# partial 16-byte groups, partial tiles, one and several tiles in both directions; 512 x 512 is exactly 1 MiB
SHAPES = [(15, 15), (63, 31), (67, 35), (256, 16), (261, 70), (5, 300), (521, 300), (512, 512)]
SIGMAS = [0.3, 1.0, 1.5, 2.0, 3.0, 10.0]                     # 1, 3, 5, 9, 13 and 45 taps


def same(a, b):
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def first_diff(a, b):
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    bad = np.flatnonzero(~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
    return "%d differ, first at %d: %r vs %r" % (bad.size, bad[0], a[bad[0]], b[bad[0]]) if bad.size else "equal"


@functools.lru_cache(maxsize=None)
def sky(w, h):
    """Gaussian sky with NaN, +-Inf, -0.0, 0.0 and values near +-1e30 sprinkled in: products overflow, inf - inf arises."""
    rng = np.random.default_rng(11 * w + h)
    img = (1000.0 + 30.0 * rng.standard_normal(w * h)).astype(np.float32)
    pick = rng.random(w * h)
    for lo, value in ((0.00, np.nan), (0.01, np.inf), (0.015, -np.inf), (0.02, -0.0), (0.04, 0.0), (0.05, 1e30),
                      (0.06, -1e30), (0.07, 3e38)):
        img[(pick >= lo) & (pick < lo + 0.005)] = value
    for i, value in enumerate((np.nan, np.inf, -np.inf, -0.0, 1e30, -1e30)):       # ... and in the smallest frame too
        img[1 + i * (w * h - 1) // 6] = value
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def calm(w, h):
    """Finite sky with a few stars, -0.0 and NaN: what an unsharp mask meets."""
    rng = np.random.default_rng(5 * w + h)
    img = (0.2 + 0.02 * rng.standard_normal(w * h)).astype(np.float32)
    img[rng.integers(0, w * h, max(3, w * h // 200))] = 0.9
    img[rng.integers(0, w * h, 3)] = np.nan
    img[rng.integers(0, w * h, 3)] = -0.0
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def plain(w, h):
    """Finite sky with -0.0 only: under a wide kernel the specials of sky() spread over the whole frame, here every
    pixel keeps a number, so every tap's weight and place shows."""
    rng = np.random.default_rng(7 * w + h)
    img = (1000.0 + 30.0 * rng.standard_normal(w * h)).astype(np.float32)
    img[rng.integers(0, w * h, 5)] = -0.0
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def blurred_ref(w, h, sigma, kind):
    import nightlight_amd as nl
    taps = nl.gaussian_kernel_1d(sigma)
    return taps, ref.convolve_separable((sky if kind == "sky" else calm)(w, h), w, taps)


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_gaussian_blur(nl, w, h, sigma):
    radius = nl.gaussian_kernel_1d(sigma).size // 2
    data = sky(w, h)
    if radius > min(w, h):                                   # deviation 2
        with pytest.raises(nl.NlError) as e:
            nl.gaussian_blur(data, w, h, sigma)
        assert e.value.code == nl.capi.ERR_INVALID_ARG and "reflect" in str(e.value)
        return
    taps, want = blurred_ref(w, h, sigma, "sky")
    assert nl.blur_tap_paths(taps.size) == (True, True)
    got = nl.gaussian_blur(data, w, h, sigma)
    assert same(got, want), first_diff(got, want)
    assert np.isnan(want).any() and not same(want, data)


def test_every_sigma_ran_somewhere(nl):
    fits = {s: [wh for wh in SHAPES if nl.gaussian_kernel_1d(s).size // 2 <= min(wh)] for s in SIGMAS}
    assert all(len(v) >= 3 for v in fits.values()) and (521, 300) in fits[10.0]


@pytest.mark.parametrize("w,h", [(6, 40), (40, 6), (6, 6)])
def test_radius_equal_to_the_size(nl, w, h):
    # sigma 3: radius 6, the reflection reaches the far edge
    taps = nl.gaussian_kernel_1d(3.0)
    assert taps.size == 13
    data = sky(w, h)
    got = nl.gaussian_blur(data, w, h, 3.0)
    want = ref.convolve_separable(data, w, taps)
    assert same(got, want), first_diff(got, want)


@pytest.mark.parametrize("w,h", [(5, 40), (40, 5)])
def test_radius_above_the_size_is_invalid_arg(nl, w, h):
    data = sky(w, h)
    for call in (lambda: nl.gaussian_blur(data, w, h, 3.0),
                 lambda: nl.unsharp_mask(data, w, h, 3.0, 1.0, 0.0, 1.0, 0.0),
                 lambda: nl.convolve_separable(data, w, h, np.ones(13, np.float32))):
        with pytest.raises(nl.NlError) as e:
            call()
        assert e.value.code == nl.capi.ERR_INVALID_ARG and "reflect" in str(e.value)
    with pytest.raises(ref.GoPanic):
        ref.convolve_separable(data, w, np.ones(13, np.float32))
    with nl.StackHandle(1, w, h, device=0) as st:
        st.upload_frame(0, data)
        with pytest.raises(nl.NlError) as e:
            st.frame_gaussian_blur(0, 3.0)
        assert e.value.code == nl.capi.ERR_INVALID_ARG
        assert same(st.download_tile(0), data)


def test_all_negative_zero_comes_out_positive_zero(nl):
    w, h = 67, 35
    data = np.full(w * h, -0.0, np.float32)
    got = nl.gaussian_blur(data, w, h, 1.5)
    assert (got.view(np.uint32) == 0).all()
    assert same(got, ref.gaussian_blur(data, w, 1.5))


def asymmetric_taps(n, seed):
    rng = np.random.default_rng(seed)
    taps = rng.uniform(0.05, 1.0, n).astype(np.float32)      # no symmetry, does not sum to 1
    taps[n // 3] = f32(-0.37)
    return taps


# (taps, row pass staged, column pass staged): radius 28 lies between the two limits
@pytest.mark.parametrize("n,row_staged,col_staged", [(1, True, True), (7, True, True), (49, True, True),
                                                     (57, True, False), (65, True, False), (67, False, False),
                                                     (81, False, False)])
@pytest.mark.parametrize("w,h", [(67, 35), (261, 70), (521, 300), (512, 512)])
def test_convolve_separable_asymmetric(nl, w, h, n, row_staged, col_staged):
    assert nl.blur_tap_paths(n) == (row_staged, col_staged)
    taps = asymmetric_taps(n, n)
    data = sky(w, h)
    if n // 2 > min(w, h):                                   # deviation 2 (81 taps on 67 x 35)
        with pytest.raises(nl.NlError) as e:
            nl.convolve_separable(data, w, h, taps)
        assert e.value.code == nl.capi.ERR_INVALID_ARG and "reflect" in str(e.value)
        return
    got = nl.convolve_separable(data, w, h, taps)
    want = ref.convolve_separable(data, w, taps)
    assert same(got, want), first_diff(got, want)
    data = plain(w, h)
    got = nl.convolve_separable(data, w, h, taps)
    want = ref.convolve_separable(data, w, taps)
    assert same(got, want), first_diff(got, want)
    assert np.isfinite(want).all()
    if n > 1:                                                # the order shows: the mirrored kernel gives other bits
        assert not same(want, ref.convolve_separable(data, w, taps[::-1].copy()))


def usm_cases(data):
    fin = data[np.isfinite(data)]
    lo, hi, med = f32(fin.min()), f32(fin.max()), f32(np.median(fin))
    return [("threshold inside the range", 1.5, lo, hi, med),
            ("NaN threshold", 1.0, lo, hi, f32(np.nan)),
            ("min above max", 2.0, hi, lo, med),
            ("negative gain", -0.75, lo, hi, med),
            ("threshold 0 against NaN and -0", 1.0, lo, hi, f32(0)),
            ("NaN bounds", 1.0, f32(np.nan), f32(np.nan), med)]


@pytest.mark.parametrize("w,h,sigma", [(67, 35, 1.5), (256, 16, 1.0), (521, 300, 1.5), (512, 512, 3.0), (261, 70, 10.0)])
def test_unsharp_mask(nl, w, h, sigma):
    for kind, data in (("calm", calm(w, h)), ("sky", sky(w, h))):
        taps, blurred = blurred_ref(w, h, sigma, kind)
        for what, gain, lo, hi, thr in usm_cases(data):
            want = ref.apply_unsharp_mask(data, blurred, gain, lo, hi, thr)
            got = nl.unsharp_mask(data, w, h, sigma, gain, lo, hi, thr)
            assert same(got, want), "%s, %s: %s" % (kind, what, first_diff(got, want))
        if kind == "calm":
            want = ref.apply_unsharp_mask(data, blurred, 1.5, 0, 1, np.median(data[np.isfinite(data)]))
            assert not same(want, data) and (want == data)[np.isfinite(data)].any()     # sharpened here, copied there


def test_unsharp_mask_direct_path(nl):
    # a radius beyond both staging limits under the epilogue: sigma 20 has 93 taps
    w, h = 261, 70
    taps = nl.gaussian_kernel_1d(20.0)
    assert nl.blur_tap_paths(taps.size) == (False, False) and taps.size // 2 <= h
    data = calm(w, h)
    want = ref.unsharp_mask(data, w, 20.0, 1.5, 0.0, 1.0, 0.2, kernel=taps)
    got = nl.unsharp_mask(data, w, h, 20.0, 1.5, 0.0, 1.0, 0.2)
    assert same(got, want), first_diff(got, want)


def test_guards_leave_every_bit(nl):
    w, h = 67, 35
    data = sky(w, h)
    assert same(nl.gaussian_blur(data, w, h, 0.0), data)
    assert same(nl.gaussian_blur(data, w, h, -0.0), data)
    assert same(nl.unsharp_mask(data, w, h, 0.0, 1.0, 0.0, 1.0, 0.0), data)
    assert same(nl.unsharp_mask(data, w, h, 1.5, 0.0, 0.0, 1.0, 0.0), data)
    with nl.StackHandle(1, w, h, device=0) as st:
        st.upload_frame(0, data)
        st.frame_gaussian_blur(0, 0.0)
        st.frame_unsharp_mask(0, 0.0, 1.0, 0.0, 1.0, 0.0)
        st.frame_unsharp_mask(0, 1.5, 0.0, 0.0, 1.0, 0.0)
        assert np.array_equal(st.download_tile(0).view(np.uint32), data.view(np.uint32))


@pytest.mark.parametrize("w,h,sigma", [(67, 35, 1.5), (521, 300, 2.0), (261, 70, 20.0)])
def test_resident_slot_equals_host(nl, w, h, sigma):
    data = sky(w, h)
    blur = nl.gaussian_blur(data, w, h, sigma)
    usm = nl.unsharp_mask(data, w, h, sigma, 1.5, -10.0, 2000.0, 990.0)
    assert not same(blur, usm)
    sentinel = np.arange(w * h, dtype=np.float32)
    with nl.StackHandle(5, w, h, device=0) as st:
        for i, frame in enumerate((sentinel, data, sentinel, data, sentinel)):
            st.upload_frame(i, frame)
        st.frame_gaussian_blur(1, sigma)
        st.frame_unsharp_mask(3, sigma, 1.5, -10.0, 2000.0, 990.0)
        assert same(st.download_tile(1), blur)
        assert same(st.download_tile(3), usm)
        for i in (0, 2, 4):
            assert np.array_equal(st.download_tile(i), sentinel)


def test_padded_stride_neighbours_and_padding_untouched(nl):
    """Three 512 x 512 slots at the padded stride of such a handle, in a buffer of this test's own filled with random
    bits: after a blur of slot 1 and an unsharp mask of it, only the slot's 512 * 512 floats have changed."""
    import torch
    w = h = 512
    npix = w * h
    data = sky(w, h)
    with nl.StackHandle(3, w, h, device=0) as st:
        stride = st.frame_stride()
        assert stride > npix                                  # a frame of exactly 1 MiB gets the padded stride
        rng = np.random.default_rng(3)
        before = rng.integers(0, 2 ** 32, 3 * stride, dtype=np.uint32)
        before[stride:stride + npix] = data.view(np.uint32)
        buf = torch.from_numpy(before.view(np.int32).copy()).to("cuda:0")
        st.attach_device_frames(buf.data_ptr(), stride)
        st.frame_gaussian_blur(1, 2.0)
        after = buf.cpu().numpy().view(np.uint32)
        want = nl.gaussian_blur(data, w, h, 2.0)
        assert same(after[stride:stride + npix].view(np.float32), want)
        changed = np.flatnonzero(after != before)
        assert changed.size and changed.min() >= stride and changed.max() < stride + npix
        st.frame_unsharp_mask(1, 1.5, 1.0, 0.0, 2000.0, 0.0)
        again = buf.cpu().numpy().view(np.uint32)
        assert same(again[stride:stride + npix].view(np.float32), nl.unsharp_mask(want, w, h, 1.5, 1.0, 0.0, 2000.0, 0.0))
        changed = np.flatnonzero(again != before)
        assert changed.min() >= stride and changed.max() < stride + npix
        st.attach_device_frames(None)


def test_result_forms(nl):
    w, h = 261, 70
    frames = [sky(w, h), calm(w, h) * f32(4000.0)]
    with nl.StackHandle(2, w, h, device=0) as st:
        for call in (lambda: st.result_gaussian_blur(2.0), lambda: st.result_unsharp_mask(1.5, 1.0, 0.0, 1.0, 0.0)):
            with pytest.raises(nl.NlError) as e:              # before any pass
                call()
            assert e.value.code == nl.capi.ERR_INVALID_ARG and "has not run a pass" in str(e.value)
        st.upload_frames(frames)
        res, _, _ = st.run(nl.ST_MEAN, 3.0, 3.0)
        st.result_gaussian_blur(2.0)
        got = st.download_rows(-1, 0, h)
        want = nl.gaussian_blur(res, w, h, 2.0)
        assert same(got, want), first_diff(got, want)
        assert not same(got, res)
        st.result_unsharp_mask(1.5, 2.0, 0.0, 3000.0, 500.0)
        got = st.download_rows(-1, 0, h)
        assert same(got, nl.unsharp_mask(want, w, h, 1.5, 2.0, 0.0, 3000.0, 500.0))
        for i in range(2):                                    # the frames stay
            assert same(st.download_tile(i), frames[i])


def test_row_tile_rejected(nl):
    with nl.StackHandle(2, 256, 256, row0=64, rows=128, device=0) as st:
        st.fill_synthetic(seed=3)
        st.run(nl.ST_MEAN, 3.0, 3.0)
        for call in (lambda: st.frame_gaussian_blur(0, 2.0), lambda: st.frame_unsharp_mask(0, 1.5, 1.0, 0.0, 1.0, 0.0),
                     lambda: st.result_gaussian_blur(2.0), lambda: st.result_unsharp_mask(1.5, 1.0, 0.0, 1.0, 0.0)):
            with pytest.raises(nl.NlError) as e:
                call()
            assert e.value.code == nl.capi.ERR_INVALID_ARG and "whole-image" in str(e.value)


def test_bad_index_and_sigma_on_a_handle(nl):
    with nl.StackHandle(1, 64, 64, device=0) as st:
        for call in (lambda: st.frame_gaussian_blur(1, 2.0), lambda: st.frame_gaussian_blur(-1, 2.0),
                     lambda: st.frame_unsharp_mask(-1, 2.0, 1.0, 0.0, 1.0, 0.0),
                     lambda: st.frame_gaussian_blur(0, float("nan")), lambda: st.frame_gaussian_blur(0, 0.1),
                     lambda: st.frame_gaussian_blur(0, 40.0)):           # radius 93 > 64
            with pytest.raises(nl.NlError) as e:
                call()
            assert e.value.code == nl.capi.ERR_INVALID_ARG
