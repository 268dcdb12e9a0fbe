"""CPU checks of the colour steps: the restatement in colour_ref.py against hand-computed vectors, the two host-only
entries of the library against the restatement, NL_ERR_NO_DEVICE from every other new entry when no device is visible,
and the cap on pixels near a rounding boundary for every input of test_gpu_colour.py that goes through a power."""
import ctypes as C

import numpy as np
import pytest

import colour_ref as ref
import tone_ref

f32 = np.float32


def bits(a):
    return np.asarray(a, np.float32).reshape(-1).view(np.uint32)


def test_darkest_block_is_decided_by_summation_order():
    # two 2x2 blocks side by side; row sums first: block 0 = (1e8 + 1) + (-1e8 + 1) = 1e8 + -1e8 = 0 (each 1 is absorbed),
    # block 1 = (0.25 + 0.25) + (0.25 + 0.25) = 1 -> means 0 and 0.25; summed in any order that keeps a 1, block 0 would
    # be 0.25 or 0.5 and lose or tie
    r = np.array([1e8, 1, 0.25, 0.25,
                  -1e8, 1, 0.25, 0.25], np.float32)
    planes = np.stack([r, r, r])
    assert ref.block_mean(r, 4, 0, 0, 2) == f32(0) and ref.block_mean(r, 4, 2, 0, 2) == f32(0.25)
    means = ref.block_means_fast(planes, 4, 2, 2, 0.0)
    assert means.shape == (2, 3) and np.array_equal(means[:, 0], [f32(0), f32(0.25)])
    assert np.array_equal(ref.darkest_block(planes, 4, 2, 2, 0.0), [0, 0, 0])
    # column sums first would give (1e8 + -1e8) + (1 + 1) = 2 -> 0.5
    assert f32(f32(f32(1e8) + f32(-1e8)) + f32(2)) / f32(4) == f32(0.5)


def test_darkest_block_tie_nan_and_no_block():
    w, h = 6, 2
    r = np.array([3, 3, 1, 1, 1, 1,
                  3, 3, 1, 1, 1, 1], np.float32)
    g = np.array([3, 3, 0, 0, 2, 2,
                  3, 3, 0, 0, 2, 2], np.float32)
    b = np.array([3, 3, 2, 2, 0, 0,
                  3, 3, 2, 2, 0, 0], np.float32)
    # blocks 1 and 2 both have l = 1: the first wins
    assert np.array_equal(ref.darkest_block(np.stack([r, g, b]), w, h, 2, 0.0), [1, 0, 2])
    # a NaN block never wins, wherever it stands
    rn = r.copy()
    rn[0] = np.nan
    assert np.array_equal(ref.darkest_block(np.stack([rn, g, b]), w, h, 2, 0.0), [1, 0, 2])
    # all NaN, and a block larger than the image: MaxFloat32
    nan = np.full(w * h, np.nan, np.float32)
    assert np.array_equal(ref.darkest_block(np.stack([nan, nan, nan]), w, h, 2, 0.0), [ref.FMAX] * 3)
    assert np.array_equal(ref.darkest_block(np.stack([r, g, b]), w, h, 3, 0.0), [ref.FMAX] * 3)
    # the grid: int32(float32(w) * border) / block * block, then (w - first) / block * block
    assert ref.block_grid(261, 70, 16, 0.1) == (16, 240, 0, 64)
    assert ref.block_grid(261, 70, 64, 0.45) == (64, 192, 0, 64)
    assert ref.block_grid(15, 15, 4, 0.0) == (0, 12, 0, 12)


def test_block_means_fast_equals_the_loops():
    w, h = 23, 17
    p = np.random.default_rng(2).random((3, w * h), dtype=np.float32) * f32(1000)
    for block, border in ((3, 0.0), (4, 0.1), (5, 0.3)):
        xf, xl, yf, yl = ref.block_grid(w, h, block, border)
        want = [[ref.block_mean(p[c], w, x, y, block) for c in range(3)]
                for y in range(yf, yl, block) for x in range(xf, xl, block)]
        assert np.array_equal(bits(ref.block_means_fast(p, w, h, block, border)), bits(np.array(want, np.float32)))


def _star(index, hfr):
    s = np.zeros(1, ref.STAR_DTYPE)
    s["index"], s["hfr"] = index, hfr
    return s


def test_star_on_the_edge_and_all_clipped():
    w, h = 5, 4
    p = np.stack([np.arange(20, dtype=np.float32), np.arange(20, dtype=np.float32) * f32(2), np.ones(20, np.float32)])
    # HFR 2: hfr = 1.5, hfrR = 2, hfrSq = 1.51^2 = 2.2801: offsets with dx^2 + dy^2 <= 2; at the corner (0, 0) the pixels
    # (0,0) (1,0) (0,1) (1,1) = indices 0 1 5 6
    assert ref.star_sums(p, w, h, 0, 2.0, (100, 100, 100)) == (f32(12), f32(24), f32(4), 4)
    got = ref.mean_star_intensity(p, w, h, _star(0, 2.0), 0.0, 0.0, (100, 100, 100))
    assert np.array_equal(got, [3, 6, 1])
    # clip on red at 6: strict <, pixel 6 drops out
    assert ref.star_sums(p, w, h, 0, 2.0, (6, 100, 100)) == (f32(6), f32(12), f32(3), 3)
    # every pixel clipped: 0 * +Inf = NaN
    assert np.isnan(ref.mean_star_intensity(p, w, h, _star(0, 2.0), 0.0, 0.0, (0, 100, 100))).all()
    # no star, and an empty range: zeros
    assert np.array_equal(ref.mean_star_intensity(p, w, h, _star(0, 2.0)[:0], 0.0, 0.0, (9, 9, 9)), [0, 0, 0])
    three = np.concatenate([_star(0, 2.0)] * 3)
    assert ref.star_range(3, 0.6, 0.6) == (1, 2) and ref.star_range(40, 0.6, 0.6) == (24, 16)
    assert np.array_equal(ref.mean_star_intensity(p, w, h, np.concatenate([three] * 2), 0.6, 0.6, (9, 9, 9)), [0, 0, 0])
    # HFR 0.4: hfr = 0.3, hfrR = int32(0.8) = 0: the centre pixel alone
    assert ref.star_sums(p, w, h, 7, 0.4, (100, 100, 100)) == (f32(7), f32(14), f32(1), 1)


def test_clamp_specials():
    x = np.array([-0.0, np.nan, -3.0, 0.5, 1.0, 7.0, np.inf, -np.inf, 0.0], np.float32)
    got = ref.scale_offset_clamp(np.stack([x, x, x]), (1, 1, 1), (0, 0, 0))[0]
    assert np.isnan(got[1])
    assert np.array_equal(bits(np.delete(got, 1)), bits(np.array([0.0, 0.0, 0.5, 1.0, 1.0, 1.0, 0.0, 0.0], np.float32)))
    # product and sum round separately: 3 * 0.1f + 0.2f
    y = ref.scale_offset_clamp(np.full((3, 1), 0.1, np.float32), (3, 3, 3), (0.2, 0.2, 0.2))[0, 0]
    assert y == f32(f32(3) * f32(0.1)) + f32(0.2)


def test_neutralize_quirk_and_hue_wrap():
    h = np.array([10, 100, 200, 300, 350, np.nan], np.float32)
    c = np.array([0.5, 0.6, 0.7, 0.8, 0.9, 0.4], np.float32)
    l = np.array([0.05, 0.15, 0.25, 0.35, np.nan, 0.01], np.float32)
    p = np.stack([h, c, l])
    # low 0.2, high 0.3: l < 0.2 zeroes c; 0.25, between the bounds, is NOT interpolated (both bounds are .Low)
    got = ref.chroma(p, ref.CHROMA_NEUTRALIZE, 0.2, 0.3)
    assert np.array_equal(bits(got[1]), bits(np.array([0, 0, 0.7, 0.8, 0.9, 0], np.float32)))
    assert np.array_equal(bits(got[0]), bits(h)) and np.array_equal(bits(got[2]), bits(l))
    # from 295 > to 30: wraps; strict at the ends; a NaN hue never matches
    got = ref.chroma(p, ref.CHROMA_FOR_HUES, 295, 30, 0.5)
    assert np.array_equal(bits(got[1]), bits(np.array([0.25, 0.6, 0.7, 0.4, 0.45, 0.4], np.float32)))
    got = ref.chroma(p, ref.CHROMA_FOR_HUES, 100, 300, 4.0)           # 100 and 300 themselves are outside
    assert np.array_equal(bits(got[1]), bits(np.array([0.5, 0.6, 1.0, 0.8, 0.9, 0.4], np.float32)))
    # rotate: l < lthres keeps h, a NaN l goes on to the hue test
    got = ref.chroma(p, ref.ROTATE_HUES, 90, 360, -30.0, 0.2)
    assert np.array_equal(bits(got[0]), bits(np.array([10, 100, 170, 270, 320, np.nan], np.float32)))
    # gamma: below the threshold the bits stay, a NaN l is powered
    got = ref.chroma(p, ref.CHROMA_GAMMA, 2.0, 0.2)
    assert np.array_equal(bits(got[1][:2]), bits(c[:2])) and got[1][4] == f32(np.sqrt(np.float64(f32(0.9))))


def test_rgba_byte_order():
    planes = np.array([[0.25], [0.5], [1.0]], np.float32)
    counts = ref.export_rgb(planes, 0.0, 1.0, 1.0, 16)
    assert counts.tolist() == [[16383, 32767, 65535, 65535]]
    assert ref.rgba64_bytes(counts) == b"\x3f\xff\x7f\xff\xff\xff\xff\xff"
    assert ref.export_rgb(planes, 0.0, 1.0, 1.0, 8).tolist() == [[63, 127, 255, 255]]


@pytest.fixture(scope="module")
def nl():
    import nightlight_amd
    nightlight_amd.capi.load()
    return nightlight_amd


def test_host_only_entries_match_the_restatement(nl):
    rng = np.random.default_rng(4)
    for _ in range(200):
        mins, maxs = rng.random(3, dtype=np.float32), rng.random(3, dtype=np.float32) + f32(1)
        got, want = nl.rgb_normalization(mins, maxs), ref.normalization(mins, maxs)
        assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1])
        v = rng.random((4, 3), dtype=np.float32)
        ga, gb = nl.rgb_balance_coeffs(*v)
        wa, wb = ref.balance_coeffs(*v)
        assert np.array_equal(bits(ga), bits(wa)) and np.array_equal(bits(gb), bits(wb))
    # strict compares from channel 0 on: a NaN in channel 1 is skipped, one in channel 0 stays
    got = nl.rgb_normalization([1.0, np.nan, 0.5], [2.0, np.nan, 3.0])
    assert got[0] == f32(0.5) and got[1] == f32(1) / f32(2.5)
    assert np.isnan(nl.rgb_normalization([np.nan, 0.0, 0.5], [2.0, 1.0, 3.0])[0])
    # equal highlights and shadows: a division by zero, as in Go
    ga, _ = nl.rgb_balance_coeffs((0.1, 0.1, 0.1), (0.1, 0.2, 0.3), (1, 1, 1), (1, 1, 1))
    assert np.isinf(ga[0]) and np.array_equal(bits(ga), bits(ref.balance_coeffs((0.1, 0.1, 0.1), (0.1, 0.2, 0.3), (1, 1, 1), (1, 1, 1))[0]))
    lib = nl.capi.load()
    assert lib.nl_rgb_normalization(None, None, None, None) == nl.capi.ERR_INVALID_ARG
    assert "rgb_normalization" in nl.capi.last_error()


def test_every_other_entry_needs_a_device(nl):
    if nl.capi.device_count() > 0:
        pytest.skip("a device is visible: the no-device contract is checked on CPU-only hosts")
    lib, capi = nl.capi.load(), nl.capi
    planes = (C.c_int * 3)(0, 1, 2)
    three = np.zeros(3, np.float32)
    rgb, out, rep = capi.Rgb(1, 1, 1), capi.Rgb(), capi.RgbBalance()
    img = np.zeros(3 * 16, np.float32)
    raw = np.zeros(16 * 8, np.uint8)
    op = capi.Chroma(0, (C.c_float * 4)(2.0, 0.0, 0.0, 0.0))
    calls = [
        lambda: lib.nl_stack_frame_combine_from(None, 0, None, 0, 0.0, 1.0),
        lambda: lib.nl_stack_rgb_scale_offset_clamp(None, planes, capi.fptr(three), capi.fptr(three), None),
        lambda: lib.nl_stack_rgb_darkest_block(None, planes, 4, 0.0, C.byref(out)),
        lambda: lib.nl_stack_rgb_mean_star_intensity(None, planes, None, 0, 0.0, 0.0, rgb, C.byref(out)),
        lambda: lib.nl_stack_rgb_balance(None, planes, None, 0, 4, 0.0, 0.0, 0.0, rgb, rgb, capi.fptr(three),
                                         capi.fptr(three), C.byref(rep)),
        lambda: lib.nl_rgb_balance(capi.fptr(img), 4, 4, None, 0, 4, 0.0, 0.0, 0.0, rgb, rgb, capi.fptr(three),
                                   capi.fptr(three), C.byref(rep), 0),
        lambda: lib.nl_stack_rgb_chroma(None, planes, C.byref(op)),
        lambda: lib.nl_stack_rgb_export(None, planes, 0.0, 1.0, 1.0, 16, raw.ctypes.data_as(C.c_void_p)),
        lambda: lib.nl_export_rgb(capi.fptr(img), 16, 0.0, 1.0, 1.0, 16, raw.ctypes.data_as(C.c_void_p), 0),
    ]
    for call in calls:
        assert call() == capi.ERR_NO_DEVICE and "no HIP device" in capi.last_error()
    assert not img.any() and not raw.any()


def test_inputs_of_the_gpu_tests():
    for w, h in ref.SHAPES:
        sky = ref.planes("sky", w, h)
        assert sky.shape == (3, w * h) and np.isfinite(ref.planes("plain", w, h)).all()
        if w * h >= 225:
            assert np.isnan(sky).any(axis=1).all() and np.isinf(sky).any(axis=1).all() and (sky < 0).any(axis=1).all()
            assert (bits(sky[0]) == 0x80000000).any() and (sky > 1).any()
        s = ref.stars(w, h)
        assert len(s) == 40 and 0.39 < s["hfr"].min() and s["hfr"].max() <= 9 and (s["index"] < w * h).all()


def test_power_inputs_stay_under_the_cap():
    """at most 1e-3 of a frame's pixels near a rounding boundary, the project's cap (test_tone_ref.py)"""
    cases = list(ref.power_cases())
    assert len(cases) >= 2 * len(ref.SHAPES) * len(ref.CHROMA_GAMMAS)
    for what, pixels, near in cases:
        assert np.count_nonzero(near) <= max(1e-3 * pixels, 0), "%s: %d of %d" % (what, np.count_nonzero(near), pixels)
