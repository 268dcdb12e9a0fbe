"""GPU parity of star detection -- star.FindStars through nl_find_stars, nl_stack_frame_find_stars and
nl_stack_result_find_stars -- against the CPU restatement in stars_ref.py.

Bar: the star count, every field's bits, and the bits of sum_of_shifts and avg_hfr equal the restatement's; any NaN
equals any NaN.  Where the restatement panics, the library returns NL_ERR_INVALID_ARG.  Everything runs in this one
pytest process.
"""
import functools
import threading

import numpy as np
import pytest

import stars_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = [(67, 29), (1080, 1920), (4096, 4096), (6000, 4000)]
RADII = [1, 3, 16, 40]
# (bp_sigma, diff_std): no rejection; a given MedianDiffStats std; nil stats (deviation 1)
BAD_PIXEL = [(0.0, None), (5.0, 12.5), (5.0, None)]


def render(img, x0, y0, peak, sigma, clip=None):
    h, w = img.shape
    r = int(4 * sigma) + 1
    ys, xs = slice(max(0, int(y0) - r), min(h, int(y0) + r + 1)), slice(max(0, int(x0) - r), min(w, int(x0) + r + 1))
    yy, xx = np.mgrid[ys, xs]
    psf = peak * np.exp(-((xx - x0) ** 2 + (yy - y0) ** 2) / (2.0 * sigma * sigma))
    if clip is not None:
        psf = np.minimum(psf, clip)
    img[ys, xs] += psf


@functools.lru_cache(maxsize=None)
def field(width, height, seed, nan_blocks=True, integer=False):
    """A star field: background with gradient and noise, Gaussian stars over three decades of flux, close pairs,
    saturated plateaus, hot pixels, stars touching every edge, NaN blocks away from the stars."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    img = 1000.0 + 0.01 * xx + 0.005 * yy + 10.0 * rng.standard_normal((height, width))
    n_stars = int(min(2000, max(6, width * height // 8000)))
    keep_out = []
    for _ in range(n_stars):
        x0, y0 = rng.uniform(0, width - 1), rng.uniform(0, height - 1)
        peak = 10.0 ** rng.uniform(2.0, 5.0)
        sigma = rng.uniform(0.8, 2.5)
        render(img, x0, y0, peak, sigma, clip=4000.0 if rng.random() < 0.1 else None)   # plateaus: ties
        keep_out.append((x0, y0))
        if rng.random() < 0.1:                                     # a close pair
            x1, y1 = x0 + rng.uniform(-6, 6), y0 + rng.uniform(-6, 6)
            render(img, x1, y1, peak * rng.uniform(0.3, 1.0), sigma)
            keep_out.append((x1, y1))
    for x0, y0 in [(0, 0), (width - 1, height // 2), (width // 2, 0), (width // 3, height - 1), (0, height // 2),
                   (width - 1, height - 1)]:                       # every edge and two corners
        render(img, x0, y0, 3000.0, 1.5)
        keep_out.append((x0, y0))
    hot = rng.integers(0, width * height, max(3, width * height // 20000))
    img.reshape(-1)[hot] += 5000.0
    if integer:
        img = np.round(img)
    img = img.astype(np.float32)
    if nan_blocks:
        pts = np.array(keep_out + [(h % width, h // width) for h in hot.tolist()])
        for _ in range(max(1, width * height // 2000000)):
            bx, by = rng.integers(0, max(1, width - 8)), rng.integers(0, max(1, height - 8))
            d = np.abs(pts[:, 0] - (bx + 4)) + np.abs(pts[:, 1] - (by + 4))
            if d.min() > 120:                                        # far from every star and hot pixel
                img[by:by + 8, bx:bx + 8] = np.nan
    return img.reshape(-1)


def loc_scale(data):
    d = data[~np.isnan(data)].astype(np.float64)
    med = np.median(d)
    return np.float32(med), np.float32(1.4826 * np.median(np.abs(d - med)))


def same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32),
                                                                            b[~nb].view(np.uint32))


def assert_same(got, want):
    stars, shifts, hfr = got
    wstars, wshifts, whfr = want
    w = ref.as_array(wstars)
    assert stars.size == w.size, "n_stars %d vs %d" % (stars.size, w.size)
    assert np.array_equal(stars["index"], w["index"])
    for f in ("value", "x", "y", "mass", "hfr"):
        assert same(stars[f], w[f]), f
    assert same(shifts, wshifts) and same(hfr, whfr), ((shifts, hfr), (wshifts, whfr))


def run_ref(data, width, loc, scale, bp, ds, radius, star_sig=15.0, star_in_out=1.4):
    try:
        return ref.find_stars(data, width, loc, scale, star_sig, bp, star_in_out, radius, ds)
    except ref.GoPanic as e:
        return e


def check(nl, got_fn, want):
    from nightlight_amd import capi
    if isinstance(want, ref.GoPanic):
        with pytest.raises(capi.NlError) as e:
            got_fn()
        assert e.value.code == capi.ERR_INVALID_ARG
        return
    assert_same(got_fn(), want)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("bp,ds", BAD_PIXEL)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_find_stars_matches_reference(nl, shape, bp, ds, radius):
    w, h = shape
    data = field(w, h, 11, nan_blocks=(bp == 0.0 or ds is not None), integer=(radius == 3))
    loc, scale = loc_scale(data)
    want = run_ref(data, w, loc, scale, bp, ds, radius)
    assert not isinstance(want, ref.GoPanic), "the synthetic field should not panic: %s" % want
    if radius in (3, 16) and w * h > 1 << 16:
        assert len(want[0]) > 0
    check(nl, lambda: nl.find_stars(data, w, h, loc, scale, bp_sigma=bp, radius=radius, diff_std=ds), want)


@pytest.mark.parametrize("shape", [(67, 29), (1080, 1920)], ids=lambda s: "%dx%d" % s)
def test_host_resident_and_result_forms_agree(nl, shape):
    w, h = shape
    data = field(w, h, 5)
    loc, scale = loc_scale(data)
    want = run_ref(data, w, loc, scale, 5.0, 12.5, 16)
    host = nl.find_stars(data, w, h, loc, scale, diff_std=12.5)
    assert_same(host, want)
    with nl.StackHandle(1, w, h) as st:
        st.upload_frame(0, data)
        assert_same(st.frame_find_stars(0, loc, scale, diff_std=12.5), want)
        result = st.run(nl.ST_MEAN)[0].reshape(-1)    # (the mean of one frame)
        assert_same(st.result_find_stars(loc, scale, diff_std=12.5),
                    run_ref(result, w, loc, scale, 5.0, 12.5, 16))


def test_cfa_upload_then_find_stars_equals_host_chain(nl):
    rw, rh = 512, 384
    mono = field(rw, rh, 7, nan_blocks=False)
    out, ow, oh, _, _ = nl.preprocess_frame_cfa(mono, rw, rh, "G", "RGGB", sigma_low=3.0, sigma_high=5.0)
    loc, scale = loc_scale(out)
    want = nl.find_stars(out, ow, oh, loc, scale, diff_std=None)
    assert_same(want, run_ref(out, ow, loc, scale, 5.0, None, 16))
    with nl.StackHandle(1, ow, oh) as st:
        st.upload_frame_cfa(0, mono, rw, rh, "G", "RGGB", sigma_low=3.0, sigma_high=5.0)
        got = st.frame_find_stars(0, loc, scale, diff_std=None)
    assert_same(got, (list(map(list, want[0].tolist())), want[1], want[2]))


def test_mono_chain_calibrate_badpixel_find_stars(nl):
    w, h = 640, 480
    light = field(w, h, 9, nan_blocks=False) + np.float32(200.0)
    dark = np.full(w * h, 200.0, np.float32)
    with nl.Calibration(0, w, h, dark=dark) as cal, nl.StackHandle(1, w, h) as st:
        st.upload_frame(0, light)
        st.frame_calibrate(0, cal)
        _, (_, std) = st.frame_badpixel(0, 3.0, 5.0)
        frame = st.download_tile(0)
        loc, scale = loc_scale(frame)
        got = st.frame_find_stars(0, loc, scale, diff_std=std)
    assert_same(got, run_ref(frame, w, loc, scale, 5.0, std, 16))


def test_short_capacity(nl):
    from nightlight_amd import capi
    import ctypes as C
    w, h = 1080, 1920
    data = field(w, h, 5)
    loc, scale = loc_scale(data)
    want = nl.find_stars(data, w, h, loc, scale)
    assert want[0].size > 3
    out = np.zeros(3, capi.STAR_DTYPE)
    n, s, a = C.c_int(0), C.c_float(0), C.c_float(0)
    capi.check(capi.load().nl_find_stars(capi.fptr(data), w, h, float(loc), float(scale), 15.0, 5.0, 1.4, 16,
                                         float("nan"), out.ctypes.data_as(C.c_void_p), 3, C.byref(n), C.byref(s),
                                         C.byref(a), 0))
    assert n.value == want[0].size
    assert out.tobytes() == want[0][:3].tobytes()
    capi.check(capi.load().nl_find_stars(capi.fptr(data), w, h, float(loc), float(scale), 15.0, 5.0, 1.4, 16,
                                         float("nan"), None, 0, C.byref(n), None, None, 0))
    assert n.value == want[0].size


def test_four_threads(nl):
    cases = []
    for seed in range(4):
        w, h = 1080, 1920
        data = field(w, h, 20 + seed)
        loc, scale = loc_scale(data)
        cases.append((data, w, h, loc, scale, nl.find_stars(data, w, h, loc, scale)))
    errors = []

    def work(c):
        data, w, h, loc, scale, want = c
        try:
            for _ in range(3):
                got = nl.find_stars(data, w, h, loc, scale)
                assert got[0].tobytes() == want[0].tobytes() and same(got[1], want[1]) and same(got[2], want[2])
        except Exception as e:    # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(c,)) for c in cases]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_rejections(nl):
    from nightlight_amd import capi
    w, h = 300, 200
    data = field(w, h, 3, nan_blocks=False)
    loc, scale = loc_scale(data)
    with nl.StackHandle(1, w, h, row0=0, rows=100) as st:
        with pytest.raises(capi.NlError) as e:
            st.frame_find_stars(0, loc, scale)
        assert e.value.code == capi.ERR_INVALID_ARG and "whole-image" in str(e.value)
    with nl.StackHandle(1, w, h) as st:
        with pytest.raises(capi.NlError) as e:
            st.result_find_stars(loc, scale)
        assert e.value.code == capi.ERR_INVALID_ARG and "not run a pass" in str(e.value)
    with pytest.raises(capi.NlError) as e:
        nl.find_stars(data, w, h, loc, scale, radius=-1)
    assert e.value.code == capi.ERR_INVALID_ARG
    for bad in (np.inf, -np.inf):
        d = data.copy()
        d[w * h // 2 + 17] = bad
        with pytest.raises(capi.NlError) as e:
            nl.find_stars(d, w, h, loc, scale)
        assert e.value.code == capi.ERR_INVALID_ARG and "Inf" in str(e.value)


def test_radius_zero_finds_nothing(nl):
    w, h = 1080, 1920
    data = field(w, h, 5)
    loc, scale = loc_scale(data)
    stars, shifts, hfr = nl.find_stars(data, w, h, loc, scale, radius=0)
    want = run_ref(data, w, loc, scale, 5.0, None, 0)
    assert stars.size == 0 and len(want[0]) == 0 and np.isnan(hfr)
    assert same(shifts, want[1])


def nan_in_centroid_window():
    w, h = 64, 48
    img = np.full((h, w), 100.0, np.float32)
    img[20, 30] = 5000.0
    img[20, 31] = 3000.0
    img[22, 33] = np.nan            # inside the +-16 window, not a candidate
    return img.reshape(-1), w, h


def centroid_past_last_cell():
    """One 256 x 256 cell: a candidate on the right edge whose 1-D window wraps into an equally bright pixel at the
    start of the next row.  Its centroid lands just below x = 255.5, which fp32 rounds to 255.5: the cell is
    int32(256.0) / 256 = 1, outside the one-cell grid (threshold 175: weights 1000.015625 and 1000)."""
    w, h = 256, 256
    img = np.full((h, w), 100.0, np.float32)
    img[100, 255] = 1175.015625
    img[101, 0] = 1175.0
    return img.reshape(-1), w, h


@pytest.mark.parametrize("case", [nan_in_centroid_window, centroid_past_last_cell])
def test_panic_paths(nl, case):
    from nightlight_amd import capi
    data, w, h = case()
    want = run_ref(data, w, 100.0, 10.0, 0.0, None, 16)
    assert isinstance(want, ref.GoPanic)
    with pytest.raises(capi.NlError) as e:
        nl.find_stars(data, w, h, 100.0, 10.0, bp_sigma=0.0, radius=16)
    assert e.value.code == capi.ERR_INVALID_ARG
    assert ("QPartitionStarsDesc" in str(e.value)) or ("filterOutOverlaps" in str(e.value))
