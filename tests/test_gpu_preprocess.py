"""GPU parity of OpCalibrate and OpBadPixel (mono) through the C ABI (nl_calib_*, nl_preprocess_frame,
nl_stack_frame_calibrate, nl_stack_frame_badpixel) against the CPU restatement in preprocess_ref.py.

Bars.  Calibrate is elementwise: bit-exact (NaN where the reference has NaN).  The bad-pixel std is an
fp64 sum whose order already differs between the reference's own two paths (pure Go, AVX2 lanes): the
device std must sit within 1 ulp of float32(sqrt(variance)) in both orders, and replaying the
sequential walk with the device's own std must give the device's frame bit for bit and the same count.
Where no difference lies within the 1-ulp threshold band the device must also match the reference run
on its own std outright.  Everything runs in this one pytest process.
"""
import threading

import numpy as np
import pytest

import preprocess_ref as ref
from test_preprocess_ref import KAT_W, kat_frame, kat_want
from util import bits_equal

pytestmark = pytest.mark.gpu


def natural_image(width, height, seed):
    """Smooth background, noise, hot and cold pixels."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    img = 1000.0 + 150.0 * np.sin(xx / 37.0) * np.cos(yy / 23.0) + 30.0 * rng.standard_normal((height, width))
    hot = rng.random((height, width)) < 0.002
    img[hot] += 5000.0 * rng.random(np.count_nonzero(hot))
    cold = rng.random((height, width)) < 0.001
    img[cold] -= 900.0 * rng.random(np.count_nonzero(cold))
    return img.astype(np.float32).reshape(-1)


def same(a, b):
    """bit-exact, except that any NaN equals any NaN (the device's NaN payload is its own)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and bits_equal(a[~na], b[~nb])


def ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def masters(width, height, seed, nan=True):
    rng = np.random.default_rng(seed)
    dark = (50.0 + 5.0 * rng.standard_normal(width * height)).astype(np.float32)
    flat = (0.8 + 0.2 * rng.random(width * height)).astype(np.float32)
    flat[7] = 0.0                      # degenerate flat pixels keep the light's value
    flat[11] = -0.25
    if nan:
        flat[13] = np.nan              # NaN is not <= 0: the pixel becomes NaN (and the bad-pixel std NaN)
    flat[(width * height) // 2] = 1.5  # the maximum
    return dark, flat


# ---- OpCalibrate ----------------------------------------------------------------------------------

@pytest.mark.parametrize("width,height", [(257, 131), (1024, 1024)])
def test_calibrate_matches_reference(nl, oracle, width, height):
    light = natural_image(width, height, 3)
    dark, flat = masters(width, height, 4)
    for d, f in ((dark, None), (None, flat), (dark, flat)):
        with nl.Calibration(0, width, height, dark=d, flat=f) as c:
            if f is not None:
                assert c.flat_max == oracle.min_mean_max(f)[2] == np.float32(1.5)
            got, removed, _ = nl.preprocess_frame(light, width, height, calib=c, sigma_low=0.0)
            assert removed == 0
            assert same(got, ref.calibrate(oracle, light, d, f)), (d is None, f is None)


def test_calibrate_row_tile_and_seestar_shape(nl, oracle):
    width, height, row0, rows = 300, 120, 37, 50
    light = natural_image(width, height, 5)
    dark, flat = masters(width, height, 6)
    want = ref.calibrate(oracle, light, dark, flat)
    with nl.Calibration(0, width, height, dark=dark, flat=flat) as c:
        with nl.StackHandle(1, width, height, row0=row0, rows=rows) as st:
            st.upload_frame(0, light)
            st.frame_calibrate(0, c)
            assert same(st.download_tile(0), want[row0 * width:(row0 + rows) * width])
        # a light of another shape with the same pixel count: the masters apply 1-D (Seestar)
        got, _, _ = nl.preprocess_frame(light, height, width, calib=c, sigma_low=0.0)
        assert same(got, want)


def test_calibrate_dimension_errors(nl):
    from nightlight_amd import capi
    a = np.ones(64 * 32, np.float32)
    with pytest.raises(capi.NlError) as e:
        nl.Calibration(0, 64, 32, dark=a, flat=a, flat_width=32, flat_height=64)
    assert e.value.code == capi.ERR_INVALID_ARG
    assert e.value.message == "dark dimensions [64 32] differ from flat dimensions [32 64]"
    light = np.ones(64 * 64, np.float32)
    for kind in ("dark", "flat"):
        with nl.Calibration(0, 64, 32, **{kind: a}) as c:
            with pytest.raises(capi.NlError) as e:
                nl.preprocess_frame(light, 64, 64, calib=c, frame_id=5)
            assert e.value.code == capi.ERR_INVALID_ARG
            assert e.value.message == "5: Light dimensions [64 64] differ from %s dimensions [64 32]" % kind
    with nl.Calibration(0, 64, 32, dark=a, flat=a) as c:         # both: the dark is checked first
        with pytest.raises(capi.NlError) as e:
            nl.preprocess_frame(light, 64, 64, calib=c, frame_id=2)
        assert e.value.message == "2: Light dimensions [64 64] differ from dark dimensions [64 32]"


# ---- OpBadPixel: exact std, replay, reference ------------------------------------------------------

def check_badpixel(nl, oracle, frame, width, height, sl=3.0, sh=5.0, calib=None, dark=None, flat=None):
    got, removed, (mean, std) = nl.preprocess_frame(frame, width, height, calib=calib, sigma_low=sl, sigma_high=sh)
    src = frame if calib is None else ref.calibrate(oracle, frame, dark, flat)
    orders = [False] + ([True] if (width * height) % 4 == 0 else [])
    for lanes4 in orders:
        tmp, rmean, rstd = ref.diff_stats(oracle, src, width, lanes4)
        assert ulps(mean, rmean) <= 1 and ulps(std, rstd) <= 1, (lanes4, mean, rmean, std, rstd)
    # the sequential walk replayed on the device's std: bit for bit
    want, wremoved, _ = ref.badpixel(oracle, src, width, sl, sh, std=std)
    assert wremoved == removed
    assert bits_equal(got, want), np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8]
    # ... and the reference on its own (AVX2-order where it applies) std, where no diff is within 1 ulp of a threshold
    tmp, _, rstd = ref.diff_stats(oracle, src, width, orders[-1])
    band = []
    for s in (np.nextafter(rstd, np.float32(-np.inf)), rstd, np.nextafter(rstd, np.float32(np.inf))):
        band.append(ref.bad_pixel_map(tmp, s, sl, sh).size)
    assert band[0] == band[1] == band[2], "a diff lies in the 1-ulp threshold band: %r" % band
    rwant, rremoved, _ = ref.badpixel(oracle, src, width, sl, sh, lanes4=orders[-1])
    assert rremoved == removed and bits_equal(got, rwant)
    return got, removed


@pytest.mark.parametrize("width,height", [(67, 29), (1024, 1024), (4096, 4096)])
def test_badpixel_matches_reference(nl, oracle, width, height):
    frame = natural_image(width, height, width + height)
    _, removed = check_badpixel(nl, oracle, frame, width, height)
    assert removed > 0


def test_badpixel_kat_on_the_device(nl):
    got, removed, _ = nl.preprocess_frame(kat_frame(), KAT_W, 6, sigma_low=1.0, sigma_high=1.0)
    assert removed == 7 and bits_equal(got, kat_want())


def test_badpixel_hot_column_row_and_block(nl, oracle):
    width = height = 4096
    frame = natural_image(width, height, 77).reshape(height, width)
    frame[:, 1000] += 20000.0
    frame[2000, :] += 20000.0
    frame[3000:3064, 500:564] += 20000.0
    _, removed = check_badpixel(nl, oracle, frame.reshape(-1), width, height)
    assert removed > 2 * 4094


def test_badpixel_mostly_chained(nl, oracle):
    width = height = 256
    frame = natural_image(width, height, 9)
    got, removed, (_, std) = nl.preprocess_frame(frame, width, height, sigma_low=0.01, sigma_high=0.01)
    assert removed > 0.8 * (width - 2) * (height - 2)
    want, wremoved, _ = ref.badpixel(oracle, frame, width, 0.01, 0.01, std=std)
    assert wremoved == removed and bits_equal(got, want)


def test_badpixel_nan_frame_unchanged(nl):
    frame = natural_image(128, 96, 1)
    frame[5000] = np.nan
    got, removed, (_, std) = nl.preprocess_frame(frame, 128, 96)
    assert removed == 0 and np.isnan(std) and bits_equal(got, frame)


def test_badpixel_sigma_rules(nl):
    from nightlight_amd import capi
    frame = natural_image(64, 64, 2)
    got, removed, stats = nl.preprocess_frame(frame, 64, 64, sigma_low=0.0, sigma_high=5.0)
    assert removed == 0 and bits_equal(got, frame) and np.isnan(stats[0])
    with pytest.raises(capi.NlError) as e:
        nl.preprocess_frame(frame, 64, 64, sigma_low=-1.0, sigma_high=5.0)
    assert e.value.code == capi.ERR_INVALID_ARG


# ---- resident form vs host form, concurrency --------------------------------------------------------

def test_resident_equals_host_form(nl, oracle):
    from nightlight_amd import capi
    width, height = 1031, 517
    light = natural_image(width, height, 12)
    dark, flat = masters(width, height, 13, nan=False)
    with nl.Calibration(0, width, height, dark=dark, flat=flat) as c:
        want, wremoved, wstats = nl.preprocess_frame(light, width, height, calib=c)
        with nl.StackHandle(2, width, height) as st:
            st.upload_frame_fits(1, np.frombuffer(light.astype(">f4").tobytes(), np.uint8), -32)
            st.frame_calibrate(1, c)
            removed, stats = st.frame_badpixel(1, 3.0, 5.0)
            assert removed == wremoved and stats == wstats
            assert bits_equal(st.download_tile(1), want)
        with nl.StackHandle(1, width, height, row0=0, rows=100) as tile:
            with pytest.raises(capi.NlError) as e:
                tile.frame_badpixel(0, 3.0, 5.0)
            assert e.value.code == capi.ERR_INVALID_ARG
        check_badpixel(nl, oracle, light, width, height, calib=c, dark=dark, flat=flat)


def test_concurrent_calls_share_one_calibration(nl, oracle):
    width = height = 2048
    frames = [natural_image(width, height, 100 + k) for k in range(8)]
    dark, flat = masters(width, height, 14, nan=False)
    results = {}
    errors = []
    with nl.Calibration(0, width, height, dark=dark, flat=flat) as c:
        def worker(t):
            try:
                for k in range(8):
                    j = (k + 2 * t) % 8
                    results[(t, j)] = nl.preprocess_frame(frames[j], width, height, calib=c, frame_id=j)
            except Exception as e:              # pragma: no cover - reported below
                errors.append(e)
        threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
    assert not errors, errors
    assert len(results) == 32
    for j in range(8):
        src = ref.calibrate(oracle, frames[j], dark, flat)
        got, removed, (_, std) = results[(0, j)]
        want, wremoved, _ = ref.badpixel(oracle, src, width, 3.0, 5.0, std=std)
        assert removed == wremoved and bits_equal(got, want)
        for t in range(1, 4):
            assert results[(t, j)][1] == removed and bits_equal(results[(t, j)][0], got)
