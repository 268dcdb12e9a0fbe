"""GPU parity of the colour-camera front -- OpCalibrate, OpBadPixel's Bayer branch, OpDebayer -- through the C ABI
(nl_preprocess_frame_cfa, nl_stack_upload_frame_cfa) against the CPU restatement in bayer_ref.py.

Bar: bit-exact everywhere -- the debayered plane, the removed count, and the bits of the delta mean and std (the
reference's fp32 sums in their fixed order) -- except that any NaN equals any NaN.  Everything runs in this one
pytest process.
"""
import threading

import numpy as np
import pytest

import bayer_ref as ref
import preprocess_ref
from util import bits_equal

pytestmark = pytest.mark.gpu

CFAS = ["RGGB", "GRBG", "GBRG", "BGGR"]
CHANNELS = ["R", "G", "B"]


def mosaic(width, height, seed):
    """A raw one-shot-colour frame: per-colour levels, smooth background, noise, hot and cold pixels."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    level = np.where((yy & 1) == (xx & 1), 1200.0, 900.0) + 100.0 * (yy & 1)
    img = level + 150.0 * np.sin(xx / 37.0) * np.cos(yy / 23.0) + 30.0 * rng.standard_normal((height, width))
    hot = rng.random((height, width)) < 0.002
    img[hot] += 5000.0 * rng.random(np.count_nonzero(hot))
    cold = rng.random((height, width)) < 0.001
    img[cold] -= 900.0 * rng.random(np.count_nonzero(cold))
    return img.astype(np.float32).reshape(-1)


def same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and bits_equal(a[~na], b[~nb])


def check_front(nl, oracle, frame, w, h, channel, cfa, sl=3.0, sh=5.0, dark=None, flat=None, calib=None):
    got = nl.preprocess_frame_cfa(frame, w, h, channel, cfa, calib=calib, sigma_low=sl, sigma_high=sh)
    want = ref.front(oracle, frame, w, h, channel, cfa, sl, sh, dark=dark, flat=flat)
    out, ow, oh, removed, (mean, std) = got
    assert (ow, oh) == (want[1], want[2])
    assert removed == want[3], (removed, want[3])
    assert same([mean, std], list(want[4])), ((mean, std), want[4])
    assert same(out, want[0])
    return got


@pytest.mark.parametrize("w, h", [(9, 7), (10, 8), (67, 29), (1080, 1920), (4096, 4096)])
@pytest.mark.parametrize("cfa", CFAS)
@pytest.mark.parametrize("channel", CHANNELS)
def test_front_matches_reference(nl, oracle, channel, cfa, w, h):
    frame = mosaic(w, h, seed=w * 31 + h)
    _, _, _, removed, _ = check_front(nl, oracle, frame, w, h, channel, cfa)
    if w * h >= 67 * 29:
        assert removed > 0


@pytest.mark.parametrize("cfa", CFAS)
@pytest.mark.parametrize("channel", CHANNELS)
def test_sigma_zero_debayers_only(nl, oracle, channel, cfa):
    frame = mosaic(67, 29, seed=5)
    for sl, sh in ((0.0, 5.0), (3.0, 0.0)):
        out, ow, oh, removed, stats = check_front(nl, oracle, frame, 67, 29, channel, cfa, sl, sh)
        assert removed == 0 and np.isnan(stats[0]) and np.isnan(stats[1])
        assert same(out, ref.debayer(frame, 67, channel, cfa)[0])


def test_negative_sigma_is_the_reference_s(nl, oracle):
    frame = mosaic(67, 29, seed=6)
    _, _, _, removed, _ = check_front(nl, oracle, frame, 67, 29, "G", "RGGB", -0.5, 5.0)
    assert removed > 100


def test_empty_channel_is_preprocess_frame(nl, oracle):
    from nightlight_amd import capi
    frame = mosaic(67, 29, seed=7)
    for sl, sh in ((3.0, 5.0), (0.0, 5.0)):
        out, ow, oh, removed, stats = nl.preprocess_frame_cfa(frame, 67, 29, "", "RGGB", sigma_low=sl, sigma_high=sh)
        mono, mremoved, mstats = nl.preprocess_frame(frame, 67, 29, sigma_low=sl, sigma_high=sh)
        assert (ow, oh) == (67, 29) and removed == mremoved and same(out, mono) and same(stats, mstats)
    with pytest.raises(capi.NlError) as e:
        nl.preprocess_frame_cfa(frame, 67, 29, "", "RGGB", sigma_low=-1.0)
    assert e.value.code == capi.ERR_INVALID_ARG and "negative sigma" in e.value.message


def test_empty_cfa_does_not_debayer(nl, oracle):
    from nightlight_amd import capi
    frame = mosaic(67, 29, seed=8)
    out, ow, oh, removed, stats = nl.preprocess_frame_cfa(frame, 67, 29, "G", "", sigma_low=0.0)
    assert (ow, oh) == (67, 29) and removed == 0 and same(out, frame)
    with pytest.raises(capi.NlError) as e:             # the Bayer branch of OpBadPixel still needs the CFA
        nl.preprocess_frame_cfa(frame, 67, 29, "G", "")
    assert e.value.message == "Unknown CFA value "


@pytest.mark.parametrize("seestar", [False, True])
def test_with_masters(nl, oracle, seestar):
    w, h = 120, 80
    rng = np.random.default_rng(9)
    light = mosaic(w, h, seed=10) + np.float32(300)
    dark = (100 + 10 * rng.random(w * h)).astype(np.float32)
    flat = (0.8 + 0.4 * rng.random(w * h)).astype(np.float32)
    flat[5] = 0
    mw, mh = (h, w) if seestar else (w, h)           # same pixel count, other shape: the masters apply 1-D
    with nl.Calibration(0, mw, mh, dark=dark, flat=flat) as cal:
        for channel, cfa in (("R", "RGGB"), ("G", "GBRG"), ("B", "BGGR")):
            check_front(nl, oracle, light, w, h, channel, cfa, dark=dark, flat=flat, calib=cal)


def adversary(kind, w, h):
    frame = mosaic(w, h, seed=11).reshape(h, w)
    if kind == "hot_column":
        frame[:, 40] += 20000
    elif kind == "hot_row":
        frame[30, :] += 20000
    elif kind == "half_hot":
        frame[0::2, 0::2][:, : w // 4] += 20000       # half of the RGGB red pixels
    elif kind == "nan_channel":
        frame[30, 40] = np.nan                        # red in RGGB, deep inside
    elif kind == "nan_other":
        frame[30, 41] = np.nan                        # green only
        frame[31, 41] = np.nan                        # blue only
    return frame.reshape(-1)


@pytest.mark.parametrize("kind", ["hot_column", "hot_row", "half_hot", "nan_channel", "nan_other"])
def test_adversaries(nl, oracle, kind):
    w, h = 130, 90
    frame = adversary(kind, w, h)
    _, _, _, removed, (mean, std) = check_front(nl, oracle, frame, w, h, "R", "RGGB")
    if kind == "nan_channel":
        assert np.isnan(std) and removed == 0
    else:
        assert not np.isnan(std) and removed > 0


def test_resident_equals_host_form_and_stacks(nl, oracle):
    w, h, n = 301, 203, 8
    ow, oh = nl.debayer_shape(w, h, "G", "GRBG")
    rng = np.random.default_rng(12)
    dark = (50 + 5 * rng.random(w * h)).astype(np.float32)
    raws = [mosaic(w, h, seed=100 + i) for i in range(n)]
    with nl.Calibration(0, w, h, dark=dark) as cal:
        host = [nl.preprocess_frame_cfa(r, w, h, "G", "GRBG", calib=cal) for r in raws]
        with nl.StackHandle(n, ow, oh) as st, nl.StackHandle(n, ow, oh) as st2:
            for i, r in enumerate(raws):
                removed, stats = st.upload_frame_cfa(i, r, w, h, "G", "GRBG", calib=cal)
                assert removed == host[i][3] and same(stats, host[i][4])
                assert same(st.download_tile(i), host[i][0])
                st2.upload_tile(i, host[i][0])
            for mode in (nl.ST_MEAN, nl.ST_SIGMA):
                st.set_exact(True)
                st2.set_exact(True)
                a = st.run(mode, 3.0, 3.0)
                b = st2.run(mode, 3.0, 3.0)
                assert same(a[0], b[0]) and a[1:] == b[1:]


def test_threads_share_one_calibration(nl, oracle):
    w, h = 256, 192
    dark = np.full(w * h, 20.0, np.float32)
    frames = [mosaic(w, h, seed=200 + i) for i in range(4)]
    want = [ref.front(oracle, f, w, h, "B", "RGGB", dark=dark) for f in frames]
    with nl.Calibration(0, w, h, dark=dark) as cal:
        got = [None] * 4
        errors = []

        def work(i):
            try:
                for _ in range(3):
                    got[i] = nl.preprocess_frame_cfa(frames[i], w, h, "B", "RGGB", calib=cal, frame_id=i)
            except Exception as e:          # pragma: no cover - reported below
                errors.append(e)

        threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    assert errors == []
    for g, wnt in zip(got, want):
        assert same(g[0], wnt[0]) and g[3] == wnt[3] and same(g[4], wnt[4])


def test_rejections(nl, oracle):
    from nightlight_amd import capi
    w, h = 67, 29
    raw = mosaic(w, h, seed=13)
    ow, oh = nl.debayer_shape(w, h, "R", "RGGB")
    with nl.StackHandle(1, ow, oh, row0=0, rows=oh // 2) as tile:
        with pytest.raises(capi.NlError) as e:
            tile.upload_frame_cfa(0, raw, w, h, "R", "RGGB")
        assert e.value.code == capi.ERR_INVALID_ARG and "whole-image" in e.value.message
    with nl.StackHandle(1, ow - 2, oh) as wrong:
        with pytest.raises(capi.NlError) as e:
            wrong.upload_frame_cfa(0, raw, w, h, "R", "RGGB")
        assert e.value.code == capi.ERR_INVALID_ARG and "debayers to" in e.value.message
    with nl.StackHandle(1, ow, oh) as st:
        for channel, cfa, msg in (("R", "XXXX", "Unknown CFA value XXXX"), ("Q", "RGGB", "Unknown debayering value Q"),
                                  ("", "RGGB", "needs a channel and a CFA"), ("R", "", "needs a channel and a CFA")):
            with pytest.raises(capi.NlError) as e:
                st.upload_frame_cfa(0, raw, w, h, channel, cfa)
            assert e.value.code == capi.ERR_INVALID_ARG and msg in e.value.message
        with pytest.raises(capi.NlError) as e:      # a light of another shape than the masters
            with nl.Calibration(0, w + 1, h, dark=np.zeros((w + 1) * h, np.float32)) as cal:
                st.upload_frame_cfa(0, raw, w, h, "R", "RGGB", calib=cal)
        assert e.value.message == "0: Light dimensions [67 29] differ from dark dimensions [68 29]"
        removed, _ = st.upload_frame_cfa(0, raw, w, h, "R", "RGGB")      # the handle still works
        assert same(st.download_tile(0), ref.front(oracle, raw, w, h, "R", "RGGB")[0])
    for channel, cfa, msg in (("R", "XXXX", "Unknown CFA value XXXX"), ("Q", "RGGB", "Unknown debayering value Q")):
        for sl in (3.0, 0.0):
            with pytest.raises(capi.NlError) as e:
                nl.preprocess_frame_cfa(raw, w, h, channel, cfa, sigma_low=sl)
            assert e.value.code == capi.ERR_INVALID_ARG and e.value.message == msg
    one_row = mosaic(8, 1, seed=14)
    with pytest.raises(capi.NlError) as e:           # a 0-pixel result (the reference divides by zero)
        nl.preprocess_frame_cfa(one_row, 8, 1, "G", "RGGB")
    assert e.value.code == capi.ERR_INVALID_ARG and "empty" in e.value.message
