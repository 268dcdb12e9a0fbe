"""GPU parity of debanding and binning -- OpDebandHoriz / OpDebandVert through nl_deband_* and nl_stack_frame_deband_*,
OpBin through nl_bin_nxn and nl_stack_frame_bin_from -- against the CPU restatement in deband_ref.py.

Bar: the bits of the frame and of the three info fields equal the restatement's; any NaN equals any NaN, and zeros
compare sign-blind (same() as in test_gpu_background.py).  In the parity matrix the restatement returns for every case,
so every case compares frames; where the restatement panics (tested apart), the library returns NL_ERR_INVALID_ARG.
Everything runs in this one pytest process.
"""
import threading

import numpy as np
import pytest

import deband_ref as ref
from test_gpu_background import first_diff, same

pytestmark = pytest.mark.gpu

f32 = np.float32
KINDS = ("sky", "int", "nan")
PERCENTILES = (50.0, 0.001, 25.0, 99.99)     # k = mid, 0, mid and n - 1
SIGMAS = (0.0, 3.0)


def frame(w, h, kind, seed=3):
    """Gaussian sky with a row and a column banding pattern ("sky"); the same integer-valued on a coarse scale, many
    ties ("int"); with NaN blocks that leave every row and column samples, two +Inf and one -Inf ("nan")."""
    rng = np.random.default_rng(seed + 7 * w + h)
    rows = 1.0 + 0.03 * np.sin(np.arange(h) * 0.9) + 0.02 * (np.arange(h) % 2)
    cols = 1.0 + 0.03 * np.cos(np.arange(w) * 0.7) + 0.02 * (np.arange(w) % 2)
    img = (1000.0 + 20.0 * rng.standard_normal((h, w))) * rows[:, None] * cols[None, :]
    if kind == "int":
        img = np.round(img / 8.0)
    img = img.astype(np.float32)
    if kind == "nan":
        y0, x0 = h // 5, w // 4
        img[y0:y0 + max(1, min(3, h // 3)), x0:x0 + max(1, min(5, w // 3))] = np.nan
        img[(3 * h) // 4, (3 * w) // 4] = np.nan
        img[h // 2, w // 3] = np.inf
        img[h // 3, w // 2] = np.inf
        img[h // 2, (2 * w) // 3] = -np.inf
    return img.reshape(-1)


def loc_scale(data):
    d = data[np.isfinite(data)].astype(np.float64)
    med = np.median(d)
    return f32(med), f32(1.4826 * np.median(np.abs(d - med)))


def check(got, want, what=""):
    g_out, g_info = got
    w_out, w_info = want
    for k in ("threshold", "lowest", "highest"):
        assert same([g_info[k]], [w_info[k]]), (what, k, g_info[k], w_info[k])
    assert same(g_out, w_out), "%s frame: %s" % (what, first_diff(g_out, w_out))


# (width, height, "h" / "v", window)
CASES = [(w, h, d, 128) for w, h in ((67, 29), (29, 67), (1024, 768), (4096, 8)) for d in "hv"]
CASES += [(130, 70, d, win) for win in (1, 2, 7, 64, 128, 4096) for d in "hv"]
CASES += [(20000, 5, "h", 128), (5, 20000, "v", 128)]       # more than 16 384 samples per line: the staging path
COMPARED = {}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h,direction,window", CASES)
def test_parity(nl, oracle, w, h, direction, window, kind):
    data = frame(w, h, kind)
    loc, scale = loc_scale(data)
    r, g = (ref.deband_horiz, nl.deband_horiz) if direction == "h" else (ref.deband_vert, nl.deband_vert)
    for p in PERCENTILES:
        for sigma in SIGMAS:
            want = r(data, w, h, p, window, sigma, loc, scale, oracle)      # (a GoPanic here fails the case)
            got = g(data, w, h, p, window, sigma, loc, scale)
            check(got, want, "P %g sigma %g" % (p, sigma))
            assert window == 1 or not same(got[0], data)                    # (window 1: every factor is p / p)
            COMPARED[(w, h, direction, window, kind, p, sigma)] = True


def test_parity_compared_every_case():
    # no case of the matrix above may end in a rejection on both sides: each one compared frames
    assert len(COMPARED) == len(CASES) * len(KINDS) * len(PERCENTILES) * len(SIGMAS) and all(COMPARED.values())


def test_panics_are_invalid_arg(nl, oracle):
    w, h = 67, 29
    data = frame(w, h, "sky")
    loc, scale = loc_scale(data)
    above = data.copy().reshape(h, w)
    above[11, :] = loc + 100 * scale                         # a row entirely above the threshold
    above[:, 5] = loc + 100 * scale                          # and a column
    cases = [(ref.deband_horiz, nl.deband_horiz, above.reshape(-1), 50, 16, 3.0, loc),
             (ref.deband_vert, nl.deband_vert, above.reshape(-1), 50, 16, 3.0, loc),
             (ref.deband_horiz, nl.deband_horiz, data, 50, 16, 3.0, np.nan),      # a NaN threshold
             (ref.deband_vert, nl.deband_vert, data, 50, 16, 3.0, np.nan),
             (ref.deband_vert, nl.deband_vert, data, 50, 0, 0.0, loc),            # vert has no window guard
             (ref.deband_vert, nl.deband_vert, data, 50, -4, 0.0, loc)]
    for r, g, d, p, window, sigma, location in cases:
        with pytest.raises(ref.GoPanic):
            r(d, w, h, p, window, sigma, location, scale, oracle)
        with pytest.raises(nl.NlError) as e:
            g(d, w, h, p, window, sigma, location, scale)
        assert e.value.code == nl.capi.ERR_INVALID_ARG
        assert "banding.go" in str(e.value)


def test_guards_leave_the_frame(nl, oracle):
    w, h = 67, 29
    data = frame(w, h, "nan")
    loc, scale = loc_scale(data)
    calls = [(nl.deband_horiz, ref.deband_horiz, p, win) for p, win in ((0, 16), (100, 16), (-3, 16), (50, 0), (50, -1))]
    calls += [(nl.deband_vert, ref.deband_vert, p, 0) for p in (0, 100, 1e9)]
    for g, r, p, window in calls:
        out, info = g(data, w, h, p, window, 3.0, loc, scale)
        want, winfo = r(data, w, h, p, window, 3.0, loc, scale, oracle)
        assert np.array_equal(out.view(np.uint32), data.view(np.uint32))
        assert info == winfo and info["lowest"] == 1 and info["highest"] == 0
        assert info["threshold"] == f32(loc + f32(f32(3.0) * scale))
    with nl.StackHandle(1, w, h, device=0) as st:
        st.upload_frame(0, data)
        info = st.frame_deband_horiz(0, 50, 0, 0.0)
        assert info == dict(threshold=np.finfo(np.float32).max, lowest=f32(1), highest=f32(0))
        st.frame_deband_vert(0, 100, 16, 0.0)
        assert np.array_equal(st.download_tile(0).view(np.uint32), data.view(np.uint32))


@pytest.mark.parametrize("w,h", [(130, 70), (1024, 768)])
def test_resident_equals_host(nl, w, h):
    data = frame(w, h, "nan")
    loc, scale = loc_scale(data)
    host_h = nl.deband_horiz(data, w, h, 50, 128, 3.0, loc, scale)
    host_v = nl.deband_vert(data, w, h, 25, 7, 0.0)
    with nl.StackHandle(2, w, h, device=0) as st:
        st.upload_frame(0, data)
        st.upload_frame(1, data)
        info_v = st.frame_deband_vert(0, 25, 7, 0.0)
        info_h = st.frame_deband_horiz(1, 50, 128, 3.0, loc, scale)
        out_v, out_h = st.download_tile(0), st.download_tile(1)
    assert np.array_equal(out_h.view(np.uint32), host_h[0].view(np.uint32)) and info_h == host_h[1]
    assert np.array_equal(out_v.view(np.uint32), host_v[0].view(np.uint32)) and info_v == host_v[1]


def test_row_tile_rejected(nl):
    with nl.StackHandle(1, 256, 256, row0=0, rows=128, device=0) as st:
        for call in (st.frame_deband_horiz, st.frame_deband_vert):
            with pytest.raises(nl.NlError) as e:
                call(0, 50, 16, 0.0)
            assert e.value.code == nl.capi.ERR_INVALID_ARG and "whole-image" in str(e.value)
        with nl.StackHandle(1, 128, 64, device=0) as dst:
            with pytest.raises(nl.NlError) as e:
                dst.frame_bin_from(0, st, 0, 2)
            assert e.value.code == nl.capi.ERR_INVALID_ARG and "whole-image" in str(e.value)


def bin_input(w, h, seed=5):
    """Noise with +-1e8 and 1 sprinkled in (1e8 + 1 == 1e8 in fp32: the summation order shows) and a few NaN."""
    rng = np.random.default_rng(seed)
    img = rng.standard_normal(w * h).astype(np.float32)
    pick = rng.random(w * h)
    img[pick < 0.10] = 1e8
    img[(pick >= 0.10) & (pick < 0.20)] = -1e8
    img[(pick >= 0.20) & (pick < 0.30)] = 1.0
    img[rng.integers(0, w * h, 5)] = np.nan
    return img


@pytest.mark.parametrize("w,h", [(67, 29), (256, 256)])
def test_bin(nl, w, h):
    data = bin_input(w, h)
    for n in (1, 2, 3, 4, 7):
        want, ow, oh = ref.bin_nxn(data, w, h, n)
        assert nl.bin_shape(w, h, n) == (ow, oh)
        got, gw, gh = nl.bin_nxn(data, w, h, n)
        assert (gw, gh) == (ow, oh)
        assert same(got, want), "n %d: %s" % (n, first_diff(got, want))
        if n == 2:
            # the order shows in this input: pairwise (tree) summation gives other bits
            img = data.reshape(h, w)[:oh * 2, :ow * 2]
            tree = ((img[0::2, 0::2] + img[1::2, 0::2]) + (img[0::2, 1::2] + img[1::2, 1::2])) * f32(0.25)
            assert not same(tree, want)


def test_bin_rejections(nl):
    data = bin_input(67, 29)
    for n in (30, 68):
        with pytest.raises(nl.NlError) as e:
            nl.bin_nxn(data, 67, 29, n)
        assert e.value.code == nl.capi.ERR_INVALID_ARG and "fits.go" in str(e.value)
        with pytest.raises(nl.NlError):
            nl.bin_shape(67, 29, n)
    with nl.StackHandle(1, 67, 29, device=0) as src, nl.StackHandle(1, 33, 15, device=0) as dst:
        with pytest.raises(nl.NlError) as e:                 # 67 x 29 by 2 is 33 x 14
            dst.frame_bin_from(0, src, 0, 2)
        assert e.value.code == nl.capi.ERR_INVALID_ARG
        with pytest.raises(nl.NlError):
            dst.frame_bin_from(1, src, 0, 2)


def test_resident_chain_into_a_stack_pass(nl, oracle):
    """deband-H, deband-V, frame_affine on a one-frame staging handle of the raw shape, frame_bin_from into the stack
    handle, against the restatements chained; then a 4-frame mean stack of the binned handle against the oracle."""
    w, h, n_frames, n = 262, 134, 4, 2
    ow, oh = ref.bin_shape(w, h, n)
    want = []
    with nl.StackHandle(1, w, h, device=0) as stage, nl.StackHandle(n_frames, ow, oh, device=0) as st:
        for i in range(n_frames):
            data = frame(w, h, "int" if i % 2 else "sky", seed=20 + i)
            loc, scale = loc_scale(data)
            stage.upload_frame(0, data)
            info_h = stage.frame_deband_horiz(0, 50, 128, 3.0, loc, scale)
            info_v = stage.frame_deband_vert(0, 50, 128, 3.0, loc, scale)
            stage.frame_affine(0, 1.5, -0.25)
            st.frame_bin_from(i, stage, 0, n)
            a, winfo_h = ref.deband_horiz(data, w, h, 50, 128, 3.0, loc, scale, oracle)
            b, winfo_v = ref.deband_vert(a, w, h, 50, 128, 3.0, loc, scale, oracle)
            c = (b * f32(1.5) + f32(-0.25)).astype(np.float32)
            d, _, _ = ref.bin_nxn(c, w, h, n)
            assert info_h == winfo_h and info_v == winfo_v
            got = st.download_tile(i)
            assert same(got, d), "frame %d: %s" % (i, first_diff(got, d))
            want.append(d)
        res, _, _ = st.run(nl.ST_MEAN, 3.0, 3.0)
    rc, exp, _, _, _ = oracle.stack_apply(nl.ST_MEAN, np.stack(want), None, 3.0, 3.0)
    assert rc == 0 and same(res, exp)


def test_four_threads(nl):
    w, h = 1024, 768
    data = frame(w, h, "int")
    loc, scale = loc_scale(data)
    want = nl.deband_horiz(data, w, h, 50, 128, 3.0, loc, scale)
    want_v = nl.deband_vert(data, w, h, 50, 128, 3.0, loc, scale)
    results, errors = [None] * 4, []

    def work(i):
        try:
            call = nl.deband_horiz if i % 2 == 0 else nl.deband_vert
            results[i] = call(data, w, h, 50, 128, 3.0, loc, scale)
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    ts = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors
    for i, r in enumerate(results):
        exp = want if i % 2 == 0 else want_v
        assert np.array_equal(r[0].view(np.uint32), exp[0].view(np.uint32)) and r[1] == exp[1]
