"""Known answers for OpBadPixel's Bayer branch and OpDebayer, checked against the CPU restatement in bayer_ref.py:
the reference's own Go tests (badpixels_bayer_test.go, debayer_test.go) restated as data, hand-traced border cases
and the reference's quirks.  Then the CPU-side contract of the new entry points: nl_debayer_shape (host only) for
every CFA and channel, the exports, and NL_ERR_NO_DEVICE from the device entries when no device is present."""
import ctypes
import os

import numpy as np
import pytest

import bayer_ref as ref
from util import bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFAS = ["RGGB", "GRBG", "GBRG", "BGGR"]


# ---- badpixels_bayer_test.go: the 13x11 frame 100 + (i & 3), one hot or cold pixel -----------------------------

def go_test_frame():
    return (100 + (np.arange(13 * 11) & 3)).astype(np.float32)


@pytest.mark.parametrize("channel, pos, value, count", [
    ("R", (2, 2), 500, 1), ("R", (2, 2), 0, 1), ("R", (4, 4), 500, 1), ("R", (4, 4), 0, 1),
    ("R", (3, 2), 500, 0),                                   # row 3 holds no red pixel: untouched
    ("G", (2, 3), 500, 1), ("G", (2, 3), 0, 1), ("G", (3, 2), 500, 1), ("G", (3, 2), 0, 1),
    ("G", (2, 2), 500, 0),                                   # (2, 2) is red: untouched
])
def test_go_cosmetic_correction(oracle, channel, pos, value, count):
    w = 13
    data = go_test_frame()
    i = pos[0] * w + pos[1]
    data[i] = value
    out, removed, _ = ref.correct(oracle, data, w, channel, "RGGB", 3.0, 5.0)
    assert removed == count
    assert (out[i] != value) == (count == 1)


# ---- debayer_test.go: ramps data[i] = sum(0..i), the pass-through positions -------------------------------------

def ramp(w, h):
    return np.cumsum(np.arange(w * h)).astype(np.float32)


def test_go_debayer_red_passes_red_through():
    w, h = 7, 11
    data = ramp(w, h)
    rs, aw, ah = ref.debayer(data, w, "R", "RGGB")
    assert (aw, ah) == (w & ~1, h & ~1) and rs.size == aw * ah
    d, r = data.reshape(h, w), rs.reshape(ah, aw)
    assert bits_equal(r[0::2, 0::2], d[0:ah:2, 0:aw:2])


def test_go_debayer_green_passes_green_through():
    w, h = 11, 13
    data = ramp(w, h)
    gs, aw, ah = ref.debayer(data, w, "G", "RGGB")
    assert (aw, ah) == (w & ~1, h & ~1)
    d, g = data.reshape(h, w), gs.reshape(ah, aw)
    assert bits_equal(g[0::2, 1::2], d[0:ah:2, 1:aw:2])
    assert bits_equal(g[1::2, 0::2], d[1:ah:2, 0:aw:2])


def test_go_debayer_blue_passes_blue_through():
    w, h = 13, 7
    data = ramp(w, h)
    bs, aw, ah = ref.debayer(data, w, "B", "RGGB")
    assert (aw, ah) == (w & ~1, h & ~1)
    d, b = data.reshape(h, w), bs.reshape(ah, aw)
    assert bits_equal(b[1::2, 1::2], d[1:ah:2, 1:aw:2])


# ---- hand-traced ------------------------------------------------------------------------------------------------

def red_grid_frame(grid):
    """6x6 RGGB mosaic whose nine red pixels (even x, even y) hold grid (3x3), the rest 0."""
    f = np.zeros((6, 6), np.float32)
    f[0::2, 0::2] = np.asarray(grid, np.float32)
    return f.reshape(-1)


GRID = [[1, 2, 3], [4, 5, 6], [7, 8, 9]]
# Same-colour medians, QSelectMedianFloat32 on 4 or 6 values at the border (0.5 * (the two middle values)):
#   corner 1 {1 2 4 5} -> 3, edge 2 {1 2 3 4 5 6} -> 3.5, corner 3 -> 4, edge 4 -> 4.5, centre 5 (nine: the network) -> 5,
#   edge 6 -> 5.5, corner 7 -> 6, edge 8 -> 6.5, corner 9 -> 7
GRID_MEDIANS = [3, 3.5, 4, 4.5, 5, 5.5, 6, 6.5, 7]
# deltas -2 -1.5 -1 -0.5 0 0.5 1 1.5 2: row sums -4.5 0 4.5, mean 0; squares sum 15, variance 15/9, std sqrt(5/3)
GRID_STD = np.float32(np.sqrt(np.float64(np.float32(15) / np.float32(9))))


def test_even_count_border_medians(oracle):
    meds = ref.medians(oracle, red_grid_frame(GRID).reshape(6, 6), "R", 0, 0)
    assert [(y, xs.tolist()) for y, xs, _ in meds] == [(0, [0, 2, 4]), (2, [0, 2, 4]), (4, [0, 2, 4])]
    assert np.concatenate([m for _, _, m in meds]).tolist() == GRID_MEDIANS
    # the oracle's median of four values is the mean of the middle two, not an element
    assert oracle.median_f32(np.float32([10, 40, 30, 20])) == np.float32(25)


def test_delta_stats_and_removal_by_hand(oracle):
    out, removed, (mean, std) = ref.correct(oracle, red_grid_frame(GRID), 6, "R", "RGGB", 1.0, 1.0)
    assert mean == 0 and std == GRID_STD
    # |delta| > std = 1.29: -2 -1.5 1.5 2 -> their medians
    assert removed == 4
    assert bits_equal(out, red_grid_frame([[3, 3.5, 3], [4, 5, 6], [7, 6.5, 7]]))


def test_negative_sigma_low_by_hand(oracle):
    # sigma_low -1: the low threshold is +std, so every delta below 1.29 is "bad" -- seven pixels, as the reference
    out, removed, (mean, std) = ref.correct(oracle, red_grid_frame(GRID), 6, "R", "RGGB", -1.0, 5.0)
    assert mean == 0 and std == GRID_STD
    assert removed == 7
    assert bits_equal(out, red_grid_frame([[3, 3.5, 4], [4.5, 5, 5.5], [6, 8, 9]]))


def flat_mosaic(w, h, value=100.0, seed=3):
    rng = np.random.default_rng(seed)
    return (np.float32(value) + rng.integers(0, 4, w * h).astype(np.float32)).astype(np.float32)


def test_bggr_blue_skips_row_and_column_zero(oracle):
    # BGGR blue is at (even x, even y), but the walk starts at (xOff+1, yOff+1) = (2, 2): row 0 and column 0 are
    # neither counted nor corrected
    w, h = 40, 30
    data = flat_mosaic(w, h)
    assert [(y, x0) for y, x0, _ in ref.channel_rows(w, h, "B", 1, 1)][:3] == [(2, 2), (4, 2), (6, 2)]
    for pos in (0, 4, 2 * w):                   # (0, 0), (0, 4), (2, 0)
        d = data.copy()
        d[pos] = 1e6
        out, removed, _ = ref.correct(oracle, d, w, "B", "BGGR", 3.0, 5.0)
        assert out[pos] == np.float32(1e6)
    d = data.copy()
    d[2 * w + 4] = 1e6                          # (4, 2): walked
    out, removed, _ = ref.correct(oracle, d, w, "B", "BGGR", 3.0, 5.0)
    assert removed >= 1 and out[2 * w + 4] != np.float32(1e6)


def test_grbg_green_skips_the_first_green(oracle):
    # GRBG green is at (0, 0), but row 0 of the walk starts at xOff + 1 = 2
    w, h = 40, 30
    data = flat_mosaic(w, h)
    assert [(y, x0) for y, x0, _ in ref.channel_rows(w, h, "G", 1, 0)][:3] == [(0, 2), (1, 1), (2, 2)]
    d = data.copy()
    d[0] = 1e6
    out, _, _ = ref.correct(oracle, d, w, "G", "GRBG", 3.0, 5.0)
    assert out[0] == np.float32(1e6)
    d = data.copy()
    d[2] = 1e6
    out, removed, _ = ref.correct(oracle, d, w, "G", "GRBG", 3.0, 5.0)
    assert removed >= 1 and out[2] != np.float32(1e6)


def test_green_border_uses_the_float32_constant():
    # 4x4 RGGB, box (0, 0): g1 = 3 at (1, 0), g2 = 5 at (0, 1); no left and no upper neighbour, so
    #   g1Left = (2*g1 + sqrt2*g2) * K,  g2Up = (sqrt2*g1 + 2*g2) * K,  out(0, 0) = 0.25 * (g1 + g2 + g1Left + g2Up)
    # sqrt2 = float32(Sqrt2) = 0x1.6a09e6p+0; K = f32(1 / f32(2 + sqrt2)) = 0x1.2bec32p-2 (rounded after every
    # operation, as go/types does for a typed constant), not the once-rounded 0x1.2bec34p-2
    assert ref.SQRT2 == np.float32(float.fromhex("0x1.6a09e6p+0"))
    assert ref.GREEN_K == np.float32(float.fromhex("0x1.2bec32p-2"))
    assert ref.GREEN_K_ONCE == np.float32(float.fromhex("0x1.2bec34p-2"))
    f = np.zeros((4, 4), np.float32)
    f[0, 1], f[1, 0] = 3, 5
    f[0, 3], f[1, 2], f[2, 1], f[3, 0], f[2, 3], f[3, 2] = 3, 5, 3, 5, 3, 5
    out, aw, ah = ref.debayer(f.reshape(-1), 4, "G", "RGGB")
    assert (aw, ah) == (4, 4)
    g1, g2, s = np.float32(3), np.float32(5), ref.SQRT2
    left = (np.float32(2) * g1 + s * g2) * ref.GREEN_K
    up = (s * g1 + np.float32(2) * g2) * ref.GREEN_K
    want = np.float32(0.25) * (g1 + g2 + left + up)
    assert want == np.float32(float.fromhex("0x1.fffffep+1"))          # 3.9999998
    left1 = (np.float32(2) * g1 + s * g2) * ref.GREEN_K_ONCE
    up1 = (s * g1 + np.float32(2) * g2) * ref.GREEN_K_ONCE
    assert np.float32(0.25) * (g1 + g2 + left1 + up1) == np.float32(4)  # the other reading would give 4
    assert out[0] == want


def test_nan_in_the_channel_removes_nothing(oracle):
    w, h = 40, 30
    data = flat_mosaic(w, h)
    data[6 * w + 6] = 1e6
    data[6 * w + 8] = np.nan                 # red, deep inside
    out, removed, (mean, std) = ref.correct(oracle, data, w, "R", "RGGB", 3.0, 5.0)
    assert np.isnan(mean) and np.isnan(std) and removed == 0 and bits_equal(out, data)
    d2 = data.copy()
    d2[6 * w + 8] = data[6 * w + 6 + 4]
    d2[6 * w + 7] = np.nan                   # green only: red is corrected as without it
    _, removed, (mean, std) = ref.correct(oracle, d2, w, "R", "RGGB", 3.0, 5.0)
    assert removed >= 1 and not np.isnan(std)


# ---- nl_debayer_shape (host only) -------------------------------------------------------------------------------

def lib_shape(w, h, channel, cfa):
    from nightlight_amd import capi
    ow, oh = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = capi.load().nl_debayer_shape(w, h, channel.encode(), cfa.encode(), ctypes.byref(ow), ctypes.byref(oh))
    return rc, (ow.value, oh.value), capi.last_error()


@pytest.mark.parametrize("cfa", CFAS)
@pytest.mark.parametrize("channel", ["R", "G", "B"])
@pytest.mark.parametrize("w, h", [(7, 11), (8, 12), (4096, 4096), (4095, 2047), (3, 3)])
def test_debayer_shape(cfa, channel, w, h):
    rc, shape, _ = lib_shape(w, h, channel, cfa)
    assert rc == 0 and shape == ref.debayer_shape(w, h, channel, cfa)
    xo, yo = ref.CFA_OFFSETS[cfa]
    assert shape == ((w - xo) & ~1, (h - yo) & ~1)
    assert lib_shape(w, h, channel.lower(), cfa.lower())[:2] == (0, shape)


def test_debayer_shape_no_debayer_and_errors():
    from nightlight_amd import capi
    import nightlight_amd as nl
    assert lib_shape(7, 5, "", "RGGB")[:2] == (0, (7, 5))
    assert lib_shape(7, 5, "R", "")[:2] == (0, (7, 5))
    assert lib_shape(7, 5, "", "nonsense")[:2] == (0, (7, 5))        # OpDebayer returns before looking at either
    rc, _, msg = lib_shape(7, 5, "R", "RGBG")
    assert rc == capi.ERR_INVALID_ARG and msg == "Unknown CFA value RGBG"
    rc, _, msg = lib_shape(7, 5, "X", "RGGB")
    assert rc == capi.ERR_INVALID_ARG and msg == "Unknown debayering value X"
    rc, _, msg = lib_shape(7, 5, "X", "Rggb")                          # the CFA first
    assert rc == capi.ERR_INVALID_ARG and msg == "Unknown CFA value Rggb"
    for w, h, cfa in ((1, 8, "GRBG"), (2, 8, "BGGR"), (8, 1, "RGGB"), (8, 2, "GBRG"), (1, 1, "RGGB")):
        rc, _, msg = lib_shape(w, h, "G", cfa)
        assert rc == capi.ERR_INVALID_ARG and "empty" in msg, (w, h, cfa)
    assert nl.debayer_shape(4096, 4096, "G", "BGGR") == (4094, 4094)
    with pytest.raises(capi.NlError) as e:
        nl.debayer_shape(8, 8, "Q", "RGGB")
    assert e.value.message == "Unknown debayering value Q"


# ---- the entry points on the CPU side ---------------------------------------------------------------------------

NEW_SYMBOLS = ["nl_debayer_shape", "nl_preprocess_frame_cfa", "nl_stack_upload_frame_cfa"]


def test_library_exports_the_bayer_entry_points():
    from nightlight_amd import capi
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert [s for s in NEW_SYMBOLS if not hasattr(lib, s)] == []
    assert set(NEW_SYMBOLS) <= set(capi.EXPORTS)
    header = open(os.path.join(ROOT, "include", "nlstack.h")).read()
    assert all(s + "(" in header for s in NEW_SYMBOLS)


def test_bayer_front_has_no_cpu_fallback():
    import nightlight_amd as nl
    from nightlight_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a HIP device is visible")
    frame = go_test_frame()
    out = np.empty(12 * 10, np.float32)
    ow, oh, removed, stats = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), (ctypes.c_float * 2)()
    rc = capi.load().nl_preprocess_frame_cfa(None, 0, capi.fptr(frame), 13, 11, b"G", b"RGGB", 3.0, 5.0,
                                             capi.fptr(out), ctypes.byref(ow), ctypes.byref(oh),
                                             ctypes.byref(removed), stats, 0)
    assert rc == capi.ERR_NO_DEVICE
    with pytest.raises(capi.NlError) as e:
        nl.preprocess_frame_cfa(frame, 13, 11, "G")
    assert e.value.code == capi.ERR_NO_DEVICE
    rc = capi.load().nl_stack_upload_frame_cfa(None, 0, capi.fptr(frame), 13, 11, None, b"G", b"RGGB", 3.0, 5.0,
                                               None, None)
    assert rc == capi.ERR_NO_DEVICE
