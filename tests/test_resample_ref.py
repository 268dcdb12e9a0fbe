"""CPU: tests/resample_ref.py, the checker of the bicubic / Lanczos-3 resampling (include/nlstack_resample.h, an
extension), held to the CPU oracle where there is one -- the bilinear kernel, the fallback ring, the set of pixels out
of bounds -- to the properties the definition promises (exact integer shifts, the clamp's range), to the library's
Lanczos-3 table, and to the reason the kernels exist: on a band-limited image each is at least twice as accurate as the
one before it."""
import numpy as np
import pytest

import resample_ref as rr
from util import same_values

SHAPES, transform, TRANSFORMS, BEST_POSSIBLE = rr.cases()
WIDE = (rr.BICUBIC, rr.LANCZOS3)


def sources(sw, sh, seed):
    from test_gpu_project_resident import sources as base_sources
    return base_sources(sw, sh, seed)


@pytest.fixture(scope="module")
def table():
    import nightlight_amd as nl
    t = nl.lanczos3_table()
    t.flags.writeable = False
    return t


def test_the_table_is_the_definition(table):
    want = rr.lanczos3_table()
    assert table.shape == (rr.PHASES, 6) and table.dtype == np.float32
    assert np.array_equal(table[0].view(np.uint32), np.array([0, 0, 1, 0, 0, 0], np.float32).view(np.uint32))
    # libm's sin against numpy's: one fp32 ulp per entry at the most
    ulp = np.spacing(np.abs(want))
    assert (np.abs(table.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
    assert (np.abs(table.astype(np.float64).sum(1) - 1.0) <= 2.0 ** -22).all()


@pytest.mark.parametrize("shape", [s for s in SHAPES if s != "7x7"])
def test_bilinear_is_the_oracle(oracle, shape):
    sw, sh, dw, dh = SHAPES[shape]
    for kind, src in enumerate(sources(sw, sh, 4)):
        for name in TRANSFORMS:
            for oob in (np.nan, 123.5):
                rc, want = oracle.project_bilinear(src, sw, sh, dw, dh, transform(shape, name), oob)
                got = rr.resample(src, sw, sh, dw, dh, transform(shape, name), oob, rr.BILINEAR, clamp=bool(kind))
                assert rc == 0 and same_values(got.out, want), (name, kind, oob)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_outside_the_wide_area_every_kernel_is_bilinear(oracle, table, shape):
    sw, sh, dw, dh = SHAPES[shape]
    for kind, src in enumerate(sources(sw, sh, 4)):
        for name in TRANSFORMS:
            trans = transform(shape, name)
            rc, want = oracle.project_bilinear(src, sw, sh, dw, dh, trans, 123.5)
            assert rc == 0
            base = rr.resample(src, sw, sh, dw, dh, trans, 123.5, rr.BILINEAR)
            if name == "all_oob":                                    # the rule of the existing test carries over
                assert not base.ok.any()
            elif (shape, name) in BEST_POSSIBLE:
                assert int(base.ok.sum()) == BEST_POSSIBLE[shape, name]
            else:
                assert 4 * int(base.ok.sum()) >= dw * dh, name
            for kernel in WIDE:
                for clamp in (False, True):
                    got = rr.resample(src, sw, sh, dw, dh, trans, 123.5, kernel, clamp, table)
                    assert np.array_equal(got.ok, base.ok)                      # the same pixels out of bounds
                    assert not (got.wide & ~got.ok).any()
                    ring = ~got.wide
                    assert same_values(got.out[ring], want[ring]), (name, kind, kernel, clamp)
            if shape == "5x3":                                       # no pixel has a wide footprint: all fallback
                assert not any(rr.resample(src, sw, sh, dw, dh, trans, 123.5, k, False, table).wide.any() for k in WIDE)


def test_wide_pixels_of_the_7x7_identity(table):
    src = sources(7, 7, 4)[0]
    wide = {k: rr.resample(src, 7, 7, 7, 7, TRANSFORMS["identity"], np.nan, k, False, table).wide.reshape(7, 7) for k in WIDE}
    want = np.zeros((7, 7), bool)
    want[1:5, 1:5] = True
    assert np.array_equal(wide[rr.BICUBIC], want)                    # 4x4
    want[:] = False
    want[2:4, 2:4] = True
    assert np.array_equal(wide[rr.LANCZOS3], want)                   # 2x2


@pytest.mark.parametrize("shape", ["131x77", "530x80", "7x7"])
def test_integer_shifts_return_the_source_pixels(table, shape):
    sw, sh, dw, dh = SHAPES[shape]
    src = sources(sw, sh, 4)[0]
    w = rr.bicubic_weights(np.zeros(1, np.float32))
    assert [float(v[0]) for v in w] == [0.0, 1.0, 0.0, 0.0] and np.signbit(w[0][0]) and np.signbit(w[3][0])
    assert not np.signbit(w[2][0])
    for name in ("identity", "int_shift"):
        trans = transform(shape, name)
        inv = rr.invert(trans)
        for kernel in WIDE:
            for clamp in (False, True):
                got = rr.resample(src, sw, sh, dw, dh, trans, np.nan, kernel, clamp, table)
                row, col = np.divmod(np.arange(dw * dh), dw)
                at = (row + int(inv[5])) * sw + col + int(inv[2])
                assert got.wide.any()
                assert np.array_equal(got.out[got.ok], src[at[got.ok]]), (name, kernel, clamp)


def test_the_clamp(table):
    sw, sh, dw, dh = SHAPES["131x77"]
    src = sources(sw, sh, 4)[0]
    const = np.full(sw * sh, 1234.5678, np.float32)
    for name in ("subpixel", "small_rot", "shear"):
        trans = transform("131x77", name)
        for kernel in WIDE:
            flat = rr.resample(const, sw, sh, dw, dh, trans, np.nan, kernel, True, table)
            # (wide pixels: on the fallback ring the clamp is a no-op by definition, and the bilinear value of a
            # constant, c * (1 - xr) + c * xr in fp32, is the bilinear projection's, not always c)
            assert flat.wide.any() and (flat.out[flat.wide] == np.float32(1234.5678)).all()
            on = rr.resample(src, sw, sh, dw, dh, trans, np.nan, kernel, True, table)
            off = rr.resample(src, sw, sh, dw, dh, trans, np.nan, kernel, False, table)
            w = on.wide
            assert w.any() and ((on.out[w] >= on.lo[w]) & (on.out[w] <= on.hi[w])).all()
            outside = (off.out[w] < off.lo[w]) | (off.out[w] > off.hi[w])
            assert outside.any(), "the clamp is never exercised"
            assert np.array_equal(on.out[w][~outside], off.out[w][~outside])


def band_limited(sw, sh, seed=8, n=256, band=0.25):
    """(the image on the pixel grid, truth(X, Y) in float64): n plane waves, both frequencies within +-band cycles per pixel"""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-band, band, n), rng.uniform(-band, band, n)
    amp, phase = rng.standard_normal(n), rng.uniform(0, 2 * np.pi, n)

    def truth(X, Y):
        out = np.zeros(X.shape, np.float64)
        for k in range(n):
            out += amp[k] * np.cos(2 * np.pi * (u[k] * X + v[k] * Y) + phase[k])
        return out

    yy, xx = np.mgrid[0:sh, 0:sw].astype(np.float64)
    return truth(xx, yy).astype(np.float32).reshape(-1), truth


def quality_errors(table):
    """relative RMS error of each kernel against the spectrum's truth, over the pixels wide for Lanczos-3"""
    sw, sh = 256, 64
    src, truth = band_limited(sw, sh)
    trans = TRANSFORMS["subpixel"]
    inv = rr.invert(trans)
    row, col = np.divmod(np.arange(sw * sh), sw)
    want = truth(col + np.float64(inv[2]), row + np.float64(inv[5]))
    wide = rr.resample(src, sw, sh, sw, sh, trans, np.nan, rr.LANCZOS3, False, table).wide
    err = {}
    for kernel in (rr.BILINEAR,) + WIDE:
        got = rr.resample(src, sw, sh, sw, sh, trans, np.nan, kernel, False, table).out.astype(np.float64)
        err[kernel] = float(np.sqrt(np.mean((got[wide] - want[wide]) ** 2) / np.mean(want[wide] ** 2)))
    return err, int(wide.sum())


def test_each_kernel_halves_the_error_of_the_one_before(table):
    err, n = quality_errors(table)
    print("relative RMS error over %d wide pixels: bilinear %.4f, bicubic %.4f, Lanczos-3 %.4f; ratios %.2f, %.2f"
          % (n, err[rr.BILINEAR], err[rr.BICUBIC], err[rr.LANCZOS3], err[rr.BILINEAR] / err[rr.BICUBIC],
             err[rr.BICUBIC] / err[rr.LANCZOS3]))
    assert n > 200 * 50
    assert 2 * err[rr.LANCZOS3] <= err[rr.BICUBIC]
    assert 2 * err[rr.BICUBIC] <= err[rr.BILINEAR]
