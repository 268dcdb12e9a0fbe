"""CPU, oracle only: the frames of the deep maps tests (tests/deepmaps_frames.py) are worth testing with.  The GPU tests
(tests/test_gpu_deepmaps.py) compare the deep maps pass with the oracle pixel by pixel; they would pass just as well if the
dominant kernel handed every pixel to the generic pass, so the frames must keep most pixels INSIDE what that kernel's
columns hold, and most pixels must clip something.

"Fits" is a sufficient bound on the oracle's totals, from MlzLayout (stack_fast_mlz_impl.hpp): a pixel stays with the
dominant kernel while the alive window [a, b) of its sorted column keeps a < ZLC = 16 and b > NTOP - ZHC, at most PADS
samples are missing, and no round clips as many samples on a side as the ranks read there (CR = 8 for sigma, 16 for
winsorized clipping).  With the smaller of the two layouts' figures (a stack that fills its lanes: ZHC = 24, PADS = 15):
    missing <= 15,  missing + reject_high < 24,  reject_low < 16,  reject_low < CR and reject_high < CR.
The bound judges totals where the kernel judges rounds, so it is conservative there.  It counts as missing the samples
that are NaN; a stack that does not fill its lanes also misses the frames up to its class (NTOP = n rounded up to a
multiple of 16), against ZHC = 32 and PADS = 23 -- the second share below counts those as well."""
import numpy as np
import pytest

import deepmaps_frames as deep
from nightlight_amd import capi

MODES = {"sigma": capi.ST_SIGMA, "winsor": capi.ST_WINSOR_SIGMA}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("n", [129, 256, 300, 512])
def test_most_pixels_fit_the_columns_and_clip_something(oracle, n, mode):
    t = deep.truth(oracle, n, MODES[mode])
    low, high = t.reject_low.astype(np.int64), t.reject_high.astype(np.int64)
    missing = n - t.coverage.astype(np.int64)
    cr = 16 if mode == "winsor" else 8
    fits = (missing <= 15) & (missing + high < 24) & (low < 16) & (low < cr) & (high < cr)
    # the same with the frames the class pads: NTOP - n more missing samples, against the layout of the class
    ntop = (n + 15) // 16 * 16
    full = ntop in (256, 512)
    short = missing + (ntop - n)
    fits_class = (short <= (15 if full else 23)) & (short + high < (24 if full else 32)) & (low < 16) & (low < cr) & (high < cr)
    clipped = (low + high) > 0
    print("n %d %s: %.1f %% fit (%.1f %% against the class layout), %.1f %% clip something; totals %d / %d"
          % (n, mode, 100.0 * fits.mean(), 100.0 * fits_class.mean(), 100.0 * clipped.mean(), t.clip_low, t.clip_high))
    assert fits.mean() >= 0.85
    assert fits_class.mean() >= 0.85
    assert clipped.mean() >= 0.85
    # the pixels built to leave the columns do, and the special pixels are what they are said to be
    assert not fits[deep.HALF_NAN].any() and not fits_class[deep.HALF_NAN].any()
    assert t.coverage[deep.NO_DATA] == 0 and t.coverage[deep.SINGLE] == 1 and t.coverage[deep.CONSTANT] == n
    assert low[deep.CONSTANT] + high[deep.CONSTANT] == 0
    assert np.all(low + high <= t.coverage)
    fr = deep.frames_of(n)
    assert fr.shape == (n, deep.P) and deep.P % 32 != 0
    assert [int(np.isinf(fr[:, p]).sum()) for p in deep.INF_PIXELS] == [1, 1, 1]
