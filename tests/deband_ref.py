"""CPU restatement of OpDebandHoriz / OpDebandVert (internal/ops/pre/banding.go:61-270) and of fits.NewImageBinNxN
(internal/fits/fits.go:163-195), in fp32 throughout.

Every select goes through the oracle's literal C QSelect* when its input holds no NaN (the samples of a row never do;
a window can, after fixWindowEdge), else through the bounds-checked literal Python select of background_ref (C would
read out of bounds where Go panics).  The window loops run literally.  Where the reference panics, GoPanic is raised."""
import numpy as np

from background_ref import GoPanic, qselect as qselect_lit, qselect_median as qselect_median_lit

f32 = np.float32
MAX_FLOAT32 = np.finfo(np.float32).max


def select(a, k, oracle):
    """QSelectFloat32(a, k) of the fp32 array a."""
    if a.size == 0:
        raise GoPanic("QSelectFloat32 on an empty slice (index 0 out of range [0])")
    if not np.isnan(a).any():
        return oracle.qselect(a, k)[0]
    return f32(qselect_lit([f32(v) for v in a], k))


def select_median(a, oracle):
    """QSelectMedianFloat32(a) of the fp32 array a."""
    if a.size == 0:
        raise GoPanic("QSelectMedianFloat32 on an empty slice (index 0 out of range [0])")
    if not np.isnan(a).any():
        return oracle.qselect_median(a)[0]
    return f32(qselect_median_lit([f32(v) for v in a]))


def threshold_of(sigma, location, scale):
    """banding.go:75-79"""
    if f32(sigma) == 0:
        return MAX_FLOAT32
    return f32(f32(location) + f32(f32(sigma) * f32(scale)))


def go_int(v):
    """int(float32) on amd64 (CVTTSS2SQ): truncation, the minimum int64 for NaN and out of range."""
    v = f32(v)
    if not (v >= f32(-2.0 ** 63) and v < f32(2.0 ** 63)):
        return -2 ** 63
    return int(v)


def line_percentile(line, threshold, percentile, oracle):
    """banding.go:83-92: the percentile of the samples <= threshold of one row / column."""
    samples = line[line <= threshold]
    k = go_int(f32(f32(f32(samples.size) * f32(percentile)) * f32(0.01)))
    return select(samples, k, oracle)


def fix_window_edge(window, missing, oracle):
    """fixWindowEdge (banding.go:134-162) on the fp32 array window, in place."""
    n = window.size
    n_left = n // 2
    left_median = select_median(window[:n_left].copy(), oracle)
    right_median = select_median(window[n_left:].copy(), oracle)
    n_right = n - n_left
    mean_of_medians = f32(f32(0.5) * f32(left_median + right_median))
    center = f32(f32(0.5) * f32(f32(n_left) + f32(n_right)))
    slope_of_medians = f32(f32(right_median - left_median) / center)
    if missing < 0:
        rng = range(n + missing, n)
        base = -n
    else:
        rng = range(0, missing)
        base = n
    for i in rng:
        if i < 0 or i >= n:
            raise GoPanic("fixWindowEdge: index %d out of range [%d]" % (i, n))
        offset = f32(f32(i + base) - center)
        window[i] = f32(mean_of_medians + f32(slope_of_medians * offset))


def factors(pct, window, oracle):
    """banding.go:96-121 / :235-259: (factors, lowest, highest) from the percentiles of all rows / columns."""
    lines = pct.size
    if window < 0:
        raise GoPanic("makeslice: len out of range")
    window = min(window, lines)
    out = np.zeros(lines, np.float32)
    lowest, highest = f32(1), f32(0)
    for i in range(lines):
        start = i - (window >> 1)
        missing = 0
        if start < 0:
            missing = start
            start = 0
        end = start + window
        if end > lines:
            missing = end - lines
            end = lines
            start = end - window
        clone = pct[start:end].copy()
        if missing != 0:
            fix_window_edge(clone, missing, oracle)
        median = select_median(clone, oracle)
        factor = f32(median / pct[i])
        if factor < lowest:
            lowest = factor
        if factor > highest:
            highest = factor
        out[i] = factor
    return out, lowest, highest


def _deband(data, width, height, cols, percentile, window, sigma, location, scale, oracle):
    img = np.array(data, np.float32).reshape(height, width)
    threshold = threshold_of(sigma, location, scale)
    info = dict(threshold=threshold, lowest=f32(1), highest=f32(0))
    percentile = f32(percentile)
    if percentile <= 0 or percentile >= 100 or (not cols and window <= 0):
        return img.reshape(-1), info
    with np.errstate(all="ignore"):
        lines = img.T if cols else img
        pct = np.array([line_percentile(np.ascontiguousarray(l), threshold, percentile, oracle) for l in lines],
                       np.float32)
        fac, info["lowest"], info["highest"] = factors(pct, int(window), oracle)
        out = img * (fac[None, :] if cols else fac[:, None])
    return out.reshape(-1), info


def deband_horiz(data, width, height, percentile, window, sigma, location, scale, oracle):
    """OpDebandHoriz.Apply (banding.go:61-132): (out, info)."""
    return _deband(data, width, height, False, percentile, window, sigma, location, scale, oracle)


def deband_vert(data, width, height, percentile, window, sigma, location, scale, oracle):
    """OpDebandVert.Apply (banding.go:197-270): (out, info)."""
    return _deband(data, width, height, True, percentile, window, sigma, location, scale, oracle)


def bin_shape(width, height, n):
    return (width, height) if n <= 1 else (width // n, height // n)


def bin_nxn(data, width, height, n):
    """OpBin.Apply (preprocess.go:324-331) with NewImageBinNxN (fits.go:163-195): (out, out_width, out_height)."""
    img = np.asarray(data, np.float32).reshape(height, width)
    if n <= 1:
        return img.reshape(-1).copy(), width, height
    ow, oh = bin_shape(width, height, n)
    normalizer = f32(f32(1.0) / f32(n * n))
    total = np.zeros((oh, ow), np.float32)
    with np.errstate(all="ignore"):
        for yoff in range(n):
            for xoff in range(n):
                total = total + img[yoff:yoff + oh * n:n, xoff:xoff + ow * n:n]
        out = total * normalizer
    return out.astype(np.float32).reshape(-1), ow, oh
