"""CPU restatement of OpCalibrate and OpBadPixel (mono) composed from the oracle's exports.

  calibrate   OpCalibrate.Apply  internal/ops/pre/preprocess.go:68-99; Subtract / Divide badpixels.go:107-123,
              the flat's maximum from calcMinMeanMax (stats.go:112-121)
  badpixel    OpBadPixel.Apply, mono branch  preprocess.go:180-195: BadPixelMap badpixels.go:32-51
              (MedianFilter3x3, Stats.StdDev stats.go:134-144), MedianFilterSparse badpixels.go:81-88
              (GatherAndMedian gather.go:26-38 over star.CreateMask(width, 1.5)) walked in index order

numpy's float32 arithmetic is IEEE single precision with correct rounding, as Go's float32.
"""
import math

import numpy as np


def divide(a, b, b_max):
    """Divide (badpixels.go:114-123): b <= 0 keeps a, else (a * bMax) / b in fp32."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    with np.errstate(all="ignore"):
        q = (a * np.float32(b_max)) / b
    return np.where(b <= 0, a, q).astype(np.float32)


def calibrate(oracle, light, dark=None, flat=None):
    """OpCalibrate.Apply on a frame (the masters apply 1-D, like the reference's slices)."""
    x = np.asarray(light, np.float32).reshape(-1).copy()
    if dark is not None:
        x = (x - np.asarray(dark, np.float32).reshape(-1)).astype(np.float32)
    if flat is not None:
        flat = np.asarray(flat, np.float32).reshape(-1)
        x = divide(x, flat, oracle.min_mean_max(flat)[2])
    return x


def diff_stats(oracle, data, width, lanes4=False):
    """tmp = data - MedianFilter3x3(data) and Stats(tmp).Mean(), StdDev() in one of the reference's two orders."""
    data = np.asarray(data, np.float32).reshape(-1)
    tmp = (data - oracle.median_filter_3x3(data, width)).astype(np.float32)
    mean = oracle.min_mean_max(tmp, lanes4=lanes4)[1]
    std = np.float32(math.sqrt(oracle.variance(tmp, mean, lanes4=lanes4)))
    return tmp, np.float32(mean), std


def bad_pixel_map(tmp, std, sigma_low, sigma_high):
    lo = np.float32(-std) * np.float32(sigma_low)
    hi = np.float32(std) * np.float32(sigma_high)
    with np.errstate(invalid="ignore"):
        return np.flatnonzero((tmp < lo) | (tmp > hi))


def _gather_median(oracle, data, i, mask):
    idx = i + mask
    idx = idx[(idx >= 0) & (idx < data.size)]
    return oracle.median_f32(data[idx])


def badpixel(oracle, data, width, sigma_low=3.0, sigma_high=5.0, std=None, lanes4=False):
    """OpBadPixel.Apply (mono).  std: replay with this standard deviation instead of the reference's
    own (e.g. the device's).  Returns (out, removed, (diff_mean, diff_std)); sigma 0: no step, stats None."""
    out = np.asarray(data, np.float32).reshape(-1).copy()
    if sigma_low == 0 or sigma_high == 0:
        return out, 0, None
    tmp, mean, own_std = diff_stats(oracle, out, width, lanes4)
    std = own_std if std is None else np.float32(std)
    bpm = bad_pixel_map(tmp, std, sigma_low, sigma_high)
    mask = oracle.create_mask(width, 1.5)
    for i in bpm:                          # MedianFilterSparse: sequential and in place
        out[i] = _gather_median(oracle, out, int(i), mask)
    return out, int(bpm.size), (mean, std)


def badpixel_one_pass(oracle, data, width, sigma_low, sigma_high):
    """What a naive parallel replacement computes: every bad pixel from the ORIGINAL frame."""
    src = np.asarray(data, np.float32).reshape(-1)
    out = src.copy()
    tmp, _, std = diff_stats(oracle, src, width)
    mask = oracle.create_mask(width, 1.5)
    for i in bad_pixel_map(tmp, std, sigma_low, sigma_high):
        out[i] = _gather_median(oracle, src, int(i), mask)
    return out
