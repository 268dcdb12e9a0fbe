"""CPU restatement of internal/ops/stretch/usm.go -- reflect, GaussianKernel1D, Convolve1DX / Convolve1DY, GaussFilter2D,
ApplyUnsharpMask, UnsharpMask -- in fp32 throughout.

The arrays are vectorised over pixels; the tap loop runs sequentially from i = -k, so every multiply and every add is a
separate fp32 operation in the reference's order (sum starts at float32(0), which decides the sign of a zero).  The
taps follow the reference's fp32 / fp64 steps with math.erf for Go's math.Erf.  Where the reference panics, loops
forever or reads a neighbouring row, GoPanic is raised."""
import math

import numpy as np

from background_ref import GoPanic

f32 = np.float32
SQRT2 = f32(math.sqrt(2.0))                      # const sqrt2 float32 = float32(math.Sqrt2)
MAX_RADIUS = 65536                               # where the library ends the radius search, too


def reflect(size, x):
    """usm.go:25-33 on an integer array"""
    x = np.asarray(x)
    return np.where(x < 0, -x - 1, np.where(x >= size, 2 * size - x - 1, x))


def gaussian_definite_integral(mu, sigma, x):
    """usm.go:36-38"""
    arg = f32(f32(x - mu) / f32(SQRT2 * sigma))
    return f32(f32(0.5) * f32(f32(1) + f32(math.erf(float(arg)))))


def gaussian_kernel_1d(sigma):
    """usm.go:41-82"""
    sigma = f32(sigma)
    mu = f32(0)
    if not sigma > 0 or np.isinf(sigma):
        raise GoPanic("GaussianKernel1D: the radius search does not end (or divides 0 by 0) for sigma %r" % sigma)
    accept_out = f32(0.01)
    radius = 0
    while True:
        val = gaussian_definite_integral(mu, sigma, f32(f32(-0.5) - f32(radius)))
        if val < accept_out:
            radius -= 1
            break
        radius += 1
        if radius > MAX_RADIUS:
            raise GoPanic("GaussianKernel1D: radius beyond %d" % MAX_RADIUS)
    if radius < 0:
        raise GoPanic("makeslice: len out of range")
    kernel = np.zeros(2 * radius + 1, np.float32)

    total = f32(0)
    lower = gaussian_definite_integral(mu, sigma, f32(f32(-0.5) - f32(radius)))
    for i in range(radius + 1):
        upper = gaussian_definite_integral(mu, sigma, f32(f32(f32(-0.5) - f32(radius)) + f32(i + 1)))
        delta = f32(upper - lower)
        kernel[i] = delta
        total = f32(total + delta)
        lower = upper
    for i in range(1, radius + 1):
        value = kernel[radius - i]
        kernel[radius + i] = value
        total = f32(total + value)
    factor = f32(f32(1.0) / total)
    return (kernel * factor).astype(np.float32)


def _taps(kernel, size):
    kernel = np.asarray(kernel, np.float32)
    if kernel.size < 1 or kernel.size % 2 == 0:
        raise GoPanic("index out of range: kernel[i+k] with %d taps" % kernel.size)
    if kernel.size // 2 > size:
        raise GoPanic("one reflect leaves [0, %d) at radius %d" % (size, kernel.size // 2))
    return kernel


def convolve_1d_x(data, width, kernel):
    """usm.go:85-98: data flat, height = len(data) / width"""
    kernel = _taps(kernel, width)
    k = kernel.size // 2
    img = np.asarray(data, np.float32).reshape(-1, width)
    x = np.arange(width)
    total = np.zeros_like(img)
    with np.errstate(all="ignore"):
        for i in range(-k, k + 1):
            total = total + img[:, reflect(width, x + i)] * kernel[i + k]
    return total.reshape(-1)


def convolve_1d_y(data, width, kernel):
    """usm.go:101-114"""
    img = np.asarray(data, np.float32).reshape(-1, width)
    height = img.shape[0]
    kernel = _taps(kernel, height)
    k = kernel.size // 2
    y = np.arange(height)
    total = np.zeros_like(img)
    with np.errstate(all="ignore"):
        for i in range(-k, k + 1):
            total = total + img[reflect(height, y + i), :] * kernel[i + k]
    return total.reshape(-1)


def convolve_separable(data, width, kernel):
    """GaussFilter2D (usm.go:118-122) with the caller's kernel"""
    _taps(kernel, np.asarray(data).size // width)
    return convolve_1d_y(convolve_1d_x(data, width, kernel), width, kernel)


def gaussian_blur(data, width, sigma):
    """OpGaussianBlur.Apply (stretch.go:368-376): the operator's guard, then GaussianBlur (usm.go:126-130)"""
    if f32(sigma) == 0:
        return np.asarray(data, np.float32).copy()
    return convolve_separable(data, width, gaussian_kernel_1d(sigma))


def apply_unsharp_mask(data, blurred, gain, lo, hi, abs_threshold):
    """usm.go:134-149"""
    d = np.asarray(data, np.float32)
    gain, lo, hi, abs_threshold = f32(gain), f32(lo), f32(hi), f32(abs_threshold)
    with np.errstate(all="ignore"):
        r = d + (d - blurred) * gain
        r = np.where(r < lo, lo, r)
        r = np.where(r > hi, hi, r)
        return np.where(d < abs_threshold, d, r).astype(np.float32)


def unsharp_mask(data, width, sigma, gain, lo, hi, abs_threshold, kernel=None):
    """OpUnsharpMask.Apply's guard (stretch.go:414), then UnsharpMask (usm.go:153-159); kernel: taps to use instead of
    GaussianKernel1D(sigma)"""
    if f32(sigma) == 0 or f32(gain) == 0:
        return np.asarray(data, np.float32).copy()
    kernel = gaussian_kernel_1d(sigma) if kernel is None else kernel
    return apply_unsharp_mask(data, convolve_separable(data, width, kernel), gain, lo, hi, abs_threshold)
