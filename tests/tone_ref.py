"""CPU restatement of the tone curves of the reference's stretch command (internal/fits/pixelops.go: pfScaleOffset
:123-128, Normalize :143-147, pfGamma :151-157, pfPartialGamma :179-191, pfMidtones :214-229, ShiftBlackToMove :649-660)
and of OpSave's two quantisers (internal/fits/tiff16.go:108-135, writejpg.go:106-131): fp32 step by step on np.float32
arrays and scalars (numpy fuses nothing), np.power on float64 for the powers.

A device pow and Go's math.Pow are both not correctly rounded, so a power close to the midpoint between two fp32 values
may be narrowed to either: near_boundary() marks those pixels, and the inputs of the GPU tests -- defined here so that
the CPU tests can hold them to the cap on such pixels -- are SHAPES x (sky, plain) x the cases below."""
import functools

import numpy as np

f32 = np.float32
f64 = np.float64
FMAX = f64(np.finfo(np.float32).max)

SCALE_OFFSET, NORMALIZE, GAMMA, PARTIAL_GAMMA, MIDTONES, SHIFT_BLACK = range(6)      # NL_TONE_*


def _pow32(x, gg):
    """float32(math.Pow(float64(x), gg)) and the float64 power itself"""
    with np.errstate(all="ignore"):
        p = np.power(np.asarray(x, np.float32).astype(np.float64), f64(gg))
        return p.astype(np.float32), p


def gamma_exponent(g):
    """gg := float64(1.0 / g): the division in fp32, then widened"""
    with np.errstate(all="ignore"):
        return f64(f32(1.0) / f32(g))


def scale_offset(d, scale, offset):
    with np.errstate(all="ignore"):
        return np.asarray(d, np.float32) * f32(scale) + f32(offset)


def normalize_constants(mn, mx):
    with np.errstate(all="ignore"):
        scale = f32(1.0) / (f32(mx) - f32(mn))
        return scale, f32(-f32(mn) * scale)


def normalize(d, mn, mx):
    return scale_offset(d, *normalize_constants(mn, mx))


def gamma(d, g):
    return _pow32(d, gamma_exponent(g))[0]


def partial_gamma_parts(d, lo, hi, g):
    """(touched, dd, the float64 power of dd): the pixels pfPartialGamma changes and what it raises"""
    d, lo, hi = np.asarray(d, np.float32), f32(lo), f32(hi)
    with np.errstate(all="ignore"):
        rescale2 = f32(hi - lo)
        rescale1 = f32(1.0) / rescale2
        touched = (d > lo) & (d < hi)
        dd = (d - lo) * rescale1
    return touched, dd, _pow32(dd, gamma_exponent(g))[1]


def partial_gamma_of_power(p32, lo, hi):
    """from + float32(pow) * rescale2: what pfPartialGamma stores for a touched pixel whose narrowed power is p32"""
    lo, hi = f32(lo), f32(hi)
    with np.errstate(all="ignore"):
        return lo + np.asarray(p32, np.float32) * f32(hi - lo)


def partial_gamma(d, lo, hi, g):
    d = np.asarray(d, np.float32)
    touched, dd, _ = partial_gamma_parts(d, lo, hi, g)
    return np.where(touched, partial_gamma_of_power(_pow32(dd, gamma_exponent(g))[0], lo, hi), d)


def midtones_constants(mid, black):
    mid, black = f32(mid), f32(black)
    with np.errstate(all="ignore"):
        clip_low = f32(black * f32(mid - f32(1.0))) / f32(f32(f32(f32(2.0) * mid) - f32(1.0)) * black - mid)
        return clip_low, f32(1.0) / f32(f32(1.0) - clip_low)


def midtones(d, mid, black):
    d, mid = np.asarray(d, np.float32), f32(mid)
    clip_low, scaler = midtones_constants(mid, black)
    with np.errstate(all="ignore"):
        value = d * f32(mid - f32(1.0)) / (f32(f32(f32(2.0) * mid) - f32(1.0)) * d - mid)
        value = np.where(value < clip_low, f32(0), np.where(value > f32(1), f32(1), value))    # NaN: neither
        return (value - clip_low) * scaler


def shift_black_constants(before, after):
    before, after = f32(before), f32(after)
    with np.errstate(all="ignore"):
        black = f32(after - before) / f32(after - f32(1.0))
        return black, f32(1.0) / f32(f32(1.0) - black)


def shift_black(d, before, after):
    black, scale = shift_black_constants(before, after)
    with np.errstate(all="ignore"):
        x = (np.asarray(d, np.float32) - black) * scale
        # Go's math.Max(0, x): NaN for a NaN, +0 for (+0, -0), 0 for a negative x
        return np.where(np.isnan(x), x, np.where(x > f32(0), x, f32(0)))


def tone(d, kind, *p):
    return {SCALE_OFFSET: scale_offset, NORMALIZE: normalize, GAMMA: gamma, PARTIAL_GAMMA: partial_gamma,
            MIDTONES: midtones, SHIFT_BLACK: shift_black}[kind](d, *p)


def export_parts(d, mn, mx, gamma_):
    """(gray in front of the power, gammaInv)"""
    with np.errstate(all="ignore"):
        scale = f32(1.0) / (f32(mx) - f32(mn))
        gray = (np.asarray(d, np.float32) - f32(mn)) * scale
        gray = np.where(np.isnan(gray) | (gray < 0), f32(0), gray)
        gray = np.where(gray > 1, f32(1), gray)
    return gray.astype(np.float32), gamma_exponent(gamma_)


def export_gray(d, mn, mx, gamma_, bits):
    """The counts of WriteMonoTIFF16 (bits 16) / WriteMonoJPG (bits 8)"""
    assert f32(gamma_) > 0 and bits in (8, 16)              # else the reference converts Inf / NaN to an integer
    gray, gamma_inv = export_parts(d, mn, mx, gamma_)
    if gamma_inv != 1.0:
        gray = _pow32(gray, gamma_inv)[0]
    return np.trunc(gray * f32(65535 if bits == 16 else 255)).astype(np.uint16 if bits == 16 else np.uint8)


def near_boundary(p, ulps=64):
    """The float64 powers p that lie within `ulps` fp64 ulps of the midpoint between two adjacent fp32 values (four
    times the 16 ulps OpenCL allows an fp64 pow): their narrowing to fp32 may go either way."""
    p = np.asarray(p, np.float64)
    with np.errstate(all="ignore"):
        lo = p.astype(np.float32)
        up = p > lo.astype(np.float64)
        other = np.where(up, np.nextafter(lo, f32(np.inf)), np.nextafter(lo, f32(-np.inf)))
        mid = 0.5 * lo.astype(np.float64) + 0.5 * other.astype(np.float64)
        # beyond the largest fp32 the boundary is FMAX + half an ulp of it
        mid = np.where(np.isinf(lo) & np.isfinite(p), np.sign(p) * (FMAX + f64(2.0) ** 103), mid)
        near = np.abs(p - mid) <= ulps * np.spacing(np.abs(p))
    return near & np.isfinite(p) & (p != lo.astype(np.float64))


# ---- the inputs of tests/test_gpu_tone.py ----------------------------------------------------------------------------

# (width, height): no quad at all; a tail of one; odd sizes over several workgroups; the padded slot stride
SHAPES = [(1, 3), (15, 15), (67, 35), (261, 70), (521, 300), (512, 512)]
STATS_SHAPE = (2049, 1024)      # 256 quads into a second grid-stride sweep of 2048 x 256 lanes
GAMMAS = [0.5, 1.5, 2.2, 3.0, 4.99, 0.0, -2.0]
# (from, to): inside the range, and from > to (no pixel qualifies)
PARTIAL_RANGES = [(0.25, 0.95), (0.6, 0.3)]
# (min, max, gamma, bits)
EXPORTS = [(0.0, 1.0, 1.0, 16), (0.0, 1.0, 1.0, 8), (0.05, 0.9, 2.2, 16), (0.05, 0.9, 2.2, 8), (0.1, 0.8, 0.5, 16),
           (0.3, 0.3, 1.0, 16), (0.3, 0.3, 1.5, 8), (0.9, 0.1, 1.0, 16)]


@functools.lru_cache(maxsize=None)
def plain(w, h):
    """A finite [0, 1) sky"""
    img = np.random.default_rng(7 * w + h).random(w * h, dtype=np.float32)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def sky(w, h):
    """A [0, 1) sky with NaN, +-Inf, -0.0, 0.0, negatives and values above 1 sprinkled in (in the smallest frames at
    least one special each as far as the pixels go)."""
    rng = np.random.default_rng(11 * w + h)
    n = w * h
    img = rng.random(n, dtype=np.float32)
    pick = rng.random(n)
    specials = (np.nan, np.inf, -np.inf, -0.0, 0.0, -0.37, 1.0, 1.75, 3e38, -1e-30)
    for i, value in enumerate(specials):
        img[(pick >= 0.006 * i) & (pick < 0.006 * i + 0.005)] = value
    for i, value in enumerate(specials):
        if n > 2 * i + 1:
            img[2 * i + 1] = value
    img.setflags(write=False)
    return img


def frames():
    """(name, width, height, data) of every frame the power tests run on"""
    for w, h in SHAPES:
        yield "plain", w, h, plain(w, h)
        yield "sky", w, h, sky(w, h)


def power_cases():
    """(what, pixels, near) for every power the GPU tests compare: how many pixels the frame has and which of them
    lie near a rounding boundary."""
    for name, w, h, data in frames():
        for g in GAMMAS:
            yield "%s %dx%d gamma %g" % (name, w, h, g), data.size, near_boundary(_pow32(data, gamma_exponent(g))[1])
            for lo, hi in PARTIAL_RANGES:
                touched, _, p = partial_gamma_parts(data, lo, hi, g)
                yield "%s %dx%d partial gamma %g [%g, %g]" % (name, w, h, g, lo, hi), data.size, touched & near_boundary(p)
        for mn, mx, gamma_, bits in EXPORTS:
            gray, gamma_inv = export_parts(data, mn, mx, gamma_)
            if gamma_inv != 1.0:
                yield "%s %dx%d export gamma %g" % (name, w, h, gamma_), data.size, near_boundary(_pow32(gray, gamma_inv)[1])
