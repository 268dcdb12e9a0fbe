"""CPU restatement of the steps of the reference's rgb / lrgb command whose arithmetic is written out in its own source
(internal/fits/rgb.go:43-281: NewRGBFromChannels, getCommonNormalizationFactors, SetBlackWhitePoints, setBlackWhitePoints,
findDarkestBlock, meanStarIntensity; internal/fits/pixelops.go:441-550 and :679-692: the chroma and hue pixel functions
and ScaleOffsetClampRGB; internal/fits/tiff16.go:45-91, writejpg.go:43-89: the colour export): fp32 step by step on
np.float32 scalars and arrays (numpy fuses nothing), explicit loops where the order of a sum matters, np.power on
float64 for the two powers.  It also defines the inputs of tests/test_gpu_colour.py, so that test_colour_ref.py can hold
the ones that go through a power to the cap on pixels near a rounding boundary (tone_ref.near_boundary)."""
import functools

import numpy as np

import tone_ref

f32 = np.float32
FMAX = np.finfo(np.float32).max
CHROMA_GAMMA, CHROMA_NEUTRALIZE, CHROMA_FOR_HUES, ROTATE_HUES = range(4)      # NL_CHROMA_* / NL_ROTATE_HUES
INT32_MIN = -2 ** 31
# star.Star (findstars.go:30-37), as capi.STAR_DTYPE
STAR_DTYPE = np.dtype([("index", "<i4"), ("value", "<f4"), ("x", "<f4"), ("y", "<f4"), ("mass", "<f4"), ("hfr", "<f4")])


def go_i32(x):
    """Go's float32 -> int32 on amd64: truncation, 0x80000000 for NaN or out of range"""
    x = float(x)
    return int(x) if -2147483648.0 <= x < 2147483648.0 else INT32_MIN


def go_int(x):
    """Go's float32 -> int (64 bits)"""
    x = float(x)
    return int(x) if -9223372036854775808.0 <= x < 9223372036854775808.0 else -2 ** 63


def go_div(a, b):
    """Go's integer division: truncation"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def go_clamp01(x):
    """float32(math.Max(math.Min(1, float64(x)), 0)) = float32(math.Max(0, math.Min(1, float64(x)))): NaN for a NaN,
    1 above 1, +0 for -0 and every negative x"""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        return np.where(np.isnan(x), x, np.where(x > f32(1), f32(1), np.where(x > f32(0), x, f32(0)))).astype(np.float32)


# ---- combine (rgb.go:43-78) ------------------------------------------------------------------------------------------

def normalization(mins, maxs):
    mn, mx = f32(mins[0]), f32(maxs[0])
    for c in (1, 2):
        if f32(mins[c]) < mn:
            mn = f32(mins[c])
        if f32(maxs[c]) > mx:
            mx = f32(maxs[c])
    with np.errstate(all="ignore"):
        return mn, f32(1.0) / (mx - mn)


def combine(d, mn, mult):
    with np.errstate(all="ignore"):
        return ((np.asarray(d, np.float32) - f32(mn)) * f32(mult)).astype(np.float32)


# ---- balance (rgb.go:94-281, pixelops.go:679-692) --------------------------------------------------------------------

def scale_offset_clamp(planes, alpha, beta):
    """planes: (3, n).  Returns the clamped copy."""
    with np.errstate(all="ignore"):
        return np.stack([go_clamp01(f32(alpha[c]) * np.asarray(planes[c], np.float32) + f32(beta[c])) for c in range(3)])


def balance_coeffs(cur_shadows, cur_highlights, target_shadows, target_highlights):
    cs, ch, ts, th = [[f32(v) for v in t] for t in (cur_shadows, cur_highlights, target_shadows, target_highlights)]
    with np.errstate(all="ignore"):
        new_shadow = (cs[0] + cs[1] + cs[2]) / f32(3)
        ns = [ts[c] * new_shadow for c in range(3)]
        new_highlight = (ch[0] + ch[1] + ch[2]) / f32(3)
        nh = [th[c] * new_highlight for c in range(3)]
        alpha = [(nh[c] - ns[c]) / (ch[c] - cs[c]) for c in range(3)]
        beta = [ns[c] - alpha[c] * cs[c] for c in range(3)]
    return np.array(alpha, np.float32), np.array(beta, np.float32)


def block_grid(width, height, block, border):
    """(xBlockFirst, xBlockLast, yBlockFirst, yBlockLast) in the reference's int32 / float32 arithmetic"""
    with np.errstate(all="ignore"):
        xf = go_div(go_i32(f32(width) * f32(border)), block) * block
        yf = go_div(go_i32(f32(height) * f32(border)), block) * block
    return xf, go_div(width - xf, block) * block, yf, go_div(height - yf, block) * block


def _ordered_sum(values):
    s = f32(0)
    for v in values:
        s = f32(s + v)
    return s


def block_mean(plane, width, x, y, block):
    """one channel's mean of the block at (x, y): row sums left to right, added top to bottom, times 1 / block^2"""
    with np.errstate(all="ignore"):
        inv = f32(1.0) / f32(block * block)
        rows = [_ordered_sum(plane[x + width * yy:x + width * yy + block]) for yy in range(y, y + block)]
        return f32(_ordered_sum(rows) * inv)


def block_means_fast(planes, width, height, block, border):
    """every visited block's (r, g, b), row-major, (n, 3): the same order of additions, vectorised over the blocks"""
    xf, xl, yf, yl = block_grid(width, height, block, border)
    nbx, nby = max(0, (xl - xf) // block), max(0, (yl - yf) // block)
    if xf < 0 or yf < 0 or nbx == 0 or nby == 0:
        return np.zeros((0, 3), np.float32)
    out = np.zeros((nby * nbx, 3), np.float32)
    with np.errstate(all="ignore"):
        inv = f32(1.0) / f32(block * block)
        for c in range(3):
            img = np.asarray(planes[c], np.float32).reshape(height, width)[yf:yf + nby * block, xf:xf + nbx * block]
            b = img.reshape(nby, block, nbx, block)
            row = np.zeros((nby, block, nbx), np.float32)
            for i in range(block):
                row = row + b[:, :, :, i]
            tot = np.zeros((nby, nbx), np.float32)
            for r in range(block):
                tot = tot + row[:, r, :]
            out[:, c] = (tot * inv).reshape(-1)
    return out


def darkest_scan(means):
    mn = [f32(FMAX)] * 3
    l_min = f32(FMAX)
    with np.errstate(all="ignore"):
        for r, g, b in means:
            l = (f32(r) + f32(g) + f32(b)) / f32(3)
            if l < l_min:
                mn, l_min = [f32(r), f32(g), f32(b)], l
    return np.array(mn, np.float32)


def darkest_block(planes, width, height, block, border):
    return darkest_scan(block_means_fast(planes, width, height, block, border))


def star_range(n, skip_bright, skip_dim):
    with np.errstate(all="ignore"):
        return go_int(f32(n) * f32(skip_bright)), n - go_int(f32(n) * f32(skip_dim))


def star_sums(planes, width, height, index, hfr_field, clip):
    """(r, g, b, pixels) of one star's disc in the reference's loop order"""
    index, clip = int(index), [f32(v) for v in clip]
    star_x = index - go_div(index, width) * width
    star_y = go_div(index, width)
    with np.errstate(all="ignore"):
        hfr = f32(hfr_field) * f32(0.75)
        hfr_r = go_i32(hfr + f32(0.5))
        t = hfr + f32(0.01)
        hfr_sq = t * t
    sr = sg = sb = f32(0)
    pixels = 0
    for off_y in range(-hfr_r, hfr_r + 1):
        y = star_y + off_y
        if not 0 <= y < height:
            continue
        for off_x in range(-hfr_r, hfr_r + 1):
            x = star_x + off_x
            if not 0 <= x < width:
                continue
            if f32(off_x * off_x + off_y * off_y) <= hfr_sq:
                r, g, b = planes[0][y * width + x], planes[1][y * width + x], planes[2][y * width + x]
                if r < clip[0] and g < clip[1] and b < clip[2]:
                    with np.errstate(all="ignore"):
                        sr, sg, sb = f32(sr + r), f32(sg + g), f32(sb + b)
                    pixels += 1
    return sr, sg, sb, pixels


def mean_star_intensity(planes, width, height, stars, skip_bright, skip_dim, clip):
    n = len(stars)
    if n == 0:
        return np.zeros(3, np.float32)
    s0, s1 = star_range(n, skip_bright, skip_dim)
    if s0 >= s1:
        return np.zeros(3, np.float32)
    assert 0 <= s0 and s1 <= n                              # else the reference's slice panics
    tot = [f32(0)] * 3
    pixels = 0
    with np.errstate(all="ignore"):
        for s in stars[s0:s1]:
            r, g, b, k = star_sums(planes, width, height, s["index"], s["hfr"], clip)
            tot = [f32(tot[0] + r), f32(tot[1] + g), f32(tot[2] + b)]
            pixels += k
        norm = f32(1.0) / f32(pixels)
        return np.array([tot[0] * norm, tot[1] * norm, tot[2] * norm], np.float32)


def channel_stats(plane):
    """(min, mean, max) as Stats.Min() / Mean() / Max() give them on NaN-free data"""
    plane = np.asarray(plane, np.float32)
    return f32(plane.min()), f32(np.sum(plane, dtype=np.float64) / plane.size), f32(plane.max())


def set_black_white_points(planes, width, height, stars, block, border, skip_bright, skip_dim, shadows, highlights, loc,
                           scale):
    """SetBlackWhitePoints (rgb.go:94-120).  Returns (balanced planes, report)."""
    with np.errstate(all="ignore"):
        scaled = [f32(loc[c]) + f32(scale[c]) * f32(3) for c in range(3)]
    a1, b1 = balance_coeffs(loc, scaled, shadows, highlights)
    planes = scale_offset_clamp(planes, a1, b1)
    darkest = darkest_block(planes, width, height, block, border)
    with np.errstate(all="ignore"):
        assert not np.isnan(planes).any()                   # (Stats.Max() of a frame with NaN depends on its position)
        clip = [f32(np.max(planes[c])) * f32(0.9) for c in range(3)]
    star_colour = mean_star_intensity(planes, width, height, stars, skip_bright, skip_dim, clip)
    a2, b2 = balance_coeffs(darkest, star_colour, shadows, highlights)
    planes = scale_offset_clamp(planes, a2, b2)
    return planes, {"alpha1": a1, "beta1": b1, "alpha2": a2, "beta2": b2, "darkest": darkest, "stars": star_colour}


# ---- chroma and hue steps (pixelops.go:441-550) on planes (h, c, l) --------------------------------------------------

def hue_in_range(h, lo, hi):
    lo, hi = f32(lo), f32(hi)
    with np.errstate(all="ignore"):
        if lo <= hi:
            return (h > lo) & (h < hi)
        if lo > hi:
            return (h > lo) | (h < hi)
    return np.zeros(np.shape(h), bool)


def chroma_gamma_parts(planes, gamma, threshold):
    """(touched, the float64 power of c): the pixels pf3ChanChroma changes and what it stores before narrowing"""
    with np.errstate(all="ignore"):
        touched = ~(np.asarray(planes[2], np.float32) < f32(threshold))
    return touched, tone_ref._pow32(planes[1], tone_ref.gamma_exponent(gamma))[1]


def chroma(planes, kind, *p):
    """Returns the three planes after the step (a copy)."""
    h, c, l = [np.array(x, np.float32) for x in planes]
    with np.errstate(all="ignore"):
        if kind == CHROMA_GAMMA:
            touched, power = chroma_gamma_parts(planes, p[0], p[1])
            c = np.where(touched, power.astype(np.float32), c)
        elif kind == CHROMA_NEUTRALIZE:                      # both bounds are read from .Low (:473)
            c = np.where(l < f32(p[0]), f32(0), c)
        elif kind == CHROMA_FOR_HUES:
            c = np.where(hue_in_range(h, p[0], p[1]), go_clamp01(c * f32(p[2])), c)
        elif kind == ROTATE_HUES:
            h = np.where(~(l < f32(p[3])) & hue_in_range(h, p[0], p[1]), h + f32(p[2]), h)
        else:
            raise ValueError(kind)
    return np.stack([h, c, l]).astype(np.float32)


# ---- colour export (tiff16.go:45-91, writejpg.go:43-89) --------------------------------------------------------------

def export_rgb(planes, mn, mx, gamma, bits):
    """(n, 4) counts R G B A of WriteTIFF16 (bits 16, uint16) / WriteJPG (bits 8, uint8)"""
    chans = [tone_ref.export_gray(planes[c], mn, mx, gamma, bits) for c in range(3)]
    return np.stack(chans + [np.full_like(chans[0], 65535 if bits == 16 else 255)], axis=1)


def rgba64_bytes(counts):
    """image.RGBA64.Pix of (n, 4) uint16 counts: big-endian"""
    return np.asarray(counts, np.uint16).astype(">u2").tobytes()


# ---- the inputs of tests/test_gpu_colour.py ----------------------------------------------------------------------------

# (width, height): no quad and no block; odd; width no multiple of 4 (slots off 16-byte alignment); several workgroups;
# the padded slot stride
SHAPES = [(5, 3), (15, 15), (67, 35), (261, 70), (512, 512)]
BLOCKS = [1, 3, 16, 64]
BORDERS = [0.0, 0.1, 0.45]
SKIPS = [(0.0, 0.75), (0.1, 0.1), (0.6, 0.6)]
CHROMA_GAMMAS = [(1.5, 0.2), (0.5, 0.0), (2.2, 0.9)]      # (gamma, threshold)
EXPORTS = [(0.0, 1.0, 1.0, 16), (0.0, 1.0, 1.0, 8), (0.05, 0.9, 2.2, 16), (0.05, 0.9, 2.2, 8), (0.3, 0.3, 1.0, 16)]


@functools.lru_cache(maxsize=None)
def planes(name, w, h):
    """(3, w * h): three different skies -- tone_ref.sky (NaN, +-Inf, -0.0, negatives, values above 1) or tone_ref.plain
    (finite, [0, 1)) with the seeds moved apart by the channel"""
    make = tone_ref.sky if name == "sky" else tone_ref.plain
    rng = np.random.default_rng(1000 + w)
    out = np.stack([np.roll(make(w, h), 17 * c) if c == 0 else rng.permutation(make(w, h)) for c in range(3)])
    out = out.astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def hcl(name, w, h):
    """(3, w * h) planes {h, c, l}: hue in [0, 360) with the specials of the sky, chroma and luminance from planes()"""
    p = planes(name, w, h)
    with np.errstate(all="ignore"):
        out = np.stack([(p[0] * f32(360)).astype(np.float32), p[1], p[2]])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def stars(w, h, n=40):
    """about n synthetic stars, brightest first: HFR 0.4 ... 9, the first ones on corners and edges"""
    rng = np.random.default_rng(5 * w + h)
    s = np.zeros(n, STAR_DTYPE)
    xs = rng.integers(0, w, n)
    ys = rng.integers(0, h, n)
    fixed = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (0, h // 2), (w - 1, h // 2), (w // 2, h - 1)]
    for i, (x, y) in enumerate(fixed[:n]):
        xs[i], ys[i] = x, y
    s["index"] = (xs + w * ys).astype(np.int32)
    s["hfr"] = np.linspace(0.4, 9.0, n).astype(np.float32)[rng.permutation(n)]
    s["x"], s["y"] = xs, ys
    s["mass"] = np.sort(rng.random(n).astype(np.float32))[::-1]
    s.setflags(write=False)
    return s


def power_cases():
    """(what, pixels, near) for every power the GPU tests compare"""
    for name in ("plain", "sky"):
        for w, h in SHAPES:
            p = hcl(name, w, h)
            for g, thr in CHROMA_GAMMAS:
                touched, power = chroma_gamma_parts(p, g, thr)
                yield "%s %dx%d chroma gamma %g" % (name, w, h, g), p.shape[1], touched & tone_ref.near_boundary(power)
            q = planes(name, w, h)
            for mn, mx, gamma, bits in EXPORTS:
                for c in range(3):
                    gray, gamma_inv = tone_ref.export_parts(q[c], mn, mx, gamma)
                    if gamma_inv != 1.0:
                        yield ("%s %dx%d export gamma %g plane %d" % (name, w, h, gamma, c), q.shape[1],
                               tone_ref.near_boundary(tone_ref._pow32(gray, gamma_inv)[1]))
