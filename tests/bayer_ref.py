"""CPU restatement of OpBadPixel's Bayer branch and OpDebayer (numpy fp32, the oracle's median for the perimeter).

  correct    CosmeticCorrectionBayer  internal/ops/pre/badpixels_bayer.go:26-351
  debayer    DebayerBilinear          internal/ops/pre/debayer.go:41-263
  front      OpCalibrate -> OpBadPixel -> OpDebayer as preprocess.go:68-251 chains them

Sequential fp32 sums are np.add.accumulate (never np.sum, which is pairwise); numpy's fp32 arithmetic is IEEE single
precision with correct rounding and no fused multiply-add, as the reference's amd64 build.
"""
import math

import numpy as np

import preprocess_ref

CFA_OFFSETS = {"RGGB": (0, 0), "rggb": (0, 0), "GRBG": (1, 0), "grbg": (1, 0),
               "GBRG": (0, 1), "gbrg": (0, 1), "BGGR": (1, 1), "bggr": (1, 1)}
CHANNELS = {"R": "R", "r": "R", "G": "G", "g": "G", "B": "B", "b": "B"}

SQRT2 = np.float32(math.sqrt(2.0))
# 1.0/(2.0+sqrt2) as a typed float32 constant: rounded to float32 after every operation
GREEN_K = np.float32(1.0 / float(np.float32(2.0 + float(SQRT2))))
GREEN_K_ONCE = np.float32(0.29289323)      # the exact value rounded once (not the reference's, see the tests)

G_OFFSETS = [(0, -2), (-1, -1), (1, -1), (-2, 0), (0, 0), (2, 0), (-1, 1), (1, 1), (0, 2)]   # (x, y), :122-132
RB_OFFSETS = [(dx, dy) for dy in (-2, 0, 2) for dx in (-2, 0, 2)]                               # row by row, :82-97


class BayerError(ValueError):
    pass


def offsets(cfa):
    """getOffsets (debayer.go:26-37)."""
    if cfa not in CFA_OFFSETS:
        raise BayerError("Unknown CFA value " + cfa)
    return CFA_OFFSETS[cfa]


def parse(channel, cfa):
    xo, yo = offsets(cfa)
    if channel not in CHANNELS:
        raise BayerError("Unknown debayering value " + channel)
    return CHANNELS[channel], xo, yo


def debayer_shape(width, height, channel, cfa):
    if channel == "" or cfa == "":
        return width, height
    _, xo, yo = parse(channel, cfa)
    return (width - xo) & ~1, (height - yo) & ~1


def channel_rows(width, height, channel, xo, yo):
    """[(y, x0, n)] of the channel's walk: R from (xo, yo), B from (xo+1, yo+1), G every row from yo starting at
    xo+1, xo, xo+1, ... (colorOffsetX)."""
    if channel == "G":
        return [(y, xo + (1 if (y - yo) % 2 == 0 else 0), None) for y in range(yo, height)]
    x0, y0 = (xo, yo) if channel == "R" else (xo + 1, yo + 1)
    return [(y, x0, None) for y in range(y0, height, 2)]


def _net9(a):
    """MedianFloat32Slice9 (median3x3.go:85-110) on nine arrays, literally (`if a[i] > a[j]`)."""
    a = [np.asarray(v, np.float32).copy() for v in a]

    def swap(i, j):
        g = a[i] > a[j]
        lo = np.where(g, a[j], a[i])
        a[j] = np.where(g, a[i], a[j])
        a[i] = lo

    def maxto(i, j):
        a[j] = np.where(a[i] > a[j], a[i], a[j])

    def minto(i, j):
        a[i] = np.where(a[i] > a[j], a[j], a[i])

    for i, j in ((0, 1), (3, 4), (6, 7), (1, 2), (4, 5), (7, 8), (0, 1), (3, 4), (6, 7)):
        swap(i, j)
    maxto(0, 3)
    maxto(3, 6)
    swap(1, 4)
    minto(4, 7)
    maxto(1, 4)
    minto(5, 8)
    minto(2, 5)
    swap(2, 4)
    minto(4, 6)
    maxto(2, 4)
    return a[4]


def medians(oracle, img, channel, xo, yo):
    """Phase 1 (MedianFilterBayer*): per channel row, the medians of its pixels from the original data."""
    h, w = img.shape
    offs = G_OFFSETS if channel == "G" else RB_OFFSETS
    out = []
    for y, x0, _ in channel_rows(w, h, channel, xo, yo):
        xs = np.arange(x0, w, 2)
        med = np.empty(xs.size, np.float32)
        inner = (xs >= 2) & (xs + 2 < w) & (y >= 2) & (y + 2 < h)
        if inner.any():
            xi = xs[inner]
            med[inner] = _net9([img[y + dy, xi + dx] for dx, dy in offs])
        for k in np.flatnonzero(~inner):
            x = int(xs[k])
            vals = [img[y + dy, x + dx] for dx, dy in offs if 0 <= y + dy < h and 0 <= x + dx < w]
            med[k] = oracle.median_f32(np.array(vals, np.float32))
        out.append((y, xs, med))
    return out


def _row_chains(rows):
    """Per row a fresh fp32 accumulator from 0 summing left to right, then the row totals in order."""
    width = max((r.size for r in rows), default=0)
    if not rows:
        return np.float32(0)
    m = np.zeros((len(rows), width + 1), np.float32)       # (+0 padding never changes a sum that started at +0)
    for i, r in enumerate(rows):
        m[i, 1:1 + r.size] = r
    row_sums = np.add.accumulate(m, axis=1, dtype=np.float32)[:, -1]
    return np.add.accumulate(np.concatenate([np.zeros(1, np.float32), row_sums]), dtype=np.float32)[-1]


def delta_stats(deltas):
    """DeltaStatsBayer* (badpixels_bayer.go:190-296) over the per-row deltas."""
    count = sum(d.size for d in deltas)
    with np.errstate(all="ignore"):
        mean = np.float32(_row_chains(deltas) / np.float32(count))
        sq = [((d - mean) * (d - mean)).astype(np.float32) for d in deltas]
        total = _row_chains(sq)
        var = np.float32(total / np.float32(count)) if count > 0 else np.float32(0)
    std = np.float32(math.sqrt(float(var))) if not np.isnan(var) else np.float32(np.nan)
    return mean, std


def correct(oracle, data, width, channel, cfa, sigma_low, sigma_high):
    """CosmeticCorrectionBayer.  Returns (out, numRemoved, (mean, std))."""
    ch, xo, yo = parse(channel, cfa)
    img = np.asarray(data, np.float32).reshape(-1, width)
    meds = medians(oracle, img, ch, xo, yo)
    with np.errstate(all="ignore"):
        deltas = [(img[y, xs] - med).astype(np.float32) for y, xs, med in meds]
    mean, std = delta_stats(deltas)
    lo = np.float32(-np.float32(sigma_low) * std)
    hi = np.float32(np.float32(sigma_high) * std)
    out = img.copy()
    removed = 0
    with np.errstate(invalid="ignore"):
        for (y, xs, med), d in zip(meds, deltas):
            bad = (d < lo) | (d > hi)
            out[y, xs[bad]] = med[bad]
            removed += int(bad.sum())
    return out.reshape(-1), removed, (mean, std)


def debayer(data, width, channel, cfa):
    """DebayerBilinear.  Returns (plane, adj_width, adj_height)."""
    ch, xo, yo = parse(channel, cfa)
    img = np.asarray(data, np.float32).reshape(-1, width)
    h, w = img.shape
    aw, ah = (w - xo) & ~1, (h - yo) & ~1
    out = np.zeros((ah, aw), np.float32)
    if aw <= 0 or ah <= 0:
        return out.reshape(-1), aw, ah
    rows = np.arange(0, ah, 2)[:, None] + yo          # source row / column of each box's origin
    cols = np.arange(0, aw, 2)[None, :] + xo
    rows, cols = np.broadcast_arrays(rows, cols)
    at = lambda dy, dx: img[np.clip(rows + dy, 0, h - 1), np.clip(cols + dx, 0, w - 1)]   # noqa: E731
    right, down = cols < w - 2, rows < h - 2
    left, up = cols > 0, rows > 0
    f = np.float32
    with np.errstate(all="ignore"):
        if ch == "R":
            r = at(0, 0)
            r_right = np.where(right, at(0, 2), r)
            r_down = np.where(down, at(2, 0), r)
            r_rd = np.where(right & down, at(2, 2), r)
            o = (r, f(0.5) * (r + r_right), f(0.5) * (r + r_down), f(0.25) * (r + r_right + r_down + r_rd))
        elif ch == "G":
            g1, g2 = at(0, 1), at(1, 0)
            fb1 = (f(2.0) * g1 + SQRT2 * g2) * GREEN_K
            fb2 = (SQRT2 * g1 + f(2.0) * g2) * GREEN_K
            g1_left = np.where(left, at(0, -1), fb1)
            g2_up = np.where(up, at(-1, 0), fb2)
            g2_right = np.where(right, at(1, 2), fb1)
            g1_down = np.where(down, at(2, 1), fb2)
            o = (f(0.25) * (g1 + g2 + g1_left + g2_up), g1, g2, f(0.25) * (g1 + g2 + g2_right + g1_down))
        else:
            b = at(1, 1)
            b_left = np.where(left, at(1, -1), b)
            b_up = np.where(up, at(-1, 1), b)
            b_lu = np.where(left & up, at(-1, -1), b)
            o = (f(0.25) * (b + b_left + b_up + b_lu), f(0.5) * (b + b_up), f(0.5) * (b + b_left), b)
    out[0::2, 0::2], out[0::2, 1::2], out[1::2, 0::2], out[1::2, 1::2] = o
    return out.reshape(-1), aw, ah


def front(oracle, light, width, height, channel, cfa, sigma_low=3.0, sigma_high=5.0, dark=None, flat=None):
    """OpCalibrate -> OpBadPixel -> OpDebayer.  Returns (out, out_w, out_h, removed, (mean, std)); stats NaN when no
    bad-pixel step ran, the mono MedianDiffStats on the mono branch."""
    x = preprocess_ref.calibrate(oracle, light, dark, flat)
    removed, stats = 0, (np.float32(np.nan), np.float32(np.nan))
    if sigma_low != 0 and sigma_high != 0:
        if channel == "":
            x, removed, stats = preprocess_ref.badpixel(oracle, x, width, sigma_low, sigma_high)
        else:
            x, removed, stats = correct(oracle, x, width, channel, cfa, sigma_low, sigma_high)
    if channel == "" or cfa == "":
        return x, width, height, removed, stats
    out, aw, ah = debayer(x, width, channel, cfa)
    if aw * ah == 0:
        raise BayerError("empty debayered image")
    return out, aw, ah, removed, stats
