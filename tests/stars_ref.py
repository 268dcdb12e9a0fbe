"""CPU restatement of star.FindStars (internal/star/findstars.go:59-103), the checker of nl_find_stars.

Literal where order matters, vectorised across independent items where it does not:
- fp32 throughout (numpy float32 scalars and arrays round every operation to fp32);
- every sum is one sequential chain in the reference's order -- a loop over the window's offsets that adds one
  term at a time, vectorised across stars only (never np.sum, which is pairwise);
- QSortStarsDesc's Hoare partition and filterOutOverlaps' bin grid verbatim;
- Go's float -> int32 conversion as amd64 does it (CVTTSS2SL: truncation, MinInt32 for NaN or out of range) and
  int32 index arithmetic with wrap-around;
- the reference's panics raised as GoPanic.
Deviation 1 of include/nlstack.h (diff_std None with bp_sigma > 0) is restated as the library defines it.
"""
import math

import numpy as np

f32 = np.float32
INT32_MIN = -(1 << 31)
MAX_FLOAT32 = f32(3.4028234663852886e38)


class GoPanic(Exception):
    pass


def go_i32(v):
    """int32(v) for a float32 / float64 v on amd64."""
    v = float(v)
    if math.isnan(v) or not (-2147483649.0 < v < 2147483648.0):
        return INT32_MIN
    return int(v)              # truncation toward zero


def wrap32(v):
    return ((int(v) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def go_div(a, b):
    """int32 a / b, truncated toward zero."""
    q = abs(a) // abs(b)
    return wrap32(q if (a >= 0) == (b >= 0) else -q)


def go_mod(a, b):
    return a - go_div(a, b) * b


def star(index, value, x, y, mass, hfr):
    return [int(index), f32(value), f32(x), f32(y), f32(mass), f32(hfr)]


IDX, VAL, X, Y, MASS, HFR = range(6)


# -- findBrightPixels (findstars.go:105-131) ---------------------------------------------------------------------
def find_bright_pixels(data, width, threshold, radius):
    stars = []
    hits = np.flatnonzero(data > threshold)          # (v > threshold: never a NaN)
    for i in hits.tolist():
        v = data[i]
        x, y = f32(i % width), f32(i // width)
        if stars:
            old = stars[-1]
            if old[Y] == y and old[X] >= f32(x - f32(radius)):
                if old[VAL] >= v:
                    continue                          # keep the old candidate, it is brighter
                stars[-1] = star(i, v, x, y, v, 1)    # replace it with the brighter new one
                continue
        stars.append(star(i, v, x, y, v, 1))
    return stars


# -- MedianFloat32Slice9 (median3x3.go:85-110), in place on a 9-slot buffer --------------------------------------
def median9_inplace(a):
    def ce(i, j):
        if a[i] > a[j]:
            a[i], a[j] = a[j], a[i]

    def maxto(i, j):
        if a[i] > a[j]:
            a[j] = a[i]

    def minto(i, j):
        if a[i] > a[j]:
            a[i] = a[j]

    ce(0, 1); ce(3, 4); ce(6, 7)
    ce(1, 2); ce(4, 5); ce(7, 8)
    ce(0, 1); ce(3, 4); ce(6, 7)
    maxto(0, 3)
    maxto(3, 6)
    ce(1, 4)
    minto(4, 7)
    maxto(1, 4)
    minto(5, 8)
    minto(2, 5)
    ce(2, 4)
    minto(4, 6)
    maxto(2, 4)
    return a[4]


def median9_vec(cols):
    """The same network over arrays (one lane per element): `if a[i] > a[j]` as np.where."""
    a = [np.array(c, dtype=np.float32) for c in cols]

    def ce(i, j):
        g = a[i] > a[j]
        lo = np.where(g, a[j], a[i])
        a[j] = np.where(g, a[i], a[j])
        a[i] = lo

    def maxto(i, j):
        a[j] = np.where(a[i] > a[j], a[i], a[j])

    def minto(i, j):
        a[i] = np.where(a[i] > a[j], a[j], a[i])

    ce(0, 1); ce(3, 4); ce(6, 7)
    ce(1, 2); ce(4, 5); ce(7, 8)
    ce(0, 1); ce(3, 4); ce(6, 7)
    maxto(0, 3)
    maxto(3, 6)
    ce(1, 4)
    minto(4, 7)
    maxto(1, 4)
    minto(5, 8)
    minto(2, 5)
    ce(2, 4)
    minto(4, 6)
    maxto(2, 4)
    return a[4]


def create_mask(width, radius):
    """CreateMask (findstars.go:187-200)."""
    mask = []
    rad = int(radius)
    for y in range(-rad, rad + 1):
        for x in range(-rad, rad + 1):
            dist = f32(math.sqrt(float(y * y + x * x)))
            if dist <= f32(f32(radius) + f32(1e-8)):
                mask.append(y * width + x)
    return mask


def gather(data, index, mask, buffer):
    """GatherAndMedian's gather (gather.go:26-38): the offsets inside the data fill buffer[0 ..)."""
    num = 0
    for o in mask:
        j = wrap32(index + o)
        if 0 <= j < data.size:
            buffer[num] = data[j]
            num += 1


def median_diff_std(data, width):
    """Deviation 1: Stats.StdDev of data[i] - median over every pixel whose whole mask lies inside the data (fp64
    sums of the fp32 differences; mean and std rounded to fp32, stats.go:134-144, 264-287)."""
    n = data.size
    lo, hi = width + 1, max(width + 1, n - width - 1)
    m = hi - lo
    if m <= 0:
        return f32("nan")
    i = np.arange(lo, hi)
    offs = [-width - 1, -width, -width + 1, -1, 0, 1, width - 1, width, width + 1]
    diff = (data[i] - median9_vec([data[i + o] for o in offs])).astype(np.float32)
    mean = f32(math.fsum(diff.astype(np.float64).tolist()) / m)
    d = (diff - mean).astype(np.float64)
    var = math.fsum((d * d).tolist()) / m
    return f32(math.sqrt(var))


# -- rejectBadPixels (findstars.go:134-168) -----------------------------------------------------------------------
def reject_bad_pixels(stars, data, width, sigma, diff_std):
    n = data.size
    mask = create_mask(width, 1.5)
    assert len(mask) == 9
    if diff_std is None or math.isnan(diff_std):
        diff_std = median_diff_std(data, width)
    threshold = f32(f32(diff_std) * f32(sigma))
    if not stars:
        return []
    idx = np.array([s[IDX] for s in stars], dtype=np.int64)
    interior = (idx >= width + 1) & (idx <= n - width - 2)
    med = np.zeros(len(stars), np.float32)
    ii = idx[interior]
    if ii.size:
        med[interior] = median9_vec([data[ii + o] for o in mask])
    # the candidates whose mask leaves the data: the buffer holds what the network left for the previous candidate
    buffer = [f32(0)] * 9
    for k in np.flatnonzero(~interior).tolist():
        if k > 0 and interior[k - 1]:
            gather(data, int(idx[k - 1]), mask, buffer)
            median9_inplace(buffer)
        gather(data, int(idx[k]), mask, buffer)
        med[k] = median9_inplace(buffer)
    diff = (data[idx] - med).astype(np.float32)
    keep = (diff < threshold) & (-diff < threshold)
    return [s for s, k in zip(stars, keep.tolist()) if k]


# -- QSortStarsDesc / QPartitionStarsDesc (qsort.go:25-57) -------------------------------------------------------
def partition_desc(a, lo, hi):
    length = hi - lo
    left, right = 0, length - 1
    mid = (left + right) >> 1
    pivot = a[lo + mid][MASS]
    l, r = left - 1, right + 1
    while True:
        while True:
            l += 1
            if l >= length:
                raise GoPanic("QPartitionStarsDesc: index out of range (NaN pivot)")
            if a[lo + l][MASS] <= pivot:
                break
        while True:
            r -= 1
            if r < 0:
                raise GoPanic("QPartitionStarsDesc: index out of range (NaN pivot)")
            if a[lo + r][MASS] >= pivot:
                break
        if l >= r:
            return r
        a[lo + l], a[lo + r] = a[lo + r], a[lo + l]


def qsort_desc(a):
    todo = [(0, len(a))]
    while todo:
        lo, hi = todo.pop()
        if hi - lo > 1:
            index = partition_desc(a, lo, hi)
            todo.append((lo + index + 1, hi))
            todo.append((lo, lo + index + 1))


# -- filterOutOverlaps (findstars.go:209-270) ---------------------------------------------------------------------
def filter_out_overlaps(stars, width, height, radius):
    bin_size = 256
    x_bins = (width + bin_size - 1) // bin_size
    y_bins = (height + bin_size - 1) // bin_size
    bins = [[] for _ in range(x_bins * y_bins)]    # each cell: its stars in insertion order (the linked list)
    radius_sq = wrap32(radius * radius)
    out = []
    for s in stars:
        x_cell = go_div(go_i32(f32(s[X] + f32(0.5))), bin_size)
        y_cell = go_div(go_i32(f32(s[Y] + f32(0.5))), bin_size)
        near = False
        for dy in (-1, 0, 1):
            if y_cell + dy < 0 or y_cell + dy >= y_bins:
                continue
            for dx in (-1, 0, 1):
                if x_cell + dx < 0 or x_cell + dx >= x_bins:
                    continue
                for s2 in bins[(x_cell + dx) + (y_cell + dy) * x_bins]:
                    x_dist = f32(s[X] - s2[X])
                    y_dist = f32(s[Y] - s2[Y])
                    sq = go_i32(f32(f32(f32(x_dist * x_dist) + f32(y_dist * y_dist)) + f32(0.5)))
                    if sq <= radius_sq:
                        near = True
                        break
                if near:
                    break
            if near:
                break
        if near:
            continue
        kept = list(s)
        out.append(kept)
        cell = wrap32(x_cell + wrap32(y_cell * x_bins))
        if cell < 0 or cell >= len(bins):
            raise GoPanic("filterOutOverlaps: index out of range (cell %d of %d)" % (cell, len(bins)))
        bins[cell].append(kept)
    return out


# -- shiftToCenterOfMass (findstars.go:274-325), vectorised across stars -----------------------------------------
def shift_to_center_of_mass(stars, data, width, threshold, radius):
    m = len(stars)
    if m == 0:
        return stars, f32(0)
    n = data.size
    idx = np.array([s[IDX] for s in stars], dtype=np.int64)
    val = np.array([s[VAL] for s in stars], dtype=np.float32)
    sx = np.array([s[X] for s in stars], dtype=np.float32)
    sy = np.array([s[Y] for s in stars], dtype=np.float32)
    smass = np.array([s[MASS] for s in stars], dtype=np.float32)
    shift_sq = np.full(m, MAX_FLOAT32, np.float32)
    active = np.ones(m, bool)
    threshold = f32(threshold)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for _round in range(10):
            active &= shift_sq > f32(0.0001)
            if not active.any():
                break
            a = np.flatnonzero(active)
            ia = idx[a]
            xm = np.zeros(a.size, np.float32)
            ym = np.zeros(a.size, np.float32)
            mass = np.zeros(a.size, np.float32)
            for y in range(-radius, radius + 1):
                rb = _wrap_vec(ia + _wrap_vec(np.int64(y) * width))
                for x in range(-radius, radius + 1):
                    j = _wrap_vec(rb + x)
                    inside = (j >= 0) & (j < n)
                    value = np.zeros(a.size, np.float32)
                    value[inside] = data[j[inside]] - threshold
                    value[value < 0] = 0
                    xm = xm + f32(x) * value
                    ym = ym + f32(y) * value
                    mass = mass + value
            x0 = _trunc_mod(ia, width)
            y0 = _trunc_div(ia, width)
            mass[mass == 0] = f32(1e-8)
            dx = xm / mass
            dy = ym / mass
            nx = x0.astype(np.float32) + dx
            ny = y0.astype(np.float32) + dy
            pdx = nx - sx[a]
            pdy = ny - sy[a]
            shift_sq[a] = pdx * pdx + pdy * pdy
            gy = np.array([go_i32(v) for v in (dy + f32(0.5)).tolist()], np.int64)
            gx = np.array([go_i32(v) for v in (dx + f32(0.5)).tolist()], np.int64)
            ni = _wrap_vec(_wrap_vec(ia + _wrap_vec(np.int64(width) * gy)) + gx)
            inside = (ni >= 0) & (ni < n)
            nv = np.zeros(a.size, np.float32)
            nv[inside] = data[ni[inside]]
            idx[a], val[a], sx[a], sy[a], smass[a] = ni, nv, nx, ny, mass
    shifts = np.sqrt(shift_sq.astype(np.float64)).astype(np.float32)
    total = f32(0)
    for s in shifts.tolist():                       # sumOfShifts: one serial chain in list order
        total = f32(total + f32(s))
    out = [star(int(idx[k]), val[k], sx[k], sy[k], smass[k], 0) for k in range(m)]
    return out, total


def _wrap_vec(v):
    return ((np.asarray(v, np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _trunc_div(a, b):
    q = np.abs(a) // abs(b)
    return np.where((a >= 0) == (b >= 0), q, -q)


def _trunc_mod(a, b):
    return a - _trunc_div(a, b) * b


# -- calcAndFilterHalfFluxRadius (findstars.go:327-383), vectorised across stars ---------------------------------
def _disc_sums(idx, data, width, rad, limit, location, with_distance):
    n = data.size
    moment = np.zeros(idx.size, np.float32)
    mass = np.zeros(idx.size, np.float32)
    pixels = 0
    for y in range(-rad, rad + 1):
        rb = _wrap_vec(idx + _wrap_vec(np.int64(y) * width))
        for x in range(-rad, rad + 1):
            dist_sq = wrap32(x * x + y * y)
            if dist_sq > limit:
                continue
            distance = f32(math.sqrt(float(dist_sq)))
            j = _wrap_vec(rb + x)
            inside = (j >= 0) & (j < n)
            value = np.zeros(idx.size, np.float32)
            v = np.zeros(idx.size, np.float32)
            v[inside] = data[j[inside]] - f32(location)
            pos = v > 0                                      # (a NaN pixel adds 0)
            value[pos] = v[pos]
            if with_distance:
                moment = moment + distance * value
            mass = mass + value
            pixels += 1
    return moment, mass, pixels


def calc_and_filter_hfr(stars, data, width, radius, location, star_in_out):
    radius = f32(radius)
    star_in_out = f32(star_in_out)
    kept, avg = [], f32(0)
    if stars:
        n = data.size
        idx = np.array([s[IDX] for s in stars], dtype=np.int64)
        rad = go_i32(math.ceil(float(radius)))
        r_eps = float(f32(radius + f32(1e-8)))
        limit = go_i32(math.ceil(r_eps * r_eps))
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            moment, mass, pixels = _disc_sums(idx, data, width, rad, limit, location, True)
            mass[mass == 0] = f32(1e-8)
            hfr = moment / mass
            # the inner disc of every star: its own innerRad and limit; one pass over the largest square, each star
            # adding only its own offsets (y outer, x inner: the same chain as its own loops)
            inner_rad = np.array([go_i32(math.ceil(float(h))) for h in hfr.tolist()], np.int64)
            inner_lim = np.array([go_i32(math.ceil(float(f32(h * h)))) for h in hfr.tolist()], np.int64)
            # (a NaN hfr gives innerRad = MinInt32: one pass of the loops with x = y = MinInt32, skipped by its
            # limit MinInt32 -- no inner pixel, as here)
            live = ~(hfr > radius)
            top = int(inner_rad[live].max()) if live.any() else -1
            inner_mass = np.zeros(idx.size, np.float32)
            inner_pixels = np.zeros(idx.size, np.int64)
            for y in range(-top, top + 1):
                rb = _wrap_vec(idx + _wrap_vec(np.int64(y) * width))
                for x in range(-top, top + 1):
                    take = live & (abs(x) <= inner_rad) & (abs(y) <= inner_rad) & (x * x + y * y <= inner_lim)
                    if not take.any():
                        continue
                    j = _wrap_vec(rb + x)
                    inside = take & (j >= 0) & (j < n)
                    v = np.zeros(idx.size, np.float32)
                    v[inside] = data[j[inside]] - f32(location)
                    value = np.where(v > 0, v, f32(0))
                    inner_mass = np.where(take, inner_mass + value, inner_mass)
                    inner_pixels += take
            for k, s in enumerate(stars):
                h = hfr[k]
                if h > radius:
                    continue
                outer_mass = f32(mass[k] - inner_mass[k])
                outer_pixels = pixels - int(inner_pixels[k])
                if f32(inner_mass[k] * f32(outer_pixels)) <= f32(f32(star_in_out * outer_mass) * f32(int(inner_pixels[k]))):
                    continue
                t = list(s)
                t[HFR] = h
                t[MASS] = mass[k]
                kept.append(t)
                avg = f32(avg + h)
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = f32(avg / f32(len(kept)))
    return kept, avg


# -- FindStars (findstars.go:59-103) -------------------------------------------------------------------------------
def find_stars(data, width, location, scale, star_sig, bp_sigma, star_in_out, radius, diff_std=None):
    """Returns (stars as [index, value, x, y, mass, hfr] lists, sumOfShifts, avgHFR); raises GoPanic where the
    reference panics."""
    data = np.ascontiguousarray(data, dtype=np.float32).reshape(-1)
    location, scale, star_sig = f32(location), f32(scale), f32(star_sig)
    height = data.size // width
    stars = find_bright_pixels(data, width, f32(location + f32(scale * star_sig)), radius)
    if f32(bp_sigma) > 0:
        stars = reject_bad_pixels(stars, data, width, bp_sigma, diff_std)
    qsort_desc(stars)
    stars = filter_out_overlaps(stars, width, height, radius)
    stars, sum_of_shifts = shift_to_center_of_mass(stars, data, width,
                                                   f32(location + f32(f32(scale * star_sig) * f32(0.5))), radius)
    qsort_desc(stars)
    stars = filter_out_overlaps(stars, width, height, radius)
    stars, avg_hfr = calc_and_filter_hfr(stars, data, width, radius, location, star_in_out)
    return stars, sum_of_shifts, avg_hfr


def as_array(stars):
    """The star list as the library's structured array (fields index value x y mass hfr)."""
    dt = np.dtype([("index", "<i4"), ("value", "<f4"), ("x", "<f4"), ("y", "<f4"), ("mass", "<f4"), ("hfr", "<f4")])
    out = np.zeros(len(stars), dt)
    for k, s in enumerate(stars):
        out[k] = tuple(s)
    return out
