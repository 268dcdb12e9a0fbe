"""CPU restatement of OpBackExtract (internal/ops/pre/preprocess.go:372-398): pre.NewBackground (background.go:68-106)
and Background.Subtract / Render (:309-462), in fp32 throughout.

The star masks are vectorised per star over a cell.  The three selects of FitCell (:464-492) go through the oracle's
literal C QSelect* (which returns the permuted array) when their input holds no NaN, else through the bounds-checked
literal Python `qselect` below (C would read out of bounds where Go panics).  The grid steps and the two state machines
of Subtract run as literal loops; the per-pixel bilinear value is vectorised in the reference's fp32 order.  Where the
reference panics, GoPanic is raised; where it would loop forever (clip, deviation 3), GoHang."""
import numpy as np

f32 = np.float32
INT32_MIN = -2 ** 31
GAUSS = (f32(0.468592), f32(0.107973), f32(0.024879))
OFFSETS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))


class GoPanic(Exception):
    pass


class GoHang(GoPanic):
    pass


def go_i32(v):
    """int32(float32) on amd64 (CVTTSS2SL): truncation, 0x80000000 for NaN and out of range."""
    v = f32(v)
    if not (v >= f32(-2147483648.0) and v < f32(2147483648.0)):
        return INT32_MIN
    return int(v)


def qselect(a, k):
    """QSelectFloat32 (qsort.go:94-126), literally, on the list a in place; GoPanic where Go's bounds check fires."""
    n = len(a)
    left, right = 0, n - 1
    while left < right:
        mid = (left + right) >> 1
        pivot = a[mid]
        l, r = left - 1, right + 1
        while True:
            while True:
                l += 1
                if l >= n:
                    raise GoPanic("QSelectFloat32: index %d out of range [%d] (NaN pivot)" % (l, n))
                if a[l] >= pivot:
                    break
            while True:
                r -= 1
                if r < 0:
                    raise GoPanic("QSelectFloat32: index -1 out of range")
                if a[r] <= pivot:
                    break
            if l >= r:
                break
            a[l], a[r] = a[r], a[l]
        offset = r - left + 1
        if k <= offset:
            right = r
        else:
            left = r + 1
            k -= offset
    if left >= n:
        raise GoPanic("QSelectFloat32: index %d out of range [%d]" % (left, n))
    return a[left]


def qselect_median(a):
    """QSelectMedianFloat32 (qsort.go:68-82), literally, on the list a in place."""
    n = len(a)
    k = (n >> 1) + 1
    upper = qselect(a, k)
    if n & 1:
        return upper
    lower = a[0]
    for i in range(1, k - 1):
        if a[i] > lower:
            lower = a[i]
    return f32(f32(0.5) * f32(lower + upper))


def select_median(a, oracle):
    """QSelectMedianFloat32 of the fp32 array a: (value, permuted array)."""
    if a.size == 0:
        raise GoPanic("QSelectFloat32 on an empty slice (index 0 out of range [0])")
    if not np.isnan(a).any():
        return oracle.qselect_median(a)
    lst = [f32(v) for v in a]
    v = qselect_median(lst)
    return f32(v), np.array(lst, np.float32)


def median_f32(a):
    """median.MedianFloat32 (median3x3.go:115-119) over at most 8 NaN-free values."""
    if len(a) == 0:
        return f32(np.nan)
    return f32(qselect_median(list(a)))


def geometry(width, height, grid):
    cx = (width + grid // 2) // grid
    cy = (height + grid // 2) // grid
    if cx == 0 or cy == 0:
        raise GoPanic("integer divide by zero (grid of %dx%d cells)" % (cx, cy))
    return cx, cy, f32(f32(width) / f32(cx)), f32(f32(height) / f32(cy))


def star_eq(a, b):
    return all(a[n] == b[n] for n in ("index", "value", "x", "y", "mass", "hfr"))


def bin_stars(stars, cx, cy, spx, spy, hfr_factor):
    """binStarsIntoCells (:108-143): per cell the list of star indices."""
    bins = [[] for _ in range(cx * cy)]
    hf = f32(hfr_factor)
    for i, s in enumerate(stars):
        sx, sy, hfr = f32(s["x"]), f32(s["y"]), f32(f32(s["hfr"]) * hf)
        for yo in (-1, 0, 1):
            for xo in (-1, 0, 1):
                x = f32(sx + f32(f32(xo) * hfr))
                y = f32(sy + f32(f32(yo) * hfr))
                cellx = min(max(go_i32(f32(x / spx)), 0), cx - 1)
                celly = min(max(go_i32(f32(y / spy)), 0), cy - 1)
                c = bins[celly * cx + cellx]
                if not c or not star_eq(stars[c[-1]], s):
                    c.append(i)
    return bins


def hfr_sq(s, hfr_factor):
    h, f = f32(s["hfr"]), f32(hfr_factor)
    return f32(f32(f32(h * h) * f) * f)


def cell_rect(x, y, spx, spy, width, height):
    y0 = go_i32(f32(f32(y) * spy + f32(0.5)))
    y1 = min(go_i32(f32(f32(f32(y) + f32(1)) * spy + f32(0.5))), height)
    x0 = go_i32(f32(f32(x) * spx + f32(0.5)))
    x1 = min(go_i32(f32(f32(f32(x) + f32(1)) * spx + f32(0.5))), width)
    return x0, x1, y0, y1


def gather(img, rect, entries):
    """gatherWithoutStars (:494-515): the cell's unmasked pixels in row-major order."""
    x0, x1, y0, y1 = rect
    block = img[y0:y1, x0:x1]
    if block.size == 0:
        return block.reshape(-1)
    xs = np.arange(x0, x1, dtype=np.float32)[None, :]
    ys = np.arange(y0, y1, dtype=np.float32)[:, None]
    masked = np.zeros(block.shape, bool)
    for sx, sy, hsq in entries:
        dx, dy = xs - sx, ys - sy
        masked |= (dx * dx + dy * dy) <= hsq
    return block[~masked]


def fit_cell(samples, sigma, oracle):
    """FitCell (:464-492) after the gather."""
    median, perm = select_median(samples, oracle)
    mad, _ = select_median(np.abs(perm - median).astype(np.float32), oracle)
    upper = f32(median + f32(f32(sigma) * f32(mad * f32(1.4826))))
    return select_median(perm[perm < upper], oracle)[0]


def interpolate(cells, w, h, neighbors):
    changes, progress = 0, False
    for y in range(h):
        for x in range(w):
            i = y * w + x
            if not np.isnan(cells[i]):
                continue
            temp = []
            for ox, oy in OFFSETS:
                x2, y2 = x + ox, y + oy
                if 0 <= x2 < w and 0 <= y2 < h and not np.isnan(cells[x2 + y2 * w]):
                    temp.append(cells[x2 + y2 * w])
            pred = median_f32(temp)
            if len(temp) >= neighbors:
                cells[i] = pred
                changes += 1
                progress = progress or not np.isnan(pred)
    return changes, progress


def clip(cells, w, h, n):
    """clip (:175-200) in place: OutlierCells."""
    buf = [f32(c) for c in cells]
    threshold = qselect(buf, len(buf) - n + 1)
    outliers = 0
    for i, c in enumerate(cells):
        if c >= threshold:
            cells[i] = f32(np.nan)
            outliers += 1
    for neighbors in range(8, -1, -1):
        while True:
            changes, progress = interpolate(cells, w, h, neighbors)
            if changes == 0:
                break
            if not progress:        # the same state on every pass from here on
                raise GoHang("clip: interpolate never settles (%d NaN cells, %d neighbours)" % (changes, neighbors))
    return outliers


def gauss3x3(cells, w, h):
    out = []
    for y in range(h):
        for x in range(w):
            s, ws = f32(0), f32(0)
            for oy in (-1, 0, 1):
                for ox in (-1, 0, 1):
                    x2, y2 = x + ox, y + oy
                    if 0 <= x2 < w and 0 <= y2 < h:
                        wt = GAUSS[ox * ox + oy * oy]
                        s = f32(s + f32(cells[x2 + y2 * w] * wt))
                        ws = f32(ws + wt)
            out.append(f32(s / ws))
    return out


def axis_table(n, sp, cells):
    """The state machine of Subtract / Render along one axis: (shifted low cell, fraction) per coordinate."""
    lo, frac = np.zeros(n, np.int64), np.zeros(n, np.float32)
    src_l, src_h = -1, 0
    dest_l = go_i32(f32(f32(-0.5) * sp - f32(0.5)))
    dest_h = go_i32(f32(f32(0.5) * sp + f32(0.5)))
    span = f32(f32(1.0) / f32(dest_h - dest_l))
    for d in range(n):
        if d >= dest_h:
            src_l, src_h = src_h, src_h + 1
            dest_l = dest_h
            dest_h = go_i32(f32(f32(f32(src_h) + f32(0.5)) * sp + f32(0.5)))
            span = f32(f32(1.0) / f32(dest_h - dest_l))
        src = f32(f32(src_l) + f32(f32(d - dest_l) * span))
        l, h = src_l, src_h
        if l < 0:
            l, h = l + 1, h + 1
        if h >= cells:
            l, h = l - 1, h - 1
        lo[d], frac[d] = l, f32(src - f32(l))
    return lo, frac


def render(cells, width, height, cx, cy, spx, spy):
    """Render (:309-384): the background image (Subtract computes the same v)."""
    xl, xr = axis_table(width, spx, cx)
    yl, yr = axis_table(height, spy, cy)
    lo = xl.min() + yl.min() * cx
    hi = xl.max() + yl.max() * cx + cx + 1
    if lo < 0 or hi >= cx * cy:
        raise GoPanic("index %d out of range [%d]" % (lo if lo < 0 else hi, cx * cy))
    c = np.asarray(cells, np.float32)
    idx = yl[:, None] * cx + xl[None, :]
    one_xr = (f32(1) - xr)[None, :]
    xr = xr[None, :]
    vyl = c[idx] * one_xr + c[idx + 1] * xr
    vyh = c[idx + cx] * one_xr + c[idx + 1 + cx] * xr
    return vyl * (f32(1) - yr)[:, None] + vyh * yr[:, None]


def new_background(data, width, height, grid, hfr_factor, sigma, clip_n, stars, oracle):
    """NewBackground (:68-106): (cells, info)."""
    cx, cy, spx, spy = geometry(width, height, grid)
    img = np.asarray(data, np.float32).reshape(height, width)
    stars = [] if stars is None else stars
    bins = bin_stars(stars, cx, cy, spx, spy, hfr_factor)
    hsq = [hfr_sq(s, hfr_factor) for s in stars]
    buf_size = go_i32(f32(spx + f32(1.5))) * go_i32(f32(spy + f32(1.5)))
    cells = []
    for y in range(cy):
        for x in range(cx):
            entries = [(f32(stars[i]["x"]), f32(stars[i]["y"]), hsq[i]) for i in bins[y * cx + x]]
            samples = gather(img, cell_rect(x, y, spx, spy, width, height), entries)
            if samples.size > buf_size:
                raise GoPanic("gatherWithoutStars: index %d out of range [%d]" % (buf_size, buf_size))
            cells.append(f32(fit_cell(samples, sigma, oracle)))
    outliers = clip(cells, cx, cy, clip_n) if clip_n > 0 else 0
    smooth = gauss3x3(cells, cx, cy)
    mn, mx = f32(np.finfo(np.float32).max), f32(-np.finfo(np.float32).max)
    for c in smooth:
        if c < mn:
            mn = c
        if c > mx:
            mx = c
    info = dict(cells_x=cx, cells_y=cy, outlier_cells=outliers, spacing_x=spx, spacing_y=spy, min=mn, max=mx)
    return np.array(smooth, np.float32), info


def back_extract(data, width, height, stars, grid, oracle, hfr_factor=4.0, sigma=1.5, clip_n=0):
    """OpBackExtract.Apply: (out, background, cells, info); grid <= 0 is the no-op (None, None, empty, None)."""
    if grid <= 0:
        return None, None, np.zeros(0, np.float32), None
    with np.errstate(all="ignore"):
        cells, info = new_background(data, width, height, grid, hfr_factor, sigma, clip_n, stars, oracle)
        bg = render(cells, width, height, info["cells_x"], info["cells_y"], info["spacing_x"], info["spacing_y"])
        out = np.asarray(data, np.float32).reshape(height, width) - bg
    return out.reshape(-1), bg.reshape(-1), cells, info
