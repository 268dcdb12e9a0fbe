"""The CPU restatement of include/nlstack_sqdrizzle.h in numpy, on top of drizzle_ref.py and cfadrizzle_ref.py (both
unchanged: the centres, the transforms, the cases, `same` and the channel masks are theirs): the geometry in double, the
accumulate step in fp32 with one rounding per operation in the header's operand order and np.where for its branches, a
brute-force gather over ALL source pixels (the completeness check of the window), the CFA form (the mono function on the
masked copy), and a float64 Sutherland-Hodgman clip as the independent yardstick of the areas.  test_sqdrizzle_ref.py
pins it by hand.  No tests in here."""
import math

import numpy as np

import cfadrizzle_ref as cref
import drizzle_ref as ref

f32 = np.float32
ZERO, HALF, ONE = f32(0.0), f32(0.5), f32(1.0)


def geometry_square_double(trans, scale, pixfrac):
    """(F, G, corners (4, 2), (bx, by), span) in double, before any rounding; span = the argument of the ceil that
    gives R"""
    F, G, _, _ = ref.geometry_double(trans, scale, pixfrac)
    Fa, Fb, _, Fd, Fe, _ = [float(v) for v in F]
    h = float(f32(pixfrac)) / 2
    det = Fa * Fe - Fb * Fd
    offsets = [(-h, -h), (-h, h), (h, h), (h, -h)]
    if det < 0:
        offsets.reverse()
    corners = np.array([[Fa * ox + Fb * oy, Fd * ox + Fe * oy] for ox, oy in offsets], np.float64)
    bx, by = h * (abs(Fa) + abs(Fb)), h * (abs(Fd) + abs(Fe))
    reach_x, reach_y = 0.5 + bx, 0.5 + by
    with np.errstate(all="ignore"):
        span = max(abs(G[0]) * reach_x + abs(G[1]) * reach_y, abs(G[3]) * reach_x + abs(G[4]) * reach_y) + 0.5 + 1.0 / 64
    return F, G, corners, np.array([bx, by], np.float64), span


def geometry_square(trans, scale, pixfrac):
    """(F, G, corners, box, R) as nl_drizzle_square_geometry returns them: float32[6], float32[6], float32[4][2],
    float32[2], int; drizzle_ref.GeometryError where the entry gives NL_ERR_INVALID_ARG"""
    t = np.asarray(trans, f32)
    scale, pixfrac = f32(scale), f32(pixfrac)
    if not (np.isfinite(scale) and scale > 0):
        raise ref.GeometryError("scale")
    if not (pixfrac > 0 and pixfrac <= 1):
        raise ref.GeometryError("pixfrac")
    with np.errstate(all="ignore"):
        eps = f32(t[1] * t[3]) - f32(t[0] * t[4])                      # coord.go:160, fp32
    if eps < f32(1e-8) and -eps < f32(1e-8):
        raise ref.GeometryError("Matrix has no inverse")
    F, G, corners, box, span = geometry_square_double(t, scale, pixfrac)
    with np.errstate(all="ignore"):
        F, G, corners, box = F.astype(f32), G.astype(f32), corners.astype(f32), box.astype(f32)
    if not all(np.all(np.isfinite(a)) for a in (F, G, corners, box)):
        raise ref.GeometryError("not finite")
    if not math.ceil(span) <= ref.MAX_RADIUS:
        raise ref.GeometryError("radius %d" % math.ceil(span))
    return F, G, corners, box, int(math.ceil(span))


def edge(x1, y1, x2, y2):
    """the header's edge(): the signed area between the segment and the x-axis inside the unit square; float32 arrays
    of one shape, every path computed and selected"""
    with np.errstate(all="ignore"):
        dx, dy = x2 - x1, y2 - y1
        back = dx < 0
        xlo, xhi = np.where(back, x2, x1), np.where(back, x1, x2)
        none = (dx == 0) | (xlo >= 1) | (xhi <= 0)
        xlo = np.where(xlo < 0, ZERO, xlo)
        xhi = np.where(xhi > 1, ONE, xhi)
        m = dy / dx
        c = y1 - m * x1
        ylo, yhi = m * xlo + c, m * xhi + c
        below = (ylo <= 0) & (yhi <= 0)
        sg = np.where(back, -ONE, ONE)
        above = (ylo >= 1) & (yhi >= 1)
        whole = sg * (xhi - xlo)
        det = x1 * y2 - y1 * x2
        x_axis = det / dy
        low = ylo < 0
        ylo, xlo = np.where(low, ZERO, ylo), np.where(low, x_axis, xlo)
        low = yhi < 0
        yhi, xhi = np.where(low, ZERO, yhi), np.where(low, x_axis, xhi)
        xtop = (dx + det) / dy
        inside = sg * ((HALF * (xhi - xlo)) * (yhi + ylo))
        leaves = sg * ((HALF * (xtop - xlo)) * (ONE + ylo) + (xhi - xtop))
        enters = sg * ((HALF * (xhi - xtop)) * (ONE + yhi) + (xtop - xlo))
        part = np.where(ylo <= 1, np.where(yhi <= 1, inside, leaves), enters)
        out = np.where(none | below, ZERO, np.where(above, whole, part))
    assert out.dtype == f32
    return out


def vertices(ux, vy, corners):
    """(x, y), each (..., 4): the corners of the drops whose centres are (ux, vy) relative to the pixel (float32
    arrays), the pixel being the unit square"""
    return (np.stack([(ux + corners[k, 0]) + HALF for k in range(4)], axis=-1),
            np.stack([(vy + corners[k, 1]) + HALF for k in range(4)], axis=-1))


def area(ux, vy, corners):
    """ar of those drops: the four edges in order"""
    x, y = vertices(ux, vy, corners)
    e = [edge(x[..., k], y[..., k], x[..., (k + 1) % 4], y[..., (k + 1) % 4]) for k in range(4)]
    return ((e[0] + e[1]) + e[2]) + e[3]


def _candidate(F, corners, box, fi, fj, px, py, weight, prefilter=True):
    """(take, wa, ar) of the source pixels (fi, fj) for the output pixels (px, py), all float32 and broadcastable.  The
    edges are evaluated only where the bounding-box test passes (what fails is skipped either way); prefilter=False
    evaluates them everywhere and tests nothing in front (the tests of the areas)."""
    u = F[0] * fi + F[1] * fj + F[2]
    vv = F[3] * fi + F[4] * fj + F[5]
    ox, oy = ref._overlap(u, box[0], px), ref._overlap(vv, box[1], py)
    boxed = np.broadcast_to((ox > 0) & (oy > 0), np.broadcast(ox, oy).shape)
    if not prefilter:
        boxed = np.ones(boxed.shape, bool)
    ux, vy = np.broadcast_to(u - px, boxed.shape), np.broadcast_to(vv - py, boxed.shape)
    ar = np.zeros(boxed.shape, f32)
    if boxed.any():
        ar[boxed] = area(ux[boxed].astype(f32), vy[boxed].astype(f32), corners)
    return boxed & (ar > 0), f32(weight) * ar, ar


def accumulate_square(src, trans, scale, pixfrac, out_w, out_h, sum_plane=None, wgt_plane=None, weight=1.0, first=True,
                      row0=0, rows=None, radius=None, contributions=None):
    """nl_stack_frame_drizzle_square_from: (sum, wgt) of the rows [row0, row0 + rows) of the out_w x out_h grid.
    radius: another window than the geometry's (tests); contributions: a dict that receives {(j, i, row, col): wa} of
    every contribution taken."""
    src = np.asarray(src, f32)
    src_h, src_w = src.shape
    rows = out_h - row0 if rows is None else rows
    F, G, corners, box, R = geometry_square(trans, scale, pixfrac)
    R = R if radius is None else radius
    with np.errstate(all="ignore"):
        px, py, xc, yc = ref._centres(G, out_w, row0, rows)
        if first:
            s, t = np.zeros((rows, out_w), f32), np.zeros((rows, out_w), f32)
        else:
            s, t = np.array(sum_plane, f32).reshape(rows, out_w), np.array(wgt_plane, f32).reshape(rows, out_w)
        live = ~(np.isnan(xc) | np.isnan(yc))
        xi = np.clip(np.where(live, xc, -100), -100, src_w + 100).astype(np.int64)
        yi = np.clip(np.where(live, yc, -100), -100, src_h + 100).astype(np.int64)
        for dj in range(-R, R + 1):
            for di in range(-R, R + 1):
                j, i = yi + dj, xi + di
                inside = live & (i >= 0) & (i < src_w) & (j >= 0) & (j < src_h)
                v = src[np.clip(j, 0, src_h - 1), np.clip(i, 0, src_w - 1)]
                take, wa, _ = _candidate(F, corners, box, i.astype(f32), j.astype(f32), px, py, weight)
                take = take & inside & ~np.isnan(v)
                s = np.where(take, s + v * wa, s)
                t = np.where(take, t + wa, t)
                if contributions is not None:
                    for r, c in zip(*np.nonzero(take)):
                        contributions[(int(j[r, c]), int(i[r, c]), int(row0 + r), int(c))] = f32(wa[r, c])
    return s, t


def accumulate_square_brute(src, trans, scale, pixfrac, out_w, out_h, weight=1.0, contributions=None):
    """The same sums over ALL source pixels in the same order (j outer, i inner), no window: what the window of radius
    R must not differ from."""
    src = np.asarray(src, f32)
    src_h, src_w = src.shape
    F, G, corners, box, _ = geometry_square(trans, scale, pixfrac)
    with np.errstate(all="ignore"):
        px, py, xc, yc = ref._centres(G, out_w, 0, out_h)
        live = ~(np.isnan(xc) | np.isnan(yc))
        s, t = np.zeros((out_h, out_w), f32), np.zeros((out_h, out_w), f32)
        for j in range(src_h):
            for i in range(src_w):
                v = src[j, i]
                if np.isnan(v):
                    continue
                take, wa, _ = _candidate(F, corners, box, f32(i), f32(j), px, py, weight)
                take = take & live
                s = np.where(take, s + v * wa, s)
                t = np.where(take, t + wa, t)
                if contributions is not None:
                    for r, c in zip(*np.nonzero(take)):
                        contributions[(j, i, int(r), int(c))] = f32(wa[r, c])
    return s, t


def accumulate_square_cfa(src, trans, scale, pixfrac, out_w, out_h, channel, cfa, **kw):
    """nl_stack_frame_drizzle_square_cfa_from: accumulate_square of the masked mosaic"""
    return accumulate_square(cref.masked(src, channel, cfa), trans, scale, pixfrac, out_w, out_h, **kw)


# ---- the independent yardstick of the areas ----------------------------------------------------------------------------

def _clip(X, Y, cnt, axis, bound, keep_below):
    """one Sutherland-Hodgman step on n polygons at once: X, Y (n, K) vertices, cnt (n,) how many of them count"""
    n, K = X.shape
    rows = np.arange(n)
    out_x, out_y, pos = np.zeros((n, K)), np.zeros((n, K)), np.zeros(n, np.int64)
    for k in range(K):
        active = k < cnt
        prev = np.where(k == 0, np.maximum(cnt - 1, 0), k - 1)
        ax, ay, bx, by = X[rows, prev], Y[rows, prev], X[:, k], Y[:, k]
        a_c, b_c = (ax, ay)[axis], (bx, by)[axis]
        a_in = a_c <= bound if keep_below else a_c >= bound
        b_in = b_c <= bound if keep_below else b_c >= bound
        with np.errstate(all="ignore"):
            f = (bound - a_c) / (b_c - a_c)
            cx, cy = ax + f * (bx - ax), ay + f * (by - ay)
        if axis == 0:
            cx = np.full(n, bound)
        else:
            cy = np.full(n, bound)
        for emit, ex, ey in ((active & (a_in != b_in), cx, cy), (active & b_in, bx, by)):
            at = np.nonzero(emit)[0]
            out_x[at, pos[at]], out_y[at, pos[at]] = ex[at], ey[at]
            pos[at] += 1
    return out_x, out_y, pos


def exact_overlap(poly):
    """the area of convex polygons (float64 vertices (4, 2) or (n, 4, 2), either orientation) inside the unit square
    [0, 1]^2: Sutherland-Hodgman against the four sides, then the shoelace sum, all in float64; a float or (n,)"""
    P = np.asarray(poly, np.float64)
    single = P.ndim == 2
    P = P.reshape(-1, P.shape[-2], 2)
    n, K = P.shape[0], P.shape[1] + 6                       # (a side adds at most one vertex to a convex polygon)
    X, Y = np.zeros((n, K)), np.zeros((n, K))
    X[:, :P.shape[1]], Y[:, :P.shape[1]] = P[:, :, 0], P[:, :, 1]
    cnt = np.full(n, P.shape[1], np.int64)
    for axis, bound, keep_below in ((0, 0.0, False), (0, 1.0, True), (1, 0.0, False), (1, 1.0, True)):
        X, Y, cnt = _clip(X, Y, cnt, axis, bound, keep_below)
    rows = np.arange(n)
    twice = np.zeros(n)
    for k in range(K):
        prev = np.where(k == 0, np.maximum(cnt - 1, 0), k - 1)
        twice += np.where(k < cnt, X[rows, prev] * Y[:, k] - X[:, k] * Y[rows, prev], 0.0)
    out = np.abs(twice) / 2
    return float(out[0]) if single else out


def drop_polygon(F, corners, fi, fj, px, py):
    """the drops of the source pixels (fi, fj) relative to the output pixels (px, py) as exact_overlap takes them,
    (..., 4, 2) float64: the corner coordinates x_k, y_k of the definition, which are fp32 values.  (The yardstick is
    one of the areas: what the rounding of u and vv at a coordinate of some hundreds moves, up to half an ulp of the
    coordinate, belongs to the definition, as it does for NL_DZ_TURBO.)"""
    u = F[0] * fi + F[1] * fj + F[2]
    vv = F[3] * fi + F[4] * fj + F[5]
    x, y = vertices(u - px, vv - py, corners)
    assert x.dtype == f32 and y.dtype == f32
    return np.stack([x.astype(np.float64), y.astype(np.float64)], axis=-1)


# ---- the cases ---------------------------------------------------------------------------------------------------------

R4_SQUARE = ("rot45-m0.45", lambda w, h: ref.rotation(w, h, 45.0, 0.45), 1.0, 1.0)  # turbo R = 3, square R = 4


def turn_cases():
    """67x35 -> 134x70 under turns of 13 and 45 degrees, in the form of drizzle_ref.gpu_cases()"""
    out = []
    for deg, p in ((13.0, 0.7), (45.0, 1.0)):
        name = "rot%g" % deg
        out.append(("67x35-134x70-%s-p%g" % (name, p), name, (67, 35), (134, 70), 2.0, p,
                    ref.rotation(67, 35, deg, 0.99, -0.2, 0.45)))
    return out


def gpu_cases():
    """every case the device tests of the square drizzle run: drizzle_ref.gpu_cases() and the two turns"""
    return ref.gpu_cases() + turn_cases()
