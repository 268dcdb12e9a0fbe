"""The CPU restatement of include/nlstack_drizzle.h in numpy: the geometry in double, the accumulate step in fp32 with
one rounding per operation in the header's operand order (vectorised over the output pixels, looping over the
candidates in the stated order), the quotient and the rejection.  Also a brute-force gather over ALL source pixels
(the completeness check of the window) and the cases the tests share.  test_drizzle_ref.py pins it by hand."""
import math

import numpy as np

f32 = np.float32
TURBO, POINT = 0, 1
MAX_RADIUS = 3
HALF = f32(0.5)


class GeometryError(ValueError):
    pass


def geometry_double(trans, scale, pixfrac):
    """(F, G, hw, span) in double, before any rounding; span = the argument of the ceil that gives R"""
    a, b, c, d, e, f = [float(f32(v)) for v in trans]
    S, p = float(f32(scale)), float(f32(pixfrac))
    Fa, Fb, Fc, Fd, Fe, Ff = S * a, S * b, S * (c + 0.5) - 0.5, S * d, S * e, S * (f + 0.5) - 0.5
    det = Fa * Fe - Fb * Fd
    with np.errstate(all="ignore"):
        det = np.float64(det)
        Ga, Gb, Gd, Ge = np.float64(Fe) / det, np.float64(-Fb) / det, np.float64(-Fd) / det, np.float64(Fa) / det
        Gc, Gf = -(Ga * Fc + Gb * Ff), -(Gd * Fc + Ge * Ff)
        hw = 0.5 * p * math.sqrt(abs(det))
        reach = 0.5 + hw
        span = max((abs(Ga) + abs(Gb)) * reach, (abs(Gd) + abs(Ge)) * reach) + 0.5 + 1.0 / 64
    return np.array([Fa, Fb, Fc, Fd, Fe, Ff]), np.array([Ga, Gb, Gc, Gd, Ge, Gf]), hw, span


def geometry(trans, scale, pixfrac):
    """(F, G, hw, R) as nl_drizzle_geometry returns them: float32[6], float32[6], float32, int; GeometryError where
    the entry gives NL_ERR_INVALID_ARG"""
    t = np.asarray(trans, f32)
    scale, pixfrac = f32(scale), f32(pixfrac)
    if not (np.isfinite(scale) and scale > 0):
        raise GeometryError("scale")
    if not (pixfrac > 0 and pixfrac <= 1):
        raise GeometryError("pixfrac")
    with np.errstate(all="ignore"):
        eps = f32(t[1] * t[3]) - f32(t[0] * t[4])                      # coord.go:160, fp32
    if eps < f32(1e-8) and -eps < f32(1e-8):
        raise GeometryError("Matrix has no inverse")
    F, G, hw, span = geometry_double(t, scale, pixfrac)
    with np.errstate(all="ignore"):
        F, G, hw = F.astype(f32), G.astype(f32), f32(hw)
    if not (np.all(np.isfinite(F)) and np.all(np.isfinite(G)) and np.isfinite(hw)):
        raise GeometryError("not finite")
    if not math.ceil(span) <= MAX_RADIUS:
        raise GeometryError("radius %d" % math.ceil(span))
    return F, G, hw, int(math.ceil(span))


def _overlap(centre, hw, pix):
    """TURBO's overlap of [centre - hw, centre + hw] with [pix - 0.5, pix + 0.5], the header's comparisons"""
    lo = centre - hw
    e = pix - HALF
    lo = np.where(e > lo, e, lo)
    hi = centre + hw
    e = pix + HALF
    hi = np.where(e < hi, e, hi)
    return hi - lo


def _candidate(F, hw, fi, fj, px, py, weight, kernel):
    """(take, wa) of the source pixels (fi, fj) for the output pixels (px, py), all float32 and broadcastable"""
    u = F[0] * fi + F[1] * fj + F[2]
    vv = F[3] * fi + F[4] * fj + F[5]
    if kernel == POINT:
        take = (np.floor(u + HALF) == px) & (np.floor(vv + HALF) == py)
        return take, np.broadcast_to(f32(weight), take.shape)
    ox, oy = _overlap(u, hw, px), _overlap(vv, hw, py)
    ar = ox * oy
    return (ox > 0) & (oy > 0), f32(weight) * ar


def _centres(G, out_w, row0, rows):
    px = np.arange(out_w, dtype=f32)[None, :]
    py = (row0 + np.arange(rows)).astype(f32)[:, None]
    X = G[0] * px + G[1] * py + G[2]
    Y = G[3] * px + G[4] * py + G[5]
    return px, py, np.floor(X + HALF), np.floor(Y + HALF)


def accumulate(src, trans, scale, pixfrac, out_w, out_h, sum_plane=None, wgt_plane=None, weight=1.0, first=True,
               kernel=TURBO, row0=0, rows=None, radius=None, contributions=None):
    """nl_stack_frame_drizzle_from: (sum, wgt) of the rows [row0, row0 + rows) of the out_w x out_h grid.  radius:
    another window than the geometry's (tests); contributions: a dict that receives {(j, i, row, col): wa} of every
    contribution taken."""
    src = np.asarray(src, f32)
    src_h, src_w = src.shape
    rows = out_h - row0 if rows is None else rows
    F, G, hw, R = geometry(trans, scale, pixfrac)
    R = R if radius is None else radius
    with np.errstate(all="ignore"):
        px, py, xc, yc = _centres(G, out_w, row0, rows)
        if first:
            s, t = np.zeros((rows, out_w), f32), np.zeros((rows, out_w), f32)
        else:
            s, t = np.array(sum_plane, f32).reshape(rows, out_w), np.array(wgt_plane, f32).reshape(rows, out_w)
        # (a NaN gives no candidates; one far outside gives none in the source: clipped so that it stays an integer)
        live = ~(np.isnan(xc) | np.isnan(yc))
        xi = np.clip(np.where(live, xc, -100), -100, src_w + 100).astype(np.int64)
        yi = np.clip(np.where(live, yc, -100), -100, src_h + 100).astype(np.int64)
        for dj in range(-R, R + 1):
            for di in range(-R, R + 1):
                j, i = yi + dj, xi + di
                inside = live & (i >= 0) & (i < src_w) & (j >= 0) & (j < src_h)
                v = src[np.clip(j, 0, src_h - 1), np.clip(i, 0, src_w - 1)]
                take, wa = _candidate(F, hw, i.astype(f32), j.astype(f32), px, py, weight, kernel)
                take = take & inside & ~np.isnan(v)
                s = np.where(take, s + v * wa, s)
                t = np.where(take, t + wa, t)
                if contributions is not None:
                    for r, c in zip(*np.nonzero(take)):
                        contributions[(int(j[r, c]), int(i[r, c]), int(row0 + r), int(c))] = f32(np.broadcast_to(wa, take.shape)[r, c])
    return s, t


def accumulate_brute(src, trans, scale, pixfrac, out_w, out_h, weight=1.0, kernel=TURBO, contributions=None):
    """The same sums over ALL source pixels in the same order (j outer, i inner), no window: what the window of
    radius R must not differ from."""
    src = np.asarray(src, f32)
    src_h, src_w = src.shape
    F, G, hw, _ = geometry(trans, scale, pixfrac)
    with np.errstate(all="ignore"):
        px, py, xc, yc = _centres(G, out_w, 0, out_h)
        live = ~(np.isnan(xc) | np.isnan(yc))
        s, t = np.zeros((out_h, out_w), f32), np.zeros((out_h, out_w), f32)
        for j in range(src_h):
            for i in range(src_w):
                v = src[j, i]
                if np.isnan(v):
                    continue
                take, wa = _candidate(F, hw, f32(i), f32(j), px, py, weight, kernel)
                take = take & live
                s = np.where(take, s + v * wa, s)
                t = np.where(take, t + wa, t)
                if contributions is not None:
                    for r, c in zip(*np.nonzero(take)):
                        contributions[(j, i, int(r), int(c))] = f32(np.broadcast_to(wa, take.shape)[r, c])
    return s, t


def finalize(sum_plane, wgt_plane, min_weight=0.0, empty=np.nan):
    s, w = np.asarray(sum_plane, f32), np.asarray(wgt_plane, f32)
    with np.errstate(all="ignore"):
        return np.where(w > f32(min_weight), s / w, f32(empty)).astype(f32)


def reject_against(frame, model, low, high):
    """(frame with its outliers NaN, n_low, n_high)"""
    v, m = np.asarray(frame, f32), np.asarray(model, f32)
    with np.errstate(all="ignore"):
        d = v - m
        is_low = d < -f32(low)
        is_high = ~is_low & (d > f32(high))
    return np.where(is_low | is_high, f32(np.nan), v), int(is_low.sum()), int(is_high.sum())


# ---- the cases ---------------------------------------------------------------------------------------------------------

def rotation(w, h, degrees, magnification=1.0, dx=0.0, dy=0.0):
    """forward transform: a turn about the centre of a w x h frame, magnified, then shifted"""
    th = math.radians(degrees)
    a, b = magnification * math.cos(th), -magnification * math.sin(th)
    d, e = magnification * math.sin(th), magnification * math.cos(th)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    return np.array([a, b, cx - (a * cx + b * cy) + dx, d, e, cy - (d * cx + e * cy) + dy], f32)


# name -> (w, h) -> forward transform; every test takes its transforms from here
TRANSFORMS = {
    "identity": lambda w, h: np.array([1, 0, 0, 0, 1, 0], f32),
    "shift": lambda w, h: np.array([1, 0, 0.37, 0, 1, -0.21], f32),
    "rot30": lambda w, h: rotation(w, h, 30.0, 1.01, 0.3, -0.4),
    "rot90": lambda w, h: rotation(w, h, 90.0),
    "flip": lambda w, h: np.array([-1, 0, w - 1, 0, 1, 0.25], f32),
    "half-out": lambda w, h: np.array([1, 0, 0.5 * w + 0.3, 0, 1, 0.1], f32),
    "all-out": lambda w, h: np.array([1, 0, 10.0 * w, 0, 1, 0], f32),
}
R3 = ("rot45-m0.9", lambda w, h: rotation(w, h, 45.0, 0.9), 1.0, 1.0)               # R = 3 at S = 1, p = 1
R1 = ("shift-S3-p0.5", TRANSFORMS["shift"], 3.0, 0.5)                                # R = 1: a fine grid, small drops
R4 = ("rot45-m0.3", lambda w, h: rotation(w, h, 45.0, 0.3), 1.0, 1.0)               # R = 4: must raise

# (source w, h) -> (output w, h), S
SHAPES = [((5, 3), (10, 6), 2.0), ((67, 35), (134, 70), 2.0), ((67, 35), (100, 52), 1.5), ((150, 20), (300, 40), 2.0)]
PIXFRACS = (1.0, 0.7, 0.5)


def gpu_cases():
    """(id, transform's name, (w, h), (out_w, out_h), S, p, trans): every shape with every transform, the pixfracs in
    turn, and the R = 3 case on a grid of the source's own size"""
    out = []
    for (w, h), (ow, oh), S in SHAPES:
        for k, (name, make) in enumerate(TRANSFORMS.items()):
            p = PIXFRACS[k % len(PIXFRACS)]
            out.append(("%dx%d-%dx%d-%s-p%g" % (w, h, ow, oh, name, p), name, (w, h), (ow, oh), S, p, make(w, h)))
    name, make, S, p = R3
    out.append(("67x35-67x35-%s" % name, name, (67, 35), (67, 35), S, p, make(67, 35)))
    name, make, S, p = R1
    out.append(("67x35-201x105-%s" % name, name, (67, 35), (201, 105), S, p, make(67, 35)))
    return out


def source(w, h, seed, holes=True):
    """a frame of positive noise with, if holes, a few NaN and one +Inf and -Inf (where the frame is large enough)"""
    rng = np.random.default_rng(seed)
    a = (0.1 + rng.random((h, w))).astype(f32)
    if holes:
        flat = a.reshape(-1)
        idx = rng.choice(flat.size, size=min(5, flat.size // 3), replace=False)
        flat[idx[:-2]] = np.nan
        flat[idx[-2]] = np.inf
        flat[idx[-1]] = -np.inf
    return a


def same(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a, f32).reshape(-1), np.asarray(b, f32).reshape(-1)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
