"""Checker of the bicubic / Lanczos-3 resampling of the resident projection (include/nlstack_resample.h): the header's
definition restated in numpy, fp32.

The wide kernels are an extension -- the reference's Image.Project resamples bilinearly -- so there is no oracle for
them.  tests/test_resample_ref.py holds this restatement to the CPU oracle where there is one (the bilinear kernel, the
fallback ring, the set of pixels out of bounds) and to the properties the definition promises everywhere else.

Vectorised over the destination's pixels: every array operation below is ONE fp32 operation per pixel (numpy rounds
float32 op float32 to float32 and never fuses a multiply with an add), the loops run over the taps, so each pixel's
sums are sequential, left to right.  The Lanczos-3 table is an argument: the GPU tests pass the library's own, the
results are bit-exact given the table."""
import collections

import numpy as np

F = np.float32
BILINEAR, BICUBIC, LANCZOS3 = range(3)
PHASES = 1024
RADIUS = {BILINEAR: 1, BICUBIC: 2, LANCZOS3: 3}

# out: the resampled frame [dw * dh]; ok: the 2x2 footprint fits (not out_of_bounds); wide: the wide footprint fits;
# lo / hi: the clamp's range of every pixel (the four central taps; meaningless outside ok)
Result = collections.namedtuple("Result", "out ok wide lo hi")


def invert(trans):
    """Transform2D.Invert (internal/star/coord.go:159-199), fp32 as written there; None: no inverse."""
    A, B, C, D, E, Fq = [F(v) for v in trans]
    bd, ae = F(B * D), F(A * E)
    eps = F(bd - ae)
    if eps < F(1e-8) and -eps < F(1e-8):
        return None
    den1, den2 = F(bd - ae), F(ae - bd)
    with np.errstate(all="ignore"):
        return [F(-E / den1), F(B / den1), F(F(F(C * E) - F(B * Fq)) / den1),
                F(-D / den2), F(A / den2), F(F(F(C * D) - F(A * Fq)) / den2)]


def lanczos3_table():
    """The header's table from a float64 numpy evaluation (the library's goes through libm: 1 ulp apart at most)."""
    q = np.arange(PHASES, dtype=np.float64)[:, None] / PHASES
    x = q - (np.arange(6, dtype=np.float64)[None, :] - 2.0)
    with np.errstate(all="ignore"):
        w = 3.0 * np.sin(np.pi * x) * np.sin(np.pi * x / 3.0) / (np.pi * np.pi * x * x)
    w[x == np.floor(x)] = 0.0
    w[x == 0.0] = 1.0
    return (w / w.sum(1, keepdims=True)).astype(F)


def bicubic_weights(t):
    """Keys, a = -0.5, the header's Horner forms; t float32 array -> four float32 arrays"""
    h, one = F(0.5), F(1.0)
    return [((-h * t + one) * t - h) * t,
            (F(1.5) * t - F(2.5)) * t * t + one,
            ((F(-1.5) * t + F(2.0)) * t + h) * t,
            (h * t - h) * t * t]


def resample(src, src_w, src_h, dst_w, dst_h, trans, out_of_bounds, kernel, clamp=False, table=None):
    """The definition for every destination pixel -> Result (arrays over the dst_w * dst_h pixels, row-major)."""
    R = RADIUS[kernel]
    inv = invert(trans)
    assert inv is not None
    src = np.ascontiguousarray(src, F).reshape(-1)
    px = np.tile(np.arange(dst_w, dtype=F), dst_h)
    py = np.repeat(np.arange(dst_h, dtype=F), dst_w)
    with np.errstate(all="ignore"):
        X = inv[0] * px + inv[1] * py + inv[2]                       # coord.go:142, left to right
        Y = inv[3] * px + inv[4] * py + inv[5]
        fx, fy = np.floor(X), np.floor(Y)
        ok = (fx >= 0) & (fy >= 0) & (fx < F(2147483520.0)) & (fy < F(2147483520.0))
        xl = np.where(ok, fx, 0).astype(np.int64)
        yl = np.where(ok, fy, 0).astype(np.int64)
        ok &= (xl + 1 < src_w) & (yl + 1 < src_h)
        xl, yl = np.where(ok, xl, 0), np.where(ok, yl, 0)
        xr = np.where(ok, X - xl.astype(F), F(0)).astype(F)      # exact, in [0, 1)
        yr = np.where(ok, Y - yl.astype(F), F(0)).astype(F)
        wide = ok & (xl - (R - 1) >= 0) & (xl + R <= src_w - 1) & (yl - (R - 1) >= 0) & (yl + R <= src_h - 1)

        def tap(dx, dy, where):                                      # source pixel (xl + dx, yl + dy) where `where`, else pixel 0
            return src[np.where(where, (yl + dy) * src_w + xl + dx, 0)]

        t00, t01, t10, t11 = tap(0, 0, ok), tap(1, 0, ok), tap(0, 1, ok), tap(1, 1, ok)
        omx, omy = F(1) - xr, F(1) - yr
        vyl = t00 * omx + t01 * xr                                   # project.go:68
        vyh = t10 * omx + t11 * xr
        bilinear = vyl * omy + vyh * yr                              # project.go:70
        lo, hi = t00.copy(), t00.copy()
        for t in (t01, t10, t11):
            lo = np.where(t < lo, t, lo)
        for t in (t01, t10, t11):
            hi = np.where(t > hi, t, hi)
        out = bilinear
        if R > 1:
            if kernel == BICUBIC:
                wx, wy = bicubic_weights(xr), bicubic_weights(yr)
            else:
                table = np.ascontiguousarray(table, F).reshape(PHASES, 6)
                qx, qy = (xr * F(PHASES)).astype(np.int64), (yr * F(PHASES)).astype(np.int64)
                assert qx.max() <= PHASES - 1 and qy.max() <= PHASES - 1
                wx, wy = [table[qx, i] for i in range(6)], [table[qy, i] for i in range(6)]
            v = None
            for j in range(2 * R):
                r = tap(-(R - 1), j - (R - 1), wide) * wx[0]
                for i in range(1, 2 * R):
                    r = r + tap(i - (R - 1), j - (R - 1), wide) * wx[i]
                v = r * wy[0] if j == 0 else v + r * wy[j]
            if clamp:
                v = np.where(v < lo, lo, v)
                v = np.where(v > hi, hi, v)
            out = np.where(wide, v, bilinear)
        out = np.where(ok, out, F(out_of_bounds)).astype(F)
    for a in (out, ok, wide, lo, hi):
        a.flags.writeable = False
    return Result(out, ok, wide, lo, hi)


# ---- the cases the CPU self-check and the GPU tests share: those of tests/test_gpu_project_resident.py plus 7x7 -> 7x7,
# the smallest square with wide pixels for both kernels (2x2 for Lanczos-3, 4x4 for bicubic under the identity)

def cases():
    """(SHAPES, transform(shape, name), TRANSFORMS, BEST_POSSIBLE) with the 7x7 shape added to the existing test's"""
    import test_gpu_project_resident as base
    shapes = dict(base.SHAPES, **{"7x7": (7, 7, 7, 7)})
    # offsets moved as there (the linear part and the offset's fractional part kept) where the literal transform
    # leaves less than a quarter of the 7x7 destination in bounds; found with this checker alone
    moved = dict(base.MOVED)
    moved.update({("7x7", "small_rot"): [0.999, 0.03, -0.2, -0.03, 0.999, -0.3], ("7x7", "rot90"): [0, -1, 6, 1, 0, 0],
                  ("7x7", "rot180"): [-1, 0, 6, 0, -1, 6]})
    best = dict(base.BEST_POSSIBLE)
    best["7x7", "half"] = 3 * 3                                      # floor((7 - 1) / 2) squared, as argued there
    return shapes, (lambda shape, name: moved.get((shape, name), base.TRANSFORMS[name])), base.TRANSFORMS, best
