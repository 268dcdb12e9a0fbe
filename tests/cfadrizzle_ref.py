"""The CPU restatement of include/nlstack_cfadrizzle.h on top of drizzle_ref.py and bayer_ref.py (both unchanged): a
channel's pixels are the pixels of CosmeticCorrectionBayer's walk (bayer_ref.channel_rows), and the CFA drizzle of a
mosaic is the mono drizzle of a copy whose other pixels are NaN.  Also a numpy walk strided exactly as the kernel
(drizzle_cfa.hip) strides its window, which test_cfadrizzle_ref.py holds against the masked full window, the transform
of the mosaic in double, and the cases the tests share.  No tests in here."""
import numpy as np

import bayer_ref
import drizzle_ref as ref

f32 = np.float32
CFAS = ["RGGB", "GRBG", "GBRG", "BGGR"]
CHANNELS = ["R", "G", "B"]
PAIRS = [(ch, cfa) for cfa in CFAS for ch in CHANNELS]                        # the 12 channel x CFA pairs


def channel_mask(w, h, channel, cfa):
    """bool (h, w): the pixels of `channel` of a w x h `cfa` mosaic"""
    ch, xo, yo = bayer_ref.parse(channel, cfa)
    mask = np.zeros((h, w), bool)
    for y, x0, _ in bayer_ref.channel_rows(w, h, ch, xo, yo):
        mask[y, x0::2] = True
    return mask


def masked(src, channel, cfa):
    """the mosaic with every pixel of another channel (or none) NaN"""
    src = np.asarray(src, f32)
    return np.where(channel_mask(src.shape[1], src.shape[0], channel, cfa), src, f32(np.nan)).astype(f32)


def accumulate_cfa(src, trans, scale, pixfrac, out_w, out_h, channel, cfa, **kw):
    """nl_stack_frame_drizzle_cfa_from: drizzle_ref.accumulate of the masked mosaic"""
    return ref.accumulate(masked(src, channel, cfa), trans, scale, pixfrac, out_w, out_h, **kw)


def reject_against_cfa(frame, model, channel, cfa, low, high):
    """(mosaic with the channel's outliers NaN, n_low, n_high); frame and model are (h, w)"""
    v, m = np.asarray(frame, f32), np.asarray(model, f32)
    mask = channel_mask(v.shape[1], v.shape[0], channel, cfa)
    with np.errstate(all="ignore"):
        d = v - m
        is_low = mask & (d < -f32(low))
        is_high = mask & ~is_low & (d > f32(high))
    return np.where(is_low | is_high, f32(np.nan), v), int(is_low.sum()), int(is_high.sum())


def cfa_transform_double(trans, cfa):
    """nl_drizzle_cfa_transform before its one rounding: T(i - xo, j - yo) in double"""
    a, b, c, d, e, f = [float(f32(v)) for v in trans]
    xo, yo = bayer_ref.offsets(cfa)
    return np.array([a, b, c - a * xo - b * yo, d, e, f - d * xo - e * yo], np.float64)


def cfa_transform(trans, cfa):
    return cfa_transform_double(trans, cfa).astype(f32)


def accumulate_strided(src, trans, scale, pixfrac, out_w, out_h, channel, cfa, weight=1.0, kernel=ref.TURBO,
                       contributions=None):
    """The kernel's walk: of the window of radius R around (xi, yi) only the channel's positions -- R and B from the
    first row / column of the window with the channel's parity in steps of 2, R + 1 steps; G every row, in row j from
    the first column of the parity the row asks for.  Parities with & 1 (window starts are negative at the frame's
    edge).  A step past the window, outside the source or in front of (xo, yo) is no candidate."""
    src = np.asarray(src, f32)
    src_h, src_w = src.shape
    ch, xo, yo = bayer_ref.parse(channel, cfa)
    F, G, hw, R = ref.geometry(trans, scale, pixfrac)
    green = ch == "G"
    if green:
        par_x, par_y = (xo + yo + 1) & 1, 0
    else:
        b = 1 if ch == "B" else 0
        par_x, par_y = (xo + b) & 1, (yo + b) & 1
    with np.errstate(all="ignore"):
        px, py, xc, yc = ref._centres(G, out_w, 0, out_h)
        s, t = np.zeros((out_h, out_w), f32), np.zeros((out_h, out_w), f32)
        live = ~(np.isnan(xc) | np.isnan(yc))
        xi = np.clip(np.where(live, xc, -100), -100, src_w + 100).astype(np.int64)
        yi = np.clip(np.where(live, yc, -100), -100, src_h + 100).astype(np.int64)
        wx, wy = xi - R, yi - R
        for dj in range(2 * R + 1 if green else R + 1):
            j = wy + dj if green else wy + ((wy ^ par_y) & 1) + 2 * dj
            i_first = wx + ((wx ^ j ^ par_x) & 1) if green else wx + ((wx ^ par_x) & 1)
            for di in range(R + 1):
                i = i_first + 2 * di
                inside = live & (i <= xi + R) & (j <= yi + R) & (i >= xo) & (j >= yo) & (i < src_w) & (j < src_h)
                v = src[np.clip(j, 0, src_h - 1), np.clip(i, 0, src_w - 1)]
                take, wa = ref._candidate(F, hw, i.astype(f32), j.astype(f32), px, py, weight, kernel)
                take = take & inside & ~np.isnan(v)
                s = np.where(take, s + v * wa, s)
                t = np.where(take, t + wa, t)
                if contributions is not None:
                    for r, c in zip(*np.nonzero(take)):
                        contributions[(int(j[r, c]), int(i[r, c]), int(r), int(c))] = f32(np.broadcast_to(wa, take.shape)[r, c])
    return s, t


def per_pixel(contributions):
    """{(row, col): [(j, i, wa), ...]} in the order the contributions were taken"""
    out = {}
    for (j, i, r, c), wa in contributions.items():
        out.setdefault((r, c), []).append((j, i, wa))
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------

def rotation_cases():
    """every case of drizzle_ref.gpu_cases() with the 12 pairs taken in rotation: (case, channel, cfa)"""
    return [(case, ) + PAIRS[k % len(PAIRS)] for k, case in enumerate(ref.gpu_cases())]


def pair_cases():
    """all 12 pairs on 7x5 -> 14x10 and on 67x35 -> 134x70 under `shift` and `rot30`, the pixfracs in turn"""
    out = []
    for (w, h), (ow, oh) in (((7, 5), (14, 10)), ((67, 35), (134, 70))):
        for name in ("shift", "rot30"):
            for k, (ch, cfa) in enumerate(PAIRS):
                p = ref.PIXFRACS[k % len(ref.PIXFRACS)]
                case = ("%dx%d-%dx%d-%s-p%g" % (w, h, ow, oh, name, p), name, (w, h), (ow, oh), 2.0, p,
                        ref.TRANSFORMS[name](w, h))
                out.append((case, ch, cfa))
    return out


def case_id(entry):
    case, ch, cfa = entry
    return "%s-%s-%s" % (case[0], ch, cfa)
