/* nlstack_sqdrizzle.h -- the square drizzle kernel: the exact overlap of a drop with an output pixel under any
 * rotation, for mono frames and for one channel of a raw Bayer mosaic, entries of the C ABI of libnlstack.so.  AN
 * EXTENSION: the reference has no drizzle.  Part of nlstack.h, which includes it behind nlstack_cfadrizzle.h: include
 * nlstack.h, not this file. */
#ifndef NLSTACK_SQDRIZZLE_H
#define NLSTACK_SQDRIZZLE_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- square drizzle (labelled extension) ----
 * NL_DZ_TURBO of nlstack_drizzle.h lays down an axis-aligned drop: the right area, the wrong shape under any rotation
 * that is no quarter turn, so that the weight plane carries a pattern of over- and under-covered pixels which the
 * quotient only partly cancels.  Field rotation is the normal case (an alt-az mount, a meridian flip, a mosaic panel).
 * The drizzle literature's "square" kernel takes the drop for what it is, the image of the shrunken pixel under the
 * transform, and lays its flux down in proportion to the exact area of its overlap with each output pixel.  These
 * entries are that kernel; they close the item "the rotated-square kernel" that nlstack_drizzle.h leaves for a later
 * change.  They are entries of their own, not a third value of `kernel`: nl_stack_frame_drizzle_from and
 * nl_stack_frame_drizzle_cfa_from keep their two.  nl_stack_drizzle_finalize, nl_stack_frame_reject_against(_cfa) and
 * nl_stack_frame_badpixel_cfa serve the square drizzle as they are.  There is no reference to compare with: this
 * text, on top of nlstack_drizzle.h's, is the contract.
 *
 * Definition.  Geometry (nl_drizzle_square_geometry, host, in double).  trans, S = scale, p = pixfrac, F, G and det
 * are nl_drizzle_geometry's.  Let h = p/2.
 *   The drop of source pixel (i, j) is the image under F of the square of side p around its centre: a parallelogram,
 *   a rotated square for a similarity.  Its corners relative to its centre (u, vv) = F(i, j) are
 *     c_k = (cx_k, cy_k) = (Fa*ox_k + Fb*oy_k, Fd*ox_k + Fe*oy_k)          k = 0..3
 *   with the offsets  o_0 = (-h, -h)   o_1 = (-h, +h)   o_2 = (+h, +h)   o_3 = (+h, -h).
 *   When det < 0 the order is reversed (o_3, o_2, o_1, o_0), so that the edge sum below comes out positive for
 *   either orientation.
 *   bx = h*(|Fa| + |Fb|)   by = h*(|Fd| + |Fe|)          the half-sides of the drop's bounding box
 *   reach_x = 0.5 + bx     reach_y = 0.5 + by
 *   R = (int)ceil( max(|Ga|*reach_x + |Gb|*reach_y, |Gd|*reach_x + |Ge|*reach_y) + 0.5 + 1.0/64 )
 * F, G, the eight corner coordinates, bx and by are rounded to fp32 once, at the end.  R is the radius of the window
 * that holds every source pixel whose drop's bounding box can touch an output pixel: the two overlap only if their
 * centres are closer than reach_x in x and reach_y in y, which G maps to less than |Ga|*reach_x + |Gb|*reach_y source
 * columns; rounding the position adds 0.5, and 1/64 covers the fp32 rounding as in nl_drizzle_geometry.  A rotated
 * drop reaches further than NL_DZ_TURBO's: R is larger for some transforms.  R > NL_DZ_MAX_RADIUS is
 * nl_drizzle_geometry's error with its wording.
 *
 * Accumulate (nl_stack_frame_drizzle_square_from): the text of nl_stack_frame_drizzle_from in nlstack_drizzle.h, word
 * for word -- X, Y, xc, yc, `first`, the window of radius R, rows outer and columns inner, skipping j, i outside the
 * source, NaN as no data (+-Inf takes part), s = s + v*wa ; t = t + wa, fp32, never fused, operands in the order
 * written -- except for a candidate's weight:
 *       u = F.a*i + F.b*j + F.c ;  vv = F.d*i + F.e*j + F.f                  (as before)
 *       the bounding-box test: ox from (u, bx, col) and oy from (vv, by, row), by the two clamps and the subtraction
 *       of NL_DZ_TURBO (bx, by in the place of hw);  skip unless ox > 0 and oy > 0
 *       ux = u - col ;  vy = vv - row
 *       x_k = (ux + cx_k) + 0.5f ;  y_k = (vy + cy_k) + 0.5f      k = 0..3   (the pixel is the unit square [0,1]^2)
 *       ar = ((E(0,1) + E(1,2)) + E(2,3)) + E(3,0)          E(k,l) = edge(x_k, y_k, x_l, y_l), added in this order
 *       skip unless ar > 0 ;  wa = weight*ar
 * edge is the signed area between a segment and the x-axis inside the unit square (the sgarea / boxer scheme of the
 * drizzle literature):
 *   edge(x1, y1, x2, y2):
 *     dx = x2 - x1 ;  dy = y2 - y1
 *     if dx == 0: return +0
 *     (xlo, xhi) = dx < 0 ? (x2, x1) : (x1, x2)
 *     if xlo >= 1 or xhi <= 0: return +0
 *     if xlo < 0: xlo = 0 ;  if xhi > 1: xhi = 1
 *     m = dy/dx ;  c = y1 - m*x1 ;  ylo = m*xlo + c ;  yhi = m*xhi + c
 *     if ylo <= 0 and yhi <= 0: return +0
 *     sg = dx < 0 ? -1 : +1
 *     if ylo >= 1 and yhi >= 1: return sg*(xhi - xlo)
 *     det = x1*y2 - y1*x2
 *     if ylo < 0: ylo = 0, xlo = det/dy
 *     if yhi < 0: yhi = 0, xhi = det/dy
 *     if ylo <= 1:
 *         if yhi <= 1: return sg*((0.5f*(xhi - xlo))*(yhi + ylo))
 *         xtop = (dx + det)/dy ;  return sg*((0.5f*(xtop - xlo))*(1 + ylo) + (xhi - xtop))
 *     xtop = (dx + det)/dy ;      return sg*((0.5f*(xhi - xtop))*(1 + yhi) + (xtop - xlo))
 * Division is IEEE.  A value computed on a path not taken is discarded, so an implementation may compute every path
 * and select.  The gather form as before: no atomics, a fixed candidate order, bit for bit what the numpy restatement
 * of this text gives.
 *
 * Noise property.  The areas are exact up to fp32 rounding, about 1e-7 absolute.  A drop whose bounding box overlaps
 * a pixel it does not touch may therefore lay down an area of rounding size (a rounding-sized negative one is skipped
 * by "ar > 0").  For axis-aligned transforms the areas agree with NL_DZ_TURBO's to rounding; the two are not bit-equal.
 *
 * The CFA entry (nl_stack_frame_drizzle_square_cfa_from): the mono square entry with nlstack_cfadrizzle.h's one
 * addition: a candidate (i, j) that is not a pixel of `channel` is skipped, as a NaN pixel is skipped.  Its planes
 * equal, bit for bit, those of nl_stack_frame_drizzle_square_from run on a copy of the mosaic whose other pixels are
 * NaN.
 *
 * Out of scope, each for a later change: a nl_group_ form; pixfrac > 1; Gaussian or Lanczos drop kernels;
 * the Go shim. */

/* The geometry of the definition above.  Host only: it needs no device.  corners = (cx_0, cy_0, cx_1, cy_1, cx_2,
 * cy_2, cx_3, cy_3) in the order the accumulate step walks them; box_half = (bx, by).  Every error of
 * nl_drizzle_geometry under this entry's name ("drizzle_square_geometry"), a corner or half-side that is not finite
 * among the coefficients, and R from the formula above. */
int nl_drizzle_square_geometry(const float trans[6], float scale, float pixfrac, float src_to_out[6], float out_to_src[6],
                               float corners[8], float box_half[2], int *radius);

/* nl_stack_frame_drizzle_from with the square kernel: the same arguments without `kernel`, the same checks in the
 * same order with the same messages under this entry's name, minus the kernel check.  Developer switch 32768 of
 * nl_stack_set_dev_flags on dst (no tile stages its source box in LDS) holds here too; switch 262144 evaluates the
 * four edges of every candidate instead of skipping those of a candidate that no work item of a wave takes (an A/B
 * measurement: the planes are the same bits either way). */
int nl_stack_frame_drizzle_square_from(nl_stack_t *dst, int sum_idx, int wgt_idx, nl_stack_t *src, int src_idx,
                                       const float trans[6], float scale, float pixfrac, float weight, int first);

/* nl_stack_frame_drizzle_cfa_from with the square kernel: the channel and the CFA are checked directly after the
 * weight, in front of anything that needs a handle, with that entry's messages. */
int nl_stack_frame_drizzle_square_cfa_from(nl_stack_t *dst, int sum_idx, int wgt_idx, nl_stack_t *src, int src_idx,
                                           const float trans[6], float scale, float pixfrac, float weight, int first,
                                           const char *channel, const char *cfa);

/* nl_stack_drizzle_tile_paths for the two entries above: the same tiles with the window of the square R.  The CFA
 * entry stages the whole candidate box, all colours, so this answers for it too. */
int nl_stack_drizzle_square_tile_paths(nl_stack_t *dst, nl_stack_t *src, int src_idx, const float trans[6], float scale,
                                       float pixfrac, int64_t *staged, int64_t *direct);

#ifdef __cplusplus
}
#endif

#endif
