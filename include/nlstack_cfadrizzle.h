/* nlstack_cfadrizzle.h -- CFA ("Bayer") drizzle: the raw mosaic of a one-shot-colour camera laid onto one colour plane
 * with no debayer in front, and the two resident steps it needs, entries of the C ABI of libnlstack.so.  AN EXTENSION:
 * the reference's colour front always ends in DebayerBilinear and it has no drizzle.  Part of nlstack.h, which includes
 * it behind nlstack_drizzle.h: include nlstack.h, not this file. */
#ifndef NLSTACK_CFADRIZZLE_H
#define NLSTACK_CFADRIZZLE_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- CFA drizzle (labelled extension) ----
 * DebayerBilinear in front of the stack is exactly the interpolation drizzle exists to avoid: three quarters of a
 * debayered R or B plane and half of G are made-up samples, and the stack averages them as if they were data.  With
 * dithered frames the mosaic's own pixels cover the output grid: every pixel of the raw mosaic is dropped onto the
 * plane of its own colour and nothing is interpolated.  One channel at a time, the reference's shape (`stack -debayer
 * R|G|B -cfa ...`, then `rgb`).  There is no reference to compare with: this text, on top of nlstack_drizzle.h's, is
 * the contract.
 *
 * Definition.  Channel membership.  cfa is "RGGB", "GRBG", "GBRG" or "BGGR" (either case) and gives (xo, yo) =
 * (0, 0), (1, 0), (0, 1), (1, 1) as getOffsets does (debayer.go:26-37); channel is "R", "G" or "B" (either case).
 * Mosaic pixel (i, j) -- column i, row j -- is a pixel of the channel if i >= xo, j >= yo and
 *   R:  (i - xo) and (j - yo) are both even
 *   B:  (i - xo) and (j - yo) are both odd
 *   G:  (i - xo) + (j - yo) is odd
 * These are exactly the pixels CosmeticCorrectionBayer walks for the channel (badpixels_bayer.go:64-351), up to the
 * mosaic's last row and column: a pixel the bad-pixel step can clean is a pixel the drizzle takes, and no other.  The
 * row above yo and the column left of xo belong to no channel (DebayerBilinear does not read them either).
 *
 * Accumulate (nl_stack_frame_drizzle_cfa_from): the text of nl_stack_frame_drizzle_from in nlstack_drizzle.h, word for
 * word -- nl_drizzle_geometry with its pixfrac in (0, 1] and NL_DZ_MAX_RADIUS, the window, the candidate order (rows
 * outer, columns inner), the operand order, `first`, NL_DZ_TURBO and NL_DZ_POINT -- with one addition: a candidate
 * (i, j) that is not a pixel of `channel` is skipped, as a NaN pixel is skipped.  One consequence: the two planes
 * equal, bit for bit, those of nl_stack_frame_drizzle_from run on a copy of the mosaic whose other pixels are NaN.
 * (That is how the tests restate it, not how it is computed: the kernel walks only the channel's positions of the
 * window, (R+1)^2 candidates for R and B and (2R+1)(R+1) for G instead of (2R+1)^2, in the same order.)
 *
 * The transform.  Alignment is estimated on a debayered plane, whose pixel (x, y) is mosaic pixel (x + xo, y + yo)
 * (debayer.go:87-90); all three channels debayer to the same shape and origin, so one transform serves all three.
 * nl_drizzle_cfa_transform, in double, rounded to fp32 once:  c' = c - a*xo - b*yo ;  f' = f - d*xo - e*yo ;
 * a, b, d, e unchanged.
 *
 * Rejection (nl_stack_frame_reject_against_cfa): nl_stack_frame_reject_against restricted to the channel's pixels;
 * every other pixel keeps its bits and counts nowhere.
 *
 * Out of scope, each for a later change: a nl_group_ form; pixfrac > 1 (a sparse channel at scale 1 leaves holes
 * that only dithering fills); the Go shim. */

/* The transform of the mosaic that belongs to trans_debayered, a forward Transform2D estimated on a plane debayered
 * with `cfa`.  Host only: it needs no device.  NL_ERR_INVALID_ARG for a null pointer (a null or empty cfa included),
 * "Unknown CFA value <cfa>", and a coefficient that is not finite, in or out. */
int nl_drizzle_cfa_transform(const float trans_debayered[6], const char *cfa, float trans_raw[6]);

/* nl_stack_frame_drizzle_from for the pixels of one channel of a raw mosaic.  src is a whole-image handle of the
 * MOSAIC's shape: the mosaic was uploaded with nl_stack_upload_tile like any mono frame (and calibrated with
 * nl_stack_frame_calibrate, cleaned with nl_stack_frame_badpixel_cfa); trans maps mosaic pixels to reference pixels
 * (nl_drizzle_cfa_transform).  Every check of nl_stack_frame_drizzle_from runs in its order with its messages under
 * this entry's name; the channel and CFA are checked directly after the kernel and the weight, in front of anything
 * that needs a handle: a NULL or empty name is NL_ERR_INVALID_ARG, otherwise "Unknown CFA value <cfa>", then "Unknown
 * debayering value <channel>".  The tiles stage the whole candidate box, all colours, so
 * nl_stack_drizzle_tile_paths answers for this entry too and developer switch 32768 holds. */
int nl_stack_frame_drizzle_cfa_from(nl_stack_t *dst, int sum_idx, int wgt_idx, nl_stack_t *src, int src_idx,
                                    const float trans[6], float scale, float pixfrac, float weight, int first,
                                    int kernel, const char *channel, const char *cfa);

/* nl_stack_frame_reject_against on the channel's pixels of the mosaic in slot idx.  The model in slot model_idx is
 * the finished plane of that colour blotted back onto the mosaic grid (nl_stack_frame_project_from with the inverse
 * of the mosaic's transform); only its values at the channel's pixels are read.  The thresholds are checked first,
 * then the channel and CFA as above, then the handle. */
int nl_stack_frame_reject_against_cfa(nl_stack_t *h, int idx, int model_idx, const char *channel, const char *cfa,
                                      float low, float high, int64_t *n_low, int64_t *n_high);

/* CosmeticCorrectionBayer (badpixels_bayer.go:26-351) for one channel, in place on the resident mosaic in slot idx:
 * the bad-pixel step of nl_stack_upload_frame_cfa without the debayer that discards the mosaic, bit for bit,
 * removed_out (numRemoved) and stats_out[2] (mean and std of data - median over the channel) included.  Called once
 * per channel it leaves the mosaic resident and clean for the three drizzles.  The device first (NL_ERR_NO_DEVICE
 * without one), then the handle, the index, the names (NULL or empty: NL_ERR_INVALID_ARG; then the CFA, then the
 * channel) and a whole-image handle, as nl_stack_upload_frame_cfa.  sigma_low == 0 || sigma_high == 0: nothing runs,
 * the stats are NaN and removed is 0; a negative sigma is well defined and accepted.  Only the compact buffers of the
 * correction live in per-handle scratch. */
int nl_stack_frame_badpixel_cfa(nl_stack_t *h, int idx, const char *channel, const char *cfa, float sigma_low,
                                float sigma_high, int64_t *removed_out, float *stats_out);

#ifdef __cplusplus
}
#endif

#endif
