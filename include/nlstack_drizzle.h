/* nlstack_drizzle.h -- drizzle integration of resident frames onto a finer output grid, and the rejection step that
 * makes it usable, entries of the C ABI of libnlstack.so.  AN EXTENSION: the reference resamples every frame onto the
 * reference grid and stacks there; it has no drizzle.  Part of nlstack.h, which includes it behind the types it needs:
 * include nlstack.h, not this file. */
#ifndef NLSTACK_DRIZZLE_H
#define NLSTACK_DRIZZLE_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- drizzle integration (labelled extension) ----
 * Interpolating a frame onto the reference grid before the stack throws away the sub-pixel phase of its samples, so
 * the stack of undersampled, dithered frames cannot be sharper than one of them.  Drizzle (Fruchter & Hook 2002)
 * keeps the phase: every pixel of the UNRESAMPLED frame is shrunk to a square "drop" of pixfrac times its side, and
 * the drop's flux is laid onto an output grid of `scale` pixels per reference pixel, in proportion to the area it
 * covers of each output pixel.  A second plane records the weight that landed on every output pixel; the image is
 * the quotient of the two.  There is no reference to compare with: this text is the contract.
 *
 * Definition.  Geometry (nl_drizzle_geometry, host, in double).  trans = (a, b, c, d, e, f) is the forward
 * Transform2D, source pixel -> reference pixel, as nl_stack_frame_project_from takes it; S = scale; p = pixfrac.
 *   Fa = S*a   Fb = S*b   Fc = S*(c+0.5)-0.5      Fd = S*d   Fe = S*e   Ff = S*(f+0.5)-0.5        source -> output pixel
 *   det = Fa*Fe - Fb*Fd
 *   Ga = Fe/det   Gb = -Fb/det   Gd = -Fd/det   Ge = Fa/det   Gc = -(Ga*Fc + Gb*Ff)   Gf = -(Gd*Fc + Ge*Ff)
 *   hw = 0.5*p*sqrt(|det|)                        half the drop's side, in output pixels
 *   reach = 0.5 + hw
 *   R = (int)ceil( max((|Ga|+|Gb|)*reach, (|Gd|+|Ge|)*reach) + 0.5 + 1.0/64 )
 * F, G and hw are rounded to fp32 once, at the end.  R is the radius of the window of source pixels around the
 * rounded source position of an output pixel that holds every source pixel whose drop can touch it: an output pixel
 * and a drop overlap only if their centres are closer than `reach` on both output axes, which G maps to less than
 * (|Ga|+|Gb|)*reach source columns; rounding the position adds 0.5, and 1/64 covers the fp32 rounding of the two
 * coordinate evaluations at coordinates below 2^15.
 *
 * Accumulate (nl_stack_frame_drizzle_from), per output pixel (col, row); row is the image row, so a row-tile
 * destination makes its own rows only.  fp32, never fused, operands in the order written; col, row, i, j enter the
 * arithmetic as fp32 values.
 *   X = G.a*col + G.b*row + G.c ;  Y = G.d*col + G.e*row + G.f
 *   xc = floor(X + 0.5f) ;  yc = floor(Y + 0.5f)
 *   s = first ? +0 : sum[row][col] ;  t = first ? +0 : wgt[row][col]
 *   for j = yc-R .. yc+R (outer), i = xc-R .. xc+R (inner), skipping j, i outside the source:
 *       v = src[j][i] ;  skip if v != v                                  (NaN = no data; +-Inf takes part)
 *       u = F.a*i + F.b*j + F.c ;  vv = F.d*i + F.e*j + F.f
 *       NL_DZ_TURBO:  lo = u - hw;  e = col - 0.5f;  if (e > lo) lo = e
 *                     hi = u + hw;  e = col + 0.5f;  if (e < hi) hi = e;   ox = hi - lo;  skip unless ox > 0
 *                     oy the same from vv and row;  skip unless oy > 0;  ar = ox*oy ;  wa = weight*ar
 *       NL_DZ_POINT:  skip unless floor(u + 0.5f) == col and floor(vv + 0.5f) == row ;  wa = weight
 *       s = s + v*wa ;  t = t + wa
 *   sum[row][col] = s ;  wgt[row][col] = t
 * A NaN xc or yc, or one whose window misses the source, gives no candidates: the pixel keeps s and t.  With
 * first != 0 what the two slots held is ignored.  This is the gather form: no atomics, a fixed candidate order, so
 * the result is deterministic and bit for bit what the numpy restatement of this text gives.
 *
 * NL_DZ_TURBO is the axis-aligned drop of the drizzle literature's "turbo" kernel: exact for shifts, flips and
 * quarter turns, an approximation under other rotations.  NL_DZ_POINT lays a pixel's whole weight onto the one
 * output pixel its centre falls in (pixfrac still sets R, not the result).
 *
 * Finalize (nl_stack_drizzle_finalize), per pixel:  out = (wgt > min_weight) ? sum / wgt : empty.  IEEE division; a
 * NaN weight gives `empty`.
 *
 * Rejection (nl_stack_frame_reject_against), per pixel, v of slot idx and m of slot model_idx:  d = v - m;
 * d < -low: v becomes NaN and counts low; otherwise d > high: v becomes NaN and counts high; otherwise v keeps its
 * bits.  A NaN on either side falls through both tests.
 *
 * Out of scope, each for a later change: a nl_group_ form (tiles on other devices need the peer copy of the group
 * projection; once this kernel has been timed); the rotated-square kernel (NL_DZ_TURBO is axis-aligned in the
 * output); the Go shim. */
#define NL_DZ_TURBO 0
#define NL_DZ_POINT 1
#define NL_DZ_MAX_RADIUS 3

/* The geometry of the definition above.  Host only: it needs no device.  NL_ERR_INVALID_ARG for a null pointer, a
 * scale that is not finite or <= 0, a pixfrac outside (0, 1] or NaN, a transform that the reference's Invert rejects
 * ("Matrix has no inverse, epsilon=...", as the projection entries say it), a coefficient of F or G that is not
 * finite, and R > NL_DZ_MAX_RADIUS (the message states R). */
int nl_drizzle_geometry(const float trans[6], float scale, float pixfrac, float src_to_out[6], float out_to_src[6],
                        float *half_width, int *radius);

/* Lays resident slot src_idx of the whole-image handle src onto the planes sum_idx (flux) and wgt_idx (weight) of
 * dst, whose own width and height are the output grid (typically round(S*W) x round(S*H); any row tile of it).
 * weight is the frame's weight, finite and > 0; first != 0 starts the two planes, 0 adds to them; kernel is NL_DZ_*.
 * NL_ERR_INVALID_ARG, what needs no handle first: every geometry error, an unknown kernel, a bad weight, a null
 * handle or transform; then a row-tile source, handles on different devices, sum_idx == wgt_idx, an index out of
 * range, a destination whose frames are attached, not owned, and a source slot that is one of the two destination
 * slots.  Synchronous like the projection; the destination's stream waits for the source's.  The developer switch
 * 32768 of nl_stack_set_dev_flags on dst (no tile stages its source box in LDS) holds here too. */
int nl_stack_frame_drizzle_from(nl_stack_t *dst, int sum_idx, int wgt_idx, nl_stack_t *src, int src_idx,
                                const float trans[6], float scale, float pixfrac, float weight, int first, int kernel);

/* out_idx = the quotient of the two planes where the weight exceeds min_weight, else `empty`.  Elementwise: the three
 * slots may alias in any way.  The result is a resident slot like any other (statistics, tone curves, blur, export);
 * the weight plane is the drizzle weight map, nl_stack_download_tile fetches it. */
int nl_stack_drizzle_finalize(nl_stack_t *h, int sum_idx, int wgt_idx, int out_idx, float min_weight, float empty);

/* Blot-and-compare with the thresholds left to the caller: takes the outliers of slot idx against the model in slot
 * model_idx out of the frame (they become NaN, which the drizzle skips).  The model is the finished conventional
 * stack laid back onto the source grid: nl_stack_frame_project_from with the inverse transform into a second slot of
 * the staging handle.  low and high are absolute and >= 0 (scale them from nl_stack_frame_noise); NaN or a negative
 * one gives NL_ERR_INVALID_ARG.  n_low / n_high (either may be null): how many pixels went each way. */
int nl_stack_frame_reject_against(nl_stack_t *h, int idx, int model_idx, float low, float high, int64_t *n_low,
                                  int64_t *n_high);

/* Developer query, what nl_stack_project_tile_paths is for the projection: of the workgroup tiles that
 * nl_stack_frame_drizzle_from(dst, ., ., src, src_idx, trans, scale, pixfrac, ...) launches, how many stage their
 * source box in LDS and how many take their candidates from global memory.  Host arithmetic only, the kernel's own. */
int nl_stack_drizzle_tile_paths(nl_stack_t *dst, nl_stack_t *src, int src_idx, const float trans[6], float scale,
                                float pixfrac, int64_t *staged, int64_t *direct);

#ifdef __cplusplus
}
#endif

#endif
