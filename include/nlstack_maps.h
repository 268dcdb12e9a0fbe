/* nlstack_maps.h -- the per-pixel rejection and coverage maps of a stack pass, entries of the C ABI of libnlstack.so.
 * Part of nlstack.h, which includes it behind the types it needs: include nlstack.h, not this file. */
#ifndef NLSTACK_MAPS_H
#define NLSTACK_MAPS_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- where a pass clipped, and how many frames cover a pixel ----
 * The reference keeps two totals per pass, clipLow and clipHigh (internal/ops/stack/stack.go:193-198).  A maps pass
 * returns the same two totals and, per pixel, what they are the sums of.
 *
 * Definitions.
 *   reject_low[p] / reject_high[p]: the number of times the reference increments clipLow / clipHigh while it
 *     processes pixel p -- the clipping loop of sigma clipping (stack.go:411-424; weighted :494-511) and of
 *     winsorized clipping (:678-691; weighted :791-808), the one pass of MAD clipping (:581-593), and the
 *     rejection loop of the linear fit (:893-904).  Counted over all clipping rounds of the pixel.
 *   Their sums over the image are the clip_low / clip_high the same call returns.
 *   Mean and median give all zeros.  So does a pixel without data (no frame has a sample there).
 *   coverage[p]: the n the gather leaves (stack.go:380-387) -- the active frames whose sample at p is not NaN.
 *     +-Inf count as data.  It does not depend on the mode, the sigmas or the weights.
 *   reject_low[p] + reject_high[p] <= coverage[p] everywhere: every increment removes one sample from the pixel.
 *
 * Host buffers.  Every map is a whole-image width x height buffer of uint16; a handle that owns the rows
 * [row0, row0 + rows) writes exactly those rows and leaves the others alone, as nl_stack_finish does with out_host.
 * Any of the host pointers of nl_stack_run_maps / nl_group_run_maps may be NULL.
 *
 * The pass.  nl_stack_run_maps is nl_stack_run with the maps: NL_ST_AUTO is resolved by frame count, weighted MAD
 * fails with NL_ERR_WEIGHTED_MAD, an invalid mode with NL_ERR_INVALID_MODE; nl_stack_set_active_frames and the
 * weights apply.  More than 65 535 active frames fail with NL_ERR_TOO_MANY_FRAMES before any device work (a count
 * would not fit its 16 bits).  It is a pass: nl_stack_last_mode and nl_stack_last_kernel_name report it (the name
 * says "maps", e.g. "stack_exact_kernel<sigma,maps>"), its result stays on the device for the nl_stack_result_*
 * steps, nl_stack_pass_times times it.  It leaves later default passes as they would have been without it: it
 * neither forces the bit-exact kernels nor touches the list-length hints.
 *
 * The result.  Every mode but the mean runs on the one-pixel-per-lane column kernel, which replays the reference's
 * per-pixel algorithm in the reference's order: out_host of a maps pass is the BIT-EXACT result, for sigma and
 * winsorized clipping too.  The default pass keeps the totals identical but may differ from the reference -- and
 * therefore from a maps pass -- by summation-order rounding, at most 1e-6 relative (nl_stack_set_exact).  The
 * mean runs the mean kernel (bit-exact as always) and zeroes the maps.  A maps pass takes longer than a default
 * pass: the column kernel is the verification engine (DESIGN.md section 6n has the numbers).
 *
 * nl_stack_coverage reads the active frames once (HBM-bound) and is no pass: the last pass's result, mode and
 * kernel name stay.  A NULL output is NL_ERR_INVALID_ARG.  nl_stack_last_coverage_ms: GPU time of its kernels in the
 * last call, in ms, from HIP events on the handle's stream; -1 before the first call.
 *
 * The group forms fan out to the tiles as nl_group_run does: all tiles are started before any is awaited, every tile
 * that started is finished, the first error with its message is returned, the totals are summed and every tile
 * writes its own rows of the three host buffers.  No counterpart in the reference (it keeps the totals only). */
int nl_stack_run_maps(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc,
                      float *out_host, int64_t *clip_low, int64_t *clip_high,
                      uint16_t *reject_low_host, uint16_t *reject_high_host);
int nl_stack_coverage(nl_stack_t *h, uint16_t *coverage_host);
float nl_stack_last_coverage_ms(nl_stack_t *h);
int nl_group_run_maps(nl_group_t *g, int mode, float sigma_low, float sigma_high, float ref_loc,
                      float *out_host, int64_t *clip_low, int64_t *clip_high,
                      uint16_t *reject_low_host, uint16_t *reject_high_host);
int nl_group_coverage(nl_group_t *g, uint16_t *coverage_host);

#ifdef __cplusplus
}
#endif

#endif
