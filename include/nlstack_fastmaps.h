/* nlstack_fastmaps.h -- the rejection maps of a stack pass from the default pass's engines, entries of the C ABI of
 * libnlstack.so.  Part of nlstack.h, which includes it behind the types it needs: include nlstack.h, not this file. */
#ifndef NLSTACK_FASTMAPS_H
#define NLSTACK_FASTMAPS_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- where a pass clipped, at the speed of the pass ----
 * nl_stack_run_maps (nlstack_maps.h) runs every mode on the column kernel, the verification engine: bit-exact, and
 * many times slower than a default pass.  nl_stack_run_maps_fast is the same call -- same arguments, same definitions
 * of reject_low / reject_high, same NULL rules (any host pointer may be NULL), same row-tile rule (a handle that owns
 * the rows [row0, row0 + rows) writes exactly those rows of the whole-image buffers), same error codes and messages
 * (NL_ERR_INVALID_MODE, NL_ERR_WEIGHTED_MAD, NL_ERR_TOO_MANY_FRAMES above 65 535 active frames) -- on the engines of
 * nl_stack_run where those can carry the per-pixel counts out, and the pass of nl_stack_run_maps everywhere else.
 *
 * When the fast engines run.  For NL_ST_SIGMA and NL_ST_WINSOR_SIGMA (after NL_ST_AUTO is resolved by frame count), when
 *   the pass is unweighted, 2 ... 128 frames are active (nl_stack_set_active_frames), the tile has fewer than 2^27
 *   pixels and the handle is not forced exact (nl_stack_set_exact): the register-resident kernels of the default pass,
 *   each lane storing its pixel's two counts beside its result; the pixels a lane cannot decide are replayed by the
 *   column kernel, which stores theirs.
 * Maps.  reject_low / reject_high equal those of nl_stack_run_maps -- and the reference's increments of clipLow /
 *   clipHigh at each pixel -- count for count: the fast kernels accept a clip decision only where it is the reference's
 *    and hand every other pixel to the exact replay before they count anything.  clip_low /
 *   clip_high are their sums.  reject_low[p] + reject_high[p] <= coverage[p] as before.
 * Result.  out_host is the DEFAULT pass's result, not the bit-exact one: it carries the reservation of nl_stack_run --
 *   summation-order rounding, at most 1e-6 relative (nl_stack_set_exact).  A pixel replayed by the exact kernel (an
 *   infinite sample, an undecidable clip) and a pixel without data (ref_loc) are bit-exact.
 * Everything else.  Median, MAD, the linear fit, the weighted modes, more than 128 active frames, a handle forced
 *   exact and tiles of 2^27 pixels or more run exactly the pass of nl_stack_run_maps: bit-exact, same kernel name
 *   ("stack_exact_kernel<...,maps>").  The mean runs the mean kernel and zeroes the maps, as there.  The caller always
 *   gets maps; nl_stack_last_kernel_name says which engine ran.
 * Kernel name.  The name of a fast maps pass is the default pass's with "maps" as its last argument, e.g.
 *   "stack_sigma_fast_kernel<128, true, false, true, false, false, maps>": it contains both "stack_sigma_fast_kernel"
 *   and "maps".
 *
 * It is a pass: nl_stack_last_mode, nl_stack_pass_times and the nl_stack_result_* steps see it, and
 * nl_stack_last_generic_pixels / nl_stack_last_fallback_pixels report the lengths of its two hand-over lists.  Like
 * nl_stack_run_maps it leaves later default passes as they would have been without it: it runs the plain protocol
 * (nl_stack_last_pass_protocol 0), neither reads nor leaves list-length hints, and does not force the bit-exact kernels.
 * DESIGN.md section 6n has the protocol and the measured times.
 *
 * nl_group_run_maps_fast fans out as nl_group_run_maps does: all tiles are started before any is awaited, every tile
 * that started is finished, the first error with its message is returned, the totals are summed and every tile writes
 * its own rows of the three host buffers.  No counterpart in the reference (it keeps the totals only). */
int nl_stack_run_maps_fast(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc,
                           float *out_host, int64_t *clip_low, int64_t *clip_high,
                           uint16_t *reject_low_host, uint16_t *reject_high_host);
int nl_group_run_maps_fast(nl_group_t *g, int mode, float sigma_low, float sigma_high, float ref_loc,
                           float *out_host, int64_t *clip_low, int64_t *clip_high,
                           uint16_t *reject_low_host, uint16_t *reject_high_host);

#ifdef __cplusplus
}
#endif

#endif
