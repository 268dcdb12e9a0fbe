/* nlstack_fullmaps.h -- the rejection maps of a MAD-sigma stack (1 ... 512 frames) from the MAD engines of the default
 * pass, and the median's zero maps from its default kernels: entries of the C ABI of libnlstack.so.  Part of nlstack.h,
 * which includes it behind the types it needs: include nlstack.h, not this file. */
#ifndef NLSTACK_FULLMAPS_H
#define NLSTACK_FULLMAPS_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- where a MAD-sigma stack clipped, at the speed of the pass ----
 * nl_stack_run_maps (nlstack_maps.h) runs every mode on the column kernel, the verification engine;
 * nl_stack_run_maps_fast (nlstack_fastmaps.h), nl_stack_run_maps_resident (nlstack_residentmaps.h) and
 * nl_stack_run_maps_deep (nlstack_deepmaps.h) take sigma / winsorized clipping and the linear fit of up to 512 frames to
 * the default pass's kernels; all four are pinned to the column kernel for MAD sigma and the median.  The three MAD
 * kernels of the default pass already hold every pixel's two counts, as integers, in the lane that stores its result, and
 * the median rejects nothing.  nl_stack_run_maps_full is the same call as the other four -- same arguments, same
 * definitions of reject_low / reject_high, same NULL rules (any host pointer may be NULL), same row-tile rule (a handle
 * that owns the rows [row0, row0 + rows) writes exactly those rows of the whole-image buffers), same error codes and
 * messages (NL_ERR_INVALID_MODE, NL_ERR_WEIGHTED_MAD on a handle with weights, NL_ERR_TOO_MANY_FRAMES above 65 535 active
 * frames) -- with MAD sigma on its own kernels and the median on its default ones as well.
 *
 * When the MAD engines run.  For NL_ST_MAD_SIGMA, when 1 ... 512 frames are active (nl_stack_set_active_frames), the
 *   handle has no weights (with weights the call fails with NL_ERR_WEIGHTED_MAD, as every unweighted entry), is not forced
 *   exact (nl_stack_set_exact), has its exact and generic lists, and the tile has fewer than 2^27 pixels: the dominant
 *   kernel of the default MAD pass in its MAPS instantiation -- stack_mad_fast_kernel of the network size (the frames
 *   rounded up to 8, 16, 32, 48, 64, 80, 96, 112 or 128); from 114 frames on stack_mad_bitonic_kernel, with
 *   stack_mad_fast_kernel<128> in its MAPS form over the pixels with fewer than 114 samples, which it hands over;
 *   129 ... 512 frames stack_mad_ml_kernel with 2 (up to 256 frames) or 4 lanes per pixel -- then the column kernel once
 *   over the pixels none of them can decide, those whose median is not finite.  The pass runs the plain protocol on the
 *   handle's one stream: no side stream, no hints read or left.
 * Maps.  reject_low / reject_high equal those of nl_stack_run_maps -- and the reference's increments of clipLow /
 *   clipHigh at each pixel -- count for count, without any guard band: the bounds come from two medians, which do not
 *   depend on the order of the samples.  clip_low / clip_high are their sums.  reject_low[p] + reject_high[p] <=
 *   coverage[p] as before.  Every pixel's word is written by exactly one kernel, by the lane that stores its result: nothing
 *   of an earlier pass on the handle shows through, whatever that pass was.
 * Result.  out_host is the default pass's, bit for bit: the same kernels and arithmetic, within the default pass's
 *   reservation against the reference (summation-order rounding of the mean of the survivors, at most 1e-6 relative).
 *   The pixels replayed by the column kernel are bit-exact, and a pixel without data gives ref_loc with zero counts, bit
 *   for bit.
 * The median.  For NL_ST_MEDIAN of up to 512 active frames on a handle that is not forced exact: the default median
 *   kernels (register network from 2 frames on, multi-lane merge from 129), the maps zeroed with one memset, totals 0 / 0.
 *   The result is bit-exact, as the median's always is.
 * Everything else.  A pass neither takes is exactly the pass of nl_stack_run_maps_deep: sigma / winsorized clipping and the
 *   linear fit on their own kernels where that entry runs them, and the pass of nl_stack_run_maps -- bit-exact, same
 *   kernel name ("stack_exact_kernel<...,maps>") -- for the rest.  On the column kernel as before: the weighted sigma /
 *   winsorized modes, stacks of more than 512 frames, a handle forced exact, a handle without lists and tiles of 2^27
 *   pixels or more.  The mean runs the mean kernel and zeroes the maps, as there.  The caller always gets maps;
 *   nl_stack_last_kernel_name says which engine ran.
 * Kernel name.  The name of a MAD maps pass is the default pass's with "maps" as its last argument:
 *   "stack_mad_fast_kernel<64, maps>", "stack_mad_bitonic_kernel<maps>", "stack_mad_ml_kernel<4, maps>".  It contains
 *   "stack_mad_" and "maps".
 *
 * It is a pass: nl_stack_last_mode, nl_stack_pass_times and the nl_stack_result_* steps see it,
 * nl_stack_last_generic_pixels and nl_stack_last_fallback_pixels report the lengths of its two lists.  Like the other maps
 * passes it leaves later default passes as they would have been without it: it runs the plain protocol
 * (nl_stack_last_pass_protocol 0), neither reads nor leaves list-length hints, and does not force the bit-exact kernels.
 * DESIGN.md section 6n has the protocol, the resources of the MAPS instantiations and the measured times.
 *
 * nl_group_run_maps_full fans out as nl_group_run_maps_deep does: all tiles are started before any is awaited, every
 * tile that started is finished, the first error with its message is returned, the totals are summed and every tile
 * writes its own rows of the three host buffers.  No counterpart in the reference (it keeps the totals only). */
int nl_stack_run_maps_full(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc,
                           float *out_host, int64_t *clip_low, int64_t *clip_high,
                           uint16_t *reject_low_host, uint16_t *reject_high_host);
int nl_group_run_maps_full(nl_group_t *g, int mode, float sigma_low, float sigma_high, float ref_loc,
                           float *out_host, int64_t *clip_low, int64_t *clip_high,
                           uint16_t *reject_low_host, uint16_t *reject_high_host);

#ifdef __cplusplus
}
#endif

#endif
