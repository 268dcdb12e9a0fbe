/* nlstack_deepmaps.h -- the rejection maps of a deep sigma / winsorized stack (129 ... 512 frames) from the LDS-column
 * engines of the default pass: entries of the C ABI of libnlstack.so.  Part of nlstack.h, which includes it behind the
 * types it needs: include nlstack.h, not this file. */
#ifndef NLSTACK_DEEPMAPS_H
#define NLSTACK_DEEPMAPS_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- where a deep sigma / winsorized stack clipped, at the speed of the pass ----
 * nl_stack_run_maps (nlstack_maps.h) runs every mode on the column kernel, the verification engine;
 * nl_stack_run_maps_fast (nlstack_fastmaps.h) takes unweighted sigma / winsorized clipping of up to 128 frames to the
 * default pass's kernels, nl_stack_run_maps_resident (nlstack_residentmaps.h) the linear fit of up to 512 as well; both
 * are pinned to the column kernel for everything else.  Sigma / winsorized clipping of 129 ... 512 frames is what the
 * deepest stacks run, and the kernels of their default pass already hold every pixel's two counts in the lane that
 * stores its result.  nl_stack_run_maps_deep is the same call as the other three -- same arguments, same definitions of
 * reject_low / reject_high, same NULL rules (any host pointer may be NULL), same row-tile rule (a handle that owns the
 * rows [row0, row0 + rows) writes exactly those rows of the whole-image buffers), same error codes and messages
 * (NL_ERR_INVALID_MODE, NL_ERR_WEIGHTED_MAD, NL_ERR_TOO_MANY_FRAMES above 65 535 active frames) -- with the deep sigma /
 * winsorized stacks on their own kernels as well.
 *
 * When the deep engines run.  For NL_ST_SIGMA and NL_ST_WINSOR_SIGMA (after NL_ST_AUTO is resolved by frame count), when
 *   129 ... 512 frames are active (nl_stack_set_active_frames), the handle has no weights (nl_stack_set_weights), the
 *   tile has fewer than 2^27 pixels and the handle is not forced exact (nl_stack_set_exact): the kernels of the default
 *   pass in their MAPS instantiations -- stack_sigma_mlz_kernel of the frame-count class (the frames rounded up to a
 *   multiple of 16; 2 lanes per pixel up to 256 frames, 4 above) over the tile, the LDS-column generic kernel over the
 *   pixels it hands over (too many missing samples, more clips than its columns hold), the column kernel once over the
 *   pixels neither can decide.  The pass runs the plain protocol on the handle's one stream: no fused protocol or tail,
 *   no side stream, no threshold record, fixed grids.
 * Maps.  reject_low / reject_high equal those of nl_stack_run_maps -- and the reference's increments of clipLow /
 *   clipHigh at each pixel -- count for count.  clip_low / clip_high are their sums.  reject_low[p] + reject_high[p]
 *   <= coverage[p] as before.  Every pixel's word is written by exactly one of the three kernels, by the lane that
 *   stores its result: nothing of an earlier pass on the handle shows through, whatever that pass was.
 * Result.  out_host is the default pass's: the same kernels and arithmetic (241 ... 255 and 497 ... 511 frames: the same
 *   kernel on a layout with room for more missing samples), within the default pass's reservation against the reference
 *   (summation-order rounding, at most 1e-6 relative).  The pixels replayed by the column kernel
 *   are bit-exact, and a pixel without data gives ref_loc with zero counts, bit for bit.
 * Everything else.  A pass the deep engines do not run is exactly the pass of nl_stack_run_maps_resident: sigma /
 *   winsorized clipping of up to 128 frames on the register-resident kernels, the linear fit of up to 512 frames on its
 *   own kernels and cascade, and the pass of nl_stack_run_maps -- bit-exact, same kernel name
 *   ("stack_exact_kernel<...,maps>") -- for the rest.  Out of scope here, and on the column kernel as before: MAD, the
 *   weighted sigma / winsorized modes, the median, stacks of more than 512 frames, a handle forced exact and tiles of
 *   2^27 pixels or more.  The mean runs the mean kernel and zeroes the maps, as there.  The caller always gets maps;
 *   nl_stack_last_kernel_name says which engine ran.
 * Kernel name.  The name of a deep maps pass is the default pass's with "maps" as its last argument, e.g.
 *   "stack_sigma_mlz_kernel<4, false, 512, 0, maps>" or "stack_sigma_mlz_kernel<2, true, 208, 0, maps>": it contains
 *   "stack_sigma_mlz_kernel" and "maps".
 *
 * It is a pass: nl_stack_last_mode, nl_stack_pass_times and the nl_stack_result_* steps see it,
 * nl_stack_last_generic_pixels and nl_stack_last_fallback_pixels report the lengths of its two lists.  Like the other maps
 * passes it leaves later default passes as they would have been without it: it runs the plain protocol
 * (nl_stack_last_pass_protocol 0), neither reads nor leaves list-length hints, and does not force the bit-exact kernels.
 * DESIGN.md section 6n has the protocol, the resources of the MAPS instantiations and the measured times.
 *
 * nl_group_run_maps_deep fans out as nl_group_run_maps_resident does: all tiles are started before any is awaited, every
 * tile that started is finished, the first error with its message is returned, the totals are summed and every tile
 * writes its own rows of the three host buffers.  No counterpart in the reference (it keeps the totals only). */
int nl_stack_run_maps_deep(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc,
                           float *out_host, int64_t *clip_low, int64_t *clip_high,
                           uint16_t *reject_low_host, uint16_t *reject_high_host);
int nl_group_run_maps_deep(nl_group_t *g, int mode, float sigma_low, float sigma_high, float ref_loc,
                           float *out_host, int64_t *clip_low, int64_t *clip_high,
                           uint16_t *reject_low_host, uint16_t *reject_high_host);

#ifdef __cplusplus
}
#endif

#endif
