/* nlstack_residentmaps.h -- the rejection maps of a stack pass from the register-resident engines, the linear fit's
 * cascade included: entries of the C ABI of libnlstack.so.  Part of nlstack.h, which includes it behind the types it
 * needs: include nlstack.h, not this file. */
#ifndef NLSTACK_RESIDENTMAPS_H
#define NLSTACK_RESIDENTMAPS_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- where a linear-fit pass clipped, at the speed of the pass ----
 * nl_stack_run_maps (nlstack_maps.h) runs every mode on the column kernel, the verification engine; nl_stack_run_maps_fast
 * (nlstack_fastmaps.h) takes unweighted sigma / winsorized clipping of up to 128 frames to the default pass's kernels and
 * is pinned to the column kernel for everything else.  The linear fit is what NL_ST_AUTO picks from 25 frames on, and its
 * default pass already holds every pixel's two counts where it stores the result.  nl_stack_run_maps_resident is the
 * same call as the other two -- same arguments, same definitions of reject_low / reject_high, same NULL rules (any host
 * pointer may be NULL), same row-tile rule (a handle that owns the rows [row0, row0 + rows) writes exactly those rows of
 * the whole-image buffers), same error codes and messages (NL_ERR_INVALID_MODE, NL_ERR_WEIGHTED_MAD,
 * NL_ERR_TOO_MANY_FRAMES above 65 535 active frames) -- with the linear fit on its own kernels as well.
 *
 * When the resident engines run.  For NL_ST_LINEAR_FIT (after NL_ST_AUTO is resolved by frame count), when 1 ... 512
 *   frames are active (nl_stack_set_active_frames), the tile has fewer than 2^27 pixels and the handle is not forced exact
 *   (nl_stack_set_exact): the kernels of the default linear-fit pass -- stack_linfit_fast_kernel up to 128 frames,
 *   stack_linfit_ml_kernel (2 or 4 lanes per pixel) above -- with the same cascade, stage quotas and grids.  The first
 *   stage stores each pixel's two counts, every later stage of the cascade adds its own to them; the pixels with an
 *   infinite sample are replayed by the column kernel, which stores theirs.  Weights set on the handle are dropped, as
 *   the linear fit drops them in nl_stack_run and nl_stack_run_maps.  For NL_ST_SIGMA and NL_ST_WINSOR_SIGMA: exactly
 *   when, and exactly as, nl_stack_run_maps_fast runs its fast engines.
 * Maps.  reject_low / reject_high equal those of nl_stack_run_maps -- and the reference's increments of clipLow /
 *   clipHigh at each pixel -- count for count.  clip_low / clip_high are their sums.  reject_low[p] + reject_high[p]
 *   <= coverage[p] as before.  Every word of the map is written by the pass that returns it: nothing of an earlier
 *   pass on the handle shows through, whatever that pass was.
 * Result.  For the linear fit out_host is bit-exact, not merely within 1e-6: both kernels sum in the reference's order,
 *   and the result equals that of nl_stack_run and of nl_stack_run_maps bit for bit.  For sigma / winsorized clipping it
 *   is the result of nl_stack_run_maps_fast, with that entry's reservation (summation-order rounding, at most 1e-6
 *   relative).  A pixel without data gives ref_loc with zero counts.
 * Everything else.  Median, MAD, the weighted sigma / winsorized modes, sigma / winsorized clipping of more than 128
 *   frames, the linear fit of more than 512, a handle forced exact and tiles of 2^27 pixels or more run exactly the pass
 *   of nl_stack_run_maps: bit-exact, same kernel name ("stack_exact_kernel<...,maps>").  The mean runs the mean kernel
 *   and zeroes the maps, as there.  The caller always gets maps; nl_stack_last_kernel_name says which engine ran.
 * Kernel name.  The name of a resident linear-fit maps pass is the default pass's with "maps" as its last argument, e.g.
 *   "stack_linfit_fast_kernel<128, false, maps>" or "stack_linfit_ml_kernel<2, false, maps>": it contains
 *   "stack_linfit_fast_kernel" or "stack_linfit_ml_kernel", and "maps".
 *
 * It is a pass: nl_stack_last_mode, nl_stack_pass_times and the nl_stack_result_* steps see it,
 * nl_stack_linfit_stage_counts reports the lengths of its cascade's lists and nl_stack_last_fallback_pixels the length of
 * its exact list, as after a default linear-fit pass.  Like the other maps passes it leaves later default passes as they
 * would have been without it: it runs the plain protocol (nl_stack_last_pass_protocol 0), neither reads nor leaves
 * list-length hints, and does not force the bit-exact kernels.  DESIGN.md section 6n has the protocol, the rule by which
 * a pixel's word is built across the cascade, and the measured times.
 *
 * nl_group_run_maps_resident fans out as nl_group_run_maps_fast does: all tiles are started before any is awaited, every
 * tile that started is finished, the first error with its message is returned, the totals are summed and every tile
 * writes its own rows of the three host buffers.  No counterpart in the reference (it keeps the totals only). */
int nl_stack_run_maps_resident(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc,
                               float *out_host, int64_t *clip_low, int64_t *clip_high,
                               uint16_t *reject_low_host, uint16_t *reject_high_host);
int nl_group_run_maps_resident(nl_group_t *g, int mode, float sigma_low, float sigma_high, float ref_loc,
                               float *out_host, int64_t *clip_low, int64_t *clip_high,
                               uint16_t *reject_low_host, uint16_t *reject_high_host);

#ifdef __cplusplus
}
#endif

#endif
