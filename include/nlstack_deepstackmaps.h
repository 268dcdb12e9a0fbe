/* nlstack_deepstackmaps.h -- the rejection maps of stacks beyond 512 frames at the speed of the pass: MAD sigma and the
 * median of 513 ... 2048 frames on the 8- and 16-lane engines of nlstack_deepstack.h, sigma / winsorized clipping beyond
 * 512 frames on the wave-per-pixel replay nl_stack_run runs there.  Entries of the C ABI of libnlstack.so.  Part of
 * nlstack.h, which includes it behind the types it needs: include nlstack.h, not this file. */
#ifndef NLSTACK_DEEPSTACKMAPS_H
#define NLSTACK_DEEPSTACKMAPS_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- where a stack of more than 512 frames clipped, at the speed of the pass ----
 * Beyond 512 active frames every other maps entry (nlstack_maps.h ... nlstack_fullmaps.h) runs the one-pixel-per-lane
 * column kernel, whose time grows with the depth, beside passes that take milliseconds.  nl_stack_run_maps_deepstack is
 * the same call as those entries -- same arguments, same definitions of reject_low / reject_high (the pixel's own
 * increments of clipLow / clipHigh), same NULL rules (any host pointer may be NULL), same row-tile rule (a handle that
 * owns the rows [row0, row0 + rows) writes exactly those rows of the whole-image buffers), same error codes and messages
 * (NL_ERR_INVALID_MODE, NL_ERR_WEIGHTED_MAD for MAD sigma on a handle with weights, NL_ERR_TOO_MANY_FRAMES above 65 535
 * active frames) -- with three more engines.  It is the sixth tier of the maps passes and includes the five below it.
 *
 * Definition per mode.
 *   NL_ST_MAD_SIGMA, 513 ... 2048 active frames (nl_stack_set_active_frames), no weights, a handle that is not forced
 *     exact (nl_stack_set_exact) and has its exact list, a frame stride within the gather's offsets (below 2^26 pixels at 8
 *     lanes per pixel, 2^25 at 16).  reject_low / reject_high and their sums clip_low / clip_high equal those of
 *     nl_stack_run_maps COUNT FOR COUNT: the bounds come from two medians, which do not depend on the order of the
 *     samples.  out_host equals nl_stack_run_deepstack's BIT FOR BIT: the same kernel and arithmetic with one more store.
 *     A pixel without a finite median is replayed by the column kernel, which writes its word; a pixel without a sample
 *     gets ref_loc and a zero word.
 *   NL_ST_MEDIAN under the same depth conditions: nl_stack_run's bits (the median is an order statistic), the maps zeroed
 *     with one memset, totals 0 / 0.
 *   NL_ST_SIGMA / NL_ST_WINSOR_SIGMA, more than 512 active frames, no weights, not forced exact, as many frames as the
 *     wave-per-pixel replay holds in LDS (up to 8192 for sigma, 5461 for winsorized clipping): out_host, both maps and both
 *     totals equal nl_stack_run_maps' BIT FOR BIT and COUNT FOR COUNT -- both kernels are replays of the reference, in
 *     the reference's order.  The counts of a pixel are what its replay added to the wave's running counts.
 *
 * Engines.  MAD sigma: "stack_mad_ml_kernel<8, maps>" (513 ... 1024 frames) / "stack_mad_ml_kernel<16, maps>"
 * (1025 ... 2048), then the column kernel's "stack_exact_kernel<mad,maps>" over the exact list and the reduction of the
 * clip counts; nl_stack_last_fallback_pixels counts the listed pixels.  The median: "stack_median_ml_kernel<8>" /
 * "stack_median_ml_kernel<16>".  Sigma / winsorized: "stack_sigma_coop_kernel<WINSOR, false, GROUP, 2, maps>" over the
 * whole tile, GROUP = 4 pixels per work item where the handle's stride and tile allow 16-byte loads, else 1, every pixel
 * with a word of its own; no decision pass stands in front of it, because the pass is unweighted.
 * nl_stack_last_kernel_name reports the name.
 *
 * Fall-throughs.  Everything else is nl_stack_run_maps_full's pass in every observable respect (result, maps, totals,
 * kernel name, protocol, list lengths): 512 active frames or fewer; weights on a clip mode; the linear fit; more than
 * 2048 frames for MAD sigma and the median; after nl_stack_set_exact; MAD sigma on a handle without an exact list; the
 * mean.  Beyond 512 frames those still take the column kernel ("stack_exact_kernel<...,maps>").
 *
 * Errors.  Those of nl_stack_run_maps, checked in the same order with the same messages; a null handle or group is
 * NL_ERR_INVALID_ARG before anything else.
 *
 * It is a pass: nl_stack_last_mode, nl_stack_pass_times and the nl_stack_result_* steps see it.  Like the other maps
 * passes it runs the plain protocol (nl_stack_last_pass_protocol 0) on the handle's one stream, neither reads nor leaves
 * list-length hints and never runs the fused protocol: default passes behind it are what they would have been without
 * it.  Every pixel's word is written by this pass: nothing of an earlier pass on the handle shows through.
 *
 * nl_group_run_maps_deepstack fans out as nl_group_run_maps_full does: all tiles are started before any is awaited, every
 * tile that started is finished, the first error with its message is returned, the totals are summed and every tile
 * writes its own rows of the three host buffers.  No counterpart in the reference (it keeps the totals only). */
int nl_stack_run_maps_deepstack(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc,
                                float *out_host, int64_t *clip_low, int64_t *clip_high,
                                uint16_t *reject_low_host, uint16_t *reject_high_host);
int nl_group_run_maps_deepstack(nl_group_t *g, int mode, float sigma_low, float sigma_high, float ref_loc,
                                float *out_host, int64_t *clip_low, int64_t *clip_high,
                                uint16_t *reject_low_host, uint16_t *reject_high_host);

#ifdef __cplusplus
}
#endif

#endif
