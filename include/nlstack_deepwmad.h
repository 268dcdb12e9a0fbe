/* nlstack_deepwmad.h -- weighted MAD-sigma stacking of 513 ... 2048 frames on the 8- and 16-lane engine of
 * nlstack_deepstack.h, entries of the C ABI of libnlstack.so.  AN EXTENSION OF DEPTH, NOT OF SEMANTICS: what the entries
 * compute is what nl_stack_run_mad_weighted (nlstack_wmad.h) computes, bit for bit; only the engine differs.  Part of
 * nlstack.h, which includes it behind the types it needs: include nlstack.h, not this file. */
#ifndef NLSTACK_DEEPWMAD_H
#define NLSTACK_DEEPWMAD_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- nl_stack_run_mad_weighted for deep stacks ----
 * Definition.  That of nlstack_wmad.h, unchanged: StackMADSigma's rejection on the values alone (median, mad * 1.4826f,
 * lo = median - sigma_low * sd, hi = median + sigma_high * sd, two roundings per bound, never fused); the survivors
 * accumulated in ascending FRAME INDEX, num += v_k * w_k, den += w_k, each with its own frame's weight; num / den.  Both
 * medians are order statistics, so the result equals nl_stack_run_mad_weighted's BIT FOR BIT and clip_low / clip_high
 * COUNT FOR COUNT, and the counters equal those of the unweighted MAD pass over the same frames.
 *
 * Engines.  With 513 ... 2048 ACTIVE frames (nl_stack_set_active_frames), on a handle that is not forced exact
 * (nl_stack_set_exact), has its exact list and can hold the threshold record (8 bytes per pixel and round, as the
 * weighted passes of nlstack_wclip.h and nlstack_wmad.h), with a frame stride within the gather's offsets (below 2^26
 * pixels at 8 lanes per pixel, 2^25 at 16):
 *   1. "stack_mad_ml_kernel<8, true>" (513 ... 1024 frames) / "stack_mad_ml_kernel<16, true>" (1025 ... 2048), record
 *      only: each pixel's (lo, hi), and no round for a pixel without a finite median or without a sample;
 *   2. "stack_clip_weighted_kernel<4, true>", one streaming read of the frames in frame order under those bounds, which
 *      hands the pixels without a round to the exact list -- the kernel nl_stack_last_kernel_name reports;
 *   3. the column kernel "stack_exact_kernel<mad,follow>" over that list, and the reduction of the clip counts.
 * nl_stack_last_fallback_pixels counts the listed pixels: those without a finite median and those without a sample.
 *
 * Fall-throughs.  Every other case is nl_stack_run_mad_weighted's pass in every observable respect (result, counters,
 * kernel name, list lengths): 512 active frames or fewer (its own engines), more than 2048 (the column kernel,
 * "stack_exact_kernel<mad,follow>"), after nl_stack_set_exact, a handle without an exact list, a handle that cannot
 * hold the threshold record.
 *
 * Errors.  Arguments, checks and messages are those of the nl_stack_run_mad_weighted family: there is no mode argument
 * (the mode is NL_ST_MAD_SIGMA); a null handle or group is NL_ERR_INVALID_ARG; a handle without weights
 * (nl_stack_set_weights) fails with NL_ERR_INVALID_ARG and the same message before any device work.  It is a pass:
 * nl_stack_last_mode reports NL_ST_MAD_SIGMA, the result stays on the device for the nl_stack_result_* steps,
 * nl_stack_pass_times times it, and the _async form is finished by nl_stack_finish.  It runs the plain protocol, reads
 * and writes no list-length hints and never runs the fused protocol.
 *
 * nl_group_run_mad_weighted_deepstack fans out over the tiles as nl_group_run_mad_weighted does: all tiles are started
 * before any is awaited, every tile that started is finished, the first error with its message is returned, the totals
 * are summed and every tile writes its own rows of out_host. */
int nl_stack_run_mad_weighted_deepstack(nl_stack_t *h, float sigma_low, float sigma_high, float ref_loc,
                                        float *out_host, int64_t *clip_low, int64_t *clip_high);
int nl_stack_run_mad_weighted_deepstack_async(nl_stack_t *h, float sigma_low, float sigma_high, float ref_loc);
int nl_group_run_mad_weighted_deepstack(nl_group_t *g, float sigma_low, float sigma_high, float ref_loc,
                                        float *out_host, int64_t *clip_low, int64_t *clip_high);

#ifdef __cplusplus
}
#endif

#endif
