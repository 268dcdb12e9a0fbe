/* nlstack_wmad.h -- weighted MAD-sigma stacking whose weights follow their frames, entries of the C ABI of
 * libnlstack.so.  AN EXTENSION: the reference panics on MAD sigma with weights (internal/ops/stack/stack.go:185).  Part
 * of nlstack.h, which includes it behind the types it needs: include nlstack.h, not this file. */
#ifndef NLSTACK_WMAD_H
#define NLSTACK_WMAD_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- StackMADSigma's rejection + the mean of the survivors, each with ITS OWN frame's weight (labelled extension) ----
 * nl_stack_run and every nl_stack_run_maps* entry keep failing with NL_ERR_WEIGHTED_MAD for MAD sigma with weights, and
 * nl_stack_run_clip_weighted keeps refusing the mode: the pass declared here is the one entry that takes it.  There is
 * no reference to compare it with: this text is the contract.
 *
 * Definition.  Per pixel, over the active frames k = 0 ... N-1 with sample v_k and weight w_k:
 *   1. Gather.  Keep the frames with v_k == v_k: NaN dropped, +-Inf kept (stack.go:380-397).  n of them remain.
 *      n == 0 gives ref_loc and touches no counter.
 *   2. Rejection.  StackMADSigma's (stack.go:565-592) on the values alone; the weights take no part in it.  With
 *      k = (n>>1)+1: median = the k-th smallest sample for odd n, 0.5f * ((k-1)-th + k-th) for even n;
 *      d_i = v_i - median, negated if < 0; mad = the same median of the d_i; sd = mad * 1.4826f;
 *      lo = median - sigma_low * sd, hi = median + sigma_high * sd -- two roundings per bound, never fused.  v < lo counts
 *      low, else v > hi counts high; a NaN bound rejects nothing.  clip_low / clip_high therefore equal those of
 *      nl_stack_run(NL_ST_MAD_SIGMA) without weights over the same frames.  Both medians are order statistics, so the
 *      bounds, every decision and both counters do not depend on any order.
 *   3. K = the frames that are neither low nor high.
 *   4. Result.  In ascending FRAME INDEX over k in K: num += v_k * w_k; den += w_k -- both fp32, sequential, never
 *      fused -- and the result is num / den.  This is StackMeanWeighted's arithmetic (stack.go:343-364) restricted to
 *      K: when nothing is rejected the result equals the weighted mean mode bit for bit.  An empty K, den == 0 and
 *      NaN weights give what that division gives.
 *   5. A median that is not finite (half or more of the samples infinite).  The reference's second quickselect is
 *      undefined there (the deviations hold Inf - Inf) and can panic.  Here the counters are those of the unweighted
 *      MAD pass (nl_stack_run(NL_ST_MAD_SIGMA), whose column kernel takes such pixels), and K follows from the bounds
 *      that kernel computes.  For sigma_low, sigma_high >= 0 those bounds reject nothing, whatever the second median
 *      comes to: a median of +Inf gives lo = Inf - Inf = NaN (or Inf - NaN) and hi = +Inf or NaN, -Inf mirrors that, and a NaN
 *      median (as many -Inf as +Inf around the middle) gives two NaN bounds -- K is every sample.  With a negative sigma the bounds of such
 *      a pixel depend on the order the column kernel's selection leaves, as they do in the unweighted pass.
 *
 * The entries.  There is no mode argument: the mode is NL_ST_MAD_SIGMA.  The weights are those of nl_stack_set_weights /
 * nl_group_set_weights; without weights the call fails with NL_ERR_INVALID_ARG before any device work (the unweighted
 * pass is nl_stack_run with NL_ST_MAD_SIGMA).  nl_stack_set_active_frames and nl_stack_set_exact apply.  It is a pass:
 * nl_stack_last_mode reports NL_ST_MAD_SIGMA, the result stays on the device for the nl_stack_result_* steps,
 * nl_stack_pass_times times it, and the _async form is finished by nl_stack_finish.
 *
 * Engines.  All of them compute the definition above bit for bit: they take the bounds from two medians and call one
 * accumulation function under that single round.  Up to 128 active frames the register-resident MAD kernels run in
 * their <follow> instantiations (nl_stack_last_kernel_name: "stack_mad_fast_kernel<NS, true>"; from 114 frames on
 * "stack_mad_bitonic_kernel<true>", which hands pixels with fewer than 114 samples to "stack_mad_fast_kernel<128, true>"):
 * their second read of the frames is in frame order already.  From 129 to 512 frames the multi-lane MAD kernel, record
 * only, leaves each pixel's (lo, hi), and one streaming read of the frames in frame order accumulates under them
 * ("stack_clip_weighted_kernel<4, true>").  Pixels without a finite median -- and, in the streaming engine, pixels
 * without a sample -- go to the one-pixel-per-lane column kernel; nl_stack_last_fallback_pixels counts them.  Beyond
 * 512 frames, and every stack after nl_stack_set_exact(h, 1), run on the column kernel alone
 * ("stack_exact_kernel<mad,follow>").  Like the other two weighted extensions the pass leaves later default passes as
 * they would have been without it: it forces no bit-exact kernels, reads and writes no list-length hints and never
 * runs the fused protocol.
 *
 * nl_group_run_mad_weighted fans out over the tiles as nl_group_run does: all tiles are started before any is awaited,
 * every tile that started is finished, the first error with its message is returned, the totals are summed and every
 * tile writes its own rows of out_host. */
int nl_stack_run_mad_weighted(nl_stack_t *h, float sigma_low, float sigma_high, float ref_loc,
                              float *out_host, int64_t *clip_low, int64_t *clip_high);
int nl_stack_run_mad_weighted_async(nl_stack_t *h, float sigma_low, float sigma_high, float ref_loc);
int nl_group_run_mad_weighted(nl_group_t *g, float sigma_low, float sigma_high, float ref_loc,
                              float *out_host, int64_t *clip_low, int64_t *clip_high);

#ifdef __cplusplus
}
#endif

#endif
