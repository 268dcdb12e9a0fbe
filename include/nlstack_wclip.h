/* nlstack_wclip.h -- weighted sigma / winsorized clipping whose weights follow their frames, entries of the C ABI of
 * libnlstack.so.  AN EXTENSION: the reference has no such mode.  Part of nlstack.h, which includes it behind the types
 * it needs: include nlstack.h, not this file. */
#ifndef NLSTACK_WCLIP_H
#define NLSTACK_WCLIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- sigma / winsorized rejection + the mean of the survivors, each with ITS OWN frame's weight (labelled extension) ----
 * The reference's StackSigmaWeighted / StackWinsorSigmaWeighted (internal/ops/stack/stack.go:442-531, :710-829) let
 * QSelectMedianFloat32 permute the samples while the weights follow only the clip swaps (stack.go:487): a survivor is
 * multiplied by whichever weight ended up in its slot.  nl_stack_run with weights reproduces that bit for bit by
 * replaying the permutation, and stays as it is.  The pass declared here applies frame k's weight to frame k's
 * sample, which is what a user of noise or HFR weighting asks for.  There is no reference to compare it with: this
 * text is the contract.
 *
 * Definition.  mode is NL_ST_SIGMA or NL_ST_WINSOR_SIGMA.  Per pixel, over the active frames k = 0 ... N-1 with sample
 * v_k and weight w_k:
 *   1. Gather.  Keep the frames with v_k == v_k: NaN dropped, +-Inf kept (stack.go:380-387).  n of them remain.
 *      n == 0 gives ref_loc and touches no counter.
 *   2. Rejection.  The loop of StackSigma / StackWinsorSigma runs on the values alone, exactly as in the reference
 *      (stack.go:401-431, :641-698); the weights take no part in it.  clip_low / clip_high are therefore those of the
 *      unweighted pass over the same frames, and those of nl_stack_run with weights.  The tests g < lowBound /
 *      else if g > highBound are predicates on the value: equal samples share their fate, so "which frames survive"
 *      needs no tie rule.
 *   3. K = the frames still in gatheredCur when the loop breaks, i.e. AFTER the last removal sweep: the set the
 *      reference's weighted functions average (stack.go:514-522).  (The unweighted functions return a mean taken
 *      BEFORE that sweep; the two sets differ only when the loop ends through len <= 1.)
 *   4. Result.  In ascending FRAME INDEX over k in K: num += v_k * w_k; den += w_k -- both fp32, sequential, never
 *      fused -- and the result is num / den.  This is StackMeanWeighted's arithmetic (stack.go:343-364) restricted to
 *      K: when nothing is rejected the result equals the weighted mean mode bit for bit.  An empty K, den == 0 and
 *      NaN weights give what that division gives.  Against "the reference with its weights permuted alongside the
 *      samples" the result differs by the order of summation only.
 *
 * The entries.  NL_ST_AUTO is resolved by the frame count (stack.go:45-55); a resolved mode other than the two is
 * NL_ERR_INVALID_MODE.  The weights are those of nl_stack_set_weights / nl_group_set_weights; without weights the call
 * fails with NL_ERR_INVALID_ARG before any device work (use nl_stack_run for the unweighted pass).
 * nl_stack_set_active_frames applies.  It is a pass: nl_stack_last_mode reports the resolved mode, the result stays on
 * the device for the nl_stack_result_* steps, nl_stack_pass_times times it, and the _async form is finished by
 * nl_stack_finish.
 *
 * Engines.  From 9 to 512 active frames the decision pass of the weighted stacks leaves, per pixel and clipping
 * round, thresholds that reproduce the reference's decisions; one streaming read of the frames in frame order
 * (nl_stack_last_kernel_name: "stack_clip_weighted_kernel<4>") tests every sample against its pixel's thresholds and
 * accumulates num and den.  Pixels without a complete record -- no round on record, or a last recorded round after
 * which the reference's loop would go on -- go to the one-pixel-per-lane column kernel; nl_stack_last_fallback_pixels
 * counts them.  Up to 8 frames, beyond 512, and every stack after nl_stack_set_exact(h, 1), run on the column kernel
 * alone ("stack_exact_kernel<sigma,follow>", "stack_exact_kernel<winsor,follow>").  Both engines call one accumulation
 * function and compute the definition above bit for bit.  Like a maps pass it leaves later default passes as they
 * would have been without it: it forces no bit-exact kernels, reads and writes no list-length hints and never runs the
 * fused protocol.
 *
 * nl_group_run_clip_weighted fans out over the tiles as nl_group_run does: all tiles are started before any is
 * awaited, every tile that started is finished, the first error with its message is returned, the totals are summed
 * and every tile writes its own rows of out_host. */
int nl_stack_run_clip_weighted(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc,
                               float *out_host, int64_t *clip_low, int64_t *clip_high);
int nl_stack_run_clip_weighted_async(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc);
int nl_group_run_clip_weighted(nl_group_t *g, int mode, float sigma_low, float sigma_high, float ref_loc,
                               float *out_host, int64_t *clip_low, int64_t *clip_high);

#ifdef __cplusplus
}
#endif

#endif
