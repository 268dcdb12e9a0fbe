/* nlstack_wlinfit.h -- the weighted linear-fit pass, entries of the C ABI of libnlstack.so.  AN EXTENSION: the reference
 * has no such mode.  Part of nlstack.h, which includes it behind the types it needs: include nlstack.h, not this file. */
#ifndef NLSTACK_WLINFIT_H
#define NLSTACK_WLINFIT_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- linear-fit rejection + weighted mean of the survivors (labelled extension) ----
 * The reference's StackLinearFit takes no weights (internal/ops/stack/stack.go:188-189, :834): -stWeight with
 * -stMode 5 computes the weights and drops them, and so does nl_stack_run with NL_ST_LINEAR_FIT, which stays as it is.
 * The pass declared here rejects by the fit, as the reference does, and averages the survivors with the frames'
 * weights, which the reference does not.  There is no reference to compare it with: this text is the contract.
 *
 * Definition.  Per pixel, over the active frames k = 0 ... N-1 with sample v_k and weight w_k:
 *   1. Gather.  Keep the frames with v_k == v_k: NaN dropped, +-Inf kept (stack.go:380-387).  n of them remain.
 *      n == 0 gives ref_loc and touches no counter.
 *   2. Rejection.  StackLinearFit's loop runs on the values exactly as in the reference (stack.go:869-911,
 *      stats.go:569-586); the weights take no part in it.  clip_low / clip_high are therefore identical to those of
 *      the unweighted pass over the same frames.  S is the set of SORTED POSITIONS the LAST regression ran over: the
 *      survivors BEFORE the final rejection sweep -- the set whose ymean the reference returns.
 *   3. Which frames.  Order the gathered frames by (value ascending, frame index ascending); sorted position r
 *      belongs to the r-th frame of that order.  +0 and -0 compare equal.  (The reference's sort is unstable; without
 *      weights it cannot tell equal samples apart, so this tie rule contradicts nothing.)  K = the frames whose
 *      position is in S.
 *   4. Result.  In ascending FRAME INDEX over k in K: num += v_k * w_k; den += w_k -- both fp32, sequential, never
 *      fused -- and the result is num / den.  This is StackMeanWeighted's arithmetic (stack.go:343-364) restricted to
 *      K: when nothing is rejected the result equals the weighted mean mode bit for bit.  den == 0 and NaN weights
 *      give what that division gives.
 *
 * The entries.  The weights are those of nl_stack_set_weights / nl_group_set_weights; without weights the call fails
 * with NL_ERR_INVALID_ARG before any device work (use nl_stack_run with NL_ST_LINEAR_FIT for the unweighted fit).
 * nl_stack_set_active_frames applies.  It is a pass: nl_stack_last_mode reports NL_ST_LINEAR_FIT, the result stays on
 * the device for the nl_stack_result_* steps, nl_stack_pass_times times it, and the _async form is finished by
 * nl_stack_finish.  Up to 128 active frames a register-resident kernel runs the fit, one pixel per lane
 * (nl_stack_last_kernel_name: "stack_linfit_weighted_kernel<64>"), and hands the pixels it cannot decide -- more than
 * four runs of survivors, a group of equal samples split by the rejection, a +-Inf sample -- to the one-pixel-per-lane
 * column kernel; nl_stack_last_fallback_pixels counts them.  Deeper stacks, and every stack after
 * nl_stack_set_exact(h, 1), run on the column kernel alone ("stack_exact_kernel<linfit,weighted>").  Both engines
 * compute the definition above bit for bit.  Like a maps pass it leaves later default passes as they would have been
 * without it: it forces no bit-exact kernels, reads and writes no list-length hints and never runs the fused protocol.
 *
 * nl_group_run_linfit_weighted fans out over the tiles as nl_group_run does: all tiles are started before any is
 * awaited, every tile that started is finished, the first error with its message is returned, the totals are summed
 * and every tile writes its own rows of out_host. */
int nl_stack_run_linfit_weighted(nl_stack_t *h, float sigma_low, float sigma_high, float ref_loc,
                                 float *out_host, int64_t *clip_low, int64_t *clip_high);
int nl_stack_run_linfit_weighted_async(nl_stack_t *h, float sigma_low, float sigma_high, float ref_loc);
int nl_group_run_linfit_weighted(nl_group_t *g, float sigma_low, float sigma_high, float ref_loc,
                                 float *out_host, int64_t *clip_low, int64_t *clip_high);

#ifdef __cplusplus
}
#endif

#endif
