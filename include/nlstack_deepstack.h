/* nlstack_deepstack.h -- the median and MAD sigma of 513 ... 2048 frames on register-resident engines, entries of the C
 * ABI of libnlstack.so.  AN EXTENSION OF DEPTH, NOT OF SEMANTICS: what the entries compute is what nl_stack_run computes
 * for the same mode; they add engines beyond 512 frames, where nl_stack_run keeps its wave-per-pixel and column kernels.
 * Part of nlstack.h, which includes it behind the types it needs: include nlstack.h, not this file. */
#ifndef NLSTACK_DEEPSTACK_H
#define NLSTACK_DEEPSTACK_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- nl_stack_run for deep stacks: both modes whose decisions rest on order statistics alone ----
 * For sigma, winsorized and linear-fit clipping the reference's answer to deep stacks is a stack of stacks
 * (OpStackBatches, nl_stack_accumulate).  A mean of batch medians is not the median, and the MAD bounds need both medians
 * of the whole column: these two modes need all frames of a pixel at once.
 *
 * Definition per mode.
 *   NL_ST_MEDIAN (stack.go:274-303).  Per pixel, the samples v_k == v_k of the active frames (NaN dropped, +-Inf kept), n
 *     of them: the (n>>1)-th smallest (counted from 0) for odd n, 0.5f * ((n>>1)-1-th + (n>>1)-th) for even n; ref_loc for
 *     n == 0.  An order statistic: the result equals nl_stack_run(NL_ST_MEDIAN)'s BIT FOR BIT, clip_low = clip_high = 0.
 *     Weights are ignored, as everywhere (stack.go:188-189).
 *   NL_ST_MAD_SIGMA (stack.go:536-605), without weights.  median as above; d_i = |v_i - median|; mad = the same median of
 *     the d_i; sd = mad * 1.4826f; lo = median - sigma_low * sd, hi = median + sigma_high * sd -- two roundings per bound,
 *     never fused.  v < lo counts low, else v > hi counts high.  Both medians are order statistics, so the bounds and every
 *     decision are exact: clip_low / clip_high equal nl_stack_run(NL_ST_MAD_SIGMA)'s COUNT FOR COUNT.  The result is the fp32
 *     mean of the same survivors, summed per lane (frames r, r + L, r + 2L, ... of the pixel's L lanes) and then over the
 *     lanes, where the reference sums them in the order its quickselect leaves: it agrees with the reference to the
 *     relative 1e-5 the 129 ... 512-frame MAD kernels of nl_stack_run are held to.  It is bit-equal to nl_stack_run's for
 *     the pixels of the exact list (no finite median: half or more of the samples infinite) and for pixels without a
 *     sample (ref_loc, no counts).
 *
 * Engines.  With 513 ... 1024 ACTIVE frames (nl_stack_set_active_frames) 8 adjacent lanes share a pixel, with
 * 1025 ... 2048 frames 16, each lane holding 128 samples in registers: the kernels of the 129 ... 512-frame engines with
 * more merge levels.  nl_stack_last_kernel_name reports "stack_median_ml_kernel<8>" / "stack_median_ml_kernel<16>" and
 * "stack_mad_ml_kernel<8>" / "stack_mad_ml_kernel<16>".  MAD sigma needs the handle's exact list (every handle but those
 * of huge tiles has one): pixels without a finite median go to the one-pixel-per-lane column kernel behind the dominant
 * kernel, and nl_stack_last_fallback_pixels counts them.
 *
 * Fall-throughs.  Every other case runs the pass nl_stack_run would run, in every observable respect (result, counters,
 * kernel name, protocol, list-length hints): another mode; 512 active frames or fewer, or more than 2048; after
 * nl_stack_set_exact(h, 1); MAD sigma on a handle without an exact list; a frame stride of 2^26 pixels or more at 8
 * lanes, 2^25 or more at 16 (L frames must lie within a signed 32-bit byte offset).
 *
 * Arguments, checks and messages are nl_stack_run's: NL_ERR_INVALID_MODE for a mode outside the enumeration, NL_ST_AUTO
 * resolved by the active frame count, and MAD sigma on a handle with weights fails with NL_ERR_WEIGHTED_MAD (the weighted
 * pass is nl_stack_run_mad_weighted, up to 512 frames on its own engines).  It is a pass: nl_stack_last_mode reports the
 * mode, the result stays on the device for the nl_stack_result_* steps, nl_stack_pass_times times it, and the _async form
 * is finished by nl_stack_finish.  On its own engines the pass reads and writes no list-length hints and never runs the
 * fused protocol: a default pass behind it is what it would have been without it.
 *
 * nl_group_run_deepstack fans out over the tiles as nl_group_run does: all tiles are started before any is awaited,
 * every tile that started is finished, the first error with its message is returned, the totals are summed and every
 * tile writes its own rows of out_host. */
int nl_stack_run_deepstack(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc,
                           float *out_host, int64_t *clip_low, int64_t *clip_high);
int nl_stack_run_deepstack_async(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc);
int nl_group_run_deepstack(nl_group_t *g, int mode, float sigma_low, float sigma_high, float ref_loc,
                           float *out_host, int64_t *clip_low, int64_t *clip_high);

#ifdef __cplusplus
}
#endif

#endif
