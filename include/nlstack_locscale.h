/* nlstack_locscale.h -- the location / scale entries of the C ABI of libnlstack.so.  Part of nlstack.h, which includes
 * it behind the types it needs: include nlstack.h, not this file. */
#ifndef NLSTACK_LOCSCALE_H
#define NLSTACK_LOCSCALE_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Stats.Location() / Scale(): updateLocationScale (internal/stats/stats.go:225-244) ----
 * The location and scale every later step takes as arguments, estimated on the resident frame, which never
 * crosses PCIe.  The estimator is the reference's global LSEstimator (stats.go:31-41; its default is
 * NL_LSE_SC_MEDIAN_QN), num_samples its numSamples (NL_LOCSCALE_SAMPLES, :226).
 *
 * Bit-exact given the seeds.  Each sampling function of the reference starts a fresh fastrand.RNG{}, whose zero
 * state the first draw replaces by a seed taken from the clock; everything behind that seed is deterministic fp32
 * and integer arithmetic.  Here the caller passes the seeds, one per sampling call in call order, and location,
 * scale and every integer of info are the reference's bits for those seeds (xorshift32 as in valyala/fastrand
 * v1.1.0, Uint32n(m) = the high 32 bits of x * m; the order statistics of NaN-free samples depend on the multiset
 * only, so the device selects by radix).  nl_locscale_seeds gives a caller that wants "any seed" its seeds.
 *   NL_LSE_MEAN_STDDEV   (:229-230) Mean() and float32(sqrt(variance)) as nl_stack_frame_stats gives them; no seed
 *   NL_LSE_MEDIAN_MAD    (:231-235) FastApproxMedian (:336-345), then FastApproxMAD (:401-410): 2 seeds
 *   NL_LSE_IKSS          (:236-237, :535-566) sorts the whole frame: not implemented on the device, NL_ERR_INVALID_ARG
 *   NL_LSE_SC_MEDIAN_QN  (:238-239) FastApproxSigmaClippedMedianAndQn(data, 2, 2, (Max() - Min()) / 65535, n)
 *                        (:477-499) over FastApproxMedian, FastApproxQn (:436-447), FastApproxBoundedMedian
 *                        (:349-364) and FastApproxBoundedQn (:450-472): NL_LOCSCALE_MAX_SEEDS seeds, of which
 *                        3 + 2 * iterations are used.  Its quirks are kept: sigmaLow bounds both sides, the loop
 *                        ends at i >= 10, and the location returned is the one before the last iteration.
 *   NL_LSE_HISTOGRAM     (:240-241) HistogramScaleLoc (:640-688) with 4096 bins: the bins are counted on the device
 *                        (integers, exact), peak and cumulation run on the host literally; no seed
 * min_max: NULL takes Min() / Max() from the frame (as nl_stack_frame_stats); else the caller's cached
 * Stats.Min() / Max(), which differ from the frame's after UpdateCachedWith (:91-99).  Read by estimators 3
 * (epsilon) and 4.  seeds is read by estimators 1 and 3 only.  info may be NULL.
 * Errors, NL_ERR_INVALID_ARG with a message naming the site, where the reference panics, never returns, or
 * cannot be restated: a zero seed (the reference would replace it) or too few seeds; num_samples outside
 * [4, 2^20]; a frame of fewer than 2 or of 2^31 or more pixels; a row-tile handle (the samples come from the
 * whole frame); a NaN among the samples of a call (QSelectFloat32 requires NaN-free input); a pixel whose
 * histogram bin is outside [0, 4096) (a NaN pixel, a stale min_max).
 * Deviations, where the reference returns something else:
 *   1. the draw budget: a bounded call that has consumed 16 * num_samples draws (median) or 32 * num_samples
 *      draws (Qn) without filling its samples fails with "fewer than 1 in 16 draws within [lo, hi]"; the
 *      reference would go on drawing, forever when the bounds are empty or NaN.  The handle stays usable.
 *   2. where the selected rank is tied between -0 and +0 the device may return the other zero (the reference's
 *      choice depends on the order its quickselect leaves).
 *   3. num_samples above 2^20 is an error (the reference takes any count; its own is 131072).
 *   4. estimator 0 is nl_stack_frame_stats' mean and variance: the fp64 sums are added in another order than
 *      the reference's sequential loop, so location and scale may differ from it by one fp32 ulp (the
 *      tolerance the mean of nl_stack_frame_stats has always had).  Without a device every entry but nl_locscale_seeds fails with NL_ERR_NO_DEVICE (argument errors
 * that need no device come first). */
enum { NL_LSE_MEAN_STDDEV = 0, NL_LSE_MEDIAN_MAD = 1, NL_LSE_IKSS = 2, NL_LSE_SC_MEDIAN_QN = 3, NL_LSE_HISTOGRAM = 4 };  /* stats.go:31-37 */
#define NL_LOCSCALE_SAMPLES 131072   /* stats.go:226 */
#define NL_LOCSCALE_MAX_SEEDS 25
typedef struct nl_locscale {
    int32_t iterations;              /* estimator 3: iterations of the loop run, i + 1 at its exit (1 .. 11); else 0 */
    int32_t converged;               /* estimator 3: 1 = the epsilon test ended the loop, 0 = i >= 10 did; else 0 */
    int32_t seeds_used;              /* sampling calls made (on an error: completed) */
    uint32_t draws[NL_LOCSCALE_MAX_SEEDS];   /* draws each call consumed, in call order; 0 behind seeds_used */
    float min, max, epsilon;         /* the Min() / Max() used and (max - min) / 65535 (:239) */
    uint32_t peak_bin, peak_count;   /* estimator 4: the inner peak (:657-662) */
    uint32_t half_width;             /* estimator 4: the last i of the cumulation (:678-684), 0 when it never ran */
} nl_locscale_t;
/* On resident slot idx of a whole-image handle; idx < 0: on the last pass's result. */
int nl_stack_frame_location_scale(nl_stack_t *h, int idx, int estimator, int num_samples,
                                  const uint32_t *seeds, int n_seeds, const float *min_max /* [2] or NULL */,
                                  float *location, float *scale, nl_locscale_t *info /* may be NULL */);
/* One host frame on a handle of its own per call: safe to call from several host threads at once. */
int nl_location_scale(const float *data_host, int width, int height, int estimator, int num_samples,
                      const uint32_t *seeds, int n_seeds, const float *min_max, float *location, float *scale,
                      nl_locscale_t *info, int device);
/* n nonzero seeds from one key (splitmix64; host only, needs no device): deterministic in key. */
int nl_locscale_seeds(uint64_t key, uint32_t *seeds, int n);

#ifdef __cplusplus
}
#endif

#endif
