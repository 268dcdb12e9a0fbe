// stack_exact.hip -- bit-exact per-pixel stacking kernels for gfx950 (MI355X).
//
// One wavefront per workgroup, one pixel per lane.  Each lane owns a column of
// the workgroup's LDS tile laid out [slot][lane] (bank = lane, so the
// data-dependent slot index of quickselect / swap-with-last never conflicts),
// and runs the reference's per-pixel algorithm in the reference's order, so
// that fp32 sums see the same permutation and results match bit for bit:
//   gather        internal/ops/stack/stack.go:380-387 (frame order, NaN skipped)
//   quickselect   internal/qsort/qsort.go:68-126     (Hoare, middle pivot, in place)
//   mean/stddev   internal/stats/stats.go:246-261    (two sequential fp32 passes)
//   sigma clip    stack.go:401-431, weighted :484-524
//   winsorized    stack.go:641-698, weighted :753-821
//   MAD           stack.go:565-600
//   linear fit    stack.go:869-911, stats.go:569-586
//   median        stack.go:274-303
// Build flags that matter for parity: -ffp-contract=off (Go/amd64 never fuses
// a*b+c) and -fhip-fp32-correctly-rounded-divide-sqrt (IEEE divide / sqrt).
//
// Roofline: HBM-bound by construction (4*(N+1) bytes per output pixel, each
// sample read exactly once with 256-byte coalesced rows per frame); in this
// exact form the kernel is limited by per-lane LDS latency and VALU issue,
// see DESIGN.md section 4.
#include "launch_common.hpp"
#include "wave_lists.hpp"
#include "wclip_common.hpp"

namespace nl {

// ---- a lane's column in the [slot][lane] LDS tile -------------------------
template <int S>
struct Col {
    float *p;
    bool live;      // lanes beyond LANES (narrow tiles) alias lane 0's column: they may read it, never write it
    __device__ __forceinline__ float get(int i) const { return p[i * S]; }
    __device__ __forceinline__ void set(int i, float v) const { if (live) p[i * S] = v; }
    __device__ __forceinline__ Col<S> shifted(int k) const { return Col<S>{p + k * S, live}; }
};

// qsort.go:94-126, k is 1-based
template <int S>
__device__ float hoare_select(Col<S> a, int n, int k)
{
    int left = 0, right = n - 1;
    while (left < right) {
        const float pivot = a.get((left + right) >> 1);
        int l = left - 1, r = right + 1;
        for (;;) {
            float al, ar;
            // (the index guards never fire on NaN-free data; they keep a NaN -- only possible in
            // MAD deviations of a pixel with an infinite median, where the reference itself dies
            // with an index panic -- from sending the scan past the column forever)
            do { l++; al = a.get(l); } while (!(al >= pivot) && l < right);
            do { r--; ar = a.get(r); } while (!(ar <= pivot) && r > left);
            if (l >= r) break;
            a.set(l, ar);
            a.set(r, al);
        }
        const int offset = r - left + 1;
        if (k <= offset) {
            right = r;
        } else {
            left = r + 1;
            k -= offset;
        }
    }
    return a.get(left);
}

// qsort.go:68-82
template <int S>
__device__ float select_median(Col<S> a, int n)
{
    const int k = (n >> 1) + 1;
    const float upper = hoare_select(a, n, k);
    float res = upper;
    if ((n & 1) == 0) {
        float lower = a.get(0);
        for (int i = 1; i < k - 1; i++) {
            const float v = a.get(i);
            if (v > lower) lower = v;
        }
        res = 0.5f * (lower + upper);
    }
    return res;
}

// stats.go:246-261
template <int S>
__device__ void mean_stddev(Col<S> a, int n, float &mean, float &sd)
{
    float s = 0.0f;
    for (int i = 0; i < n; i++) s += a.get(i);
    const float fn = (float)n;
    const float m = s / fn;
    float v = 0.0f;
    for (int i = 0; i < n; i++) {
        const float d = a.get(i) - m;
        v += d * d;
    }
    v = v / fn;
    mean = m;
    sd = sqrt_go(v);
}

// stack.go:411-424 (+ :494-511 with the mirrored weight column)
template <int S, bool W>
__device__ int clip_pass(Col<S> a, Col<S> w, int n, float lo, float hi, int &c_lo, int &c_hi)
{
    int j = 0;
    while (j < n) {
        const float g = a.get(j);
        const bool low = g < lo;
        const bool high = !low && (g > hi);
        if (low || high) {
            n--;
            a.set(j, a.get(n));
            if (W) w.set(j, w.get(n));
            c_lo += low ? 1 : 0;
            c_hi += high ? 1 : 0;
        } else {
            j++;
        }
    }
    return n;
}

// stack.go:514-522
template <int S>
__device__ float weighted_mean(Col<S> a, Col<S> w, int n)
{
    float s = 0.0f, ws = 0.0f;
    for (int i = 0; i < n; i++) {
        const float wi = w.get(i);
        const float p = a.get(i) * wi;
        s += p;
        ws += wi;
    }
    return s / ws;
}

// stack.go:646-672.  The reference copies the column and clamps the copy
// repeatedly; all clamp intervals share the centre `median`, so after any
// number of rounds the copy equals clamp(a[i], max(lo_j), min(hi_j)).  We keep
// only those two running bounds and re-derive the copy on the fly: identical
// values in identical order, no second column.
template <int S>
__device__ float winsorized_stddev(Col<S> a, int n, float median, float sd)
{
    float Leff = -__builtin_inff(), Heff = __builtin_inff();
    const float fn = (float)n;
    for (;;) {
        const float t = 1.5f * sd;
        const float lo = median - t, hi = median + t;
        int changed = 0;
        float s = 0.0f;
        const float Lnew = fmaxf(Leff, lo), Hnew = fminf(Heff, hi);
        const bool ok = (lo == lo);   // NaN stddev: every comparison false, nothing changes
        for (int i = 0; i < n; i++) {
            const float x = a.get(i);
            float wz = fminf(fmaxf(x, Leff), Heff);       // copy before this round
            if (ok) {
                if (wz < lo) { wz = lo; changed++; }
                else if (wz > hi) { wz = hi; changed++; }
            }
            s += wz;
        }
        if (ok) { Leff = Lnew; Heff = Hnew; }
        const float m = s / fn;
        float v = 0.0f;
        for (int i = 0; i < n; i++) {
            const float wz = fminf(fmaxf(a.get(i), Leff), Heff);
            const float d = wz - m;
            v += d * d;
        }
        v = v / fn;
        const float old = sd;
        sd = 1.134f * sqrt_go(v);
        const float factor = fabsf(sd - old) / old;
        if (changed == 0 || factor <= 0.0005f) break;
    }
    return sd;
}

// In-column bitonic sort, ascending, n_pad = power of two; every lane runs the
// same compare-exchange sequence (no divergence, no bank conflicts).  A sorted
// column is unique, so any sorting algorithm reproduces qsort.go:26-32 exactly.
template <int S>
__device__ void bitonic_sort(Col<S> a, int n_pad)
{
    for (int k = 2; k <= n_pad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int half = n_pad >> 1;
            for (int t = 0; t < half; t++) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const float x = a.get(i), y = a.get(l);
                const float mn = fminf(x, y), mx = fmaxf(x, y);
                const bool asc = (i & k) == 0;
                a.set(i, asc ? mn : mx);
                a.set(l, asc ? mx : mn);
            }
        }
    }
}

// The same network on (value, index) pairs: ascending by value, equal values (+0 == -0) by index.  The
// weighted linear-fit pass only: it has to know WHICH frame sits at a sorted position.
template <int S>
__device__ void bitonic_sort_keyed(Col<S> a, Col<S> b, int n_pad)
{
    for (int k = 2; k <= n_pad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int half = n_pad >> 1;
            for (int t = 0; t < half; t++) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const float x = a.get(i), y = a.get(l);
                const float xi = b.get(i), yi = b.get(l);
                const bool y_first = y < x || (y == x && __float_as_int(yi) < __float_as_int(xi));
                const bool asc = (i & k) == 0;
                if (y_first == asc) {
                    a.set(i, y); a.set(l, x);
                    b.set(i, yi); b.set(l, xi);
                }
            }
        }
    }
}

// The weighted clip pass whose weights follow their frames (include/nlstack_wclip.h; no counterpart in the
// reference), behind the UNWEIGHTED rejection loop: slots 0 .. n-1 of the column hold the survivors K.  A
// sample's fate is a predicate on its value and the survivors of a chain of intervals are the samples inside
// one interval, so K = the samples in [min K, max K] (an empty K has no interval: nothing is in).  The frames
// are read again in frame order and go through the accumulation the streaming kernel uses (wclip_take).
template <int S>
__device__ float follow_mean(Col<S> a, int n, const float *fr, const StackArgs &p)
{
    float2 bd = make_float2(__builtin_inff(), -__builtin_inff());      // (no sample is inside)
    if (n > 0) {
        float mn = a.get(0), mx = mn;
        for (int i = 1; i < n; i++) {
            const float g = a.get(i);
            mn = g < mn ? g : mn;
            mx = g > mx ? g : mx;
        }
        bd = make_float2(mn, mx);
    }
    WclipAcc acc;
    for (int k = 0; k < p.n_frames; k++) wclip_take<0>(fr[(int64_t)k * p.stride], p.weights[k], nullptr, bd, acc);
    return acc.num / acc.den;
}

// ---- the kernel -----------------------------------------------------------
// MODE: NL_ST_* (0 median, 2 sigma, 3 winsor, 4 MAD, 5 linear fit);
// W: weighted (sigma / winsor; with the linear fit: the weighted linear-fit
// pass of include/nlstack_wlinfit.h, an extension); LANES: pixels per wavefront (64/32/16,
// smaller when a 64-wide tile would not fit the 160 KiB LDS); MAPS: the maps
// pass (nl_stack_run_maps) -- the lane also stores its pixel's own two clip
// counts, p.reject_map[pix] (whole tile, or the listed pixels: the replay of
// the fast maps pass; no other instantiation reads it).  FOLLOW (sigma / winsor,
// W = false): the weighted clip pass whose weights follow their frames
// (include/nlstack_wclip.h, an extension) -- the unweighted rejection, then
// follow_mean over the frames; p.weights is set.  FOLLOW with MAD sigma: the
// weighted MAD-sigma pass (include/nlstack_wmad.h, an extension) -- the
// unweighted bounds, then the frames in frame order under them.
template <int MODE, bool W, int LANES, bool MAPS = false, bool FOLLOW = false>
__global__ __launch_bounds__(64) void stack_exact_kernel(StackArgs p)
{
    extern __shared__ float lds[];
    const int lane = threadIdx.x;
    const bool lane_on = lane < LANES;
    const int n_alloc = (MODE == NL_ST_LINEAR_FIT) ? p.n_pad : p.n_frames;
    Col<LANES> a{lds + (lane_on ? lane : 0), lane_on};
    Col<LANES> b{lds + (size_t)n_alloc * LANES + (lane_on ? lane : 0), lane_on};   // weights / abs-dev column

    int c_lo = 0, c_hi = 0;

    // list mode: redo only the pixels a fast kernel could not decide
    int64_t limit = p.npix, tiles = p.tiles;
    if (p.list) {
        const unsigned cnt = *p.list_count;
        limit = cnt < p.list_capacity ? cnt : p.list_capacity;
        tiles = (limit + LANES - 1) / LANES;
    }

    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int c_lo0 = c_lo, c_hi0 = c_hi;      // (MAPS: the lane's running counts before this pixel)
        const int64_t idx = tile * LANES + lane;
        const bool on = lane_on && idx < limit;
        const int64_t pix = p.list ? (int64_t)p.list[on ? idx : 0] : idx;
        const float *fr = p.frames + (on ? pix : 0);

        // ---- gather (stack.go:380-387): frame order, NaN dropped ----
        int n = 0;
        int k = 0;
        const int N = p.n_frames;
        for (; k + 8 <= N; k += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = fr[(int64_t)(k + u) * p.stride];
            if (on) {
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    if (v[u] == v[u]) {
                        a.set(n, v[u]);
                        if (W) b.set(n, (MODE == NL_ST_LINEAR_FIT) ? __int_as_float(k + u) : p.weights[k + u]);
                        n++;
                    }
                }
            }
        }
        for (; k < N; k++) {
            const float v = fr[(int64_t)k * p.stride];
            if (on && v == v) {
                a.set(n, v);
                if (W) b.set(n, (MODE == NL_ST_LINEAR_FIT) ? __int_as_float(k) : p.weights[k]);
                n++;
            }
        }

        float res = p.ref_loc;     // stack.go:388-397: no valid sample -> RefFrameLoc

        if (MODE == NL_ST_MEDIAN) {
            if (n > 0) res = select_median(a, n);
        } else if (MODE == NL_ST_SIGMA || MODE == NL_ST_WINSOR_SIGMA) {
            if (n > 0) {
                for (;;) {
                    const float median = select_median(a, n);
                    float mean, sd;
                    mean_stddev(a, n, mean, sd);
                    if (MODE == NL_ST_WINSOR_SIGMA) sd = winsorized_stddev(a, n, median, sd);
                    const float t_lo = p.sig_lo * sd, t_hi = p.sig_hi * sd;
                    const float lo = median - t_lo, hi = median + t_hi;
                    const int before = n;
                    n = clip_pass<LANES, W>(a, b, n, lo, hi, c_lo, c_hi);
                    if (n == before || n <= 1) {
                        if constexpr (FOLLOW) res = follow_mean(a, n, fr, p);
                        else res = W ? weighted_mean(a, b, n) : mean;
                        break;
                    }
                }
            }
        } else if (MODE == NL_ST_MAD_SIGMA) {
            if (n > 0) {
                const float median = select_median(a, n);
                for (int i = 0; i < n; i++) {
                    float d = a.get(i) - median;
                    if (d < 0) d = -d;
                    b.set(i, d);
                }
                const float mad = select_median(b, n);
                const float sd = mad * 1.4826f;
                const float t_lo = p.sig_lo * sd, t_hi = p.sig_hi * sd;
                const float lo = median - t_lo, hi = median + t_hi;
                if constexpr (FOLLOW) {
                    // (the one round (lo, hi) decides every sample as clip_pass does: the counts come from the same calls)
                    WclipAcc acc;
                    for (int k2 = 0; k2 < N; k2++)
                        wclip_take<0>(fr[(int64_t)k2 * p.stride], p.weights[k2], nullptr, make_float2(lo, hi), acc);
                    c_lo += acc.lo;
                    c_hi += acc.hi;
                    res = acc.num / acc.den;
                } else {
                    n = clip_pass<LANES, false>(a, b, n, lo, hi, c_lo, c_hi);
                    float s = 0.0f;
                    for (int i = 0; i < n; i++) s += a.get(i);
                    res = s / (float)n;
                }
            }
        } else if (MODE == NL_ST_LINEAR_FIT && W) {
            // The weighted linear-fit pass (include/nlstack_wlinfit.h; no counterpart in the reference).  The
            // fit below is the unweighted branch's, operation for operation; what differs is what it keeps:
            // the second column carries every sample's FRAME INDEX through the sort -- keys (value, index),
            // pads (+Inf, N + slot) behind every real sample -- and through the stable compaction, and the
            // sweep that ends the loop does not compact, so that slots 0 .. n-1 of the index column name the
            // frames the LAST regression ran over.  Their samples are then averaged with the frames' weights
            // in frame order: StackMeanWeighted's arithmetic (stack.go:343-364) over those frames.
            for (int i = n; i < p.n_pad; i++) { a.set(i, __builtin_inff()); b.set(i, __int_as_float(N + i)); }
            bitonic_sort_keyed(a, b, p.n_pad);
            if (n > 0) {
                for (;;) {
                    const float fn = (float)n;
                    const float xm = p.xstat[2 * n], xsd = p.xstat[2 * n + 1];
                    float ym, ysd;
                    mean_stddev(a, n, ym, ysd);
                    float corr = 0.0f;
                    for (int i = 0; i < n; i++) {
                        const float dx = (float)i - xm;
                        const float dy = a.get(i) - ym;
                        const float d = dx * dy;
                        corr += d;
                    }
                    float den = xsd * ysd;
                    den = den * (fn + 1.0f);
                    corr = corr / den;
                    float slope = corr * ysd;
                    slope = slope / xsd;
                    const float sx = slope * xm;
                    const float icpt = ym - sx;
                    float sg = 0.0f;
                    for (int i = 0; i < n; i++) {
                        float lin = (float)i * slope;
                        lin = lin + icpt;
                        const float diff = a.get(i) - lin;
                        sg += fabsf(diff);
                    }
                    sg = sg / fn;
                    const float lb = p.sig_lo * sg, hb = p.sig_hi * sg;
                    const bool last = n < 3;            // this sweep ends the loop whatever it rejects: count only
                    int kept = 0;
                    for (int i = 0; i < n; i++) {
                        const float g = a.get(i);
                        float lin = (float)i * slope;
                        lin = lin + icpt;
                        const bool low = (lin - g) > lb;
                        const bool high = !low && ((g - lin) > hb);
                        if (low) c_lo++;
                        else if (high) c_hi++;
                        else {
                            if (!last) { a.set(kept, g); b.set(kept, b.get(i)); }
                            kept++;
                        }
                    }
                    if (kept == n || last) break;       // (nothing rejected: the compaction wrote every slot onto itself)
                    n = kept;
                }
                // the value column is free now: slot k = "frame k is one of the n frames of the last regression"
                for (int k2 = 0; k2 < N; k2++) a.set(k2, 0.0f);
                for (int i = 0; i < n; i++) a.set(__float_as_int(b.get(i)), 1.0f);
                float num = 0.0f, wsum = 0.0f;
                for (int k2 = 0; k2 < N; k2++) {
                    const float v = fr[(int64_t)k2 * p.stride];
                    if (a.get(k2) != 0.0f) {
                        const float wk = p.weights[k2];
                        const float pr = v * wk;
                        num += pr;
                        wsum += wk;
                    }
                }
                res = num / wsum;
            }
        } else if (MODE == NL_ST_LINEAR_FIT) {
            // pad the column with +Inf up to n_pad and sort once; rejects are
            // removed by stable compaction, which keeps the column sorted, so
            // the reference's per-iteration re-sort (stack.go:872) is implied.
            for (int i = n; i < p.n_pad; i++) a.set(i, __builtin_inff());
            bitonic_sort(a, p.n_pad);
            if (n > 0) {
                float mean = 0.0f;
                for (;;) {
                    const float fn = (float)n;
                    // stats.go:570 on xs = 0..n-1: depends on n only, tabulated on the host
                    const float xm = p.xstat[2 * n], xsd = p.xstat[2 * n + 1];
                    float ym, ysd;
                    mean_stddev(a, n, ym, ysd);
                    float corr = 0.0f;
                    for (int i = 0; i < n; i++) {
                        const float dx = (float)i - xm;
                        const float dy = a.get(i) - ym;
                        const float d = dx * dy;
                        corr += d;
                    }
                    float den = xsd * ysd;
                    den = den * (fn + 1.0f);
                    corr = corr / den;
                    float slope = corr * ysd;
                    slope = slope / xsd;
                    const float sx = slope * xm;
                    const float icpt = ym - sx;
                    mean = ym;
                    float sg = 0.0f;
                    for (int i = 0; i < n; i++) {
                        float lin = (float)i * slope;
                        lin = lin + icpt;
                        const float diff = a.get(i) - lin;
                        sg += fabsf(diff);
                    }
                    sg = sg / fn;
                    const float lb = p.sig_lo * sg, hb = p.sig_hi * sg;
                    int kept = 0;
                    for (int i = 0; i < n; i++) {
                        const float g = a.get(i);
                        float lin = (float)i * slope;
                        lin = lin + icpt;
                        const bool low = (lin - g) > lb;
                        const bool high = !low && ((g - lin) > hb);
                        if (low) c_lo++;
                        else if (high) c_hi++;
                        else { a.set(kept, g); kept++; }
                    }
                    const int left = n - kept;
                    if (left == 0 || n < 3) break;
                    n = kept;
                }
                res = mean;
            }
        }

        if (on) p.out[pix] = res;
        // a pixel's counts are bounded by its samples (every increment removes one): 16 bits each, nlstack_pass.hip
        // refuses a maps pass over more than 65 535 frames
        if (MAPS && on) p.reject_map[pix] = (unsigned)(c_lo - c_lo0) | ((unsigned)(c_hi - c_hi0) << 16);
    }

    const int t_lo = wave_sum(c_lo), t_hi = wave_sum(c_hi);
    if (lane == 0) add_clip_totals(partial_slot(p, blockIdx.x), t_lo, t_hi);
}

// zero_after: the scratch set goes back to all zeros behind the sums -- the clip slots and the two words of list
// lengths / snapshot behind them (kScratchWords) -- so that the next pass on the handle needs no memset in front
__global__ __launch_bounds__(256) void reduce_counters_kernel(unsigned long long *partial,
                                                               int n_slots,
                                                               unsigned long long *counters,
                                                               const unsigned *list_counts, int n_lists, int list_stride,
                                                               int zero_after)
{
    __shared__ unsigned long long s_lo[256], s_hi[256];
    unsigned long long lo = 0, hi = 0;
    for (int i = threadIdx.x; i < n_slots; i += 256) {
        lo += partial[2 * (size_t)i];
        hi += partial[2 * (size_t)i + 1];
    }
    s_lo[threadIdx.x] = lo;
    s_hi[threadIdx.x] = hi;
    __syncthreads();
    if (zero_after)
        for (int i = threadIdx.x; i < 2 * n_slots; i += 256) partial[i] = 0ull;
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            s_lo[threadIdx.x] += s_lo[threadIdx.x + off];
            s_hi[threadIdx.x] += s_hi[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        counters[0] = s_lo[0];
        counters[1] = s_hi[0];
        if (list_counts) {             // (chunked passes keep one pair of list lengths per chunk)
            unsigned fb = 0, gen = 0;
            for (int i = 0; i < n_lists; i++) { fb += list_counts[i * list_stride]; gen += list_counts[i * list_stride + 1]; }
            counters[2] = (unsigned long long)fb | ((unsigned long long)gen << 32);
        }
        if (zero_after) { partial[2 * n_slots] = 0ull; partial[2 * n_slots + 1] = 0ull; }
    }
}

// ---- host-side launcher ----------------------------------------------------
template <int MODE, bool W, bool MAPS = false, bool FOLLOW = false>
static hipError_t launch_exact(const StackArgs &args, int lanes, int grid, size_t lds_bytes, hipStream_t stream)
{
    Launcher L(stream);
    L(lanes == 64 ? stack_exact_kernel<MODE, W, 64, MAPS, FOLLOW> : lanes == 32 ? stack_exact_kernel<MODE, W, 32, MAPS, FOLLOW>
      : lanes == 16 ? stack_exact_kernel<MODE, W, 16, MAPS, FOLLOW> : stack_exact_kernel<MODE, W, 4, MAPS, FOLLOW>, grid, 64, lds_bytes, args);
    return L.err;
}

int exact_plan(int mode, bool weighted, int n_frames, int n_pad, int max_lanes, int *lanes,
               size_t *lds_bytes)
{
    const int columns = ((mode == NL_ST_MAD_SIGMA) ||
                         (weighted && (mode == NL_ST_SIGMA || mode == NL_ST_WINSOR_SIGMA || mode == NL_ST_LINEAR_FIT))) ? 2 : 1;
    const size_t n_alloc = (mode == NL_ST_LINEAR_FIT) ? (size_t)n_pad : (size_t)n_frames;
    for (int l = 64; l >= 4; l >>= 1) {
        if (l > max_lanes || l == 8) continue;
        const size_t bytes = (size_t)columns * n_alloc * l * sizeof(float);
        if (bytes <= kLdsBudgetBytes) {
            *lanes = l;
            *lds_bytes = bytes;
            return 0;
        }
    }
    return -1;
}

// every instantiation of the column kernel a pass can ask for: plain, then <follow> (include/nlstack_wclip.h: one column,
// plan with weighted = false), then MAPS (every pixel's two clip counts go to args.reject_map)
struct ExactEntry {
    Form form; int mode; bool weighted; const char *name;
    hipError_t (*launch)(const StackArgs &, int, int, size_t, hipStream_t);
};
static const ExactEntry kExactTable[] = {
    {Form::Plain, NL_ST_MEDIAN, false, "stack_exact_kernel<median>", launch_exact<NL_ST_MEDIAN, false>},
    {Form::Plain, NL_ST_SIGMA, true, "stack_exact_kernel<sigma,weighted>", launch_exact<NL_ST_SIGMA, true>},
    {Form::Plain, NL_ST_SIGMA, false, "stack_exact_kernel<sigma>", launch_exact<NL_ST_SIGMA, false>},
    {Form::Plain, NL_ST_WINSOR_SIGMA, true, "stack_exact_kernel<winsor,weighted>", launch_exact<NL_ST_WINSOR_SIGMA, true>},
    {Form::Plain, NL_ST_WINSOR_SIGMA, false, "stack_exact_kernel<winsor>", launch_exact<NL_ST_WINSOR_SIGMA, false>},
    {Form::Plain, NL_ST_MAD_SIGMA, false, "stack_exact_kernel<mad>", launch_exact<NL_ST_MAD_SIGMA, false>},
    // (the weighted linear-fit pass, include/nlstack_wlinfit.h: never a default pass)
    {Form::Plain, NL_ST_LINEAR_FIT, true, "stack_exact_kernel<linfit,weighted>", launch_exact<NL_ST_LINEAR_FIT, true>},
    {Form::Plain, NL_ST_LINEAR_FIT, false, "stack_exact_kernel<linearfit>", launch_exact<NL_ST_LINEAR_FIT, false>},
    {Form::Follow, NL_ST_SIGMA, false, "stack_exact_kernel<sigma,follow>", launch_exact<NL_ST_SIGMA, false, false, true>},
    {Form::Follow, NL_ST_WINSOR_SIGMA, false, "stack_exact_kernel<winsor,follow>", launch_exact<NL_ST_WINSOR_SIGMA, false, false, true>},
    // (the weighted MAD-sigma pass, include/nlstack_wmad.h: two columns, as the plain MAD kernel)
    {Form::Follow, NL_ST_MAD_SIGMA, false, "stack_exact_kernel<mad,follow>", launch_exact<NL_ST_MAD_SIGMA, false, false, true>},
    {Form::Maps, NL_ST_MEDIAN, false, "stack_exact_kernel<median,maps>", launch_exact<NL_ST_MEDIAN, false, true>},
    {Form::Maps, NL_ST_SIGMA, true, "stack_exact_kernel<sigma,weighted,maps>", launch_exact<NL_ST_SIGMA, true, true>},
    {Form::Maps, NL_ST_SIGMA, false, "stack_exact_kernel<sigma,maps>", launch_exact<NL_ST_SIGMA, false, true>},
    {Form::Maps, NL_ST_WINSOR_SIGMA, true, "stack_exact_kernel<winsor,weighted,maps>", launch_exact<NL_ST_WINSOR_SIGMA, true, true>},
    {Form::Maps, NL_ST_WINSOR_SIGMA, false, "stack_exact_kernel<winsor,maps>", launch_exact<NL_ST_WINSOR_SIGMA, false, true>},
    {Form::Maps, NL_ST_MAD_SIGMA, false, "stack_exact_kernel<mad,maps>", launch_exact<NL_ST_MAD_SIGMA, false, true>},
    {Form::Maps, NL_ST_LINEAR_FIT, false, "stack_exact_kernel<linearfit,maps>", launch_exact<NL_ST_LINEAR_FIT, false, true>},
};

// Form::Maps: every pixel's two clip counts also go to args.reject_map; Form::Follow (sigma / winsorized: one column, plan
// with weighted = false; MAD sigma, the weighted MAD-sigma pass: two columns): the weights come from args.weights
hipError_t launch_stack_exact(int mode, bool weighted, const StackArgs &args, int lanes, int grid,
                              size_t lds_bytes, hipStream_t stream, const char **name, Form form)
{
    // (the median and MAD sigma never weigh, a maps pass drops the linear fit's weights as every unweighted entry does,
    // and the <follow> instantiations are keyed as unweighted)
    if (mode == NL_ST_MEDIAN || mode == NL_ST_MAD_SIGMA || (form == Form::Maps && mode == NL_ST_LINEAR_FIT) || form == Form::Follow)
        weighted = false;
    if (!form_args_ok(form, args) || (mode == NL_ST_LINEAR_FIT && weighted && !args.weights)) return hipErrorInvalidValue;
    for (const ExactEntry &e : kExactTable)
        if (e.form == form && e.mode == mode && e.weighted == weighted) {
            *name = e.name;
            return e.launch(args, lanes, grid, lds_bytes, stream);
        }
    return hipErrorInvalidValue;
}

hipError_t launch_reduce_counters(unsigned long long *partial, int n_blocks,
                                  unsigned long long *counters, hipStream_t stream, const unsigned *list_counts,
                                  bool zero_after)
{
    Launcher L(stream);
    L(reduce_counters_kernel, 1, 256, 0, partial, n_blocks, counters, list_counts, 1, 0, zero_after ? 1 : 0);
    return L.err;
}

}  // namespace nl
