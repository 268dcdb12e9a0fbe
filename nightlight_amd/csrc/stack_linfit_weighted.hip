// stack_linfit_weighted.hip -- the weighted linear-fit pass (include/nlstack_wlinfit.h), register-resident, for gfx950.
// AN EXTENSION: the reference's StackLinearFit takes no weights (stack.go:188-189, :834).
//
// Rejection is the reference's, bit for bit, by the argument of stack_linfit.hip: one sorting network, the rejected
// samples marked dead in a per-pixel bit mask, every sum accumulated sequentially in register order = sorted order with
// the reference's own fp32 operations.  This kernel runs that loop without the chunk classes and the cascade of
// stack_linfit.hip (every position takes the masked code), because it needs something they do not keep: S, the mask the
// LAST regression ran over -- the survivors before the sweep that ends the loop.
//
// The result is the weighted mean, in frame order, of the frames whose sorted position is in S.  The sorted column does
// not know which frame a sample came from, so S is turned into VALUES: its maximal runs of live positions are closed
// intervals [v[first], v[last]], at most kRuns of them, and the frames are read a second time, in frame order (coalesced
// as in the gather); a frame is in if its value lies in one of the intervals.  That is exact unless equal samples sit on
// both sides of a run's end (the definition breaks such ties by frame index, the values cannot): such a pixel, a pixel
// with more than kRuns runs and a pixel with a +-Inf sample (which cannot be told from the pads) go to the hand-over
// list, and the column kernel (stack_exact.hip, <linfit,weighted>) computes them, rejections included.
// One pixel per lane, samples in VGPRs, no LDS.
#include "linfit_common.hpp"
#include "launch_common.hpp"

namespace nl {

constexpr int kWlfRuns = 4;       // runs of survivors a pixel may have (one run covers 70 - 88 % of pixels, four all but a few per cent)

template <int NS>
__global__ __launch_bounds__(256) void stack_linfit_weighted_kernel(StackArgs p, FastArgs q)
{
    constexpr int NW = (NS + 31) / 32;          // liveness words per pixel
    const int lane = threadIdx.x & 63;
    int N = p.n_frames;
    const int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = pix < p.npix;
    const unsigned boff = (unsigned)(on ? pix : 0) * 4u;
    float v[NS];
    const int n = gather_sorted<NS, 32>(p.frames, p.stride, N, boff, v);

    // positions 0 .. n-1 hold the samples; the pads (+Inf) become +0 so that dead positions stay finite, and a
    // genuine +-Inf sample cannot be told from a pad afterwards: column kernel (as stack_linfit.hip)
    unsigned live[NW], real[NW];
    static_range<0, NW>([&](auto W) NL_INL {
        constexpr int w = decltype(W)::value;
        const int c = min(max(n - 32 * w, 0), 32);
        live[w] = c >= 32 ? 0xFFFFFFFFu : ((1u << c) - 1u);
        real[w] = live[w];
    });
    unsigned inf_any = 0;
    {
        int nn = n;
        static_chunks<0, NS, 8>([&](auto K) NL_INL {
            constexpr int k = decltype(K)::value;
            if constexpr ((k & 7) == 0) nn = opaque(nn);
            const unsigned pad = (unsigned)((nn - 1 - k) >> 31);                // all ones for k >= n
            const unsigned bits = (unsigned)__float_as_int(v[k]);
            inf_any |= (((bits & 0x7fffffffu) == 0x7f800000u) ? 1u : 0u) & ~pad;
            v[k] = __int_as_float((int)(bits & ~pad));                       // pads -> +0.0f
        });
    }
    bool to_exact = inf_any != 0;

    int p_lo = 0, p_hi = 0;
    int m = n;                                  // surviving samples
    bool active = on && n > 0 && !to_exact;

    // liveness of position k as an all-ones / zero word, x & m = x or +0: a dead sample adds +0 to a sum, as skipping
    // it does (stack_linfit.hip has the reasons for the integer form)
#define NL_M(k) ((int)(live[(k) >> 5] << (31 - ((k) & 31))) >> 31)
#define NL_AND(x, m) __int_as_float(__float_as_int(x) & (m))
    while (__any(active)) {
        const float fm = (float)m;
        const int mt = (active && m >= 1) ? m : 1;
        const float xm = p.xstat[2 * mt], xsd = p.xstat[2 * mt + 1];
        // ---- MeanStdDev(ys), stats.go:246-261, sequential in sorted order ----
        float s = 0.0f;
        static_range<0, NS>([&](auto K) NL_INL {
            constexpr int k = decltype(K)::value;
            s = __fadd_rn(s, NL_AND(v[k], NL_M(k)));
        });
        const float ym = s / fm;
        // ---- variance of the ys and the correlation sum (stats.go:573-579) in one sweep: each accumulator sees its
        // terms in index order ----
        float vs = 0.0f, corr = 0.0f, fi = 0.0f;
        forget_words<NW>(live);
        static_range<0, NS>([&](auto K) NL_INL {
            constexpr int k = decltype(K)::value;
            const int lm = NL_M(k);
            const float dy = __fsub_rn(v[k], ym);
            const float dd = __fmul_rn(dy, dy);
            vs = __fadd_rn(vs, NL_AND(dd, lm));
            const float dx = __fsub_rn(fi, xm);
            const float t = __fmul_rn(dx, dy);
            corr = __fadd_rn(corr, NL_AND(t, lm));
            fi += NL_AND(1.0f, lm);                              // index among the survivors
        });
        const float ysd = sqrt_go(vs / fm);
        float den = __fmul_rn(xsd, ysd);
        den = __fmul_rn(den, __fadd_rn(fm, 1.0f));
        corr = corr / den;
        float slope = __fmul_rn(corr, ysd);
        slope = slope / xsd;
        float icpt = __fsub_rn(ym, __fmul_rn(slope, xm));
        // ---- mean absolute deviation from the fit, stack.go:879-886 ----
        float sg = 0.0f;
        fi = 0.0f;
        forget_words<NW>(live);
        static_range<0, NS>([&](auto K) NL_INL {
            constexpr int k = decltype(K)::value;
            const int lm = NL_M(k);
            const float lin = __fadd_rn(__fmul_rn(fi, slope), icpt);
            const float diff = __fsub_rn(v[k], lin);
            sg = __fadd_rn(sg, NL_AND(fabsf(diff), lm));
            fi += NL_AND(1.0f, lm);
        });
        sg = sg / fm;
        // ---- reject, stack.go:890-904: lin - g > lb -> low, else g - lin > hb -> high; a NaN fit rejects nothing ----
        float lb = __fmul_rn(p.sig_lo, sg), hb = __fmul_rn(p.sig_hi, sg);
        const bool bad = !(slope == slope) || !(icpt == icpt) || !(lb == lb) || !(hb == hb);
        if (bad) { slope = 0.0f; icpt = 0.0f; lb = __builtin_inff(); hb = __builtin_inff(); }
        unsigned lo_n = 0, hi_n = 0;
        unsigned nlive[NW];
        static_range<0, NW>([&](auto W) NL_INL { nlive[decltype(W)::value] = live[decltype(W)::value]; });
        fi = 0.0f;
        forget_words<NW>(live);
        slope = opaque_f(slope);
        static_range<0, NS>([&](auto K) NL_INL {
            constexpr int k = decltype(K)::value;
            const unsigned alive = (live[k >> 5] >> (k & 31)) & 1u;
            const float lin = __fadd_rn(__fmul_rn(fi, slope), icpt);
            const float t = __fsub_rn(lin, v[k]);                      // fl(g - lin) == -fl(lin - g)
            const unsigned low = sign_bit(__fsub_rn(lb, t)) & alive;   // lb - (lin - g) < 0
            const unsigned high = sign_bit(__fadd_rn(hb, t)) & alive & ~low;
            lo_n += low;
            hi_n += high;
            nlive[k >> 5] &= ~((low | high) << (k & 31));
            fi += NL_AND(1.0f, NL_M(k));
        });
        if (active) {
            p_lo += (int)lo_n;
            p_hi += (int)hi_n;
            const int left = (int)(lo_n + hi_n);
            if (left == 0 || m < 3) {
                active = false;                 // live[] stays: the positions of this, the last regression = S
            } else {
                m -= left;
                static_range<0, NW>([&](auto W) NL_INL { live[decltype(W)::value] = nlive[decltype(W)::value]; });
            }
        }
    }
#undef NL_AND

    // ---- S as value intervals: its maximal runs of live positions, [v[first], v[last]] each ----
    float r_lo[kWlfRuns], r_hi[kWlfRuns];
    static_range<0, kWlfRuns>([&](auto R) NL_INL {
        r_lo[decltype(R)::value] = __builtin_inff();             // an empty interval holds no value
        r_hi[decltype(R)::value] = -__builtin_inff();
    });
    int runs = 0;
    bool split = false;
    static_range<0, NS>([&](auto K) NL_INL {
        constexpr int k = decltype(K)::value;
        const bool here = NL_M(k) != 0;
        bool before = false, after = false, real_after = false;
        if constexpr (k > 0) before = NL_M(k - 1) != 0;
        if constexpr (k + 1 < NS) {
            after = NL_M(k + 1) != 0;
            real_after = ((real[(k + 1) >> 5] >> ((k + 1) & 31)) & 1u) != 0;
        }
        const bool first = here && !before, last = here && !after;
        // a group of equal samples on both sides of the run's end: the values cannot say which frames survived
        if constexpr (k > 0) split = split || (first && v[k - 1] == v[k]);
        if constexpr (k + 1 < NS) split = split || (last && real_after && v[k + 1] == v[k]);
        static_range<0, kWlfRuns>([&](auto R) NL_INL {
            constexpr int r = decltype(R)::value;
            r_lo[r] = (first && runs == r) ? v[k] : r_lo[r];
            r_hi[r] = (last && runs == r) ? v[k] : r_hi[r];
        });
        runs += last ? 1 : 0;
    });
#undef NL_M
    to_exact = to_exact || runs > kWlfRuns || split;

    // ---- the frames again, in frame order: StackMeanWeighted's sums (stack.go:343-364) over the frames in S ----
    float num = 0.0f, wsum = 0.0f;
    const float *fr = p.frames + (on ? pix : 0);
    auto take = [&](float x, float w) NL_INL {
        bool in = false;
        static_range<0, kWlfRuns>([&](auto R) NL_INL {
            constexpr int r = decltype(R)::value;
            in = in || (x >= r_lo[r] && x <= r_hi[r]);          // (NaN: in no interval, as the gather drops it)
        });
        if (in) {
            num = __fadd_rn(num, __fmul_rn(x, w));
            wsum = __fadd_rn(wsum, w);
        }
    };
    int k = 0;
    for (; k + 8 <= N; k += 8) {
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; u++) x[u] = fr[(int64_t)(k + u) * p.stride];
#pragma unroll
        for (int u = 0; u < 8; u++) take(x[u], p.weights[k + u]);
    }
    for (; k < N; k++) take(fr[(int64_t)k * p.stride], p.weights[k]);
    const float res = n > 0 ? num / wsum : p.ref_loc;          // stack.go:388-397: no valid sample -> RefFrameLoc

    // a pixel of the hand-over list is the column kernel's: it stores the result and counts the rejections
    int c_lo = 0, c_hi = 0;
    if (on && !to_exact) {
        NL_STORE_RESULT(&p.out[pix], res);
        c_lo = p_lo;
        c_hi = p_hi;
    }
    wave_append(q.fb_list, q.fb_count, q.fb_capacity, on && to_exact, (unsigned)pix, lane);

    __shared__ int s_lo[4], s_hi[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        c_lo += __shfl_xor(c_lo, o, 64);
        c_hi += __shfl_xor(c_hi, o, 64);
    }
    if (lane == 0) { s_lo[threadIdx.x >> 6] = c_lo; s_hi[threadIdx.x >> 6] = c_hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int t_lo = s_lo[0] + s_lo[1] + s_lo[2] + s_lo[3];      // (four waves: the launcher starts 256 threads)
        const int t_hi = s_hi[0] + s_hi[1] + s_hi[2] + s_hi[3];
        add_clip_totals(partial_slot(p, blockIdx.x), t_lo, t_hi);
    }
}

int linfit_weighted_supported(int n_frames, int64_t npix)
{
    return (n_frames >= 1 && n_frames <= 128 && npix < kFastMaxPixels) ? 1 : 0;
}

constexpr char kLinfitWeightedName[] = "stack_linfit_weighted_kernel";

hipError_t launch_stack_linfit_weighted(const StackArgs &args, const FastArgs &fargs, hipStream_t stream, const char **name)
{
    if (!args.weights || !fargs.fb_list || !fargs.fb_count || !linfit_weighted_supported(args.n_frames, args.npix))
        return hipErrorInvalidValue;
    Launcher L(stream);
    with_class<8, 16, 32, 48, 64, 96, 128>(args.n_frames, [&](auto C) {
        constexpr int NS = decltype(C)::value;
        *name = kernel_name<kLinfitWeightedName, NS>();
        L(stack_linfit_weighted_kernel<NS>, pixel_grid(args.npix), 256, 0, args, fargs);
    });
    return L.err;
}

}  // namespace nl
