// stack_clip_weighted.hip -- weighted sigma / winsorized clipping whose weights follow their frames
// (include/nlstack_wclip.h), the streaming engine, for gfx950.  AN EXTENSION: the reference multiplies a survivor by
// whichever weight Hoare's permutation left in its slot (stack.go:487).
//
// The rejection of the weighted modes ignores the weights, and the decision pass of the weighted stacks
// (stack_sigma_fast_kernel<..., RECORD>, the record-only LDS-column kernels) has already left, per pixel and clipping
// round, thresholds (lo, hi) that reproduce the reference's decisions on every surviving sample.  A sample's fate
// depends on its own value and those thresholds alone, so no permutation has to be replayed: this kernel reads the
// frames once, in frame order, tests each sample against its pixel's rounds and accumulates v * w and w
// (wclip_take, wclip_common.hpp -- the column kernel's <follow> instantiations call the same function).
//
// Shape of stack_mean.hip: each lane owns 4 consecutive pixels (16-byte loads) where stride and pointers allow it, 8
// frames of loads in flight, no LDS in the frame loop; HBM-bound at 4 * (N + 1) bytes per pixel plus 1 + 8 * rounds bytes
// of record.
//
// Rounds.  A pixel's rounds are walked IN ORDER (R = kBoundRounds - 1 rounds in front of the last one).  Where it provably
// gives the same members and the same two counts the rounds in front of the last one are folded into one,
// [max lo_r, min hi_r] (R = 1: the fold, then the last round): that holds when max lo_r <= min hi_r -- then no sample is below one round's lo and above another's hi,
// so the side on which a sample leaves does not depend on the order -- and not when a recorded round has lo_r > hi_r; a
// NaN threshold rejects nothing in either form.  The wave takes the folded form when all its pixels may.
//
// Hand-over.  A record is complete when the reference's loop ends behind its last round (stack.go:427: that sweep
// removed nothing, or left at most one sample).  The register-resident decision kernels record complete pixels or none
// (nrounds == 0); the LDS-column ones also leave the decided FRONT of a pixel they could not finish, so the test is made
// here, on the data.  A pixel with no round on record, without samples, or with an incomplete record is appended to the
// exact list; nothing is stored or counted for it.
#include "launch_common.hpp"
#include "wave_lists.hpp"
#include "wclip_common.hpp"

namespace nl {

// (R = 0: no front rounds, `front` is not read)
template <int PX, int R>
__device__ __forceinline__ void wclip_frames(const StackArgs &p, int64_t pix0, const float2 (&front)[PX][R > 0 ? R : 1],
                                             const float2 (&last)[PX], WclipAcc (&acc)[PX])
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    const float *fr = p.frames + pix0;
    const int N = p.n_frames;
    auto load = [&](int k, float (&x)[PX]) {
        if constexpr (PX == 4) {
            const f4 t = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(fr + (int64_t)k * p.stride));
            x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
        } else {
            x[0] = fr[(int64_t)k * p.stride];
        }
    };
    int k = 0;
    for (; k + 8 <= N; k += 8) {
        float x[8][PX];
#pragma unroll
        for (int u = 0; u < 8; u++) load(k + u, x[u]);
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const float w = p.weights[k + u];
#pragma unroll
            for (int j = 0; j < PX; j++) wclip_take<R>(x[u][j], w, front[j], last[j], acc[j]);
        }
    }
    for (; k < N; k++) {
        float x[PX];
        load(k, x);
        const float w = p.weights[k];
#pragma unroll
        for (int j = 0; j < PX; j++) wclip_take<R>(x[j], w, front[j], last[j], acc[j]);
    }
}

// PX pixels per lane: 4 (aligned tiles, first = 0) or 1 (the pixels from `first` on: tails, unaligned tiles)
// ONE: the weighted MAD-sigma pass (include/nlstack_wmad.h) -- its rejection has no loop, the record-only
// stack_mad_ml_kernel leaves the pixel's one round (lo, hi) with nrounds = 1, or 0 for a pixel without a finite median or
// without a sample, and one recorded round IS a complete record: no front rounds, no completeness test.
template <int PX, bool ONE = false>
__global__ __launch_bounds__(256) void stack_clip_weighted_kernel(StackArgs p, FastArgs q, int64_t first)
{
    static_assert(PX == 1 || PX == 4, "one pixel or one 16-byte load per lane");
    const int lane = threadIdx.x & 63;
    const int64_t items = (p.npix - first) / PX;
    int c_lo = 0, c_hi = 0;
    // (every lane of a workgroup makes the same trips: the ballots below want whole waves)
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < items; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t item = base + threadIdx.x;
        const bool on = item < items;
        const int64_t pix0 = first + (on ? item : 0) * PX;

        // ---- the record: rounds per pixel, thresholds per round ----
        int nr[PX];
        if constexpr (PX == 4) {
            const unsigned w = *reinterpret_cast<const unsigned *>(p.nrounds + pix0);
#pragma unroll
            for (int j = 0; j < 4; j++) nr[j] = min((int)((w >> (8 * j)) & 0xffu), kBoundRounds);
        } else {
            nr[0] = min((int)p.nrounds[pix0], kBoundRounds);
        }
        // front: the rounds before the last one, in order (a round that rejects nothing where the pixel has fewer);
        // fold: all of them as one; last: the round behind which the record ends
        float2 front[PX][kBoundRounds - 1], fold[PX][1], last[PX];
        bool may_fold = true;
        if constexpr (ONE) {
#pragma unroll
            for (int j = 0; j < PX; j++) last[j] = nr[j] > 0 ? p.bounds[(size_t)(pix0 + j)] : wclip_no_round();
        } else {
#pragma unroll
            for (int j = 0; j < PX; j++) {
                float lo = -__builtin_inff(), hi = __builtin_inff();
                last[j] = wclip_no_round();
#pragma unroll
                for (int r = 0; r < kBoundRounds; r++) {
                    const float2 b = r < nr[j] ? p.bounds[(size_t)r * (size_t)p.npix + (size_t)(pix0 + j)] : wclip_no_round();
                    const bool in_front = r < nr[j] - 1;
                    if (r < kBoundRounds - 1) front[j][r] = in_front ? b : wclip_no_round();
                    lo = (in_front && b.x > lo) ? b.x : lo;
                    hi = (in_front && b.y < hi) ? b.y : hi;
                    last[j] = (r == nr[j] - 1) ? b : last[j];
                }
                fold[j][0] = make_float2(lo, hi);
                may_fold = may_fold && lo <= hi;
            }
        }

        // ---- one read of the frames in frame order ----
        WclipAcc acc[PX];
        if constexpr (ONE)        wclip_frames<PX, 0>(p, pix0, fold, last, acc);
        else if (__all(may_fold)) wclip_frames<PX, 1>(p, pix0, fold, last, acc);
        else                      wclip_frames<PX, kBoundRounds - 1>(p, pix0, front, last, acc);

        // ---- results, counts, hand-over ----
        float res[PX];
        bool done[PX];
        bool all_done = true;
#pragma unroll
        for (int j = 0; j < PX; j++) {
            const int n = acc[j].kept + acc[j].lo + acc[j].hi;
            // the reference's loop ends behind the last round on record (stack.go:427)
            done[j] = nr[j] > 0 && n > 0 && (ONE || acc[j].last == 0 || acc[j].kept <= 1);
            res[j] = acc[j].num / acc[j].den;
            all_done = all_done && done[j];
            if (on && done[j]) {
                c_lo += acc[j].lo;
                c_hi += acc[j].hi;
            }
        }
        if constexpr (PX == 4) {
            if (on && all_done) {
                typedef float f4 __attribute__((ext_vector_type(4)));
                const f4 rv = {res[0], res[1], res[2], res[3]};
                NL_STORE_RESULT(reinterpret_cast<f4 *>(p.out + pix0), rv);
            }
        }
#pragma unroll
        for (int j = 0; j < PX; j++) {
            if (on && done[j] && (PX == 1 || !all_done)) NL_STORE_RESULT(&p.out[pix0 + j], res[j]);
            const bool to_exact = on && !done[j];
            const unsigned long long em = __ballot(to_exact);
            if (em) {
                unsigned at = 0;
                if (lane == 0) at = atomicAdd(q.fb_count, (unsigned)__popcll(em));
                at = __shfl(at, 0, 64);
                const unsigned slot = at + lane_rank(em, lane);
                if (to_exact && slot < q.fb_capacity) q.fb_list[slot] = (unsigned)(pix0 + j);
            }
        }
    }

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

static int wclip_grid(int64_t items)
{
    const int64_t g = (items + 255) / 256;
    return (int)(g > 256 * 64 ? 256 * 64 : (g < 1 ? 1 : g));
}

constexpr char kClipWeightedName[] = "stack_clip_weighted_kernel";

// one_round: the ONE instantiations (the weighted MAD-sigma pass)
hipError_t launch_stack_clip_weighted(const StackArgs &args, const FastArgs &fargs, hipStream_t stream, const char **name, bool one_round)
{
    // (the exact list holds 32-bit pixel indices)
    if (!args.weights || !args.bounds || !args.nrounds || !fargs.fb_list || !fargs.fb_count || args.npix < 1 ||
        args.npix >= kFastMaxPixels || fargs.fb_capacity < (unsigned)args.npix)
        return hipErrorInvalidValue;
    const bool vec_ok = (args.stride % 4 == 0) && ((reinterpret_cast<uintptr_t>(args.frames) & 15) == 0) &&
                        ((reinterpret_cast<uintptr_t>(args.out) & 15) == 0) && ((reinterpret_cast<uintptr_t>(args.nrounds) & 3) == 0);
    Launcher L(stream);
    with_bool(one_round, [&](auto O) {
        constexpr bool ONE = decltype(O)::value;
        // (the default instantiations keep the names they had before the second parameter)
        auto named = [](auto PX) { if constexpr (ONE) return kernel_name<kClipWeightedName, decltype(PX)::value, true>();
                                   else               return kernel_name<kClipWeightedName, decltype(PX)::value>(); };
        int64_t done = 0;
        *name = named(std::integral_constant<int, 1>{});
        if (vec_ok && args.npix >= 4) {
            *name = named(std::integral_constant<int, 4>{});
            const int64_t quads = args.npix >> 2;
            L(stack_clip_weighted_kernel<4, ONE>, wclip_grid(quads), 256, 0, args, fargs, (int64_t)0);
            if (L.err != hipSuccess) return;
            done = quads << 2;
        }
        if (done < args.npix) L(stack_clip_weighted_kernel<1, ONE>, wclip_grid(args.npix - done), 256, 0, args, fargs, done);
    });
    return L.err;
}

}  // namespace nl
