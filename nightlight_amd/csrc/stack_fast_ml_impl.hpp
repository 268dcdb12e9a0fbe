// stack_fast_ml_impl.hpp -- the median and MAD-sigma kernels with LPP adjacent lanes per pixel, 128 samples per lane
// (fast_ml_common.hpp).  Two units instantiate them: stack_fast_ml.hip with 2 and 4 lanes (129 ... 512 frames, the
// default pass) and stack_fast_ml_deep.hip with 8 and 16 (513 ... 2048 frames, include/nlstack_deepstack.h).
#pragma once
#include "fast_ml_common.hpp"
#include "wave_lists.hpp"

namespace nl {

// 8 and 16 lanes per pixel: the thread's wave in its workgroup, kept in a scalar register, and from it the thread's role,
// pixel and `on` computed anew (fresh_lane, fast_ml_common.hpp) wherever the kernel comes back to them behind a sort --
// held in vector registers across it they are spilled.  2 and 4 lanes keep theirs from the top of the kernel.
// What cannot be computed anew -- the pixel's sample count, its median -- waits in LDS, one word per thread (park / parked).
struct DeepThread {
    int wave;
    __device__ __forceinline__ DeepThread() : wave(__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) {}
    __device__ __forceinline__ int tid() const { return (wave << 6) | fresh_lane(); }
    template <int LPP>
    __device__ __forceinline__ void renew(int &role, int64_t &pix, bool &on, int64_t npix) const
    {
        const int t = tid();
        role = t % LPP;
        pix = (int64_t)blockIdx.x * (blockDim.x / LPP) + t / LPP;
        on = pix < npix;
    }
    template <class T>
    __device__ __forceinline__ void park(T *slots, T x) const { slots[tid()] = x; }
    template <class T>
    __device__ __forceinline__ T parked(const T *slots) const { return slots[tid()]; }
};

// StackMedian (stack.go:274-303) for 129..512 frames (2 / 4 lanes) and 513..2048 (8 / 16): the merged column gives the
// median exactly (order independent); both middle ranks are looked up over whole lanes, so any
// number of missing samples is fine and nothing is handed over.
template <int LPP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 8)))
void stack_median_ml_kernel(StackArgs p)
{
    constexpr int NS = kMlNS;
    int role = threadIdx.x % LPP;
    int64_t item = (int64_t)blockIdx.x * (blockDim.x / LPP) + threadIdx.x / LPP;
    bool on = item < p.npix;
    const DeepThread me;
    int N = p.n_frames;
    asm volatile("" : "+s"(N));
    float v[NS];
    int n;
    if constexpr (LPP >= 8) {
        __shared__ int s_n[256];
        me.park(s_n, ml_gather_raw<LPP, NS>(p.frames, p.stride, N, on, item, role, v));
        ml_sort_merge<LPP, NS, false>(v, role);
        n = me.parked(s_n);
        me.template renew<LPP>(role, item, on, p.npix);
    } else {
        n = ml_gather_sorted<LPP, NS, false, 16, 32, NS, NS / 2, NS, LPP == 2>(p.frames, p.stride, N, on, item, role, v);      // (nt loads at two lanes per pixel: fast_ml_common.hpp)
    }
    const int kk = n >> 1;
    const float upper = pick_rank<LPP, NS, NS, NS>(v, kk, role, 0);
    const float lower = pick_rank<LPP, NS, NS, NS>(v, kk > 0 ? kk - 1 : 0, role, 0);
    float res = (n & 1) ? upper : 0.5f * (lower + upper);          // qsort.go:73-81
    if (n == 0) res = p.ref_loc;
    if (on && role == 0) NL_STORE_RESULT(&p.out[item], res);
}

// StackMADSigma (stack.go:536-605) for 129..512 frames (513..2048 on 8 / 16 lanes), as stack_mad_fast_kernel: merged
// column -> median; column := |x - median| -> bitonic merge -> MAD; second read of the
// pixel's frames (every lane its own) for the clip counts and the mean of the survivors.
// RECORD (the weighted MAD-sigma pass, include/nlstack_wmad.h): the kernel stops behind the bounds and leaves the pixel's
// one round, p.bounds[pix] = (lo, hi) with p.nrounds[pix] = 1 -- or 0 for a pixel without a finite median or without a
// sample -- for stack_clip_weighted_kernel<PX, true>: no second read, no result, no list, no counters.  (The lanes of a
// pixel interleave the frames in the second read; a frame-order fp32 sum would be a chain through them per frame.)
// MAPS (the full maps pass, include/nlstack_fullmaps.h): the lane that stores a pixel's result also stores its two clip
// counts, p.reject_map[pix] = c_lo | c_hi << 16 (zero beside ref_loc; nothing for a pixel of the exact list).
// Both forms exist at every lane count: 8 and 16 lanes serve include/nlstack_deepwmad.h (RECORD) and
// include/nlstack_deepstackmaps.h (MAPS), and take pixel, role and `on` anew behind the sorts as the plain form does.
template <int LPP, bool RECORD = false, bool MAPS = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 8)))
void stack_mad_ml_kernel(StackArgs p, FastArgs q)
{
    static_assert(!(RECORD && MAPS), "the record-only kernel stores no result and no map");
    constexpr int NS = kMlNS;
    int lane = threadIdx.x & 63;
    int role = threadIdx.x % LPP;
    int64_t pix = (int64_t)blockIdx.x * (blockDim.x / LPP) + threadIdx.x / LPP;
    bool on = pix < p.npix;
    const DeepThread me;
    int N = p.n_frames;
    asm volatile("" : "+s"(N));
    float v[NS];
    __shared__ int s_n[LPP >= 8 ? 256 : 1];
    __shared__ float s_median[LPP >= 8 ? 256 : 1];
    int n;
    if constexpr (LPP >= 8) {
        me.park(s_n, ml_gather_raw<LPP, NS>(p.frames, p.stride, N, on, pix, role, v));
        ml_sort_merge<LPP, NS, false>(v, role);
        n = me.parked(s_n);
        role = fresh_role<LPP>();
    } else {
        n = ml_gather_sorted<LPP, NS, false>(p.frames, p.stride, N, on, pix, role, v);
    }
    int kk = n >> 1;
    const float upper = pick_rank<LPP, NS, NS, NS>(v, kk, role, 0);
    const float lower = pick_rank<LPP, NS, NS, NS>(v, kk > 0 ? kk - 1 : 0, role, 0);
    float median = (n & 1) ? upper : 0.5f * (lower + upper);
    bool degenerate = n > 0 && !(__builtin_fabsf(median) < __builtin_inff());
    const float msafe = degenerate ? 0.0f : median;
    if constexpr (LPP >= 8) me.park(s_median, median);
    static_chunks<0, NS, 16>([&](auto K) NL_INL {
        constexpr int k = decltype(K)::value;
        v[k] = __builtin_fabsf(v[k] - msafe);
    });
    // The deviations of the sorted column (lane r: ranks [128 r, 128 r + 128)) fall to the median and rise
    // again, +Inf pads on top: ONE bitonic sequence over the lanes of the pixel.  The half-cleaner cascade
    // of a bitonic merge sorts it -- lane distance 2 and 1 (element i meets the partner's element i), then
    // the in-lane cascade -- without the 2 184-operation sort of every lane and the run merges.
    // (8 / 16 lanes per pixel: lane distances 4 / 8 and 4 in front)
    if constexpr (LPP >= 8) role = fresh_role<LPP>();
    if constexpr (LPP == 16) cross_stage<NS, kSwap8, false>(v, (role & 8) == 0);
    if constexpr (LPP >= 8) {
        cross_stage<NS, kSwap4, false>(v, (role & 4) == 0);
        cross_stage<NS, kSwap2, false>(v, (role & 2) == 0);
    }
    if constexpr (LPP == 4) cross_stage<NS, kSwap2, false>(v, role < 2);
    cross_stage<NS, kSwap1, false>(v, (role & 1) == 0);
    run_network<FusedBitonic<NS, 0>, NS>(v);
    if constexpr (LPP >= 8) {
        role = fresh_role<LPP>();
        n = me.parked(s_n);
        kk = n >> 1;
    }
    const float dupper = pick_rank<LPP, NS, NS, NS>(v, kk, role, 0);
    const float dlower = pick_rank<LPP, NS, NS, NS>(v, kk > 0 ? kk - 1 : 0, role, 0);
    const float mad = (n & 1) ? dupper : 0.5f * (dlower + dupper);
    const float sd = mad * 1.4826f;
    if constexpr (LPP >= 8) {
        median = me.parked(s_median);
        degenerate = n > 0 && !(__builtin_fabsf(median) < __builtin_inff());
    }
    const float t_lo = p.sig_lo * sd, t_hi = p.sig_hi * sd;
    const float lo = median - t_lo, hi = median + t_hi;
    if constexpr (RECORD) {
        if constexpr (LPP >= 8) me.template renew<LPP>(role, pix, on, p.npix);
        if (on && role == 0) {
            p.bounds[(size_t)pix] = make_float2(lo, hi);
            p.nrounds[(size_t)pix] = (n > 0 && !degenerate) ? 1 : 0;
        }
        return;
    }

    // second read: lane role r takes frames r, r+LPP, ... again (clipped descriptors as in the gather)
    int N2 = p.n_frames;
    asm volatile("" : "+s"(N2));
    int frame_bytes = (int)(p.stride * (int64_t)sizeof(float));
    asm volatile("" : "+s"(frame_bytes));
    if constexpr (LPP >= 8) { me.template renew<LPP>(role, pix, on, p.npix); lane = fresh_lane(); }
    const int voff = (int)((unsigned)(on ? pix : 0) * 4u) + role * frame_bytes;
    static_chunks<0, NS, 4>([&](auto K) NL_INL {
        constexpr int k = decltype(K)::value;
        const int avail = min(max(N2 - k * LPP, 0), LPP);
        const char *gb = reinterpret_cast<const char *>(p.frames) + (int64_t)(k * LPP) * frame_bytes;
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(gb), 0, avail * frame_bytes, 0x00020000);
        v[k] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff, 0, 0));
    });
    float f_lo = 0.0f, f_hi = 0.0f, f_kept = 0.0f, sum = 0.0f;
    static_chunks<0, NS, 4>([&](auto K) NL_INL {
        constexpr int k = decltype(K)::value;
        const float x = v[k];
        const bool present = (k * LPP + role < N2) && (x == x);
        const bool below = present && x < lo;
        const bool above = present && !below && x > hi;
        const bool keep = present && !below && !above;
        f_lo += below ? 1.0f : 0.0f;
        f_hi += above ? 1.0f : 0.0f;
        f_kept += keep ? 1.0f : 0.0f;
        sum += keep ? x : 0.0f;
        asm volatile("" : "+v"(f_lo), "+v"(f_hi), "+v"(f_kept), "+v"(sum));
    });
    int c_lo = (int)quad_sum<LPP>(f_lo), c_hi = (int)quad_sum<LPP>(f_hi);
    float res = quad_sum<LPP>(sum) / quad_sum<LPP>(f_kept);
    if (n == 0) res = p.ref_loc;
    const bool rep = on && role == 0;
    const bool to_exact = rep && degenerate;
    if (rep && !to_exact) NL_STORE_RESULT(&p.out[pix], res);
    if (!rep || to_exact || n == 0) { c_lo = 0; c_hi = 0; }
    if constexpr (MAPS) {
        if (rep && !to_exact) p.reject_map[pix] = (unsigned)c_lo | ((unsigned)c_hi << 16);
    }
    wave_append(q.fb_list, q.fb_count, q.fb_capacity, to_exact, (unsigned)pix, lane);
    __shared__ int s_lo[4], s_hi[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        c_lo += __shfl_xor(c_lo, o, 64);
        c_hi += __shfl_xor(c_hi, o, 64);
    }
    const int wave = LPP >= 8 ? me.wave : (int)(threadIdx.x >> 6);
    if (lane == 0) { s_lo[wave] = c_lo; s_hi[wave] = c_hi; }
    __syncthreads();
    if (wave == 0 && lane == 0) {
        const int t_l = s_lo[0] + s_lo[1] + s_lo[2] + s_lo[3];      // (four waves: the launcher starts 256 threads)
        const int t_h = s_hi[0] + s_hi[1] + s_hi[2] + s_hi[3];
        add_clip_totals(partial_slot(p, blockIdx.x), t_l, t_h);
    }
}

constexpr char kMedianMlName[] = "stack_median_ml_kernel";
constexpr char kMadMlName[] = "stack_mad_ml_kernel";

}  // namespace nl
