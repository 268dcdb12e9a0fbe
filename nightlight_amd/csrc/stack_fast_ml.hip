// stack_fast_ml.hip -- register-resident sigma clipping for 129..512 frames:
// LPP = 2 or 4 ADJACENT lanes share one pixel, each lane keeps 128 samples in
// VGPRs (so the register footprint equals the 128-frame kernel's).
//
//   * lane role r loads frames r, r+LPP, r+2*LPP, ... of the pixel;
//   * each lane sorts its 128 values with the odd-even merge network;
//   * the 2 (4) sorted runs are merged across lanes with bitonic merge stages:
//     the cross-lane compare-exchanges read the partner's register through a
//     DPP quad permute (no LDS), the remaining stages are in-lane;
//     afterwards lane r holds the pixel's sorted ranks [128 r, 128 r + 128);
//   * everything after the sort is the algorithm of stack_fast.hip (exact
//     median by rank lookup, shifted moments, rigorous bracket of the
//     reference's stddev, clip decisions accepted only when unambiguous, exact
//     kernel for the rest -- see that file and DESIGN.md section 5); sums,
//     counts and lookups are combined over the quad with DPP adds / ors, which
//     are commutative, so all lanes of a pixel hold bit-identical values and
//     take the same branches.
//
// StackSigma: internal/ops/stack/stack.go:372-436.  HBM traffic: every sample is
// read once; a wave instruction covers 64/LPP consecutive pixels of LPP frames.
#include <cstdlib>
#include <cstring>

#include "fast_ml_common.hpp"
#include "launch_common.hpp"

namespace nl {

#ifdef NL_ROUND_STATS
__device__ unsigned long long nl_dbg_rounds_ml[8];           // as nl_dbg_rounds in stack_fast.hip
extern "C" int nl_debug_round_stats_ml(unsigned long long *out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(nl_dbg_rounds_ml), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[8] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(nl_dbg_rounds_ml), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#define NL_STAT(i, x) atomicAdd(&nl_dbg_rounds_ml[i], (unsigned long long)(x))
#else
#define NL_STAT(i, x) ((void)0)
#endif

// StackMedian (stack.go:274-303) for 129..512 frames: the merged column gives the median
// exactly (order independent); both middle ranks are looked up over whole lanes, so any
// number of missing samples is fine and nothing is handed over.
template <int LPP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 8)))
void stack_median_ml_kernel(StackArgs p)
{
    constexpr int NS = kMlNS;
    const int role = threadIdx.x % LPP;
    const int64_t item = (int64_t)blockIdx.x * (blockDim.x / LPP) + threadIdx.x / LPP;
    const bool on = item < p.npix;
    int N = p.n_frames;
    asm volatile("" : "+s"(N));
    float v[NS];
    const int n = ml_gather_sorted<LPP, NS, false, 16, 32, NS, NS / 2, NS, LPP == 2>(p.frames, p.stride, N, on, item, role, v);      // (nt loads at two lanes per pixel: fast_ml_common.hpp)
    const int kk = n >> 1;
    const float upper = pick_rank<LPP, NS, NS, NS>(v, kk, role, 0);
    const float lower = pick_rank<LPP, NS, NS, NS>(v, kk > 0 ? kk - 1 : 0, role, 0);
    float res = (n & 1) ? upper : 0.5f * (lower + upper);          // qsort.go:73-81
    if (n == 0) res = p.ref_loc;
    if (on && role == 0) NL_STORE_RESULT(&p.out[item], res);
}

constexpr char kMedianMlName[] = "stack_median_ml_kernel";
constexpr char kMadMlName[] = "stack_mad_ml_kernel";

hipError_t launch_stack_median_ml(const StackArgs &args, hipStream_t stream, const char **name)
{
    Launcher L(stream);
    with_ml_lanes(args.n_frames, [&](auto LPP) {
        *name = kernel_name<kMedianMlName, decltype(LPP)::value>();
        L(stack_median_ml_kernel<decltype(LPP)::value>, pixel_grid(args.npix, LPP), 256, 0, args);
    });
    return L.err;
}

// StackMADSigma (stack.go:536-605) for 129..512 frames, as stack_mad_fast_kernel: merged
// column -> median; column := |x - median| -> bitonic merge -> MAD; second read of the
// pixel's frames (every lane its own) for the clip counts and the mean of the survivors.
// RECORD (the weighted MAD-sigma pass, include/nlstack_wmad.h): the kernel stops behind the bounds and leaves the pixel's
// one round, p.bounds[pix] = (lo, hi) with p.nrounds[pix] = 1 -- or 0 for a pixel without a finite median or without a
// sample -- for stack_clip_weighted_kernel<PX, true>: no second read, no result, no list, no counters.  (The lanes of a
// pixel interleave the frames in the second read; a frame-order fp32 sum would be a chain through them per frame.)
// MAPS (the full maps pass, include/nlstack_fullmaps.h): the lane that stores a pixel's result also stores its two clip
// counts, p.reject_map[pix] = c_lo | c_hi << 16 (zero beside ref_loc; nothing for a pixel of the exact list).
template <int LPP, bool RECORD = false, bool MAPS = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 8)))
void stack_mad_ml_kernel(StackArgs p, FastArgs q)
{
    static_assert(!(RECORD && MAPS), "the record-only kernel stores no result and no map");
    constexpr int NS = kMlNS;
    const int lane = threadIdx.x & 63;
    const int role = threadIdx.x % LPP;
    const int64_t pix = (int64_t)blockIdx.x * (blockDim.x / LPP) + threadIdx.x / LPP;
    const bool on = pix < p.npix;
    int N = p.n_frames;
    asm volatile("" : "+s"(N));
    float v[NS];
    const int n = ml_gather_sorted<LPP, NS, false>(p.frames, p.stride, N, on, pix, role, v);
    const int kk = n >> 1;
    const float upper = pick_rank<LPP, NS, NS, NS>(v, kk, role, 0);
    const float lower = pick_rank<LPP, NS, NS, NS>(v, kk > 0 ? kk - 1 : 0, role, 0);
    const float median = (n & 1) ? upper : 0.5f * (lower + upper);
    const bool degenerate = n > 0 && !(__builtin_fabsf(median) < __builtin_inff());
    const float msafe = degenerate ? 0.0f : median;
    static_chunks<0, NS, 16>([&](auto K) NL_INL {
        constexpr int k = decltype(K)::value;
        v[k] = __builtin_fabsf(v[k] - msafe);
    });
    // The deviations of the sorted column (lane r: ranks [128 r, 128 r + 128)) fall to the median and rise
    // again, +Inf pads on top: ONE bitonic sequence over the lanes of the pixel.  The half-cleaner cascade
    // of a bitonic merge sorts it -- lane distance 2 and 1 (element i meets the partner's element i), then
    // the in-lane cascade -- without the 2 184-operation sort of every lane and the run merges.
    if constexpr (LPP == 4) cross_stage<NS, kSwap2, false>(v, role < 2);
    cross_stage<NS, kSwap1, false>(v, (role & 1) == 0);
    run_network<FusedBitonic<NS, 0>, NS>(v);
    const float dupper = pick_rank<LPP, NS, NS, NS>(v, kk, role, 0);
    const float dlower = pick_rank<LPP, NS, NS, NS>(v, kk > 0 ? kk - 1 : 0, role, 0);
    const float mad = (n & 1) ? dupper : 0.5f * (dlower + dupper);
    const float sd = mad * 1.4826f;
    const float t_lo = p.sig_lo * sd, t_hi = p.sig_hi * sd;
    const float lo = median - t_lo, hi = median + t_hi;
    if constexpr (RECORD) {
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
    if (lane == 0) { s_lo[threadIdx.x >> 6] = c_lo; s_hi[threadIdx.x >> 6] = c_hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int t_l = s_lo[0] + s_lo[1] + s_lo[2] + s_lo[3];      // (four waves: the launcher starts 256 threads)
        const int t_h = s_hi[0] + s_hi[1] + s_hi[2] + s_hi[3];
        add_clip_totals(partial_slot(p, blockIdx.x), t_l, t_h);
    }
}

// Form::Maps: the full maps pass, named as the default pass's kernel with "maps" as its last argument.  Form::Record: the
// weighted MAD-sigma pass; the kernel writes no list, so it gets an all-zero FastArgs and `fargs` is not read
hipError_t launch_stack_mad_ml(const StackArgs &args, const FastArgs &fargs, hipStream_t stream, const char **name, Form form)
{
    if (form == Form::Follow || !form_args_ok(form, args)) return hipErrorInvalidValue;
    Launcher L(stream);
    with_ml_lanes(args.n_frames, [&](auto LPP) {
        if (form == Form::Maps) {
            *name = maps_kernel_name<kMadMlName, decltype(LPP)::value>();
            L(stack_mad_ml_kernel<decltype(LPP)::value, false, true>, pixel_grid(args.npix, LPP), 256, 0, args, fargs);
        } else if (form == Form::Record) {
            FastArgs none;
            memset(&none, 0, sizeof none);
            *name = kernel_name<kMadMlName, decltype(LPP)::value, true>();
            L(stack_mad_ml_kernel<decltype(LPP)::value, true>, pixel_grid(args.npix, LPP), 256, 0, args, none);
        } else {
            *name = kernel_name<kMadMlName, decltype(LPP)::value>();
            L(stack_mad_ml_kernel<decltype(LPP)::value>, pixel_grid(args.npix, LPP), 256, 0, args, fargs);
        }
    });
    return L.err;
}

int fast_ml_supported(int mode, bool weighted, int n_frames, int64_t npix)
{
    // 4 frames of the tile must be addressable with a 31-bit buffer offset
    if (n_frames <= 128 || n_frames > 512 || npix >= kFastMaxPixels) return 0;
    if (mode == NL_ST_MEDIAN) return 1;
    if (mode == NL_ST_MAD_SIGMA) return weighted ? 0 : 1;
    return ((mode == NL_ST_SIGMA || mode == NL_ST_WINSOR_SIGMA) && !weighted) ? 1 : 0;
}

// workgroups of the generic pass behind an LDS-column dominant kernel (launch_stack_sigma_mlg): generic_grid at 64 / LPP pixels each
unsigned ml_generic_grid(int n_frames, unsigned gen_hint)
{
    return with_ml_lanes(n_frames, [&](auto LPP) { return generic_grid(gen_hint, 64 / LPP, 4 * kGenericGrid); });
}

}  // namespace nl
