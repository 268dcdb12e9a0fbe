// stack_fast_mlg.hip -- the GENERIC pass of the multi-lane sigma / winsorized sigma kernels
// (129..512 frames; 65..128 frames for winsorized clipping): pixels a zonal kernel (stack_fast.hip,
// stack_fast_ml.hip, stack_fast_mlz.hip) handed over
// because they miss too many samples (the NaN borders of aligned frames) or clip / clamp more
// samples than its zones hold.
//
// As stack_fast_mlz.hip, but with the WHOLE merged column of a pixel in LDS ([rank][pixel],
// conflict-free) next to prefix sums of (x-c) and (x-c)^2 at every 4th rank: the alive window
// [a, b), the clamp positions and the median are plain indices into the column, any number of
// missing, clipped or clamped samples, and a round costs a few dozen LDS reads whatever the frame
// count.  (The register version of this pass masks all 128 positions of every lane in every
// round and runs one wave per SIMD: 1.9 ms for the 34 k border pixels of the C3 tile, half of
// that pass.)  One wave per workgroup, 48 KiB of LDS: three waves per CU -- this kernel only ever
// sees hand-over lists.
//
// The prefix sums run upwards from rank 0, so a sum over [i, j) is a difference of two entries
// that both contain every sample below i -- dead low outliers included.  The rounding bound
// therefore uses the magnitude of the prefix itself (`mag` below) instead of the alive samples'
// moments: a pixel with a deep cold outlier gets a wider interval, never a wrong decision.
// Exactness otherwise as in stack_fast.hip / DESIGN.md section 5.
#include "fast_ml_common.hpp"

namespace nl {

#ifdef NL_ROUND_STATS
__device__ unsigned long long nl_dbg_rounds_mlg[8];          // as nl_dbg_rounds in stack_fast.hip; [5] walk steps
extern "C" int nl_debug_round_stats_mlg(unsigned long long *out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(nl_dbg_rounds_mlg), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[8] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(nl_dbg_rounds_mlg), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#define NL_STAT(i, x) atomicAdd(&nl_dbg_rounds_mlg[i], (unsigned long long)(x))
#else
#define NL_STAT(i, x) ((void)0)
#endif

}  // namespace nl
#include "stack_fast_mlg_impl.hpp"
#include "launch_common.hpp"
namespace nl {

template <int LPP, bool WINSOR>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2)))
void stack_sigma_mlg_kernel(StackArgs p, FastArgs q)
{
    mlg_body<LPP, WINSOR>(p, q, blockIdx.x, gridDim.x);
}

// generic pass over fargs.in_list (the hand-over list of a zonal kernel): 2 or 4 lanes per pixel for
// 129..512 frames; one lane per pixel (64 pixels per wave, the same 48 KiB) for the winsorized
// one-lane kernels of stack_fast.hip, whose register version of this pass runs 28 lock-step
// winsorization rounds over all 128 masked positions -- 1.0 ms for the 57 k border pixels of a
// 128 x 4096^2 stack, less than one wave per SIMD, pure latency
static hipError_t launch_mlg_lanes_maps(const StackArgs &args, const FastArgs &fargs, unsigned grid, hipStream_t stream, bool winsor);

hipError_t launch_stack_sigma_mlg(const StackArgs &args, const FastArgs &fargs, unsigned grid, hipStream_t stream,
                                  bool winsor, Form form)
{
    if ((form != Form::Plain && form != Form::Maps) || !form_args_ok(form, args)) return hipErrorInvalidValue;
    if (form == Form::Maps) return launch_mlg_lanes_maps(args, fargs, grid, stream, winsor);
    Launcher L(stream);
    with_bool(winsor, [&](auto W) {
        constexpr bool WINSOR = decltype(W)::value;
        if (args.n_frames <= kMlNS)
            L(stack_sigma_mlg_kernel<1, WINSOR>, grid, 64, 0, args, fargs);
        else
            with_ml_lanes(args.n_frames, [&](auto LPP) {
                L(stack_sigma_mlg_kernel<decltype(LPP)::value, WINSOR>, grid, 64, 0, args, fargs);
            });
    });
    return L.err;
}

// the MAPS instantiations for 129 ... 512 frames (2 or 4 lanes per pixel): the generic pass of the deep maps pass
// (include/nlstack_deepmaps.h).  mlg_body's one store of a pixel's word sits beside the store of its result, under
// `on && role == 0`: one lane of the 2 or 4 that hold the pixel, which all carry the same counts.
template <int LPP, bool WINSOR>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2)))
void stack_sigma_mlg_lanes_maps_kernel(StackArgs p, FastArgs q)
{
    static_assert(LPP == 2 || LPP == 4, "one lane per pixel: stack_fast_maps_impl.hpp");
    mlg_body<LPP, WINSOR, true>(p, q, blockIdx.x, gridDim.x);
}

// over fargs.in_list, args.reject_map set; the list's length is only known on the device and a maps pass reads no hint:
// its caller passes the grid without one, ml_generic_grid(n, 0)
static hipError_t launch_mlg_lanes_maps(const StackArgs &args, const FastArgs &fargs, unsigned grid, hipStream_t stream, bool winsor)
{
    if (args.n_frames <= kMlNS || args.n_frames > 4 * kMlNS) return hipErrorInvalidValue;
    Launcher L(stream);
    with_bool(winsor, [&](auto W) {
        with_ml_lanes(args.n_frames, [&](auto LPP) {
            L(stack_sigma_mlg_lanes_maps_kernel<decltype(LPP)::value, decltype(W)::value>, grid, 64, 0, args, fargs);
        });
    });
    return L.err;
}

}  // namespace nl
