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

#include "launch_common.hpp"
#include "stack_fast_ml_impl.hpp"

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

hipError_t launch_stack_median_ml(const StackArgs &args, hipStream_t stream, const char **name)
{
    Launcher L(stream);
    with_ml_lanes(args.n_frames, [&](auto LPP) {
        *name = kernel_name<kMedianMlName, decltype(LPP)::value>();
        L(stack_median_ml_kernel<decltype(LPP)::value>, pixel_grid(args.npix, LPP), 256, 0, args);
    });
    return L.err;
}

// (the kernels: stack_fast_ml_impl.hpp, shared with the 8- and 16-lane instantiations of stack_fast_ml_deep.hip)
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
