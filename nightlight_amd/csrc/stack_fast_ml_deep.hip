// stack_fast_ml_deep.hip -- the median and MAD sigma of 513 ... 2048 frames, register-resident: the kernels of
// stack_fast_ml.hip (stack_fast_ml_impl.hpp) with LPP = 8 or 16 ADJACENT lanes per pixel, 128 samples per lane -- half a
// DPP row or a whole one, 32 or 16 pixels per workgroup.  An extension of depth, not of semantics
// (include/nlstack_deepstack.h): both modes rest on order statistics alone, so the wider column needs no guard band, no
// generic pass and no replay of undecidable pixels.
//
//   * gather and in-lane sort as on 2 and 4 lanes: lane role r loads frames r, r+LPP, ... (8 lanes serve 513 ... 1024
//     frames and 16 lanes 1025 ... 2048, always more than half of LPP * 128: ml_gather_raw's invariant);
//   * the bitonic merge of the sorted runs grows by one level per doubling: two 4-lane runs meet mirrored against lane
//     7 - r (row_half_mirror), two 8-lane runs against lane 15 - r (row_mirror); the half-cleaners behind a mirrored stage
//     run at lane distances 4 (ds_swizzle SWAP,4: no DPP control reaches lane r ^ 4), 2 and 1, then in the lane;
//   * the MAD kernel's deviations are one bitonic sequence over the pixel's lanes as before: half-cleaners at lane distance
//     8 (row_ror:8, 16 lanes only), 4, 2 and 1, then in the lane.
// Per sample the cross-lane work is 2 instructions per stage (partner move + med3): 1 / 3 / 6 / 10 cross-lane stages
// on 2 / 4 / 8 / 16 lanes for the median, 1 / 2 / 3 / 4 more for the MAD kernel.
//
// No non-temporal loads (they pay only where a wave reads whole 128-byte lines: two lanes per pixel).  The MAD kernel also
// runs in its MAPS and RECORD forms here (include/nlstack_deepstackmaps.h, include/nlstack_deepwmad.h): what they need behind
// the sorts -- pixel, role, `on` -- is computed anew like everything else (DeepThread::renew), so they spill as little.
#include <cstring>

#include "launch_common.hpp"
#include "stack_fast_ml_impl.hpp"

namespace nl {

hipError_t launch_stack_median_ml_deep(const StackArgs &args, hipStream_t stream, const char **name)
{
    Launcher L(stream);
    with_deep_lanes(args.n_frames, [&](auto LPP) {
        *name = kernel_name<kMedianMlName, decltype(LPP)::value>();
        L(stack_median_ml_kernel<decltype(LPP)::value>, pixel_grid(args.npix, LPP), 256, 0, args);
    });
    return L.err;
}

// Form::Maps (include/nlstack_deepstackmaps.h): named as the plain kernel with "maps" as its last argument.  Form::Record
// (include/nlstack_deepwmad.h): the kernel writes no list, so it gets an all-zero FastArgs and `fargs` is not read
hipError_t launch_stack_mad_ml_deep(const StackArgs &args, const FastArgs &fargs, hipStream_t stream, const char **name, Form form)
{
    if (form == Form::Follow || !form_args_ok(form, args)) return hipErrorInvalidValue;
    Launcher L(stream);
    with_deep_lanes(args.n_frames, [&](auto LPP) {
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

// 513 ... 2048 active frames, the median or MAD sigma without weights, and LPP frames of the handle's stride within a signed
// 32-bit byte offset (the gather's descriptors and per-lane offsets: pixel + role * frame < LPP * frame): a stride below
// 2^26 pixels at 8 lanes, below 2^25 at 16
int deep_ml_supported(int mode, bool weighted, int n_frames, int64_t stride)
{
    if (n_frames <= 4 * kMlNS || n_frames > 16 * kMlNS || stride <= 0) return 0;
    const int64_t lanes = with_deep_lanes(n_frames, [](auto LPP) { return (int64_t)decltype(LPP)::value; });
    if (lanes * stride * (int64_t)sizeof(float) >= ((int64_t)1 << 31)) return 0;
    if (mode == NL_ST_MEDIAN) return 1;
    return (mode == NL_ST_MAD_SIGMA && !weighted) ? 1 : 0;
}

}  // namespace nl
