// stack_fast_decide_shallow.hip -- the DECISION pass (stack_fast_decide.hip) for shallow stacks: the RECORD instantiations
// of the zonal sigma / winsorized kernel at network sizes 16 / 24 / 32, i.e. 9 ... 32 frames.
//
// The weighted default pass has no use for them (up to 40 / 32 frames the tile replay wins, stack_kernels.h), so
// stack_fast_decide.hip starts at 33 frames and stays as it is.  The weighted clip pass whose weights follow their
// frames (include/nlstack_wclip.h, stack_clip_weighted.hip) does: the reference's auto mode picks sigma at 6 ... 14 and
// winsorized sigma at 15 ... 24 frames, and that pass needs nothing but the thresholds.  Below 9 frames there is no zonal
// kernel (network size 8 has no room between the zones); the column kernel takes those stacks.
#include <string.h>

#define NL_STAT(i, x) ((void)0)
#include "stack_fast_sigma_impl.hpp"
#include "launch_common.hpp"

namespace nl {

int decide_shallow_supported(int mode, int n_frames, int64_t npix)
{
    if (mode != NL_ST_SIGMA && mode != NL_ST_WINSOR_SIGMA) return 0;
    return (n_frames >= 9 && n_frames <= 32 && npix < kFastMaxPixels) ? 1 : 0;
}

constexpr char kSigmaFastName[] = "stack_sigma_fast_kernel";

hipError_t launch_stack_sigma_decide_shallow(const StackArgs &args, hipStream_t stream, bool winsor, const char **name)
{
    if (!args.bounds || !args.nrounds || args.n_frames < 9 || args.n_frames > 32) return hipErrorInvalidValue;
    Launcher L(stream);
    FastArgs f;
    memset(&f, 0, sizeof f);
    with_bool(winsor, [&](auto W) {
        with_class<16, 24, 32>(args.n_frames, [&](auto C) {
            with_bool(args.n_frames == decltype(C)::value, [&](auto T) {
                constexpr int NS = decltype(C)::value;
                constexpr bool WINSOR = decltype(W)::value, TIGHT = decltype(T)::value;
                *name = kernel_name<kSigmaFastName, NS, true, WINSOR, TIGHT, true, false>();
                L(stack_sigma_fast_kernel<NS, true, WINSOR, TIGHT, true>, pixel_grid(args.npix), 256, 0, args, f);
            });
        });
    });
    return L.err;
}

}  // namespace nl
