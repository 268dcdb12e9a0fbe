// stack_fast_decide.hip -- weighted sigma / winsorized sigma clipping: the DECISION pass.
//
// StackSigmaWeighted / StackWinsorSigmaWeighted (stack.go:442-531, 710-829) reject exactly as their unweighted
// twins -- median and standard deviation ignore the weights -- and differ only in the result: the weighted mean of
// the survivors IN THE ORDER the quickselects and the clip swaps left them, with weights that followed only the
// clip swaps (stack.go:487).  That order has to be replayed (stack_exact_coop*.hip), but the bounds of every
// clipping round need not be: the register-resident kernel (stack_fast_sigma_impl.hpp, RECORD) decides them with its
// interval guard -- on the sorted column, no permutation involved -- and leaves thresholds per round and pixel; the
// replay then only permutes and clips, without the sequential sums of MeanStdDev (stats.go:246-261) and without the
// winsorization loop (stack.go:646-672: about 20 such sums per clipping round).  Pixels the guard cannot decide
// (1e-4 .. 1e-2 of them), the NaN borders and pixels that clip more than the zones hold are replayed in full.
#include <string.h>

#define NL_STAT(i, x) ((void)0)
#include "stack_fast_sigma_impl.hpp"
#include "launch_common.hpp"

namespace nl {

int decide_supported(int mode, int n_frames, int64_t npix)
{
    if (mode != NL_ST_SIGMA && mode != NL_ST_WINSOR_SIGMA) return 0;
    return (n_frames >= 33 && n_frames <= 128 && npix < kFastMaxPixels) ? 1 : 0;
}

constexpr char kSigmaFastName[] = "stack_sigma_fast_kernel";

hipError_t launch_stack_sigma_decide(const StackArgs &args, hipStream_t stream, bool winsor, const char **name)
{
    Launcher L(stream);
    FastArgs f;
    memset(&f, 0, sizeof f);
    with_bool(winsor, [&](auto W) {
        with_class<48, 64, 80, 96, 112, 128>(args.n_frames, [&](auto C) {
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
