// stack_exact_coop.hip -- bit-exact StackSigma / StackWinsorSigma replay, one WAVEFRONT per pixel.
//
// The register-resident kernels hand ~1e-4 of the pixels (a sample inside the
// few-ulp clip window) to an exact replay.  With so few pixels the
// one-pixel-per-lane kernel of stack_exact.hip is pure latency (a handful of
// active lanes crawling through divergent loops); here the 64 lanes of a wave
// cooperate on ONE pixel and still execute the reference's algorithm in the
// reference's order, so every bit and both counters are unchanged:
//   gather      stack.go:380-387   64 frames per step, order-preserving compaction (ballot + popcount)
//   quickselect qsort.go:94-126    a whole Hoare partition pass at once: the misplaced elements of
//                                  both sides are listed with ballot + popcount and the pass's
//                                  swaps are done in parallel (see coop_select)
//   mean/stddev stats.go:246-261   the fp32 sums stay sequential: a DPP wave-shift add chain, 64
//                                  elements per step; differences and squares are computed 64 at a time
//   winsorize   stack.go:646-672   the copy is clamped 64 samples at a time (ballot counts `changed`),
//                                  its mean / stddev are the same sequential sums
//   clip        stack.go:411-424   swap-with-last, same visiting order, clean stretches skipped 64 at a time
// The pixel's column lives in LDS as a plain array (n_frames floats per wave;
// the winsorized variant keeps its clamped copy in a second one).
#include <stdint.h>
#include <stdlib.h>

#include "stack_kernels.h"

namespace nl {

#ifdef NL_PROBE
__device__ unsigned long long nl_probe_cycles[8];
#define NL_T0() nl_t = (long long)__builtin_readcyclecounter()
#define NL_T(slot) do { const long long nl_n = (long long)__builtin_readcyclecounter(); nl_acc[slot] += nl_n - nl_t; nl_t = nl_n; } while (0)
#define NL_TDECL() long long nl_t = 0, nl_acc[5] = {0, 0, 0, 0, 0}; const long long nl_c0 = (long long)__builtin_readcyclecounter(), nl_r0 = (long long)__builtin_amdgcn_s_memrealtime()
#define NL_TFLUSH() do { if (threadIdx.x == 0) { for (int q = 0; q < 5; q++) atomicAdd(&nl_probe_cycles[q], (unsigned long long)nl_acc[q]); \
        atomicAdd(&nl_probe_cycles[5], (unsigned long long)((long long)__builtin_readcyclecounter() - nl_c0)); \
        const unsigned long long nl_w = (unsigned long long)((long long)__builtin_amdgcn_s_memrealtime() - nl_r0); \
        atomicAdd(&nl_probe_cycles[6], nl_w); atomicMax(&nl_probe_cycles[7], nl_w); } } while (0)
#endif

}  // namespace nl
#include "stack_exact_coop_impl.hpp"
#include "launch_common.hpp"
namespace nl {

template <bool WINSOR, bool W, int GROUP, int PF = 2, bool MAPS = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(PF <= 2 ? 8 : 5, 8))) void stack_sigma_coop_kernel(StackArgs p)
{
    extern __shared__ float a[];
    coop_body<WINSOR, W, GROUP, PF, MAPS>(p, a, blockIdx.x, gridDim.x);
}

// StackMedian (stack.go:274-303) beyond the register kernels' 512 frames: gather and the
// same wave-wide quickselect, nothing else.
__global__ __launch_bounds__(64) void stack_median_coop_kernel(StackArgs p)
{
    extern __shared__ float a[];
    unsigned short *lpos = reinterpret_cast<unsigned short *>(a + p.n_frames);
    unsigned short *rfwd = lpos + p.n_frames;
    const int lane = threadIdx.x;
    const int N = p.n_frames;
    int64_t wg = blockIdx.x;                       // XCD-contiguous pixels, see stack_sigma_coop_kernel
    if ((gridDim.x & 7u) == 0u) wg = (int64_t)(blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    for (int64_t pix = wg; pix < p.npix; pix += gridDim.x) {
        const float *fr = p.frames + pix;
        lds_fence();
        int n = 0;
        for (int base = 0; base < N; base += 64) {
            const int k = base + lane;
            const float x = k < N ? fr[(int64_t)k * p.stride] : __builtin_nanf("");
            const bool valid = x == x;
            const unsigned long long m = ballot64(valid);
            if (valid) a[n + below64(m)] = x;
            n += __popcll(m);
        }
        lds_fence();
        const float res = n > 0 ? coop_select_median(a, lpos, rfwd, n) : p.ref_loc;
        if (lane == 0) p.out[pix] = res;
    }
}

hipError_t launch_stack_median_coop(const StackArgs &args, int grid, hipStream_t stream, const char **name)
{
    Launcher L(stream);
    *name = "stack_median_coop_kernel";
    L(stack_median_coop_kernel, grid, 64, (size_t)args.n_frames * 2 * sizeof(float), args);
    return L.err;
}

static size_t coop_columns(int mode, bool weighted)
{
    return (mode == NL_ST_WINSOR_SIGMA ? 2 : 1) + (weighted ? 1 : 0) + 1;      // samples (+copy) (+weights) + 2 scratch columns of 16 bits
}

int coop_supported(int mode, bool weighted, int n_frames)
{
    if (mode == NL_ST_MEDIAN) return (n_frames <= 65535 && (size_t)n_frames * 2 * sizeof(float) <= 64 * 1024) ? 1 : 0;
    if (mode != NL_ST_SIGMA && mode != NL_ST_WINSOR_SIGMA) return 0;
    return (n_frames <= 65535 && (size_t)n_frames * coop_columns(mode, weighted) * sizeof(float) <= 64 * 1024) ? 1 : 0;
}

// whole-tile replays take four pixels per work item when the 16-byte loads are aligned (nlstack_api.hip sizes the grid
// with the same predicate)
int coop_group(const StackArgs &args)
{
    const bool ok = args.list == nullptr && args.npix % 4 == 0 && args.stride % 4 == 0 && args.npix >= 1024 &&
                    (reinterpret_cast<uintptr_t>(args.frames) & 15u) == 0;
    return ok ? 4 : 1;
}

constexpr char kSigmaCoopName[] = "stack_sigma_coop_kernel";

template <bool WINSOR, bool W, int GROUP, int PF>
static void launch_coop(Launcher &L, const StackArgs &args, int grid, size_t lds, const char **name)
{
    *name = kernel_name<kSigmaCoopName, WINSOR, W, GROUP, PF>();
    L(stack_sigma_coop_kernel<WINSOR, W, GROUP, PF>, grid, 64, lds, args);
}

// Form::Maps (include/nlstack_deepstackmaps.h): {sigma, winsorized} x {1, 4 pixels per work item}, two chunks in registers
// (the PF = 8 variants serve up to 512 frames, where the maps passes have engines of their own)
template <bool WINSOR, int GROUP>
static void launch_coop_maps(Launcher &L, const StackArgs &args, int grid, size_t lds, const char **name)
{
    *name = maps_kernel_name<kSigmaCoopName, WINSOR, false, GROUP, 2>();
    L(stack_sigma_coop_kernel<WINSOR, false, GROUP, 2, true>, grid, 64, lds, args);
}

hipError_t launch_stack_sigma_coop(int mode, const StackArgs &args, int grid, hipStream_t stream, const char **name, Form form)
{
    if (form == Form::Follow || form == Form::Record || !form_args_ok(form, args)) return hipErrorInvalidValue;
    if (form == Form::Maps) {
        if (args.weights || args.list) return hipErrorInvalidValue;      // the whole-tile, unweighted replay only
        const size_t lds = (size_t)args.n_frames * sizeof(float) * coop_columns(mode, false);
        const bool group4 = coop_group(args) == 4;
        Launcher L(stream);
        with_bool(mode == NL_ST_WINSOR_SIGMA, [&](auto WS) {
            if (group4) launch_coop_maps<decltype(WS)::value, 4>(L, args, grid, lds, name);
            else        launch_coop_maps<decltype(WS)::value, 1>(L, args, grid, lds, name);
        });
        return L.err;
    }
    // (measured, profiles/r05_wsigma512_pf8_*, r05_wwinsor512_*: with PF = 8 a weighted sigma replay of 512 frames fetches
    // 1.45 x the algorithmic bytes instead of 13.7 x and takes 35.8 instead of 34.6 ms per 1024 x 4096 pixels -- it is bound by
    // the issue of the partition passes, not by its fetches; the winsorized replay, whose loops wait on memory between
    // their chains, gains 10 - 12 %: 40.5 -> 36.5 ms.  PF = 4 at 129 ... 256 frames lost 6 - 7 % in both modes.)
    static const bool deep_on = [] { const char *e = getenv("NL_COOP_PF"); return !(e && e[0] == '0'); }();      // NL_COOP_PF=0: two chunks at every depth (A/B)
    static const bool deep_all = [] { const char *e = getenv("NL_COOP_PF"); return e && e[0] == '2'; }();       // NL_COOP_PF=2: plain sigma too
    const bool weighted = args.weights != nullptr;
    const size_t lds = (size_t)args.n_frames * sizeof(float) * coop_columns(mode, weighted);
    const bool group4 = coop_group(args) == 4;
    Launcher L(stream);
    with_bool(mode == NL_ST_WINSOR_SIGMA, [&](auto WS) {
        with_bool(weighted, [&](auto WT) {
            constexpr bool WINSOR = decltype(WS)::value, W = decltype(WT)::value;
            if (group4 && deep_on && (WINSOR || deep_all) && args.n_frames > 256 && args.n_frames <= 512)
                launch_coop<WINSOR, W, 4, 8>(L, args, grid, lds, name);
            else if (group4)
                launch_coop<WINSOR, W, 4, 2>(L, args, grid, lds, name);
            else
                launch_coop<WINSOR, W, 1, 2>(L, args, grid, lds, name);
        });
    });
    return L.err;
}

}  // namespace nl

#ifdef NL_PROBE
extern "C" int nl_debug_probe(unsigned long long *out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(nl::nl_probe_cycles), sizeof(nl::nl_probe_cycles)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[8] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(nl::nl_probe_cycles), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
