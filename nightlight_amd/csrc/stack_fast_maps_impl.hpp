// stack_fast_maps_impl.hpp -- the MAPS instantiations of the register-resident sigma / winsorized sigma kernels and of
// their LDS-column generic pass, with their launchers: the engines of the fast maps pass (include/nlstack_fastmaps.h,
// run_sigma_maps in nlstack_pass.hip).  Included by stack_fast_maps_sigma.hip and stack_fast_maps_winsor.hip, one
// translation unit per mode (compile time); stack_fast.hip and stack_fast_mlg.hip instantiate exactly what they did.
//
// The kernels are those of the default pass (stack_fast.hip has the exactness contract) with one more store: the lane
// that stores a pixel's result also stores the pixel's two clip counts in StackArgs::reject_map.  The pass runs the
// plain protocol without a winsorization cascade, so the launchers here know neither: the dominant kernel over the tile
// (network size 8: the generic kernel over the whole tile), then the generic pass over the generic list, on a grid
// sized without a hint -- up to 64 frames the one-lane register kernel, above that the LDS-column kernel.
#pragma once
#include <algorithm>
#include <string>

#define NL_STAT(i, x) ((void)0)
#include "stack_fast_sigma_impl.hpp"
#include "stack_fast_mlg_impl.hpp"
#include "launch_common.hpp"

namespace nl {

constexpr int kMapsZonalMinSize = 16;      // smallest network size with a zonal instantiation (kZonalMinSize, stack_fast.hip)
constexpr char kSigmaFastMapsBase[] = "stack_sigma_fast_kernel";

// one lane per pixel, whole columns in LDS (stack_fast_mlg.hip): the generic pass of 65 ... 128 frames
template <bool WINSOR>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2)))
void stack_sigma_mlg_maps_kernel(StackArgs p, FastArgs q)
{
    mlg_body<1, WINSOR, true>(p, q, blockIdx.x, gridDim.x);
}

// FastArgs of a kernel of the maps pass over the whole tile: both hand-over lists, no cascade, no budgets
inline FastArgs maps_tile_args(const FastArgs &fargs)
{
    FastArgs f = whole_tile(fargs);
    f.cont_list = nullptr; f.cont_state = nullptr; f.cont_count = nullptr; f.cont_region = 0; f.in_state = nullptr;
    f.in_region = f.in_regions = f.in_group = 0;
    f.pass_budget = f.round_cap = 0;
    f.fb_snap = nullptr;
    return f;
}

template <int NS, bool WINSOR>
hipError_t launch_maps_dominant(const StackArgs &args, const FastArgs &fargs, hipStream_t stream, const char **name,
                                hipEvent_t dominant_done)
{
    Launcher L(stream);
    const unsigned tile_blocks = pixel_grid(args.npix);
    const FastArgs f = maps_tile_args(fargs);
    if constexpr (NS >= kMapsZonalMinSize) {
        with_bool(args.n_frames == NS, [&](auto T) {
            constexpr bool TIGHT = decltype(T)::value;
            *name = maps_kernel_name<kSigmaFastMapsBase, NS, true, WINSOR, TIGHT, false, false>();
            L(stack_sigma_fast_kernel<NS, true, WINSOR, TIGHT, false, false, true>, tile_blocks, 256, 0, args, f);
        });
    } else {
        *name = maps_kernel_name<kSigmaFastMapsBase, NS, false, WINSOR, false, false, false>();
        L(stack_sigma_fast_kernel<NS, false, WINSOR, false, false, false, true>, tile_blocks, 256, 0, args, f);
    }
    L.record(dominant_done);
    return L.err;
}

// over the generic list, whose length is only known on the device: a fixed grid (no hint), grid-stride loop
template <int NS, bool WINSOR>
hipError_t launch_maps_generic(const StackArgs &args, const FastArgs &fargs, hipStream_t stream)
{
    Launcher L(stream);
    if constexpr (NS >= kMapsZonalMinSize) {
        const unsigned tile_blocks = pixel_grid(args.npix);
        const FastArgs fg = over_generic_list(maps_tile_args(fargs));
        if constexpr (NS > 64)
            L(stack_sigma_mlg_maps_kernel<WINSOR>, generic_grid(0, 64, 4 * std::min(tile_blocks, kGenericGrid)), 64, 0, args, fg);
        else
            L(stack_sigma_fast_kernel<NS, false, WINSOR, false, false, false, true>,
              generic_grid(0, 256, std::min(tile_blocks, kGenericGrid)), 256, 0, args, fg);
    }
    return L.err;
}

template <bool WINSOR>
hipError_t maps_dominant(const StackArgs &args, const FastArgs &fargs, hipStream_t stream, const char **name,
                         hipEvent_t dominant_done)
{
    if (args.n_frames < 2 || args.n_frames > 128) return hipErrorInvalidValue;      // (args.reject_map: checked by the public launcher)
    return with_class<8, 16, 24, 32, 48, 64, 80, 96, 112, 128>(args.n_frames, [&](auto C) {
        return launch_maps_dominant<decltype(C)::value, WINSOR>(args, fargs, stream, name, dominant_done);
    });
}

template <bool WINSOR>
hipError_t maps_generic(const StackArgs &args, const FastArgs &fargs, hipStream_t stream)
{
    if (args.n_frames < 2 || args.n_frames > 128) return hipErrorInvalidValue;      // (args.reject_map: checked by the public launcher)
    return with_class<8, 16, 24, 32, 48, 64, 80, 96, 112, 128>(args.n_frames, [&](auto C) {
        return launch_maps_generic<decltype(C)::value, WINSOR>(args, fargs, stream);
    });
}

}  // namespace nl
