// stack_fast_mlz.hip -- dispatch of the LDS-column sigma / winsor kernels (stack_fast_mlz_impl.hpp) over the
// frame-count classes: NTOP = frames rounded up to a multiple of 16, 2 lanes per pixel up to 256 frames, else 4
#include <string.h>

#include "launch_common.hpp"

namespace nl {

bool launch_mlz_part_a(int ntop, bool winsor, const StackArgs &args, const FastArgs &f, Launcher &L, const char **name);
bool launch_mlz_part_b(int ntop, bool winsor, const StackArgs &args, const FastArgs &f, Launcher &L, const char **name);
bool launch_mlz_part_c(int ntop, bool winsor, const StackArgs &args, const FastArgs &f, Launcher &L, const char **name);
bool launch_mlz_part_d(int ntop, bool winsor, const StackArgs &args, const FastArgs &f, Launcher &L, const char **name);
// (stack_fast_mlz_maps_{a,b,c,d}.hip: the MAPS instantiations of the same classes)
bool launch_mlz_maps_part_a(int ntop, bool winsor, const StackArgs &args, const FastArgs &f, Launcher &L, const char **name);
bool launch_mlz_maps_part_b(int ntop, bool winsor, const StackArgs &args, const FastArgs &f, Launcher &L, const char **name);
bool launch_mlz_maps_part_c(int ntop, bool winsor, const StackArgs &args, const FastArgs &f, Launcher &L, const char **name);
bool launch_mlz_maps_part_d(int ntop, bool winsor, const StackArgs &args, const FastArgs &f, Launcher &L, const char **name);
static constexpr decltype(&launch_mlz_part_a) kParts[4] = {launch_mlz_part_a, launch_mlz_part_b, launch_mlz_part_c, launch_mlz_part_d};
static constexpr decltype(&launch_mlz_part_a) kMapsParts[4] = {launch_mlz_maps_part_a, launch_mlz_maps_part_b, launch_mlz_maps_part_c,
                                                               launch_mlz_maps_part_d};

int fast_mlz_supported(int mode, bool weighted, int n_frames)
{
    if (weighted || (mode != NL_ST_SIGMA && mode != NL_ST_WINSOR_SIGMA)) return 0;
    return (n_frames > 128 && n_frames <= 512) ? 1 : 0;
}

int decide_ml_supported(int mode, int n_frames, int64_t npix)
{
    return (fast_mlz_supported(mode, false, n_frames) && npix < kFastMaxPixels) ? 1 : 0;
}

// the zonal launch over the whole tile (the generic pass over its hand-over list is stack_fast_mlg.hip); the part that
// instantiates the class sets *name.  Form::Maps: the MAPS instantiation of the class -- every pixel the kernel decides gets
// its word of args.reject_map beside its result.  Form::Record: the plain instantiation as a decision pass, which reads
// FastArgs::record_only -- the kernel gets a FastArgs of its own, all bytes zero (cert_every too) but that field; `fargs`
// is not read
hipError_t launch_stack_sigma_mlz(const StackArgs &args, const FastArgs &fargs, hipStream_t stream, const char **name,
                                  bool winsor, Form form)
{
    const bool maps = form == Form::Maps;
    if (form == Form::Follow || !form_args_ok(form, args) ||
        (maps && (fargs.record_only || !fast_mlz_supported(winsor ? NL_ST_WINSOR_SIGMA : NL_ST_SIGMA, false, args.n_frames))))
        return hipErrorInvalidValue;
    Launcher L(stream);
    FastArgs f = whole_tile(fargs);
    if (form == Form::Record) {
        memset(&f, 0, sizeof f);
        f.record_only = 1;
    }
    const int ntop = (args.n_frames + 15) / 16 * 16;
    const auto *const parts = maps ? kMapsParts : kParts;
    bool ok = false;
    for (int i = 0; i < 4 && !ok; i++) ok = parts[i](ntop, winsor, args, f, L, name);
    return ok ? L.err : hipErrorInvalidValue;
}

}  // namespace nl
