// stack_linfit_maps.hip -- the MAPS instantiations of both linear-fit kernels (stack_linfit_impl.hpp, which states how a
// pixel's word is built across the cascade), reached through the launchers of stack_linfit.hip.  Same classes, lane
// counts, cascade, quotas and continuation grids as the default pass; args.reject_map must be set.
#include "stack_linfit_impl.hpp"

namespace nl {

hipError_t launch_linfit_ml_maps(const StackArgs &args, const FastArgs &fargs, const LinfitCascade *cascade,
                                 hipStream_t stream, const char **name, hipEvent_t dominant_done)
{
    return launch_linfit_ml<true>(args, fargs, cascade, stream, name, dominant_done);
}

hipError_t launch_linfit_fast_maps(const StackArgs &args, const FastArgs &fargs, const LinfitCascade *cascade,
                                   hipStream_t stream, const char **name, hipEvent_t dominant_done)
{
    return launch_linfit_fast<true>(args, fargs, cascade, stream, name, dominant_done);
}

}  // namespace nl
