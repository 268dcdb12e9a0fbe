// stack_fast_maps_sigma.hip -- the fast maps pass (include/nlstack_fastmaps.h), plain sigma clipping: the MAPS
// instantiations of the register-resident kernels and of the LDS-column generic pass (stack_fast_maps_impl.hpp), and the
// two parts of the pass as launch_stack_sigma_dominant / launch_stack_sigma_generic (stack_fast.hip) forward Form::Maps to
// them, which reach the winsorized instantiations in their own unit.
#include "stack_fast_maps_impl.hpp"

namespace nl {

// (stack_fast_maps_winsor.hip: the winsorized instantiations)
hipError_t maps_winsor_dominant(const StackArgs &args, const FastArgs &fargs, hipStream_t stream, const char **name,
                                hipEvent_t dominant_done);
hipError_t maps_winsor_generic(const StackArgs &args, const FastArgs &fargs, hipStream_t stream);

hipError_t sigma_maps_dominant(const StackArgs &args, const FastArgs &fargs, hipStream_t stream, const char **name,
                               hipEvent_t dominant_done, bool winsor)
{
    return winsor ? maps_winsor_dominant(args, fargs, stream, name, dominant_done)
                  : maps_dominant<false>(args, fargs, stream, name, dominant_done);
}

hipError_t sigma_maps_generic(const StackArgs &args, const FastArgs &fargs, hipStream_t stream, bool winsor)
{
    return winsor ? maps_winsor_generic(args, fargs, stream) : maps_generic<false>(args, fargs, stream);
}

}  // namespace nl
