// stack_fast_maps_sigma.hip -- the fast maps pass (include/nlstack_fastmaps.h), plain sigma clipping: the MAPS
// instantiations of the register-resident kernels and of the LDS-column generic pass (stack_fast_maps_impl.hpp).
#include "stack_fast_maps_impl.hpp"

namespace nl {

hipError_t launch_stack_sigma_maps_dominant(const StackArgs &args, const FastArgs &fargs, hipStream_t stream,
                                            const char **name, hipEvent_t dominant_done)
{
    return maps_dominant<false>(args, fargs, stream, name, dominant_done);
}

hipError_t launch_stack_sigma_maps_generic(const StackArgs &args, const FastArgs &fargs, hipStream_t stream)
{
    return maps_generic<false>(args, fargs, stream);
}

}  // namespace nl
