// stack_fast_maps_winsor.hip -- the fast maps pass (include/nlstack_fastmaps.h), winsorized sigma clipping: the MAPS
// instantiations of the register-resident kernels and of the LDS-column generic pass (stack_fast_maps_impl.hpp).
#include "stack_fast_maps_impl.hpp"

namespace nl {

hipError_t maps_winsor_dominant(const StackArgs &args, const FastArgs &fargs, hipStream_t stream, const char **name,
                                hipEvent_t dominant_done)
{
    return maps_dominant<true>(args, fargs, stream, name, dominant_done);
}

hipError_t maps_winsor_generic(const StackArgs &args, const FastArgs &fargs, hipStream_t stream)
{
    return maps_generic<true>(args, fargs, stream);
}

}  // namespace nl
