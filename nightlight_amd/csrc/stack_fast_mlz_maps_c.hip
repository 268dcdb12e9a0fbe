// stack_fast_mlz_maps_c.hip -- the MAPS instantiations of the LDS-column sigma / winsor kernels (stack_fast_mlz_impl.hpp) of
// the frame-count classes 368 .. 432 (4 lanes per pixel): the dominant kernels of the deep maps pass
// (include/nlstack_deepmaps.h); units of their own beside stack_fast_mlz_c.hip, which instantiates exactly what it did
#include "stack_fast_mlz_impl.hpp"

namespace nl {

bool launch_mlz_maps_part_c(int ntop, bool winsor, const StackArgs &args, const FastArgs &f, Launcher &L, const char **name)
{
    return launch_mlz_classes<4, true, 368, 384, 400, 416, 432>(ntop, winsor, args, f, L, name);
}

}  // namespace nl
