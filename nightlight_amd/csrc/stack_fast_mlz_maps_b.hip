// stack_fast_mlz_maps_b.hip -- the MAPS instantiations of the LDS-column sigma / winsor kernels (stack_fast_mlz_impl.hpp) of
// the frame-count classes 272 .. 352 (4 lanes per pixel): the dominant kernels of the deep maps pass
// (include/nlstack_deepmaps.h); units of their own beside stack_fast_mlz_b.hip, which instantiates exactly what it did
#include "stack_fast_mlz_impl.hpp"

namespace nl {

bool launch_mlz_maps_part_b(int ntop, bool winsor, const StackArgs &args, const FastArgs &f, Launcher &L, const char **name)
{
    return launch_mlz_classes<4, true, 272, 288, 304, 320, 336, 352>(ntop, winsor, args, f, L, name);
}

}  // namespace nl
