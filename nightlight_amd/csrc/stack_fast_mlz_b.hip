// stack_fast_mlz_b.hip -- the LDS-column sigma / winsor kernels (stack_fast_mlz_impl.hpp) of the frame-count
// classes 272 .. 352 (4 lanes per pixel); the classes are spread over four files so that they build in parallel
#include "stack_fast_mlz_impl.hpp"

namespace nl {

bool launch_mlz_part_b(int ntop, bool winsor, const StackArgs &args, const FastArgs &f, Launcher &L, const char **name)
{
    return launch_mlz_classes<4, false, 272, 288, 304, 320, 336, 352>(ntop, winsor, args, f, L, name);
}

}  // namespace nl
