// gpad_loop_fleet.hip -- gpad_loop_fleet_kernel (gpad_loop.h): per-pack matrices.
#include "gpad_loop.h"

namespace gpad {

LoopFn loop_fn_fleet(int ka, int kb) { return loop_fn_of<kLoopFleet>(ka, kb); }

}  // namespace gpad
