// gpad_loop_fleet_farkas.hip -- gpad_loop_fleet_farkas_kernel (gpad_loop.h): per-pack matrices:
// the asynchronous loop with the infeasibility certificate (gpad_infeasibility_loop_async).
#include "gpad_loop.h"

namespace gpad {

LoopFarkasFn loop_farkas_fn_fleet(int ka, int kb) { return loop_farkas_fn_of<kLoopFleet>(ka, kb); }

}  // namespace gpad
