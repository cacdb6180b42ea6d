// gpad_loop_plant_farkas.hip -- gpad_loop_farkas_kernel (gpad_loop.h) for per-pack plant maps on shared matrices:
// the asynchronous loop with the infeasibility certificate (gpad_infeasibility_loop_async).
#include "gpad_loop.h"

namespace gpad {

LoopFarkasFn loop_farkas_fn_per_plant(int ka, int kb) { return loop_farkas_fn_of<kLoopPerPlant>(ka, kb); }

}  // namespace gpad
