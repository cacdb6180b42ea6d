// gpad_loop_plant.hip -- gpad_loop_kernel (gpad_loop.h) for per-pack plant maps on shared matrices.
#include "gpad_loop.h"

namespace gpad {

LoopFn loop_fn_per_plant(int ka, int kb) { return loop_fn_of<kLoopPerPlant>(ka, kb); }

}  // namespace gpad
