// gpad_loop_farkas.hip -- gpad_loop_farkas_kernel (gpad_loop.h) for one shared plant:
// the asynchronous loop with the infeasibility certificate (gpad_infeasibility_loop_async).
#include "gpad_loop.h"

namespace gpad {

LoopFarkasFn loop_farkas_fn_shared(int ka, int kb) { return loop_farkas_fn_of<kLoopShared>(ka, kb); }

}  // namespace gpad
