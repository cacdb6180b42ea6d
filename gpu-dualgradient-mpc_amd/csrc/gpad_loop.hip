// gpad_loop.hip -- the asynchronous closed loop (gpad_loop.h): the shared-plant instantiations of the
// two-slot kernel and the launcher.
#include "gpad_loop.h"

namespace gpad {

// the instantiation for a: the two-slot kernel for shared matrices (with one plant or per-pack maps),
// the fleet kernel for per-pack matrices
static LoopFn loop_fn(const LoopArgs& a) {
    const SolveArgs<float>& s = a.s;
    const int ka = res_bucket(s.m), kb = res_bucket(s.n);
    if (s.strideA || s.strideB) return loop_fn_fleet(ka, kb);
    return a.per_plant ? loop_fn_per_plant(ka, kb) : loop_fn_of<kLoopShared>(ka, kb);
}
// its twin with the infeasibility certificate
static LoopFarkasFn loop_farkas_fn(const LoopArgs& a) {
    const SolveArgs<float>& s = a.s;
    const int ka = res_bucket(s.m), kb = res_bucket(s.n);
    if (s.strideA || s.strideB) return loop_farkas_fn_fleet(ka, kb);
    return a.per_plant ? loop_farkas_fn_per_plant(ka, kb) : loop_farkas_fn_shared(ka, kb);
}
static int loop_threads(const SolveArgs<float>& s) { return 64 * (((s.n + 63) >> 6) + ((s.m + 63) >> 6)); }

bool loop_supported(int n, int m, int nx, int nu) {
    return resident_supported(n, m) && nx >= 1 && nx <= kLoopMaxState && nu >= 1 && nu <= kLoopMaxState && nu <= n;
}

int loop_blocks_per_cu(const LoopArgs& a, bool farkas) {
    const SolveArgs<float>& s = a.s;
    if (!(s.strideA || s.strideB)) return 1;
    int nb = 0;
    // (the function that will be launched: the certificate twin has its own registers and LDS)
    const void* fn = farkas ? reinterpret_cast<const void*>(loop_farkas_fn(a)) : reinterpret_cast<const void*>(loop_fn(a));
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, loop_threads(s), 0) != hipSuccess)
        return 1;
    return nb < 1 ? 1 : (nb > 2 ? 2 : nb);
}

hipError_t launch_loop(const LoopArgs& a, int grid, hipStream_t st, const FarkasArgs* fk) {
    const SolveArgs<float>& s = a.s;
    if (!loop_supported(s.n, s.m, a.nx + a.ns, a.nu) || a.nx < 1 || a.ns < 0 || (a.ns && !a.S) || !s.qctr || s.N < 1 || a.steps < 1 || s.batch < 1 || grid < 1 ||
        grid > s.batch || grid > kAbsmaxMaxBlocks)
        return hipErrorInvalidValue;
    if (fk) {
        if (!fk->rabs || !(fk->R > 0.0) || !(s.tol > 0.0)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(loop_farkas_fn(a), dim3(grid), dim3(loop_threads(s)), 0, st, a, *fk);
    } else {
        hipLaunchKernelGGL(loop_fn(a), dim3(grid), dim3(loop_threads(s)), 0, st, a);
    }
    return hipGetLastError();
}

}  // namespace gpad
