// gpad_resident_farkas.hip -- gpad_resident_farkas_kernel<KA, KB>: the resident kernel's text
// (gpad_resident_solve.inc, non-flat) with the infeasibility certificate of gpad_farkas.h.  A unit of its
// own, so that its 64 bucket pairs compile beside gpad_resident.hip's.
//
// At a certificate event (every fourth test) the G/L lanes publish y+ and pD of their rows to LDS and the
// G/L waves their fp64 partials of q = sum y+ pD; after Algorithm 1 found no code, q > 0 nominates and
// farkas_decide -- the stream kernel's text, on the k-major G_L image in global memory -- decides.  Beyond
// the event countdown the iteration is gpad_resident_kernel's.  LDS: 8 KA + 8 KB + 64 bytes more (< 4 KB).
// Registers and scratch per bucket pair against the unbound twin: profiles/r21_infeasible_resident.txt.
#include <hip/hip_runtime.h>

#include <cmath>

#include "gpad_chain.h"
#include "gpad_farkas.h"
#include "gpad_internal.h"

namespace gpad {

#define GPAD_RSTAMP(P) \
    do {               \
    } while (0)

#define GPAD_RESIDENT_FK 1
#include "gpad_resident_solve.inc"
#undef GPAD_RESIDENT_FK

hipError_t launch_resident_farkas(const SolveArgs<float>& a, const FarkasArgs& fk, int ka, int kb, int threads,
                                  hipStream_t st) {
    with_buckets(ka, kb, [&](auto KA, auto KB) {
        hipLaunchKernelGGL((gpad_resident_farkas_kernel<decltype(KA)::value, decltype(KB)::value>), dim3(a.batch),
                           dim3(threads), 0, st, a, fk);
    });
    return hipGetLastError();
}

}  // namespace gpad
