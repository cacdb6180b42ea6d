// gpad_resident.hip -- gpad_resident_kernel<KA, KB, FLAT>, the latency family (f32, n, m <= 208).
// One workgroup per instance; each lane holds ONE matrix row in VGPRs for the whole solve, so an
// iteration touches no memory but LDS.  Waves [0,nA) own the rows of -ML, waves [nA,nA+nB) the rows
// of G/L; w and zhat are broadcast through LDS (ds_read_b128).  Numerics: gpad_stream.hip's header.
// The kernel's text is gpad_resident_solve.inc; its variant with the infeasibility certificate,
// gpad_resident_farkas_kernel<KA, KB>, is instantiated in gpad_resident_farkas.hip.
#include <hip/hip_runtime.h>

#include <cmath>

#include "gpad_chain.h"
#include "gpad_farkas.h"
#include "gpad_internal.h"

namespace gpad {

// FLAT = the structure-exploiting battery variant (gpad_flat.hip header; seq_functions.cpp:5-43):
// a primal row (i, j) carries only its 6N structural coefficients (KA = bucket(6N)) and chains
// over a per-cell permuted copy of w (wP[j][s] = w[j + n_u s], s < 4N; w[4 n_u N + s - 4N] after),
// so the 8b half-iteration is 6N steps long instead of m.  A-lanes are laid out so every 16-lane
// DPP row serves one cell j (lane = 16 times of that cell), hence one broadcast segment per row.
// Constraint rows chain over the natural zhat with the flat G_L expanded to full rows (exact: the
// added terms are exact zeros), with the flat step's epilogue (s + w) + p_D, y < 0 -> 0.
// (kFlatMaxCells: gpad_chain.h)

// Iteration anatomy stamps of the resident kernel (diagnostic builds only, -DGPAD_STAMP): shader
// clock of workgroup 0, every wave, iterations [101, 105), at six points -- loop top, 8b chain done,
// after the first barrier, 8d chain done, its epilogue done, after the second barrier
// (gpad_debug_res_stamps, tools/stamp_resident.py).
#ifdef GPAD_STAMP
__device__ unsigned long long g_res_stamps[8][4][6];
#define GPAD_RSTAMP(P)                                                                         \
    do {                                                                                       \
        if (blockIdx.x == 0 && v >= 101 && v < 105 && (tid & 63) == 0)                        \
            g_res_stamps[tid >> 6][v - 101][P] = __builtin_amdgcn_s_memtime();                 \
    } while (0)
hipError_t read_res_stamps(unsigned long long* out, size_t bytes) {
    if (bytes > sizeof(g_res_stamps)) bytes = sizeof(g_res_stamps);
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_res_stamps), bytes, 0, hipMemcpyDeviceToHost);
}
#else
#define GPAD_RSTAMP(P) \
    do {               \
    } while (0)
#endif

#define GPAD_RESIDENT_FK 0
#include "gpad_resident_solve.inc"
#undef GPAD_RESIDENT_FK

// one launch of the (ka, kb) bucket pair's instantiation (gpad_chain.h with_buckets)
template <bool FLAT>
static hipError_t launch_res(const SolveArgs<float>& a, int ka, int kb, int threads, hipStream_t st) {
    with_buckets(ka, kb, [&](auto KA, auto KB) {
        hipLaunchKernelGGL((gpad_resident_kernel<decltype(KA)::value, decltype(KB)::value, FLAT>), dim3(a.batch),
                           dim3(threads), 0, st, a);
    });
    return hipGetLastError();
}

bool resident_supported(int n, int m) {
    const int mx = n > m ? n : m;
    const int threads = 64 * (((n + 63) >> 6) + ((m + 63) >> 6));
    return mx <= kResidentMaxRow && threads <= kResidentMaxThreads && n > 0 && m > 0;
}

hipError_t launch_resident(const SolveArgs<float>& a, hipStream_t st, bool* supported, const FarkasArgs* fk) {
    *supported = resident_supported(a.n, a.m);
    if (!*supported) return hipSuccess;
    const int threads = 64 * (((a.n + 63) >> 6) + ((a.m + 63) >> 6));
    if (fk) return launch_resident_farkas(a, *fk, res_bucket(a.m), res_bucket(a.n), threads, st);
    return launch_res<false>(a, res_bucket(a.m), res_bucket(a.n), threads, st);  // A rows run over m, B rows over n
}

// flat battery variant: primal chains of 6N, constraint chains of n (flat G_L expanded to the
// k-major image a.GLt by the host at gpad_setup_flat); a.MGt = flat -ML (Nh x m row-major)
bool flat_resident_supported(int n, int m, int n_u) {
    if (n_u <= 0 || n_u > kFlatMaxCells || n % n_u) return false;
    const int Nh = n / n_u;
    const int laneA = n_u * ((Nh + 15) / 16) * 16;
    const int threads = 64 * ((laneA + 63) / 64) + 64 * ((m + 63) / 64);
    return 6 * Nh <= kResidentMaxRow && n <= kResidentMaxRow && threads <= kResidentMaxThreads &&
           m >= 4 * n;
}

hipError_t launch_flat_resident(const SolveArgs<float>& a, hipStream_t st) {
    const int Nh = a.n / a.n_u;
    const int laneA = a.n_u * ((Nh + 15) / 16) * 16;
    const int threads = 64 * ((laneA + 63) / 64) + 64 * ((a.m + 63) / 64);
    return launch_res<true>(a, res_bucket(6 * Nh), res_bucket(a.n), threads, st);
}

}  // namespace gpad
