// gpad_pairs.hip -- the panel-pair and relay kernel gpad_panel2_kernel<T, KQ, DROP> for shared-matrix
// batches with T = 9..16 row tiles (gfx950, f32 MFMA; layout in gpad_panel.h), its launcher with the
// KQ / DROP instantiation choice, and the diagnostic stamps.  The kernel's body is gpad_pairs.h.
#include <hip/hip_runtime.h>

#include "gpad_internal.h"
#include "gpad_panel.h"

namespace gpad {

// Phase anatomy stamps (diagnostic builds only, -DGPAD_STAMP; never in the product library): the
// shader clock (s_memtime) of workgroup 0, every wave, iterations [kStampV0, kStampV0 + kStampIts),
// at six points per iteration -- loop top, GEMM-1 issued, before its barrier, after it, GEMM-2
// issued, before the closing barrier -- read back with gpad_debug_stamps (tools/stamp_panel.py).
#ifdef GPAD_STAMP
#ifndef GPAD_STAMP_V0
#define GPAD_STAMP_V0 101
#endif
#ifndef GPAD_STAMP_PHASE_V
#define GPAD_STAMP_PHASE_V 100
#endif
constexpr int kStampV0 = GPAD_STAMP_V0, kStampIts = 4, kStampPts = 8;  // 6, 7: GEMM 1 / 2 hand-off wait returned
__device__ unsigned long long g_stamps[16][kStampIts][kStampPts];
// s_memtime into SGPRs at each point (pinned by scheduling barriers), stored once per iteration after
// the closing barrier: the store's lgkmcnt wait then sits where no LDS or scalar load is in flight,
// instead of behind each stamp (where it made every stamp wait for the LDS operands and the
// schedule's scalar loads, r03_stamp_*.txt)
#define GPAD_STAMP_AT(P)                                      \
    do {                                                      \
        __builtin_amdgcn_sched_barrier(0);                    \
        stv[P] = __builtin_amdgcn_s_memtime();                \
        __builtin_amdgcn_sched_barrier(0);                    \
    } while (0)
#define GPAD_STAMP_FLUSH()                                                                  \
    do {                                                                                    \
        if (blockIdx.x == 0 && v >= kStampV0 && v < kStampV0 + kStampIts && lane == 0)      \
            for (int q_ = 0; q_ < kStampPts; ++q_) g_stamps[threadIdx.x >> 6][v - kStampV0][q_] = stv[q_]; \
    } while (0)
#define GPAD_STAMP_DECL unsigned long long stv[kStampPts] = {0, 0, 0, 0, 0, 0, 0, 0};
// phase anatomy of workgroup 0 in the phase that starts at kStampPhaseV: entry, state loaded, after
// the load barrier, loop exit, survivors parked, after the closing barrier
constexpr int kStampPhaseV = GPAD_STAMP_PHASE_V, kStampPhasePts = 10;  // 6..9: the phase's last test (below)
__device__ unsigned long long g_pstamps[16][kStampPhasePts];
#define GPAD_PSTAMP(P)                                                                              \
    do {                                                                                            \
        __builtin_amdgcn_sched_barrier(0);                                                          \
        if (blockIdx.x == 0 && a.v_begin == kStampPhaseV && (threadIdx.x & 63) == 0)               \
            g_pstamps[threadIdx.x >> 6][P] = __builtin_amdgcn_s_memtime();                          \
        __builtin_amdgcn_sched_barrier(0);                                                          \
    } while (0)
#define GPAD_STAMP_PTR(P) (&stv[P])
// the test at the phase's last iteration: entry, decisions voted, verification done, results out
#define GPAD_PSTAMP_END(P)                  \
    do {                                    \
        if (v >= a.v_end) GPAD_PSTAMP(P);   \
    } while (0)
#else
#define GPAD_PSTAMP_END(P) \
    do {                   \
    } while (0)
#define GPAD_STAMP_AT(P) \
    do {                 \
    } while (0)
#define GPAD_STAMP_FLUSH() \
    do {                   \
    } while (0)
#define GPAD_STAMP_DECL
#define GPAD_STAMP_PTR(P) nullptr
#define GPAD_PSTAMP(P) \
    do {               \
    } while (0)
#endif

}  // namespace gpad

#include "gpad_pairs.h"  // (panel2_run: its stamp points are the macros above)

namespace gpad {

// KQ > 0 (panel2_run): the pair layout's compile-time chain shape.  The one-panel layout runs the
// runtime-shape code (KQ = 0) in every instantiation: specialised, its relay measured slower
// (6.16 vs 5.98 us per iteration at 4 panels, profiles/r03_single_mode_ab.txt).  DROP: the
// test-only fault-injection instantiation (GPAD_OPT_DEBUG_DROP_HANDOFF), launched instead of the
// product kernel only while that option is set, so the product kernel carries no trace of it.
template <int T, int KQ, bool DROP = false>
__global__ __launch_bounds__(1024) void gpad_panel2_kernel(SolveArgs<float> a) {
    static_assert(T > 8 && T <= 16, "panel pairs need 8 < T <= 16");
    constexpr int D = 2 * T - 16;  // double waves
    __shared__ Panel2Lds<T> L;
    const int count = a.count_in ? __builtin_amdgcn_readfirstlane(*a.count_in) : a.batch;
    if (a.count_in && count <= a.fin_thresh) return;  // the finisher has them
    const int panels = (count + 15) / 16;
    const bool pair = panels > (int)gridDim.x;
    // Role index.  The SIMD issues MFMAs oldest wave first, so a role's wave index sets its share
    // of the SIMD while the SIMD is contended.  One-panel layout: the roles are dealt from the
    // last wave down, so the relay pieces of tile T-1 (roles T, T+1) and its receiver run on the
    // oldest waves of their SIMDs and the sequential relay is not starved -- 5.92 -> 5.71 us per
    // iteration at one panel per CU, 6.93 -> 6.75 at 4096 (r03_wave_order_ab.txt).  Pairs: the
    // two hand-off receivers (roles 12, 13, SIMDs 0, 1) swap waves with the doubles of roles 8, 9,
    // so a receiver's chain -- which starts only when its piece arrives -- is not the youngest on
    // its SIMD: -1 to -3 % per pair iteration, C4 -0.2 to -1.0 % (r03_pair_perm_ab.txt; helpers
    // older than the singles, receivers oldest, or both, measured no better).
    const int w0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int w = pair ? ((w0 >> 1) == 4 ? w0 + 4 : ((w0 >> 1) == 6 ? w0 - 4 : w0)) : 15 - w0;
    const int items = pair ? (panels + 1) / 2 : panels;
    // hand-off (Handoff): both GEMMs run full-length chains on tiles T-2 and T-1 -- the host's
    // panel_handoff_shape (gpad_panel.h), spelled out here so the kernel's code stays as measured
    const bool ho = Handoff<T>::on && (KQ > 0 || (16 * (T - 1) < a.n && 16 * (T - 1) < a.m &&
                                                  (a.m + 15) / 16 == T && (a.n + 15) / 16 == T));
    if (threadIdx.x < 6) L.hflag[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        L.herr = 0;
        L.hdrop = DROP && blockIdx.x == 0;  // tests: workgroup 0 drops one post
    }
    if (threadIdx.x < 16) L.gred[threadIdx.x] = 0.0f;
    if (blockIdx.x == 0) {  // (r06: instead of memset dispatches before the solve)
        if (a.zero_w)
            for (int i = threadIdx.x; i < a.zero_n; i += blockDim.x) a.zero_w[i] = 0;
        if (a.gmax_part && a.v_begin == 0)  // the slots no workgroup of this launch writes
            for (int i = gridDim.x + threadIdx.x; i < kAbsmaxMaxBlocks; i += blockDim.x) a.gmax_part[i] = 0.0;
    }
    __syncthreads();
    if constexpr (Handoff<T>::on) {
        using H = Handoff<T>;
        if (pair) {  // waves 12, 13 (SIMDs 0, 1; tile T-2) receive from 14, 15 (SIMDs 2, 3; tile T-1)
            if (w < D) panel2_run<T, 2, 0, 0, 0, false, KQ, DROP>(a, L, w, 0, true, items, count);
            else if (ho && w >= 14)
                panel2_run<T, 1, 1, 0, H::S, false, KQ, DROP>(a, L, T - 1, w & 1, true, items, count, HoSlots{-1, w & 1});
            else if (ho && w >= 12)
                panel2_run<T, 1, 2, H::S, 0, false, KQ, DROP>(a, L, T - 2, w & 1, true, items, count, HoSlots{w & 1, -1});
            else panel2_run<T, 1, 0, 0, 0, false, KQ, DROP>(a, L, D + ((w - D) >> 1), (w - D) & 1, true, items, count);
        } else {  // tile T-1 as a relay: waves T -> T+1 -> T-1
            if constexpr (!H::relay) {
                if (w < T) panel2_run<T, 1, 0, 0, 0, false, 0, DROP>(a, L, w, 0, false, items, count);
                else panel2_run<T, 0, 0, 0, 0, false, 0, DROP>(a, L, 0, 0, false, items, count);
            } else if (ho && w == T - 1) panel2_run<T, 1, 2, H::R2, 0, true, 0, DROP>(a, L, w, 0, false, items, count, HoSlots{1, -1});
            else if (ho && w == T)
                panel2_run<T, 0, 3, 0, H::R1, true, 0, DROP>(a, L, T - 1, 0, false, items, count, HoSlots{-1, 0});
            else if (ho && w == T + 1)
                panel2_run<T, 0, 3, H::R1, H::R2, true, 0, DROP>(a, L, T - 1, 0, false, items, count, HoSlots{0, 1});
            else if (w < T)
                panel2_run<T, 1, 0, 0, 0, false, 0, DROP>(a, L, w, 0, false, items, count);
            else panel2_run<T, 0, 0, 0, 0, false, 0, DROP>(a, L, 0, 0, false, items, count);
        }
    } else if (pair) {
        if (w < D) panel2_run<T, 2, 0, 0, 0, false, KQ, DROP>(a, L, w, 0, true, items, count);
        else panel2_run<T, 1, 0, 0, 0, false, KQ, DROP>(a, L, D + ((w - D) >> 1), (w - D) & 1, true, items, count);
    } else {
        if (w < T) panel2_run<T, 1, 0, 0, 0, false, 0, DROP>(a, L, w, 0, false, items, count);
        else panel2_run<T, 0, 0, 0, 0, false, 0, DROP>(a, L, 0, 0, false, items, count);
    }
    if (Handoff<T>::on || a.gmax_part) {
        __syncthreads();
        // an expired hand-off or dataflow wait fails the run (GPAD_ERR_DEVICE)
        if (Handoff<T>::on && threadIdx.x == 0 && L.herr) atomicOr(a.err, kDevErrHandoff);
        if (a.gmax_part && threadIdx.x == 0) {  // the run's max |g|: this workgroup's slot
            float g = 0.0f;
            for (int i = 0; i < 16; ++i) g = absmax_nan(g, L.gred[i]);
            // the run's first launch stores (gmax_part note, gpad_internal.h), later phases max in
            a.gmax_part[blockIdx.x] = a.v_begin == 0 ? (double)g : absmax_nan(a.gmax_part[blockIdx.x], (double)g);
        }
    }
}

template <int T>
static void launch_pairs_t(const SolveArgs<float>& a, int grid, hipStream_t s) {
    if constexpr (T == 13) {
        // the C3/C4 shapes (T = 13) with full-length chains and one last-block length in both
        // GEMMs: the compile-time variant (panel2_run KQ)
        const int kq1 = (a.m - 16 * (T - 1) + 3) / 4, kq2 = (a.n - 16 * (T - 1) + 3) / 4;
        const bool full = panel_handoff_shape(T, a.n, a.m) && kq1 == kq2;
        if (a.debug & kDebugDropHandoff) {  // tests only: the fault-injection instantiations
            if (full && kq1 == 2) hipLaunchKernelGGL((gpad_panel2_kernel<T, 2, true>), dim3(grid), dim3(1024), 0, s, a);
            else hipLaunchKernelGGL((gpad_panel2_kernel<T, 0, true>), dim3(grid), dim3(1024), 0, s, a);
            return;
        }
        if (full && kq1 == 1) { hipLaunchKernelGGL((gpad_panel2_kernel<T, 1>), dim3(grid), dim3(1024), 0, s, a); return; }
        if (full && kq1 == 2) { hipLaunchKernelGGL((gpad_panel2_kernel<T, 2>), dim3(grid), dim3(1024), 0, s, a); return; }
        if (full && kq1 == 3) { hipLaunchKernelGGL((gpad_panel2_kernel<T, 3>), dim3(grid), dim3(1024), 0, s, a); return; }
        if (full && kq1 == 4) { hipLaunchKernelGGL((gpad_panel2_kernel<T, 4>), dim3(grid), dim3(1024), 0, s, a); return; }
    }
    hipLaunchKernelGGL((gpad_panel2_kernel<T, 0>), dim3(grid), dim3(1024), 0, s, a);
}

// one phase launch of the pair kernel, T = 9..16 (the phase loop is gpad_phases.cpp's)
hipError_t launch_panel_pairs(int T, const SolveArgs<float>& a, int grid, hipStream_t s) {
    switch (T) {
        case 9: launch_pairs_t<9>(a, grid, s); break;
        case 10: launch_pairs_t<10>(a, grid, s); break;
        case 11: launch_pairs_t<11>(a, grid, s); break;
        case 12: launch_pairs_t<12>(a, grid, s); break;
        case 13: launch_pairs_t<13>(a, grid, s); break;
        case 14: launch_pairs_t<14>(a, grid, s); break;
        case 15: launch_pairs_t<15>(a, grid, s); break;
        case 16: launch_pairs_t<16>(a, grid, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

#ifdef GPAD_STAMP
hipError_t read_stamps(unsigned long long* out, size_t bytes) {
    // g_stamps, then (when the buffer has room) g_pstamps
    size_t b0 = bytes > sizeof(g_stamps) ? sizeof(g_stamps) : bytes;
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), b0, 0, hipMemcpyDeviceToHost);
    if (e != hipSuccess || bytes <= sizeof(g_stamps)) return e;
    size_t b1 = bytes - sizeof(g_stamps);
    if (b1 > sizeof(g_pstamps)) b1 = sizeof(g_pstamps);
    return hipMemcpyFromSymbol(out + sizeof(g_stamps) / 8, HIP_SYMBOL(g_pstamps), b1, 0, hipMemcpyDeviceToHost);
}
#endif

}  // namespace gpad
