// gpad_panel.hip -- shared-matrix batches on the f32 MFMA pipe (gfx950): the fragment packer, the
// size helpers and the T-wave single-panel kernel gpad_panel_kernel<T> (T <= 8).  The fragment
// layout is described in gpad_panel.h; the panel pairs (8 < T <= 16) are gpad_pairs.hip, the phase
// boundary gpad_compact.hip, and the host loop over phases gpad_phases.cpp.
#include <hip/hip_runtime.h>

#include <cmath>

#include "gpad_farkas.h"
#include "gpad_internal.h"
#include "gpad_panel.h"

namespace gpad {

// ---------------------------------------------------------------------------------------
// packing
// ---------------------------------------------------------------------------------------
__global__ void pack_panel_kernel(const float* __restrict__ src, int rows, int cols, double scale,
                                  int T, float4* __restrict__ dst) {
    // dst[(b*T + t)*64 + lane] for b < T (16-col blocks), t < T (16-row tiles)
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= T * T * 64) return;
    const int lane = idx & 63, t = (idx >> 6) % T, b = (idx >> 6) / T;
    const int row = 16 * t + pi16(lane & 15);
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int col = 16 * b + 4 * q + (lane >> 4);
        v[q] = (row < rows && col < cols) ? (float)(scale * (double)src[(size_t)row * cols + col]) : 0.0f;
    }
    dst[idx] = make_float4(v[0], v[1], v[2], v[3]);
}

// n or m beyond 256 rows: the big-panel layout (gpad_bigpanel.hip), rectangular tile grids
size_t panel_frag_bytes(int n, int m, int /*batch*/) {
    const int T = panel_tiles_for(n, m);
    if (!T) return bigpanel_frag_bytes(n, m);
    return (size_t)2 * T * T * 64 * sizeof(float4);
}

int panel_tiles(int n, int m, int /*batch*/) {
    const int T = panel_tiles_for(n, m);
    if (T) return T;
    return bigpanel_supported(n, m) ? ((n > m ? n : m) + 15) / 16 : 0;
}

hipError_t launch_pack_panel(const float* ML, const float* G, int n, int m, int /*batch*/,
                             float mg_sign, double g_scale, void* frag, hipStream_t s) {
    const int T = panel_tiles_for(n, m);
    if (!T) return bigpanel_supported(n, m) ? launch_pack_bigpanel(ML, G, n, m, mg_sign, g_scale, frag, s)
                                            : hipSuccess;
    float4* pa1 = reinterpret_cast<float4*>(frag);
    float4* pa2 = pa1 + (size_t)T * T * 64;
    const int tot = T * T * 64;
    // A1 = sign * ML (n x m);  A2 = g_scale * G (m x n)
    hipLaunchKernelGGL(pack_panel_kernel, dim3((tot + 255) / 256), dim3(256), 0, s, ML, n, m,
                       (double)mg_sign, T, pa1);
    hipLaunchKernelGGL(pack_panel_kernel, dim3((tot + 255) / 256), dim3(256), 0, s, G, m, n, g_scale, T,
                       pa2);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// the panel kernel: workgroup = panel of 16 instances, wave t = row tile t
// ---------------------------------------------------------------------------------------
// Phased compaction (continuous batching at phase granularity).  A solve with a tolerance is
// cut into phases of iterations [v_begin, v_end).  Within a phase every column runs the same
// global iteration index v, so theta/beta and the test events (v % K == 0) are uniform scalars
// and the per-iteration path has no per-column bookkeeping.  At a phase end the still-running
// instances park their state (z, y in the output arrays, w and u in carry buffers) and append
// their ids to a dense list; the next phase packs only those into panels.  Converged instances
// therefore stop occupying MFMA columns after at most one phase, instead of idling until the
// slowest instance of their static panel finishes.  Columns are independent in the MFMA, so an
// instance's arithmetic does not depend on its column, panel or phase (bit-exact either way).
// A workgroup walks panels grid-stride, so any batch size runs on a resident-sized grid.
#define GPAD_PANEL_RS 0
#define GPAD_PANEL_FK 0
#include "gpad_panel_solve.inc"
#undef GPAD_PANEL_FK
#define GPAD_PANEL_FK 1
#include "gpad_panel_solve.inc"
#undef GPAD_PANEL_FK
#undef GPAD_PANEL_RS
#define GPAD_PANEL_RS 1
#define GPAD_PANEL_FK 0
#include "gpad_panel_solve.inc"
#undef GPAD_PANEL_FK
#undef GPAD_PANEL_RS

// one phase launch of gpad_panel_kernel<T>, T = 1..8 (the phase loop is gpad_phases.cpp's); with fk the
// variant with the infeasibility certificate, with rs (and no fk) the one with the adaptive restart, T = 1..16
hipError_t launch_panel_single(int T, const SolveArgs<float>& a, int grid, hipStream_t s, const FarkasArgs* fk,
                               const RestartArgs* rs) {
    if (rs) {
        if (fk || rs->R < 1 || !rs->count || !rs->pos) return hipErrorInvalidValue;
#define PANEL_CASE(TT) \
    case TT: hipLaunchKernelGGL((gpad_panel_restart_kernel<TT>), dim3(grid), dim3(64 * TT), 0, s, a, *rs); break;
        switch (T) {
            PANEL_CASE(1) PANEL_CASE(2) PANEL_CASE(3) PANEL_CASE(4) PANEL_CASE(5) PANEL_CASE(6) PANEL_CASE(7)
            PANEL_CASE(8) PANEL_CASE(9) PANEL_CASE(10) PANEL_CASE(11) PANEL_CASE(12) PANEL_CASE(13) PANEL_CASE(14)
            PANEL_CASE(15) PANEL_CASE(16)
            default: return hipErrorInvalidValue;
        }
#undef PANEL_CASE
        return hipGetLastError();
    }
    if (fk) {
#define PANEL_CASE(TT) \
    case TT: hipLaunchKernelGGL((gpad_panel_farkas_kernel<TT>), dim3(grid), dim3(64 * TT), 0, s, a, *fk); break;
        switch (T) {
            PANEL_CASE(1) PANEL_CASE(2) PANEL_CASE(3) PANEL_CASE(4) PANEL_CASE(5) PANEL_CASE(6) PANEL_CASE(7)
            PANEL_CASE(8) PANEL_CASE(9) PANEL_CASE(10) PANEL_CASE(11) PANEL_CASE(12) PANEL_CASE(13) PANEL_CASE(14)
            PANEL_CASE(15) PANEL_CASE(16)
            default: return hipErrorInvalidValue;
        }
#undef PANEL_CASE
        return hipGetLastError();
    }
#define PANEL_CASE(TT) \
    case TT: hipLaunchKernelGGL((gpad_panel_kernel<TT>), dim3(grid), dim3(64 * TT), 0, s, a); break;
    switch (T) {
        PANEL_CASE(1) PANEL_CASE(2) PANEL_CASE(3) PANEL_CASE(4)
        PANEL_CASE(5) PANEL_CASE(6) PANEL_CASE(7) PANEL_CASE(8)
        default: return hipErrorInvalidValue;
    }
#undef PANEL_CASE
    return hipGetLastError();
}

}  // namespace gpad
