// gpad_panel.hip -- shared-matrix batches on the f32 MFMA pipe (gfx950): the fragment packer, the
// size helpers and the T-wave single-panel kernel gpad_panel_kernel<T> (T <= 8).  The fragment
// layout is described in gpad_panel.h; the panel pairs (8 < T <= 16) are gpad_pairs.hip, the phase
// boundary gpad_compact.hip, and the host loop over phases gpad_phases.cpp.
#include <hip/hip_runtime.h>

#include <cmath>

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
template <int T>
__global__ __launch_bounds__(64 * T) void gpad_panel_kernel(SolveArgs<float> a) {
    __shared__ __attribute__((aligned(16))) float Wl[T * 256];  // [T][64][4] w    (B of GEMM 1)
    __shared__ __attribute__((aligned(16))) float Zh[T * 256];  // [T][64][4] zhat (B of GEMM 2)
    // per-lane constants of the current instance, parked in LDS rather than VGPRs:
    // g_P rows and p_D rows of tile t
    __shared__ __attribute__((aligned(16))) float Gp[T * 256];
    __shared__ __attribute__((aligned(16))) float Pd[T * 256];
    __shared__ TestSlot<float> slots[T];

    const int lane = threadIdx.x & 63;
    const int t = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // row tile of this wave
    const int j = lane >> 4, c = lane & 15;
    const int n = a.n, m = a.m, N = a.N, K = a.check_every;
    const int abytes = T * T * 1024;  // one packed operand
    const __amdgpu_buffer_rsrc_t PA1 =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.frag), 0, abytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t PA2 = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)a.frag + abytes), 0, abytes, 0x00020000);
    const int voff = t * 1024 + lane * 16;
    const int slot = t * 64 + lane;  // this lane's float4 in Wl / Zh / Gp / Pd
    float4* Wl4 = reinterpret_cast<float4*>(Wl);
    float4* Zh4 = reinterpret_cast<float4*>(Zh);
    float4* Gp4 = reinterpret_cast<float4*>(Gp);
    float4* Pd4 = reinterpret_cast<float4*>(Pd);
    const bool use_tol = a.tol > 0.0;
    const bool fresh = a.v_begin == 0;      // first phase: start from the caller's z0, y0
    const bool carry = a.v_end < N;         // not the last phase: park the survivors
    const int count = a.count_in ? __builtin_amdgcn_readfirstlane(*a.count_in) : a.batch;
    if (a.count_in && count <= a.fin_thresh) return;  // the resident finisher has them
    const int panels = (count + 15) / 16;

    for (int p = blockIdx.x; p < panels; p += gridDim.x) {
        // ---- load the panel: column c <-> instance idx[16p + c] -------------------------
        const int k = 16 * p + c;
        bool active = k < count;
        const int inst = active ? (a.idx_in ? a.idx_in[k] : k) : 0;
        // register r <-> row 16t + 4r + j of the column's instance
        float z[4], y[4], u[4];
        {
            float gp[4], pd[4], w[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * t + 4 * r + j;
                const bool okn = active && i < n, okm = active && i < m;
                z[r] = okn ? a.z[(size_t)inst * n + i] : 0.0f;
                gp[r] = okn ? a.gP[(size_t)inst * a.ld_gP + i] : 0.0f;
                y[r] = okm ? a.y[(size_t)inst * m + i] : 0.0f;
                pd[r] = okm ? (float)(a.gscale * (double)a.g[(size_t)inst * a.ld_g + i]) : 0.0f;
                if (fresh) {  // w_0 = y_0 + beta_0 (y_0 - y_{-1}), y_{-1} = y_0; u set below
                    w[r] = __builtin_fmaf(a.beta[0], y[r] - y[r], y[r]);
                    u[r] = 0.0f;
                } else {
                    w[r] = okm ? a.wc[(size_t)inst * m + i] : 0.0f;
                    u[r] = okm && use_tol ? a.uc[(size_t)inst * m + i] : 0.0f;
                }
            }
            Gp4[slot] = make_float4(gp[0], gp[1], gp[2], gp[3]);
            Pd4[slot] = make_float4(pd[0], pd[1], pd[2], pd[3]);
            Wl4[slot] = make_float4(w[0], w[1], w[2], w[3]);
        }
        if (fresh && use_tol) {  // u = G_L z_{-1} (one GEMM for the panel); then the 8c recursion
            Zh4[slot] = make_float4(z[0], z[1], z[2], z[3]);
            __syncthreads();
            const f32x4 cz = panel_gemm<T>(PA2, Zh, voff, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) u[r] = cz[r];
        }
        __syncthreads();

        int v = a.v_begin;
        float th = a.theta[v], bn = a.beta[v + 1];
        while (true) {
            // schedule prefetched one iteration ahead (tables hold N + 2 entries)
            const float th_next = a.theta[v + 1], bn_next = a.beta[v + 2];
            ++v;
            const bool chk = use_tol && (v % K) == 0;  // uniform: every column is at iteration v
            const float omt = 1.0f - th;
            // ---- GEMM 1 + epilogue: zhat = -ML w - g_P (8b), z = (1-th) z + th zhat (8c) ----
            panel_primal(panel_gemm<T>(PA1, Wl, voff, lane), Gp4, Zh4, slot, omt, th, active, z);
            __syncthreads();
            // ---- GEMM 2 + epilogue: y+ = [w + G_L zhat + p_D]+ (8d), next w (8a) ----------
            TestPart<float> part = panel_dual(panel_gemm<T>(PA2, Zh, voff, lane), Wl4, Pd4, slot, omt, th, bn,
                                              use_tol, chk, active, 16 * t + j, m, y, u);
            th = th_next;
            bn = bn_next;
            __syncthreads();
            if (!chk && v < a.v_end) continue;

            // ---- Algorithm 1 test, per column: lane groups j, then row tiles through LDS ----
            int code = 0;
            bool zh_out = true;  // this iteration's zhat still in Zh (no verification GEMM ran)
            if (chk) {
                part.fold();
                part.put(slots[t], c, j == 0);
                __syncthreads();
                int st1 = 0;
                if (active) st1 = stage1<float, T>(slots, 0, T, c, a.L, a.tol, a.tol_gap).bits;
                bool ver = false;
                if (__syncthreads_or(st1 & 1)) {  // (A) nominated somewhere: G_L z for the panel
                    zh_out = false;
                    if (st1 & 2) {  // test (B)'s result (zhat) out now: Zh is about to hold z
                        const float4 h4 = Zh4[slot];
                        const float zh[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int i = 16 * t + 4 * r + j;
                            if (i < n) a.z[(size_t)inst * n + i] = zh[r];
                        }
                    }
                    Zh4[slot] = make_float4(z[0], z[1], z[2], z[3]);
                    __syncthreads();
                    const f32x4 cz = panel_gemm<T>(PA2, Zh, voff, lane);
                    const float4 p4 = Pd4[slot];
                    const float pd[4] = {p4.x, p4.y, p4.z, p4.w};
                    VerPart<float> vp;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if ((st1 & 1) && (16 * t + 4 * r + j) < m) {
                            u[r] = cz[r];  // the recursion restarts from the direct value
                            vp.row(cz[r], pd[r]);
                        }
                    }
                    vp.fold();
                    vp.put(slots[t], c, j == 0);
                    __syncthreads();
                    if (st1 & 1) ver = verified<float, T>(slots, 0, T, c, a.L, a.tol);
                }
                code = check_code(st1, ver);
            }
            // ---- finished columns: results out ---------------------------------------------
            if (active && (code != 0 || v >= N)) {
                const float4 h4 = Zh4[slot];  // this iteration's zhat (own slot), unless verified over
                const float zh[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * t + 4 * r + j;
                    if (i < n && (code != 2 || zh_out)) a.z[(size_t)inst * n + i] = code == 2 ? zh[r] : z[r];
                    if (i < m) a.y[(size_t)inst * m + i] = y[r];
                }
                if (t == 0 && j == 0) {
                    a.iters[inst] = v;
                    a.conv[inst] = code;
                }
                active = false;
            }
            if (v >= a.v_end || !__syncthreads_or(active ? 1 : 0)) break;
        }
        // ---- phase end: park the survivors for the next phase ------------------------------
        if (carry) {
            const bool park = active && v >= a.v_end;
            if (park) {
                const float4 w4 = Wl4[slot];  // w of iteration v (own slot)
                const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * t + 4 * r + j;
                    if (i < n) a.z[(size_t)inst * n + i] = z[r];
                    if (i < m) {
                        a.y[(size_t)inst * m + i] = y[r];
                        a.wc[(size_t)inst * m + i] = wv[r];
                        if (use_tol) a.uc[(size_t)inst * m + i] = u[r];
                    }
                }
            }
            if (t == 0) list_survivors(a, p, park, inst, lane, j);  // lanes 0..15 speak for the columns
        }
        __syncthreads();  // the next panel reuses the LDS tiles
    }
}

// one phase launch of gpad_panel_kernel<T>, T = 1..8 (the phase loop is gpad_phases.cpp's)
hipError_t launch_panel_single(int T, const SolveArgs<float>& a, int grid, hipStream_t s) {
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
