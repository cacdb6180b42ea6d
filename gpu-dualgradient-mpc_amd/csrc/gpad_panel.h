// gpad_panel.h -- what every f32 MFMA panel unit shares (gfx950):
//   * the fragment layout (below), the vector types and the tile row permutation pi16 -- every unit;
//   * the host-side shape rules: tile count, resident grid, hand-off shapes -- gpad_phases.cpp too;
//   * the Algorithm-1 test, through gpad_panel_test.h (its one text; the f64 panels include that
//     header alone) -- gpad_panel.hip, gpad_loop_panel.hip, gpad_bigpanel.hip, gpad_flatpanel.hip;
//     gpad_pairs.hip keeps its own packed slots;
//   * the iteration of the T-wave panel -- panel_gemm, panel_primal (GEMM 1's epilogue) and
//     panel_dual (GEMM 2's, with the test partials) -- which gpad_panel_kernel (a batch of
//     independent solves, T <= 8) and gpad_loop_panel_kernel (a queue of closed-loop packs) both
//     call: their MFMA chains, epilogues and test are one text and cannot drift apart.
//
// Shared-matrix batches on the f32 MFMA pipe.  When every instance of a batch shares ML and G (one
// plant, many states: the battery scenario batch), the two mat-vecs of a GPAD iteration over 16
// instances are two skinny GEMMs:  Zhat[n x 16] = (-ML) W[m x 16]  and  Y'[m x 16] = G_L Zhat[n x 16].
// One workgroup owns a panel of 16 instances for the whole solve (no inter-workgroup traffic at all).
// Both GEMMs are padded to T tiles of 16 rows (T = ceil(max(n, m)/16)) and the workgroup has
// T waves: wave t owns row tile t of BOTH GEMMs (one 4-register accumulator each), so every
// per-row quantity (z, y, u = G_L z, g_P, p_D) of the panel lives in registers, and W / Zhat
// are exchanged through LDS.  Many waves per SIMD hide the 40-cycle MFMA dependency and
// overlap one wave's epilogue with another wave's MFMAs.
//
// MFMA: v_mfma_f32_16x16x4_f32 (f32 in, f32 accumulate).  Lane l holds A[l&15][k=l>>4],
// B[k=l>>4][l&15] and C/D rows 4(l>>4)+r, column l&15 (r = 0..3).  Its result is bit-for-bit
// a k-ordered fmaf chain, so accumulating k-steps in ascending order reproduces the
// reference's sequential `sum += a*b` exactly (seq_functions.cpp:61,82).
//
// Row permutation pi(rho) = 4(rho&3) + (rho>>2) inside every 16-row tile of the packed A
// operands makes accumulator register r of lane (j = l>>4, c = l&15) hold original row
// 16t + 4r + j -- which is exactly the B-operand fragment of k-step 4t + r of the NEXT GEMM.
// So W and Zhat live in LDS in "fragment order" [tile][lane][4]: a ds_read_b128 per 16-k block
// yields the four B registers, with no transposes and no bank conflicts.
//
// Packed operands in HBM/L2 (built once by pack_panel_kernel at setup; T x T tiles each):
//   PA1[b][t][lane][q] = -ML[16t + pi(lane&15)][16b + 4q + (lane>>4)]   (b < TM, t < TN)
//   PA2[b][t][lane][q] = G_L[16t + pi(lane&15)][16b + 4q + (lane>>4)]   (b < TN, t < TM)
// one float4 per lane per (block, tile): 1 KiB per wave-instruction, fully coalesced.
#pragma once

#include <hip/hip_runtime.h>

#include "gpad_panel_test.h"

namespace gpad {

// ---- host-side shape rules ---------------------------------------------------------------------
constexpr int kPanelMaxTiles = 16;  // n, m <= 256 (1024-thread workgroups)

// T = ceil(max(n, m) / 16) when the T-wave / pair kernels take the shape, else 0
inline int panel_tiles_for(int n, int m) {
    const int t = ((n > m ? n : m) + 15) / 16;
    return t >= 1 && t <= kPanelMaxTiles ? t : 0;
}

// Resident workgroups of a panel grid: a panel-pair workgroup (T > 8) or a big-panel one (T = 0)
// fills a CU; T-wave panels (T <= 8) share one, 32 / T of them.
inline int panel_resident_grid(int T, int num_cus) { return (T < 1 || T > 8) ? num_cus : num_cus * (32 / T); }

// The chain hand-off shapes of the panel pairs (gpad_pairs.h Handoff): T = 9, 11, 13 with full-length
// chains on every tile of both GEMMs, i.e. both dimensions in (16 (T - 1), 16 T].
inline bool panel_handoff_shape(int T, int n, int m) {
    return (T == 9 || T == 11 || T == 13) && n > 16 * (T - 1) && m > 16 * (T - 1) && (n + 15) / 16 == T &&
           (m + 15) / 16 == T;
}

// ---- device pieces -----------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int pi16(int rho) { return 4 * (rho & 3) + (rho >> 2); }

// the 128-bit buffer load's result as the four floats it holds
__device__ __forceinline__ float4 as_float4(u32x4 v) {
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z),
                       __uint_as_float(v.w));
}

// acc = A[tile t] (T k-blocks, streamed from L2 one block ahead) x B (LDS, fragment order).
// The MFMA k-order is ascending (block 0..T-1, step 0..3), i.e. the reference's sequential chain.
// A is read with buffer loads: one 32-bit lane offset (t*1 KiB + lane*16 B) in a VGPR and the
// k-block offset as a compile-time scalar, so the unrolled blocks cost no address registers.
template <int T>
__device__ __forceinline__ f32x4 panel_gemm(__amdgpu_buffer_rsrc_t PA, const float* Bl, int voff,
                                            int lane) {
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    float4 a[2], b[2];
    a[0] = as_float4(__builtin_amdgcn_raw_buffer_load_b128(PA, voff, 0, 0));
    b[0] = *reinterpret_cast<const float4*>(Bl + lane * 4);
#pragma unroll
    for (int kb = 0; kb < T; ++kb) {
        const int cur = kb & 1, nxt = cur ^ 1;
        if (kb + 1 < T) {
            a[nxt] = as_float4(__builtin_amdgcn_raw_buffer_load_b128(PA, voff, (kb + 1) * T * 1024, 0));
            b[nxt] = *reinterpret_cast<const float4*>(Bl + ((kb + 1) * 64 + lane) * 4);
        }
        // the next block's loads issue BEFORE this block's MFMAs (else the scheduler sinks them
        // below and waits on them at once: a full L2 round trip per k-block)
        __builtin_amdgcn_sched_barrier(0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur].x, b[cur].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur].y, b[cur].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur].z, b[cur].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur].w, b[cur].w, acc, 0, 0, 0);
        asm volatile("" ::: "memory");  // keep the prefetch one k-block deep
    }
    return acc;
}

// The two epilogues of the T-wave panel's iteration.  `slot`: this lane's float4 in the [T][64][4]
// LDS tiles; register r of z / y / u <-> row row0 + 4r of the column (row0 = 16t + j).
// GEMM 1 (acc = -ML w): zhat = acc - g_P (8b) into Zh, z = (1-th) z + th zhat (8c)
__device__ __forceinline__ void panel_primal(f32x4 acc, const float4* Gp4, float4* Zh4, int slot, float omt,
                                             float th, bool active, float (&z)[4]) {
    const float4 g4 = Gp4[slot];
    const float gp[4] = {g4.x, g4.y, g4.z, g4.w};
    float zh[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        zh[r] = acc[r] - gp[r];
        const float zn = __builtin_fmaf(omt, z[r], th * zh[r]);
        if (active) z[r] = zn;
    }
    Zh4[slot] = make_float4(zh[0], zh[1], zh[2], zh[3]);
}
// GEMM 2 (acc = G_L zhat): y+ = [w + acc + p_D]+ (8d), the next w (8a) into Wl, the recursion
// u = (1-th) u + th acc; at a test event (chk) the partials of the column's live rows (< m)
// FK: the kernel variant with the infeasibility certificate; at a certificate event (cert) fq gets q
template <bool FK = false>
__device__ __forceinline__ TestPart<float> panel_dual(f32x4 acc, float4* Wl4, const float4* Pd4, int slot,
                                                      float omt, float th, float bn, bool use_tol, bool chk,
                                                      bool active, int row0, int m, float (&y)[4],
                                                      float (&u)[4], bool cert = false, FarkasPart* fq = nullptr) {
    TestPart<float> part;
    const float4 w4 = Wl4[slot];
    const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
    const float4 p4 = Pd4[slot];
    const float pd[4] = {p4.x, p4.y, p4.z, p4.w};
    float wn[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float cv = acc[r];
        const float sv = (wv[r] + pd[r]) + cv;
        const float yp = (__builtin_fabsf(sv) + sv) * 0.5f;
        wn[r] = __builtin_fmaf(bn, yp - y[r], yp);
        if (use_tol) {
            const float un = __builtin_fmaf(omt, u[r], th * cv);
            if (active) u[r] = un;
            if (chk && active && (row0 + 4 * r) < m) part.row(cv, pd[r], wv[r], u[r]);
            if constexpr (FK)
                if (cert && active && (row0 + 4 * r) < m) fq->row(yp, pd[r]);
        }
        if (active) y[r] = yp;
    }
    if (active) Wl4[slot] = make_float4(wn[0], wn[1], wn[2], wn[3]);
    return part;
}

}  // namespace gpad
