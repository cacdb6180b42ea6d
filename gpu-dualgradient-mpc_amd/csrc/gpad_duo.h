// gpad_duo.h -- the slot state and the half-steps of the two-instance ping-pong kernels, shared by
// gpad_duo.hip (gpad_duo_kernel: a queue of independent instances) and gpad_loop.hip
// (gpad_loop_kernel: a queue of closed-loop packs).  Both kernels run exactly these functions per
// iteration, so their counts and results cannot drift apart.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "gpad_chain.h"
#include "gpad_internal.h"

namespace gpad {

struct DuoSlot {  // one instance slot; bookkeeping is uniform, the floats are this lane's rows
    int pos, vs, nextp;  // list position (>= count: empty), iterations done, pre-claimed next
    int kc;              // 8d steps to the next test: the test runs at iteration vs + 1 when kc == 1
    bool need8d;         // 8b done, 8d pending
    float th, bn;        // theta_vs, beta_{vs+1}: loaded one step before their use (a deeper
                         // prefetch, or g_P / p_D in registers instead of LDS, spills: the rows
                         // take 200 of the 256 VGPRs -- profiles/r03_duo_solo.txt)
    float x0, x1, x2;    // -ML lanes: z, zhat, -;  G/L lanes: y, w, u = G_L z (g_P, p_D in LDS)
};
struct DuoCtx {
    int tid, count, G, v0, n, m, N, Kc, kc0, nA, nwaves, row, claim_base, b0;  // b0: first G/L wave
    bool fresh, use_tol, isA, live;
#ifdef GPAD_STAMP
    int step;  // steps taken (stamps)
#endif
};

// The schedule through the constant address space: the index is uniform, so theta / beta arrive by
// scalar loads into SGPRs (four fewer VGPRs next to the 200 register-resident matrix entries;
// the time per step is the same as with vector loads, profiles/r03_duo_solo.txt "duo3").
__device__ __forceinline__ float sched(const float* t, int v) {
    return ((const __attribute__((address_space(4))) float*)(t))[v];
}

// An instance's row vectors through buffer operations: the base (instance row b of a [batch][ld]
// array) is uniform and lives in SGPRs, the lane's offset is one 32-bit VGPR (4 row), so a refill
// holds no per-lane 64-bit pointers (six of them, hoisted out of the loop, were spilled to scratch).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const void* base, size_t b, int ld) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(static_cast<const char*>(base) + 4 * b * (size_t)ld),
                                             0, 4 * ld, 0x00020000);
}
__device__ __forceinline__ float row_ld(const void* base, size_t b, int ld, int off4) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(row_rsrc(base, b, ld), off4, 0, 0));
}
__device__ __forceinline__ void row_st(void* base, size_t b, int ld, int off4, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), row_rsrc(base, b, ld), off4, 0, 0);
}

// Step anatomy stamps: gpad_duo.hip defines GPAD_DSTAMP before this header in its diagnostic
// builds (-DGPAD_STAMP); everywhere else the stamp points are empty.
#ifndef GPAD_DSTAMP
#define GPAD_DSTAMP(P) \
    do {               \
    } while (0)
#endif

// The half-steps (every wave calls the one of its role; control flow uniform per role).
// 8b + 8c of slot sa on the -ML waves: zhat to the slot's LDS vector, z updated.
template <int KA, int K>
__device__ __forceinline__ void duo_half_a(const DuoCtx& c, DuoSlot& sa, const float* wa_l, float* zha_l,
                                           const float* gpa_l, const float (&r)[K]) {
    const float th = sa.th;
    const float gpv = gpa_l[c.row];  // read before the chain: its LDS latency hides there
    const float acc = chain_regs<KA, K>(r, wa_l);
    GPAD_DSTAMP(1);
    if (c.live) {
        const float zhv = acc - gpv;
        sa.x0 = __builtin_fmaf(1.0f - th, sa.x0, th * zhv);
        zha_l[c.row] = zhv;
        sa.x1 = zhv;
    }
}

// 8d + 8a (+ the test partials when chk) of slot sb on the G/L waves: w to the slot's LDS vector.
template <int KB, int K>
__device__ __forceinline__ void duo_half_b(const DuoCtx& c, DuoSlot& sb, bool chk, const float* zhb_l, float* wb_l,
                                           const float* pdb_l, CheckSlot* slots_b, const float (&r)[K]) {
    TestRows<float> tp;
    const float th = sb.th, bn = sb.bn;
    const float pdv = pdb_l[c.row];  // (before the chain, as gpv)
    const float cv = chain_regs<KB, K>(r, zhb_l);
    GPAD_DSTAMP(1);
    if (c.live) {
        const float wi = sb.x1;
        if (c.use_tol) sb.x2 = row_u(th, sb.x2, cv);
        if (chk) tp.only_row(cv, pdv, wi, sb.x2);
        const RowStep<float> nx = row_step_dense(cv, wi, pdv, sb.x0, bn);
        sb.x1 = nx.w;
        sb.x0 = nx.y;
        wb_l[c.row] = sb.x1;
    }
    if (chk) tp.publish(slots_b);
}

// after the barrier that closes slot sb's 8d half (every wave): iteration count, schedule and the
// test's decision.  Returns the termination code (0: continue, 1: test (A), 2: test (B), which
// certifies zhat = sb.x1 of the -ML lanes); sb.vs is the iteration count.  The caller ends the
// instance when the code is non-zero or sb.vs >= c.N.
// PRE: the schedule of the next iteration was fetched ahead (th_n, bn_n; duo_solo), else it is
// loaded here
template <int KB, int K, bool PRE = false>
__device__ __forceinline__ int duo_test_b(const SolveArgs<float>& a, const DuoCtx& c, DuoSlot& sb, bool chk,
                                          float* pdb_l, CheckSlot* slots_b, CheckSlot* vslots, float* z_l,
                                          const float (&r)[K], float th_n = 0.0f, float bn_n = 0.0f) {
    sb.need8d = false;
    sb.kc = chk ? c.Kc : sb.kc - 1;
    const int v = ++sb.vs;
    if constexpr (PRE) {
        sb.th = th_n;
        sb.bn = bn_n;
    } else {
        sb.th = sched(a.theta, v);  // next iteration's schedule (tables hold N + 2 entries)
        sb.bn = sched(a.beta, v + 1);
    }
    int done = 0;
    if (chk) {
        const int st1 = check_stage1<float>(slots_b + c.b0, c.nwaves - c.nA, a.L, a.tol, a.tol_gap);
        bool verified = false;
        if (st1 & 1) {  // (A) nominated: decide on the direct chain G_L z, reset u to it
            if (c.isA && c.live) z_l[c.row] = sb.x0;
            __syncthreads();
            // (VerRows::row / publish of the lane's one row, written out: through the struct 13 register-
            // bound gpad_loop_fleet_kernel instantiations spill 8 more bytes, r19_row_test_isa.txt)
            float vc = -INFINITY, mc = 0.0f;
            if (!c.isA) {
                const float cz = chain_regs<KB, K>(r, z_l);
                if (c.live) {
                    sb.x2 = cz;
                    vc = cz + pdb_l[c.row];
                    mc = __builtin_fabsf(cz) + __builtin_fabsf(pdb_l[c.row]);
                }
                check_publish<float>(vslots, vc, vc, vc, 0.0, mc);
            }
            __syncthreads();
            verified = check_verify<float>(vslots + c.b0, c.nwaves - c.nA, a.L, a.tol);
        }
        done = check_code(st1, verified);
    }
    return done;
}

}  // namespace gpad
