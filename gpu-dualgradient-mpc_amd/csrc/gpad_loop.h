// gpad_loop.h -- the asynchronous closed-loop kernels (GPAD_OPT_LOOP_ASYNC, gpad_closed_loop):
// gpad_duo_kernel's two-slot ping-pong over a queue of closed-loop PACKS instead of single solves, and
// its one-slot variant for fleets of distinct plants.  Templates only: gpad_loop.hip,
// gpad_loop_plant.hip and gpad_loop_fleet.hip each instantiate one LoopMode's 64 buckets, so the
// three compile side by side (one file took as long as the rest of the library together).
// gpad_loop_farkas.hip, gpad_loop_plant_farkas.hip and gpad_loop_fleet_farkas.hip do the same for the
// variants with the infeasibility certificate (gpad_farkas.h, gpad_infeasibility_loop_async).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "gpad_chain.h"
#include "gpad_duo.h"
#include "gpad_farkas.h"
#include "gpad_internal.h"

namespace gpad {

// =========================================================================================
// gpad_loop_kernel: one launch for a whole T-step closed loop, every pack stepping on its own.
// =========================================================================================
// The lockstep loop (gpad_host.cpp state_typed) enqueues per MPC step the two affine maps, the
// solve, the |g| maxima and the plant update, and with a tolerance every step lasts as long as its
// slowest pack.  A pack's next step depends on its own z* only (gpad.m:91-93), so here a slot holds
// (pack b, MPC step t, state x_t) and, when its solve terminates, advances the SAME pack: the plant
// update and the affine maps g_P(x), g(x) are evaluated in place by the workgroup (x in LDS, the P,
// A, B rows through uniform-base buffer loads), and the slot restarts at iteration 0 of step t + 1.
// Only after its last step is the slot refilled from the queue, exactly as the duo kernel claims
// instances.  No workgroup waits for another: every loop is bounded by N, by `steps` and by the
// finite queue.
//
// Per iteration the arithmetic is gpad_duo.h's half-steps and test, i.e. the duo / resident
// kernels'; the step boundary restates affine2_kernel and plant_step_kernel (gpad_plant.hip) in
// their order with explicit fmas.  Results, counts and codes are therefore bit-identical to the
// lockstep loop.
//
// Exogenous signals (LoopArgs::ns, S; gpad_setup_signals): the state row of a slot is [x_t; S[t][pack]],
// the maps are the packed images [PM SM], [Pg Sg], [A E] with rows of nx + ns columns, and the same
// chains run over nx + ns columns -- today's binding on the augmented state.  The signal lanes
// (nx <= tid < nx + ns) load their words at the start of every step (loop_start), for a refill and
// for a pack's next step alike; nothing of S or ns is held across the solve loop.
//
// Per-pack plant maps (LoopArgs::per_plant, gpad_setup_plant_batch): a slot reads the P, A, B rows of
// its own pack -- the instance index of row_ld, 0 for one shared plant.  Per-pack matrices
// (SolveArgs::strideA/strideB != 0, a fleet of distinct plants) run gpad_loop_fleet_kernel below.
struct LoopSlot : DuoSlot {
    int t;  // MPC step of the pack in this slot (uniform)
};
// the slot of a certificate variant.  A type of its own: with the countdown as a member of LoopSlot, unused as
// it is there, every gpad_loop_kernel instantiation orders a block of register copies differently
struct LoopSlotFk : LoopSlot {
    int kf;  // tests to the next certificate event (uniform): cert <=> (vs + 1) % (4 Kc) == 0
};
template <bool FK>
using LoopSlotOf = std::conditional_t<FK, LoopSlotFk, LoopSlot>;

typedef const __attribute__((address_space(4))) LoopArgs LoopKernArgs;
// the kernel's LoopArgs read afresh from its kernarg segment (as kargs(): nothing kept live in
// SGPRs across the solve loop); its first member is the SolveArgs the shared half-steps take
__device__ __forceinline__ LoopKernArgs& largs() {
    LoopKernArgs* p = (LoopKernArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *p;
}
// the FarkasArgs of a certificate variant: the kernel's second parameter, behind the LoopArgs
typedef const __attribute__((address_space(4))) FarkasArgs LoopFarkasKernArgs;
__device__ __forceinline__ LoopFarkasKernArgs& lfargs() {
    static_assert(alignof(FarkasArgs) == 8 && sizeof(LoopArgs) % 8 == 0, "FarkasArgs directly behind LoopArgs");
    const __attribute__((address_space(4))) char* p =
        (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(LoopFarkasKernArgs*)(p + sizeof(LoopArgs));
}

// LDS of the step boundaries
struct LoopLds {
    float x[2][2][64];   // per slot: [x_t; s_t] at [t & 1] (s_t = S[t][pack], gpad_setup_signals; nx + ns
                         // <= 64), x_{t+1} written to the other half
    float u[64];         // u = z*[0:nu] of the slot at its boundary
    float gm[kResidentMaxThreads];  // per lane: NaN-keeping max |g| of every g row it formed
};

// c + P x for this lane's row of copy `pi` of a [rows][nx] map (affine2_kernel's order): acc =
// c0[row] (0 if absent), then fma(P[row][k], x[k], acc) for ascending k
__device__ __forceinline__ float loop_affine(const float* P, const float* c0, size_t pi, int rows, int row, int nx,
                                             const float* x_l) {
    float acc = c0 ? row_ld(c0, pi, rows, 4 * row) : 0.0f;
    const int o4 = 4 * row * nx;
#pragma unroll 1
    for (int k = 0; k < nx; ++k) acc = __builtin_fmaf(row_ld(P, pi, rows * nx, o4 + 4 * k), x_l[k], acc);
    return acc;
}

// Lane tid in [nx, nx + ns) reads word tid - nx of row `row` of the signals S ([rows][ns]): the row's
// descriptor starts nx words early, so the lane's offset is the 4 tid its state accesses already hold
// (no per-lane subtraction); lanes below nx must not call (their words lie before the row).
__device__ __forceinline__ float loop_sig_ld(const float* S, size_t row, int ns, int nx, int tid4) {
    const char* base = reinterpret_cast<const char*>(S) + 4 * (row * (size_t)ns) - 4 * (size_t)nx;
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
        __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(base), 0, 4 * (nx + ns), 0x00020000), tid4, 0, 0));
}

// What a kernel is compiled for.  The shared-plant two-slot kernel is at its register budget (an
// index multiply more costs it a VGPR in every bucket), so the plant index is a compile-time choice
// there; the fleet kernel, with one slot, reads the flag at run time.
enum LoopMode { kLoopShared = 0, kLoopPerPlant = 1, kLoopFleet = 2 };

// the copy of the plant maps pack `pos` reads
template <int MODE>
__device__ __forceinline__ size_t loop_plant_of(LoopKernArgs& A, int pos) {
    if constexpr (MODE == kLoopShared) return 0;
    if constexpr (MODE == kLoopPerPlant) return (size_t)pos;
    return A.per_plant ? (size_t)pos : 0;
}

// This lane's matrix rows of pack p into its registers, as the kernels' prologues load them, from the
// pack's own k-major images (fleet kernel).  The wave's role is uniform, so the image is addressed
// through one buffer descriptor of exactly its m * ldn (n * ldm) words.
template <int K>
__device__ __forceinline__ void loop_rows(const DuoCtx& c, int p, float (&r)[K]) {
    LoopKernArgs& A = largs();
    const bool ua = __builtin_amdgcn_readfirstlane((int)c.isA) != 0;
    const float* Mt = ua ? A.s.MGt : A.s.GLt;
    const int len = ua ? c.m : c.n, ld = ua ? A.s.ldn : A.s.ldm;
    const int o4 = 4 * c.row;
#pragma unroll
    for (int k0 = 0; k0 < K; k0 += 8) {  // eight loads in flight: more would spill next to K live rows
#pragma unroll
        for (int k = k0; k < k0 + 8 && k < K; ++k) {
            // (k >= len reads row 0 and drops it: a live lane's word is always inside the image)
            const float v = row_ld(Mt, (size_t)p, len * ld, o4 + 4 * (k < len ? k : 0) * ld);
            r[k] = (c.live && k < len) ? v : 0.0f;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Start the solve of slot s at state x_l (barrier-published by the caller) from (z_{-1}, y_0) = v0
// of this lane's row: g_P(x) / p_D(x) to the slot's LDS rows, then the fresh path of duo_refill.
// Uniform, contains barriers.  FK: a certificate variant (the slot's event countdown starts over).
template <int KB, int K, int MODE, bool FK = false>
__device__ __forceinline__ void loop_start(const SolveArgs<float>& a, const DuoCtx& c, LoopSlotOf<FK>& s, float v0,
                                           float* x_l, float* w_l, float* gp_l, float* pd_l, float* z_l,
                                           float* gm_l, const float (&r)[K]) {
    s.vs = 0;
    s.kc = c.Kc;
    if constexpr (FK) s.kf = 4;
    s.need8d = false;
    s.th = sched(a.theta, 0);
    s.bn = sched(a.beta, 1);
    s.x0 = s.x1 = s.x2 = 0.0f;
    if (largs().ns) {  // the step's signals beside its state: x_l = [x_t; S[t][pack]]
        LoopKernArgs& A = largs();
        if (c.tid >= A.nx && c.tid < A.nx + A.ns)
            x_l[c.tid] = loop_sig_ld(A.S, (size_t)s.t * (size_t)c.count + (size_t)s.pos, A.ns, A.nx, 4 * c.tid);
        __syncthreads();
    }
    if (c.live) {
        LoopKernArgs& A = largs();
        if (c.isA) {
            gp_l[c.row] = loop_affine(A.PM, A.M0, loop_plant_of<MODE>(A, s.pos), c.n, c.row, A.nx + A.ns, x_l);
            s.x0 = v0;
            if (c.use_tol) z_l[c.row] = v0;
        } else {
            const float gv = loop_affine(A.Pg, A.g0, loop_plant_of<MODE>(A, s.pos), c.m, c.row, A.nx + A.ns, x_l);
            gm_l[c.tid] = absmax_nan(gm_l[c.tid], gv);
            pd_l[c.row] = (float)(A.s.gscale * (double)gv);
            s.x0 = v0;
            s.x1 = __builtin_fmaf(A.s.beta[0], v0 - v0, v0);
            w_l[c.row] = s.x1;
        }
    }
    __syncthreads();
    if (c.use_tol) {  // u = G_L z_{-1}, then the 8c recursion
        if (!c.isA) {
            const float us = chain_regs<KB, K>(r, z_l);
            s.x2 = c.live ? us : 0.0f;
        }
        __syncthreads();  // z_l free again
    }
}

// slot s takes pack p at its step 0 (empty if p >= count): x from the input states, (z, y) from the
// caller's arrays when warm, else zero.  FLEET: the pack brings its own matrices, the rows r are
// reloaded and stay for its `steps` steps.  Uniform, contains barriers.
template <int KB, int K, int MODE, bool FK = false>
__device__ __forceinline__ void loop_refill(const SolveArgs<float>& a, const DuoCtx& c, LoopSlotOf<FK>& s, int p,
                                            float* x_s, float* w_l, float* gp_l, float* pd_l, float* z_l,
                                            float* gm_l, float (&r)[K]) {
    s.pos = __builtin_amdgcn_readfirstlane(p);
    s.t = 0;
    const bool has = p < c.count;
    float v0 = 0.0f;
    if (has) {
        LoopKernArgs& A = largs();
        if constexpr (MODE == kLoopFleet) loop_rows<K>(c, s.pos, r);
        if (c.tid < A.nx) x_s[c.tid] = row_ld(A.x_in, (size_t)p, A.nx, 4 * c.tid);
        if (A.warm && c.live)
            v0 = c.isA ? row_ld(A.s.z, (size_t)p, c.n, 4 * c.row) : row_ld(A.s.y, (size_t)p, c.m, 4 * c.row);
    }
    __syncthreads();  // x_s (and the claim cell, loop_claim) published
    if (has) {
        loop_start<KB, K, MODE, FK>(a, c, s, v0, x_s, w_l, gp_l, pd_l, z_l, gm_l, r);
    } else {
        s.vs = 0;
        s.kc = c.Kc;
        if constexpr (FK) s.kf = 4;
        s.need8d = false;
        s.th = s.bn = 0.0f;
        s.x0 = s.x1 = s.x2 = 0.0f;
    }
}

// consume the pre-claimed position of slot s, claim its next one (claim_l: this slot's cell)
template <int KB, int K, int MODE, bool FK = false>
__device__ __forceinline__ void loop_claim(const SolveArgs<float>& a, const DuoCtx& c, LoopSlotOf<FK>& s, int* claim_l,
                                           float* x_s, float* w_l, float* gp_l, float* pd_l, float* z_l,
                                           float* gm_l, float (&r)[K]) {
    const int p = s.nextp;
    if (c.tid == 0 && p < c.count) *claim_l = c.claim_base + atomicAdd(a.qctr, 1);
    loop_refill<KB, K, MODE, FK>(a, c, s, p, x_s, w_l, gp_l, pd_l, z_l, gm_l, r);  // (its barrier publishes *claim_l)
    s.nextp = p < c.count ? __builtin_amdgcn_readfirstlane(*claim_l) : c.count;
}

// A certificate event of slot sb (gpad_farkas.h; certificate variants only), after Algorithm 1 found no
// code at a test with (vs + 1) % (4 check_every) == 0: the G/L lanes publish y+ = sb.x0 and reduce
// q = sum y+ pD as gpad_resident_farkas_kernel does (the wave butterfly, then the G/L waves' partials in
// wave order); q > 0 nominates and farkas_decide -- the stream kernel's text, on the pack's k-major G_L
// image in global memory, not on the row registers -- decides.  Returns kCodeInfeasible or 0.  The
// scratch is one set per workgroup, shared by both slots as vslots and z_l are.  Uniform, contains
// barriers; rare, so it keeps nothing in registers across the solve loop.
template <int KA, int KB>
__device__ __forceinline__ int loop_farkas(const DuoCtx& c, const LoopSlotFk& sb, const float* pdb_l) {
    __shared__ float yf_l[KA];
    __shared__ double fq_l[kResidentMaxThreads / 64], ft_l[KB];
    if (!c.isA) {
        double fq = 0.0;  // this row's term of q
        if (c.live) {
            yf_l[c.row] = sb.x0;
            fq = (double)sb.x0 * (double)pdb_l[c.row];
        }
        fq = wave_sum(fq);
        if ((c.tid & 63) == 0) fq_l[c.tid >> 6] = fq;
    }
    __syncthreads();
    double q = 0.0;
    for (int i = 0; i < c.nwaves - c.nA; ++i) q += fq_l[c.b0 + i];
    if (!(q > 0.0)) return 0;  // (uniform: every thread summed the same words)
    LoopKernArgs& A = largs();
    LoopFarkasKernArgs& fk = lfargs();
    const size_t b = (size_t)sb.pos;
    return farkas_decide<float>(A.s.GLt + b * A.s.strideB, A.s.ldm, c.n, c.m, yf_l, pdb_l, fk.rabs + b * fk.stride,
                                fk.R, q, ft_l)
               ? kCodeInfeasible
               : 0;
}

// after the barrier that closes slot sb's 8d half (every wave): the shared test, and when the solve
// terminates the step boundary -- record the step, x_{t+1} = A x_t + B u, then either the pack's
// next step in place or, after its last step, the results out and the next pack from the queue.
// x_b: this slot's two x vectors; u_l: boundary scratch.  FKA: the KA of a certificate variant (0:
// none), which holds a certificate event after every fourth test of a solve; its code 5 ends the solve
// as the cap does (z* = z, y* = y+).
template <int KB, int K, int MODE, bool PRE = false, int FKA = 0>
__device__ __forceinline__ void loop_post_b(const SolveArgs<float>& a, const DuoCtx& c, LoopSlotOf<FKA != 0>& sb,
                                            bool chk, float* wb_l, float* gpb_l, float* pdb_l, CheckSlot* slots_b,
                                            CheckSlot* vslots, int* claim_b, float* z_l, float* x_b, float* u_l,
                                            float* gm_l, float (&r)[K], float th_n = 0.0f,
                                            float bn_n = 0.0f) {
    int done = duo_test_b<KB, K, PRE>(a, c, sb, chk, pdb_l, slots_b, vslots, z_l, r, th_n, bn_n);
    if constexpr (FKA != 0) {
        if (chk) {
            const bool cert = sb.kf == 1;
            sb.kf = cert ? 4 : sb.kf - 1;
            if (cert && !done) done = loop_farkas<FKA, KB>(c, sb, pdb_l);  // Algorithm 1 first: any code of its wins
        }
    }
    const int v = sb.vs;
    if (done || v >= c.N) {
        LoopKernArgs& A = largs();
        const int t = sb.t, nx = A.nx, nu = A.nu;
        const size_t b = (size_t)sb.pos;
        const size_t tb = (size_t)t * (size_t)c.count + b;  // (step, pack) row of xs / us
        const size_t pi = loop_plant_of<MODE>(A, sb.pos);
        const bool last = t + 1 == A.steps;
        // z* (-ML lanes; (B) certifies zhat) or y* (G/L lanes) of this lane's row
        const float star = c.isA ? (done == 2 ? sb.x1 : sb.x0) : sb.x0;
        const float* xc = x_b + 64 * (t & 1);
        float* xn = x_b + 64 * ((t + 1) & 1);
        if (c.tid == 0) {  // the counters of step t: [iters[batch] | conv[batch]]
            A.s.iters[(size_t)(2 * t) * c.count + b] = v;
            A.s.conv[(size_t)(2 * t + 1) * c.count + b] = done;
        }
        if (c.isA && c.row < nu) {
            u_l[c.row] = star;
            if (A.us) row_st(A.us, tb, nu, 4 * c.row, star);
        }
        if (c.tid < nx && A.xs) row_st(A.xs, tb, nx, 4 * c.tid, xc[c.tid]);
        __syncthreads();  // u_l published
        if (c.tid < nx) {  // plant_step_kernel's order: A x (then E s_t: the row is [A E]), then B u, one fma chain
            float acc = 0.0f;
            const int nxa = nx + A.ns;
            const int oa = 4 * c.tid * nxa, ob = 4 * c.tid * nu;
#pragma unroll 1
            for (int k = 0; k < nxa; ++k) acc = __builtin_fmaf(row_ld(A.A, pi, nx * nxa, oa + 4 * k), xc[k], acc);
#pragma unroll 1
            for (int j = 0; j < nu; ++j) acc = __builtin_fmaf(row_ld(A.B, pi, nx * nu, ob + 4 * j), u_l[j], acc);
            xn[c.tid] = acc;
            if (last) row_st(A.x_out, b, nx, 4 * c.tid, acc);
        }
        if (last && c.live) {
            if (c.isA) row_st(A.s.z, b, c.n, 4 * c.row, star);
            else row_st(A.s.y, b, c.m, 4 * c.row, star);
        }
        __syncthreads();  // xn published; xc and u_l free
        if (last) {
            loop_claim<KB, K, MODE, FKA != 0>(a, c, sb, claim_b, x_b, wb_l, gpb_l, pdb_l, z_l, gm_l, r);
        } else {
            sb.t = t + 1;  // cold: z = y = 0 (acceldualgrad.m:16-17); warm: z_{-1} = z*, y_0 = y*
            loop_start<KB, K, MODE, FKA != 0>(a, c, sb, A.warm ? star : 0.0f, xn, wb_l, gpb_l, pdb_l, z_l, gm_l, r);
        }
    }
}

// one step: -ML waves run 8b+8c of slot sa, G/L waves 8d+8a (+ test) of slot sb (as duo_step)
template <int KA, int KB, int K, int MODE, int FKA = 0>
__device__ __forceinline__ void loop_step(const SolveArgs<float>& a, const DuoCtx& c, LoopSlotOf<FKA != 0>& sa,
                                          LoopSlotOf<FKA != 0>& sb, float* wa_l, float* zha_l,
                                          const float* gpa_l, float* wb_l,
                                          const float* zhb_l, float* gpb_l, float* pdb_l, CheckSlot* slots_b,
                                          CheckSlot* vslots, int* claim_b, float* z_l, float* x_b, float* u_l,
                                          float* gm_l, float (&r)[K]) {
    const bool runA = sa.pos < c.count && !sa.need8d;
    const bool runB = sb.need8d;
    const bool chk = runB && c.use_tol && sb.kc == 1;  // ((vs + 1) % Kc == 0, as a countdown)
    if (c.isA) {
        if (runA) duo_half_a<KA, K>(c, sa, wa_l, zha_l, gpa_l, r);
    } else {
        if (runB) duo_half_b<KB, K>(c, sb, chk, zhb_l, wb_l, pdb_l, slots_b, r);
    }
    __syncthreads();
    if (runA) sa.need8d = true;
    if (runB)
        loop_post_b<KB, K, MODE, false, FKA>(a, c, sb, chk, wb_l, gpb_l, pdb_l, slots_b, vslots, claim_b, z_l, x_b, u_l,
                                             gm_l, r);
}

// One live slot left, the queue drained: the resident kernel's loop on it (as duo_solo; with at
// most one pack per workgroup this is the whole run; the fleet kernel's only loop)
template <int KA, int KB, int K, int MODE, int FKA = 0>
__device__ __forceinline__ void loop_solo(const SolveArgs<float>& a, const DuoCtx& c, LoopSlotOf<FKA != 0>& s,
                                          float* w_l, float* zh_l, float* gp_l, float* pd_l, CheckSlot* slots,
                                          CheckSlot* vslots, int* claim, float* z_l, float* x_s, float* u_l,
                                          float* gm_l, float (&r)[K]) {
    float th_n = a.theta[s.vs + 1], bn_n = a.beta[s.vs + 2];
    while (s.pos < c.count) {
        if (!s.need8d) {  // (a slot that enters after its 8b half starts at 8d)
            if (c.isA) {
                duo_half_a<KA, K>(c, s, w_l, zh_l, gp_l, r);
            } else {
                th_n = a.theta[s.vs + 1];
                bn_n = a.beta[s.vs + 2];
            }
            __syncthreads();
        }
        const bool chk = c.use_tol && s.kc == 1;
        if (!c.isA) {
            duo_half_b<KB, K>(c, s, chk, zh_l, w_l, pd_l, slots, r);
        } else {
            th_n = a.theta[s.vs + 1];
            bn_n = a.beta[s.vs + 2];
        }
        __syncthreads();
        loop_post_b<KB, K, MODE, true, FKA>(a, c, s, chk, w_l, gp_l, pd_l, slots, vslots, claim, z_l, x_s, u_l, gm_l, r,
                                            th_n, bn_n);
    }
}

// The fleet kernel's context and its max |g| epilogue: gpad_loop_kernel's own text of both, kept
// apart because that kernel's register allocation moves when they are hoisted out of its body
// (+1 VGPR in most buckets, other scratch at 208/208).  (The kernels: gpad_loop_kernels.inc, below.)
// the workgroup's context; claim_base: the queue's first position, after the static starts
__device__ __forceinline__ DuoCtx loop_ctx(const SolveArgs<float>& a, int claim_base) {
    DuoCtx c;
    c.tid = threadIdx.x;
    c.count = a.batch;
    c.G = gridDim.x;
    c.v0 = 0;
    c.fresh = true;
    c.use_tol = a.tol > 0.0;
    c.n = a.n;
    c.m = a.m;
    c.N = a.N;
    c.Kc = a.check_every;
    c.kc0 = c.Kc;
    c.nA = (c.n + 63) >> 6;
    c.nwaves = blockDim.x >> 6;
    {   // the G/L waves first (the older wave of each SIMD), as gpad_duo_kernel
        const int nB = c.nwaves - c.nA;
        c.isA = (c.tid >> 6) >= nB;
        c.row = c.isA ? c.tid - 64 * nB : c.tid;
        c.b0 = 0;
    }
    c.live = c.isA ? c.row < c.n : c.row < c.m;
    c.claim_base = claim_base;
    return c;
}

// the run's max |g| (the certification floor): this workgroup's slot, workgroup 0 zeroes the rest.
// gm_l: the per-lane maxima (LoopLds::gm).  Uniform, contains barriers.
__device__ __forceinline__ void loop_gmax_out(const DuoCtx& c, float* gm_l) {
    LoopKernArgs& A = largs();
    if (A.gmax) {
        const float wm = wave_reduce(gm_l[c.tid], OpAbsmaxNan{});
        __syncthreads();  // (every lane has read its gm word)
        if ((c.tid & 63) == 0) gm_l[c.tid >> 6] = wm;
        __syncthreads();
        if (c.tid == 0) {
            float mx = 0.0f;
            for (int w = 0; w < c.nwaves; ++w) mx = absmax_nan(mx, gm_l[w]);
            A.gmax[blockIdx.x] = (double)mx;
        }
        if (blockIdx.x == 0)
            for (int i = c.G + c.tid; i < kAbsmaxMaxBlocks; i += blockDim.x) A.gmax[i] = 0.0;
    }
}

// the kernels: the unbound pair, then the pair with the infeasibility certificate
#define GPAD_LOOP_FK 0
#include "gpad_loop_kernels.inc"
#undef GPAD_LOOP_FK
#define GPAD_LOOP_FK 1
#include "gpad_loop_kernels.inc"
#undef GPAD_LOOP_FK

// ---- host side: the instantiation of a (KA, KB) bucket pair, per translation unit ----------------
typedef void (*LoopFn)(LoopArgs);
template <int MODE, int KA, int KB>
LoopFn loop_fn_ab() {
    if constexpr (MODE == kLoopFleet) return gpad_loop_fleet_kernel<KA, KB>;
    else return gpad_loop_kernel<KA, KB, MODE>;
}
// ka = res_bucket(m), kb = res_bucket(n)
template <int MODE>
LoopFn loop_fn_of(int ka, int kb) {
    return with_buckets(ka, kb, [](auto KA, auto KB) {
        return loop_fn_ab<MODE, decltype(KA)::value, decltype(KB)::value>();
    });
}
// defined in gpad_loop_plant.hip / gpad_loop_fleet.hip
LoopFn loop_fn_per_plant(int ka, int kb);
LoopFn loop_fn_fleet(int ka, int kb);

// the certificate twins, one unit per mode: gpad_loop_farkas.hip, gpad_loop_plant_farkas.hip,
// gpad_loop_fleet_farkas.hip
typedef void (*LoopFarkasFn)(LoopArgs, FarkasArgs);
template <int MODE, int KA, int KB>
LoopFarkasFn loop_farkas_fn_ab() {
    if constexpr (MODE == kLoopFleet) return gpad_loop_fleet_farkas_kernel<KA, KB>;
    else return gpad_loop_farkas_kernel<KA, KB, MODE>;
}
template <int MODE>
LoopFarkasFn loop_farkas_fn_of(int ka, int kb) {
    return with_buckets(ka, kb, [](auto KA, auto KB) {
        return loop_farkas_fn_ab<MODE, decltype(KA)::value, decltype(KB)::value>();
    });
}
LoopFarkasFn loop_farkas_fn_shared(int ka, int kb);
LoopFarkasFn loop_farkas_fn_per_plant(int ka, int kb);
LoopFarkasFn loop_farkas_fn_fleet(int ka, int kb);

}  // namespace gpad
