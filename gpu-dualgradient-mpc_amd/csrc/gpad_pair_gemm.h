// gpad_pair_gemm.h -- the GEMM primitives of the panel pairs (gpad_pairs.h panel2_run, 8 < T <= 16):
// one or two MFMA chains per wave over the fragment images of gpad_panel.h, with the A ring, the
// early A prefetch, the runtime-length variant and the chain pieces of the hand-off.
#pragma once

#include <hip/hip_runtime.h>

#include "gpad_panel.h"

namespace gpad {

// Prelude priority (r05).  The SIMD issues oldest wave first, VALU and MFMA from one port: while
// an older wave has an MFMA ready (a double wave always has), a younger wave cannot issue even the
// VALU ops between the barrier and its first MFMA (uniform-branch compares, spilled-SGPR
// v_readlanes, LDS addresses), so it does not even read its first B fragment until the older
// chains are done, and each hand-over between the waves of a SIMD costs the younger wave's whole
// prelude plus the LDS latency of its B reads (~600 cycles, profiles/r05_stamp_*.txt: the loop tops
// of a SIMD's waves fall 1.3k, 5k, 7.6k cycles after the barrier).  So every wave raises its
// priority before the barriers of the solve loop and drops it right before its first MFMA of the
// next GEMM: all waves get through their preludes and issue their first B reads right after the
// barrier, and the chains then run oldest-first with their operands already in registers.
// Invariant: a wave holds priority 2 only between a loop barrier and its next chain (or the point
// where it learns it has none); every path out of that window -- a GEMM helper's prelude, the
// no-GEMM branches of the tiles past the output rows, the loop exit -- drops it to 0.
#define GPAD_PRELUDE_HI() __builtin_amdgcn_s_setprio(2)
#define GPAD_PRELUDE_LO()                  \
    do {                                   \
        __builtin_amdgcn_sched_barrier(0); \
        __builtin_amdgcn_s_setprio(0);     \
        __builtin_amdgcn_sched_barrier(0); \
    } while (0)

// ---------------------------------------------------------------------------------------
// Panel pairs (8 < T <= 16): a 16-wave workgroup owns TWO panels, balanced over the SIMDs.
// A 13-wave single-panel workgroup puts 4,3,3,3 waves (tile chains) on the CU's SIMDs, and a
// second one is not co-resident at its register budget, so the busiest SIMD carries 4 chains
// while the mean is 3.25.  Here the 2T (panel, tile) chains of two panels are dealt to 16 waves
// (4 per SIMD, waves w, w+4, w+8, w+12 share one): D = 2T-16 "double" waves own tile w of BOTH
// panels -- one A fragment feeds two MFMA chains, which also hides the 40-cycle MFMA
// dependency -- and the 32-2T "single" waves own one (panel, tile) each.  Doubles go to waves
// 0..D-1, i.e. round-robin over the SIMDs, so the SIMD loads differ by at most one chain
// (T = 13: 7,7,6,6 for 26 chains).  When a phase has no more panels than workgroups, a
// workgroup takes one panel (waves 0..T-1, one tile each): pairing would only idle CUs.
// ---------------------------------------------------------------------------------------
template <int T, bool DUAL>
__device__ __forceinline__ void panel_gemm2(__amdgpu_buffer_rsrc_t PA, const float4* B0, const float4* B1,
                                            int voff, int lane, f32x4& acc0, f32x4& acc1) {
    acc0 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    acc1 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float4 a[2], b0[2], b1[2];
    a[0] = as_float4(__builtin_amdgcn_raw_buffer_load_b128(PA, voff, 0, 0));
    b0[0] = B0[lane];
    if constexpr (DUAL) b1[0] = B1[lane];
    GPAD_PRELUDE_LO();
#pragma unroll
    for (int kb = 0; kb < T; ++kb) {
        const int cur = kb & 1, nxt = cur ^ 1;
        if (kb + 1 < T) {
            a[nxt] = as_float4(__builtin_amdgcn_raw_buffer_load_b128(PA, voff, (kb + 1) * T * 1024, 0));
            b0[nxt] = B0[(kb + 1) * 64 + lane];
            if constexpr (DUAL) b1[nxt] = B1[(kb + 1) * 64 + lane];
        }
        __builtin_amdgcn_sched_barrier(0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur].x, b0[cur].x, acc0, 0, 0, 0);
        if constexpr (DUAL) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur].x, b1[cur].x, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur].y, b0[cur].y, acc0, 0, 0, 0);
        if constexpr (DUAL) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur].y, b1[cur].y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur].z, b0[cur].z, acc0, 0, 0, 0);
        if constexpr (DUAL) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur].z, b1[cur].z, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur].w, b0[cur].w, acc0, 0, 0, 0);
        if constexpr (DUAL) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur].w, b1[cur].w, acc1, 0, 0, 0);
        // both chains advance together, one k-block per step (else the scheduler defers the
        // second chain past the loop and keeps every B fragment live)
        if constexpr (DUAL) asm volatile("" : "+v"(acc0), "+v"(acc1)::"memory");
        else asm volatile("" : "+v"(acc0)::"memory");
    }
}

// A fragments of the first PD k-blocks, issued early (before the barrier that precedes the
// GEMM: A is the constant matrix, so its L2 latency need not start at the barrier).
template <int T, int PD>
__device__ __forceinline__ void panel_a_prefetch(__amdgpu_buffer_rsrc_t PA, int voff, float4 (&ap)[PD]) {
#pragma unroll
    for (int p = 0; p < PD; ++p)
        if (p < T) ap[p] = as_float4(__builtin_amdgcn_raw_buffer_load_b128(PA, voff, p * T * 1024, 0));
}

// panel_gemm2 with an A ring PD blocks deep, seeded by panel_a_prefetch.  The last k-block
// issues only its first kq MFMA steps: k-steps past the matrix are zero in both operands, so
// skipping them is exact (an accumulator started at +0 never holds -0).  kq is wave-uniform.
template <int T, bool DUAL, int PD>
__device__ __forceinline__ void panel_gemm3(__amdgpu_buffer_rsrc_t PA, const float4* B0, const float4* B1,
                                            int voff, int lane, f32x4& acc0, f32x4& acc1,
                                            const float4 (&ap)[PD], int kq) {
    acc0 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    acc1 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    constexpr int R = PD + 1;
    float4 a[R], b0[2], b1[2];
#pragma unroll
    for (int p = 0; p < PD; ++p) a[p] = ap[p];
    b0[0] = B0[lane];
    if constexpr (DUAL) b1[0] = B1[lane];
    b0[1] = B0[64 + lane];  // (block 1 too, so the whole prelude precedes the priority drop)
    if constexpr (DUAL) b1[1] = B1[64 + lane];
    GPAD_PRELUDE_LO();
#pragma unroll
    for (int kb = 0; kb < T; ++kb) {
        const int cur = kb & 1, nxt = cur ^ 1;
        const float4 ak = a[kb % R];
        if (kb + PD < T)
            a[(kb + PD) % R] = as_float4(__builtin_amdgcn_raw_buffer_load_b128(PA, voff, (kb + PD) * T * 1024, 0));
        if (kb >= 1 && kb + 1 < T) {  // (blocks 0 and 1 were read before the loop)
            b0[nxt] = B0[(kb + 1) * 64 + lane];
            if constexpr (DUAL) b1[nxt] = B1[(kb + 1) * 64 + lane];
        }
        __builtin_amdgcn_sched_barrier(0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ak.x, b0[cur].x, acc0, 0, 0, 0);
        if constexpr (DUAL) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ak.x, b1[cur].x, acc1, 0, 0, 0);
        if (kb + 1 < T || kq > 1) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ak.y, b0[cur].y, acc0, 0, 0, 0);
            if constexpr (DUAL) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ak.y, b1[cur].y, acc1, 0, 0, 0);
        }
        if (kb + 1 < T || kq > 2) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ak.z, b0[cur].z, acc0, 0, 0, 0);
            if constexpr (DUAL) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ak.z, b1[cur].z, acc1, 0, 0, 0);
        }
        if (kb + 1 < T || kq > 3) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ak.w, b0[cur].w, acc0, 0, 0, 0);
            if constexpr (DUAL) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ak.w, b1[cur].w, acc1, 0, 0, 0);
        }
        if constexpr (DUAL) asm volatile("" : "+v"(acc0), "+v"(acc1)::"memory");
        else asm volatile("" : "+v"(acc0)::"memory");
    }
}

// Runtime-length variant for a GEMM whose K spans fewer k-blocks than the tile count
// (n != m: e.g. the battery's n = 40 against m = 180 -> 3 of 12 blocks).  Unrolled by two with
// fixed register roles (even blocks in a0, odd in a1) and every load unconditional (indices
// clamped to the last block), so each block's waitcnt counts only the loads issued after its
// operands -- a rotated ring with conditional loads made the compiler drain both counters at
// every block.  A is PD (1 or 2) blocks ahead, B one block ahead; soffset in an SGPR.
template <int T, bool DUAL, int PD>
__device__ __forceinline__ void panel_gemm_rt(__amdgpu_buffer_rsrc_t PA, const float4* B0, const float4* B1,
                                              int voff, int lane, f32x4& acc0, f32x4& acc1,
                                              const float4 (&ap)[PD], int nkb, int kq) {
    constexpr int PR = PD > 2 ? 2 : PD;  // (deeper rings seed only their first two blocks here)
    acc0 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    acc1 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int last = nkb - 1;
    auto lda = [&](int kb) -> float4 {
        return as_float4(__builtin_amdgcn_raw_buffer_load_b128(PA, voff, (kb < last ? kb : last) * T * 1024, 0));
    };
    auto blk = [&](const float4& ak, const float4& bk0, const float4& bk1, int steps) {
        __builtin_amdgcn_sched_barrier(0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ak.x, bk0.x, acc0, 0, 0, 0);
        if constexpr (DUAL) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ak.x, bk1.x, acc1, 0, 0, 0);
        if (steps > 1) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ak.y, bk0.y, acc0, 0, 0, 0);
            if constexpr (DUAL) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ak.y, bk1.y, acc1, 0, 0, 0);
        }
        if (steps > 2) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ak.z, bk0.z, acc0, 0, 0, 0);
            if constexpr (DUAL) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ak.z, bk1.z, acc1, 0, 0, 0);
        }
        if (steps > 3) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ak.w, bk0.w, acc0, 0, 0, 0);
            if constexpr (DUAL) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ak.w, bk1.w, acc1, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    float4 a0 = ap[0], a1 = PR == 2 ? ap[1] : ap[0];
    float4 e0 = B0[lane], f0 = DUAL ? B1[lane] : e0, e1, f1;
    GPAD_PRELUDE_LO();
    for (int kb = 0;; kb += 2) {
        const int k1 = kb + 1 < last ? kb + 1 : last, k2 = kb + 2 < last ? kb + 2 : last;
        if constexpr (PR == 1) a1 = lda(kb + 1);
        e1 = B0[k1 * 64 + lane];
        if constexpr (DUAL) f1 = B1[k1 * 64 + lane];
        blk(a0, e0, f0, kb < last ? 4 : kq);
        if constexpr (PR == 2) a0 = lda(kb + 2);
        if (kb + 1 > last) break;
        if constexpr (PR == 1) a0 = lda(kb + 2);
        e0 = B0[k2 * 64 + lane];
        if constexpr (DUAL) f0 = B1[k2 * 64 + lane];
        blk(a1, e1, f1, kb + 1 < last ? 4 : kq);
        if constexpr (PR == 2) a1 = lda(kb + 3);
        if (kb + 2 > last) break;
    }
    if constexpr (DUAL) asm volatile("" : "+v"(acc0), "+v"(acc1)::"memory");
    else asm volatile("" : "+v"(acc0)::"memory");
}

// k-blocks [KB0, KB1) of one chain, continuing acc (not reset): the A ring PD blocks deep is
// seeded with blocks KB0.. by panel_a_prefetch_from; the last matrix block issues kq steps.
template <int T, int PD, int KB0, int KB1, bool LO = true>
__device__ __forceinline__ void panel_chain(__amdgpu_buffer_rsrc_t PA, const float4* B0, int voff, int lane,
                                            f32x4& acc, const float4 (&ap)[PD], int kq) {
    constexpr int R = PD + 1;
    float4 a[R], b[2];
#pragma unroll
    for (int p = 0; p < PD; ++p) a[p] = ap[p];
    b[0] = B0[KB0 * 64 + lane];
    if constexpr (LO) GPAD_PRELUDE_LO();  // (LO = false: a relay piece that runs at its own priority)
#pragma unroll
    for (int kb = KB0; kb < KB1; ++kb) {
        const int i = kb - KB0, cur = i & 1, nxt = cur ^ 1;
        const float4 ak = a[i % R];
        if (kb + PD < KB1)
            a[(i + PD) % R] = as_float4(__builtin_amdgcn_raw_buffer_load_b128(PA, voff, (kb + PD) * T * 1024, 0));
        if (kb + 1 < KB1) b[nxt] = B0[(kb + 1) * 64 + lane];
        __builtin_amdgcn_sched_barrier(0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ak.x, b[cur].x, acc, 0, 0, 0);
        if (kb + 1 < T || kq > 1) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ak.y, b[cur].y, acc, 0, 0, 0);
        if (kb + 1 < T || kq > 2) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ak.z, b[cur].z, acc, 0, 0, 0);
        if (kb + 1 < T || kq > 3) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ak.w, b[cur].w, acc, 0, 0, 0);
        asm volatile("" : "+v"(acc)::"memory");
    }
}

template <int T, int PD>
__device__ __forceinline__ void panel_a_prefetch_from(__amdgpu_buffer_rsrc_t PA, int voff, float4 (&ap)[PD],
                                                      int kb0) {
#pragma unroll
    for (int p = 0; p < PD; ++p)
        if (kb0 + p < T) ap[p] = as_float4(__builtin_amdgcn_raw_buffer_load_b128(PA, voff, (kb0 + p) * T * 1024, 0));
}

}  // namespace gpad
