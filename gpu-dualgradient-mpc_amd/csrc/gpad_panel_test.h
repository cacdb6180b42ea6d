// gpad_panel_test.h -- the Algorithm-1 termination test of the MFMA panel kernels, written once
// (gfx950).  gpad_chain.h states the test and holds its per-row terms (TestRows / VerRows); this is
// the rest of it for kernels whose wave holds four rows of each of a panel's 16 columns: lane
// (j = lane >> 4, c = lane & 15) has rows 4r + j of column c.  S is the kernels' scalar (float:
// gpad_panel.hip, gpad_loop_panel.hip, gpad_bigpanel.hip, gpad_flatpanel.hip; double: gpad_panel64.hip).
// The panel pairs (gpad_pairs.h) keep their own packed slots and reduction, measured into place.
//
// One test event, per column (the numbers are gpad_chain.h's):
//   1. every live row adds to the five partials (TestPart::row), they meet over the column's four
//      lane groups, xor 16, xor 32 (fold), and go to the slot of the wave (row tile, unit) (put)
//      -- barrier --
//   2. the column's slots are reduced and decided on: stage1
//   3. a nominated (A) is decided on cz = G_L z of a verification GEMM, through violz / magh of the
//      same slots: VerPart::row / fold / put, -- barrier --, verified (the kernel resets u to cz)
//   4. check_code(bits, verified) -- as ballot masks where lanes 0..15 / 0..63 decide for the
//      columns: m1 = verified, m2 = (B) & ~m1
// What stays in the kernels: which rows are live, which slot a wave writes, who reduces and how the
// outcome becomes uniform (__syncthreads_or, or ballots), and the bookkeeping of zhat in LDS.
//
// Every step in one workgroup -- stage 1, the verification GEMM and both codes 1 and 2 in one
// 16-column panel of the reference -- is exercised by:
//   gpad_panel_kernel       tests/test_schedule_tables.py test_seed[37x53-panel]
//   gpad_loop_panel_kernel  tests/test_loop_panel.py test_both_codes_in_one_panel
//   gpad_bigpanel_kernel    tests/test_schedule_tables.py test_seed[300x280-bigpanel]; at every <NT1, NT2>,
//                           with a code-1 and a code-2 finish at one test: tests/test_bigpanel.py test_algorithm1
//   gpad_flatpanel_kernel   tests/test_schedule_tables.py test_flat_seed[4x10-panels]
//   gpad_panel64_kernel     tests/test_schedule_tables.py test_seed_f64_both_codes_in_one_panel
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "gpad_chain.h"  // (TestRows / VerRows, bfly, OpMax / OpMin / OpAdd, absd, check_code)
#include "gpad_internal.h"

namespace gpad {

// per wave (row tile, unit) and column: the partials of the test.  The verification of a
// nominated (A) reuses violz / magh for max(G_L z + pD) / max(|G_L z| + |pD|).
template <typename S>
struct TestSlot {
    S violz[16], violh[16], wmin[16];
    double gap[16];
    S magh[16];  // max(|G_L zhat| + |pD|): test (B)'s rounding scale
};

// one value over the four lane groups of a column: xor 16, then xor 32, on the VALU (gpad_chain.h
// bfly).  SHFL: the same partners and values by __shfl_xor (ds_bpermute), for gpad_bigpanel_kernel and
// gpad_flatpanel_kernel: three of their register-bound instantiations spill one more dword with
// the VALU butterfly, none with this one (profiles/r15_panel_test_isa.txt).
template <bool SHFL = false, typename V, typename Op>
__device__ __forceinline__ V col_fold(V v, Op op) {
    if constexpr (SHFL) {
        v = op(v, __shfl_xor(v, 16, 64));
        return op(v, __shfl_xor(v, 32, 64));
    } else {
        return bfly<32>(bfly<16>(v, op), op);
    }
}

// row(): gpad_chain.h TestRows, the one text of the per-row terms
template <typename S>
struct TestPart : TestRows<S> {
    template <bool SHFL = false>
    __device__ __forceinline__ void fold() {
        this->violz = col_fold<SHFL>(this->violz, OpMax{});
        this->violh = col_fold<SHFL>(this->violh, OpMax{});
        this->magh = col_fold<SHFL>(this->magh, OpMax{});
        this->wmin = col_fold<SHFL>(this->wmin, OpMin{});
        this->gap = col_fold<SHFL>(this->gap, OpAdd{});
    }
    __device__ __forceinline__ void put(TestSlot<S>& s, int c, bool lead) const {  // lead: lane group j == 0
        if (lead) {
            s.violz[c] = this->violz;
            s.violh[c] = this->violh;
            s.magh[c] = this->magh;
            s.wmin[c] = this->wmin;
            s.gap[c] = this->gap;
        }
    }
};

// The infeasibility certificate's nomination partial (gpad_farkas.h): q = sum y+ pD over a column's live
// rows at a certificate event, folded and summed as gap is (lane groups, then the slots ascending).  Only
// the kernel variants that carry the certificate hold one; the others' code does not change.
struct FarkasPart {
    double q = 0.0;
    __device__ __forceinline__ void row(float yp, float pd) { q += (double)yp * (double)pd; }
    __device__ __forceinline__ void fold() { q = col_fold<false>(q, OpAdd{}); }
};

// f(s) for the slots s of [first, first + count) in ascending order (the fp64 gap sum's order is
// part of the result); N > 0: count == N at compile time, unrolled
template <int N, typename F>
__device__ __forceinline__ void slot_range(int first, int count, F f) {
    if constexpr (N > 0) {
#pragma unroll
        for (int s = 0; s < N; ++s) f(first + s);
    } else {
        for (int s = first; s < first + count; ++s) f(s);
    }
}

struct Stage1 {
    int bits;          // 1: (A) nominated, 2: (B) passed
    bool vh_ok, w_ok;  // (B)'s violation part and w >= 0 on their own, and its gap term:
    double gq;         // the f64 kernel's value-function branches read them
};

template <typename S, int N = 0>
__device__ __forceinline__ Stage1 stage1(const TestSlot<S>* slots, int first, int count, int c, double L,
                                         double tol, double tol_gap) {
    double vz = -INFINITY, vh = -INFINITY, wm = INFINITY, gq = 0.0, mh = 0.0;
    slot_range<N>(first, count, [&](int s) {
        vz = fmax(vz, (double)slots[s].violz[c]);
        vh = fmax(vh, (double)slots[s].violh[c]);
        mh = fmax(mh, (double)slots[s].magh[c]);
        wm = fmin(wm, (double)slots[s].wmin[c]);
        gq += slots[s].gap[c];
    });
    Stage1 r;
    r.vh_ok = viol_ok(vh, mh, L, tol, ViolMargin<S>::value);
    r.w_ok = wm >= 0.0;
    r.gq = gq;
    r.bits = (vz * L <= tol ? 1 : 0) | ((r.vh_ok && r.w_ok && (gq * L <= tol_gap)) ? 2 : 0);
    return r;
}

// row(): gpad_chain.h VerRows, on the live rows of a nominated column
template <typename S>
struct VerPart : VerRows<S> {
    template <bool SHFL = false>
    __device__ __forceinline__ void fold() {
        this->viol = col_fold<SHFL>(this->viol, OpMax{});
        this->mag = col_fold<SHFL>(this->mag, OpMax{});
    }
    // (every wave's stage-1 reads of the slots precede the barrier before the verification GEMM)
    __device__ __forceinline__ void put(TestSlot<S>& s, int c, bool lead) const {
        if (lead) {
            s.violz[c] = this->viol;
            s.magh[c] = this->mag;
        }
    }
};

template <typename S, int N = 0>
__device__ __forceinline__ bool verified(const TestSlot<S>* slots, int first, int count, int c, double L,
                                         double tol) {
    double vc = -INFINITY, mc = 0.0;
    slot_range<N>(first, count, [&](int s) {
        vc = fmax(vc, (double)slots[s].violz[c]);
        mc = fmax(mc, (double)slots[s].magh[c]);
    });
    return viol_ok(vc, mc, L, tol, ViolMargin<S>::value);
}

}  // namespace gpad
