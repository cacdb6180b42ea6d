// gpad_pairs.h -- the body of the panel-pair kernel (gpad_pairs.hip gpad_panel2_kernel, 8 < T <= 16):
// the chain hand-off, the workgroup's LDS, the LDS-DMA row I/O and panel2_run, the solve loop of one
// wave role.  Included by gpad_pairs.hip alone, after it has defined the GPAD_STAMP_* / GPAD_PSTAMP*
// macros (empty in the product build).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "gpad_chain.h"  // (the VALU butterflies of the test reductions)
#include "gpad_internal.h"
#include "gpad_pair_gemm.h"

namespace gpad {

// two rows per VALU instruction (v_pk_add / v_pk_mul / v_pk_fma_f32: IEEE f32 per element, the
// same rounding as the scalar forms, so the epilogues stay bit-identical)
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 f2(float a, float b) { return f32x2{a, b}; }
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

// Chain hand-off (T = 9, 11, 13, both GEMMs full-length).  A chain is an ascending-k sequence of
// f32 MFMAs whose C operand is the previous step's result; it may be cut at any k-block and
// continued on another wave -- even on another SIMD -- from an accumulator parked in LDS, and the
// result is bit-identical.  The layouts use this to even out the SIMDs' chain loads:
// * pairs: with 2T chains per GEMM the 16-wave deal leaves SIMDs 0,1 one chain above SIMDs 2,3
//   (7,7,6,6; the phase lasts 7 chains of a mean 6.5).  The single wave on SIMD 2 (3) that owns
//   tile T-1 of panel 0 (1) first runs k-blocks [0, S) of tile T-2 of the same panel -- the chain
//   of wave 12 (13) on SIMD 0 (1) -- then its own chain; wave 12 (13) continues from block S.
//   Every SIMD then carries 6.5 chains.
// * one panel per workgroup: T waves put 4,3,3,3 chains on the SIMDs while waves 13..15 idle.
//   Tile T-1's chain (wave 12, SIMD 0) instead runs as a relay: blocks [0,4) on wave 13 (SIMD 1),
//   [4,8) on 14 (SIMD 2), [8,T) and the epilogue on wave 12 -- the busiest SIMD carries 3.36
//   chains (T = 9 likewise: 3,2,2,2 chains, tile 8 over waves 9 -> 10 -> 8).  The relay is a
//   sequential path through three SIMDs (each piece issues at most every other MFMA slot of its
//   SIMD, plus ~300 cycles per hand-off), so it must stay shorter than the SIMDs' own chains:
//   raised issue priorities, whole pieces prefetched before the barrier, and a fourth hop (a
//   4-way relay) measured slower than none.
// A slot's flag carries the hand-off generation (one per GEMM, counted alike by every wave), so
// flags are never reset; a receiver waits with a bound, and a wait that expires fails the run
// (handoff_wait: GPAD_ERR_DEVICE) rather than hanging the GPU or returning stale results.
template <int T>
struct Handoff {
    // pairs: odd T with singles on waves 12..15 (T = 9, 11, 13: SIMD loads 5,5,4,4 / 6,6,5,5 /
    // 7,7,6,6); one panel: T = 9, 13 (T % 4 == 1: SIMD 0 carries the extra tile, waves T, T+1 idle)
    static constexpr bool on = T == 9 || T == 11 || T == 13;
    static constexpr bool relay = T == 9 || T == 13;
    static constexpr int S = T / 2;      // pairs: helper blocks 4S MFMAs vs 4(T-S)-4+kq on the receiver
    static constexpr int R1 = T / 3, R2 = 2 * (T / 3);  // one panel: relay cuts (equal pieces, prefetched whole)
};

// Per (panel, row tile) partials of the test, one entry per column: the four float terms packed
// (violz, violh, magh, wmin: one ds_read_b128 per tile on the reduction side) and the fp64 gap.
// The verification of a nominated (A) reuses .x / .z for max(G_L z + pD) / max(|G_L z| + |pD|).
struct PanelSlot2 {
    float4 f[16];
    double gap[16];
};

// The tile reduction of the test, every wave at once (uniform result, no vote barrier): lane
// 16 pp + cc reduces tiles [0, H) of column cc of panel pp, lane 32 + 16 pp + cc tiles [H, T);
// the halves meet through one xor-32 exchange.  The f32 maxima / minima are exact in any order
// (one conversion to fp64 after them instead of one per tile); the fp64 gap is summed per half,
// then the halves added.
template <int T>
__device__ __forceinline__ void panel2_reduce(const PanelSlot2 (&S)[2][T], int lane, float4& f, double& gap) {
    constexpr int H = (T + 1) / 2;
    const int pp = (lane >> 4) & 1, cc = lane & 15, lo = lane < 32 ? 0 : H, hi = lane < 32 ? H : T;
    f = make_float4(-INFINITY, -INFINITY, 0.0f, INFINITY);
    gap = 0.0;
#pragma unroll
    for (int s2 = 0; s2 < H; ++s2) {
        // every step but the last is in range on both halves (2H - 2 <= T - 1): no per-lane branch,
        // whose exec masks the compiler kept in spilled SGPRs; the last step selects
        const bool ok = s2 < H - 1 || lo + s2 < hi;
        const int si = ok ? lo + s2 : lo;
        const float4 e = S[pp][si].f[cc];
        const double gv = S[pp][si].gap[cc];
        f.x = ok ? fmaxf(f.x, e.x) : f.x;
        f.y = ok ? fmaxf(f.y, e.y) : f.y;
        f.z = ok ? fmaxf(f.z, e.z) : f.z;
        f.w = ok ? fminf(f.w, e.w) : f.w;
        gap = ok ? gap + gv : gap;
    }
    f.x = bfly<32>(f.x, OpMax{});  // (gfx950 v_permlane32_swap, gpad_chain.h)
    f.y = bfly<32>(f.y, OpMax{});
    f.z = bfly<32>(f.z, OpMax{});
    f.w = bfly<32>(f.w, OpMin{});
    gap = bfly<32>(gap, OpAdd{});  // (lower half + upper half on every lane, as before)
}

template <int T>
struct Panel2Lds {
    float4 Wl[2][T * 64];  // fragment order, per panel: w    (B of GEMM 1)
    float4 Zh[2][T * 64];  //                            zhat (B of GEMM 2)
    float4 Gp[2][T * 64];  //                            g_P rows
    float4 Pd[2][T * 64];  //                            p_D rows
    PanelSlot2 slots[2][T];
    float4 hand[2][64];    // hand-off accumulators (the pair helpers' / the relay's slots)
    int hflag[2];          // hand-off generation per slot
    int herr;              // a wait expired (handoff_wait): reported to the run's error word at exit
    int hdrop;             // fault injection (kDebugDropHandoff) for this workgroup
    int znz[16];           // per wave: a non-zero z_{-1} among its rows (fresh seed GEMM needed)
    float gred[16];        // per wave: max |g| over the rows it loaded (SolveArgs::gmax_part)
};

struct HoSlots {
    int in, out;  // LDS hand-off slots taken / given (-1: none)
};

// The results-out and park sites launder the column's instance index and the lane through an empty
// asm before forming its row pointers and offsets (r06): otherwise the compiler hoists the six per-panel 64-bit row pointers
// (z, y, wc, uc ... of each panel) out of the solve loop, and at 128 VGPRs the double waves spilled them
// -- 240 B of scratch per lane whose dirty lines were written back to HBM, ~39 MB per phase-1 launch at
// C4 (profiles/r06_write_probe.txt: a fixed-N launch that stores only z*, y* (13 MB) wrote 52 MB).
// This lane's four rows 16t + 4r + j (r = 0..3) of one instance's vector.  vec (16-B aligned rows):
// rows4_dma, one global_load_lds_dwordx4 per lane (the 16 columns x 64 contiguous bytes of a wave's
// tile, a quarter of the requests of four 4-B loads per lane) into 1 KiB of LDS the wave owns, then
// rows4_rd.  The DMA lands lane-linearly: lane l carries column c' = l >> 2's rows 16t + 4j' .. +3,
// j' = (l & 3) ^ ((c' >> 2) & 3), so the block holds column c's 16 floats with the 16-B chunks
// XOR-swizzled by c >> 2 and the four reads are conflict-free.  colbase is column c''s instance
// row 0; the tile's rows past `rows` read the last four rows (the caller zeroes them).  r05 loaded
// into VGPRs and transposed through the block, which serialised the operands' loads behind each
// other's LDS waits; r06 stages by DMA, every operand of every panel in flight at once and no VGPRs
// held meanwhile (batching the VGPR loads instead spilled: 45-69 VGPRs in the pair kernels).
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_void_t;

__device__ __forceinline__ void rows4_dma(const float* colbase, int t, int rows, int lane, float4* blk) {
    const int cc = lane >> 2;
    const int jj = (lane & 3) ^ ((cc >> 2) & 3);
    const int r0 = 16 * t + 4 * jj;
    const int rr = r0 + 3 < rows ? r0 : rows - 4;
    __builtin_amdgcn_global_load_lds((gbl_void_t*)(colbase + rr), (lds_void_t*)blk, 16, 0, 0);
}

__device__ __forceinline__ void rows4_rd(const float4* blk, int lane, float (&out)[4]) {
    const float* st = reinterpret_cast<const float*>(blk);
    const int j = lane >> 4, c = lane & 15, sw = (c >> 2) & 3;
#pragma unroll
    for (int r = 0; r < 4; ++r) out[r] = st[16 * c + 4 * (r ^ sw) + j];
}

// the scalar path (rows not 16-B aligned): four 4-B loads at clamped rows
__device__ __forceinline__ void rows4(const float* base, int t, int rows, int lane, float (&out)[4]) {
    const int j = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = 16 * t + 4 * r + j;
        out[r] = base[i < rows ? i : rows - 1];
    }
}

// The reverse of the loads above: this lane's rows 16t + 4r + j to an instance's vector, on lanes
// whose `on` holds (uniform over a column's four lanes); vec: transposed through the wave's LDS block
// into one 16-B store per lane of rows 16t + 4j .. +3 (every lane takes part in the transpose; rows
// past `rows` not stored).
__device__ __forceinline__ void rows4_store(float* base, int t, int rows, bool vec, float* st, int lane,
                                            const float (&v)[4], bool on) {
    const int j = lane >> 4, c = lane & 15, sw = (c >> 2) & 3;
    if (vec) {
#pragma unroll
        for (int r = 0; r < 4; ++r) st[16 * c + 4 * (r ^ sw) + j] = v[r];
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const float4 o = *reinterpret_cast<const float4*>(st + 16 * c + 4 * (j ^ sw));
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const int r0 = 16 * t + 4 * j;
        if (on && r0 < rows) *reinterpret_cast<float4*>(base + r0) = o;
    } else if (on) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * t + 4 * r + j;
            if (i < rows) base[i] = v[r];
        }
    }
}

// The waves of a workgroup are co-resident, so a post always arrives unless the layout logic is
// broken; the wait is still bounded (2^20 sleeps, ~30 ms) so that such a bug cannot hang the GPU,
// and an expired wait is recorded (L.herr) and ORed into the run's error word when the workgroup
// exits (gpad_panel2_kernel): the host then fails the run with GPAD_ERR_DEVICE instead of
// returning the stale accumulator's results as GPAD_OK.  Nothing of this sits on the hand-off's
// own path: the record is made only after the bound expired.
template <int T>
__device__ __forceinline__ f32x4 handoff_wait(Panel2Lds<T>& L, int slot, int gen, int lane) {
    for (int s = 0;; ++s) {
        if (__hip_atomic_load(&L.hflag[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == gen) break;
        if (s == (1 << 20)) {
            L.herr = 1;
            break;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    asm volatile("" ::: "memory");
    const float4 hv = L.hand[slot][lane];
    return f32x4{hv.x, hv.y, hv.z, hv.w};
}

template <int T>
__device__ __forceinline__ void handoff_post(Panel2Lds<T>& L, int slot, int gen, int lane, const f32x4& h) {
    L.hand[slot][lane] = make_float4(h[0], h[1], h[2], h[3]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the accumulator lands before the flag
    __hip_atomic_store(&L.hflag[slot], gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// a piece of another wave's chain: k-blocks [KB0, KB1) (KB1 < T) of the tile at voff, continued
// from slot hs.in (or from zero), parked in slot hs.out; PRIO raises the wave's issue priority
// fault injection (DROP, the kernel's test-only instantiation; L.hdrop): the first piece of the
// first hand-off withholds its post, so its receiver's wait expires
template <int T, int PD, int KB0, int KB1, bool PRIO, bool DROP>
__device__ __forceinline__ void handoff_piece(Panel2Lds<T>& L, __amdgpu_buffer_rsrc_t PA, const float4* B0, int voff,
                                              int lane, const float4 (&aph)[PD], HoSlots hs, int gen,
                                              unsigned long long* ts = nullptr) {
    f32x4 h = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (hs.in >= 0) h = handoff_wait(L, hs.in, gen, lane);
    if (ts) *ts = __builtin_amdgcn_s_memtime();  // (stamped builds only)
    if constexpr (PRIO) __builtin_amdgcn_s_setprio(3);
    panel_chain<T, PD, KB0, KB1, !PRIO>(PA, B0, voff, lane, h, aph, 4);
    if (!(DROP && gen == 1 && hs.in < 0 && L.hdrop)) handoff_post(L, hs.out, gen, lane, h);
    if constexpr (PRIO) __builtin_amdgcn_s_setprio(0);
}

// the chain's last piece on its owner: blocks [KB0, T) from slot hs.in
template <int T, int PD, int KB0, bool PRIO>
__device__ __forceinline__ void handoff_take(Panel2Lds<T>& L, __amdgpu_buffer_rsrc_t PA, const float4* B0, int voff,
                                             int lane, const float4 (&ap)[PD], HoSlots hs, int gen, int kq,
                                             f32x4& acc, unsigned long long* ts = nullptr) {
    acc = handoff_wait(L, hs.in, gen, lane);
    if (ts) *ts = __builtin_amdgcn_s_memtime();  // (stamped builds only)
    if constexpr (PRIO) __builtin_amdgcn_s_setprio(2);
    panel_chain<T, PD, KB0, T, !PRIO>(PA, B0, voff, lane, acc, ap, kq);
    if constexpr (PRIO) __builtin_amdgcn_s_setprio(0);
}

// Hand-off roles (Handoff): 0 none; 1 pair helper (NU = 1: blocks [KB0, KB1) of tile t-1 into
// slot hs.out, then its own chain); 2 receiver (NU = 1: its own chain from block KB0, slot hs.in);
// 3 relay (NU = 0: blocks [KB0, KB1) of tile t from slot hs.in, or zero, into slot hs.out).
// PRIO: the one-panel relay raises issue priority for its pieces.
// KQ > 0: the shape is known at compile time to have full-length chains on every tile of both
// GEMMs (16 (T-1) < n, m <= 16 T) whose last k-block issues KQ steps in both: no runtime kq tests
// (scalar branches whose conditions the compiler spilled to VGPR lanes) and no short-chain paths.
// DROP: the fault-injection instantiation (handoff_piece).
template <int T, int NU, int ROLE = 0, int KB0 = 0, int KB1 = 0, bool PRIO = false, int KQ = 0, bool DROP = false>
__device__ __forceinline__ void panel2_run(const SolveArgs<float>& a, Panel2Lds<T>& L, int t, int p0,
                                           bool pair, int items, int count, HoSlots hs = HoSlots{-1, -1}) {
    static_assert(ROLE == 0 || (Handoff<T>::on && (ROLE == 3 ? NU == 0 : NU == 1)), "hand-off roles");
    const int lane = threadIdx.x & 63;
    const int j = lane >> 4, c = lane & 15;
    const int n = a.n, m = a.m, N = a.N, K = a.check_every;
    const int abytes = T * T * 1024;
    const __amdgpu_buffer_rsrc_t PA1 =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.frag), 0, abytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t PA2 = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)a.frag + abytes), 0, abytes, 0x00020000);
    const bool use_tol = a.tol > 0.0;
    const bool fresh = a.v_begin == 0;
    const bool carry = a.v_end < N;
    const int voff = t * 1024 + lane * 16;
    const int slot = t * 64 + lane;
    constexpr int Q = NU > 0 ? NU : 1;  // array extent
    // GEMM 1: K = m, output rows n; GEMM 2: K = n, output rows m.  The last k-block issues only
    // the steps inside K when K is the padded dimension (kq), and a wave whose tile lies past
    // the output rows skips its GEMM (zeros).
    constexpr bool FULL = KQ > 0;
    const int nkb1 = FULL ? T : (m + 15) / 16, nkb2 = FULL ? T : (n + 15) / 16;  // k-blocks of each GEMM (<= T)
    const int kq1 = FULL ? KQ : (m - 16 * (nkb1 - 1) + 3) / 4, kq2 = FULL ? KQ : (n - 16 * (nkb2 - 1) + 3) / 4;
    const bool on1 = FULL || 16 * t < n, on2 = FULL || 16 * t < m;
    const int voff_r = voff - 1024;  // helper: the receiver's tile t - 1 (Handoff)
    int hgen = 0;                    // hand-off generation, counted alike by helper and receiver
    float gmx = 0.0f;                // max |g| over the rows this lane loads (gmax_part)
    // 16-B vector state I/O (rows4 / rows4_store) when every row start is 16-B aligned (uniform)
    const bool vec_io = ((n | m | (int)a.ld_gP | (int)a.ld_g) & 3) == 0 && n >= 4 && m >= 4 &&
                        ((reinterpret_cast<size_t>(a.z) | reinterpret_cast<size_t>(a.gP) |
                          reinterpret_cast<size_t>(a.y) | reinterpret_cast<size_t>(a.g) |
                          reinterpret_cast<size_t>(a.wc) | reinterpret_cast<size_t>(a.uc)) & 15) == 0;

    for (int it = blockIdx.x; it < items; it += gridDim.x) {
        GPAD_PSTAMP(0);
        // columns still running, bit 16 pp + c for panel pp of this item: the same word in every
        // wave (derived from uniform values and LDS), so the test needs no vote barrier
        unsigned live = 0u;
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
            if (pp == 1 && !pair) break;
            const int left = count - 16 * (pair ? 2 * it + pp : it);
            const int cnt = left < 0 ? 0 : (left > 16 ? 16 : left);
            live |= ((1u << cnt) - 1u) << (16 * pp);
        }
        bool act[Q];
        int inst[Q];
        float z[Q][4], y[Q][4], u[Q][4];
        // The columns' state, so that the loads are in flight together (r05): the instance of each
        // column (one load), then per panel every operand load unconditionally at clamped addresses
        // (an inactive column reads instance 0, a padding row the last real row), then the selects.  Loading under per-row / per-column conditions made the compiler branch around
        // every load and drain vmcnt at the joins -- 8-18 dependent round trips to memory per wave,
        // 10-23 us per phase start (profiles/r05_phase_*.txt).
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            act[q] = false;
            inst[q] = 0;
            if constexpr (NU == 0) continue;
            const int k = 16 * (pair ? 2 * it + p0 + q : it) + c;
            act[q] = k < count;
            KernArgs& A = kargs();
            inst[q] = A.idx_in ? A.idx_in[act[q] ? k : 0] : (act[q] ? k : 0);
        }
        if constexpr (NU > 0) {
            KernArgs& A = kargs();  // (gpad_internal.h: the row pointers are not kept across the loop)
            const float beta0 = A.beta[0];
            const bool vec = vec_io;
            // vec (r06): the operands arrive by LDS-DMA (rows4_dma), every panel's in flight at once:
            // z, gP, y, g into the wave's (panel, tile) blocks of Zh, Gp, Wl, Pd, then (carried
            // phases) wc, uc into those of Zh, Wl once the first four are read.  The final Gp / Pd /
            // Wl / Zh rows are stored after the reads of the same blocks (LDS is in order per wave).
            // Before: each operand's load waited behind the previous one's LDS transpose, four to
            // six round trips to memory per panel (profiles/r05_phase_stamps_vecio_*.txt: 14-30
            // kcycles to the first barrier).
            if (vec) {
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    int ln = lane;
                    asm volatile("" : "+v"(ln));  // (offsets formed per item, not kept across the item loop)
                    const size_t bc = (size_t)__shfl(inst[q], ln >> 2);
                    const int pq = p0 + q;
                    rows4_dma(A.z + bc * n, t, n, ln, &L.Zh[pq][64 * t]);
                    rows4_dma(A.gP + bc * A.ld_gP, t, n, ln, &L.Gp[pq][64 * t]);
                    rows4_dma(A.y + bc * m, t, m, ln, &L.Wl[pq][64 * t]);
                    rows4_dma(A.g + bc * A.ld_g, t, m, ln, &L.Pd[pq][64 * t]);
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();
            }
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                float zl[4], gpl[4], yl[4], gl[4];
                int ln = lane;
                asm volatile("" : "+v"(ln));
                const size_t b = (size_t)inst[q];
                const int pq = p0 + q;
                if (vec) {
                    rows4_rd(&L.Zh[pq][64 * t], ln, zl);
                    rows4_rd(&L.Gp[pq][64 * t], ln, gpl);
                    rows4_rd(&L.Wl[pq][64 * t], ln, yl);
                    rows4_rd(&L.Pd[pq][64 * t], ln, gl);
                } else {
                    rows4(A.z + b * n, t, n, ln, zl);
                    rows4(A.gP + b * A.ld_gP, t, n, ln, gpl);
                    rows4(A.y + b * m, t, m, ln, yl);
                    rows4(A.g + b * A.ld_g, t, m, ln, gl);
                }
                float gp[4], pd[4], wv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * t + 4 * r + j;
                    const bool okn = act[q] && i < n, okm = act[q] && i < m;
                    z[q][r] = okn ? zl[r] : 0.0f;
                    gp[r] = okn ? gpl[r] : 0.0f;
                    y[q][r] = okm ? yl[r] : 0.0f;
                    const float gr = okm ? gl[r] : 0.0f;
                    pd[r] = (float)(A.gscale * (double)gr);
                    gmx = absmax_nan(gmx, gr);
                    // w_0 = y_0 + beta_0 (y_0 - y_{-1}), y_{-1} = y_0 (fresh; carried: wc below)
                    wv[r] = __builtin_fmaf(beta0, y[q][r] - y[q][r], y[q][r]);
                    u[q][r] = 0.0f;
                }
                L.Gp[pq][slot] = make_float4(gp[0], gp[1], gp[2], gp[3]);
                L.Pd[pq][slot] = make_float4(pd[0], pd[1], pd[2], pd[3]);
                if (fresh) {
                    L.Wl[pq][slot] = make_float4(wv[0], wv[1], wv[2], wv[3]);
                    if (use_tol) L.Zh[pq][slot] = make_float4(z[q][0], z[q][1], z[q][2], z[q][3]);
                } else if (vec) {  // round two: wc, uc into the blocks just read
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    const size_t bc = (size_t)__shfl(inst[q], ln >> 2);
                    rows4_dma(A.wc + bc * m, t, m, ln, &L.Zh[pq][64 * t]);
                    if (use_tol) rows4_dma(A.uc + bc * m, t, m, ln, &L.Wl[pq][64 * t]);
                }
            }
            if (!fresh) {
                if (vec) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __builtin_amdgcn_wave_barrier();
                }
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    float wl[4], ul[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    int ln = lane;
                    asm volatile("" : "+v"(ln));
                    const size_t b = (size_t)inst[q];
                    const int pq = p0 + q;
                    if (vec) {
                        rows4_rd(&L.Zh[pq][64 * t], ln, wl);
                        if (use_tol) rows4_rd(&L.Wl[pq][64 * t], ln, ul);
                    } else {
                        rows4(A.wc + b * m, t, m, ln, wl);
                        if (use_tol) rows4(A.uc + b * m, t, m, ln, ul);
                    }
                    float wv[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const bool okm = act[q] && 16 * t + 4 * r + j < m;
                        wv[r] = okm ? wl[r] : 0.0f;
                        u[q][r] = okm ? ul[r] : 0.0f;
                    }
                    L.Wl[pq][slot] = make_float4(wv[0], wv[1], wv[2], wv[3]);
                }
            }
        }
#ifdef GPAD_STAMP
        if constexpr (NU > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's state is in
#endif
        GPAD_PSTAMP(1);
        if (fresh && use_tol) {  // u = G_L z_{-1} -- zero, and no GEMM, when every z_{-1} is zero
            // (a cold start: every chain step fma(G_L, 0, +0) gives +0, so u = +0 exactly)
            bool nz = false;
            if constexpr (NU > 0) {
#pragma unroll
                for (int q = 0; q < Q; ++q)
#pragma unroll
                    for (int r = 0; r < 4; ++r) nz = nz || z[q][r] != 0.0f;
            }
            const bool wnz = __ballot(nz) != 0ull;
            if (lane == 0) L.znz[threadIdx.x >> 6] = wnz ? 1 : 0;
            __syncthreads();
            int anynz = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) anynz |= L.znz[i];
            if constexpr (NU > 0) {
                if (anynz) {
                    f32x4 c0, c1;
                    panel_gemm2<T, NU == 2>(PA2, L.Zh[p0], L.Zh[NU == 2 ? 1 : p0], voff, lane, c0, c1);
#pragma unroll
                    for (int r = 0; r < 4; ++r) u[0][r] = c0[r];
                    if constexpr (NU == 2) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) u[Q - 1][r] = c1[r];
                    }
                }
            }
        }
        __syncthreads();

        // A ring depth: doubles 1 block ahead, singles 2 (deeper rings measured within noise,
        // profiles/r05_a_ring_depth_ab.txt); a relay piece prefetches its whole first piece
        constexpr int PD = NU == 2 ? 1 : (ROLE == 3 ? Handoff<T>::R1 : 2);
        float4 ap[PD];  // A blocks of the next GEMM, in flight across the barrier before it
        float4 aph[PD];  // helper / relay: the piece's first blocks
        auto prefetch = [&](__amdgpu_buffer_rsrc_t PA) {
            if constexpr (ROLE == 2) panel_a_prefetch_from<T, PD>(PA, voff, ap, KB0);
            else if constexpr (NU > 0) panel_a_prefetch<T, PD>(PA, voff, ap);
            if constexpr (ROLE == 1) panel_a_prefetch<T, PD>(PA, voff_r, aph);
            if constexpr (ROLE == 3) panel_a_prefetch_from<T, PD>(PA, voff, aph, KB0);
        };
        GPAD_PSTAMP(2);
        prefetch(PA1);
        int v = a.v_begin;
        GPAD_STAMP_DECL
        int kc = K - v % K;  // iterations to the next test: chk <=> v % K == 0 (a countdown, no division)
        while (true) {
            GPAD_STAMP_AT(0);  // (before the schedule's scalar loads, which a later s_memtime queues behind)
            // this iteration's schedule, loaded here and first used after GEMM 1: the loads are older
            // than every A load of the GEMM, so the GEMM's own vmcnt waits cover them (r09: loading
            // one iteration ahead cost two carried registers and two moves per iteration)
            const float th = a.theta[v], bn = a.beta[v + 1];
            ++v;
            const bool chk = use_tol && --kc == 0;
            if (kc == 0) kc = K;
            const float omt = 1.0f - th;
            // ---- GEMM 1 + epilogue: zhat = -ML w - g_P (8b), z = (1-th) z + th zhat (8c) ----
            if constexpr (NU > 0) {
                f32x4 acc[2];
                ++hgen;
                if constexpr (ROLE == 1)
                    handoff_piece<T, PD, KB0, KB1, PRIO, DROP>(L, PA1, L.Wl[p0], voff_r, lane, aph, hs, hgen,
                                                               GPAD_STAMP_PTR(6));
                if constexpr (ROLE == 2)
                    handoff_take<T, PD, KB0, PRIO>(L, PA1, L.Wl[p0], voff, lane, ap, hs, hgen, kq1, acc[0],
                                                   GPAD_STAMP_PTR(6));
                else if (on1 && nkb1 == T)
                    panel_gemm3<T, NU == 2, PD>(PA1, L.Wl[p0], L.Wl[NU == 2 ? 1 : p0], voff, lane, acc[0], acc[1],
                                                ap, kq1);
                else if (on1)
                    panel_gemm_rt<T, NU == 2, PD>(PA1, L.Wl[p0], L.Wl[NU == 2 ? 1 : p0], voff, lane, acc[0],
                                                   acc[1], ap, nkb1, kq1);
                else {
                    GPAD_PRELUDE_LO();
                    acc[0] = acc[1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                }
                GPAD_STAMP_AT(1);
                prefetch(PA2);
                float4 g4[Q];
#pragma unroll
                for (int q = 0; q < Q; ++q) g4[q] = L.Gp[p0 + q][slot];
                const f32x2 th2 = f2(th, th), omt2 = f2(omt, omt);
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const f32x2 h0 = f2(acc[q][0], acc[q][1]) - f2(g4[q].x, g4[q].y);
                    const f32x2 h1 = f2(acc[q][2], acc[q][3]) - f2(g4[q].z, g4[q].w);
                    L.Zh[p0 + q][slot] = make_float4(h0.x, h0.y, h1.x, h1.y);
                    // 8c on every column (see the epilogue note below)
                    const f32x2 z0 = pk_fma(omt2, f2(z[q][0], z[q][1]), th2 * h0);
                    const f32x2 z1 = pk_fma(omt2, f2(z[q][2], z[q][3]), th2 * h1);
                    z[q][0] = z0.x;
                    z[q][1] = z0.y;
                    z[q][2] = z1.x;
                    z[q][3] = z1.y;
                }
            } else if constexpr (ROLE == 3) {
                ++hgen;
                handoff_piece<T, PD, KB0, KB1, PRIO, DROP>(L, PA1, L.Wl[p0], voff, lane, aph, hs, hgen,
                                                           GPAD_STAMP_PTR(6));
                prefetch(PA2);
            } else {
                GPAD_PRELUDE_LO();  // (a wave with no chain: the window of the invariant ends here)
            }
            GPAD_STAMP_AT(2);
            GPAD_PRELUDE_HI();
            __syncthreads();
            GPAD_STAMP_AT(3);
            // ---- GEMM 2 + epilogue: y+ = [w + G_L zhat + p_D]+ (8d), next w (8a) ----------
            if constexpr (NU > 0) {
                f32x4 acc[2];
                ++hgen;
                if constexpr (ROLE == 1)
                    handoff_piece<T, PD, KB0, KB1, PRIO, DROP>(L, PA2, L.Zh[p0], voff_r, lane, aph, hs, hgen,
                                                               GPAD_STAMP_PTR(7));
                if constexpr (ROLE == 2)
                    handoff_take<T, PD, KB0, PRIO>(L, PA2, L.Zh[p0], voff, lane, ap, hs, hgen, kq2, acc[0],
                                                   GPAD_STAMP_PTR(7));
                else if (on2 && nkb2 == T)
                    panel_gemm3<T, NU == 2, PD>(PA2, L.Zh[p0], L.Zh[NU == 2 ? 1 : p0], voff, lane, acc[0], acc[1],
                                                ap, kq2);
                else if (on2)
                    panel_gemm_rt<T, NU == 2, PD>(PA2, L.Zh[p0], L.Zh[NU == 2 ? 1 : p0], voff, lane, acc[0],
                                                   acc[1], ap, nkb2, kq2);
                else {
                    GPAD_PRELUDE_LO();
                    acc[0] = acc[1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                }
                GPAD_STAMP_AT(4);
                prefetch(PA1);
                // (reading these LDS operands before the GEMM measured no faster: profiles/r02_epilogue_ab.txt)
                float4 w4[Q], p4[Q];
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    w4[q] = L.Wl[p0 + q][slot];
                    p4[q] = L.Pd[p0 + q][slot];
                }
                // The state updates run on every column, packed two rows per instruction: a
                // finished (or padding) column's z, y, u and w are never read again -- its results
                // left at the test that finished it, and MFMA output column c depends on B column c
                // only -- so the per-element masks of the active columns are not needed.  This
                // epilogue sits between the GEMM and the barrier on every SIMD at once; packing
                // halves its VALU issue: C4 to eps +1.3-1.5 % (profiles/r02_epilogue_ab.txt).
                // Three straight-line stages (r09): 8d / 8a of every panel, then the u recursion, then
                // (test iterations only) the partials.  Interleaved per panel, the uniform use_tol / chk
                // branches cut the epilogue into blocks that shared the splats and the partials' seeds:
                // a plain iteration of a double wave paid 10 seed moves and 3 splat moves (each stage now
                // forms its own splats, which the packed ops read by op_sel broadcast).
                {
                    const f32x2 bn2 = f2(bn, bn), half2 = f2(0.5f, 0.5f);
#pragma unroll
                    for (int q = 0; q < Q; ++q) {
                        const f32x2 c0 = f2(acc[q][0], acc[q][1]), c1 = f2(acc[q][2], acc[q][3]);
                        const f32x2 s0 = (f2(w4[q].x, w4[q].y) + f2(p4[q].x, p4[q].y)) + c0;
                        const f32x2 s1 = (f2(w4[q].z, w4[q].w) + f2(p4[q].z, p4[q].w)) + c1;
                        const f32x2 y0 = f2(__builtin_fabsf(s0.x) + s0.x, __builtin_fabsf(s0.y) + s0.y) * half2;
                        const f32x2 y1 = f2(__builtin_fabsf(s1.x) + s1.x, __builtin_fabsf(s1.y) + s1.y) * half2;
                        const f32x2 n0 = pk_fma(bn2, y0 - f2(y[q][0], y[q][1]), y0);
                        const f32x2 n1 = pk_fma(bn2, y1 - f2(y[q][2], y[q][3]), y1);
                        L.Wl[p0 + q][slot] = make_float4(n0.x, n0.y, n1.x, n1.y);
                        y[q][0] = y0.x;
                        y[q][1] = y0.y;
                        y[q][2] = y1.x;
                        y[q][3] = y1.y;
                    }
                }
                if (use_tol) {
                    const f32x2 th2 = f2(th, th), omt2 = f2(omt, omt);
#pragma unroll
                    for (int q = 0; q < Q; ++q) {
                        const f32x2 c0 = f2(acc[q][0], acc[q][1]), c1 = f2(acc[q][2], acc[q][3]);
                        const f32x2 u0 = pk_fma(omt2, f2(u[q][0], u[q][1]), th2 * c0);
                        const f32x2 u1 = pk_fma(omt2, f2(u[q][2], u[q][3]), th2 * c1);
                        u[q][0] = u0.x;
                        u[q][1] = u0.y;
                        u[q][2] = u1.x;
                        u[q][3] = u1.y;
                    }
                }
                if (chk) {  // (implies use_tol) this tile's per-column partials of the test -> LDS
#pragma unroll
                    for (int q = 0; q < Q; ++q) {
                        float violz = -INFINITY, violh = -INFINITY, wmin = INFINITY, magh = 0.0f;
                        double gap = 0.0;
                        if (act[q]) {
                            const float wv[4] = {w4[q].x, w4[q].y, w4[q].z, w4[q].w};
                            const float pd[4] = {p4[q].x, p4[q].y, p4[q].z, p4[q].w};
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                if ((16 * t + 4 * r + j) < m) {
                                    const float cv = acc[q][r];
                                    const float tt = cv + pd[r];
                                    violh = fmaxf(violh, tt);
                                    magh = fmaxf(magh, __builtin_fabsf(cv) + __builtin_fabsf(pd[r]));
                                    wmin = fminf(wmin, wv[r]);
                                    gap -= (double)wv[r] * (double)tt;
                                    violz = fmaxf(violz, u[q][r] + pd[r]);
                                }
                            }
                        }
                        // lane groups j (xor 16, 32) on the VALU (gpad_chain.h)
                        violz = bfly<32>(bfly<16>(violz, OpMax{}), OpMax{});
                        violh = bfly<32>(bfly<16>(violh, OpMax{}), OpMax{});
                        magh = bfly<32>(bfly<16>(magh, OpMax{}), OpMax{});
                        wmin = bfly<32>(bfly<16>(wmin, OpMin{}), OpMin{});
                        gap = bfly<32>(bfly<16>(gap, OpAdd{}), OpAdd{});
                        if (j == 0) {
                            PanelSlot2& S = L.slots[p0 + q][t];
                            S.f[c] = make_float4(violz, violh, magh, wmin);
                            S.gap[c] = gap;
                        }
                    }
                }
            } else if constexpr (ROLE == 3) {
                ++hgen;
                handoff_piece<T, PD, KB0, KB1, PRIO, DROP>(L, PA2, L.Zh[p0], voff, lane, aph, hs, hgen,
                                                           GPAD_STAMP_PTR(7));
                prefetch(PA1);
            } else {
                GPAD_PRELUDE_LO();
            }
            GPAD_STAMP_AT(5);
            GPAD_PRELUDE_HI();
            __syncthreads();
            GPAD_STAMP_FLUSH();
            if (!chk && v < a.v_end) continue;

            // ---- Algorithm 1 test per column: every wave reduces the tile partials of all the
            // item's columns (lane 16 pp + cc <-> panel pp, column cc) and votes by ballot, so the
            // outcome is uniform across the workgroup without a second barrier ---------------------
            GPAD_PSTAMP_END(6);
            unsigned m1 = 0u, m2 = 0u;
            bool zh_out = true;  // this iteration's zhat still in L.Zh (no verification GEMM ran)
            if (chk) {
                int st1 = 0;
                float4 red;
                double gq;
                panel2_reduce<T>(L.slots, lane, red, gq);
                // the pair layout re-reads the test's doubles here (kargs) rather than keeping them
                // in SGPRs across the loop: fewer spilled SGPRs reloaded in its loop (the one-panel
                // roles keep them: re-reading moved their spills to scratch)
                double tL, ttol, ttg;
                if constexpr (KQ > 0) {
                    KernArgs& A = kargs();
                    tL = A.L;
                    ttol = A.tol;
                    ttg = A.tol_gap;
                } else {
                    tL = a.L;
                    ttol = a.tol;
                    ttg = a.tol_gap;
                }
                if (lane < 32 && ((live >> lane) & 1u))
                    st1 = ((double)red.x * tL <= ttol ? 1 : 0) |
                          ((viol_ok((double)red.y, (double)red.z, tL, ttol, ViolMargin<float>::value) &&
                            (red.w >= 0.0f) && (gq * tL <= ttg)) ? 2 : 0);
                const unsigned mA = (unsigned)__ballot(st1 & 1);
                m2 = (unsigned)__ballot(st1 & 2);
                GPAD_PSTAMP_END(7);
                if (mA) {  // (A) nominated for some column of the item: G_L z of both panels
                    zh_out = false;
                    if constexpr (NU > 0) {
#pragma unroll
                        for (int q = 0; q < Q; ++q) {
                            const int bit = 16 * (p0 + q) + c;
                            if (act[q] && ((m2 >> bit) & 1u)) {  // test (B)'s zhat out before z replaces it
                                const float4 h4 = L.Zh[p0 + q][slot];
                                const float zh[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const int i = 16 * t + 4 * r + j;
                                    if (i < n) a.z[(size_t)inst[q] * n + i] = zh[r];
                                }
                            }
                            L.Zh[p0 + q][slot] = make_float4(z[q][0], z[q][1], z[q][2], z[q][3]);
                        }
                    }
                    __syncthreads();
                    if constexpr (NU > 0) {
                        f32x4 cz[2];
                        panel_gemm2<T, NU == 2>(PA2, L.Zh[p0], L.Zh[NU == 2 ? 1 : p0], voff, lane, cz[0], cz[1]);
#pragma unroll
                        for (int q = 0; q < Q; ++q) {
                            const bool nom = act[q] && ((mA >> (16 * (p0 + q) + c)) & 1u);
                            const float4 p4 = L.Pd[p0 + q][slot];
                            const float pd[4] = {p4.x, p4.y, p4.z, p4.w};
                            float vc = -INFINITY, mc = 0.0f;
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                if (nom && (16 * t + 4 * r + j) < m) {
                                    u[q][r] = cz[q][r];  // the recursion restarts from the direct value
                                    vc = fmaxf(vc, cz[q][r] + pd[r]);
                                    mc = fmaxf(mc, __builtin_fabsf(cz[q][r]) + __builtin_fabsf(pd[r]));
                                }
                            }
                            vc = bfly<32>(bfly<16>(vc, OpMax{}), OpMax{});
                            mc = bfly<32>(bfly<16>(mc, OpMax{}), OpMax{});
                            if (j == 0)  // the stage-1 reads of every wave precede the barrier above
                                L.slots[p0 + q][t].f[c] = make_float4(vc, vc, mc, INFINITY);
                        }
                    }
                    __syncthreads();
                    bool ver = false;
                    float4 vred;
                    double vgap;
                    panel2_reduce<T>(L.slots, lane, vred, vgap);
                    if (lane < 32 && ((mA >> lane) & 1u))
                        ver = viol_ok((double)vred.x, (double)vred.z, tL, ttol, ViolMargin<float>::value);
                    m1 = (unsigned)__ballot(ver);
                    m2 &= ~m1;
                }
                GPAD_PSTAMP_END(8);
            }
            // ---- finished columns: results out ---------------------------------------------
            // (r09) nothing finished and the run goes on -- m1, m2, v are uniform over the workgroup: skip
            // results-out.  Before, every test ran its selects, row pointers and the LDS transposes of
            // both stores with every lane masked off: ~17 of phase 1's 26 tests at C4.
            if ((m1 | m2) == 0u && v < N) {
                if (v >= a.v_end) break;
                continue;
            }
            if constexpr (NU > 0) {
                // values and row pointers first, the stores after (see the phase-end park below)
                bool out[Q];
                int cd[Q];
                float zo[Q][4];
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const int bit = 16 * (p0 + q) + c;
                    cd[q] = ((m1 >> bit) & 1u) ? 1 : (((m2 >> bit) & 1u) ? 2 : 0);
                    out[q] = act[q] && (cd[q] != 0 || v >= N);
                    const float4 h4 = L.Zh[p0 + q][slot];
                    const bool use_zh = cd[q] == 2;
                    zo[q][0] = use_zh ? h4.x : z[q][0];
                    zo[q][1] = use_zh ? h4.y : z[q][1];
                    zo[q][2] = use_zh ? h4.z : z[q][2];
                    zo[q][3] = use_zh ? h4.w : z[q][3];
                }
#pragma unroll
                for (int q = 0; q < Q; ++q) {  // (Zh's block is free again: the rows4 transpose)
                    int iq = inst[q], ln = lane;
                    asm volatile("" : "+v"(iq), "+v"(ln));  // (no hoisted row pointers / offsets: rows4 note)
                    const size_t b = (size_t)iq;
                    float* const st = reinterpret_cast<float*>(&L.Zh[p0 + q][64 * t]);
                    const bool zw = cd[q] != 2 || zh_out;  // (B)'s zhat already out before (A)'s GEMM
                    KernArgs& A = kargs();
                    rows4_store(A.z + b * n, t, n, vec_io, st, ln, zo[q], out[q] && zw);
                    rows4_store(A.y + b * m, t, m, vec_io, st, ln, y[q], out[q]);
                    if (out[q]) {
                        if (t == 0 && j == 0) {
                            A.iters[iq] = v;
                            A.conv[iq] = cd[q];
                        }
                        act[q] = false;
                    }
                }
            }
            GPAD_PSTAMP_END(9);
            live &= ~(m1 | m2);
            if (v >= N) live = 0u;
            if (v >= a.v_end || live == 0u) break;
        }
        GPAD_PRELUDE_LO();  // (the loop's last barrier left every wave at priority 2)
        // ---- phase end: park the survivors -----------------------------------------------
        GPAD_PSTAMP(3);
        if constexpr (NU > 0) {
            if (carry) {
                // the stores after every value they take (r05): vmcnt counts stores on gfx9, so a
                // spill reload between stores would wait for all the stores before it
                bool pk[Q];
                float wv[Q][4];
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    pk[q] = act[q] && v >= a.v_end;
                    const float4 w4 = L.Wl[p0 + q][slot];
                    wv[q][0] = w4.x;
                    wv[q][1] = w4.y;
                    wv[q][2] = w4.z;
                    wv[q][3] = w4.w;
                }
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    int iq = inst[q], ln = lane;
                    asm volatile("" : "+v"(iq), "+v"(ln));  // (no hoisted row pointers / offsets: rows4 note)
                    const size_t b = (size_t)iq;
                    float* const st = reinterpret_cast<float*>(&L.Zh[p0 + q][64 * t]);
                    KernArgs& A = kargs();
                    rows4_store(A.z + b * n, t, n, vec_io, st, ln, z[q], pk[q]);
                    rows4_store(A.y + b * m, t, m, vec_io, st, ln, y[q], pk[q]);
                    rows4_store(A.wc + b * m, t, m, vec_io, st, ln, wv[q], pk[q]);
                    if (use_tol) rows4_store(A.uc + b * m, t, m, vec_io, st, ln, u[q], pk[q]);
                }
                if (t == 0) {  // the tile-0 owner of each panel lists its survivors
#pragma unroll
                    for (int q = 0; q < Q; ++q) {
                        int iq = inst[q], ln = lane;
                        asm volatile("" : "+v"(iq), "+v"(ln));
                        list_survivors(kargs(), pair ? 2 * it + p0 + q : it, pk[q], iq, ln, ln >> 4);
                    }
                }
            }
        }
        GPAD_PSTAMP(4);
        __syncthreads();
        GPAD_PSTAMP(5);
    }
    if (a.gmax_part) {  // this wave's max |g| -> L.gred (reduced by the kernel at exit)
        for (int o = 32; o > 0; o >>= 1) gmx = absmax_nan(gmx, __shfl_xor(gmx, o, 64));
        if (lane == 0) L.gred[threadIdx.x >> 6] = gmx;
    }
}
}  // namespace gpad
