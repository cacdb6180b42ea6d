// gpad_compact.hip -- the boundary between two phases of a phased panel solve (gpad_phases.cpp):
// one workgroup densifies the per-panel survivor lists and orders the finisher's queue.
#include <hip/hip_runtime.h>

#include "gpad_internal.h"

namespace gpad {

// Phase boundary (launch_phase_compact): the survivors the previous phase listed per panel
// (list_survivors: seg_cnt[P], seg_idx[16 P + rank]) become the dense list idx[0 .. count) of the
// next phase.  One workgroup: thread t owns a contiguous run of panels, an LDS scan of the
// per-thread totals gives each run its base, and the run's entries are copied in panel order.
//
// When the list is the finisher's (count <= fin_cur) and the previous solve's counts are known
// (pred), it is then reordered longest-predicted-first so the duo kernel's queue starts the
// longest remaining solves first (list scheduling, LPT): a counting sort on the counts (4096
// bins, larger counts share the last) -- histogram, descending exclusive scan, scatter.  The order
// inside a bin is arbitrary; results never depend on the order, only the schedule does.
constexpr int kSortMax = 8192;
constexpr int kSortBins = 4096;
// exclusive scan over 1024 threads: an inclusive scan inside each wave (six shuffles), then the 16
// wave totals through LDS -- two barriers (r06; the LDS Hillis-Steele scan before it took twenty)
__device__ __forceinline__ int block_scan_1024(int* part, int tid, int v) {
    const int lane = tid & 63, w = tid >> 6;
    int x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == 63) part[w] = x;
    __syncthreads();
    int wb = 0;
    for (int i = 0; i < w; ++i) wb += part[i];
    __syncthreads();  // (the caller's next scan rewrites part)
    return wb + x - v;
}

constexpr int kCompactMaxPanels = 8192;  // per-panel bases in LDS up to here (131072 instances)
constexpr int kCompactU = 8;             // entries per thread and round: loads issued together
__global__ __launch_bounds__(1024) void phase_compact_kernel(const int* __restrict__ seg_cnt,
                                                             const int* __restrict__ seg_idx, const int* count_prev,
                                                             int batch, int fin_prev, int* idx, int* count_out,
                                                             const int* pred, int fin_cur) {
    __shared__ int hist[kSortBins];
    __shared__ int ids[kSortMax];
    __shared__ int part[1024];
    __shared__ int pbase[kCompactMaxPanels];
    __shared__ int pcnt[kCompactMaxPanels];
    __shared__ int total_l;
    const int tid = threadIdx.x;
    // the thread -> panel runs from the batch's panel count, so the per-panel counts load together
    // with count_prev (one round trip, not two); panels past the previous phase's count as 0
    const int pmax = (batch + 15) / 16;
    const int per = (pmax + 1023) / 1024;
    const int p0 = tid * per < pmax ? tid * per : pmax, p1 = p0 + per < pmax ? p0 + per : pmax;
    constexpr int kPer = 8;  // counts held in registers per thread (pmax <= 8192 panels)
    int cl[kPer];
#pragma unroll
    for (int u = 0; u < kPer; ++u) cl[u] = (per <= kPer && p0 + u < p1) ? seg_cnt[p0 + u] : 0;
    const int prev = count_prev ? *count_prev : batch;
    if (count_prev && prev <= fin_prev) {  // the finisher took the previous list: nothing was listed
        if (tid == 0) *count_out = 0;
        return;
    }
    const int panels = (prev + 15) / 16;
    const bool lds_bases = panels <= kCompactMaxPanels;
    const int q1 = p1 < panels ? p1 : panels;  // this thread's panels of the previous phase: [p0, q1)
    int sum = 0;
    if (per <= kPer) {
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            if (p0 + u < q1) {
                if (lds_bases) pcnt[p0 + u] = cl[u];
                sum += cl[u];
            }
        }
    } else {
        for (int p = p0; p < q1; ++p) {
            const int c = seg_cnt[p];
            if (lds_bases) pcnt[p] = c;
            sum += c;
        }
    }
    int base = block_scan_1024(part, tid, sum);
    if (tid == 1023) total_l = base + sum;
    if (lds_bases) {
        for (int p = p0; p < q1; ++p) {
            const int c = pcnt[p];
            pbase[p] = c ? base : -1;
            base += c;
        }
    }
    __syncthreads();
    const int count = total_l;
    const bool sort = pred && count > 1 && count <= fin_cur && count <= kSortMax;
    int* dst = sort ? ids : idx;
    if (lds_bases) {  // entry r of panel p by thread (16 p + r) mod 1024: coalesced loads, kCompactU of
        // them in flight per thread before any store (one L2 round trip per round, not per entry)
        for (int i0 = tid; i0 < 16 * panels; i0 += 1024 * kCompactU) {
            int v[kCompactU], at[kCompactU];
#pragma unroll
            for (int u = 0; u < kCompactU; ++u) {
                const int i = i0 + 1024 * u;
                at[u] = -1;
                v[u] = 0;
                if (i < 16 * panels) {
                    const int p = i >> 4, r = i & 15, b = pbase[p];
                    if (b >= 0 && r < pcnt[p]) {
                        at[u] = b + r;
                        v[u] = seg_idx[i];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < kCompactU; ++u)
                if (at[u] >= 0) dst[at[u]] = v[u];
        }
    } else {
        for (int p = p0; p < q1; ++p) {
            const int c = seg_cnt[p];
            for (int r = 0; r < c; ++r) dst[base + r] = seg_idx[16 * p + r];
            base += c;
        }
    }
    if (tid == 0) *count_out = count;
    if (!sort) return;
    __syncthreads();  // ids complete
    // the bins of this thread's entries (count <= kSortMax = 8 x 1024: one predicted count per entry,
    // loaded once, used by the histogram and the scatter)
    int bn[kSortMax / 1024];
#pragma unroll
    for (int u = 0; u < kSortMax / 1024; ++u) {
        const int i = tid + 1024 * u;
        bn[u] = 0;
        if (i < count) {
            const int q = pred[ids[i]];  // descending count -> ascending bin
            const int k = q < 0 ? 0 : (q >= kSortBins ? kSortBins - 1 : q);
            bn[u] = kSortBins - 1 - k;
        }
    }
    for (int i = tid; i < kSortBins; i += 1024) hist[i] = 0;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kSortMax / 1024; ++u)
        if (tid + 1024 * u < count) atomicAdd(&hist[bn[u]], 1);  // (LDS atomics)
    __syncthreads();
    int local[4], hs = 0;  // thread tid owns bins 4 tid .. 4 tid + 3
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        local[q] = hs;
        hs += hist[4 * tid + q];
    }
    const int hb = block_scan_1024(part, tid, hs);
#pragma unroll
    for (int q = 0; q < 4; ++q) hist[4 * tid + q] = hb + local[q];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kSortMax / 1024; ++u) {
        const int i = tid + 1024 * u;
        if (i < count) idx[atomicAdd(&hist[bn[u]], 1)] = ids[i];
    }
}

hipError_t launch_phase_compact(const int* seg_cnt, const int* seg_idx, const int* count_prev, int batch,
                                int fin_prev, int* idx_out, int* count_out, const int* pred, int fin_cur,
                                hipStream_t s) {
    hipLaunchKernelGGL(phase_compact_kernel, dim3(1), dim3(1024), 0, s, seg_cnt, seg_idx, count_prev, batch,
                       fin_prev, idx_out, count_out, pred, fin_cur);
    return hipGetLastError();
}

}  // namespace gpad
