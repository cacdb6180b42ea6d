// gpad_farkas.h -- the infeasibility certificate (include/gpad.h gpad_setup_infeasibility): what a kernel
// that carries it reads beyond its SolveArgs, and the decision.
//
// For y >= 0 and any z with |z|_inf <= R:  y'(G z - g) >= -(g'y) - R |G'y|_1, so g'y + R |G'y|_1 < 0 proves
// that no z of the box satisfies G z <= g: the dual iterate is its own Farkas certificate.  On the device's
// data, G_L = G/L and pD = -g/L (the factor 1/L > 0 drops out):
//   nomination (in the test epilogue's reduction, at the iterations v with v % (4 check_every) == 0, after
//     Algorithm 1 found no code):  q = sum_i (double)y+_i (double)pD_i > 0
//   decision (fp64, i and j ascending, products and sums unfused):
//     t_j = sum_i y+_i G_L[i][j],  a = sum_j |t_j|,  p = sum_i |y+_i pD_i|,  s = sum_i y+_i r_i with
//     r_i = sum_j |G_L[i][j]| (launch_farkas_rows, once per bound matrix, for the stream kernel; the panels sum
//     the same r_i from their fragment image at a decision, farkas_decide_panel);
//     infeasible  <=>  q - R a > mu (p + R s),  mu = ViolMargin (16 units of 2^-24 / 2^-53): the roundings of
//     G/L and -g/L and the fp64 sums, so the certificate holds on the caller's own G, g (gpad_farkas_margin).
// Code 5 returns z* = z (as the cap exit), y* = y+ and the iteration count.  The rule keeps no state between
// events.  Six kernels carry it, each as a second variant of its one text: gpad_stream_farkas_kernel,
// gpad_panel_farkas_kernel, gpad_loop_panel_farkas_kernel, gpad_resident_farkas_kernel (opt-in per handle,
// gpad_infeasibility_resident), gpad_loop_farkas_kernel and gpad_loop_fleet_farkas_kernel (the asynchronous loop,
// opt-in per handle, gpad_infeasibility_loop_async).  Kernels without it never see a bound: the host routes (gpad_run.cpp launch_solve,
// gpad_state.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include "gpad_internal.h"

namespace gpad {

constexpr int kCodeInfeasible = 5;  // GPAD_CODE_INFEASIBLE

struct FarkasArgs {
    const double* rabs;  // [copies][ldm] r_i of each bound G_L image
    long long stride;    // elements between consecutive instances' r (0 = shared)
    double R;            // the caller's bound on |z|_inf, > 0
};

// r[i] = sum_k |GLt[k ldm + i]| (k ascending, fp64) for every image: GLt k-major [n][ldm] per copy
hipError_t launch_farkas_rows(const void* GLt, int f64, int n, int m, int ldm, int copies, double* rabs, hipStream_t s);
// gpad_resident_farkas.hip: one launch of the (ka, kb) bucket pair's gpad_resident_farkas_kernel (launch_resident)
hipError_t launch_resident_farkas(const SolveArgs<float>& a, const FarkasArgs& fk, int ka, int kb, int threads,
                                  hipStream_t s);

#ifdef __HIPCC__
// The decision for a workgroup that holds y+ and pD of one instance in LDS.  Every thread calls it with the
// same q (two barriers inside) and gets the same answer.  t: LDS scratch of n doubles.  Every thread repeats
// the serial sums a, p, s, and a t_j is one thread's serial loop: acceptable only because the event is rare
// (nominated instances at every fourth test), and it needs no broadcast.
template <typename T>
__device__ inline bool farkas_decide(const T* __restrict__ GLt, int ldm, int n, int m, const T* y, const T* pd,
                                     const double* __restrict__ rabs, double R, double q, double* t) {
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const T* col = GLt + (size_t)j * ldm;
        double acc = 0.0;
        for (int i = 0; i < m; ++i) acc += (double)y[i] * (double)col[i];
        t[j] = acc;
    }
    __syncthreads();
    double a = 0.0, p = 0.0, s = 0.0;
    for (int j = 0; j < n; ++j) a += __builtin_fabs(t[j]);
    for (int i = 0; i < m; ++i) {
        const double yi = (double)y[i];
        p += __builtin_fabs(yi * (double)pd[i]);
        s += yi * rabs[i];
    }
    __syncthreads();  // t is free again
    return q - R * a > ViolMargin<T>::value * (p + R * s);
}

// ---- the MFMA panels (gpad_panel.hip, gpad_loop_panel.hip): a workgroup of 64 T threads decides one column ----
// element (i, j) of a matrix in the T x T-tile fragment image of gpad_panel.h (zero beyond its rows / columns)
__device__ __forceinline__ float frag_at(const float* __restrict__ F, int T, int i, int j) {
    const int ri = i & 15, rho = (ri >> 2) + 4 * (ri & 3);  // pi16(rho) = ri
    const int lane = ((j & 3) << 4) + rho;
    return F[((((size_t)(j >> 4)) * T + (i >> 4)) * 64 + lane) * 4 + ((j & 15) >> 2)];
}
// row i of column cc in a [T][64][4] LDS tile (fragment order: register r of lane (jg, cc) <-> row 16 t + 4 r + jg)
__device__ __forceinline__ float tile_at(const float* L, int i, int cc) {
    return L[(((i >> 4) * 64) + ((i & 3) << 4) + cc) * 4 + ((i & 15) >> 2)];
}
// The decision for column cc, by every thread of the workgroup with the same arguments (two barriers inside)
// and the same answer.  F2: the G_L fragment image, Pd: the p_D tile, yc: y+ of the column (global, written
// before the last barrier), tb: LDS scratch of n + m doubles (t, then r).
template <int T>
__device__ inline bool farkas_decide_panel(const float* __restrict__ F2, const float* Pd, int cc, const float* yc, int n,
                                           int m, double R, double q, double* tb) {
    for (int w = threadIdx.x; w < n + m; w += 64 * T) {
        double acc = 0.0;
        if (w < n) {
            for (int i = 0; i < m; ++i) acc += (double)yc[i] * (double)frag_at(F2, T, i, w);
        } else {
            for (int jj = 0; jj < n; ++jj) acc += __builtin_fabs((double)frag_at(F2, T, w - n, jj));
        }
        tb[w] = acc;
    }
    __syncthreads();
    double a = 0.0, p = 0.0, s = 0.0;
    for (int jj = 0; jj < n; ++jj) a += __builtin_fabs(tb[jj]);
    for (int i = 0; i < m; ++i) {
        const double yi = (double)yc[i];
        p += __builtin_fabs(yi * (double)tile_at(Pd, i, cc));
        s += yi * tb[n + i];
    }
    __syncthreads();  // tb is free again
    return q - R * a > ViolMargin<float>::value * (p + R * s);
}
#endif

}  // namespace gpad
