// gpad_stream.hip -- gpad_stream_kernel<T>, the generic fused GPAD solve kernel (gfx950, wave64): the
// whole iteration loop of main.cu:160-175 in ONE launch, f32 / f64, any n, m up to the LDS budget.
// One workgroup per instance; -ML and G/L are read every iteration from HBM/L2 in k-major layout,
// 4 rows per lane (one 16-B/32-B load per lane per k, fully coalesced), 8 k-steps in flight.
//
// Numerics (bit-exact with the reference CPU path, see oracle/gpad_oracle.h): every dot
// product is ONE sequential fmaf chain per output row, k = 0..K-1 from +0 -- exactly what
// seq_functions.cpp:61,82 compute under FMA contraction and what the reference's
// one-thread-per-row CUDA kernels compute (kernel_functions.cu:46-61,176-191).  Every unit is
// compiled with -ffp-contract=off; every fused multiply-add is an explicit __builtin_fma.
#include <hip/hip_runtime.h>

#include <cmath>

#include "gpad_chain.h"
#include "gpad_farkas.h"
#include "gpad_internal.h"

namespace gpad {

// =========================================================================================
// gpad_stream_kernel
// =========================================================================================
constexpr int kStreamBlock = 256;
static_assert(kStreamBlock / 64 <= 8, "test slots: one per lane over lanes 0..7 (gpad_chain.h check_stage1)");
constexpr int kUnrollK = 8;

template <typename T>
struct StreamLds {
    T *w, *zh, *zs, *ys, *gp, *pd, *us;
    CheckSlot* slots;
    double* red;  // [waves] block-sum partials of the value functions
    double* zp;   // [ldn] z(y+) of the dual function (value-function branches only); the certificate's
                  // variant, which excludes them: red = the nomination's wave partials of q, zp = t = G_L'y+
};

template <typename T>
__device__ __forceinline__ StreamLds<T> stream_lds(unsigned char* smem, int ldn, int ldm) {
    StreamLds<T> s;
    s.w = reinterpret_cast<T*>(smem);   // [ldm] current w (read by every lane in phase 1)
    s.zh = s.w + ldm;                   // [ldn] zhat (read by every lane in phase 2)
    s.zs = s.zh + ldn;                  // [ldn] z (averaged primal)
    s.ys = s.zs + ldn;                  // [ldm] y
    s.gp = s.ys + ldm;                  // [ldn] g_P
    s.pd = s.gp + ldn;                  // [ldm] p_D
    s.us = s.pd + ldm;                  // [ldm] u = G_L z (termination test, by recursion)
    s.slots = reinterpret_cast<CheckSlot*>(s.us + ldm);  // [2][waves]: test, verification of (A)
    s.red = reinterpret_cast<double*>(s.slots + 2 * (kStreamBlock / 64));
    s.zp = s.red + kStreamBlock / 64;
    return s;
}

// LDS bytes of the stream kernel: the vectors, the test slots and (value branches, or the infeasibility
// certificate) the block-sum partials and z(y+); the restart variant: the partials alone (red = the wave
// partials of its q)
template <typename T>
size_t stream_lds_bytes(int ldn, int ldm, bool value, bool restart = false) {
    return sizeof(T) * (size_t)(3 * ldn + 4 * ldm) + sizeof(CheckSlot) * 2 * (kStreamBlock / 64) +
           (value ? sizeof(double) * (size_t)(kStreamBlock / 64 + ldn)
                  : (restart ? sizeof(double) * (size_t)(kStreamBlock / 64) : 0));
}

// acc[r] = sum_k Mt[k*ld + r0 + r] * v[k], sequential in k, 4 rows per lane.
template <typename T>
__device__ __forceinline__ void chain4(const T* __restrict__ Mt, int ld, int r0, const T* v, int K,
                                       T (&acc)[4]) {
    using V = typename V4<T>::type;
    const T* col = Mt + r0;
    int k = 0;
    for (; k + kUnrollK <= K; k += kUnrollK) {
        V a[kUnrollK];
#pragma unroll
        for (int u = 0; u < kUnrollK; ++u) a[u] = *reinterpret_cast<const V*>(col + (size_t)(k + u) * ld);
#pragma unroll
        for (int u = 0; u < kUnrollK; ++u) {
            const T vk = v[k + u];
            acc[0] = fmad(a[u].x, vk, acc[0]);
            acc[1] = fmad(a[u].y, vk, acc[1]);
            acc[2] = fmad(a[u].z, vk, acc[2]);
            acc[3] = fmad(a[u].w, vk, acc[3]);
        }
    }
    for (; k < K; ++k) {
        const V a = *reinterpret_cast<const V*>(col + (size_t)k * ld);
        const T vk = v[k];
        acc[0] = fmad(a.x, vk, acc[0]);
        acc[1] = fmad(a.y, vk, acc[1]);
        acc[2] = fmad(a.z, vk, acc[2]);
        acc[3] = fmad(a.w, vk, acc[3]);
    }
}

// acc[r] = sum_k Mt[k*ld + r0 + r] * v[k] as fp64 fma chains (ascending k) over the run's own
// matrix and vector values: the products of the value-function branches
template <typename T, typename V>
__device__ __forceinline__ void chain4d(const T* __restrict__ Mt, int ld, int r0, const V* v, int K,
                                        double (&acc)[4]) {
    using W = typename V4<T>::type;
    const T* col = Mt + r0;
    for (int k = 0; k < K; ++k) {
        const W x = *reinterpret_cast<const W*>(col + (size_t)k * ld);
        const double vk = (double)v[k];
        acc[0] = __builtin_fma((double)x.x, vk, acc[0]);
        acc[1] = __builtin_fma((double)x.y, vk, acc[1]);
        acc[2] = __builtin_fma((double)x.z, vk, acc[2]);
        acc[3] = __builtin_fma((double)x.w, vk, acc[3]);
    }
}

// sum over the workgroup (every thread gets it): wave sums, then the waves' partials in order
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < kStreamBlock / 64; ++i) t += red[i];
    __syncthreads();  // red is reused by the next sum
    return t;
}

// valuefcn V(x) = sum_i (x_i / 2 + M_i) (H x)_i (acceldualgrad.m:30 with f = H M)
template <typename T, typename V>
__device__ __forceinline__ double stream_valuefcn(const T* __restrict__ Hq, int ldn, int n, const V* x, const T* gp,
                                                  double* red) {
    double part = 0.0;
    for (int r0 = 4 * threadIdx.x; r0 < n; r0 += 4 * kStreamBlock) {
        double hx[4] = {0.0, 0.0, 0.0, 0.0};
        chain4d<T, V>(Hq, ldn, r0, x, n, hx);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r0 + r < n) part += (0.5 * (double)x[r0 + r] + (double)gp[r0 + r]) * hx[r];
    }
    return block_sum(part, red);
}

// The value-function branches of Algorithm 1 (acceldualgrad.m:73,76), reached after test (B)'s
// violation part passed (w_ok: w >= 0 with the gap term above e_V, else w not >= 0); the same
// fp64 quantities as orc_value_branch_f32 / _f64 (oracle/gpad_oracle.c).  Returns 3, 4 or 0.
template <typename T>
__device__ int stream_value_branch(const SolveArgs<T>& a, const StreamLds<T>& s, const T* __restrict__ MGt,
                                   const T* __restrict__ GLt, const T* __restrict__ Hq, bool w_ok, double gapL) {
    const int n = a.n, m = a.m, ldn = a.ldn, ldm = a.ldm;
    const double eV = a.tol_gap;
    const double V = stream_valuefcn<T, T>(Hq, ldn, n, s.zh, s.gp, s.red);
    if (w_ok) return gapL <= V * eV / (1.0 + eV) ? 3 : 0;  // :73
    // dualfcn(y+) = V(z(y+)) + y+'(G z(y+) - g), z(y+) = -ML y+ - M       (:31-33, :76)
    for (int r0 = 4 * threadIdx.x; r0 < n; r0 += 4 * kStreamBlock) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        chain4d<T, T>(MGt, ldn, r0, s.ys, m, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r0 + r < n) s.zp[r0 + r] = acc[r] - (double)s.gp[r0 + r];
    }
    __syncthreads();
    const double Vp = stream_valuefcn<T, double>(Hq, ldn, n, s.zp, s.gp, s.red);
    double lin = 0.0;
    for (int r0 = 4 * threadIdx.x; r0 < m; r0 += 4 * kStreamBlock) {
        double c[4] = {0.0, 0.0, 0.0, 0.0};
        chain4d<T, double>(GLt, ldm, r0, s.zp, n, c);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r0 + r < m) lin += (double)s.ys[r0 + r] * (c[r] + (double)s.pd[r0 + r]);
    }
    const double D = Vp + a.L * block_sum(lin, s.red);
    return V - D <= eV * (D > 1.0 ? D : 1.0) ? 4 : 0;  // :76
}

// the three variants of the kernel (gpad_stream_solve.inc)
#define GPAD_STREAM_RS 0
#define GPAD_STREAM_FK 0
#include "gpad_stream_solve.inc"
#undef GPAD_STREAM_FK
#define GPAD_STREAM_FK 1
#include "gpad_stream_solve.inc"
#undef GPAD_STREAM_FK
#undef GPAD_STREAM_RS
#define GPAD_STREAM_RS 1
#define GPAD_STREAM_FK 0
#include "gpad_stream_solve.inc"
#undef GPAD_STREAM_FK
#undef GPAD_STREAM_RS

// fk: the infeasibility certificate of this run, or null (the kernel without it); rs: its adaptive restart
// (rs->R >= 1, rs->count [batch]), or null -- not both, and neither with the value-function branches
template <typename T>
hipError_t launch_stream(const SolveArgs<T>& a, hipStream_t st, const FarkasArgs* fk, const RestartArgs* rs) {
    const size_t lds = stream_lds_bytes<T>(a.ldn, a.ldm, a.Hq != nullptr || fk != nullptr, rs != nullptr);
    if (lds > 160 * 1024 || (fk && a.Hq) || (rs && (fk || a.Hq || rs->R < 1 || !rs->count)))
        return hipErrorInvalidValue;
    const void* fn = rs   ? (const void*)gpad_stream_restart_kernel<T>
                     : fk ? (const void*)gpad_stream_farkas_kernel<T>
                          : (const void*)gpad_stream_kernel<T>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    if (rs)
        hipLaunchKernelGGL(gpad_stream_restart_kernel<T>, dim3(a.batch), dim3(kStreamBlock), lds, st, a, *rs);
    else if (fk)
        hipLaunchKernelGGL(gpad_stream_farkas_kernel<T>, dim3(a.batch), dim3(kStreamBlock), lds, st, a, *fk);
    else
        hipLaunchKernelGGL(gpad_stream_kernel<T>, dim3(a.batch), dim3(kStreamBlock), lds, st, a);
    return hipGetLastError();
}
template hipError_t launch_stream<float>(const SolveArgs<float>&, hipStream_t, const FarkasArgs*, const RestartArgs*);
template hipError_t launch_stream<double>(const SolveArgs<double>&, hipStream_t, const FarkasArgs*,
                                          const RestartArgs*);

// r_i = sum_k |G_L[i][k]| of every bound image, fp64, k ascending (the certificate's s term)
template <typename T>
__global__ void farkas_rows_kernel(const T* __restrict__ GLt, int n, int m, int ldm, double* __restrict__ rabs) {
    const T* img = GLt + (size_t)blockIdx.y * n * ldm;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ldm) return;
    double acc = 0.0;
    if (i < m)
        for (int k = 0; k < n; ++k) acc += __builtin_fabs((double)img[(size_t)k * ldm + i]);
    rabs[(size_t)blockIdx.y * ldm + i] = acc;
}
hipError_t launch_farkas_rows(const void* GLt, int f64, int n, int m, int ldm, int copies, double* rabs,
                              hipStream_t s) {
    const dim3 grid((ldm + 255) / 256, copies);
    if (f64)
        hipLaunchKernelGGL(farkas_rows_kernel<double>, grid, dim3(256), 0, s, (const double*)GLt, n, m, ldm, rabs);
    else
        hipLaunchKernelGGL(farkas_rows_kernel<float>, grid, dim3(256), 0, s, (const float*)GLt, n, m, ldm, rabs);
    return hipGetLastError();
}

}  // namespace gpad
