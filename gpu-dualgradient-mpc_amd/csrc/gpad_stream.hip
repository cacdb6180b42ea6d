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
    double* zp;   // [ldn] z(y+) of the dual function (value-function branches only)
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

// LDS bytes of the stream kernel: the vectors, the test slots and (value branches) the block-sum
// partials and z(y+)
template <typename T>
size_t stream_lds_bytes(int ldn, int ldm, bool value) {
    return sizeof(T) * (size_t)(3 * ldn + 4 * ldm) + sizeof(CheckSlot) * 2 * (kStreamBlock / 64) +
           (value ? sizeof(double) * (size_t)(kStreamBlock / 64 + ldn) : 0);
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

template <typename T>
__global__ __launch_bounds__(kStreamBlock) void gpad_stream_kernel(SolveArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int n = a.n, m = a.m, ldn = a.ldn, ldm = a.ldm;
    const StreamLds<T> s = stream_lds<T>(smem, ldn, ldm);
    const T* __restrict__ MGt = a.MGt + (size_t)b * a.strideA;
    const T* __restrict__ GLt = a.GLt + (size_t)b * a.strideB;
    T* zg = a.z + (size_t)b * n;
    T* yg = a.y + (size_t)b * m;
    const T* gPg = a.gP + (size_t)b * a.ld_gP;
    const T* gg = a.g + (size_t)b * a.ld_g;
    const T beta0 = a.beta[0];

    for (int i = tid; i < ldn; i += kStreamBlock) {
        s.zs[i] = i < n ? zg[i] : T(0);
        s.gp[i] = i < n ? gPg[i] : T(0);
        s.zh[i] = T(0);
    }
    for (int i = tid; i < ldm; i += kStreamBlock) {
        const T yv = i < m ? yg[i] : T(0);
        s.ys[i] = yv;
        s.pd[i] = i < m ? (T)(a.gscale * (double)gg[i]) : T(0);
        s.w[i] = fmad(beta0, yv - yv, yv);  // 8a with y_0 = y_{-1} (acceldualgrad.m:16,43)
    }
    __syncthreads();
    const bool use_tol = a.tol > 0.0;
    if (use_tol) {  // u = G_L z_{-1}; afterwards u follows the 8c recursion (u = G_L z exactly)
        for (int r0 = 4 * tid; r0 < m; r0 += 4 * kStreamBlock) {
            T c[4] = {T(0), T(0), T(0), T(0)};
            chain4<T>(GLt, ldm, r0, s.zs, n, c);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (r0 + r < m) s.us[r0 + r] = c[r];
        }
    }

    const int nwaves = kStreamBlock / 64;
    int it = 0;
    int done = 0;
    for (int v = 0; v < a.N; ++v) {
        const T th = a.theta[v];
        const T omt = T(1) - th;
        const T bnext = a.beta[v + 1];
        // ---- phase 1: 8b + 8c, rows of -ML ----------------------------------------------
        for (int r0 = 4 * tid; r0 < n; r0 += 4 * kStreamBlock) {
            T acc[4] = {T(0), T(0), T(0), T(0)};
            chain4<T>(MGt, ldn, r0, s.w, m, acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = r0 + r;
                if (i < n) {
                    const T zhv = acc[r] - s.gp[i];                 // seq_functions.cpp:63
                    s.zh[i] = zhv;
                    s.zs[i] = fmad(omt, s.zs[i], th * zhv);         // seq_functions.cpp:70
                }
            }
        }
        __syncthreads();
        // ---- phase 2: 8d + next 8a, rows of G/L ------------------------------------------
        // (own text of gpad_chain.h's row step and test terms: slower through them, r19_row_test_noreg.txt)
        const bool chk = use_tol && ((v + 1) % a.check_every) == 0;
        T violz = neg_inf<T>(), violh = neg_inf<T>(), wmin = -neg_inf<T>(), magh = T(0);
        double gap = 0.0;
        for (int r0 = 4 * tid; r0 < m; r0 += 4 * kStreamBlock) {
            T c[4] = {T(0), T(0), T(0), T(0)};
            chain4<T>(GLt, ldm, r0, s.zh, n, c);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = r0 + r;
                if (i < m) {
                    const T wi = s.w[i], pdi = s.pd[i], yi = s.ys[i];
                    const T sv = (wi + pdi) + c[r];                 // seq_functions.cpp:84
                    const T yp = (absd(sv) + sv) * T(0.5);          // seq_functions.cpp:85
                    if (use_tol) {
                        const T ui = fmad(omt, s.us[i], th * c[r]);  // u = G_L z (8c form)
                        s.us[i] = ui;
                        if (chk) {
                            const T t = c[r] + pdi;
                            violh = fmax(violh, t);
                            magh = fmax(magh, absd(c[r]) + absd(pdi));
                            wmin = fmin(wmin, wi);
                            gap -= (double)wi * (double)t;
                            violz = fmax(violz, ui + pdi);
                        }
                    }
                    s.w[i] = fmad(bnext, yp - yi, yp);               // next 8a
                    s.ys[i] = yp;
                }
            }
        }
        if (chk) check_publish<T>(s.slots, violz, violh, wmin, gap, magh);
        __syncthreads();
        it = v + 1;
        if (chk) {
            const int st1 = check_stage1<T>(s.slots, nwaves, a.L, a.tol, a.tol_gap);
            bool verified = false;
            if (st1 & 1) {  // (A) nominated: decide on the direct chain G_L z, reset u to it
                T vc = neg_inf<T>(), mc = T(0);
                for (int r0 = 4 * tid; r0 < m; r0 += 4 * kStreamBlock) {
                    T c[4] = {T(0), T(0), T(0), T(0)};
                    chain4<T>(GLt, ldm, r0, s.zs, n, c);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = r0 + r;
                        if (i < m) {
                            s.us[i] = c[r];
                            vc = fmax(vc, c[r] + s.pd[i]);
                            mc = fmax(mc, absd(c[r]) + absd(s.pd[i]));
                        }
                    }
                }
                check_publish<T>(s.slots + nwaves, vc, vc, vc, 0.0, mc);
                __syncthreads();
                verified = check_verify<T>(s.slots + nwaves, nwaves, a.L, a.tol);
            }
            done = check_code(st1, verified);
            if (!done && a.Hq) {  // value-function branches where the MATLAB test reaches them
                double vh = -INFINITY, mh = 0.0, wm = INFINITY, gq = 0.0;
                for (int i = 0; i < nwaves; ++i) {
                    vh = fmax(vh, s.slots[i].violh);
                    mh = fmax(mh, s.slots[i].magh);
                    wm = fmin(wm, s.slots[i].wmin);
                    gq += s.slots[i].gap;
                }
                if (viol_ok(vh, mh, a.L, a.tol, ViolMargin<T>::value))  // uniform
                    done = stream_value_branch<T>(a, s, MGt, GLt, a.Hq + (size_t)b * a.strideHq, wm >= 0.0,
                                                  gq * a.L);
            }
        }
        if (done) break;
    }
    const T* zout = done >= 2 ? s.zh : s.zs;  // tests (B), (B'), (B'') certify zhat
    for (int i = tid; i < n; i += kStreamBlock) zg[i] = zout[i];
    for (int i = tid; i < m; i += kStreamBlock) yg[i] = s.ys[i];
    if (tid == 0) {
        a.iters[b] = it;
        a.conv[b] = done;
    }
}

template <typename T>
hipError_t launch_stream(const SolveArgs<T>& a, hipStream_t st) {
    const size_t lds = stream_lds_bytes<T>(a.ldn, a.ldm, a.Hq != nullptr);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)gpad_stream_kernel<T>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(gpad_stream_kernel<T>, dim3(a.batch), dim3(kStreamBlock), lds, st, a);
    return hipGetLastError();
}
template hipError_t launch_stream<float>(const SolveArgs<float>&, hipStream_t);
template hipError_t launch_stream<double>(const SolveArgs<double>&, hipStream_t);

}  // namespace gpad
