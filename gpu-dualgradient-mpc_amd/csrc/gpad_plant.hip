// gpad_plant.hip -- per-state QP data and plant update on the device.
//
// The reference rebuilds the state-dependent QP data on the host for every MPC step
// (gpad.m:80-85: f = x0'F, b_i(x0)) and then runs GPAD (acceldualgrad.m:20-23 precompute,
// :38-64 loop).  For an LTI plant both vectors are affine in the state x:
//     M(x) = M0 + PM x        (n;  PM = H^-1 F', so M = H^-1 f'   -- acceldualgrad.m:21)
//     g(x) = g0 + Pg x        (m;  b_i(x), gpad.m:85)
// and the receding-horizon update is x+ = A x + B u with u = z*[0:nu] (gpad.m:91-93).
// These kernels evaluate both on the device so a batch of states (or a whole closed-loop
// simulation) never leaves HBM.
//
// Arithmetic (restated by oracle/gpad_oracle.c orc_affine / orc_plant_step, bit-exact):
//   affine:  acc = c0[i] (0 if absent); for k < nx: acc = fma(P[i][k], x[k], acc)
//   plant :  acc = 0;  for k < nx: acc = fma(A[i][k], x[k], acc);
//                      for j < nu: acc = fma(B[i][j], u[j], acc)
// The work is O(batch (n + m) nx) per step -- a few hundred flops per instance against the
// O(iterations n m) of the solve -- so one thread per output row with the short chain in
// registers is the right shape; P rows are re-read from L2 by every instance.
//
// Every map has an element stride between consecutive instances' copies (gpad_setup_plant_batch);
// 0 = one map for the batch (gpad_setup_plant).  The stride only moves the row an instance reads:
// the chain above is the same, so stride 0 gives the shared binding's bits.
#include "gpad_internal.h"

namespace gpad {

// out1[b][i] = affine row i (i < rows1) ; out2[b][j] = affine row j (j < rows2).
// grid.x covers the rows of one instance, grid.y the instances (grid-stride beyond 65535):
// no integer division on the path, the state x[b] is a broadcast read per block.
// sP*, sc*: elements between consecutive instances' P / c (0 = shared).
template <typename T>
__global__ __launch_bounds__(256) void affine2_kernel(const T* __restrict__ P1, const T* __restrict__ c1,
                                                      int rows1, T* __restrict__ out1, long long sP1,
                                                      long long sc1, const T* __restrict__ P2,
                                                      const T* __restrict__ c2, int rows2,
                                                      T* __restrict__ out2, long long sP2, long long sc2,
                                                      const T* __restrict__ x, int nx, int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows1 + rows2) return;
    const T* P = P1;
    const T* c = c1;
    T* out = out1;
    int ld = rows1;
    long long sP = sP1, sc = sc1;
    if (i >= rows1) {
        i -= rows1;
        P = P2;
        c = c2;
        out = out2;
        ld = rows2;
        sP = sP2;
        sc = sc2;
    }
    P += (size_t)i * nx;
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        const T* xb = x + (size_t)b * nx;
        const T* Pi = P + b * sP;
        T acc = c ? c[b * sc + i] : T(0);
        for (int k = 0; k < nx; ++k) acc = __builtin_fma(Pi[k], xb[k], acc);
        out[(size_t)b * ld + i] = acc;
    }
}

// xn[b] = A x[b] + B z[b][0:nu];  optional trajectories xs[b] = x[b], us[b] = z[b][0:nu]
// sA, sB: elements between consecutive instances' A / B (0 = shared)
template <typename T>
__global__ __launch_bounds__(256) void plant_step_kernel(const T* __restrict__ A, const T* __restrict__ B,
                                                         long long sA, long long sB,
                                                         const T* __restrict__ x, const T* __restrict__ z,
                                                         long long ldz, T* __restrict__ xn, int nx, int nu,
                                                         int batch, T* __restrict__ xs, T* __restrict__ us) {
    const int per = nx > nu ? nx : nu;
    const long long total = (long long)batch * per;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(t / per);
        const int i = (int)(t - (long long)b * per);
        const T* xb = x + (long long)b * nx;
        const T* ub = z + (long long)b * ldz;
        if (i < nx) {
            T acc = T(0);
            const T* Ai = A + b * sA + (long long)i * nx;
            for (int k = 0; k < nx; ++k) acc = __builtin_fma(Ai[k], xb[k], acc);
            const T* Bi = B + b * sB + (long long)i * nu;
            for (int j = 0; j < nu; ++j) acc = __builtin_fma(Bi[j], ub[j], acc);
            xn[(long long)b * nx + i] = acc;
            if (xs) xs[(long long)b * nx + i] = xb[i];
        }
        if (i < nu && us) us[(long long)b * nu + i] = ub[i];
    }
}

static dim3 grid_for(long long total) {
    long long blocks = (total + 255) / 256;
    if (blocks > 65535) blocks = 65535;
    if (blocks < 1) blocks = 1;
    return dim3((unsigned)blocks);
}

// ---- exogenous signals (gpad_setup_signals) ------------------------------------------------
// The binding with signals is the plain binding on the augmented state x~ = [x; s]: the maps are
// packed once into images with rows of nx + ns columns, [P S] (zeros where S is absent, so a NULL map's
// terms are evaluated), affine2_kernel runs over x~ as it stands, and the step below is
// plant_step_kernel with a row stride of nx + ns that also moves the next step's signals in.

// out[c][i][0:nx] = P[c][i][:], out[c][i][nx:nx+ns] = S[c][i][:] (or zeros), c < copies, i < rows
template <typename T>
__global__ __launch_bounds__(256) void pack_aug_kernel(const T* __restrict__ P, const T* __restrict__ S,
                                                       T* __restrict__ out, long long rows_total, int nx, int ns) {
    const int nxa = nx + ns;
    const long long total = rows_total * nxa;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const long long r = t / nxa;
        const int k = (int)(t - r * nxa);
        out[t] = k < nx ? P[r * nx + k] : (S ? S[r * ns + (k - nx)] : T(0));
    }
}

// xt[b] = [x[b]; s[b]] (rows of nx + ns)
template <typename T>
__global__ __launch_bounds__(256) void sig_state_kernel(const T* __restrict__ x, const T* __restrict__ s,
                                                        T* __restrict__ xt, int nx, int ns, int batch) {
    const int nxa = nx + ns;
    const long long total = (long long)batch * nxa;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const long long b = t / nxa;
        const int k = (int)(t - b * nxa);
        xt[t] = k < nx ? x[b * nx + k] : s[b * ns + (k - nx)];
    }
}

// xt, xtn: [batch][nx + ns] = [x; s].  xtn[b][0:nx] = [A E] xt[b] + B z[b][0:nu] (one chain: the A x
// terms, the E s terms, the B u terms), xtn[b][nx:] = sn[b] (the next step's signals; null after the
// last step: left alone).  xs[b] = x[b] and xo[b] = x+ are dense rows of nx, us[b] = z[b][0:nu]; all
// three optional.  AE: [nx][nx + ns] per copy.
template <typename T>
__global__ __launch_bounds__(256) void plant_step_sig_kernel(const T* __restrict__ AE, const T* __restrict__ B,
                                                             long long sA, long long sB,
                                                             const T* __restrict__ xt, const T* __restrict__ z,
                                                             long long ldz, T* __restrict__ xtn,
                                                             const T* __restrict__ sn, int nx, int ns, int nu,
                                                             int batch, T* __restrict__ xs, T* __restrict__ us,
                                                             T* __restrict__ xo) {
    const int nxa = nx + ns;
    const int per = nxa > nu ? nxa : nu;
    const long long total = (long long)batch * per;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(t / per);
        const int i = (int)(t - (long long)b * per);
        const T* xb = xt + (long long)b * nxa;
        const T* ub = z + (long long)b * ldz;
        if (i < nx) {
            T acc = T(0);
            const T* Ai = AE + b * sA + (long long)i * nxa;
            for (int k = 0; k < nxa; ++k) acc = __builtin_fma(Ai[k], xb[k], acc);
            const T* Bi = B + b * sB + (long long)i * nu;
            for (int j = 0; j < nu; ++j) acc = __builtin_fma(Bi[j], ub[j], acc);
            xtn[(long long)b * nxa + i] = acc;
            if (xo) xo[(long long)b * nx + i] = acc;
            if (xs) xs[(long long)b * nx + i] = xb[i];
        } else if (i < nxa && sn) {
            xtn[(long long)b * nxa + i] = sn[(long long)b * ns + (i - nx)];
        }
        if (i < nu && us) us[(long long)b * nu + i] = ub[i];
    }
}

template <typename T>
hipError_t launch_pack_aug(const T* P, const T* S, T* out, long long rows_total, int nx, int ns, hipStream_t s) {
    if (rows_total <= 0) return hipSuccess;
    hipLaunchKernelGGL(pack_aug_kernel<T>, grid_for(rows_total * (nx + ns)), dim3(256), 0, s, P, S, out, rows_total,
                       nx, ns);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_sig_state(const T* x, const T* sg, T* xt, int nx, int ns, int batch, hipStream_t s) {
    hipLaunchKernelGGL(sig_state_kernel<T>, grid_for((long long)batch * (nx + ns)), dim3(256), 0, s, x, sg, xt, nx,
                       ns, batch);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_plant_step_sig(const T* AE, const T* B, const T* xt, const T* z, long long ldz, T* xtn,
                                 const T* sn, int nx, int ns, int nu, int batch, T* xs, T* us, T* xo,
                                 bool per_instance, hipStream_t s) {
    const int nxa = nx + ns, per = nxa > nu ? nxa : nu;
    const long long p = per_instance ? 1 : 0;
    hipLaunchKernelGGL(plant_step_sig_kernel<T>, grid_for((long long)batch * per), dim3(256), 0, s, AE, B,
                       p * nx * nxa, p * nx * nu, xt, z, ldz, xtn, sn, nx, ns, nu, batch, xs, us, xo);
    return hipGetLastError();
}

template hipError_t launch_pack_aug<float>(const float*, const float*, float*, long long, int, int, hipStream_t);
template hipError_t launch_pack_aug<double>(const double*, const double*, double*, long long, int, int, hipStream_t);
template hipError_t launch_sig_state<float>(const float*, const float*, float*, int, int, int, hipStream_t);
template hipError_t launch_sig_state<double>(const double*, const double*, double*, int, int, int, hipStream_t);
template hipError_t launch_plant_step_sig<float>(const float*, const float*, const float*, const float*, long long,
                                                 float*, const float*, int, int, int, int, float*, float*, float*,
                                                 bool, hipStream_t);
template hipError_t launch_plant_step_sig<double>(const double*, const double*, const double*, const double*,
                                                  long long, double*, const double*, int, int, int, int, double*,
                                                  double*, double*, bool, hipStream_t);

template <typename T>
hipError_t launch_affine2(const T* P1, const T* c1, int rows1, T* out1, const T* P2, const T* c2,
                          int rows2, T* out2, const T* x, int nx, int batch, bool per_instance, hipStream_t s) {
    const dim3 grid((rows1 + rows2 + 255) / 256, batch < 65535 ? batch : 65535);
    const long long p = per_instance ? 1 : 0;
    hipLaunchKernelGGL(affine2_kernel<T>, grid, dim3(256), 0, s, P1, c1, rows1, out1, p * rows1 * nx, p * rows1,
                       P2, c2, rows2, out2, p * rows2 * nx, p * rows2, x, nx, batch);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_plant_step(const T* A, const T* B, const T* x, const T* z, long long ldz, T* xn, int nx,
                             int nu, int batch, T* xs, T* us, bool per_instance, hipStream_t s) {
    const int per = nx > nu ? nx : nu;
    const long long p = per_instance ? 1 : 0;
    hipLaunchKernelGGL(plant_step_kernel<T>, grid_for((long long)batch * per), dim3(256), 0, s, A, B,
                       p * nx * nx, p * nx * nu, x, z, ldz, xn, nx, nu, batch, xs, us);
    return hipGetLastError();
}

template hipError_t launch_affine2<float>(const float*, const float*, int, float*, const float*,
                                          const float*, int, float*, const float*, int, int, bool, hipStream_t);
template hipError_t launch_affine2<double>(const double*, const double*, int, double*, const double*,
                                           const double*, int, double*, const double*, int, int, bool,
                                           hipStream_t);
template hipError_t launch_plant_step<float>(const float*, const float*, const float*, const float*,
                                             long long, float*, int, int, int, float*, float*, bool, hipStream_t);
template hipError_t launch_plant_step<double>(const double*, const double*, const double*, const double*,
                                              long long, double*, int, int, int, double*, double*, bool,
                                              hipStream_t);

// acc += sum of per-instance iteration counts (one workgroup; wave sums then one atomic per wave)
__global__ void accumulate_iters_kernel(const int* __restrict__ iters, long long count, long long* acc) {
    long long sum = 0;
    for (long long i = threadIdx.x; i < count; i += blockDim.x) sum += iters[i];
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(reinterpret_cast<unsigned long long*>(acc), (unsigned long long)sum);
}

hipError_t launch_accumulate_iters(const int* iters, long long count, long long* acc, hipStream_t s) {
    hipLaunchKernelGGL(accumulate_iters_kernel, dim3(1), dim3(1024), 0, s, iters, count, acc);
    return hipGetLastError();
}

// part[b] = max |g_i| of workgroup b, the other slots zeroed (the certification floor, include/gpad.h
// gpad_run): up to 1024 workgroups of 256 threads, 16 elements per thread and pass with the loads of
// a pass issued together (one pass at the C4 shard), each workgroup reducing through LDS into its
// own slot.  No atomics: hundreds of same-address atomics serialise at L2 (~30 us per solve
// measured); the host reduces the slots when it reads the stats.
template <typename T>
__global__ __launch_bounds__(256) void absmax_kernel(const T* __restrict__ g, long long count, double* part) {
    __shared__ double red[4];
    double mx = 0.0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long base = (long long)blockIdx.x * blockDim.x + threadIdx.x; base < count; base += 16 * stride) {
        T v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const long long i = base + u * stride;
            v[u] = i < count ? g[i] : T(0);
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) mx = absmax_nan(mx, (double)v[u]);
    }
    for (int o = 32; o > 0; o >>= 1) mx = absmax_nan(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {  // (the run's only writer of part: SolveArgs::gmax_part)
        mx = absmax_nan(absmax_nan(red[0], red[1]), absmax_nan(red[2], red[3]));
        part[blockIdx.x] = mx;
    }
    if (blockIdx.x == 0)
        for (int i = gridDim.x + threadIdx.x; i < kAbsmaxMaxBlocks; i += blockDim.x) part[i] = 0.0;
}

template <typename T>
hipError_t launch_absmax(const T* g, long long count, double* part, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(absmax_kernel<T>, dim3(absmax_blocks(count)), dim3(256), 0, s, g, count, part);
    return hipGetLastError();
}
template hipError_t launch_absmax<float>(const float*, long long, double*, hipStream_t);
template hipError_t launch_absmax<double>(const double*, long long, double*, hipStream_t);

// One step of a multi-step run: fold the step's per-workgroup maxima into the run's (slot-wise; the
// host reduces the slots).  Step 0 stores, so `acc` needs no zeroing either.
__global__ __launch_bounds__(256) void absmax_fold_kernel(const double* __restrict__ part, double* acc, int first) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < kAbsmaxMaxBlocks) acc[i] = first ? part[i] : absmax_nan(acc[i], part[i]);
}

hipError_t launch_absmax_fold(const double* part, double* acc, bool first, hipStream_t s) {
    hipLaunchKernelGGL(absmax_fold_kernel, dim3((kAbsmaxMaxBlocks + 255) / 256), dim3(256), 0, s, part, acc,
                       first ? 1 : 0);
    return hipGetLastError();
}

}  // namespace gpad
