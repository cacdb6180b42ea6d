// gpad_steps.hip -- the row kernels' k-major packer and the per-step mirrors of kernel_functions.h
#include <hip/hip_runtime.h>

#include <cmath>

#include "gpad_chain.h"
#include "gpad_internal.h"

namespace gpad {

// =========================================================================================
// layout kernels
// =========================================================================================
// out[k*ld + i] = (T)(scale * in[i*cols + k]); 32x32 tiles through LDS so both the read of
// the row-major input and the write of the k-major output are coalesced.
template <typename T>
__global__ __launch_bounds__(256) void pack_kmajor_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                          int rows, int cols, int ld, double scale,
                                                          long long in_stride, long long out_stride) {
    __shared__ T tile[32][33];
    const T* src = in + (size_t)blockIdx.z * in_stride;
    T* dst = out + (size_t)blockIdx.z * out_stride;
    const int i0 = blockIdx.y * 32, k0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        const int i = i0 + r, k = k0 + tx;
        tile[r][tx] = (i < rows && k < cols) ? (T)(scale * (double)src[(size_t)i * cols + k]) : T(0);
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int k = k0 + r, i = i0 + tx;
        if (k < cols && i < ld) dst[(size_t)k * ld + i] = tile[tx][r];
    }
}

template <typename T>
hipError_t launch_pack_kmajor(const T* in, T* out, int rows, int cols, int ld, double scale,
                              int batch, long long in_stride, long long out_stride, hipStream_t s) {
    const dim3 grid((cols + 31) / 32, (ld + 31) / 32, batch);
    hipLaunchKernelGGL(pack_kmajor_kernel<T>, grid, dim3(256), 0, s, in, out, rows, cols, ld, scale,
                       in_stride, out_stride);
    return hipGetLastError();
}
template hipError_t launch_pack_kmajor<float>(const float*, float*, int, int, int, double, int,
                                              long long, long long, hipStream_t);
template hipError_t launch_pack_kmajor<double>(const double*, double*, int, int, int, double, int,
                                               long long, long long, hipStream_t);

// =========================================================================================
// per-step kernels (kernel_functions.h:9-41 one for one; seq_functions.cpp semantics)
// =========================================================================================
__global__ void step1_kernel(const float* __restrict__ y, const float* __restrict__ ym1,
                             float* __restrict__ w, float beta, int m) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x)
        w[i] = __builtin_fmaf(beta, y[i] - ym1[i], y[i]);
}

// One lane per output row, sequential chain over the row (bit-exact with the CPU step);
// the vector is staged in LDS (as StepTwoGPADKernel's w_vs, kernel_functions.cu:37-42).
__global__ __launch_bounds__(256) void step_gemv_kernel(const float* __restrict__ A,
                                                        const float* __restrict__ x, int rows, int cols,
                                                        const float* __restrict__ bias, float bsign,
                                                        const float* __restrict__ addv,
                                                        float* __restrict__ out, int relu) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    for (int k = threadIdx.x; k < cols; k += blockDim.x) xs[k] = x[k];
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const float* row = A + (size_t)i * cols;
    float acc = 0.0f;
    for (int k = 0; k < cols; ++k) acc = __builtin_fmaf(row[k], xs[k], acc);
    if (!relu) {
        out[i] = acc - bias[i];  // 8b: zhat = MGneg w - gP
    } else {
        const float s = (addv[i] + bias[i]) + acc;  // 8d: (w + pD) + sum
        out[i] = (__builtin_fabsf(s) + s) * 0.5f;
    }
    (void)bsign;
}

__global__ void step3_kernel(float theta, const float* zm1, const float* __restrict__ zhat, float* z,
                             int n) {
    const float omt = 1.0f - theta;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        z[i] = __builtin_fmaf(omt, zm1[i], theta * zhat[i]);
}

static dim3 grid1d(int n) {
    int g = (n + 255) / 256;
    if (g < 1) g = 1;
    if (g > 2048) g = 2048;
    return dim3(g);
}

hipError_t launch_step1(const float* y, const float* ym1, float* w, float beta, int m, hipStream_t s) {
    hipLaunchKernelGGL(step1_kernel, grid1d(m), dim3(256), 0, s, y, ym1, w, beta, m);
    return hipGetLastError();
}
hipError_t launch_step2(const float* MGneg, const float* w, const float* gP, float* zhat, int n,
                        int m, hipStream_t s) {
    hipLaunchKernelGGL(step_gemv_kernel, dim3((n + 255) / 256), dim3(256), sizeof(float) * (size_t)m, s,
                       MGneg, w, n, m, gP, -1.0f, (const float*)nullptr, zhat, 0);
    return hipGetLastError();
}
hipError_t launch_step3(float theta, const float* zm1, const float* zhat, float* z, int n,
                        hipStream_t s) {
    hipLaunchKernelGGL(step3_kernel, grid1d(n), dim3(256), 0, s, theta, zm1, zhat, z, n);
    return hipGetLastError();
}
hipError_t launch_step4(const float* GL, float* yp1, const float* w, const float* pD,
                        const float* zhat, int n, int m, hipStream_t s) {
    hipLaunchKernelGGL(step_gemv_kernel, dim3((m + 255) / 256), dim3(256), sizeof(float) * (size_t)n, s,
                       GL, zhat, m, n, pD, 1.0f, w, yp1, 1);
    return hipGetLastError();
}

}  // namespace gpad
