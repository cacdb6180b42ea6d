// gpad_lipschitz.hip -- the batched fp64 products behind gpad_lipschitz (gpad_setup.cpp): an upper bound
// on lambda_max(G H^-1 G') = rho(G ML), the smallest L that GPAD may run with.
//
// With K = min(n, m) and S = ML G (n <= m) or G ML (m < n), the host chains
//   B_0 = S / |S|_F,   B_{j+1} = B_j^2 / |B_j^2|_F,   L = prod_j |.|_F^(1 / 2^j)  >=  rho(S),
// and this file holds the one kernel of that chain: C = (s A)(s B) on v_mfma_f64_16x16x4_f64 for a batch
// of instances, with the sum of squares of C beside it.  The first launch forms S from the caller's f32 or
// f64 matrices (widened on load, s = 1); every later launch squares the previous launch's output, s being
// the reciprocal of its Frobenius norm, so the buffers hold the unnormalised squares and the normalisation
// rides on the loads.
//
// A workgroup of four waves owns a 64 x 64 tile of C, wave w the 32 x 32 quarter (w >> 1, w & 1) as 2 x 2
// MFMA tiles; the operands pass through LDS 16 values of k at a time, zero beyond the matrices' edges, so a
// ragged last tile needs no other care.  Operand layout as in gpad_panel64.hip: lane l supplies
// A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15], accumulator register r holds D[(l >> 4) + 4 r][l & 15].
//
// Norms without atomics: a workgroup reduces its tile's squares in a fixed order (per lane in register
// order, then a halving tree over the 256 lanes) and *stores* the sum into its own slot; the next launch,
// and the host at the end, add an instance's slots with lip_slot_sum's fixed order (256 strided partial
// sums, ascending, then the same tree).  An instance's tiles and slots depend on nothing but its own
// matrices, so its result has the same bits alone or anywhere in a batch, on every run.
#include <hip/hip_runtime.h>

#include "gpad_internal.h"

namespace gpad {

typedef double lip_f64x4 __attribute__((ext_vector_type(4)));

// sum of slots[0 .. count) by the whole workgroup, the order the host repeats (gpad_setup.cpp lip_slot_sum)
__device__ __forceinline__ double lip_slot_sum_dev(const double* __restrict__ slots, int count, double* red, int tid) {
    double p = 0.0;
    for (int i = tid; i < count; i += kLipThreads) p += slots[i];
    red[tid] = p;
    __syncthreads();
    for (int s = kLipThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();  // (red is used again)
    return r;
}

template <typename T>
__global__ __launch_bounds__(kLipThreads) void lip_gemm_kernel(LipGemmArgs a) {
    // As[k][row] (padded: the store below walks k fastest), Bs[k][col]
    __shared__ double As[kLipKc][kLipTile + 1];
    __shared__ double Bs[kLipKc][kLipTile];
    __shared__ double red[kLipThreads];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int inst = blockIdx.z;
    const int row0 = blockIdx.y * kLipTile, col0 = blockIdx.x * kLipTile;
    const int K = a.K;
    const long long P = a.P;
    const T* __restrict__ A = (const T*)a.A + (long long)inst * a.sA;
    const T* __restrict__ B = (const T*)a.B + (long long)inst * a.sB;

    double s = 1.0;
    if (a.in_slots) {  // |previous output|_F; a zero or non-finite norm ends the chain in zeros (the host reports it)
        const double ssq = lip_slot_sum_dev(a.in_slots + (long long)inst * a.slot_stride, a.nslots, red, tid);
        s = (ssq > 0.0 && ssq <= 1.7976931348623157e308) ? 1.0 / sqrt(ssq) : 0.0;
    }

    lip_f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = lip_f64x4{0.0, 0.0, 0.0, 0.0};
    const int wr = 32 * (wave >> 1), wc = 32 * (wave & 1);
    const int l15 = lane & 15, lk = lane >> 4;

    for (long long k0 = 0; k0 < P; k0 += kLipKc) {
#pragma unroll
        for (int i = 0; i < kLipKc * kLipTile / kLipThreads; ++i) {
            const int e = tid + kLipThreads * i;
            {  // A: 16 consecutive k of one row
                const int r = e / kLipKc, kk = e % kLipKc;
                const int gr = row0 + r;
                const long long gk = k0 + kk;
                As[kk][r] = (gr < K && gk < P) ? (double)A[(long long)gr * a.lda + gk] * s : 0.0;
            }
            {  // B: 64 consecutive columns of one k
                const int kk = e / kLipTile, c = e % kLipTile;
                const int gc = col0 + c;
                const long long gk = k0 + kk;
                Bs[kk][c] = (gc < K && gk < P) ? (double)B[gk * a.ldb + gc] * s : 0.0;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kLipKc / 4; ++q) {
            const int k = 4 * q + lk;
            const double a0 = As[k][wr + l15], a1 = As[k][wr + 16 + l15];
            const double b0 = Bs[k][wc + l15], b1 = Bs[k][wc + 16 + l15];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }

    double* __restrict__ C = a.C + (long long)inst * K * K;
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + wr + 16 * i + lk + 4 * r, col = col0 + wc + 16 * j + l15;
                const double v = acc[i][j][r];
                if (row < K && col < K) {
                    C[(long long)row * K + col] = v;
                    ss += v * v;
                }
            }
    red[tid] = ss;
    __syncthreads();
    for (int st = kLipThreads / 2; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    if (tid == 0)
        a.out_slots[(long long)inst * a.slot_stride + (long long)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

int lip_tiles(int K) { return (K + kLipTile - 1) / kLipTile; }

hipError_t launch_lip_gemm(const LipGemmArgs& a, bool f32_in, int count, hipStream_t s) {
    const int t = lip_tiles(a.K);
    const dim3 grid(t, t, count), block(kLipThreads);
    if (f32_in)
        hipLaunchKernelGGL(lip_gemm_kernel<float>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(lip_gemm_kernel<double>, grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace gpad
