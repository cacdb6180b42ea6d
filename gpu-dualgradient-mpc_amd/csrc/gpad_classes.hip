// gpad_classes.hip -- row permutations of the class binding (gpad_setup_classes, gpad_classes.cpp).
//
// A class-bound handle solves class k's instances as one shared-matrix sub-batch, which needs that
// class's rows of every [batch][len] array contiguous.  The caller's arrays stay in the caller's
// instance order, so each call gathers its inputs into a class-sorted workspace, lets every class's
// child handle work on its slice in place, and scatters the results back:
//   gather :  sorted[pos][:]        = caller[perm[pos]][:]     (z, y, M, g  /  x, z, y: one launch)
//   scatter:  caller[perm[pos]][:]  = sorted[pos][:]           (z, y  /  x, z, y: one launch)
//   traj   :  caller[t][perm[pos]][:] = class block of pos, row (t, pos - offsets[k])   (xs, us: one launch)
//   signals:  class block of pos, row (t, pos - offsets[k]) = caller[t][perm[pos]][:]   (s / S: one launch)
// Pure data movement, O(batch (n + m)) words per call against the O(iterations n m) of the solves:
// plain grid-stride kernels, one element per thread and trip, coalesced on the sorted side (the
// caller's side is coalesced within a row).  perm is a permutation, so no two threads write one
// word: no atomics, no kernel waits on another workgroup.
#include "gpad_classes.h"

namespace gpad {

// column r of the concatenated row [len0 | len1 | ...] -> that array's pointers, its row length and the
// column j inside it (static indices into the kernel argument: no private copy of the struct)
template <typename T, typename M>
__device__ __forceinline__ void locate(const M& mv, int r, const T*& src, T*& dst, int& len, int& j) {
    constexpr int kArrays = (int)(sizeof(mv.len) / sizeof(int));
    src = mv.src[0];
    dst = mv.dst[0];
    len = mv.len[0];
    j = r;
    int a = 0;
#pragma unroll
    for (int k = 1; k < kArrays; ++k) {
        if (a == k - 1 && k < mv.count && j >= len) {
            j -= len;
            a = k;
            src = mv.src[k];
            dst = mv.dst[k];
            len = mv.len[k];
        }
    }
}

template <typename T, bool kGather>
__global__ __launch_bounds__(256) void class_rows_kernel(RowMove<T> mv, const int* __restrict__ perm, int batch,
                                                         int row) {
    const long long total = (long long)batch * row;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        const int pos = (int)(e / row);
        const T* src;
        T* dst;
        int len, j;
        locate<T>(mv, (int)(e - (long long)pos * row), src, dst, len, j);
        const long long sorted = (long long)pos * len + j;
        const long long caller = (long long)perm[pos] * len + j;
        if (kGather) dst[sorted] = src[caller];
        else dst[caller] = src[sorted];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void class_traj_kernel(TrajMove<T> mv, const int* __restrict__ perm,
                                                         const int* __restrict__ pos_off,
                                                         const int* __restrict__ pos_cnt, int batch, int steps,
                                                         int row) {
    const long long per_step = (long long)batch * row, total = per_step * steps;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        const int t = (int)(e / per_step);
        const long long r = e - (long long)t * per_step;
        const int pos = (int)(r / row);
        const T* src;
        T* dst;
        int len, j;
        locate<T>(mv, (int)(r - (long long)pos * row), src, dst, len, j);
        // (no tables: one block [steps][batch][len] of every class, the fused class loop's)
        const long long off = pos_off ? pos_off[pos] : 0, cnt = pos_cnt ? pos_cnt[pos] : batch;
        // class block [steps][cnt][len] at steps * off * len; row (t, pos - off)
        const long long from = ((long long)steps * off + (long long)t * cnt + (pos - off)) * len + j;
        const long long to = ((long long)t * batch + perm[pos]) * len + j;
        dst[to] = src[from];
    }
}

// The inverse of class_traj_kernel for the one array of signals: thread e owns destination word e.  The
// class blocks [steps][cnt_k][ns] lie one after the other, class k's at steps * off_k * ns, so word e sits
// in the block of the class that sorted position e / (steps * ns) belongs to (off_k <= that < off_k + cnt_k).
template <typename T>
__global__ __launch_bounds__(256) void class_sig_kernel(const T* __restrict__ src, T* __restrict__ dst,
                                                        const int* __restrict__ perm,
                                                        const int* __restrict__ pos_off,
                                                        const int* __restrict__ pos_cnt, int batch, int steps,
                                                        int ns) {
    const long long per_pos = (long long)steps * ns, total = per_pos * batch;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        const int q = (int)(e / per_pos);
        // (no tables: one sorted [steps][batch][ns] array, the fused class loop's)
        const long long off = pos_off ? pos_off[q] : 0, cnt = pos_cnt ? pos_cnt[q] : batch;
        const long long local = e - per_pos * off;  // word of the class block [steps][cnt][ns]
        const long long step_words = cnt * ns;
        const int t = (int)(local / step_words);
        const long long r = local - (long long)t * step_words;
        const int i = (int)(r / ns), j = (int)(r - (long long)i * ns);
        dst[e] = src[((long long)t * batch + perm[off + i]) * ns + j];
    }
}

static unsigned move_grid(long long total) {
    long long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;  // grid-stride beyond
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}

template <typename M>
static int row_len(const M& mv) {
    int row = 0;
    for (int a = 0; a < mv.count; ++a) row += mv.len[a];
    return row;
}

template <typename T>
hipError_t launch_class_gather(const RowMove<T>& mv, const int* perm, int batch, hipStream_t s) {
    const int row = row_len(mv);
    if (row == 0 || batch == 0) return hipSuccess;
    class_rows_kernel<T, true><<<move_grid((long long)batch * row), 256, 0, s>>>(mv, perm, batch, row);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_class_scatter(const RowMove<T>& mv, const int* perm, int batch, hipStream_t s) {
    const int row = row_len(mv);
    if (row == 0 || batch == 0) return hipSuccess;
    class_rows_kernel<T, false><<<move_grid((long long)batch * row), 256, 0, s>>>(mv, perm, batch, row);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_class_traj_scatter(const TrajMove<T>& mv, const int* perm, const int* pos_off,
                                     const int* pos_cnt, int batch, int steps, hipStream_t s) {
    const int row = row_len(mv);
    if (row == 0 || batch == 0 || steps == 0) return hipSuccess;
    class_traj_kernel<T><<<move_grid((long long)batch * row * steps), 256, 0, s>>>(mv, perm, pos_off, pos_cnt, batch,
                                                                                   steps, row);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_class_sig_gather(const T* src, T* dst, int ns, const int* perm, const int* pos_off,
                                   const int* pos_cnt, int batch, int steps, hipStream_t s) {
    if (ns == 0 || batch == 0 || steps == 0) return hipSuccess;
    class_sig_kernel<T><<<move_grid((long long)batch * ns * steps), 256, 0, s>>>(src, dst, perm, pos_off, pos_cnt,
                                                                                 batch, steps, ns);
    return hipGetLastError();
}

template hipError_t launch_class_gather<float>(const RowMove<float>&, const int*, int, hipStream_t);
template hipError_t launch_class_gather<double>(const RowMove<double>&, const int*, int, hipStream_t);
template hipError_t launch_class_scatter<float>(const RowMove<float>&, const int*, int, hipStream_t);
template hipError_t launch_class_scatter<double>(const RowMove<double>&, const int*, int, hipStream_t);
template hipError_t launch_class_traj_scatter<float>(const TrajMove<float>&, const int*, const int*, const int*, int,
                                                     int, hipStream_t);
template hipError_t launch_class_traj_scatter<double>(const TrajMove<double>&, const int*, const int*, const int*,
                                                      int, int, hipStream_t);

template hipError_t launch_class_sig_gather<float>(const float*, float*, int, const int*, const int*, const int*, int,
                                                   int, hipStream_t);
template hipError_t launch_class_sig_gather<double>(const double*, double*, int, const int*, const int*, const int*,
                                                    int, int, hipStream_t);

}  // namespace gpad
