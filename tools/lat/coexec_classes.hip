// Micro-benchmark: what does one non-MFMA vector instruction of a partner wave cost the f32 MFMA
// chains of the same SIMD, per instruction class?  (coexec.hip asked it for v_fma_f32 only.)
// 512-thread workgroups, one per CU: two waves per SIMD.  One wave of each SIMD runs four
// interleaved v_mfma_f32_16x16x4_f32 chains at the pair layout's depth (50 dependent steps from a
// zero accumulator, the T = 13 chain: 12 k-blocks of 4 steps and one of 2), kReps times, and stamps
// its own duration with s_memtime.  Its partner issues kBlocks blocks of 16 independent
// instructions of one class, then exits; with no other stall it needs 4 cycles each, so it is
// done well inside the MFMA wave's 4 * 50 * kReps * 32 cycles.  Both start at one barrier.
//   cost = (MFMA wave's cycles beside the class - its cycles beside an idle partner) / (16 kBlocks)
// is the MFMA time lost per partner instruction.  Both age orders run: the partner as the older
// wave of the SIMD (waves 0-3) and as the younger one (waves 4-7); the SIMD issues oldest first.
// One process, fixed step counts:  hipcc --offload-arch=gfx950 -O3 -o coexec_classes coexec_classes.hip
//                                  timeout -k 10 120 ./coexec_classes
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));
constexpr int kDepth = 50, kReps = 24, kBlocks = 512, kLaunches = 5;

enum Class { kNone, kMov, kAddU32, kLshlAddU64, kCndmask, kLane, kPkFma, kFma, kClasses };
static const char* const kNames[kClasses] = {"nothing",     "v_mov_b32",          "v_add_u32",    "v_lshl_add_u64",
                                             "v_cndmask_b32", "v_readlane+v_writelane", "v_pk_fma_f32", "v_fma_f32"};

__device__ __forceinline__ unsigned long long mfma_wave(float a, float b, float* sink) {
    f4 c[4];
    float s = 0.0f;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int rep = 0; rep < kReps; ++rep) {
#pragma unroll
        for (int q = 0; q < 4; ++q) c[q] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < kDepth; ++k) {
#pragma unroll
            for (int q = 0; q < 4; ++q) c[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b + q, c[q], 0, 0, 0);
        }
        asm volatile("" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]));
        s += c[0][0] + c[1][1] + c[2][2] + c[3][3];
        a += 1e-6f;
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    *sink = s;
    return t1 - t0;
}

// 16 independent instructions per block (8 registers, each written twice)
#define REP8(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
#define REP16(X) REP8(X) REP8(X)

template <int CLS>
__device__ __forceinline__ void partner_wave(float seed, float* sink) {
    if constexpr (CLS == kNone) return;
    float r[8];
    unsigned u[8];
    unsigned long long w[8];
    f2 p[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        r[i] = seed + i;
        u[i] = (unsigned)(threadIdx.x + i);
        w[i] = threadIdx.x * 8ull + i;
        p[i] = f2{seed, seed + i};
    }
    const f2 pa = f2{0.999f, 0.998f}, pb = f2{1e-3f, 2e-3f};
    const float fa = 0.999f * seed, fb = 1e-3f;
    unsigned sv = __builtin_amdgcn_readfirstlane(u[0]);
    for (int blk = 0; blk < kBlocks; ++blk) {
        if constexpr (CLS == kMov) {
#define X(i) asm volatile("v_mov_b32 %0, %1" : "=v"(r[i]) : "v"(r[(i + 1) & 7]));
            REP16(X)
#undef X
        } else if constexpr (CLS == kAddU32) {
#define X(i) asm volatile("v_add_u32 %0, %0, %1" : "+v"(u[i]) : "v"(u[(i + 1) & 7]));
            REP16(X)
#undef X
        } else if constexpr (CLS == kLshlAddU64) {
#define X(i) asm volatile("v_lshl_add_u64 %0, %0, 1, %1" : "+v"(w[i]) : "v"(w[(i + 1) & 7]));
            REP16(X)
#undef X
        } else if constexpr (CLS == kCndmask) {
            asm volatile("s_mov_b64 vcc, 0x55555555" ::: "vcc");
#define X(i) asm volatile("v_cndmask_b32 %0, %0, %1, vcc" : "+v"(u[i]) : "v"(u[(i + 1) & 7]) : "vcc");
            REP16(X)
#undef X
        } else if constexpr (CLS == kLane) {  // 8 reads into SGPRs, 8 writes from another SGPR
            unsigned s0, s1, s2, s3, s4, s5, s6, s7;
            asm volatile(
                "v_readlane_b32 %0, %8, 1\n v_readlane_b32 %1, %9, 2\n v_readlane_b32 %2, %10, 3\n"
                "v_readlane_b32 %3, %11, 4\n v_readlane_b32 %4, %8, 5\n v_readlane_b32 %5, %9, 6\n"
                "v_readlane_b32 %6, %10, 7\n v_readlane_b32 %7, %11, 8\n"
                : "=s"(s0), "=s"(s1), "=s"(s2), "=s"(s3), "=s"(s4), "=s"(s5), "=s"(s6), "=s"(s7)
                : "v"(u[0]), "v"(u[1]), "v"(u[2]), "v"(u[3]));
#define X(i) asm volatile("v_writelane_b32 %0, %1, " #i : "+v"(u[4 + (i & 3)]) : "s"(sv));
            REP8(X)
#undef X
            asm volatile("" ::"s"(s0), "s"(s1), "s"(s2), "s"(s3), "s"(s4), "s"(s5), "s"(s6), "s"(s7));
        } else if constexpr (CLS == kPkFma) {
#define X(i) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(p[i]) : "v"(pa), "v"(pb));
            REP16(X)
#undef X
        } else if constexpr (CLS == kFma) {
#define X(i) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(r[i]) : "v"(fa), "v"(fb));
            REP16(X)
#undef X
        }
    }
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += r[i] + (float)u[i] + (float)w[i] + p[i].x + p[i].y;
    *sink = s;
}

// out[block][wave]: the MFMA waves' cycles; sink: one float per thread
template <int CLS, bool PARTNER_OLDER>
__global__ __launch_bounds__(512) void probe(unsigned long long* out, float* sink, float seed) {
    const int w = threadIdx.x >> 6;
    const bool mf = PARTNER_OLDER ? w >= 4 : w < 4;
    float* sk = sink + (size_t)blockIdx.x * 512 + threadIdx.x;
    __syncthreads();
    if (mf) {
        const unsigned long long d = mfma_wave(seed * (threadIdx.x & 63), seed + (threadIdx.x & 15), sk);
        if ((threadIdx.x & 63) == 0) out[blockIdx.x * 4 + (w & 3)] = d;
    } else {
        partner_wave<CLS>(seed, sk);
    }
}

template <int CLS, bool OLDER>
double run(unsigned long long* out, float* sink, int grid) {
    std::vector<unsigned long long> h((size_t)grid * 4), all;
    for (int r = 0; r < kLaunches; ++r) {
        hipLaunchKernelGGL((probe<CLS, OLDER>), dim3(grid), dim3(512), 0, 0, out, sink, 1.0f);
        if (hipDeviceSynchronize() != hipSuccess) {
            fprintf(stderr, "launch failed\n");
            exit(1);
        }
        if (r == 0) continue;  // (warm-up)
        (void)hipMemcpy(h.data(), out, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost);
        all.insert(all.end(), h.begin(), h.end());
    }
    std::sort(all.begin(), all.end());
    return (double)all[all.size() / 2];
}

template <int CLS>
void row(unsigned long long* out, float* sink, int grid, double (&base)[2]) {
    const double o = run<CLS, true>(out, sink, grid), y = run<CLS, false>(out, sink, grid);
    if (CLS == kNone) {
        base[0] = o;
        base[1] = y;
    }
    const double n = 16.0 * kBlocks, mf = 4.0 * kDepth * kReps;
    printf("%-24s partner older: %8.0f cyc (%.2f/MFMA) lost/instr %6.2f | partner younger: %8.0f cyc (%.2f/MFMA) lost/instr %6.2f\n",
           kNames[CLS], o, o / mf, (o - base[0]) / n, y, y / mf, (y - base[1]) / n);
}

int main() {
    int dev;
    (void)hipGetDevice(&dev);
    hipDeviceProp_t p;
    (void)hipGetDeviceProperties(&p, dev);
    const int grid = p.multiProcessorCount;
    unsigned long long* out;
    float* sink;
    (void)hipMalloc(&out, (size_t)grid * 4 * sizeof(*out));
    (void)hipMalloc(&sink, (size_t)grid * 512 * sizeof(float));
    printf("CUs %d; MFMA wave: %d MFMAs (4 chains x depth %d x %d); partner: %d instructions; median of %d waves\n",
           grid, 4 * kDepth * kReps, kDepth, kReps, 16 * kBlocks, grid * 4 * (kLaunches - 1));
    double base[2] = {0, 0};
    row<kNone>(out, sink, grid, base);
    row<kMov>(out, sink, grid, base);
    row<kAddU32>(out, sink, grid, base);
    row<kLshlAddU64>(out, sink, grid, base);
    row<kCndmask>(out, sink, grid, base);
    row<kLane>(out, sink, grid, base);
    row<kPkFma>(out, sink, grid, base);
    row<kFma>(out, sink, grid, base);
    return 0;
}
