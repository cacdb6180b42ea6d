// gpad_resident.hip -- gpad_resident_kernel<KA, KB, FLAT>, the latency family (f32, n, m <= 208).
// One workgroup per instance; each lane holds ONE matrix row in VGPRs for the whole solve, so an
// iteration touches no memory but LDS.  Waves [0,nA) own the rows of -ML, waves [nA,nA+nB) the rows
// of G/L; w and zhat are broadcast through LDS (ds_read_b128).  Numerics: gpad_stream.hip's header.
#include <hip/hip_runtime.h>

#include <cmath>

#include "gpad_chain.h"
#include "gpad_internal.h"

namespace gpad {

// FLAT = the structure-exploiting battery variant (gpad_flat.hip header; seq_functions.cpp:5-43):
// a primal row (i, j) carries only its 6N structural coefficients (KA = bucket(6N)) and chains
// over a per-cell permuted copy of w (wP[j][s] = w[j + n_u s], s < 4N; w[4 n_u N + s - 4N] after),
// so the 8b half-iteration is 6N steps long instead of m.  A-lanes are laid out so every 16-lane
// DPP row serves one cell j (lane = 16 times of that cell), hence one broadcast segment per row.
// Constraint rows chain over the natural zhat with the flat G_L expanded to full rows (exact: the
// added terms are exact zeros), with the flat step's epilogue (s + w) + p_D, y < 0 -> 0.
constexpr int kFlatMaxCells = 16;

// Iteration anatomy stamps of the resident kernel (diagnostic builds only, -DGPAD_STAMP): shader
// clock of workgroup 0, every wave, iterations [101, 105), at six points -- loop top, 8b chain done,
// after the first barrier, 8d chain done, its epilogue done, after the second barrier
// (gpad_debug_res_stamps, tools/stamp_resident.py).
#ifdef GPAD_STAMP
__device__ unsigned long long g_res_stamps[8][4][6];
#define GPAD_RSTAMP(P)                                                                         \
    do {                                                                                       \
        if (blockIdx.x == 0 && v >= 101 && v < 105 && (tid & 63) == 0)                        \
            g_res_stamps[tid >> 6][v - 101][P] = __builtin_amdgcn_s_memtime();                 \
    } while (0)
hipError_t read_res_stamps(unsigned long long* out, size_t bytes) {
    if (bytes > sizeof(g_res_stamps)) bytes = sizeof(g_res_stamps);
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_res_stamps), bytes, 0, hipMemcpyDeviceToHost);
}
#else
#define GPAD_RSTAMP(P) \
    do {               \
    } while (0)
#endif

template <int KA, int KB, bool FLAT>
__global__ __launch_bounds__(kResidentMaxThreads) void gpad_resident_kernel(SolveArgs<float> a) {
    constexpr int K = KA > KB ? KA : KB;
    constexpr int PA = (KA + 63) / 64 * 64, PB = (KB + 63) / 64 * 64;  // whole 64-element groups
    __shared__ __attribute__((aligned(16))) float w_l[FLAT ? kFlatMaxCells * PA : PA];  // w (flat: wP)
    __shared__ __attribute__((aligned(16))) float zh_l[PB];  // zhat, broadcast to G/L rows
    __shared__ __attribute__((aligned(16))) float z_l[PB];   // z_{-1}, to seed u = G_L z
    __shared__ CheckSlot slots[2][kResidentMaxThreads / 64];  // test, verification of (A)

    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int n = a.n, m = a.m;
    const int n_u = FLAT ? a.n_u : 1, Nh = FLAT ? n / n_u : 0, mc = 4 * n_u * Nh;
    const int nq = (Nh + 15) >> 4;  // flat: 16-lane DPP rows per cell
    const int nA = FLAT ? (n_u * nq * 16 + 63) >> 6 : (n + 63) >> 6;
    const int nwaves = blockDim.x >> 6;
    const bool isA = (tid >> 6) < nA;               // wave-uniform role
    int row = isA ? tid : tid - 64 * nA;
    int cell = 0;                                   // flat A-lanes: cell j of this lane
    bool live = isA ? row < n : row < m;
    if (FLAT && isA) {  // lane -> (cell j, time i): row r = i n_u + j
        const int q = tid >> 4, i = 16 * (q % nq) + (tid & 15);
        cell = q / nq;
        live = cell < n_u && i < Nh;
        row = live ? i * n_u + cell : 0;
    }

    // preload the row once
    float r[K];
    if (FLAT && isA) {  // flat -ML row i (Nh x m, row-major): the 6N structural entries
        const float* Mi = a.MGt + (size_t)(row / n_u) * m;
#pragma unroll
        for (int k = 0; k < K; ++k)
            r[k] = (!live || k >= 6 * Nh) ? 0.0f : Mi[k < 4 * Nh ? cell + n_u * k : mc + (k - 4 * Nh)];
    } else {  // k-major images: consecutive lanes read consecutive words
        const int len = isA ? m : n;
        const float* __restrict__ Mt = isA ? a.MGt + (size_t)b * a.strideA : a.GLt + (size_t)b * a.strideB;
        const int ld = isA ? a.ldn : a.ldm;
#pragma unroll
        for (int k = 0; k < K; ++k) r[k] = (live && k < len) ? Mt[(size_t)k * ld + row] : 0.0f;
    }
    // where constraint row `row` lands in the A-side vector
    auto put_w = [&](float wv) {
        if constexpr (FLAT) {
            if (row < mc) {
                w_l[(row % n_u) * PA + row / n_u] = wv;
            } else {
                for (int j = 0; j < n_u; ++j) w_l[j * PA + 4 * Nh + (row - mc)] = wv;
            }
        } else {
            w_l[row] = wv;
        }
    };
    const float* wvec = FLAT ? w_l + cell * PA : w_l;  // this lane's broadcast segment

    float* zg = a.z + (size_t)b * n;
    float* yg = a.y + (size_t)b * m;
    float zi = 0.0f, gpi = 0.0f, yi = 0.0f, pdi = 0.0f, wi = 0.0f;
    if (isA) {
        if (live) {
            zi = zg[row];
            gpi = a.gP[(size_t)b * a.ld_gP + row];
        }
    } else if (live) {
        yi = yg[row];
        pdi = (float)(a.gscale * (double)a.g[(size_t)b * a.ld_g + row]);
        wi = __builtin_fmaf(a.beta[0], yi - yi, yi);
    }
    for (int i = tid; i < (FLAT ? kFlatMaxCells * PA : PA); i += blockDim.x) w_l[i] = 0.0f;
    for (int i = tid; i < PB; i += blockDim.x) {
        zh_l[i] = 0.0f;
        z_l[i] = 0.0f;
    }
    __syncthreads();
    if (!isA && live) put_w(wi);
    if (isA && live) z_l[row] = zi;
    __syncthreads();
    const bool use_tol = a.tol > 0.0;
    float ui = 0.0f;  // u = G_L z: seeded once, then the 8c recursion (no extra chain per test)
    if (use_tol && !isA) {
        const float us = chain_regs<KB, K>(r, z_l);  // (uniform control flow around the DPP chain)
        ui = us;
    }

    int it = 0;
    int done = 0;
    float zhi = 0.0f;
    // theta/beta are fetched one iteration ahead, by each role in its idle half (the A waves while
    // the 8d chains run, the B waves while the 8b chains run), and the test period is a countdown:
    // between barrier 2 and the next 8b chain only the loop branch remains (tables hold N + 2
    // entries).
    float th = a.theta[0], bn = a.beta[1];
    float th_next = 0.0f, bn_next = 0.0f;
    const int Kc = a.check_every;
    int kc = Kc;  // iterations to the next test: chk <=> (v + 1) % Kc == 0
    for (int v = 0; v < a.N; ++v) {
        const bool chk = use_tol && --kc == 0;
        if (chk) kc = Kc;
        GPAD_RSTAMP(0);
        if (isA) {  // ---- 8b + 8c --------------------------------------------------------
            const float acc = chain_regs<KA, K>(r, wvec);
            GPAD_RSTAMP(1);
            if (live) {
                const float zhv = acc - gpi;
                zh_l[row] = zhv;  // (the exchange first: 8c is off the critical path)
                zi = __builtin_fmaf(1.0f - th, zi, th * zhv);
                zhi = zhv;
            }
        } else {
            th_next = a.theta[v + 1];
            bn_next = a.beta[v + 2];
        }
        __syncthreads();
        GPAD_RSTAMP(2);
        float violz = -INFINITY, violh = -INFINITY, wmin = INFINITY, magh = 0.0f;
        double gap = 0.0;
        // (own text of gpad_chain.h's row step and test terms: slower through them, r19_row_test_noreg.txt)
        if (!isA) {  // ---- 8d + next 8a ------------------------------------------------
            const float c = chain_regs<KB, K>(r, zh_l);
            GPAD_RSTAMP(3);
            if (live) {
                float sv, yp;
                if constexpr (FLAT) {
                    sv = (c + wi) + pdi;             // seq_functions.cpp:37
                    yp = sv < 0.0f ? 0.0f : sv;      // seq_functions.cpp:40-42
                } else {
                    sv = (wi + pdi) + c;             // seq_functions.cpp:84
                    yp = (__builtin_fabsf(sv) + sv) * 0.5f;
                }
                const float wn = __builtin_fmaf(bn, yp - yi, yp);
                put_w(wn);  // (the exchange first: u and the test partials are off the critical path)
                if (use_tol) ui = __builtin_fmaf(1.0f - th, ui, th * c);
                if (chk) {
                    const float t = c + pdi;
                    violh = t;
                    magh = __builtin_fabsf(c) + __builtin_fabsf(pdi);
                    wmin = wi;
                    gap = -((double)wi * (double)t);
                    violz = ui + pdi;
                }
                wi = wn;
                yi = yp;
            }
        } else {
            th_next = a.theta[v + 1];
            bn_next = a.beta[v + 2];
        }
        if (chk) check_publish<float>(slots[0], violz, violh, wmin, gap, magh);
        GPAD_RSTAMP(4);
        __syncthreads();
        GPAD_RSTAMP(5);
        it = v + 1;
        th = th_next;
        bn = bn_next;
        if (chk) {
            const int st1 = check_stage1<float>(slots[0], nwaves, a.L, a.tol, a.tol_gap);
            bool verified = false;
            if (st1 & 1) {  // (A) nominated: decide on the direct chain G_L z, reset u to it
                if (isA && live) z_l[row] = zi;
                __syncthreads();
                float vc = -INFINITY, mc = 0.0f;
                if (!isA) {
                    const float cz = chain_regs<KB, K>(r, z_l);
                    if (live) {
                        ui = cz;
                        vc = cz + pdi;
                        mc = __builtin_fabsf(cz) + __builtin_fabsf(pdi);
                    }
                }
                check_publish<float>(slots[1], vc, vc, vc, 0.0, mc);
                __syncthreads();
                verified = check_verify<float>(slots[1], nwaves, a.L, a.tol);
            }
            done = check_code(st1, verified);
        }
        if (done) break;
    }
    if (live) {
        if (isA)
            zg[row] = done == 2 ? zhi : zi;  // test (B) certifies zhat
        else
            yg[row] = yi;
    }
    if (tid == 0) {
        a.iters[b] = it;
        a.conv[b] = done;
    }
}

// one launch of the (ka, kb) bucket pair's instantiation (gpad_chain.h with_buckets)
template <bool FLAT>
static hipError_t launch_res(const SolveArgs<float>& a, int ka, int kb, int threads, hipStream_t st) {
    with_buckets(ka, kb, [&](auto KA, auto KB) {
        hipLaunchKernelGGL((gpad_resident_kernel<decltype(KA)::value, decltype(KB)::value, FLAT>), dim3(a.batch),
                           dim3(threads), 0, st, a);
    });
    return hipGetLastError();
}

bool resident_supported(int n, int m) {
    const int mx = n > m ? n : m;
    const int threads = 64 * (((n + 63) >> 6) + ((m + 63) >> 6));
    return mx <= kResidentMaxRow && threads <= kResidentMaxThreads && n > 0 && m > 0;
}

hipError_t launch_resident(const SolveArgs<float>& a, hipStream_t st, bool* supported) {
    *supported = resident_supported(a.n, a.m);
    if (!*supported) return hipSuccess;
    const int threads = 64 * (((a.n + 63) >> 6) + ((a.m + 63) >> 6));
    return launch_res<false>(a, res_bucket(a.m), res_bucket(a.n), threads, st);  // A rows run over m, B rows over n
}

// flat battery variant: primal chains of 6N, constraint chains of n (flat G_L expanded to the
// k-major image a.GLt by the host at gpad_setup_flat); a.MGt = flat -ML (Nh x m row-major)
bool flat_resident_supported(int n, int m, int n_u) {
    if (n_u <= 0 || n_u > kFlatMaxCells || n % n_u) return false;
    const int Nh = n / n_u;
    const int laneA = n_u * ((Nh + 15) / 16) * 16;
    const int threads = 64 * ((laneA + 63) / 64) + 64 * ((m + 63) / 64);
    return 6 * Nh <= kResidentMaxRow && n <= kResidentMaxRow && threads <= kResidentMaxThreads &&
           m >= 4 * n;
}

hipError_t launch_flat_resident(const SolveArgs<float>& a, hipStream_t st) {
    const int Nh = a.n / a.n_u;
    const int laneA = a.n_u * ((Nh + 15) / 16) * 16;
    const int threads = 64 * ((laneA + 63) / 64) + 64 * ((a.m + 63) / 64);
    return launch_res<true>(a, res_bucket(6 * Nh), res_bucket(a.n), threads, st);
}

}  // namespace gpad
