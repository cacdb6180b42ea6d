// gpad_resident_solve.inc -- the text of the resident kernel, included once per variant:
// GPAD_RESIDENT_FK 0 (gpad_resident.hip): gpad_resident_kernel<KA, KB, FLAT>; 1 (gpad_resident_farkas.hip):
// gpad_resident_farkas_kernel<KA, KB>, the non-flat solve with the infeasibility certificate (gpad_farkas.h)
// at every fourth test.  Two inclusions for gpad_stream_solve.inc's reason: with nothing bound the kernel
// must be the code it has as a kernel of its own (tools/isa_diff.py).
#if GPAD_RESIDENT_FK
template <int KA, int KB, bool FLAT = false>
__global__ __launch_bounds__(kResidentMaxThreads) void gpad_resident_farkas_kernel(SolveArgs<float> a, FarkasArgs fk) {
    static_assert(!FLAT, "the flat variant carries no certificate: a bound on a flat setup is refused at the bind");
    // a certificate event: y+ and pD of the instance, the G/L waves' partials of q, the decision's scratch
    __shared__ float yf_l[KA], pf_l[KA];
    __shared__ double fq_l[kResidentMaxThreads / 64], ft_l[KB];
#else
template <int KA, int KB, bool FLAT>
__global__ __launch_bounds__(kResidentMaxThreads) void gpad_resident_kernel(SolveArgs<float> a) {
#endif
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
#if GPAD_RESIDENT_FK
    int kf = 4;  // tests to the next certificate event: cert <=> (v + 1) % (4 Kc) == 0
#endif
    for (int v = 0; v < a.N; ++v) {
        const bool chk = use_tol && --kc == 0;
        if (chk) kc = Kc;
#if GPAD_RESIDENT_FK
        const bool cert = chk && --kf == 0;
        if (cert) kf = 4;
        double fq = 0.0;  // this row's term of q = sum y+ pD
#endif
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
#if GPAD_RESIDENT_FK
                if (cert) {
                    yf_l[row] = yp;
                    pf_l[row] = pdi;
                    fq = (double)yp * (double)pdi;
                }
#endif
                wi = wn;
                yi = yp;
            }
        } else {
            th_next = a.theta[v + 1];
            bn_next = a.beta[v + 2];
        }
        if (chk) check_publish<float>(slots[0], violz, violh, wmin, gap, magh);
#if GPAD_RESIDENT_FK
        if (cert && !isA) {  // reduced as gap is: the wave butterfly, then the G/L waves' partials in order
            fq = wave_sum(fq);
            if ((tid & 63) == 0) fq_l[tid >> 6] = fq;
        }
#endif
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
#if GPAD_RESIDENT_FK
            if (!done && cert) {  // Algorithm 1 first: any code of its wins
                double q = 0.0;
                for (int i = nA; i < nwaves; ++i) q += fq_l[i];
                // nominated (uniform): g'y+ < 0.  The decision reads the k-major G_L image, not the row
                // registers: the stream kernel's text and bits
                if (q > 0.0 && farkas_decide<float>(a.GLt + (size_t)b * a.strideB, a.ldm, n, m, yf_l, pf_l,
                                                    fk.rabs + (size_t)b * fk.stride, fk.R, q, ft_l))
                    done = kCodeInfeasible;
            }
#endif
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
