// gpad_stream_solve.inc -- the text of the stream kernel, included by gpad_stream.hip once per variant:
// GPAD_STREAM_FK 0: gpad_stream_kernel<T>; 1: gpad_stream_farkas_kernel<T>, the same solve with the
// infeasibility certificate (gpad_farkas.h) at every fourth test.  Two inclusions rather than one device
// function inlined into two kernels: through such a function gpad_stream_kernel's code is not the one it
// has as a kernel of its own (tools/isa_diff.py), and with nothing bound it must be.
// GPAD_STREAM_RS 1 (with GPAD_STREAM_FK 0): gpad_stream_restart_kernel<T>, the same solve with the adaptive
// restart of the momentum (GPAD_OPT_RESTART, include/gpad.h): the workgroup's instance reads theta / beta at
// its own position `pos` of the schedule, and a decision iteration -- one whose count is a multiple of rs.R
// and which neither ends the solve nor is its last -- sums q = sum_i (w_i - y+_i)(y+_i - y_i) over its rows
// (the differences rounded in T, products and sum in fp64: per lane in row order, the wave butterfly, the
// waves' partials in order).  q > 0: w = y+ is written over the extrapolated w and pos returns to 0.
// Its additions are preprocessor blocks, not `if constexpr`: the other two variants must preprocess to the text
// they had without it -- dead declarations alone moved their register allocation (tools/isa_diff.py).
#if GPAD_STREAM_RS
#define GPAD_STREAM_POS pos
#else
#define GPAD_STREAM_POS v
#endif
template <typename T>
#if GPAD_STREAM_RS
__global__ __launch_bounds__(kStreamBlock) void gpad_stream_restart_kernel(SolveArgs<T> a, RestartArgs rs) {
    constexpr bool FK = false;
    const FarkasArgs fk{};  // (never read)
#elif GPAD_STREAM_FK
__global__ __launch_bounds__(kStreamBlock) void gpad_stream_farkas_kernel(SolveArgs<T> a, FarkasArgs fk) {
    constexpr bool FK = true;
#else
__global__ __launch_bounds__(kStreamBlock) void gpad_stream_kernel(SolveArgs<T> a) {
    constexpr bool FK = false;
    const FarkasArgs fk{};  // (never read)
#endif
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
#if GPAD_STREAM_RS
    int pos = 0, nrs = 0;  // the instance's position in the schedule, its restarts so far
#endif
    for (int v = 0; v < a.N; ++v) {
        const T th = a.theta[GPAD_STREAM_POS];
        const T omt = T(1) - th;
        const T bnext = a.beta[GPAD_STREAM_POS + 1];
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
        bool cert = false;  // a certificate event: every fourth test
        double fq = 0.0;    // q = sum y+ pD
        if constexpr (FK) cert = chk && ((v + 1) % (4 * a.check_every)) == 0;
        T violz = neg_inf<T>(), violh = neg_inf<T>(), wmin = -neg_inf<T>(), magh = T(0);
        double gap = 0.0;
#if GPAD_STREAM_RS
        // a restart decision follows this iteration, unless it ends the solve, on q = sum (w - y+)(y+ - y)
        const bool dec = v + 1 < a.N && ((v + 1) % rs.R) == 0;
        double rq = 0.0;
#endif
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
                            if constexpr (FK)
                                if (cert) fq += (double)yp * (double)pdi;
                        }
                    }
#if GPAD_STREAM_RS
                    if (dec) rq += (double)(wi - yp) * (double)(yp - yi);
#endif
                    s.w[i] = fmad(bnext, yp - yi, yp);               // next 8a
                    s.ys[i] = yp;
                }
            }
        }
        if (chk) check_publish<T>(s.slots, violz, violh, wmin, gap, magh);
        if constexpr (FK) {
            if (cert) {  // reduced as gap is: the wave butterfly, then the waves' partials in order
                fq = wave_sum(fq);
                if ((tid & 63) == 0) s.red[tid >> 6] = fq;
            }
        }
#if GPAD_STREAM_RS
        if (dec) {  // reduced as gap is: the wave butterfly, then the waves' partials in order
            rq = wave_sum(rq);
            if ((tid & 63) == 0) s.red[tid >> 6] = rq;
        }
#endif
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
            if constexpr (FK) {
                if (!done && cert) {  // Algorithm 1 first: any code of its wins
                    double q = 0.0;
                    for (int i = 0; i < nwaves; ++i) q += s.red[i];
                    if (q > 0.0 &&  // nominated (uniform): g'y+ < 0
                        farkas_decide<T>(GLt, ldm, n, m, s.ys, s.pd, fk.rabs + (size_t)b * fk.stride, fk.R, q, s.zp))
                        done = kCodeInfeasible;
                }
            }
        }
        if (done) break;
#if GPAD_STREAM_RS
        ++pos;
        if (dec) {  // Algorithm 1 came first: this iteration did not end the solve
            double q = 0.0;
            for (int i = 0; i < nwaves; ++i) q += s.red[i];
            if (q > 0.0) {  // (uniform) the momentum points uphill: drop it, the schedule starts again
                for (int i = tid; i < m; i += kStreamBlock) s.w[i] = s.ys[i];
                pos = 0;
                ++nrs;
                __syncthreads();
            }
        }
#endif
    }
    const T* zout = done >= 2 && !(FK && done == kCodeInfeasible) ? s.zh : s.zs;  // tests (B), (B'), (B'') certify zhat
    for (int i = tid; i < n; i += kStreamBlock) zg[i] = zout[i];
    for (int i = tid; i < m; i += kStreamBlock) yg[i] = s.ys[i];
    if (tid == 0) {
        a.iters[b] = it;
        a.conv[b] = done;
#if GPAD_STREAM_RS
        rs.count[b] = nrs;
#endif
    }
}
#undef GPAD_STREAM_POS

