// gpad_loop_panel_solve.inc -- the text of the panel loop kernel, included by gpad_loop_panel.hip once per variant:
// GPAD_LOOP_PANEL_FK 0: gpad_loop_panel_kernel<T, kCls>; 1: gpad_loop_panel_farkas_kernel<T, kCls>, the same loop
// with the infeasibility certificate (gpad_farkas.h; zbound: the caller's R): a column whose solve is certified
// infeasible takes its step boundary like any finished column, with code 5 and z* = z.  Two inclusions rather
// than a template parameter or a shared device function: either changes the names or the code of the existing
// instantiations (tools/isa_diff.py), which with nothing bound must be what they were.
template <int T, bool kCls = false>
#if GPAD_LOOP_PANEL_FK
__global__ __launch_bounds__(64 * T) void gpad_loop_panel_farkas_kernel(LoopArgs la, double zbound) {
#else
__global__ __launch_bounds__(64 * T) void gpad_loop_panel_kernel(LoopArgs la) {
#endif
    __shared__ LoopPanelLds<T> L;
    __shared__ int lp_sw[2];  // class loop only: the class the workgroup takes next (-1: none), its claimed base
#if GPAD_LOOP_PANEL_FK
    __shared__ double lp_fq[T][16];  // the certificate's nomination partials q of (row tile, column)
#endif
    extern __shared__ __attribute__((aligned(16))) float lp_dyn[];
    const SolveArgs<float>& a = la.s;

    const int tid = threadIdx.x, lane = tid & 63;
    const int t = __builtin_amdgcn_readfirstlane(tid >> 6);  // row tile of this wave
    const int j = lane >> 4, c = lane & 15;
    const int n = a.n, m = a.m, N = a.N, batch = a.batch;
    const int nx = la.nx, nxa = la.nx + la.ns, nu = la.nu, steps = la.steps;
    const int abytes = T * T * 1024;  // one packed operand
    // (class loop: rebuilt from class kc's image, the K images 2 * abytes apart, whenever kc changes)
    __amdgpu_buffer_rsrc_t PA1 =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.frag), 0, abytes, 0x00020000);
    __amdgpu_buffer_rsrc_t PA2 = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)a.frag + abytes), 0, abytes, 0x00020000);
    const int voff = t * 1024 + lane * 16;
    const int slot = t * 64 + lane;  // this lane's float4 in Wl / Zh / Gp / Pd
    float4* Wl4 = reinterpret_cast<float4*>(L.Wl);
    float4* Zh4 = reinterpret_cast<float4*>(L.Zh);
    float4* Gp4 = reinterpret_cast<float4*>(L.Gp);
    float4* Pd4 = reinterpret_cast<float4*>(L.Pd);
    TestSlot<float>* slots = L.slots;
    const bool use_tol = a.tol > 0.0;
    // row tiles whose results nobody reads: 16t >= n in GEMM 1, 16t >= m in GEMM 2 (their packed rows
    // are zero)
    const bool g1 = 16 * t < n, g2 = 16 * t < m;
    const int period = use_tol ? a.check_every : N;  // iterations between events

    float* X = lp_dyn;                       // [2][16][nxa]: [x_t; s_t] of column c at [t & 1][c]
    float* U = X + 32 * nxa;                 // [16][nu]: u = z*[0:nu] of a column at its boundary
    float* tab = U + 16 * nu;                // theta | beta when they fit
    const float* thp = a.theta;
    const float* btp = a.beta;
    if (lp_tab_in_lds<T>(N, nxa, nu)) {
        for (int i = tid; i < N + 2; i += 64 * T) {
            tab[i] = a.theta[i];
            tab[N + 2 + i] = a.beta[i];
        }
        thp = tab;
        btp = tab + (N + 2);
    }

    // per column (the same value in the 4 T lanes of column c)
    int pk = 16 * blockIdx.x + c;  // pack
    int ts = 0;                    // its MPC step
    int vc = 0;                    // iterations of its current solve
    bool active = pk < batch;
    // register r <-> row 16t + 4r + j of the column's pack
    float z[4] = {0.0f, 0.0f, 0.0f, 0.0f}, y[4] = {0.0f, 0.0f, 0.0f, 0.0f}, u[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float star[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // z* of a finished solve
    float th = 0.0f, bn = 0.0f;
    float gm = 0.0f;  // NaN-keeping max |g| of every g row this lane formed
    // the start is a boundary at which every column with a pack is refilled (static start: column c
    // of workgroup b takes pack 16 b + c; later packs are claimed from the counter, from 16 grid on;
    // the class loop has no static start: enter_class below)
    bool fin = active, was_last = true, first = true;
    // class loop: the workgroup's class, its first sorted position and its size (workgroup-uniform)
    int kc = 0, cb0 = 0, cnt = batch;
    // the workgroup takes class k with the 16 positions base .. base + 15 of it; every column restarts
    auto enter_class = [&](int k, int base) {
        kc = k;
        cb0 = la.cls_off[k];
        cnt = la.cls_off[k + 1] - cb0;
        const char* f = (const char*)a.frag + (size_t)k * 2 * (size_t)abytes;
        PA1 = __builtin_amdgcn_make_buffer_rsrc((void*)f, 0, abytes, 0x00020000);
        PA2 = __builtin_amdgcn_make_buffer_rsrc((void*)(f + abytes), 0, abytes, 0x00020000);
        pk = base + c < cnt ? cb0 + base + c : batch;
        ts = 0;
        vc = 0;
        active = pk < batch;
        fin = active;
        was_last = true;
        first = true;
    };
    if constexpr (kCls) {  // the class the host dealt; its first 16 packs come from the class's queue too
        if (tid == 0) {
            const int k = la.cls_start[blockIdx.x];
            lp_sw[0] = k;
            lp_sw[1] = atomicAdd(a.qctr + k, 16);
        }
        __syncthreads();
        enter_class(__builtin_amdgcn_readfirstlane(lp_sw[0]), __builtin_amdgcn_readfirstlane(lp_sw[1]));
    }
    if (t == 0 && j == 0) {
        L.col[c].pack = -1;
        L.col[c].t = 0;
        L.col[c].refill = active ? pk : -1;
    }
    __syncthreads();  // L.col (and the tables) published
    int ke = period;  // iterations to the next event

    while (true) {
        if (!first) {
            // schedule prefetched one iteration ahead (tables hold N + 2 entries; vc < N here)
            const float th_next = thp[vc + 1], bn_next = btp[vc + 2];
            const bool ev = --ke == 0;
            if (ev) ke = period;
            const bool chk = use_tol && ev;
            const float omt = 1.0f - th;
            // ---- GEMM 1 and GEMM 2 with their epilogues: gpad_panel.h's, as gpad_panel_kernel calls them ----
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
            if (g1) acc = panel_gemm<T>(PA1, L.Wl, voff, lane);
            panel_primal(acc, Gp4, Zh4, slot, omt, th, active, z);
            __syncthreads();
            acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (g2) acc = panel_gemm<T>(PA2, L.Zh, voff, lane);
#if GPAD_LOOP_PANEL_FK
            // a certificate event of this lane's column: its solve's count a multiple of 4 K (per column: the
            // columns of a panel are at different counts)
            const bool cert = chk && active && ((vc + 1) % (4 * a.check_every)) == 0;
            FarkasPart fq;
            TestPart<float> part = panel_dual<true>(acc, Wl4, Pd4, slot, omt, th, bn, use_tol, chk, active, 16 * t + j, m,
                                                    y, u, cert, &fq);
#else
            TestPart<float> part = panel_dual(acc, Wl4, Pd4, slot, omt, th, bn, use_tol, chk, active, 16 * t + j, m, y, u);
#endif
            th = th_next;
            bn = bn_next;
            if (active) ++vc;
            __syncthreads();
            if (!ev) continue;

            // this iteration's zhat (own slot), before a verification GEMM puts z there
            const float4 h4 = Zh4[slot];
            const float zk[4] = {h4.x, h4.y, h4.z, h4.w};
            // ---- Algorithm 1 test, per column: lane groups j, then row tiles through LDS ----
            int code = 0;
            if (chk) {
                part.fold();
                part.put(slots[t], c, j == 0);
#if GPAD_LOOP_PANEL_FK
                fq.fold();
                if (j == 0) lp_fq[t][c] = fq.q;
#endif
                __syncthreads();
                int st1 = 0;
                if (active) st1 = stage1<float, T>(slots, 0, T, c, a.L, a.tol, a.tol_gap).bits;
                bool ver = false;
                if (__syncthreads_or(st1 & 1)) {  // (A) nominated somewhere: G_L z for the panel
                    Zh4[slot] = make_float4(z[0], z[1], z[2], z[3]);
                    __syncthreads();
                    f32x4 cz = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (g2) cz = panel_gemm<T>(PA2, L.Zh, voff, lane);
                    const float4 p4 = Pd4[slot];
                    const float pd[4] = {p4.x, p4.y, p4.z, p4.w};
                    VerPart<float> vp;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if ((st1 & 1) && (16 * t + 4 * r + j) < m) {
                            u[r] = cz[r];  // the recursion restarts from the direct value
                            vp.row(cz[r], pd[r]);
                        }
                    }
                    vp.fold();
                    vp.put(slots[t], c, j == 0);
                    __syncthreads();
                    if (st1 & 1) ver = verified<float, T>(slots, 0, T, c, a.L, a.tol);
                }
                code = check_code(st1, ver);
#if GPAD_LOOP_PANEL_FK
                {  // the infeasibility certificate (gpad_farkas.h), after Algorithm 1: any code of its wins
                    double q = 0.0;
                    for (int s = 0; s < T; ++s) q += lp_fq[s][c];
                    const bool certc = cert && code == 0;
                    const unsigned nomm = (unsigned)__ballot(certc && j == 0 && q > 0.0) & 0xffffu;  // uniform
                    if (nomm) {
                        // Zh is free (zk holds this iteration's zhat): t = G_L' y+ and r there.  y+ of a nominated
                        // column goes through its pack's own row of a.y, which only the pack's last step fills
                        double* tb = reinterpret_cast<double*>(L.Zh);
                        if (certc && (nomm >> c & 1u)) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int i = 16 * t + 4 * r + j;
                                if (i < m) a.y[(size_t)pk * m + i] = y[r];
                            }
                        }
                        __syncthreads();
                        const float* F2 = reinterpret_cast<const float*>((const char*)a.frag + (size_t)kc * 2 * (size_t)abytes +
                                                                         abytes);  // (class kc's G_L image; kc = 0 without classes)
                        for (int cc = 0; cc < 16; ++cc) {  // uniform
                            if (!(nomm >> cc & 1u)) continue;
                            const int pc = __shfl(pk, cc, 64);
                            const double qc = lane_read(q, cc);
                            if (farkas_decide_panel<T>(F2, L.Pd, cc, a.y + (size_t)pc * m, n, m, zbound, qc, tb) &&
                                c == cc && certc)
                                code = kCodeInfeasible;
                        }
                    }
                }
#endif
            }
            // ---- step boundary of the columns whose solve ended ------------------------------
            fin = active && (code != 0 || vc >= N);
            if (!__syncthreads_or(fin ? 1 : 0)) continue;  // (also: Zh and the slots are free again)
            was_last = ts + 1 == steps;
            if (fin) {
                // z*: (B) certifies zhat
#pragma unroll
                for (int r = 0; r < 4; ++r) star[r] = code == 2 ? zk[r] : z[r];
                const size_t tb = (size_t)ts * (size_t)batch + (size_t)pk;  // (step, pack) row of xs / us
                if (t == 0 && j == 0) {  // the counters of step ts: [iters[batch] | conv[batch]]
                    a.iters[(size_t)(2 * ts) * batch + pk] = vc;
                    a.conv[(size_t)(2 * ts + 1) * batch + pk] = code;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * t + 4 * r + j;
                    if (i < nu) {
                        U[c * nu + i] = star[r];
                        if (la.us) la.us[tb * nu + i] = star[r];
                    }
                    if (was_last) {  // the pack's results
                        if (i < n) a.z[(size_t)pk * n + i] = star[r];
                        if (i < m) a.y[(size_t)pk * m + i] = y[r];
                    }
                }
            }
            if (t == 0) {  // lanes 0..15 of wave 0 speak for the columns: one claim per event
                const bool want = fin && was_last && j == 0;
                const unsigned long long lv = __ballot(want);
                int base = 0;
                if (lane == 0 && lv) base = atomicAdd(a.qctr + kc, (int)__popcll(lv));
                base = __shfl(base, 0, 64);
                if (j == 0) {
                    int np = -1;
                    if (want) {
                        np = base + (int)__popcll(lv & ((1ull << lane) - 1ull));
                        if constexpr (kCls) {  // the next position of class kc, or none left in it
                            np = np < cnt ? cb0 + np : batch;
                        } else {
                            np += 16 * (int)gridDim.x;
                            if (np > batch) np = batch;
                        }
                    }
                    L.col[c].pack = fin ? pk : -1;
                    L.col[c].t = ts;
                    L.col[c].refill = np;
                }
            }
            __syncthreads();  // U, L.col published
            // x+ = A x (+ E s_t: the row is [A E]) + B u, one fma chain (plant_step_kernel's order);
            // next to it the next step's signals.  Work item = (column, row of the state row).
            for (int w = tid; w < 16 * nxa; w += 64 * T) {
                const int col = w & 15, row = w >> 4;
                const int pc = L.col[col].pack, tc = L.col[col].t;
                if (pc < 0) continue;
                const bool lastc = tc + 1 == steps;
                const float* xc = X + ((tc & 1) * 16 + col) * nxa;
                float* xn = X + (((tc + 1) & 1) * 16 + col) * nxa;
                if (row < nx) {
                    const size_t pi = la.per_plant ? (size_t)(kCls ? kc : pc) : 0;  // (class loop: a copy per class)
                    const float* Ar = la.A + (pi * nx + row) * nxa;
                    const float* Br = la.B + (pi * nx + row) * nu;
                    float acc = 0.0f;
#pragma unroll 1
                    for (int k = 0; k < nxa; ++k) acc = __builtin_fmaf(Ar[k], xc[k], acc);
#pragma unroll 1
                    for (int k = 0; k < nu; ++k) acc = __builtin_fmaf(Br[k], U[col * nu + k], acc);
                    if (la.xs) la.xs[((size_t)tc * batch + pc) * nx + row] = xc[row];
                    if (lastc) la.x_out[(size_t)pc * nx + row] = acc;
                    else xn[row] = acc;
                } else if (!lastc) {
                    xn[row] = la.S[((size_t)(tc + 1) * batch + pc) * la.ns + (row - nx)];
                }
            }
            __syncthreads();  // x_{t+1} published; x_t, U and the old L.col readers done
        }
        first = false;
        // ---- the columns at a boundary start their next solve ----------------------------------
        if (fin) {
            if (was_last) {  // the next pack from the queue, at its step 0
                pk = L.col[c].refill;
                ts = 0;
                active = pk < batch;
                if (!active) vc = 0;  // (an idle column's schedule prefetch stays inside the tables)
            } else {
                ts += 1;
            }
        }
        for (int w = tid; w < 16 * nxa; w += 64 * T) {  // a refilled column's [x_0; S[0][pack]]
            const int col = w & 15, row = w >> 4;
            const int rp = L.col[col].refill;
            if (rp < 0 || rp >= batch) continue;
            X[col * nxa + row] = row < nx ? la.x_in[(size_t)rp * nx + row] : la.S[(size_t)rp * la.ns + (row - nx)];
        }
        const bool go = fin && active;  // this lane's column starts a solve
        if (go) {  // cold: z = y = 0 (acceldualgrad.m:16-17); warm: z_{-1} = z*, y_0 = y* (a new pack: the caller's)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * t + 4 * r + j;
                float zv = 0.0f, yv = 0.0f;
                if (la.warm) {
                    if (was_last) {
                        if (i < n) zv = a.z[(size_t)pk * n + i];
                        if (i < m) yv = a.y[(size_t)pk * m + i];
                    } else {
                        if (i < n) zv = star[r];
                        if (i < m) yv = y[r];
                    }
                }
                z[r] = zv;
                y[r] = yv;
            }
        }
        __syncthreads();  // X published
        if (go) {
            // M(x), g(x) of this lane's rows (affine2_kernel's order): acc = c0[i] (0 if absent), then
            // fma(P[i][k], x[k], acc) for ascending k over the nx + ns columns
            const float* xr = X + ((ts & 1) * 16 + c) * nxa;
            const size_t pi = la.per_plant ? (size_t)(kCls ? kc : pk) : 0;
            const float b0 = btp[0];
            float gp[4], pd[4], w[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * t + 4 * r + j;
                gp[r] = 0.0f;
                pd[r] = 0.0f;
                if (i < n) {
                    float acc = la.M0 ? la.M0[pi * n + i] : 0.0f;
                    const float* P = la.PM + (pi * n + i) * nxa;
#pragma unroll 1
                    for (int k = 0; k < nxa; ++k) acc = __builtin_fmaf(P[k], xr[k], acc);
                    gp[r] = acc;
                }
                if (i < m) {
                    float acc = la.g0 ? la.g0[pi * m + i] : 0.0f;
                    const float* P = la.Pg + (pi * m + i) * nxa;
#pragma unroll 1
                    for (int k = 0; k < nxa; ++k) acc = __builtin_fmaf(P[k], xr[k], acc);
                    gm = absmax_nan(gm, acc);
                    pd[r] = (float)(a.gscale * (double)acc);
                }
                // w_0 = y_0 + beta_0 (y_0 - y_{-1}), y_{-1} = y_0
                w[r] = __builtin_fmaf(b0, y[r] - y[r], y[r]);
                u[r] = 0.0f;
            }
            Gp4[slot] = make_float4(gp[0], gp[1], gp[2], gp[3]);
            Pd4[slot] = make_float4(pd[0], pd[1], pd[2], pd[3]);
            Wl4[slot] = make_float4(w[0], w[1], w[2], w[3]);
            vc = 0;
            th = thp[0];
            bn = btp[1];
        }
        if (use_tol) {  // u = G_L z_{-1}: one GEMM over the panel's z, taken by the starting columns
            Zh4[slot] = make_float4(z[0], z[1], z[2], z[3]);
            __syncthreads();
            f32x4 cz = {0.0f, 0.0f, 0.0f, 0.0f};
            if (g2) cz = panel_gemm<T>(PA2, L.Zh, voff, lane);
            if (go) {
#pragma unroll
                for (int r = 0; r < 4; ++r) u[r] = cz[r];
            }
        }
        fin = false;
        if (!__syncthreads_or(active ? 1 : 0)) {  // (also publishes Wl, Gp, Pd; Zh free)
            if constexpr (!kCls) {
                break;
            } else {
                // class kc has nothing left for this workgroup: on to the next class with unclaimed packs
                if (tid == 0) {
                    int nk = -1, base = 0;
                    for (int i = 1; i < la.cls_K && nk < 0; ++i) {
                        const int k = kc + i < la.cls_K ? kc + i : kc + i - la.cls_K;
                        const int ck = la.cls_off[k + 1] - la.cls_off[k];
                        if (__hip_atomic_load(a.qctr + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= ck) continue;
                        base = atomicAdd(a.qctr + k, 16);
                        if (base < ck) nk = k;  // (else other workgroups took the last ones meanwhile)
                    }
                    lp_sw[0] = nk;
                    lp_sw[1] = base;
                }
                __syncthreads();
                const int nk = __builtin_amdgcn_readfirstlane(lp_sw[0]);
                if (nk < 0) break;
                enter_class(nk, __builtin_amdgcn_readfirstlane(lp_sw[1]));
                ke = period;
                if (t == 0 && j == 0) {
                    L.col[c].pack = -1;
                    L.col[c].t = 0;
                    L.col[c].refill = active ? pk : -1;
                }
                __syncthreads();  // L.col published (and lp_sw read by every wave)
            }
        }
    }

    // the run's max |g| (the certification floor): this workgroup's slot, workgroup 0 zeroes the rest
    if (la.gmax) {
        const float wm = wave_reduce(gm, OpAbsmaxNan{});
        if (lane == 0) L.gmw[t] = wm;
        __syncthreads();
        if (tid == 0) {
            float mx = 0.0f;
            for (int w = 0; w < T; ++w) mx = absmax_nan(mx, L.gmw[w]);
            la.gmax[blockIdx.x] = (double)mx;
        }
        if (blockIdx.x == 0)
            for (int i = (int)gridDim.x + tid; i < kAbsmaxMaxBlocks; i += 64 * T) la.gmax[i] = 0.0;
    }
}

