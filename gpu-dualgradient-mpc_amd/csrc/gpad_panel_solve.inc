// gpad_panel_solve.inc -- the text of the T-wave panel kernel, included by gpad_panel.hip once per variant:
// GPAD_PANEL_FK 0: gpad_panel_kernel<T>; 1: gpad_panel_farkas_kernel<T>, the same solve with the infeasibility
// certificate (gpad_farkas.h), at every fourth test, after Algorithm 1,
// the columns nominated by q > 0 are decided one after the other by the whole workgroup, and a certified
// column leaves the panel like a converged one (code 5, z* = z, y* = y+).  Two inclusions rather than one
// device function inlined into two kernels: through such a function gpad_panel_kernel's code is not the one
// it has as a kernel of its own (tools/isa_diff.py), and with nothing bound it must be.
// GPAD_PANEL_RS 1 (with GPAD_PANEL_FK 0): gpad_panel_restart_kernel<T>, the same solve with the adaptive restart
// of the momentum (GPAD_OPT_RESTART, include/gpad.h).  Every column carries its own position `pos` in the
// theta / beta tables (read per lane from global memory) and its restart count.  On a decision iteration -- v a
// multiple of rs.R below N; v is every column's own count, also in a carried phase -- a lane sums
// (double)(w - y+) * (double)(y+ - y) over its four rows, the lane groups j are folded by two butterflies and
// the T row tiles meet through one LDS word per (tile, column), read after the iteration's closing barrier.
// Algorithm 1 comes first; a column with q > 0 that goes on then writes w = y+ over its slot and returns to
// position 0, and one more barrier follows, on decision iterations only.  A parked column keeps pos and count
// in rs.pos / rs.count.  The additions are preprocessor blocks: the other variants keep their text.
template <int T>
#if GPAD_PANEL_RS
__global__ __launch_bounds__(64 * T) void gpad_panel_restart_kernel(SolveArgs<float> a, RestartArgs rs) {
    constexpr bool FK = false;
#elif GPAD_PANEL_FK
__global__ __launch_bounds__(64 * T) void gpad_panel_farkas_kernel(SolveArgs<float> a, FarkasArgs fk) {
    constexpr bool FK = true;
#else
__global__ __launch_bounds__(64 * T) void gpad_panel_kernel(SolveArgs<float> a) {
    constexpr bool FK = false;
#endif
    __shared__ __attribute__((aligned(16))) float Wl[T * 256];  // [T][64][4] w    (B of GEMM 1)
    __shared__ __attribute__((aligned(16))) float Zh[T * 256];  // [T][64][4] zhat (B of GEMM 2)
    // per-lane constants of the current instance, parked in LDS rather than VGPRs:
    // g_P rows and p_D rows of tile t
    __shared__ __attribute__((aligned(16))) float Gp[T * 256];
    __shared__ __attribute__((aligned(16))) float Pd[T * 256];
    __shared__ TestSlot<float> slots[T];
#if GPAD_PANEL_FK
    __shared__ double fqs[T][16];  // the nomination partials q of (row tile, column)
#endif
#if GPAD_PANEL_RS
    __shared__ double rqs[T][16];  // the restart partials q of (row tile, column)
#endif

    const int lane = threadIdx.x & 63;
    const int t = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // row tile of this wave
    const int j = lane >> 4, c = lane & 15;
    const int n = a.n, m = a.m, N = a.N, K = a.check_every;
    const int abytes = T * T * 1024;  // one packed operand
    const __amdgpu_buffer_rsrc_t PA1 =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.frag), 0, abytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t PA2 = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)a.frag + abytes), 0, abytes, 0x00020000);
    const int voff = t * 1024 + lane * 16;
    const int slot = t * 64 + lane;  // this lane's float4 in Wl / Zh / Gp / Pd
    float4* Wl4 = reinterpret_cast<float4*>(Wl);
    float4* Zh4 = reinterpret_cast<float4*>(Zh);
    float4* Gp4 = reinterpret_cast<float4*>(Gp);
    float4* Pd4 = reinterpret_cast<float4*>(Pd);
    const bool use_tol = a.tol > 0.0;
    const bool fresh = a.v_begin == 0;      // first phase: start from the caller's z0, y0
    const bool carry = a.v_end < N;         // not the last phase: park the survivors
    const int count = a.count_in ? __builtin_amdgcn_readfirstlane(*a.count_in) : a.batch;
    if (a.count_in && count <= a.fin_thresh) return;  // the resident finisher has them
    const int panels = (count + 15) / 16;

    for (int p = blockIdx.x; p < panels; p += gridDim.x) {
        // ---- load the panel: column c <-> instance idx[16p + c] -------------------------
        const int k = 16 * p + c;
        bool active = k < count;
        const int inst = active ? (a.idx_in ? a.idx_in[k] : k) : 0;
        // register r <-> row 16t + 4r + j of the column's instance
        float z[4], y[4], u[4];
        {
            float gp[4], pd[4], w[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * t + 4 * r + j;
                const bool okn = active && i < n, okm = active && i < m;
                z[r] = okn ? a.z[(size_t)inst * n + i] : 0.0f;
                gp[r] = okn ? a.gP[(size_t)inst * a.ld_gP + i] : 0.0f;
                y[r] = okm ? a.y[(size_t)inst * m + i] : 0.0f;
                pd[r] = okm ? (float)(a.gscale * (double)a.g[(size_t)inst * a.ld_g + i]) : 0.0f;
                if (fresh) {  // w_0 = y_0 + beta_0 (y_0 - y_{-1}), y_{-1} = y_0; u set below
                    w[r] = __builtin_fmaf(a.beta[0], y[r] - y[r], y[r]);
                    u[r] = 0.0f;
                } else {
                    w[r] = okm ? a.wc[(size_t)inst * m + i] : 0.0f;
                    u[r] = okm && use_tol ? a.uc[(size_t)inst * m + i] : 0.0f;
                }
            }
            Gp4[slot] = make_float4(gp[0], gp[1], gp[2], gp[3]);
            Pd4[slot] = make_float4(pd[0], pd[1], pd[2], pd[3]);
            Wl4[slot] = make_float4(w[0], w[1], w[2], w[3]);
        }
        if (fresh && use_tol) {  // u = G_L z_{-1} (one GEMM for the panel); then the 8c recursion
            Zh4[slot] = make_float4(z[0], z[1], z[2], z[3]);
            __syncthreads();
            const f32x4 cz = panel_gemm<T>(PA2, Zh, voff, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) u[r] = cz[r];
        }
        __syncthreads();

        int v = a.v_begin;
#if GPAD_PANEL_RS
        int pos = 0, nrs = 0;  // the column's position in the schedule and its restarts (the same in every lane of it)
        if (!fresh && active) {
            pos = rs.pos[inst];
            nrs = rs.count[inst];
        }
        while (true) {
            const float th = a.theta[pos], bn = a.beta[pos + 1];
            ++pos;
            ++v;
            const bool dec = v < N && (v % rs.R) == 0;  // uniform: a restart decision follows this iteration
            float4 wo4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float yo[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (dec) {  // this iteration's w (own slot) and y, which panel_dual overwrites
                wo4 = Wl4[slot];
#pragma unroll
                for (int r = 0; r < 4; ++r) yo[r] = y[r];
            }
#else
        float th = a.theta[v], bn = a.beta[v + 1];
        while (true) {
            // schedule prefetched one iteration ahead (tables hold N + 2 entries)
            const float th_next = a.theta[v + 1], bn_next = a.beta[v + 2];
            ++v;
#endif
            const bool chk = use_tol && (v % K) == 0;  // uniform: every column is at iteration v
            const bool cert = FK && chk && (v % (4 * K)) == 0;  // a certificate event
            FarkasPart fq;
            const float omt = 1.0f - th;
            // ---- GEMM 1 + epilogue: zhat = -ML w - g_P (8b), z = (1-th) z + th zhat (8c) ----
            panel_primal(panel_gemm<T>(PA1, Wl, voff, lane), Gp4, Zh4, slot, omt, th, active, z);
            __syncthreads();
            // ---- GEMM 2 + epilogue: y+ = [w + G_L zhat + p_D]+ (8d), next w (8a) ----------
            TestPart<float> part = panel_dual<FK>(panel_gemm<T>(PA2, Zh, voff, lane), Wl4, Pd4, slot, omt, th, bn,
                                                  use_tol, chk, active, 16 * t + j, m, y, u, cert, &fq);
#if GPAD_PANEL_RS
            if (dec) {
                const float wo[4] = {wo4.x, wo4.y, wo4.z, wo4.w};
                double q = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (active && (16 * t + 4 * r + j) < m) q += (double)(wo[r] - y[r]) * (double)(y[r] - yo[r]);
                q += __shfl_xor(q, 16, 64);
                q += __shfl_xor(q, 32, 64);
                if (j == 0) rqs[t][c] = q;
            }
            __syncthreads();
            bool rhit = false;  // the column restarts, unless this iteration ends its solve
            if (dec) {
                double q = 0.0;
                for (int s = 0; s < T; ++s) q += rqs[s][c];
                rhit = q > 0.0;
            }
            if (!chk && v < a.v_end) {
                if (dec) {
                    if (rhit && active) {
                        Wl4[slot] = make_float4(y[0], y[1], y[2], y[3]);
                        pos = 0;
                        ++nrs;
                    }
                    __syncthreads();
                }
                continue;
            }
#else
            th = th_next;
            bn = bn_next;
            __syncthreads();
            if (!chk && v < a.v_end) continue;
#endif

            // ---- Algorithm 1 test, per column: lane groups j, then row tiles through LDS ----
            int code = 0;
            bool zh_out = true;  // this iteration's zhat still in Zh (no verification GEMM ran)
            if (chk) {
                part.fold();
                part.put(slots[t], c, j == 0);
#if GPAD_PANEL_FK
                if (cert) {
                    fq.fold();
                    if (j == 0) fqs[t][c] = fq.q;
                }
#endif
                __syncthreads();
                int st1 = 0;
                if (active) st1 = stage1<float, T>(slots, 0, T, c, a.L, a.tol, a.tol_gap).bits;
                bool ver = false;
                if (__syncthreads_or(st1 & 1)) {  // (A) nominated somewhere: G_L z for the panel
                    zh_out = false;
                    if (st1 & 2) {  // test (B)'s result (zhat) out now: Zh is about to hold z
                        const float4 h4 = Zh4[slot];
                        const float zh[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int i = 16 * t + 4 * r + j;
                            if (i < n) a.z[(size_t)inst * n + i] = zh[r];
                        }
                    }
                    Zh4[slot] = make_float4(z[0], z[1], z[2], z[3]);
                    __syncthreads();
                    const f32x4 cz = panel_gemm<T>(PA2, Zh, voff, lane);
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
            }
            // ---- finished columns: results out ---------------------------------------------
            // (a certificate event decides first, below: a column at N may still end with code 5)
            if (active && (code != 0 || (v >= N && !cert))) {
                const float4 h4 = Zh4[slot];  // this iteration's zhat (own slot), unless verified over
                const float zh[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * t + 4 * r + j;
                    if (i < n && (code != 2 || zh_out)) a.z[(size_t)inst * n + i] = code == 2 ? zh[r] : z[r];
                    if (i < m) a.y[(size_t)inst * m + i] = y[r];
                }
                if (t == 0 && j == 0) {
                    a.iters[inst] = v;
                    a.conv[inst] = code;
#if GPAD_PANEL_RS
                    rs.count[inst] = nrs;
#endif
                }
                active = false;
            }
#if GPAD_PANEL_RS
            if (dec) {  // Algorithm 1 came first: the columns that go on (also into the next phase)
                if (rhit && active) {
                    Wl4[slot] = make_float4(y[0], y[1], y[2], y[3]);
                    pos = 0;
                    ++nrs;
                }
                __syncthreads();
            }
#endif
#if GPAD_PANEL_FK
            if (cert) {
                // nomination, per column and the same in every wave: q = the slots' partials in order
                double q = 0.0;
                for (int s = 0; s < T; ++s) q += fqs[s][c];
                const unsigned nomm = (unsigned)__ballot(active && j == 0 && q > 0.0) & 0xffffu;  // uniform
                if (nomm) {
                    // Zh is free (zhat went out above, the next GEMM 1 rewrites it): t = G_L' y+ there.
                    // y+ of the nominated columns goes through the instance's own row of a.y
                    double* tb = reinterpret_cast<double*>(Zh);
                    if (active && (nomm >> c & 1u)) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int i = 16 * t + 4 * r + j;
                            if (i < m) a.y[(size_t)inst * m + i] = y[r];
                        }
                    }
                    __syncthreads();
                    for (int cc = 0; cc < 16; ++cc) {  // uniform
                        if (!(nomm >> cc & 1u)) continue;
                        const int ic = __shfl(inst, cc, 64);
                        const double qc = lane_read(q, cc);
                        if (farkas_decide_panel<T>(reinterpret_cast<const float*>(a.frag) + T * T * 256, Pd, cc,
                                               a.y + (size_t)ic * m, n, m, fk.R, qc, tb) &&
                            c == cc && active)
                            code = kCodeInfeasible;
                    }
                }
                if (active && (code != 0 || v >= N)) {  // certified, or the cap: z* = z, y* = y+
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = 16 * t + 4 * r + j;
                        if (i < n) a.z[(size_t)inst * n + i] = z[r];
                        if (i < m) a.y[(size_t)inst * m + i] = y[r];
                    }
                    if (t == 0 && j == 0) {
                        a.iters[inst] = v;
                        a.conv[inst] = code;
                    }
                    active = false;
                }
            }
#endif
            if (v >= a.v_end || !__syncthreads_or(active ? 1 : 0)) break;
        }
        // ---- phase end: park the survivors for the next phase ------------------------------
        if (carry) {
            const bool park = active && v >= a.v_end;
            if (park) {
                const float4 w4 = Wl4[slot];  // w of iteration v (own slot)
                const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * t + 4 * r + j;
                    if (i < n) a.z[(size_t)inst * n + i] = z[r];
                    if (i < m) {
                        a.y[(size_t)inst * m + i] = y[r];
                        a.wc[(size_t)inst * m + i] = wv[r];
                        if (use_tol) a.uc[(size_t)inst * m + i] = u[r];
                    }
                }
#if GPAD_PANEL_RS
                if (t == 0 && j == 0) {
                    rs.pos[inst] = pos;
                    rs.count[inst] = nrs;
                }
#endif
            }
            if (t == 0) list_survivors(a, p, park, inst, lane, j);  // lanes 0..15 speak for the columns
        }
        __syncthreads();  // the next panel reuses the LDS tiles
    }
}

