// gpad_setup.cpp -- binding a problem to a handle: the packed device copies of the constant matrices
// (k-major -ML and G/L, the MFMA fragment images), the Hessian, the flat battery form, the theta/beta
// table, the one-time QP precompute and the step-bound estimate (gpad_lipschitz).  Replaces the set-up
// half of the reference's host driver (main.cu:79-203: file read, 9 cudaMallocs, H2D copies).
#include <algorithm>
#include <cmath>

#include "gpad_farkas.h"
#include "gpad_host.h"

int validate_dims(const gpad_dims_t* d) {
    if (!d) return fail(GPAD_ERR_INVALID, "null dims");
    if (d->n <= 0 || d->m <= 0 || d->batch <= 0)
        return fail(GPAD_ERR_INVALID, "dims: n, m, batch must be positive");
    if (d->dtype != GPAD_DTYPE_F32 && d->dtype != GPAD_DTYPE_F64)
        return fail(GPAD_ERR_INVALID, "dims: bad dtype");
    if (d->memory != GPAD_MEM_HOST && d->memory != GPAD_MEM_DEVICE)
        return fail(GPAD_ERR_INVALID, "dims: bad memory kind");
    if (d->schedule != GPAD_SCHEDULE_MATLAB && d->schedule != GPAD_SCHEDULE_PAPER)
        return fail(GPAD_ERR_INVALID, "dims: bad schedule");
    if (d->kernel < GPAD_KERNEL_AUTO || d->kernel > GPAD_KERNEL_PANEL)
        return fail(GPAD_ERR_INVALID, "dims: bad kernel");
    if (!std::isfinite(d->tol_gap)) return fail(GPAD_ERR_INVALID, "dims: tol_gap must be finite");
    if (d->reserved != 0) return fail(GPAD_ERR_INVALID, "dims: reserved must be 0");
    return GPAD_OK;
}

void unbind_problem(gpad_handle_t h) {
    end_classes(h);
    h->ready = false;
    h->flat = false;
    h->own_plant.ns = 0;
    h->shadow_ok = false;
    h->hess_ok = false;
    h->zbound = 0.0;
    h->frag64_ok = false;
    h->hfrag64_ok = false;
    h->plan.nph = 0;
    h->p64_order_batch = 0;  // (the previous counts order nothing)
    h->flat_vpred = 0;
    h->plan_pending = false;
    h->last_phased = false;
}

static int setup_impl(gpad_handle_t h, const gpad_dims_t* d, const void* A, const void* B, double L,
                      bool scaled) {
    if (!h) return fail(GPAD_ERR_INVALID, "gpad_setup: null handle");
    int rc = validate_dims(d);
    if (rc) return rc;
    if (!A || !B) return fail(GPAD_ERR_INVALID, "gpad_setup: null matrix");
    if (!(L > 0.0) || !std::isfinite(L)) return fail(GPAD_ERR_INVALID, "gpad_setup: L must be > 0");
    HIP_TRY(hipSetDevice(h->device));
    unbind_problem(h);
    h->dims = *d;
    if (h->dims.check_every <= 0) h->dims.check_every = 10;
    h->L = L;
    h->scaled = scaled;
    const int n = d->n, m = d->m;
    h->ldn = round4(n);
    h->ldm = round4(m);
    const size_t es = esize(d->dtype);
    const int nmats = d->shared ? 1 : d->batch;
    const size_t a_elems = (size_t)m * h->ldn, b_elems = (size_t)n * h->ldm;
    if ((rc = h->MGt.ensure(es * a_elems * nmats))) return rc;
    if ((rc = h->GLt.ensure(es * b_elems * nmats))) return rc;
    const size_t raw = (size_t)n * m * nmats * es;
    const void* dA = A;
    const void* dB = B;
    if (d->memory == GPAD_MEM_HOST) {
        if ((rc = h->stage.ensure(2 * raw))) return rc;
        HIP_TRY(hipMemcpyAsync(h->stage.p, A, raw, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync((char*)h->stage.p + raw, B, raw, hipMemcpyHostToDevice, h->stream));
        dA = h->stage.p;
        dB = (char*)h->stage.p + raw;
    }
    // -ML -> k-major [m][ldn];  G/L -> k-major [n][ldm]   (acceldualgrad.m:20,22)
    const double sa = scaled ? 1.0 : -1.0;
    const double sb = scaled ? 1.0 : 1.0 / L;
    const long long in_stride = d->shared ? 0 : (long long)n * m;
    if (d->dtype == GPAD_DTYPE_F32) {
        HIP_TRY(gpad::launch_pack_kmajor<float>((const float*)dA, (float*)h->MGt.p, n, m, h->ldn, sa,
                                                nmats, in_stride, (long long)a_elems, h->stream));
        HIP_TRY(gpad::launch_pack_kmajor<float>((const float*)dB, (float*)h->GLt.p, m, n, h->ldm, sb,
                                                nmats, in_stride, (long long)b_elems, h->stream));
    } else {
        HIP_TRY(gpad::launch_pack_kmajor<double>((const double*)dA, (double*)h->MGt.p, n, m, h->ldn, sa,
                                                 nmats, in_stride, (long long)a_elems, h->stream));
        HIP_TRY(gpad::launch_pack_kmajor<double>((const double*)dB, (double*)h->GLt.p, m, n, h->ldm, sb,
                                                 nmats, in_stride, (long long)b_elems, h->stream));
    }
    // f64 panels: -ML | G_L in the f64 MFMA fragment layout (gpad_panel64.hip)
    if (d->shared && d->dtype == GPAD_DTYPE_F64 && gpad::panel64_supported(n, m)) {
        const int T = gpad::panel64_tiles(n, m);
        const size_t ob = gpad::panel64_frag_bytes(n, m);
        if ((rc = h->frag64.ensure(2 * ob))) return rc;
        HIP_TRY(gpad::launch_pack_panel64((const double*)dA, n, m, sa, T, h->frag64.p, h->stream));
        HIP_TRY(gpad::launch_pack_panel64((const double*)dB, m, n, sb, T, (char*)h->frag64.p + ob, h->stream));
        h->frag64_tiles = T;
        h->frag64_ok = true;
    }
    // fragment image for the MFMA panel kernel (shared f32 matrices only); the buffer is kept
    // across setups and only grows
    h->frag_ok = false;
    h->frag_tiles = 0;
    if (d->shared && d->dtype == GPAD_DTYPE_F32) {
        const size_t fb = gpad::panel_frag_bytes(n, m, d->batch);
        if (fb > 0) {
            if ((rc = h->frag.ensure(fb))) return rc;
            HIP_TRY(gpad::launch_pack_panel((const float*)dA, (const float*)dB, n, m, d->batch,
                                            (float)sa, sb, h->frag.p, h->stream));
            h->frag_tiles = gpad::panel_tiles(n, m, d->batch);
            h->frag_ok = true;
        }
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (d->memory == GPAD_MEM_HOST && !h->keep_stage) h->stage.release();
    h->ready = true;
    return GPAD_OK;
}

static void host_schedule(int N, int kind, double* theta, double* beta) {
    // acceldualgrad.m:18,27,55-56 (MATLAB: beta lagged one iteration) / paper eq. (8e)
    double th = 1.0, thm1 = 1.0, b = 0.0;
    for (int v = 0; v < N; ++v) {
        const double thn = (std::sqrt(std::pow(th, 4.0) + 4.0 * std::pow(th, 2.0)) - std::pow(th, 2.0)) / 2.0;
        theta[v] = th;
        if (kind == GPAD_SCHEDULE_PAPER) {
            beta[v] = th * (1.0 / thm1 - 1.0);
        } else {
            beta[v] = b;
            b = th * (1.0 / thm1 - 1.0);
        }
        thm1 = th;
        th = thn;
    }
}

int ensure_schedule(gpad_handle_t h, int N, const void* theta_in, const void* beta_in) {
    const int dt = h->dims.dtype;
    const size_t es = esize(dt);
    const bool custom = theta_in != nullptr || beta_in != nullptr;
    if (!custom && h->sched_len >= N + 2 && h->sched_kind == h->dims.schedule && h->sched_dtype == dt)
        return GPAD_OK;
    const int len = N + 2;  // kernels prefetch theta[v+1], beta[v+2]
    std::vector<double> th(len, 0.0), be(len, 0.0);
    host_schedule(N, h->dims.schedule, th.data(), be.data());
    if (custom) {
        if (!theta_in || !beta_in) return fail(GPAD_ERR_INVALID, "run_scaled: give both theta and beta");
        for (int v = 0; v < N; ++v) {
            th[v] = dt == GPAD_DTYPE_F64 ? ((const double*)theta_in)[v] : ((const float*)theta_in)[v];
            be[v] = dt == GPAD_DTYPE_F64 ? ((const double*)beta_in)[v] : ((const float*)beta_in)[v];
        }
    }
    th[N] = th[N + 1] = 0.0;  // pads: read by the prefetch, never used
    be[N] = be[N + 1] = 0.0;
    int rc;
    if ((rc = h->theta.ensure(es * len))) return rc;
    if ((rc = h->beta.ensure(es * len))) return rc;
    const std::vector<float> tf(th.begin(), th.end()), bf(be.begin(), be.end());  // (f32 handles)
    const bool f64 = dt == GPAD_DTYPE_F64;
    HIP_TRY(hipMemcpyAsync(h->theta.p, f64 ? (const void*)th.data() : tf.data(), es * len, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->beta.p, f64 ? (const void*)be.data() : bf.data(), es * len, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->sched_len = custom ? 0 : len;  // custom tables are never reused
    h->sched_kind = h->dims.schedule;
    h->sched_dtype = dt;
    return GPAD_OK;
}

// ---- gpad_lipschitz: L >= rho(G ML) by repeated squaring (include/gpad.h; kernel in gpad_lipschitz.hip) ----
namespace {

constexpr size_t kLipWorkCap = (size_t)1 << 30;  // bytes of handle workspace one chunk of instances may take
constexpr int kLipMaxChunk = 1024;               // ... and instances per launch (the grid's z extent)
constexpr int kLipMaxK = 4096;
constexpr int kLipMaxSquarings = 16;
// L is rounded up by this relative margin.  The chain's fp64 rounding is of order (K + k) 2^-53 relative -- a norm
// per squaring, each a sum of K^2 squares of sums of K products, and the k + 1 logarithms -- below 1e-12 for every
// K <= 4096; the exact chain is >= rho(S), the computed one came out 2e-15 under it in one case.
constexpr double kLipMargin = 1e-9;

// smallest k with K^(1 / 2^(k+1)) <= 1 + rtol
int lip_squarings(int K, double rtol) {
    const double lim = std::log1p(rtol), lk = std::log((double)K);
    int k = 0;
    while (k < kLipMaxSquarings && std::ldexp(lk, -(k + 1)) > lim) ++k;
    return k;
}

// the order of gpad_lipschitz.hip lip_slot_sum_dev: 256 strided partial sums, then the halving tree
double lip_slot_sum(const double* slots, int count) {
    double red[gpad::kLipThreads];
    for (int t = 0; t < gpad::kLipThreads; ++t) {
        double p = 0.0;
        for (int i = t; i < count; i += gpad::kLipThreads) p += slots[i];
        red[t] = p;
    }
    for (int s = gpad::kLipThreads / 2; s > 0; s >>= 1)
        for (int t = 0; t < s; ++t) red[t] += red[t + s];
    return red[0];
}

inline double lip_scale(double ssq) { return (ssq > 0.0 && std::isfinite(ssq)) ? 1.0 / std::sqrt(ssq) : 0.0; }

// ssq[j] = |B_{j-1}^2|_F^2 (j = 0: |S|_F^2)  ->  L = exp(c_k / 2^k) (1 + margin), c_0 = log |S|_F, c_{j+1} = 2 c_j + log |.|_F
int lip_finish(const char* fn, const double* ssq, int k, int inst, double* L) {
    double c = 0.0;
    for (int j = 0; j <= k; ++j) {
        const double nj = std::sqrt(ssq[j]);
        if (!std::isfinite(nj))
            return fail(GPAD_ERR_INVALID, std::string(fn) + ": instance " + std::to_string(inst) +
                                              ": a norm of the chain is not finite (NaN, infinity or overflow in ML, G)");
        if (nj == 0.0) {
            *L = 0.0;
            return GPAD_OK;
        }
        c = 2.0 * c + std::log(nj);
    }
    *L = std::exp(std::ldexp(c, -k)) * (1.0 + kLipMargin);
    return GPAD_OK;
}

int lip_validate(const char* fn, int n, int m, int batch, int dtype, const void* ML, const void* G, double* rtol,
                 const double* L) {
    if (n <= 0 || m <= 0 || batch <= 0 || !ML || !G || !L || (dtype != GPAD_DTYPE_F32 && dtype != GPAD_DTYPE_F64))
        return fail(GPAD_ERR_INVALID, std::string(fn) + ": bad arguments");
    if (!(*rtol >= 0.0) || *rtol > 1.0) return fail(GPAD_ERR_INVALID, std::string(fn) + ": rtol must be in [0, 1]");
    if (*rtol == 0.0) *rtol = 0.01;
    if (std::min(n, m) > kLipMaxK)
        return fail(GPAD_ERR_UNSUPPORTED, std::string(fn) + ": min(n, m) > " + std::to_string(kLipMaxK));
    return GPAD_OK;
}

// one pair on the host: plain fp64 loops, every sum ascending in k
int lip_host_one(int n, int m, int dtype, const void* ML, const void* G, size_t off, int k, int inst, double* L) {
    const bool f64 = dtype == GPAD_DTYPE_F64;
    const size_t nm = (size_t)n * m;
    std::vector<double> ml(nm), g(nm);
    for (size_t i = 0; i < nm; ++i) {
        ml[i] = f64 ? ((const double*)ML)[off + i] : (double)((const float*)ML)[off + i];
        g[i] = f64 ? ((const double*)G)[off + i] : (double)((const float*)G)[off + i];
    }
    const bool small_n = n <= m;  // S = ML G (n x n), else G ML (m x m)
    const double* A = small_n ? ml.data() : g.data();
    const double* B = small_n ? g.data() : ml.data();
    const size_t K = (size_t)std::min(n, m), P = (size_t)std::max(n, m);
    std::vector<double> cur(K * K, 0.0), nxt(K * K), ssq((size_t)k + 1, 0.0);
    auto gemm = [&](const double* a, const double* b, size_t p, double* c) {  // c = a b, a K x p, b p x K
        std::fill(c, c + K * K, 0.0);
        for (size_t i = 0; i < K; ++i)
            for (size_t kk = 0; kk < p; ++kk) {
                const double aik = a[i * p + kk];
                for (size_t j = 0; j < K; ++j) c[i * K + j] += aik * b[kk * K + j];
            }
        double s = 0.0;
        for (size_t i = 0; i < K * K; ++i) s += c[i] * c[i];
        return s;
    };
    ssq[0] = gemm(A, B, P, cur.data());
    for (int j = 1; j <= k; ++j) {
        const double s = lip_scale(ssq[j - 1]);
        for (double& v : cur) v *= s;
        ssq[j] = gemm(cur.data(), cur.data(), K, nxt.data());
        cur.swap(nxt);
    }
    return lip_finish("gpad_lipschitz_host", ssq.data(), k, inst, L);
}

}  // namespace

extern "C" {

int gpad_lipschitz(gpad_handle_t h, int n, int m, int batch, int shared, int dtype, int memory, const void* ML,
                   const void* G, double rtol, double* L) {
    return gpad::abi_guard("gpad_lipschitz", [&]() -> int {
        if (!h) return fail(GPAD_ERR_INVALID, "gpad_lipschitz: null handle");
        if (memory != GPAD_MEM_HOST && memory != GPAD_MEM_DEVICE)
            return fail(GPAD_ERR_INVALID, "gpad_lipschitz: bad memory kind");
        int rc = lip_validate("gpad_lipschitz", n, m, batch, dtype, ML, G, &rtol, L);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(h->device));
        const bool host = memory == GPAD_MEM_HOST, small_n = n <= m;
        const int nmat = shared ? 1 : batch, K = std::min(n, m);
        const int k = lip_squarings(K, rtol), nslots = gpad::lip_tiles(K) * gpad::lip_tiles(K);
        const size_t es = esize(dtype), nm = (size_t)n * m, kk = (size_t)K * K;
        // per instance: the two K x K buffers the squarings alternate between, a slot row per launch, and for host
        // operands their staged copies
        const size_t per = sizeof(double) * (2 * kk + (size_t)(k + 1) * nslots) + (host ? 2 * nm * es : 0);
        const int chunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)nmat, (size_t)kLipMaxChunk, kLipWorkCap / per}));
        if ((rc = h->lipwork.ensure(per * chunk))) return rc;
        double* buf[2] = {(double*)h->lipwork.p, (double*)h->lipwork.p + kk * chunk};
        double* slots = buf[1] + kk * chunk;  // [k + 1][chunk][nslots]
        char* stML = (char*)(slots + (size_t)(k + 1) * chunk * nslots);
        char* stG = stML + nm * es * chunk;
        const size_t slot_row = (size_t)chunk * nslots;
        std::vector<double> hs((size_t)(k + 1) * slot_row), ssq((size_t)k + 1), Lh((size_t)nmat);
        for (int b0 = 0; b0 < nmat; b0 += chunk) {
            const int cnt = std::min(chunk, nmat - b0);
            const char* dML = (const char*)ML + (size_t)b0 * nm * es;
            const char* dG = (const char*)G + (size_t)b0 * nm * es;
            if (host) {
                HIP_TRY(hipMemcpyAsync(stML, dML, nm * es * cnt, hipMemcpyHostToDevice, h->stream));
                HIP_TRY(hipMemcpyAsync(stG, dG, nm * es * cnt, hipMemcpyHostToDevice, h->stream));
                dML = stML;
                dG = stG;
            }
            gpad::LipGemmArgs a{};
            a.A = small_n ? dML : dG;
            a.B = small_n ? dG : dML;
            a.sA = a.sB = (long long)nm;
            a.lda = small_n ? m : n;
            a.ldb = small_n ? n : m;
            a.P = std::max(n, m);
            a.K = K;
            a.in_slots = nullptr;
            a.C = buf[0];
            a.out_slots = slots;
            a.nslots = a.slot_stride = nslots;
            HIP_TRY(gpad::launch_lip_gemm(a, dtype == GPAD_DTYPE_F32, cnt, h->stream));
            for (int j = 1; j <= k; ++j) {  // buf[(j-1) & 1] squared into buf[j & 1]
                a.A = a.B = buf[(j - 1) & 1];
                a.sA = a.sB = (long long)kk;
                a.lda = a.ldb = a.P = K;
                a.in_slots = slots + (size_t)(j - 1) * slot_row;
                a.C = buf[j & 1];
                a.out_slots = slots + (size_t)j * slot_row;
                HIP_TRY(gpad::launch_lip_gemm(a, false, cnt, h->stream));
            }
            HIP_TRY(hipMemcpyAsync(hs.data(), slots, sizeof(double) * hs.size(), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
            for (int i = 0; i < cnt; ++i) {
                for (int j = 0; j <= k; ++j) ssq[j] = lip_slot_sum(hs.data() + (size_t)j * slot_row + (size_t)i * nslots, nslots);
                if ((rc = lip_finish("gpad_lipschitz", ssq.data(), k, b0 + i, &Lh[b0 + i]))) return rc;
            }
        }
        if (host) {
            std::copy(Lh.begin(), Lh.end(), L);
        } else {
            HIP_TRY(hipMemcpyAsync(L, Lh.data(), sizeof(double) * nmat, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
        return GPAD_OK;
    });
}

int gpad_lipschitz_host(int n, int m, int batch, int shared, int dtype, const void* ML, const void* G, double rtol,
                        double* L) {
    return gpad::abi_guard("gpad_lipschitz_host", [&]() -> int {
        int rc = lip_validate("gpad_lipschitz_host", n, m, batch, dtype, ML, G, &rtol, L);
        if (rc) return rc;
        const int nmat = shared ? 1 : batch, k = lip_squarings(std::min(n, m), rtol);
        for (int b = 0; b < nmat; ++b)
            if ((rc = lip_host_one(n, m, dtype, ML, G, (size_t)b * n * m, k, b, &L[b]))) return rc;
        return GPAD_OK;
    });
}

int gpad_setup(gpad_handle_t h, const gpad_dims_t* d, const void* ML, const void* G, double L) {
    return gpad::abi_guard("gpad_setup", [&]() -> int {
        return setup_impl(h, d, ML, G, L, false);
    });
}

int gpad_setup_scaled(gpad_handle_t h, const gpad_dims_t* d, const void* MGneg, const void* GL,
                      double L) {
    return gpad::abi_guard("gpad_setup_scaled", [&]() -> int {
        return setup_impl(h, d, MGneg, GL, L, true);
    });
}

int gpad_setup_hessian(gpad_handle_t h, const void* H) {
    return gpad::abi_guard("gpad_setup_hessian", [&]() -> int {
        if (!h) return fail(GPAD_ERR_INVALID, "gpad_setup_hessian: null handle");
        if (h->cls) return no_classes("gpad_setup_hessian");
        if (!h->ready) return fail(GPAD_ERR_NOT_SETUP, "gpad_setup_hessian: call gpad_setup first");
        if (h->flat) return fail(GPAD_ERR_UNSUPPORTED, "gpad_setup_hessian: not on the flat battery path");
        if (H && h->zbound > 0.0)
            return fail(GPAD_ERR_UNSUPPORTED, "gpad_setup_hessian: an infeasibility bound is in force "
                                              "(gpad_setup_infeasibility); unbind it first");
        h->hess_ok = false;
        h->hfrag64_ok = false;
        if (!H) return GPAD_OK;
        HIP_TRY(hipSetDevice(h->device));
        const gpad_dims_t& d = h->dims;
        const int n = d.n, nmats = d.shared ? 1 : d.batch;
        const size_t es = esize(d.dtype), raw = (size_t)n * n * nmats * es;
        int rc;
        if ((rc = h->Hq.ensure(es * (size_t)n * h->ldn * nmats))) return rc;
        const void* dH = H;
        DevBuf stage;
        if (d.memory == GPAD_MEM_HOST) {
            if ((rc = stage.ensure(raw))) return rc;
            HIP_TRY(hipMemcpyAsync(stage.p, H, raw, hipMemcpyHostToDevice, h->stream));
            dH = stage.p;
        }
        const long long in_stride = d.shared ? 0 : (long long)n * n, out_stride = (long long)n * h->ldn;
        if (d.dtype == GPAD_DTYPE_F32)
            HIP_TRY(gpad::launch_pack_kmajor<float>((const float*)dH, (float*)h->Hq.p, n, n, h->ldn, 1.0, nmats, in_stride,
                                                    out_stride, h->stream));
        else
            HIP_TRY(gpad::launch_pack_kmajor<double>((const double*)dH, (double*)h->Hq.p, n, n, h->ldn, 1.0, nmats,
                                                     in_stride, out_stride, h->stream));
        if (h->frag64_ok) {  // shared f64: H for the f64 panels' value branches
            if ((rc = h->hfrag64.ensure(gpad::panel64_frag_bytes(n, d.m)))) return rc;
            HIP_TRY(gpad::launch_pack_panel64((const double*)dH, n, n, 1.0, h->frag64_tiles, h->hfrag64.p, h->stream));
            h->hfrag64_ok = true;
        }
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->hess_ok = true;
        return GPAD_OK;
    });
}

int gpad_setup_infeasibility(gpad_handle_t h, double zbound) {
    return gpad::abi_guard("gpad_setup_infeasibility", [&]() -> int {
        if (!h) return fail(GPAD_ERR_INVALID, "gpad_setup_infeasibility: null handle");
        if (!h->cls && !h->ready) return fail(GPAD_ERR_NOT_SETUP, "gpad_setup_infeasibility: call gpad_setup first");
        if (!(zbound >= 0.0) || !std::isfinite(zbound))
            return fail(GPAD_ERR_INVALID, "gpad_setup_infeasibility: zbound must be finite and >= 0");
        HIP_TRY(hipSetDevice(h->device));
        if (h->cls) {  // every class binds it, and the handles the binding makes later
            if (const int rc = gpad::classes_setup_infeasibility(h->cls, zbound)) return rc;
            h->zbound = zbound;
            return GPAD_OK;
        }
        if (zbound > 0.0 && h->flat)
            return fail(GPAD_ERR_UNSUPPORTED, "gpad_setup_infeasibility: not on the flat battery path");
        if (zbound > 0.0 && h->hess_ok)
            return fail(GPAD_ERR_UNSUPPORTED, "gpad_setup_infeasibility: a Hessian is bound (gpad_setup_hessian); "
                                              "unbind it first");
        h->zbound = 0.0;
        if (zbound == 0.0) return GPAD_OK;
        const gpad_dims_t& d = h->dims;
        const int nmats = d.shared ? 1 : d.batch;
        if (int rc = h->frows.ensure(sizeof(double) * (size_t)h->ldm * nmats)) return rc;
        HIP_TRY(gpad::launch_farkas_rows(h->GLt.p, d.dtype == GPAD_DTYPE_F64, d.n, d.m, h->ldm, nmats,
                                         (double*)h->frows.p, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->zbound = zbound;
        return GPAD_OK;
    });
}

// A handle setting, kept in Tuning beside the options: it survives every setup and unbinding, and a class binding
// hands it to its children as it hands them the options (gpad_classes.cpp apply_tuning, classes_set_option's way)
int gpad_infeasibility_resident(gpad_handle_t h, int on) {
    return gpad::abi_guard("gpad_infeasibility_resident", [&]() -> int {
        if (!h) return fail(GPAD_ERR_INVALID, "gpad_infeasibility_resident: null handle");
        if (on != 0 && on != 1) return fail(GPAD_ERR_INVALID, "gpad_infeasibility_resident: on must be 0 or 1");
        h->tune.fk_resident = on;
        if (!h->cls) return GPAD_OK;
        HIP_TRY(hipSetDevice(h->device));
        return gpad::classes_infeasibility_resident(h->cls, on);
    });
}

// gpad_infeasibility_resident's twin for GPAD_OPT_LOOP_ASYNC (gpad_state.cpp one_launch_engine)
int gpad_infeasibility_loop_async(gpad_handle_t h, int on) {
    return gpad::abi_guard("gpad_infeasibility_loop_async", [&]() -> int {
        if (!h) return fail(GPAD_ERR_INVALID, "gpad_infeasibility_loop_async: null handle");
        if (on != 0 && on != 1) return fail(GPAD_ERR_INVALID, "gpad_infeasibility_loop_async: on must be 0 or 1");
        h->tune.fk_loop_async = on;
        if (!h->cls) return GPAD_OK;
        HIP_TRY(hipSetDevice(h->device));
        return gpad::classes_infeasibility_loop_async(h->cls, on);
    });
}

// -(g'y) - R |G'y|_1 in fp64 on host arrays (no device): > 0 exactly when y >= 0 proves that no z with
// |z|_inf <= R satisfies G z <= g; -inf when y has a negative entry (or a NaN)
int gpad_farkas_margin(int n, int m, int dtype, const void* G, const void* g, const void* y, double zbound,
                       double* margin) {
    return gpad::abi_guard("gpad_farkas_margin", [&]() -> int {
        if (n <= 0 || m <= 0 || !G || !g || !y || !margin || (dtype != GPAD_DTYPE_F32 && dtype != GPAD_DTYPE_F64) ||
            !(zbound >= 0.0) || !std::isfinite(zbound))
            return fail(GPAD_ERR_INVALID, "gpad_farkas_margin: bad arguments");
        const bool f64 = dtype == GPAD_DTYPE_F64;
        auto at = [&](const void* p, size_t i) { return f64 ? ((const double*)p)[i] : (double)((const float*)p)[i]; };
        std::vector<double> t((size_t)n, 0.0);
        double gy = 0.0;
        for (int i = 0; i < m; ++i) {
            const double yi = at(y, i);
            if (!(yi >= 0.0)) {
                *margin = -INFINITY;
                return GPAD_OK;
            }
            gy += at(g, i) * yi;
            for (int j = 0; j < n; ++j) t[j] += yi * at(G, (size_t)i * n + j);
        }
        double a = 0.0;
        for (int j = 0; j < n; ++j) a += std::fabs(t[j]);
        *margin = -gy - zbound * a;
        return GPAD_OK;
    });
}

int gpad_setup_flat(gpad_handle_t h, const gpad_dims_t* d, int n_u, const float* MGf, const float* GLf,
                    double L) {
    return gpad::abi_guard("gpad_setup_flat", [&]() -> int {
        if (!h) return fail(GPAD_ERR_INVALID, "gpad_setup_flat: null handle");
        int rc = validate_dims(d);
        if (rc) return rc;
        if (!MGf || !GLf) return fail(GPAD_ERR_INVALID, "gpad_setup_flat: null matrix");
        if (!(L > 0.0) || !std::isfinite(L)) return fail(GPAD_ERR_INVALID, "gpad_setup_flat: L must be > 0");
        if (d->dtype != GPAD_DTYPE_F32 || !d->shared)
            return fail(GPAD_ERR_UNSUPPORTED, "gpad_setup_flat: f32 and shared matrices only");
        if (n_u <= 0 || d->n % n_u != 0 || d->m < 4 * d->n)
            return fail(GPAD_ERR_INVALID, "gpad_setup_flat: need n = n_u*N and m >= 4 n_u N");
        HIP_TRY(hipSetDevice(h->device));
        unbind_problem(h);
        h->dims = *d;
        if (h->dims.check_every <= 0) h->dims.check_every = 10;
        h->L = L;
        h->scaled = true;
        const int Nh = d->n / n_u, m = d->m;
        const size_t bytes = sizeof(float) * (size_t)Nh * m;
        h->ldn = round4(d->n);
        h->ldm = round4(m);
        if ((rc = h->MGt.ensure(bytes)) || (rc = h->GLt.ensure(bytes))) return rc;
        const void* dG = GLf;
        if (d->memory == GPAD_MEM_HOST) {
            if ((rc = h->stage.ensure(bytes))) return rc;
            HIP_TRY(hipMemcpyAsync(h->MGt.p, MGf, bytes, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(h->stage.p, GLf, bytes, hipMemcpyHostToDevice, h->stream));
            dG = h->stage.p;
        } else {
            HIP_TRY(hipMemcpyAsync(h->MGt.p, MGf, bytes, hipMemcpyDeviceToDevice, h->stream));
        }
        HIP_TRY(gpad::launch_transpose_flat((const float*)dG, (float*)h->GLt.p, m, Nh, h->stream));
        h->GLx.release();
        if (gpad::flat_resident_supported(d->n, m, n_u)) {
            if ((rc = h->GLx.ensure(sizeof(float) * (size_t)d->n * h->ldm))) return rc;
            HIP_TRY(gpad::launch_expand_flat_gl((const float*)dG, (float*)h->GLx.p, Nh, n_u, m, h->ldm,
                                                h->stream));
        }
        h->frag_ok = false;
        h->frag_tiles = 0;
        {  // MFMA panels over the flat data (gpad_flatpanel.hip)
            const size_t fb = gpad::flatpanel_frag_bytes(d->n, m, n_u);
            if (fb) {
                if ((rc = h->frag.ensure(fb))) return rc;
                HIP_TRY(gpad::launch_pack_flatpanel((const float*)h->MGt.p, (const float*)h->GLt.p, d->n, m, n_u,
                                                    h->frag.p, h->stream));
                h->frag_ok = true;
            }
        }
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (d->memory == GPAD_MEM_HOST && !h->keep_stage) h->stage.release();
        h->n_u = n_u;
        h->flat = true;
        h->ready = true;
        return GPAD_OK;
    });
}

int gpad_schedule(int N, int kind, double* theta, double* beta) {
    return gpad::abi_guard("gpad_schedule", [&]() -> int {
        if (N < 0 || !theta || !beta) return fail(GPAD_ERR_INVALID, "gpad_schedule: bad arguments");
        host_schedule(N, kind, theta, beta);
        return GPAD_OK;
    });
}

int gpad_precompute(gpad_handle_t h, int n, int m, int batch, int shared, int memory, const double* H,
                    const double* A, const double* f, double* ML, double* gP, double* L) {
    return gpad::abi_guard("gpad_precompute", [&]() -> int {
        if (!h) return fail(GPAD_ERR_INVALID, "gpad_precompute: null handle");
        if (n <= 0 || m < 0 || batch <= 0 || !H || !A || !ML || !L || (f == nullptr) != (gP == nullptr) ||
            (memory != GPAD_MEM_HOST && memory != GPAD_MEM_DEVICE))
            return fail(GPAD_ERR_INVALID, "gpad_precompute: bad arguments");
        HIP_TRY(hipSetDevice(h->device));
        const bool host = memory == GPAD_MEM_HOST;
        const int nmat = shared ? 1 : batch;  // eliminations
        const size_t nH = (size_t)nmat * n * n, nA = (size_t)nmat * m * n, nML = (size_t)nmat * n * m;
        const size_t nF = f ? (size_t)batch * n : 0;
        // shared: one elimination of [H | A' | I] gives ML and inv(H); gP = inv(H) f' per row after
        const int fchunk = shared ? (f ? n : 0) : (f ? 1 : 0);
        if (!gpad::precompute_supported(n, m, fchunk))
            return fail(GPAD_ERR_UNSUPPORTED, "gpad_precompute: 2n + m too large for the LDS pivot row");
        // device views of the operands (host memory: staged copies)
        DevBuf stage, work;
        const double *dH = H, *dA = A, *df = f;
        double *dML = ML, *dgP = gP, *dL = L;
        const size_t tot = nH + nA + nF + nML + nF + nmat;
        int rc;
        if (host) {
            if ((rc = stage.ensure(sizeof(double) * tot))) return rc;
            double* b = (double*)stage.p;
            double* sH = b;
            double* sA = sH + nH;
            double* sf = sA + nA;
            dML = sf + nF;
            dgP = f ? dML + nML : nullptr;
            dL = dML + nML + nF;
            HIP_TRY(hipMemcpyAsync(sH, H, sizeof(double) * nH, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(sA, A, sizeof(double) * nA, hipMemcpyHostToDevice, h->stream));
            if (f) HIP_TRY(hipMemcpyAsync(sf, f, sizeof(double) * nF, hipMemcpyHostToDevice, h->stream));
            dH = sH;
            dA = sA;
            df = f ? sf : nullptr;
        }
        if (shared) {
            const size_t wb = gpad::precompute_work_bytes(n, m, fchunk, 1);
            if ((rc = work.ensure(wb + (f ? sizeof(double) * (size_t)n * n : 0)))) return rc;
            double* Hinv = f ? (double*)((char*)work.p + wb) : nullptr;
            HIP_TRY(gpad::launch_precompute(n, m, fchunk, dH, 0, dA, 0, nullptr, 0, (double*)work.p, dML, Hinv, dL, 0, 1,
                                            h->stream));
            if (f) HIP_TRY(gpad::launch_apply_inv(n, batch, Hinv, df, dgP, h->stream));
        } else {
            const size_t per = gpad::precompute_work_bytes(n, m, fchunk, 1);
            int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)batch, ((size_t)1 << 30) / per));
            chunk = std::min(chunk, 4 * h->num_cus);
            if ((rc = work.ensure(per * chunk))) return rc;
            for (int b0 = 0; b0 < batch; b0 += chunk) {
                const int cnt = std::min(chunk, batch - b0);
                HIP_TRY(gpad::launch_precompute(n, m, fchunk, dH, (long long)n * n, dA, (long long)m * n, df, n,
                                                (double*)work.p, dML, dgP, dL, b0, cnt, h->stream));
            }
        }
        if (host) {
            HIP_TRY(hipMemcpyAsync(ML, dML, sizeof(double) * nML, hipMemcpyDeviceToHost, h->stream));
            if (f) HIP_TRY(hipMemcpyAsync(gP, dgP, sizeof(double) * nF, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(L, dL, sizeof(double) * nmat, hipMemcpyDeviceToHost, h->stream));
        }
        HIP_TRY(hipStreamSynchronize(h->stream));
        return GPAD_OK;
    });
}

}  // extern "C"
