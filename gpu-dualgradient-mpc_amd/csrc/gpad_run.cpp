// gpad_run.cpp -- one solve: the phase-plan cache, the engine selection (launch_solve), host staging
// (gpad_run / gpad_run_scaled) and the one-shot gpad_solve with its per-thread handle.  Replaces the
// solve half of the reference's host driver (main.cu:79-203: 100 x (6 launches + 3 syncs), D2H).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>

#include "gpad_farkas.h"
#include "gpad_host.h"

// Shape-keyed plan prior.  A handle plans a phased solve from its OWN previous
// solve's counts, so its first solve ran the default schedule -- ~15 % slower on fresh C4 inputs
// (3.86 vs 3.3-3.4 ms, a second handle's first solve in a warm process), which every new
// gpad_solve caller thread paid once.  The last plan any handle of the process made is kept per
// (n, m, batch, check_every, N, CUs, finisher threshold option), and a handle with no plan of its
// own follows it.  A plan only moves launch boundaries and the finisher takeover (results are
// bit-identical under any plan), so a stale prior costs time, never correctness.
using PlanShape = std::tuple<int, int, int, int, int, int, int>;
static std::mutex g_prior_mu;
static std::map<PlanShape, gpad::PanelPlan>& prior_plans() {
    static std::map<PlanShape, gpad::PanelPlan> m;
    return m;
}
static PlanShape plan_shape(gpad_handle_t h, int batch, int N) {
    return PlanShape{h->dims.n, h->dims.m, batch, h->dims.check_every, N, h->num_cus, h->tune.finish_thresh};
}
static void plan_prior_store(gpad_handle_t h, int batch, int N) {
    if (h->plan.nph <= 0) return;
    std::lock_guard<std::mutex> lk(g_prior_mu);
    auto& m = prior_plans();
    if (m.size() >= 64 && !m.count(plan_shape(h, batch, N))) m.clear();  // (bounded: a handful of shapes)
    m[plan_shape(h, batch, N)] = h->plan;
}
// the plan a phased solve of this handle follows: its own, else the shape's prior (or none)
static const gpad::PanelPlan* plan_for(gpad_handle_t h, int batch, int N) {
    h->last_prior = false;
    if (!h->tune.plan) return nullptr;
    if (h->plan.nph > 0 && h->plan.N == N) return &h->plan;
    std::lock_guard<std::mutex> lk(g_prior_mu);
    auto it = prior_plans().find(plan_shape(h, batch, N));
    if (it == prior_plans().end()) return nullptr;
    h->prior = it->second;
    h->last_prior = true;
    return &h->prior;
}

// The phase plan is a pure function of the per-instance counts (and the shape): rebuild it only
// when they changed (repeated solves of one batch skip the DP).
void update_plan(gpad_handle_t h, const int* counts, int batch, int N) {
    if (h->flat) {  // the flat panels' phases run to the previous solve's last iteration
        int mx = 0;
        for (int b = 0; b < batch; ++b) mx = std::max(mx, counts[b]);
        h->flat_vpred = mx;
        return;
    }
    unsigned long long key = 1469598103934665603ull ^ (unsigned long long)N;
    for (int b = 0; b < batch; ++b) key = (key ^ (unsigned)counts[b]) * 1099511628211ull;
    if (key != h->plan_key || h->plan.nph == 0) {
        gpad::panel_plan(counts, batch, h->dims.n, h->dims.m, N, h->dims.check_every, h->num_cus, &h->tune,
                         &h->plan);
        h->plan_key = key;
        plan_prior_store(h, batch, N);
    }
}

// f64 panels: the next solve starts its instances longest-predicted-first, so
// the column refills pair long instances with short ones (greedy list scheduling over the columns)
// instead of in batch order -- each column's two-or-more instances then end together.  Predicted =
// the previous solve's counts on the same batch size (an MPC stream's statistics, or the same batch
// re-solved); ties keep batch order (stable).  Only the schedule changes: every instance runs the same
// arithmetic in any column (bit-identical results, tests/test_panel64.py).
void build_p64_order(gpad_handle_t h, const int* counts, int batch) {
    h->p64_order_host.resize(batch);
    for (int b = 0; b < batch; ++b) h->p64_order_host[b] = b;
    std::stable_sort(h->p64_order_host.begin(), h->p64_order_host.end(),
                     [&](int x, int y) { return counts[x] > counts[y]; });
    h->p64_order_batch = batch;
    h->p64_order_dirty = true;
}

template <typename T>
void fill_solve_args(gpad_handle_t h, int N, double tol, gpad::SolveArgs<T>* a) {
    const gpad_dims_t& d = h->dims;
    a->MGt = (const T*)h->MGt.p;
    a->GLt = (const T*)h->GLt.p;
    a->strideA = d.shared ? 0 : (long long)d.m * h->ldn;
    a->strideB = d.shared ? 0 : (long long)d.n * h->ldm;
    a->n = d.n;
    a->m = d.m;
    a->ldn = h->ldn;
    a->ldm = h->ldm;
    a->batch = d.batch;
    a->N = N;
    a->check_every = d.check_every;
    a->tol = tol;
    a->tol_gap = d.tol_gap > 0.0 ? d.tol_gap : tol;
    a->L = h->L;
    a->theta = (const T*)h->theta.p;
    a->beta = (const T*)h->beta.p;
    a->num_cus = h->num_cus;
    a->tune = &h->tune;
    a->err = (int*)h->status.p;
}
template void fill_solve_args<float>(gpad_handle_t, int, double, gpad::SolveArgs<float>*);
template void fill_solve_args<double>(gpad_handle_t, int, double, gpad::SolveArgs<double>*);

int restart_counts(gpad_handle_t h, int nsolve, int** out) {
    if (out) *out = nullptr;
    h->last_restart = h->tune.restart > 0;
    if (!h->last_restart) return GPAD_OK;
    if (int rc = h->restarts.ensure(sizeof(int) * (size_t)h->dims.batch * nsolve)) return rc;
    if (out) *out = (int*)h->restarts.p;
    return GPAD_OK;
}

// GPAD_OPT_RESTART on: what the restart kernels do not carry (the follow-ups of include/gpad.h), refused by
// name rather than run without the restart
static int restart_refusal(gpad_handle_t h, double tol) {
    const char* what = h->flat                                   ? "flat setups (gpad_setup_flat)"
                       : h->hess_ok                              ? "a bound Hessian (gpad_setup_hessian)"
                       : h->zbound > 0.0 && tol > 0.0            ? "an infeasibility bound in force with tol > 0"
                       : h->dims.kernel == GPAD_KERNEL_RESIDENT ? "a forced resident kernel"
                       : h->dims.kernel == GPAD_KERNEL_PANEL && h->dims.dtype == GPAD_DTYPE_F64
                           ? "the f64 panels (f64 runs the stream kernel)"
                           : nullptr;
    if (!what) return GPAD_OK;
    return fail(GPAD_ERR_UNSUPPORTED, std::string("adaptive restart (GPAD_OPT_RESTART) runs on the stream kernel and the "
                                                  "f32 T-wave panels: not with ") + what);
}

template <typename T>
int launch_solve(gpad_handle_t h, T* dz, T* dy, const T* dM, const T* dg, int N, double tol,
                 bool scaled_vec, int* iters, int* conv, int* kernel_out, int* restarts) {
    const gpad_dims_t& d = h->dims;
    const int n = d.n, m = d.m, batch = d.batch;
    gpad::SolveArgs<T> a{};
    fill_solve_args<T>(h, N, tol, &a);
    a.frag = h->frag_ok ? h->frag.p : nullptr;
    a.frag_tiles = h->frag_tiles;
    a.gP = dM;
    a.g = dg;
    a.ld_gP = n;
    a.ld_g = m;
    a.gscale = scaled_vec ? 1.0 : -1.0 / h->L;
    a.z = dz;
    a.y = dy;
    a.iters = iters;
    a.conv = conv;
    a.Hq = (h->hess_ok && tol > 0.0) ? (const T*)h->Hq.p : nullptr;
    a.strideHq = d.shared ? 0 : (long long)n * h->ldn;
    a.debug = h->tune.debug_drop_handoff ? gpad::kDebugDropHandoff : 0;
    // the certification floor's data term max |g| (stats: tol_floor, GPAD_FLAG_TOL_FLOOR): folded
    // into the panel pairs' own loads, else one launch_absmax after the solve's launches
    double* gpart = tol > 0.0 ? reinterpret_cast<double*>((char*)h->status.p + offsetof(RunStatus, part)) : nullptr;
    bool gmax_done = false;
    if constexpr (sizeof(T) == sizeof(float)) a.gmax_part = gpart;
    auto finish = [&](int rc) {
        if (rc == GPAD_OK && gpart && !gmax_done) {
            const hipError_t ea = gpad::launch_absmax<T>(dg, (long long)batch * m, gpart, h->stream);
            if (ea != hipSuccess) return fail(GPAD_ERR_HIP, std::string("absmax: ") + hipGetErrorString(ea));
        }
        return rc;
    };
    int kernel = d.kernel;
    const bool prev_phased = h->last_phased;  // the previous launch's counts are still in `iters`
    h->last_phased = false;  // set again below when this launch is a phased panel solve
    h->last_p64 = false;
    h->last_N = N;
    hipError_t e = hipSuccess;
    bool ok = false;
    if (h->tune.restart > 0) {
        if (int rc = restart_refusal(h, tol)) {
            h->last_restart = false;  // (nothing ran: gpad_last_restarts reports zeros)
            return rc;
        }
        if (!restarts) return fail(GPAD_ERR_INVALID, "launch_solve: no restart counters");
    }
    if (N == 0) {  // nothing to iterate: outputs are the inputs, zero counts
        HIP_TRY(hipMemsetAsync(a.iters, 0, sizeof(int) * (size_t)batch, h->stream));
        HIP_TRY(hipMemsetAsync(a.conv, 0, sizeof(int) * (size_t)batch, h->stream));
        if (h->tune.restart > 0) HIP_TRY(hipMemsetAsync(restarts, 0, sizeof(int) * (size_t)batch, h->stream));
        *kernel_out = d.kernel == GPAD_KERNEL_AUTO ? GPAD_KERNEL_STREAM : d.kernel;
        return finish(GPAD_OK);
    }
    // Adaptive restart (GPAD_OPT_RESTART): the position in the schedule is per instance.  A forced PANEL, and AUTO
    // where unbound AUTO runs panels, run the T-wave panels' restart variant where it applies (shared f32 matrices,
    // n, m <= 256: T <= 16) -- no pair layout, no finisher, as with a certificate bound; AUTO otherwise and a
    // forced STREAM the stream kernel's, f32 and f64, every shape.  The engines that share one position per
    // launch (pairs, finisher, resident, the f64 and big panels) are not entered
    if (h->tune.restart > 0) {
        gpad::RestartArgs rs{h->tune.restart, restarts, nullptr};
        if constexpr (sizeof(T) == sizeof(float)) {
            const int panel_min = gpad::resident_supported(n, m) ? 4 * h->num_cus : 64;
            const bool want = kernel == GPAD_KERNEL_PANEL || (kernel == GPAD_KERNEL_AUTO && batch > panel_min);
            bool pok = false;
            if (want && d.shared && h->frag_ok) {
                int rc = h->pwork.ensure(gpad::panel_work_bytes(m, batch));
                if (!rc) rc = h->rs_pos.ensure(sizeof(int) * (size_t)batch);
                if (rc) return rc;
                rs.pos = (int*)h->rs_pos.p;
                a.pwork = h->pwork.p;
                a.used = &h->last_phases;  // (no plan: the planner models the pairs and the finisher)
                e = gpad::launch_panel(a, h->stream, &pok, nullptr, &rs);
                if (e != hipSuccess) return fail(GPAD_ERR_HIP, std::string("panel: ") + hipGetErrorString(e));
                if (!pok) a.pwork = nullptr, a.used = nullptr;
            }
            if (!pok && kernel == GPAD_KERNEL_PANEL)
                return fail(GPAD_ERR_UNSUPPORTED, "adaptive restart (GPAD_OPT_RESTART) on the panels needs shared f32 "
                                                  "matrices with n, m <= 256");
            if (pok) {
                *kernel_out = GPAD_KERNEL_PANEL;
                h->last_phased = tol > 0.0 && h->tune.phased;  // (else one launch: no phases to report)
                return finish(GPAD_OK);
            }
        }
        e = gpad::launch_stream<T>(a, h->stream, nullptr, &rs);
        if (e != hipSuccess)
            return fail(e == hipErrorInvalidValue ? GPAD_ERR_UNSUPPORTED : GPAD_ERR_HIP,
                        std::string("stream kernel: ") + hipGetErrorString(e) + " (n+m beyond the LDS budget?)");
        *kernel_out = GPAD_KERNEL_STREAM;
        return finish(GPAD_OK);
    }
    // The infeasibility certificate (gpad_setup_infeasibility) is carried by the stream kernel and by the f32
    // T-wave panels (shared matrices, n, m <= 256).  With a bound in force (tol > 0) AUTO and PANEL run those
    // panels where they apply -- no pair layout, no finisher -- AUTO else the stream kernel, and a forced engine
    // without the branch is refused rather than run without it.  On a handle with gpad_infeasibility_resident on,
    // the resident kernel carries it too (f32, n, m <= 208): forced, and by AUTO exactly where unbound AUTO runs
    // the resident kernel -- distinct matrices at any batch, shared ones up to 4 instances per CU
    const bool fk_on = h->zbound > 0.0 && tol > 0.0;
    const gpad::FarkasArgs fk{(const double*)h->frows.p, d.shared ? 0 : (long long)h->ldm, h->zbound};
    if (fk_on) {
        if constexpr (sizeof(T) == sizeof(float)) {
            if (h->tune.fk_resident && (kernel == GPAD_KERNEL_RESIDENT ||
                                        (kernel == GPAD_KERNEL_AUTO && gpad::resident_supported(n, m) &&
                                         !(d.shared && batch > 4 * h->num_cus)))) {
                bool rok = false;
                e = gpad::launch_resident(a, h->stream, &rok, &fk);
                if (e != hipSuccess) return fail(GPAD_ERR_HIP, std::string("resident: ") + hipGetErrorString(e));
                if (!rok) return fail(GPAD_ERR_UNSUPPORTED, "resident kernel: needs n, m <= 208");
                *kernel_out = GPAD_KERNEL_RESIDENT;
                return finish(GPAD_OK);
            }
        }
        if (kernel == GPAD_KERNEL_RESIDENT)
            return fail(GPAD_ERR_UNSUPPORTED, "the infeasibility certificate (gpad_setup_infeasibility) runs on the "
                                              "stream kernel and the f32 T-wave panels, not on the resident kernel "
                                              "(f32 handles: gpad_infeasibility_resident)");
        bool pok = false;
        if constexpr (sizeof(T) == sizeof(float)) {
            if (kernel != GPAD_KERNEL_STREAM && d.shared && h->frag_ok) {
                int rc = h->pwork.ensure(gpad::panel_work_bytes(m, batch));
                if (rc) return rc;
                a.pwork = h->pwork.p;
                a.used = &h->last_phases;  // (no plan: the planner models the pairs and the finisher)
                e = gpad::launch_panel(a, h->stream, &pok, &fk);
                if (e != hipSuccess) return fail(GPAD_ERR_HIP, std::string("panel: ") + hipGetErrorString(e));
                if (!pok) a.pwork = nullptr, a.used = nullptr;
            }
        }
        if (!pok && kernel == GPAD_KERNEL_PANEL)
            return fail(GPAD_ERR_UNSUPPORTED, "the infeasibility certificate on the panels needs shared f32 matrices "
                                              "with n, m <= 256");
        if (!pok) {
            e = gpad::launch_stream<T>(a, h->stream, &fk);
            if (e != hipSuccess)
                return fail(e == hipErrorInvalidValue ? GPAD_ERR_UNSUPPORTED : GPAD_ERR_HIP,
                            std::string("stream kernel: ") + hipGetErrorString(e) + " (n+m beyond the LDS budget?)");
        }
        *kernel_out = pok ? GPAD_KERNEL_PANEL : GPAD_KERNEL_STREAM;
        h->last_phased = pok;
        return finish(GPAD_OK);
    }
    if constexpr (sizeof(T) == sizeof(double)) {
        // f64 panels on the f64 MFMA pipe (shared matrices, n, m <= 256; value branches included):
        // forced, or from one panel per CU on (below that the one-instance-per-workgroup stream
        // kernel has the shorter iteration)
        if (h->frag64_ok && (kernel == GPAD_KERNEL_PANEL || (kernel == GPAD_KERNEL_AUTO && batch >= 16 * h->num_cus))) {
            a.frag = h->frag64.p;
            a.frag_tiles = h->frag64_tiles;
            if (int rq = h->q64.ensure(sizeof(int))) return rq;
            a.qctr = static_cast<int*>(h->q64.p);
            a.hfrag64 = (a.Hq && h->hfrag64_ok) ? h->hfrag64.p : nullptr;
            a.Hq = nullptr;
            if (tol > 0.0 && h->tune.lpt && h->p64_order_batch == batch && (int)h->p64_order_host.size() == batch) {
                if (h->p64_order_dirty) {
                    if (int ro = h->p64_order.ensure(sizeof(int) * (size_t)batch)) return ro;
                    HIP_TRY(hipMemcpyAsync(h->p64_order.p, h->p64_order_host.data(), sizeof(int) * (size_t)batch,
                                           hipMemcpyHostToDevice, h->stream));
                    h->p64_order_dirty = false;
                }
                a.order = static_cast<const int*>(h->p64_order.p);
            }
            e = gpad::launch_panel64(a, h->stream);
            if (e != hipSuccess) return fail(GPAD_ERR_HIP, hip_detail("f64 panel", e));
            h->last_p64 = tol > 0.0;
            *kernel_out = GPAD_KERNEL_PANEL;
            return finish(GPAD_OK);
        }
    }
    if (a.Hq) {  // value-function branches: the stream kernel family (and the f64 panels, above)
        if (kernel != GPAD_KERNEL_AUTO && kernel != GPAD_KERNEL_STREAM)
            return fail(GPAD_ERR_UNSUPPORTED, "the value-function test (gpad_setup_hessian) runs on the stream kernel "
                                              "(f32) or the stream / f64 panel kernels (f64)");
        kernel = GPAD_KERNEL_STREAM;
    }
    if constexpr (sizeof(T) == sizeof(float)) {
        if (kernel == GPAD_KERNEL_STREAM && !h->flat) {
            // forced stream kernel (or the value-function test): none of the f32 families below
        } else if (h->flat) {  // (flat data with STREAM forced: the LDS flat kernel)  // structure-exploiting battery path (gpad_setup_flat)
            a.n_u = h->n_u;
            // flat panels from 8 instances per CU when the register-resident flat chains exist
            // (their per-CU cost grows with the batch, a panel's does not until every CU holds
            // one: crossover ~2048 at C1, tools/fp_cross.py); always when only the LDS flat
            // kernel would be left (several times slower at any batch)
            const int fpm = h->tune.flat_panel_min >= 0 ? h->tune.flat_panel_min : (h->GLx.p ? 8 * h->num_cus : 0);
            if (h->frag_ok && (kernel == GPAD_KERNEL_PANEL || (kernel == GPAD_KERNEL_AUTO && batch >= fpm))) {
                if (tol > 0.0) {  // phased compaction workspace (gpad_flatpanel.hip)
                    int rc = h->pwork.ensure(gpad::panel_work_bytes(m, batch));
                    if (rc) return rc;
                    a.pwork = h->pwork.p;
                    a.v_pred = h->flat_vpred;  // the previous solve's last iteration (0: unknown)
                }
                e = gpad::launch_flatpanel(a, h->stream);
                h->last_phased = a.pwork != nullptr;
            } else if (h->GLx.p && kernel != GPAD_KERNEL_STREAM) {  // register-resident flat chains
                a.GLt = (const T*)h->GLx.p;
                a.strideA = a.strideB = 0;
                e = gpad::launch_flat_resident(a, h->stream);
            } else {
                e = gpad::launch_flat(a, h->stream);
            }
            if (e != hipSuccess)
                return fail(e == hipErrorInvalidValue ? GPAD_ERR_UNSUPPORTED : GPAD_ERR_HIP,
                            std::string("flat kernel: ") + hipGetErrorString(e));
            *kernel_out = GPAD_KERNEL_FLAT;
            return finish(GPAD_OK);
        }
        // shared matrices: panels once there are more instances than the latency kernel can
        // run at ~one round (4 per CU: 4 x its 1/6-panel iteration time < one panel iteration)
        const int panel_min = gpad::resident_supported(n, m) ? 4 * h->num_cus : 64;
        if (kernel == GPAD_KERNEL_PANEL || (kernel == GPAD_KERNEL_AUTO && d.shared && batch > panel_min)) {
            if (tol > 0.0 && h->frag_ok) {  // phased compaction workspace (gpad_phases.cpp)
                int rc = h->pwork.ensure(gpad::panel_work_bytes(m, batch));
                if (rc) return rc;
                a.pwork = h->pwork.p;
                a.plan = plan_for(h, batch, N);
                a.used = &h->last_phases;
                // the previous phased solve's counts are still in `iters` for every instance this
                // solve has not finished yet: the finisher orders its queue by them
                if (prev_phased && h->last_batch == batch && h->last_steps == 1) a.pred = iters;
            }
            e = gpad::launch_panel(a, h->stream, &ok);
            if (e != hipSuccess) return fail(GPAD_ERR_HIP, std::string("panel: ") + hipGetErrorString(e));
            if (ok) kernel = GPAD_KERNEL_PANEL;
            else if (kernel == GPAD_KERNEL_PANEL)
                return fail(GPAD_ERR_UNSUPPORTED, "panel kernel: needs shared f32 matrices");
            gmax_done = ok && gpad::panel_folds_gmax(n, m);
        }
        if (!ok && (kernel == GPAD_KERNEL_RESIDENT || kernel == GPAD_KERNEL_AUTO)) {
            e = gpad::launch_resident(a, h->stream, &ok);
            if (e != hipSuccess) return fail(GPAD_ERR_HIP, std::string("resident: ") + hipGetErrorString(e));
            if (ok) kernel = GPAD_KERNEL_RESIDENT;
            else if (kernel == GPAD_KERNEL_RESIDENT)
                return fail(GPAD_ERR_UNSUPPORTED, "resident kernel: needs n, m <= 208");
        }
    } else {
        if (kernel == GPAD_KERNEL_PANEL || kernel == GPAD_KERNEL_RESIDENT)
            return fail(GPAD_ERR_UNSUPPORTED, "f64: the resident kernel is f32 only; the f64 panels need shared "
                                              "matrices with n, m <= 256");
    }
    if (!ok) {
        kernel = GPAD_KERNEL_STREAM;
        e = gpad::launch_stream<T>(a, h->stream);
        if (e != hipSuccess)
            return fail(e == hipErrorInvalidValue ? GPAD_ERR_UNSUPPORTED : GPAD_ERR_HIP,
                        std::string("stream kernel: ") + hipGetErrorString(e) +
                            " (n+m beyond the LDS budget?)");
    }
    *kernel_out = kernel;
    h->last_phased = kernel == GPAD_KERNEL_PANEL && a.pwork != nullptr;
    return finish(GPAD_OK);
}
template int launch_solve<float>(gpad_handle_t, float*, float*, const float*, const float*, int, double, bool, int*,
                                 int*, int*, int*);
template int launch_solve<double>(gpad_handle_t, double*, double*, const double*, const double*, int, double, bool,
                                  int*, int*, int*, int*);

template <typename T>
static int run_typed(gpad_handle_t h, T* z, T* y, const T* M, const T* g, int N, double tol,
                     const void* theta_in, const void* beta_in, bool scaled_vec, gpad_stats_t* st) {
    const gpad_dims_t& d = h->dims;
    const int n = d.n, m = d.m, batch = d.batch;
    int rc = ensure_schedule(h, N, theta_in, beta_in);
    if (rc) return rc;
    // [iters | conv]
    if ((rc = h->counters.ensure(sizeof(int) * 2 * (size_t)batch))) return rc;
    int* restarts = nullptr;
    if ((rc = restart_counts(h, 1, &restarts))) return rc;
    T *dz = z, *dy = y;
    const T *dM = M, *dg = g;
    const size_t zb = sizeof(T) * (size_t)batch * n, yb = sizeof(T) * (size_t)batch * m;
    if (d.memory == GPAD_MEM_HOST) {
        if ((rc = h->work.ensure(2 * zb + 2 * yb))) return rc;
        char* base = (char*)h->work.p;
        dz = (T*)base;
        dy = (T*)(base + zb);
        T* wM = (T*)(base + zb + yb);
        T* wg = (T*)(base + 2 * zb + yb);
        HIP_TRY(hipMemcpyAsync(dz, z, zb, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(dy, y, yb, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(wM, M, zb, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(wg, g, yb, hipMemcpyHostToDevice, h->stream));
        dM = wM;
        dg = wg;
    }
    int* iters = (int*)h->counters.p;
    int kernel = 0;
    const double margin = sizeof(T) == sizeof(float) ? gpad::ViolMargin<float>::value : gpad::ViolMargin<double>::value;
    if ((rc = reset_status(h, tol, margin * h->L * (scaled_vec ? 1.0 : 1.0 / h->L)))) return rc;
    if (h->plan_pending && hipEventQuery(h->plan_ev) == hipSuccess) {  // a previous solve's counts landed
        if (h->plan_pending_batch == batch) {
            if (h->plan_pending_p64) build_p64_order(h, h->plan_pin, batch);
            else update_plan(h, h->plan_pin, batch, h->plan_pending_N);
        }
        h->plan_pending = false;
    }
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    if ((rc = launch_solve<T>(h, dz, dy, dM, dg, N, tol, scaled_vec, iters, iters + batch, &kernel, restarts)))
        return rc;
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    h->timed = true;
    h->last_kernel = kernel;
    h->last_batch = batch;
    h->last_steps = 1;
    const bool bound_run = (h->zbound > 0.0 && tol > 0.0) || h->last_restart;  // (plans nothing: collect_stats)
    if (!st && ((h->last_phased && h->tune.plan && !bound_run) || (h->last_p64 && h->tune.lpt))) {  // asynchronous run: counts
        // to the host behind it
        const size_t want = sizeof(int) * (size_t)batch;
        if (h->plan_pin_cap < want) {
            if (h->plan_pending) {  // the previous run's copy into the old buffer must land first
                HIP_TRY(hipEventSynchronize(h->plan_ev));
                h->plan_pending = false;
            }
            if (h->plan_pin) (void)hipHostFree(h->plan_pin);
            h->plan_pin = nullptr;
            h->plan_pin_cap = 0;
            HIP_TRY(hipHostMalloc((void**)&h->plan_pin, want, hipHostMallocDefault));
            h->plan_pin_cap = want;
        }
        if (!h->plan_ev) HIP_TRY(hipEventCreateWithFlags(&h->plan_ev, hipEventDisableTiming));
        HIP_TRY(hipMemcpyAsync(h->plan_pin, iters, want, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipEventRecord(h->plan_ev, h->stream));
        h->plan_pending = true;
        h->plan_pending_N = N;
        h->plan_pending_batch = batch;
        h->plan_pending_p64 = h->last_p64;
    }
    if (d.memory == GPAD_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(z, dz, zb, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(y, dy, yb, hipMemcpyDeviceToHost, h->stream));
    }
    if (st) return collect_stats(h, st);  // synchronises; a device error fails the run
    return d.memory == GPAD_MEM_HOST ? gpad_sync(h) : GPAD_OK;
}

static int run_impl(gpad_handle_t h, void* z0, void* y0, const void* M, const void* g, int N,
                    double tol, const void* theta, const void* beta, bool scaled_vec,
                    gpad_stats_t* st) {
    if (!h) return fail(GPAD_ERR_INVALID, "gpad_run: null handle");
    if (h->cls) {
        if (scaled_vec) return no_classes("gpad_run_scaled");
        HIP_TRY(hipSetDevice(h->device));
        return gpad::classes_run(h->cls, z0, y0, M, g, N, tol, st);
    }
    if (!h->ready) return fail(GPAD_ERR_NOT_SETUP, "gpad_run: call gpad_setup first");
    if (!z0 || !y0 || !M || !g) return fail(GPAD_ERR_INVALID, "gpad_run: null vector");
    if (N < 0) return fail(GPAD_ERR_INVALID, "gpad_run: N < 0");
    if (!(tol <= 0.0) && !std::isfinite(tol)) return fail(GPAD_ERR_INVALID, "gpad_run: bad tol");
    if ((theta || beta) && h->zbound > 0.0 && tol > 0.0)  // (the certificate's events follow the library's schedule)
        return fail(GPAD_ERR_UNSUPPORTED, "gpad_run_scaled: caller theta / beta tables with an infeasibility bound "
                                          "in force (gpad_setup_infeasibility)");
    if ((theta || beta) && h->tune.restart > 0)  // (a restart returns to position 0 of the library's schedule)
        return fail(GPAD_ERR_UNSUPPORTED, "gpad_run_scaled: caller theta / beta tables with adaptive restart on "
                                          "(GPAD_OPT_RESTART)");
    HIP_TRY(hipSetDevice(h->device));
    if (h->dims.dtype == GPAD_DTYPE_F64)
        return run_typed<double>(h, (double*)z0, (double*)y0, (const double*)M, (const double*)g, N,
                                 tol, theta, beta, scaled_vec, st);
    return run_typed<float>(h, (float*)z0, (float*)y0, (const float*)M, (const float*)g, N, tol, theta,
                            beta, scaled_vec, st);
}

// field by field: a stack-built dims may carry different padding bytes on every call
static bool same_dims(const gpad_dims_t& a, const gpad_dims_t& b) {
    return a.n == b.n && a.m == b.m && a.batch == b.batch && a.shared == b.shared && a.dtype == b.dtype &&
           a.memory == b.memory && a.schedule == b.schedule && a.check_every == b.check_every &&
           a.kernel == b.kernel && a.reserved == b.reserved && a.tol_gap == b.tol_gap;
}

// gpad_solve's per-thread handle: freed by gpad_release_cached(), not by a thread-exit destructor
// (at process exit that may run after the HIP runtime tore down; the OS reclaims it then).
namespace {
struct SolveCache {
    gpad_handle_t h = nullptr;
    int device = -1;
};
thread_local SolveCache t_solve_cache;
}  // namespace

extern "C" {

int gpad_run(gpad_handle_t h, void* z0, void* y0, const void* M, const void* g, int N, double tol,
             gpad_stats_t* st) {
    return gpad::abi_guard("gpad_run", [&]() -> int {
        return run_impl(h, z0, y0, M, g, N, tol, nullptr, nullptr, false, st);
    });
}

int gpad_run_scaled(gpad_handle_t h, void* z0, void* y0, const void* gP, const void* pD, int N,
                    double tol, const void* theta, const void* beta, gpad_stats_t* st) {
    return gpad::abi_guard("gpad_run_scaled", [&]() -> int {
        return run_impl(h, z0, y0, gP, pD, N, tol, theta, beta, true, st);
    });
}

void gpad_release_cached(void) {
    if (t_solve_cache.h) gpad_destroy(t_solve_cache.h);
    t_solve_cache.h = nullptr;
    t_solve_cache.device = -1;
    gpad::release_sharded_cache();
}

int gpad_solve(void* z0, void* y0, const void* ML, const void* M, const void* G, const void* g, int N,
               double L, double tol, const gpad_dims_t* dims, gpad_stats_t* st) {
    return gpad::abi_guard("gpad_solve", [&]() -> int {
        // One handle per thread and device, kept between calls: a per-MPC-step caller (gpad.m:90)
        // pays the handle, the workspaces and -- when the host matrices are unchanged -- the H2D
        // copy and repack of ML/G once, not per call.  gpad_release_cached() frees it.
        SolveCache& cache = t_solve_cache;
        int rc = validate_dims(dims);
        if (rc) return rc;
        if (!ML || !G) return fail(GPAD_ERR_INVALID, "gpad_solve: null matrix");
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        if (!cache.h || cache.device != dev) {
            if (cache.h) gpad_destroy(cache.h);
            cache.h = nullptr;
            if ((rc = gpad_create(&cache.h, dev, nullptr))) return rc;
            cache.device = dev;
            cache.h->keep_stage = true;
        }
        gpad_handle_t h = cache.h;
        // host matrices: reuse the bound problem when (dims, L, ML, G) equal the last call's; the
        // comparison is the full contents (a caller may rewrite its buffers in place).  Device
        // matrices are always repacked (two stream-ordered pack kernels, no copy).
        const bool host = dims->memory == GPAD_MEM_HOST;
        const size_t bytes = (size_t)dims->n * dims->m * esize(dims->dtype) * (dims->shared ? 1 : dims->batch);
        bool same = false;
        if (host && h->ready && h->shadow_ok && L == h->shadow_L && same_dims(h->shadow_dims, *dims) &&
            h->shadow.size() == 2 * bytes)
            same = std::memcmp(h->shadow.data(), ML, bytes) == 0 && std::memcmp(h->shadow.data() + bytes, G, bytes) == 0;
        if (!same) {
            if ((rc = gpad_setup(h, dims, ML, G, L))) return rc;
            if (host) {
                h->shadow.resize(2 * bytes);
                std::memcpy(h->shadow.data(), ML, bytes);
                std::memcpy(h->shadow.data() + bytes, G, bytes);
                h->shadow_dims = *dims;
                h->shadow_L = L;
                h->shadow_ok = true;
            }
        }
        if ((rc = gpad_run(h, z0, y0, M, g, N, tol, st))) return rc;
        return gpad_sync(h);
    });
}

}  // extern "C"
