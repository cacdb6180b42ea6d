// gpad_state.cpp -- per-state QP data and closed-loop MPC (gpad.m:79-95): the
// plant, signal and class bindings, gpad_run_state and gpad_closed_loop.  A closed loop runs either as
// one launch (gpad_loop*.hip: run_loop_one_launch) or step by step (run_loop_lockstep).
#include <algorithm>
#include <cmath>

#include "gpad_farkas.h"
#include "gpad_host.h"

void attach_plant(gpad_handle_t h, const gpad::PlantStore* store, int first, bool all) {
    h->plant = store;
    h->plant_first = first;
    h->plant_all = all;
}

// gpad_setup_plant (one plant) and gpad_setup_plant_batch (dims.batch copies) into the handle's own store
static int setup_plant_impl(gpad_handle_t h, int nx, int nu, const void* PM, const void* M0, const void* Pg,
                            const void* g0, const void* A, const void* B, bool per_instance, const char* fn) {
    const std::string where(fn);
    if (!h) return fail(GPAD_ERR_INVALID, where + ": null handle");
    if (h->cls) {
        if (per_instance) return no_classes(fn);
        HIP_TRY(hipSetDevice(h->device));
        return gpad::classes_setup_plant(h->cls, false, nx, nu, PM, M0, Pg, g0, A, B);  // the same maps for every class
    }
    if (!h->ready) return fail(GPAD_ERR_NOT_SETUP, where + ": call gpad_setup first");
    HIP_TRY(hipSetDevice(h->device));
    return h->own_plant.bind_plant(fn, h->dims, per_instance ? h->dims.batch : 0, nx, nu, PM, M0, Pg, g0, A, B,
                                   h->stream);
}

extern "C" int gpad_setup_plant(gpad_handle_t h, int nx, int nu, const void* PM, const void* M0,
                                const void* Pg, const void* g0, const void* A, const void* B) {
    return gpad::abi_guard("gpad_setup_plant", [&]() -> int {
        return setup_plant_impl(h, nx, nu, PM, M0, Pg, g0, A, B, false, "gpad_setup_plant");
    });
}

extern "C" int gpad_setup_plant_batch(gpad_handle_t h, int nx, int nu, const void* PM, const void* M0,
                                      const void* Pg, const void* g0, const void* A, const void* B) {
    return gpad::abi_guard("gpad_setup_plant_batch", [&]() -> int {
        return setup_plant_impl(h, nx, nu, PM, M0, Pg, g0, A, B, true, "gpad_setup_plant_batch");
    });
}

// ---- class binding (gpad_classes.cpp) ---------------------------------------------------------------
extern "C" int gpad_class_order(const int* class_of, int batch, int K, int* perm, int* offsets) {
    return gpad::abi_guard("gpad_class_order", [&]() -> int {
        if (!class_of || !perm || !offsets) return fail(GPAD_ERR_INVALID, "gpad_class_order: null argument");
        if (batch < 1 || K < 1) return fail(GPAD_ERR_INVALID, "gpad_class_order: batch and K must be >= 1");
        if (!gpad::class_order(class_of, batch, K, perm, offsets))
            return fail(GPAD_ERR_INVALID, "gpad_class_order: class_of holds an id outside 0..K-1");
        return GPAD_OK;
    });
}

extern "C" int gpad_setup_classes(gpad_handle_t h, const gpad_dims_t* dims, int K, const int* class_of,
                                  const void* ML, const void* G, double L) {
    return gpad::abi_guard("gpad_setup_classes", [&]() -> int {
        if (!h) return fail(GPAD_ERR_INVALID, "gpad_setup_classes: null handle");
        HIP_TRY(hipSetDevice(h->device));
        gpad::ClassBinding* cb = nullptr;
        const int rc = gpad::classes_setup(&cb, h->device, h->stream, h->tune, dims, K, class_of, ML, G, L);
        if (rc) return rc;  // (the handle keeps what it had)
        // the handle's own problem, plant and last run go too: the binding serves every run from here on
        unbind_problem(h);
        h->own_plant.unbind();
        h->last_batch = 0;
        h->cls = cb;
        return GPAD_OK;
    });
}

extern "C" int gpad_setup_plant_classes(gpad_handle_t h, int nx, int nu, const void* PM, const void* M0,
                                        const void* Pg, const void* g0, const void* A, const void* B) {
    return gpad::abi_guard("gpad_setup_plant_classes", [&]() -> int {
        if (!h) return fail(GPAD_ERR_INVALID, "gpad_setup_plant_classes: null handle");
        if (!h->cls) return fail(GPAD_ERR_NOT_SETUP, "gpad_setup_plant_classes: call gpad_setup_classes first");
        HIP_TRY(hipSetDevice(h->device));
        return gpad::classes_setup_plant(h->cls, true, nx, nu, PM, M0, Pg, g0, A, B);
    });
}

extern "C" int gpad_class_loop_fused(gpad_handle_t h, int on) {
    return gpad::abi_guard("gpad_class_loop_fused", [&]() -> int {
        if (!h) return fail(GPAD_ERR_INVALID, "gpad_class_loop_fused: null handle");
        if (on != 0 && on != 1) return fail(GPAD_ERR_INVALID, "gpad_class_loop_fused: on must be 0 or 1");
        if (!h->cls) return fail(GPAD_ERR_NOT_SETUP, "gpad_class_loop_fused: call gpad_setup_classes first");
        HIP_TRY(hipSetDevice(h->device));
        return gpad::classes_loop_fused(h->cls, on != 0, h->tune);
    });
}

extern "C" int gpad_class_loop_deal(const int* counts, int K, int grid, int* start_class) {
    return gpad::abi_guard("gpad_class_loop_deal", [&]() -> int {
        if (!counts || !start_class) return fail(GPAD_ERR_INVALID, "gpad_class_loop_deal: null argument");
        if (K < 1 || grid < 1) return fail(GPAD_ERR_INVALID, "gpad_class_loop_deal: K and grid must be >= 1");
        if (!gpad::class_loop_deal(counts, K, grid, start_class))
            return fail(GPAD_ERR_INVALID, "gpad_class_loop_deal: a negative count, or every class empty");
        return GPAD_OK;
    });
}

// the store the handle runs with holds a plant of its problem (its own: bound for this batch)
static bool plant_bound(gpad_handle_t h) {
    const gpad::PlantStore& ps = *h->plant;
    return ps.bound_for(h->dims) && (h->plant != &h->own_plant || !ps.stacked || ps.copies == h->dims.batch);
}

extern "C" int gpad_setup_signals(gpad_handle_t h, int ns, const void* SM, const void* Sg, const void* E) {
    return gpad::abi_guard("gpad_setup_signals", [&]() -> int {
        if (!h) return fail(GPAD_ERR_INVALID, "gpad_setup_signals: null handle");
        if (h->cls)
            return fail(GPAD_ERR_UNSUPPORTED, "gpad_setup_signals: not available on a handle with a class binding "
                                              "(gpad_setup_classes); bind class signals with gpad_setup_class_signals");
        if (!h->ready || !plant_bound(h))
            return fail(GPAD_ERR_NOT_SETUP, "gpad_setup_signals: call gpad_setup_plant first");
        if (ns < 0) return fail(GPAD_ERR_INVALID, "gpad_setup_signals: ns < 0");
        gpad::PlantStore& ps = h->own_plant;
        if (ns > 0 && E && !ps.dyn)
            return fail(GPAD_ERR_INVALID, "gpad_setup_signals: E given, plant bound without A, B");
        HIP_TRY(hipSetDevice(h->device));
        return ps.bind_signals(h->dims.memory, ns, ps.stacked ? ps.copies : 0, SM, Sg, E, h->stream);
    });
}

// gpad_setup_signals for a class-bound handle: one copy of SM, Sg, E per class (per_class) or one for all
extern "C" int gpad_setup_class_signals(gpad_handle_t h, int ns, int per_class, const void* SM, const void* Sg,
                                        const void* E) {
    return gpad::abi_guard("gpad_setup_class_signals", [&]() -> int {
        if (!h) return fail(GPAD_ERR_INVALID, "gpad_setup_class_signals: null handle");
        if (!h->cls) return fail(GPAD_ERR_NOT_SETUP, "gpad_setup_class_signals: call gpad_setup_classes first");
        bool dyn = false;
        if (!gpad::classes_has_plant(h->cls, &dyn))
            return fail(GPAD_ERR_NOT_SETUP, "gpad_setup_class_signals: call gpad_setup_plant or gpad_setup_plant_classes first");
        if (ns < 0) return fail(GPAD_ERR_INVALID, "gpad_setup_class_signals: ns < 0");
        if (per_class != 0 && per_class != 1)
            return fail(GPAD_ERR_INVALID, "gpad_setup_class_signals: per_class must be 0 or 1");
        if (ns > 0 && E && !dyn)
            return fail(GPAD_ERR_INVALID, "gpad_setup_class_signals: E given, plant bound without A, B");
        HIP_TRY(hipSetDevice(h->device));
        return gpad::classes_setup_signals(h->cls, ns, per_class != 0, SM, Sg, E);
    });
}

// The device arrays of one gpad_run_state / gpad_closed_loop call.  Handle::state holds
//   M(x) | g(x) | x ping | x pong | (signals) x in / out | (host callers) z | y | xs | us | S
// and the maps are the view `v` of the store the handle runs with: the plant's, or with signals their packed
// images [PM SM], [Pg Sg], [A E] (v.nxa: columns of an x ping-pong row, nx + ns).
template <typename T>
struct StateWork {
    int ns;                            // signal columns in use
    size_t zn, yn, xn, xan, xsn, usn, sn;  // element counts (xan: one x ping-pong array)
    T *Mx, *gx, *xa, *xb;
    T* xd;                             // signals: the dense [batch][nx] states in, then out; else null
    T *dz, *dy, *dxs, *dus;            // the caller's arrays, or (host callers) their staged copies
    T* S_up;                           // host callers with signals: where S is staged; else null
    const T* dS;                       // [nsolve][batch][ns]
    gpad::PlantView<T> v;
};

// sizes Handle::state for the call and places the arrays in it (nothing is enqueued)
template <typename T>
static int state_work(gpad_handle_t h, T* z, T* y, const T* sg, int steps, T* xs, T* us, StateWork<T>* w) {
    const gpad_dims_t& d = h->dims;
    const size_t batch = (size_t)d.batch;
    const bool loop = steps > 0, host = d.memory == GPAD_MEM_HOST;
    const gpad::PlantStore& ps = *h->plant;
    const int ns = w->ns = sg ? ps.ns : 0;
    w->v = ps.view<T>(h->plant_first, h->plant_all, ns > 0);  // (taken per call: a rebinding may move the buffers)
    if (w->v.per_copy && w->v.copies != d.batch && !h->cloop)
        return fail(GPAD_ERR_INVALID, "a handle that sees a copy of the maps per class runs only the fused class loop");
    w->zn = batch * d.n;
    w->yn = batch * d.m;
    w->xn = batch * ps.nx;
    w->xan = batch * w->v.nxa;
    w->xsn = loop && xs ? (size_t)steps * w->xn : 0;
    w->usn = loop && us ? (size_t)steps * batch * ps.nu : 0;
    w->sn = (size_t)(loop ? steps : 1) * batch * ns;
    size_t elems = w->zn + w->yn + 2 * w->xan + (ns ? w->xn : 0);
    if (host) elems += w->zn + w->yn + w->xsn + w->usn + w->sn;
    if (int rc = h->state.ensure(sizeof(T) * elems)) return rc;
    w->Mx = (T*)h->state.p;
    w->gx = w->Mx + w->zn;
    w->xa = w->gx + w->yn;
    w->xb = w->xa + w->xan;
    w->xd = ns ? w->xb + w->xan : nullptr;
    w->dz = z;
    w->dy = y;
    w->dxs = xs;
    w->dus = us;
    w->dS = sg;
    if (host) {
        w->dz = w->xb + w->xan + (ns ? w->xn : 0);
        w->dy = w->dz + w->zn;
        w->dxs = w->xsn ? w->dy + w->yn : nullptr;
        w->dus = w->usn ? w->dy + w->yn + w->xsn : nullptr;
        if (ns) w->dS = w->S_up = w->dy + w->yn + w->xsn + w->usn;
    }
    return GPAD_OK;
}

// The shape rules of GPAD_OPT_LOOP_PANEL: shared matrices with a fragment image of at most 16 tiles; with a
// tolerance the iteration limit must fall on a test (the kernel's events are workgroup-uniform).
bool loop_panel_shape(gpad_handle_t h, int N, double tol, int nxa) {
    const gpad_dims_t& d = h->dims;
    return d.shared && h->frag_ok && h->frag_tiles >= 1 && h->frag_tiles <= 16 && !h->flat && !h->hess_ok && N >= 1 &&
           (d.kernel == GPAD_KERNEL_AUTO || d.kernel == GPAD_KERNEL_PANEL) &&
           (!(tol > 0.0) || N % d.check_every == 0) && gpad::loop_panel_supported(d.n, d.m, nxa, h->plant->nu);
}

// Which one-launch engine serves a closed loop of an f32 handle: GPAD_KERNEL_LOOP_PANEL, GPAD_KERNEL_LOOP, or
// 0 for the lockstep loop.
// GPAD_OPT_LOOP_ASYNC: the whole loop in one launch of gpad_loop_kernel, every pack stepping on
// its own (gpad_loop.hip).  Anything it does not cover runs the lockstep loop.
// (per-instance matrices: its solo variant, where the resident kernel holds the shape)
// GPAD_OPT_LOOP_PANEL comes first: the same loop on the MFMA panels (gpad_loop_panel.hip).
// A handle with the class tables attached (Handle::cloop) runs the fused class loop, GPAD_KERNEL_LOOP_CLASSES:
// gpad_classes.cpp attaches them only to a loop that meets loop_panel_shape.
static int one_launch_engine(gpad_handle_t h, bool loop, int N, double tol, int nxa) {
    if (h->cloop) return GPAD_KERNEL_LOOP_CLASSES;
    if (h->tune.restart > 0) return 0;  // GPAD_OPT_RESTART: the one-launch loops do not carry the restart
    const gpad_dims_t& d = h->dims;
    const int n = d.n, m = d.m, nu = h->plant->nu;
    const bool lpanel = loop && h->tune.loop_panel && loop_panel_shape(h, N, tol, nxa);
    const bool async = lpanel || (loop && h->tune.loop_async && !h->flat && !h->hess_ok && N >= 1 &&
                                  (!(h->zbound > 0.0 && tol > 0.0) || h->tune.fk_loop_async) &&
                                  (d.kernel == GPAD_KERNEL_AUTO || d.kernel == GPAD_KERNEL_RESIDENT) &&
                                  gpad::loop_supported(n, m, nxa, nu));
    return lpanel ? GPAD_KERNEL_LOOP_PANEL : async ? GPAD_KERNEL_LOOP : 0;
}

// The whole loop in one launch (Handle::q64, the pack queue counter, is zeroed by the caller).  The final
// states land in *x_end.
static int run_loop_one_launch(gpad_handle_t h, const StateWork<float>& w, int engine, int nsolve, int N, double tol,
                               int warm, const float** x_end) {
    const gpad_dims_t& d = h->dims;
    const gpad::ClassLoop* cl = engine == GPAD_KERNEL_LOOP_CLASSES ? h->cloop : nullptr;
    const bool lpanel = engine == GPAD_KERNEL_LOOP_PANEL || cl;
    const int ns = w.ns;
    gpad::LoopArgs la{};
    gpad::SolveArgs<float>& a = la.s;
    fill_solve_args<float>(h, N, tol, &a);
    a.gscale = -1.0 / h->L;
    a.z = w.dz;
    a.y = w.dy;
    a.iters = (int*)h->counters.p;
    a.conv = a.iters;  // (the kernel indexes both from the counters' base, [steps][iters | conv])
    a.qctr = static_cast<int*>(h->q64.p);
    la.PM = w.v.PM;
    la.M0 = w.v.M0;
    la.Pg = w.v.Pg;
    la.g0 = w.v.g0;
    la.A = w.v.A;
    la.B = w.v.B;
    la.x_in = ns ? w.xd : w.xa;  // (dense rows of nx either way; the kernel reads S itself)
    la.x_out = ns ? w.xa : w.xb;
    la.ns = ns;
    la.S = ns ? w.dS : nullptr;
    la.xs = w.dxs;
    la.us = w.dus;
    la.gmax = tol > 0.0 ? reinterpret_cast<double*>((char*)h->status.p + (nsolve > 1 ? offsetof(RunStatus, acc)
                                                                                     : offsetof(RunStatus, part)))
                        : nullptr;
    la.nx = h->plant->nx;
    la.nu = h->plant->nu;
    la.steps = nsolve;
    la.warm = warm ? 1 : 0;
    la.per_plant = w.v.per_copy ? 1 : 0;
    const bool fk_on = h->zbound > 0.0 && tol > 0.0;  // the infeasibility certificate (gpad_setup_infeasibility)
    int grid;
    if (cl) {  // every class in one launch: its images, counters and tables (the maps are in w already)
        a.frag = cl->frag;
        a.frag_tiles = h->frag_tiles;
        a.qctr = cl->qctr;
        la.cls_K = cl->K;
        la.cls_off = cl->off;
        la.cls_start = cl->start;
        grid = cl->grid;
    } else if (lpanel) {
        a.frag = h->frag.p;
        a.frag_tiles = h->frag_tiles;
        grid = gpad::loop_panel_grid(d.n, d.m, d.batch, h->num_cus, &h->tune);
    } else {
        grid = std::min(d.batch, h->num_cus * gpad::loop_blocks_per_cu(la, fk_on));
        if (h->tune.duo_max_grid > 0 && h->tune.duo_max_grid < grid) grid = h->tune.duo_max_grid;
        grid = std::min(grid, (int)gpad::kAbsmaxMaxBlocks);
    }
    // (the panel loop reads the bound alone; gpad_loop_kernel's certificate twins the values launch_solve builds.
    // A bound reaches launch_loop only with gpad_infeasibility_loop_async on: one_launch_engine)
    const gpad::FarkasArgs fk{lpanel ? nullptr : (const double*)h->frows.p, d.shared ? 0 : (long long)h->ldm, h->zbound};
    const hipError_t e = lpanel ? gpad::launch_loop_panel(la, grid, h->stream, fk_on ? &fk : nullptr)
                                : gpad::launch_loop(la, grid, h->stream, fk_on ? &fk : nullptr);
    if (e != hipSuccess) return fail(GPAD_ERR_HIP, std::string("loop kernel: ") + hipGetErrorString(e));
    h->last_phased = false;
    h->last_p64 = false;
    h->last_N = N;
    *x_end = la.x_out;
    return GPAD_OK;
}

// x_{t+1} from x_t and step t's z (gpad.m:91-94: u = z*(1:nu); x <- A x + B u); with signals
// x <- A x + E S[t] + B u, with S[t + 1] moved in beside it and the last step's dense states written to xd
template <typename T>
static hipError_t plant_step(gpad_handle_t h, const StateWork<T>& w, int t, int nsolve, const T* xc, T* xnext) {
    const int n = h->dims.n, batch = h->dims.batch, nx = h->plant->nx, nu = h->plant->nu, ns = w.ns;
    T* xs_t = w.dxs ? w.dxs + (size_t)t * w.xn : nullptr;
    T* us_t = w.dus ? w.dus + (size_t)t * batch * nu : nullptr;
    if (!ns) return gpad::launch_plant_step<T>(w.v.A, w.v.B, xc, w.dz, n, xnext, nx, nu, batch, xs_t, us_t, w.v.per_copy, h->stream);
    const bool last = t + 1 == nsolve;
    return gpad::launch_plant_step_sig<T>(w.v.A, w.v.B, xc, w.dz, n, xnext, last ? nullptr : w.dS + (size_t)(t + 1) * batch * ns,
                                          nx, ns, nu, batch, xs_t, us_t, last ? w.xd : nullptr, w.v.per_copy, h->stream);
}

// Step by step: the two affine maps, the solve, the fold of its max |g| and the plant step, nsolve times
// (loop == false: the one solve of gpad_run_state).  *kernel = the last solve's family; the final states land
// in *x_end.
template <typename T>
static int run_loop_lockstep(gpad_handle_t h, const StateWork<T>& w, bool loop, int nsolve, int N, double tol, int warm,
                             int* kernel, const T** x_end) {
    const gpad_dims_t& d = h->dims;
    const int n = d.n, m = d.m, batch = d.batch, ns = w.ns;
    int* counters = (int*)h->counters.p;
    T* xc = w.xa;
    T* xnext = w.xb;
    if (ns) HIP_TRY(gpad::launch_sig_state<T>(w.xd, w.dS, w.xa, h->plant->nx, ns, batch, h->stream));  // [x_0; S[0]]
    for (int t = 0; t < nsolve; ++t) {
        HIP_TRY(gpad::launch_affine2<T>(w.v.PM, w.v.M0, n, w.Mx, w.v.Pg, w.v.g0, m, w.gx, xc, w.v.nxa, batch, w.v.per_copy,
                                        h->stream));
        if (loop && !warm) {  // acceldualgrad.m:16-17: every MPC step starts from z = y = 0
            HIP_TRY(hipMemsetAsync(w.dz, 0, sizeof(T) * w.zn, h->stream));
            HIP_TRY(hipMemsetAsync(w.dy, 0, sizeof(T) * w.yn, h->stream));
        }
        int* it = counters + 2 * (size_t)batch * t;
        int* rst = h->last_restart ? (int*)h->restarts.p + (size_t)batch * t : nullptr;  // (restart_counts)
        if (int rc = launch_solve<T>(h, w.dz, w.dy, w.Mx, w.gx, N, tol, false, it, it + batch, kernel, rst)) return rc;
        if (nsolve > 1 && tol > 0.0) {  // this step's max |g| slots -> the run's (RunStatus::acc)
            char* sp = (char*)h->status.p;
            HIP_TRY(gpad::launch_absmax_fold(reinterpret_cast<const double*>(sp + offsetof(RunStatus, part)),
                                             reinterpret_cast<double*>(sp + offsetof(RunStatus, acc)), t == 0,
                                             h->stream));
        }
        if (loop) {
            HIP_TRY(plant_step<T>(h, w, t, nsolve, xc, xnext));
            std::swap(xc, xnext);
        }
    }
    *x_end = ns ? w.xd : xc;  // (signals: the last step wrote the dense states there)
    return GPAD_OK;
}

template <typename T>
static int state_typed(gpad_handle_t h, T* x, T* z, T* y, const T* sg, int steps, int N, double tol, int warm,
                       T* xs, T* us, gpad_stats_t* st) {
    // steps == 0: one solve at x (gpad_run_state); steps >= 1: closed loop (gpad_closed_loop)
    // signals (sg != null): the same run on the augmented state [x; s], rows of nxa = nx + ns columns over
    // the packed images of gpad_setup_signals; sg is [batch][ns], or [steps][batch][ns] for a loop
    const gpad_dims_t& d = h->dims;
    const bool loop = steps > 0, host = d.memory == GPAD_MEM_HOST;
    const int nsolve = loop ? steps : 1;
    int rc = ensure_schedule(h, N, nullptr, nullptr);
    if (rc) return rc;
    if ((rc = h->counters.ensure(sizeof(int) * 2 * (size_t)d.batch * nsolve))) return rc;
    if ((rc = restart_counts(h, nsolve, nullptr))) return rc;
    StateWork<T> w{};
    if ((rc = state_work<T>(h, z, y, sg, steps, xs, us, &w))) return rc;
    if (w.S_up) HIP_TRY(hipMemcpyAsync(w.S_up, sg, sizeof(T) * w.sn, hipMemcpyHostToDevice, h->stream));
    const hipMemcpyKind in_kind = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    const hipMemcpyKind out_kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    HIP_TRY(hipMemcpyAsync(w.ns ? w.xd : w.xa, x, sizeof(T) * w.xn, in_kind, h->stream));
    if (host && (!loop || warm)) {
        HIP_TRY(hipMemcpyAsync(w.dz, z, sizeof(T) * w.zn, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(w.dy, y, sizeof(T) * w.yn, hipMemcpyHostToDevice, h->stream));
    }
    const double margin = sizeof(T) == sizeof(float) ? gpad::ViolMargin<float>::value : gpad::ViolMargin<double>::value;
    if ((rc = reset_status(h, tol, margin))) return rc;  // g(x) unscaled: margin * L * (1/L)
    const int engine = sizeof(T) == sizeof(float) ? one_launch_engine(h, loop, N, tol, w.v.nxa) : 0;
    if (engine == GPAD_KERNEL_LOOP_CLASSES) {  // one claim counter per class
        HIP_TRY(hipMemsetAsync(h->cloop->qctr, 0, sizeof(int) * (size_t)h->cloop->K, h->stream));
    } else if (engine) {  // the pack queue counter, zeroed ahead of the timed launch
        if ((rc = h->q64.ensure(sizeof(int)))) return rc;
        HIP_TRY(hipMemsetAsync(h->q64.p, 0, sizeof(int), h->stream));
    }
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    int kernel = engine;
    const T* x_end = nullptr;
    if (engine) {
        if constexpr (sizeof(T) == sizeof(float)) rc = run_loop_one_launch(h, w, engine, nsolve, N, tol, warm, &x_end);
    } else {
        rc = run_loop_lockstep<T>(h, w, loop, nsolve, N, tol, warm, &kernel, &x_end);
    }
    if (rc) return rc;
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    h->timed = true;
    h->last_kernel = kernel;
    h->last_batch = d.batch;
    h->last_steps = nsolve;
    if (loop) HIP_TRY(hipMemcpyAsync(x, x_end, sizeof(T) * w.xn, out_kind, h->stream));
    if (host) {
        HIP_TRY(hipMemcpyAsync(z, w.dz, sizeof(T) * w.zn, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(y, w.dy, sizeof(T) * w.yn, hipMemcpyDeviceToHost, h->stream));
        if (w.xsn) HIP_TRY(hipMemcpyAsync(xs, w.dxs, sizeof(T) * w.xsn, hipMemcpyDeviceToHost, h->stream));
        if (w.usn) HIP_TRY(hipMemcpyAsync(us, w.dus, sizeof(T) * w.usn, hipMemcpyDeviceToHost, h->stream));
        if (!st) return gpad_sync(h);
    }
    if (st) return collect_stats(h, st);
    return GPAD_OK;
}

// with_sig: the _signals entry points (sg: their s / S)
static int state_impl(gpad_handle_t h, void* x, void* z, void* y, const void* sg, bool with_sig, int steps, int N,
                      double tol, int warm, void* xs, void* us, gpad_stats_t* st, const char* where) {
    if (!h) return fail(GPAD_ERR_INVALID, std::string(where) + ": null handle");
    if (h->cls) {  // (with_sig: class signals, gpad_setup_class_signals; without them unsupported as before)
        HIP_TRY(hipSetDevice(h->device));
        return gpad::classes_state(h->cls, x, z, y, sg, with_sig, where, steps, N, tol, warm, xs, us, st);
    }
    if (!h->ready) return fail(GPAD_ERR_NOT_SETUP, std::string(where) + ": call gpad_setup first");
    if (!plant_bound(h))
        return fail(GPAD_ERR_NOT_SETUP, std::string(where) + ": call gpad_setup_plant after gpad_setup");
    if (with_sig && h->plant->ns== 0)
        return fail(GPAD_ERR_NOT_SETUP, std::string(where) + ": call gpad_setup_signals first");
    if (!with_sig && h->plant->ns!= 0)  // (dropping a disturbance silently is worse than an error)
        return fail(GPAD_ERR_INVALID, std::string(where) + ": signals are bound, call the _signals entry point");
    if (steps > 0 && !h->plant->dyn)
        return fail(GPAD_ERR_NOT_SETUP, std::string(where) + ": plant bound without A, B");
    if (!x || !z || !y || (with_sig && !sg)) return fail(GPAD_ERR_INVALID, std::string(where) + ": null vector");
    if (N < 0 || steps < 0) return fail(GPAD_ERR_INVALID, std::string(where) + ": N, steps must be >= 0");
    if (!(tol <= 0.0) && !std::isfinite(tol)) return fail(GPAD_ERR_INVALID, std::string(where) + ": bad tol");
    HIP_TRY(hipSetDevice(h->device));
    if (h->dims.dtype == GPAD_DTYPE_F64)
        return state_typed<double>(h, (double*)x, (double*)z, (double*)y, (const double*)sg, steps, N, tol, warm,
                                   (double*)xs, (double*)us, st);
    return state_typed<float>(h, (float*)x, (float*)z, (float*)y, (const float*)sg, steps, N, tol, warm, (float*)xs,
                              (float*)us, st);
}

extern "C" {

int gpad_run_state(gpad_handle_t h, const void* x, void* z0, void* y0, int N, double tol,
                   gpad_stats_t* st) {
    return gpad::abi_guard("gpad_run_state", [&]() -> int {
        return state_impl(h, const_cast<void*>(x), z0, y0, nullptr, false, 0, N, tol, 1, nullptr, nullptr, st,
                          "gpad_run_state");
    });
}

int gpad_run_state_signals(gpad_handle_t h, const void* x, const void* s, void* z0, void* y0, int N, double tol,
                           gpad_stats_t* st) {
    return gpad::abi_guard("gpad_run_state_signals", [&]() -> int {
        return state_impl(h, const_cast<void*>(x), z0, y0, s, true, 0, N, tol, 1, nullptr, nullptr, st,
                          "gpad_run_state_signals");
    });
}

int gpad_closed_loop(gpad_handle_t h, void* x, void* z, void* y, int steps, int N, double tol, int warm,
                     void* xs, void* us, gpad_stats_t* st) {
    return gpad::abi_guard("gpad_closed_loop", [&]() -> int {
        if (steps == 0) return GPAD_OK;
        return state_impl(h, x, z, y, nullptr, false, steps, N, tol, warm, xs, us, st, "gpad_closed_loop");
    });
}

int gpad_closed_loop_signals(gpad_handle_t h, void* x, void* z, void* y, const void* S, int steps, int N, double tol,
                             int warm, void* xs, void* us, gpad_stats_t* st) {
    return gpad::abi_guard("gpad_closed_loop_signals", [&]() -> int {
        if (steps == 0) return GPAD_OK;
        return state_impl(h, x, z, y, S, true, steps, N, tol, warm, xs, us, st, "gpad_closed_loop_signals");
    });
}

}  // extern "C"
