// gpad_host.cpp -- host runtime behind the C-ABI of include/gpad.h: the handle's life cycle, the
// options, the run status block and the stats, phase and per-step entry points.
//
// A handle owns the packed device copies of the constant matrices (k-major -ML and G/L,
// and the MFMA fragment image for shared-matrix batches), the theta/beta table, per-instance
// workspaces for host-memory callers, per-instance iteration/convergence counters and the
// HIP events that time the solve launch (gpad_host.h gpad_handle_s).  Binding a problem is
// gpad_setup.cpp, a solve gpad_run.cpp, the per-state and closed-loop runs gpad_state.cpp.
#include <algorithm>
#include <cmath>
#include <memory>

#include "gpad_host.h"

static thread_local std::string g_last_error;

int gpad::set_last_error(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

int reset_status(gpad_handle_t h, double tol, double floor_scale) {
    const bool fresh = h->status.p == nullptr;
    int rc = h->status.ensure(sizeof(RunStatus));
    if (rc) return rc;
    // the error word once (fetch_status clears it behind each read); the |g| slots are stored by
    // the run's first writer (SolveArgs::gmax_part), so a solve enqueues no memset here
    if (fresh) HIP_TRY(hipMemsetAsync(h->status.p, 0, sizeof(RunStatus), h->stream));
    h->last_tol = tol;
    h->last_floor_scale = floor_scale;
    h->failed_run = false;
    return GPAD_OK;
}

// Enqueue the copy of the status block to *rs (the caller synchronises the stream): the error word,
// and with `maxima` the per-workgroup |g| maxima of the run (RunStatus::part).  The error word is
// cleared behind the copy: every error bit is reported exactly once.
static int fetch_status(gpad_handle_t h, RunStatus* rs, bool maxima = false) {
    rs->err = 0;
    if (!h->status.p) return GPAD_OK;
    const size_t bytes = !maxima ? offsetof(RunStatus, part)
                                 : (h->last_steps > 1 ? sizeof(RunStatus) : offsetof(RunStatus, acc));
    HIP_TRY(hipMemcpyAsync(rs, h->status.p, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemsetAsync(h->status.p, 0, sizeof(int), h->stream));
    return GPAD_OK;
}

static double status_gmax(gpad_handle_t h, const RunStatus& rs) {
    const double* part = h->last_steps > 1 ? rs.acc : rs.part;  // several solves: folded per step
    double g = 0.0;
    for (int b = 0; b < gpad::kAbsmaxMaxBlocks; ++b) {
        if (std::isnan(part[b])) return part[b];  // a NaN in g (absmax_nan keeps it)
        g = std::max(g, part[b]);
    }
    return g;
}

static int status_error(gpad_handle_t h, const RunStatus& rs) {
    if (rs.err == 0 && !h->failed_run) return GPAD_OK;
    if (rs.err == 0)
        return fail(GPAD_ERR_DEVICE, "the run failed on the device (reported by an earlier call; its results "
                                     "are invalid)");
    h->failed_run = true;
    return fail(GPAD_ERR_DEVICE, std::string("device error bits 0x") + std::to_string(rs.err) +
                                     ((rs.err & gpad::kDevErrHandoff) ? ": a chain hand-off wait expired "
                                                                        "(the run's results are invalid)"
                                                                      : ""));
}

void end_classes(gpad_handle_t h) {
    gpad::classes_free(h->cls);
    h->cls = nullptr;
}

int no_classes(const char* fn) {
    return fail(GPAD_ERR_UNSUPPORTED, std::string(fn) + ": not available on a handle with a class binding "
                                                        "(gpad_setup_classes)");
}

// the handle's own option (a class binding's children each get the call forwarded, gpad_set_option below)
static int set_own_option(gpad_handle_t h, int option, int value) {
    for (const OptionSpec& o : kOptions) {
        if (o.id != option) continue;
        if (option == GPAD_OPT_PLAN) {
            h->plan.nph = 0;
            h->plan_key = 0;
        }
        if (option == GPAD_OPT_FLAT_WAVES && value != GPAD_OPT_DEFAULT && value != 0 && value != 8 && value != 16)
            return fail(GPAD_ERR_INVALID, "gpad_set_option: flat waves must be 0, 8 or 16");
        int& field = h->tune.*o.field;
        if (value == GPAD_OPT_DEFAULT) {
            field = gpad::Tuning{}.*o.field;
            return GPAD_OK;
        }
        if (value < o.lo || value > o.hi) return fail(GPAD_ERR_INVALID, "gpad_set_option: value out of range");
        field = o.inverted ? 1 - value : value;
        return GPAD_OK;
    }
    return fail(GPAD_ERR_INVALID, "gpad_set_option: unknown option");
}

// Counters are laid out [steps][iters[batch] | conv[batch]].
int collect_stats(gpad_handle_t h, gpad_stats_t* st) {
    const int batch = h->last_batch;
    const size_t entries = (size_t)batch * h->last_steps;
    h->h_counts.resize(2 * entries);
    HIP_TRY(hipMemcpyAsync(h->h_counts.data(), h->counters.p, sizeof(int) * 2 * entries,
                           hipMemcpyDeviceToHost, h->stream));
    RunStatus& rs = h->h_status;
    int rc = fetch_status(h, &rs, true);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    st->iterations = 0;
    st->converged = 0;
    st->total_iterations = 0;
    for (int t = 0; t < h->last_steps; ++t) {
        const int* it = h->h_counts.data() + (size_t)2 * batch * t;
        const int* cv = it + batch;
        for (int b = 0; b < batch; ++b) {
            st->iterations = std::max(st->iterations, it[b]);
            st->converged += cv[b] != 0 && cv[b] != GPAD_CODE_INFEASIBLE;  // (a certificate is no convergence)
            st->total_iterations += it[b];
            if (st->iters) st->iters[(size_t)t * batch + b] = it[b];
            if (st->codes) st->codes[(size_t)t * batch + b] = cv[b];
        }
    }
    // (a run with an infeasibility bound in force plans nothing: its phases have no pairs and no finisher, which
    // the planner models, and its counts are cut short by code 5)
    if (h->last_phased && h->last_steps == 1 && !(h->zbound > 0.0 && h->last_tol > 0.0) && !h->last_restart) {
        update_plan(h, h->h_counts.data(), batch, h->last_N);
        h->plan_pending = false;  // these counts are at least as recent as any copy in flight
    }
    if (h->last_p64 && h->last_steps == 1) {
        build_p64_order(h, h->h_counts.data(), batch);
        h->plan_pending = false;
    }
    st->kernel = h->last_kernel;
    float ms = 0.0f;
    st->kernel_ms = 0.0;
    if (h->timed && hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) st->kernel_ms = ms;
    st->tol_floor = h->last_tol > 0.0 ? h->last_floor_scale * status_gmax(h, rs) : 0.0;
    st->flags = (h->last_tol > 0.0 && h->last_tol < st->tol_floor) ? GPAD_FLAG_TOL_FLOOR : 0;
    if (h->last_tol > 0.0 && !std::isfinite(st->tol_floor))  // NaN / inf in g: nothing certifies
        st->flags |= GPAD_FLAG_TOL_FLOOR | GPAD_FLAG_NONFINITE_G;
    return status_error(h, rs);
}

extern "C" {

const char* gpad_version(void) { return "gpad-mi355x 0.6 (gfx950)"; }

int gpad_device_count(void) {
    return gpad::abi_guard("gpad_device_count", [&]() -> int {
        int count = 0;
        const hipError_t e = hipGetDeviceCount(&count);
        if (e != hipSuccess) return fail(GPAD_ERR_NO_DEVICE, hip_detail("gpad_device_count: hipGetDeviceCount", e));
        return count;
    });
}

const char* gpad_strerror(int status) {
    switch (status) {
        case GPAD_OK: return "ok";
        case GPAD_ERR_INVALID: return "invalid argument";
        case GPAD_ERR_HIP: return "HIP runtime error";
        case GPAD_ERR_NOMEM: return "device out of memory";
        case GPAD_ERR_UNSUPPORTED: return "unsupported shape/kernel combination";
        case GPAD_ERR_NOT_SETUP: return "gpad_run before gpad_setup";
        case GPAD_ERR_NO_DEVICE: return "no HIP device";
        case GPAD_ERR_DEVICE: return "device-side failure (results invalid)";
        default: return "unknown status";
    }
}

const char* gpad_last_error(void) { return g_last_error.c_str(); }

int gpad_create(gpad_handle_t* out, int device, void* stream) {
    return gpad::abi_guard("gpad_create", [&]() -> int {
        if (!out) return fail(GPAD_ERR_INVALID, "gpad_create: null handle pointer");
        *out = nullptr;
        int count = 0;
        const hipError_t e = hipGetDeviceCount(&count);
        if (e != hipSuccess) return fail(GPAD_ERR_NO_DEVICE, hip_detail("gpad_create: hipGetDeviceCount", e));
        if (count <= 0) return fail(GPAD_ERR_NO_DEVICE, "gpad_create: hipGetDeviceCount reported 0 devices");
        if (device < 0 || device >= count)
            return fail(GPAD_ERR_INVALID, "gpad_create: bad device index " + std::to_string(device) + " (" +
                                              std::to_string(count) + " visible)");
        HIP_TRY(hipSetDevice(device));
        auto h = std::make_unique<gpad_handle_s>();
        h->device = device;
        h->stream = static_cast<hipStream_t>(stream);  // NULL = the device's default (null) stream
        {
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
                h->num_cus = prop.multiProcessorCount;
        }
        HIP_TRY(hipEventCreate(&h->ev0));
        HIP_TRY(hipEventCreate(&h->ev1));
        *out = h.release();
        return GPAD_OK;
    });
}

int gpad_destroy(gpad_handle_t h) {
    return gpad::abi_guard("gpad_destroy", [&]() -> int {
        if (!h) return GPAD_OK;
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
        end_classes(h);
        h->MGt.release();
        h->GLt.release();
        h->GLx.release();
        h->Hq.release();
        h->frows.release();
        h->frag64.release();
        h->hfrag64.release();
        h->q64.release();
        h->p64_order.release();
        h->frag.release();
        h->stage.release();
        h->theta.release();
        h->beta.release();
        h->work.release();
        h->counters.release();
        h->restarts.release();
        h->rs_pos.release();
        h->pwork.release();
        h->lipwork.release();
        h->status.release();
        h->own_plant.release();
        h->state.release();
        if (h->ev0) (void)hipEventDestroy(h->ev0);
        if (h->ev1) (void)hipEventDestroy(h->ev1);
        if (h->plan_ev) (void)hipEventDestroy(h->plan_ev);
        if (h->plan_pin) (void)hipHostFree(h->plan_pin);
        delete h;
        return GPAD_OK;
    });
}

int gpad_set_stream(gpad_handle_t h, void* stream) {
    return gpad::abi_guard("gpad_set_stream", [&]() -> int {
        if (!h) return fail(GPAD_ERR_INVALID, "gpad_set_stream: null handle");
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipStreamSynchronize(h->stream));  // work queued on the old stream completes first
        h->stream = static_cast<hipStream_t>(stream);
        if (h->cls) return gpad::classes_set_stream(h->cls, h->stream);
        return GPAD_OK;
    });
}

int gpad_set_option(gpad_handle_t h, int option, int value) {
    return gpad::abi_guard("gpad_set_option", [&]() -> int {
        if (!h) return fail(GPAD_ERR_INVALID, "gpad_set_option: null handle");
        const int rc = set_own_option(h, option, value);
        if (rc || !h->cls) return rc;
        HIP_TRY(hipSetDevice(h->device));
        return gpad::classes_set_option(h->cls, option, value);  // every class applies it by its own rules
    });
}

int gpad_sync(gpad_handle_t h) {
    return gpad::abi_guard("gpad_sync", [&]() -> int {
        if (!h) return fail(GPAD_ERR_INVALID, "gpad_sync: null handle");
        HIP_TRY(hipSetDevice(h->device));
        if (h->cls) return gpad::classes_sync(h->cls);
        RunStatus& rs = h->h_status;
        int rc = fetch_status(h, &rs);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(h->stream));
        return status_error(h, rs);
    });
}

int gpad_accumulate_iterations(gpad_handle_t h, long long* acc) {
    return gpad::abi_guard("gpad_accumulate_iterations", [&]() -> int {
        if (!h || !acc) return fail(GPAD_ERR_INVALID, "gpad_accumulate_iterations: null argument");
        if (h->cls) {
            HIP_TRY(hipSetDevice(h->device));
            return gpad::classes_accumulate(h->cls, acc);
        }
        if (h->last_batch <= 0) return fail(GPAD_ERR_NOT_SETUP, "gpad_accumulate_iterations: no run yet");
        HIP_TRY(hipSetDevice(h->device));
        // counters: [steps][iters[batch] | conv[batch]]; each solve's iteration block in turn
        for (int t = 0; t < h->last_steps; ++t)
            HIP_TRY(gpad::launch_accumulate_iters((const int*)h->counters.p + (size_t)2 * h->last_batch * t,
                                                  h->last_batch, acc, h->stream));
        return GPAD_OK;
    });
}

int gpad_last_stats(gpad_handle_t h, gpad_stats_t* st) {
    return gpad::abi_guard("gpad_last_stats", [&]() -> int {
        if (!h || !st) return fail(GPAD_ERR_INVALID, "gpad_last_stats: null argument");
        if (h->cls) {
            HIP_TRY(hipSetDevice(h->device));
            return gpad::classes_last_stats(h->cls, st);
        }
        if (h->last_batch <= 0) return fail(GPAD_ERR_NOT_SETUP, "gpad_last_stats: no run yet");
        HIP_TRY(hipSetDevice(h->device));
        return collect_stats(h, st);
    });
}

int gpad_last_restarts(gpad_handle_t h, int* restarts, int cap) {
    return gpad::abi_guard("gpad_last_restarts", [&]() -> int {
        if (!h || !restarts || cap < 0) return fail(GPAD_ERR_INVALID, "gpad_last_restarts: bad argument");
        if (h->cls) {
            HIP_TRY(hipSetDevice(h->device));
            return gpad::classes_last_restarts(h->cls, restarts, cap);
        }
        // (no run yet: the zeros of one solve of the bound batch)
        const size_t entries = h->last_batch > 0 ? (size_t)h->last_batch * h->last_steps : (size_t)h->dims.batch;
        const int k = (int)std::min(entries, (size_t)cap);
        if (h->last_batch <= 0 || !h->last_restart || !h->restarts.p) {
            std::fill(restarts, restarts + k, 0);
            return k;
        }
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipMemcpyAsync(restarts, h->restarts.p, sizeof(int) * (size_t)k, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        return k;
    });
}

int gpad_phase_plan(gpad_handle_t h, int* ends, int* fins, int cap, double* cost_us) {
    return gpad::abi_guard("gpad_phase_plan", [&]() -> int {
        if (!h) return fail(GPAD_ERR_INVALID, "gpad_phase_plan: null handle");
        if (h->cls) return 0;  // (every class plans for itself)
        const int n = h->plan.nph;
        for (int i = 0; i < n && i < cap; ++i) {
            if (ends) ends[i] = h->plan.ends[i];
            if (fins) fins[i] = h->plan.fins[i];
        }
        if (cost_us) *cost_us = h->plan.cost_us;
        return n;
    });
}

int gpad_last_phases(gpad_handle_t h, int* ends, int* fins, int* counts, int cap, int* prior) {
    return gpad::abi_guard("gpad_last_phases", [&]() -> int {
        if (!h || cap < 0) return fail(GPAD_ERR_INVALID, "gpad_last_phases: bad argument");
        if (prior) *prior = 0;
        if (h->cls) return 0;
        if (!h->last_phased || !h->pwork.p || h->flat) return 0;  // not phased: no plan, no prior
        if (prior) *prior = h->last_prior ? 1 : 0;
        const int k = std::min(cap, h->last_phases.nph);
        for (int i = 0; i < k; ++i) {
            if (ends) ends[i] = h->last_phases.ends[i];
            if (fins) fins[i] = h->last_phases.fins[i];
        }
        if (counts && k > 0) {
            HIP_TRY(hipSetDevice(h->device));
            const int* dev = reinterpret_cast<const int*>(h->pwork.p) + 2 * (size_t)h->last_batch;  // panel_work_bytes
            HIP_TRY(hipMemcpyAsync(counts, dev, sizeof(int) * (size_t)k, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
        return k;
    });
}

int gpad_phase_counts(gpad_handle_t h, int* counts, int cap) {
    return gpad::abi_guard("gpad_phase_counts", [&]() -> int {
        if (!h || !counts || cap < 0) return fail(GPAD_ERR_INVALID, "gpad_phase_counts: bad argument");
        if (h->cls) return 0;
        if (!h->last_phased || !h->pwork.p) return 0;
        HIP_TRY(hipSetDevice(h->device));
        const int k = cap < gpad::kPanelMaxPhases ? cap : gpad::kPanelMaxPhases;
        const int* dev = reinterpret_cast<const int*>(h->pwork.p) + 2 * (size_t)h->last_batch;  // panel_work_bytes
        HIP_TRY(hipMemcpyAsync(counts, dev, sizeof(int) * (size_t)k, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        return k;
    });
}

#ifdef GPAD_STAMP
}  // extern "C"
namespace gpad {
hipError_t read_stamps(unsigned long long* out, size_t bytes);      // gpad_pairs.hip (diagnostic builds)
hipError_t read_res_stamps(unsigned long long* out, size_t bytes);  // gpad_resident.hip
hipError_t read_duo_stamps(unsigned long long* out, size_t bytes);  // gpad_duo.hip
}
extern "C" {
int gpad_debug_res_stamps(unsigned long long* out, size_t bytes) {
    return gpad::abi_guard("gpad_debug_res_stamps", [&]() -> int {
        HIP_TRY(gpad::read_res_stamps(out, bytes));
        return GPAD_OK;
    });
}
int gpad_debug_duo_stamps(unsigned long long* out, size_t bytes) {
    return gpad::abi_guard("gpad_debug_duo_stamps", [&]() -> int {
        HIP_TRY(gpad::read_duo_stamps(out, bytes));
        return GPAD_OK;
    });
}
// diagnostic builds only (not declared in gpad.h): the phase-anatomy stamps of the last panel-pair run
int gpad_debug_stamps(unsigned long long* out, size_t bytes) {
    return gpad::abi_guard("gpad_debug_stamps", [&]() -> int {
        HIP_TRY(gpad::read_stamps(out, bytes));
        return GPAD_OK;
    });
}
#endif

int gpad_plan_phases(const int* iters, int batch, int n, int m, int N, int check_every, int num_cus,
                     int* ends, int* fins, int cap, double* cost_us) {
    return gpad::abi_guard("gpad_plan_phases", [&]() -> int {
        if (!iters || batch <= 0 || n <= 0 || m <= 0 || N <= 0 || num_cus <= 0)
            return fail(GPAD_ERR_INVALID, "gpad_plan_phases: bad argument");
        gpad::PanelPlan p;
        gpad::panel_plan(iters, batch, n, m, N, check_every, num_cus, nullptr, &p);
        for (int i = 0; i < p.nph && i < cap; ++i) {
            if (ends) ends[i] = p.ends[i];
            if (fins) fins[i] = p.fins[i];
        }
        if (cost_us) *cost_us = p.cost_us;
        return p.nph;
    });
}

// ---- per-step entry points ---------------------------------------------------------------
int gpad_step1_extrapolate(gpad_handle_t h, const float* y, const float* ym1, float* w, float beta,
                           int m) {
    return gpad::abi_guard("gpad_step1_extrapolate", [&]() -> int {
        if (!h || !y || !ym1 || !w || m < 0) return fail(GPAD_ERR_INVALID, "gpad_step1: bad arguments");
        if (m == 0) return GPAD_OK;
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(gpad::launch_step1(y, ym1, w, beta, m, h->stream));
        return GPAD_OK;
    });
}

int gpad_step2_primal(gpad_handle_t h, const float* MGneg, const float* w, const float* gP,
                      float* zhat, int n, int m) {
    return gpad::abi_guard("gpad_step2_primal", [&]() -> int {
        if (!h || !MGneg || !w || !gP || !zhat || n <= 0 || m <= 0)
            return fail(GPAD_ERR_INVALID, "gpad_step2: bad arguments");
        if ((size_t)m * sizeof(float) > 64 * 1024) return fail(GPAD_ERR_UNSUPPORTED, "gpad_step2: m too large");
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(gpad::launch_step2(MGneg, w, gP, zhat, n, m, h->stream));
        return GPAD_OK;
    });
}

int gpad_step2_primal_flat(gpad_handle_t h, const float* MGf, const float* w, const float* gP,
                           float* zhat, int N, int n_u, int m) {
    return gpad::abi_guard("gpad_step2_primal_flat", [&]() -> int {
        if (!h || !MGf || !w || !gP || !zhat || N <= 0 || n_u <= 0 || m < 4 * n_u * N)
            return fail(GPAD_ERR_INVALID, "gpad_step2_flat: bad arguments");
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(gpad::launch_step2_flat(MGf, w, gP, zhat, N, n_u, m, h->stream));
        return GPAD_OK;
    });
}

int gpad_step4_project_flat(gpad_handle_t h, const float* GLf, float* yp1, const float* w,
                            const float* pD, const float* zhat, int N, int n_u, int m) {
    return gpad::abi_guard("gpad_step4_project_flat", [&]() -> int {
        if (!h || !GLf || !yp1 || !w || !pD || !zhat || N <= 0 || n_u <= 0 || m < 4 * n_u * N)
            return fail(GPAD_ERR_INVALID, "gpad_step4_flat: bad arguments");
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(gpad::launch_step4_flat(GLf, yp1, w, pD, zhat, N, n_u, m, h->stream));
        return GPAD_OK;
    });
}

int gpad_step3_average(gpad_handle_t h, float theta, const float* zm1, const float* zhat, float* z,
                       int n) {
    return gpad::abi_guard("gpad_step3_average", [&]() -> int {
        if (!h || !zm1 || !zhat || !z || n < 0) return fail(GPAD_ERR_INVALID, "gpad_step3: bad arguments");
        if (n == 0) return GPAD_OK;
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(gpad::launch_step3(theta, zm1, zhat, z, n, h->stream));
        return GPAD_OK;
    });
}

int gpad_step4_project(gpad_handle_t h, const float* GL, float* yp1, const float* w,
                       const float* pD, const float* zhat, int n, int m) {
    return gpad::abi_guard("gpad_step4_project", [&]() -> int {
        if (!h || !GL || !yp1 || !w || !pD || !zhat || n <= 0 || m <= 0)
            return fail(GPAD_ERR_INVALID, "gpad_step4: bad arguments");
        if ((size_t)n * sizeof(float) > 64 * 1024) return fail(GPAD_ERR_UNSUPPORTED, "gpad_step4: n too large");
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(gpad::launch_step4(GL, yp1, w, pD, zhat, n, m, h->stream));
        return GPAD_OK;
    });
}

}  // extern "C"
