// gpad_host.h -- what the host translation units share (gpad_host.cpp, gpad_setup.cpp, gpad_run.cpp,
// gpad_state.cpp, gpad_plant_store.cpp, gpad_classes.cpp, gpad_group.cpp): the error plumbing, the device buffer, the handle,
// the option table and the few functions that cross files.  Host only: never included by a .hip file.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <vector>

#include "../../include/gpad.h"
#include "gpad_abi.h"
#include "gpad_classes.h"
#include "gpad_internal.h"

inline int fail(int code, const std::string& msg) { return gpad::set_last_error(code, msg); }

// "<what>: hipErrorName (code N): description" -- the name and number of the HIP status, so a
// failure report says which runtime error it was (include/gpad.h gpad_last_error)
inline std::string hip_detail(const std::string& what, hipError_t e) {
    return what + ": " + hipGetErrorName(e) + " (code " + std::to_string((int)e) + "): " + hipGetErrorString(e);
}

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            return fail(_e == hipErrorOutOfMemory ? GPAD_ERR_NOMEM : GPAD_ERR_HIP,           \
                        hip_detail(#expr, _e));                                              \
        }                                                                                    \
    } while (0)

inline size_t esize(int dtype) { return dtype == GPAD_DTYPE_F64 ? sizeof(double) : sizeof(float); }
inline int round4(int x) { return (x + 3) & ~3; }

// A device allocation that only grows.  No freeing destructor: the thread-local gpad_solve and sharded
// caches can outlive the HIP runtime at process exit; owners release explicitly (gpad_destroy).
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int ensure(size_t want) {
        if (want <= bytes && p) return GPAD_OK;
        release();
        if (want == 0) return GPAD_OK;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(e == hipErrorOutOfMemory ? GPAD_ERR_NOMEM : GPAD_ERR_HIP,
                        hip_detail("hipMalloc(" + std::to_string(want) + " bytes)", e));
        }
        bytes = want;
        return GPAD_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

#include "gpad_plant_store.h"  // (uses DevBuf)

// gpad_set_option: one line per option -- its id, its Tuning member and the accepted range.  inverted:
// the member stores 1 - value.  GPAD_OPT_DEFAULT restores the member's Tuning{} value.  Walked by
// gpad_host.cpp set_own_option and by gpad_classes.cpp apply_tuning (a parent's options on a new child).
struct OptionSpec {
    int id;
    int gpad::Tuning::*field;
    int lo, hi;
    bool inverted;
};
inline constexpr int kOptBig = 1 << 30;
inline constexpr OptionSpec kOptions[] = {
    {GPAD_OPT_PHASE_LEN, &gpad::Tuning::phase_len, 0, kOptBig, false},
    {GPAD_OPT_FINISH_THRESH, &gpad::Tuning::finish_thresh, 0, kOptBig, false},
    {GPAD_OPT_PLAN, &gpad::Tuning::plan, 0, 1, false},  // (also drops the handle's plan)
    {GPAD_OPT_PHASED, &gpad::Tuning::phased, 0, 2, false},
    {GPAD_OPT_LPT, &gpad::Tuning::lpt, 0, 1, false},
    {GPAD_OPT_PANEL_MAX_GRID, &gpad::Tuning::panel_max_grid, 0, kOptBig, false},
    {GPAD_OPT_DUO_MAX_GRID, &gpad::Tuning::duo_max_grid, 0, kOptBig, false},
    {GPAD_OPT_FLAT_PANEL_MIN, &gpad::Tuning::flat_panel_min, 0, kOptBig, false},
    {GPAD_OPT_FLAT_PANELS, &gpad::Tuning::flat_panels, 0, 4, false},
    {GPAD_OPT_FLAT_WAVES, &gpad::Tuning::flat_waves, 0, 16, false},  // (0, 8 or 16 only)
    {GPAD_OPT_FLAT_A_LDS, &gpad::Tuning::flat_a_lds, 0, 1, false},
    {GPAD_OPT_DEBUG_DROP_HANDOFF, &gpad::Tuning::debug_drop_handoff, 0, 1, false},
    {GPAD_OPT_P64_RELAY, &gpad::Tuning::p64_no_relay, 0, 1, true},
    {GPAD_OPT_P64_REFILL, &gpad::Tuning::p64_no_refill, 0, 1, true},
    {GPAD_OPT_LOOP_ASYNC, &gpad::Tuning::loop_async, 0, 1, false},
    {GPAD_OPT_LOOP_PANEL, &gpad::Tuning::loop_panel, 0, 1, false},
    {GPAD_OPT_RESTART, &gpad::Tuning::restart, 0, kOptBig, false},  // (changes results: include/gpad.h)
};

// Run status block (gpad_handle_s::status): the device error word, then the per-workgroup maxima
// of |g| from which the host takes gmax.  The maxima are never zeroed by the host: the first writer
// of each solve (the panel pairs' launch at v_begin == 0, or launch_absmax) stores its own slots
// and zeroes the rest, later phase launches of that solve max in (SolveArgs::gmax_part).  A run of
// several solves (gpad_closed_loop with steps > 1) would so keep only its last step's maxima in
// `part`: after each step launch_absmax_fold folds `part` into `acc` (stored at step 0, maxed in
// afterwards) and the host reduces `acc` instead, so the floor covers every (step, instance).  The
// error word is sticky -- zeroed only when the block is created and right after gpad_sync / the
// stats collection copied it out -- so a fault of an asynchronous run still reaches the next sync
// when further runs were queued behind it.
struct RunStatus {
    int err;
    int pad;
    double part[gpad::kAbsmaxMaxBlocks];
    double acc[gpad::kAbsmaxMaxBlocks];  // multi-step runs: slot-wise maxima of `part` over the steps
};

struct gpad_handle_s {
    int device = 0;
    hipStream_t stream = nullptr;
    bool ready = false;
    bool flat = false;   // gpad_setup_flat: the flat battery path (gpad_flat.hip)
    int n_u = 0;
    gpad_dims_t dims{};
    double L = 1.0;
    bool scaled = false;
    int ldn = 0, ldm = 0;
    DevBuf MGt, GLt, frag, stage;
    bool frag_ok = false;      // frag holds the fragment image of the bound matrices
    bool keep_stage = false;   // gpad_solve's cached handle keeps its staging buffer
    // gpad_solve: host copy of the last bound (ML, G, L, dims) so a repeated one-shot call on
    // the same host matrices skips the H2D copy and repack
    std::vector<unsigned char> shadow;
    gpad_dims_t shadow_dims{};
    double shadow_L = 0.0;
    bool shadow_ok = false;
    DevBuf GLx;  // flat path: flat G_L expanded to the full k-major image (flat resident kernel)
    DevBuf Hq;           // gpad_setup_hessian: H, k-major [n][ldn] per matrix (value-function branches)
    bool hess_ok = false;
    double zbound = 0.0;  // gpad_setup_infeasibility: the bound R on |z|_inf (0: none); a class-bound handle keeps
                         // it for the handles its binding makes later
    DevBuf frows;        // ... and r_i = sum_j |G_L[i][j]| per bound matrix, fp64 [copies][ldm] (gpad_farkas.h)
    DevBuf frag64;       // f64 panels (gpad_panel64.hip): -ML | G_L fragment images, shared f64 matrices
    bool frag64_ok = false;
    int frag64_tiles = 0;
    DevBuf hfrag64;      // ... and H's, bound by gpad_setup_hessian (value branches on the f64 panels)
    DevBuf q64;          // f64 panels: the refill queue counter (one int, zeroed per launch); f32: the
                         // asynchronous closed loop's pack queue counter (gpad_loop.hip)
    // f64 panels with refills: the start order of the next solve -- the previous solve's instances by
    // its counts, longest first (SolveArgs::order; GPAD_OPT_LPT), rebuilt whenever counts arrive
    DevBuf p64_order;
    std::vector<int> p64_order_host;
    int p64_order_batch = 0;
    bool p64_order_dirty = false;
    bool last_p64 = false;  // the last run was an f64 panel solve with a tolerance (its counts order the next)
    bool hfrag64_ok = false;
    int frag_tiles = 0;
    DevBuf theta, beta;
    int sched_len = 0, sched_kind = -1, sched_dtype = -1;
    DevBuf work, counters, pwork;
    DevBuf lipwork;      // gpad_lipschitz: the squaring buffers, norm slots and staged operands of one chunk
    std::vector<int> h_counts;
    DevBuf restarts;           // GPAD_OPT_RESTART: restarts per solve of the last run, [steps][batch]
    DevBuf rs_pos;             // ... on the panels: a parked instance's position in the schedule, [batch]
    bool last_restart = false;  // ... which ran with the option on (else gpad_last_restarts reports zeros)
    // run status block on the device (RunStatus above): the error word the kernels report into and
    // the per-workgroup maxima of |g|, the certification floor's data term (include/gpad.h gpad_run)
    DevBuf status;             // RunStatus
    RunStatus h_status;        // ... its host copy for the stats
    double last_tol = 0.0;          // tol of the last run
    double last_floor_scale = 0.0;  // tol_floor = this * max |g| (margin * L * |gscale|)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int last_kernel = 0, last_batch = 0, last_steps = 1;
    // phased panel solves: the plan made from the previous solve (gpad::panel_plan)
    bool last_phased = false;
    int last_N = 0;
    gpad::PanelPlan plan;
    unsigned long long plan_key = 0;    // fingerprint of the counts the plan was built from
    gpad::PanelPlan prior;              // a handle without its own plan: the shape's last plan (plan_prior)
    bool last_prior = false;            // the last run followed `prior`
    gpad::PanelPlan last_phases;        // the phases the last phased panel solve launched (gpad_last_phases)
    int flat_vpred = 0;                 // flat panels: last iteration of the previous phased solve
    // asynchronous runs (no stats): the counts of each phased solve are copied to pinned host
    // memory behind it; the next run re-plans from them once that copy has landed, so a pipeline
    // of back-to-back solves plans from its most recent completed solve without a host sync
    int* plan_pin = nullptr;
    size_t plan_pin_cap = 0;
    hipEvent_t plan_ev = nullptr;
    bool plan_pending = false;
    int plan_pending_N = 0, plan_pending_batch = 0;
    bool plan_pending_p64 = false;      // ... the pending counts are an f64 panel solve's (build_p64_order)
    // plant maps and exogenous signals (gpad_plant_store.h): what gpad_setup_plant[_batch] and gpad_setup_signals
    // bind on this handle -- one copy, or dims.batch -- and the store its runs read: its own, unless a class
    // binding lent it its store (attach_plant below)
    gpad::PlantStore own_plant;
    const gpad::PlantStore* plant = &own_plant;
    int plant_first = 0;                // a run reads copy plant_first of the store ...
    bool plant_all = true;              // ... or every copy: one per instance, or with the class tables attached
                                        // (cloop) one per class.  Without them a handle that sees several copies
                                        // but not dims.batch of them does not run.
    DevBuf state;                       // per-state workspaces (M(x), g(x), x ping-pong, ...)
    int num_cus = 256;
    bool timed = false;
    gpad::Tuning tune;                  // gpad_set_option
    gpad::ClassBinding* cls = nullptr;  // gpad_setup_classes: the class binding (gpad_classes.cpp), which then
                                        // serves the handle's runs; null: none
    const gpad::ClassLoop* cloop = nullptr;  // set by a class binding on its whole-batch handle around one
                                        // gpad_closed_loop call: that call is the fused class loop
    bool failed_run = false;            // the last run's device error was reported (fetch_status
                                        // clears the device word): later stats calls for that
                                        // run keep returning GPAD_ERR_DEVICE until the next run
};

// ---- gpad_host.cpp ----------------------------------------------------------------------------------
int reset_status(gpad_handle_t h, double tol, double floor_scale);
// the last run's counters and status -> *st (synchronises; a device error fails the call)
int collect_stats(gpad_handle_t h, gpad_stats_t* st);
// gpad_setup / gpad_setup_scaled / gpad_setup_flat (and gpad_destroy) end a class binding and free what it held
void end_classes(gpad_handle_t h);
// entry points a class-bound handle does not serve
int no_classes(const char* fn);

// ---- gpad_setup.cpp ---------------------------------------------------------------------------------
int validate_dims(const gpad_dims_t* d);
// a new problem unbinds everything bound to the old one: the class binding, the signals, the Hessian,
// the fragment images' validity, gpad_solve's shadow, and what was planned or predicted from its solves
void unbind_problem(gpad_handle_t h);
int ensure_schedule(gpad_handle_t h, int N, const void* theta_in, const void* beta_in);

// ---- gpad_state.cpp ---------------------------------------------------------------------------------
// Internal (not exported): h's runs read `store` from now on -- copy `first` of it, or (all) every copy.  The store
// must outlive the handle's runs; a class binding lends its own to its children and its whole-batch handle.
void attach_plant(gpad_handle_t h, const gpad::PlantStore* store, int first, bool all);
// the shape rules of GPAD_OPT_LOOP_PANEL for a closed loop of h's problem and plant (the option itself aside):
// what the fused class loop asks of its whole-batch handle
bool loop_panel_shape(gpad_handle_t h, int N, double tol, int nxa);

// ---- gpad_run.cpp -----------------------------------------------------------------------------------
// the counts of a finished solve: the next phased solve's plan / the f64 panels' next start order
void update_plan(gpad_handle_t h, const int* counts, int batch, int N);
void build_p64_order(gpad_handle_t h, const int* counts, int batch);
// The SolveArgs fields every engine reads from the handle alone: matrices and strides, n, m, ldn, ldm,
// batch, N, check_every, tol, tol_gap, L, theta, beta, num_cus, tune, err.  The rest stays zero for
// the caller (launch_solve; gpad_state.cpp's one-launch loop) to set.
template <typename T>
void fill_solve_args(gpad_handle_t h, int N, double tol, gpad::SolveArgs<T>* a);
// Enqueue one fused solve on device buffers (no staging, no sync).  Counters: iters/conv
// [batch] each.  *kernel_out = the family that ran.  restarts: with GPAD_OPT_RESTART on, [batch] of
// Handle::restarts for this solve's restart counts (restart_counts below sizes the buffer for the run).
template <typename T>
int launch_solve(gpad_handle_t h, T* dz, T* dy, const T* dM, const T* dg, int N, double tol, bool scaled_vec,
                 int* iters, int* conv, int* kernel_out, int* restarts = nullptr);
// Before a run of nsolve solves: notes whether GPAD_OPT_RESTART is on (Handle::last_restart) and, when it is,
// sizes Handle::restarts; *out (out nullable) = its base, or null with the option off
int restart_counts(gpad_handle_t h, int nsolve, int** out);
