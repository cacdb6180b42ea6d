// gpad_classes.cpp -- the class binding: a fleet made of K plant classes (SKUs, capacity bins, ageing
// bins) on the shared-matrix engines (include/gpad.h gpad_setup_classes).
//
// A fleet bound with dims.shared = 0 carries one matrix pair per pack and has no MFMA engine; a fleet
// of a few pack types needs only K pairs.  The binding composes what exists, as gpad_group.cpp does for
// devices: the parent handle keeps, per non-empty class, one child libgpad handle on the same device
// and the same stream, bound through the public C-ABI with gpad_setup (shared = 1, batch = the class
// size, GPAD_MEM_DEVICE; the caller's dtype, schedule, check_every, kernel and tol_gap).  Every class
// so picks its own engine for its own size -- panel pairs, phased compaction, finisher, the one-launch
// loops -- and no solve kernel knows about classes.
//
// Data path of a call, the same for host and device callers:
//   (host callers) inputs staged to a device workspace in the caller's order
//   gather  : rows -> a class-sorted device workspace, class k's rows one contiguous slice (one launch)
//   solve   : child k works on its slice in place; the children run one after the other on the
//             handle's stream (a loop: class 0's `steps` steps, then class 1's ...).  Classes are
//             independent, so the order changes no result.
//   scatter : sorted rows -> the caller's order (one launch), trajectories from each class's
//             [steps][count_k][len] block (one launch); (host callers) copied out.
// Per-step counts and codes are placed by the host from each child's gpad_last_stats.
//
// The per-instance arithmetic is that of the engines, which is the oracle's whatever the engine, so the
// results are bit for bit those of the shared = 0 binding of the same fleet.
//
// The fused class loop (gpad_class_loop_fused, opt-in) replaces the `solve` stage of a closed loop by ONE
// launch of the class-aware panel loop (gpad_loop_panel.hip) over every class, run through one more handle of
// the whole batch in the sorted order (fused_create, fused_loop); the trajectories are then one
// [steps][batch][len] array in the sorted order and the counts and codes come from that handle.  Every other
// call still pays each class's own tail.
//
// The plant maps and the class signals live once, in the binding's plant store (gpad_plant_store.h): one copy
// of the six maps and of the packed images [PM SM], [Pg Sg], [A E], or one per class.  No handle holds a copy of
// its own: the binding lends the store (lend_plant), copy k to child k and every copy to the whole-batch handle.
//
// Exogenous signals (gpad_setup_class_signals): child k runs the _signals entry points on its own contiguous
// [steps][count_k][ns] block of S, which one more launch gathers from the caller's [steps][batch][ns]
// (launch_class_sig_gather).  The fused loop reads S as one [steps][batch][ns] array in the sorted order.
//
// Not in this file: classes running concurrently on several streams, per-pack true plants under a class
// binding, Hessian branches.
#include <algorithm>
#include <cmath>

#include "gpad_host.h"

namespace gpad {

struct ClassBinding {
    int device = 0;
    hipStream_t stream = nullptr;
    gpad_dims_t dims{};               // the caller's: the whole batch, the caller's memory kind
    int K = 0;
    std::vector<int> perm, offsets;   // class_order
    std::vector<gpad_handle_t> child; // [K]; null for an empty class
    double zbound = 0.0;              // gpad_setup_infeasibility, for the whole-batch handle made later
    int major = 0;                    // the class with the most instances (ties: the lowest): stats kernel
    DevBuf idx;                          // device: perm[batch] | pos_off[batch] | pos_cnt[batch]
    DevBuf sorted, stage;                // class-sorted workspace; host callers' staging in caller order
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    int last_steps = 0;               // solves per instance of the last run (0: no run yet)
    std::vector<int> it, cd;          // one child's counts and codes on their way to the caller
    // the plant maps and class signals (classes_setup_plant, classes_setup_signals): one copy, or one per class.
    // The children and the whole-batch handle read them here (lend_plant)
    PlantStore plant;
    // the fused class loop (gpad_class_loop_fused): every class in one launch of the class-aware panel loop,
    // run through a handle of the whole batch in the sorted order (shared = 1 with the major class's matrices,
    // which the launch never reads: it takes every class's fragment image from `frags`).  That handle owns
    // the run's counters, status block, schedule tables and timing, as any handle does.
    bool fused_on = false;
    gpad_handle_t fused = nullptr;    // made the first time the loop is turned on (f32 only)
    DevBuf mats;                      // f32: the major class's ML | G, kept for that setup
    DevBuf frags;                     // K fragment images copied from the children
    DevBuf ftab;                      // ints: off[K + 1] | qctr[K] | start[kAbsmaxMaxBlocks]
    std::vector<int> start;           // host copy of the start classes dealt for start_grid workgroups
    int start_grid = 0;
    bool last_fused = false;          // the last run was the fused loop: its stats are the fused handle's

    int count(int k) const { return offsets[k + 1] - offsets[k]; }
    const int* d_perm() const { return (const int*)idx.p; }
    const int* d_pos_off() const { return (const int*)idx.p + dims.batch; }
    const int* d_pos_cnt() const { return (const int*)idx.p + 2 * (size_t)dims.batch; }
};

bool class_order(const int* class_of, int batch, int K, int* perm, int* offsets) {
    std::vector<int> cnt((size_t)K + 1, 0);
    for (int b = 0; b < batch; ++b) {
        if (class_of[b] < 0 || class_of[b] >= K) return false;
        ++cnt[(size_t)class_of[b] + 1];
    }
    for (int k = 0; k < K; ++k) cnt[(size_t)k + 1] += cnt[k];
    for (int k = 0; k <= K; ++k) offsets[k] = cnt[k];
    for (int b = 0; b < batch; ++b) perm[cnt[class_of[b]]++] = b;  // ascending b inside a class: stable
    return true;
}

// The class each workgroup of the fused loop starts on.  First one workgroup for every non-empty class, the
// classes with the most panels first (a grid below their number leaves the smallest to be reached by
// switching); then every further workgroup goes where a workgroup has the most panels to serve,
// panels_k / (dealt_k + 1) the largest (ties: the lowest class) -- the shares so follow the panel counts, and
// no class holds more workgroups than panels while another is short.  start_class lists class 0's
// workgroups, then class 1's ...
bool class_loop_deal(const int* counts, int K, int grid, int* start_class) {
    std::vector<long long> panels((size_t)K), dealt((size_t)K, 0);
    std::vector<int> by_size;
    for (int k = 0; k < K; ++k) {
        if (counts[k] < 0) return false;
        panels[k] = ((long long)counts[k] + 15) / 16;
        if (panels[k]) by_size.push_back(k);
    }
    if (by_size.empty()) return false;
    std::stable_sort(by_size.begin(), by_size.end(), [&](int a, int b) { return panels[a] > panels[b]; });
    int left = grid;
    for (size_t i = 0; i < by_size.size() && left > 0; ++i, --left) dealt[by_size[i]] = 1;
    for (; left > 0; --left) {
        int best = by_size[0];
        for (int k : by_size)  // panels_k / (dealt_k + 1) > panels_best / (dealt_best + 1), in integers
            if (panels[k] * (dealt[best] + 1) > panels[best] * (dealt[k] + 1) ||
                (panels[k] * (dealt[best] + 1) == panels[best] * (dealt[k] + 1) && k < best))
                best = k;
        ++dealt[best];
    }
    int w = 0;
    for (int k = 0; k < K; ++k)
        for (long long i = 0; i < dealt[k]; ++i) start_class[w++] = k;
    return true;
}

void classes_free(ClassBinding* cb) {
    if (!cb) return;
    (void)hipSetDevice(cb->device);
    for (gpad_handle_t c : cb->child)
        if (c) (void)gpad_destroy(c);  // (synchronises the stream first)
    if (cb->fused) (void)gpad_destroy(cb->fused);
    cb->plant.release();
    cb->mats.release();
    cb->frags.release();
    cb->ftab.release();
    cb->idx.release();
    cb->sorted.release();
    cb->stage.release();
    if (cb->ev0) (void)hipEventDestroy(cb->ev0);
    if (cb->ev1) (void)hipEventDestroy(cb->ev1);
    delete cb;
}

// the parent's options on a new child (gpad_set_option calls made before the binding)
static int apply_tuning(gpad_handle_t c, const Tuning& t) {
    const Tuning def{};
    for (const OptionSpec& o : kOptions) {  // (a member at its default goes as GPAD_OPT_DEFAULT: -1 is no value)
        const int v = t.*o.field;
        const int rc = gpad_set_option(c, o.id, v == def.*o.field ? GPAD_OPT_DEFAULT : o.inverted ? 1 - v : v);
        if (rc) return rc;
    }
    // (the handle settings that are no options)
    if (const int rc = gpad_infeasibility_resident(c, t.fk_resident)) return rc;
    return gpad_infeasibility_loop_async(c, t.fk_loop_async);
}

static int setup_body(ClassBinding* cb, const Tuning& tune, const void* ML, const void* G, double L) {
    const gpad_dims_t& d = cb->dims;
    const int batch = d.batch, K = cb->K;
    HIP_TRY(hipEventCreate(&cb->ev0));
    HIP_TRY(hipEventCreate(&cb->ev1));
    // perm | pos_off | pos_cnt on the device
    std::vector<int> host_idx(3 * (size_t)batch);
    cb->major = 0;
    for (int k = 0; k < K; ++k) {
        if (cb->count(k) > cb->count(cb->major)) cb->major = k;
        for (int pos = cb->offsets[k]; pos < cb->offsets[k + 1]; ++pos) {
            host_idx[(size_t)batch + pos] = cb->offsets[k];
            host_idx[2 * (size_t)batch + pos] = cb->count(k);
        }
    }
    std::copy(cb->perm.begin(), cb->perm.end(), host_idx.begin());
    int rc = cb->idx.ensure(sizeof(int) * host_idx.size());
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(cb->idx.p, host_idx.data(), sizeof(int) * host_idx.size(), hipMemcpyHostToDevice, cb->stream));
    HIP_TRY(hipStreamSynchronize(cb->stream));
    // the K matrix pairs on the device: the children are GPAD_MEM_DEVICE handles
    const size_t mat = (size_t)d.n * d.m * esize(d.dtype);
    const char* dML = (const char*)ML;
    const char* dG = (const char*)G;
    DevBuf up;
    if (d.memory == GPAD_MEM_HOST) {
        if ((rc = up.ensure(2 * mat * K))) return rc;
        hipError_t e = hipMemcpyAsync(up.p, ML, mat * K, hipMemcpyHostToDevice, cb->stream);
        if (e == hipSuccess) e = hipMemcpyAsync((char*)up.p + mat * K, G, mat * K, hipMemcpyHostToDevice, cb->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(cb->stream);
        if (e != hipSuccess) {
            up.release();
            return fail(GPAD_ERR_HIP, std::string("gpad_setup_classes: matrix upload: ") + hipGetErrorString(e));
        }
        dML = (const char*)up.p;
        dG = dML + mat * K;
    }
    cb->child.assign((size_t)K, nullptr);
    for (int k = 0; k < K && !rc; ++k) {
        if (cb->count(k) == 0) continue;
        gpad_dims_t cd = d;
        cd.batch = cb->count(k);
        cd.shared = 1;
        cd.memory = GPAD_MEM_DEVICE;
        if ((rc = gpad_create(&cb->child[k], cb->device, cb->stream))) break;
        if ((rc = gpad_setup(cb->child[k], &cd, dML + mat * k, dG + mat * k, L))) break;  // (synchronises)
        rc = apply_tuning(cb->child[k], tune);
    }
    if (!rc && d.dtype == GPAD_DTYPE_F32 && !(rc = cb->mats.ensure(2 * mat))) {  // for classes_loop_fused
        hipError_t e = hipMemcpyAsync(cb->mats.p, dML + mat * cb->major, mat, hipMemcpyDeviceToDevice, cb->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync((char*)cb->mats.p + mat, dG + mat * cb->major, mat, hipMemcpyDeviceToDevice, cb->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(cb->stream);
        if (e != hipSuccess) rc = fail(GPAD_ERR_HIP, std::string("gpad_setup_classes: matrix copy: ") + hipGetErrorString(e));
    }
    up.release();
    return rc;
}

int classes_setup(ClassBinding** out, int device, hipStream_t stream, const Tuning& tune, const gpad_dims_t* dims,
                  int K, const int* class_of, const void* ML, const void* G, double L) {
    *out = nullptr;
    if (!dims) return fail(GPAD_ERR_INVALID, "gpad_setup_classes: null dims");
    if (dims->n <= 0 || dims->m <= 0 || dims->batch <= 0)
        return fail(GPAD_ERR_INVALID, "gpad_setup_classes: dims: n, m, batch must be positive");
    if (dims->shared != 1)
        return fail(GPAD_ERR_INVALID, "gpad_setup_classes: dims.shared must be 1 (matrices are shared inside a class)");
    if (dims->dtype != GPAD_DTYPE_F32 && dims->dtype != GPAD_DTYPE_F64)
        return fail(GPAD_ERR_INVALID, "gpad_setup_classes: dims: bad dtype");
    if (dims->memory != GPAD_MEM_HOST && dims->memory != GPAD_MEM_DEVICE)
        return fail(GPAD_ERR_INVALID, "gpad_setup_classes: dims: bad memory kind");
    if (K < 1 || K > dims->batch) return fail(GPAD_ERR_INVALID, "gpad_setup_classes: need 1 <= K <= dims.batch");
    if (!class_of || !ML || !G) return fail(GPAD_ERR_INVALID, "gpad_setup_classes: null argument");
    if (!(L > 0.0) || !std::isfinite(L)) return fail(GPAD_ERR_INVALID, "gpad_setup_classes: L must be > 0");
    ClassBinding* cb = new ClassBinding();
    cb->device = device;
    cb->stream = stream;
    cb->dims = *dims;
    cb->K = K;
    cb->perm.resize((size_t)dims->batch);
    cb->offsets.resize((size_t)K + 1);
    if (!class_order(class_of, dims->batch, K, cb->perm.data(), cb->offsets.data())) {
        classes_free(cb);
        return fail(GPAD_ERR_INVALID, "gpad_setup_classes: class_of holds an id outside 0..K-1");
    }
    const int rc = setup_body(cb, tune, ML, G, L);  // (the rest of dims is validated by the children's gpad_setup)
    if (rc) {
        classes_free(cb);
        return rc;
    }
    *out = cb;
    return GPAD_OK;
}

int classes_set_stream(ClassBinding* cb, hipStream_t stream) {
    for (gpad_handle_t c : cb->child) {
        if (!c) continue;
        const int rc = gpad_set_stream(c, stream);
        if (rc) return rc;
    }
    if (cb->fused)
        if (const int rc = gpad_set_stream(cb->fused, stream)) return rc;
    cb->stream = stream;
    return GPAD_OK;
}

int classes_set_option(ClassBinding* cb, int option, int value) {
    for (gpad_handle_t c : cb->child) {
        if (!c) continue;
        const int rc = gpad_set_option(c, option, value);
        if (rc) return rc;
    }
    if (cb->fused) return gpad_set_option(cb->fused, option, value);  // (GPAD_OPT_PANEL_MAX_GRID caps its grid)
    return GPAD_OK;
}

int classes_infeasibility_resident(ClassBinding* cb, int on) {
    for (gpad_handle_t c : cb->child) {
        if (!c) continue;
        if (const int rc = gpad_infeasibility_resident(c, on)) return rc;
    }
    if (cb->fused) return gpad_infeasibility_resident(cb->fused, on);  // (its loop keeps its own kernel)
    return GPAD_OK;
}

int classes_infeasibility_loop_async(ClassBinding* cb, int on) {
    for (gpad_handle_t c : cb->child) {
        if (!c) continue;
        if (const int rc = gpad_infeasibility_loop_async(c, on)) return rc;
    }
    if (cb->fused) return gpad_infeasibility_loop_async(cb->fused, on);  // (its loop keeps its own kernel)
    return GPAD_OK;
}

// The binding lends its store: child k runs with copy k of the maps and images (or the one copy), the whole-batch
// handle with every copy, a copy per class.  Called after every bind, rebind or unbind and for a new handle.
static void lend_plant(ClassBinding* cb) {
    for (int k = 0; k < cb->K; ++k)
        if (cb->child[k]) attach_plant(cb->child[k], &cb->plant, k, false);
    if (cb->fused) attach_plant(cb->fused, &cb->plant, 0, true);
}

// The whole-batch handle of the fused loop with what its launch reads: the K fragment images (copied from
// the children, which packed them at gpad_setup) and the offsets table.  f64 bindings have none: their
// loops always run class by class.
static int fused_create(ClassBinding* cb, const Tuning& tune) {
    const gpad_dims_t& d = cb->dims;
    if (d.dtype != GPAD_DTYPE_F32) return GPAD_OK;
    gpad_dims_t fd = d;
    fd.shared = 1;
    fd.memory = GPAD_MEM_DEVICE;
    const size_t mat = (size_t)d.n * d.m * sizeof(float);
    gpad_handle_t f = nullptr;
    int rc = gpad_create(&f, cb->device, cb->stream);
    if (!rc) rc = gpad_setup(f, &fd, cb->mats.p, (const char*)cb->mats.p + mat, cb->child[cb->major]->L);
    if (!rc) rc = apply_tuning(f, tune);
    if (!rc && cb->zbound > 0.0) rc = gpad_setup_infeasibility(f, cb->zbound);
    const int K = cb->K;
    const size_t image = f && f->frag_ok && f->frag_tiles >= 1 && f->frag_tiles <= 16
                             ? (size_t)2 * f->frag_tiles * f->frag_tiles * 1024
                             : 0;  // (0: not a shape of the panel loop -- every loop falls back)
    if (!rc && image) rc = cb->frags.ensure(image * K);
    if (!rc) rc = cb->ftab.ensure(sizeof(int) * ((size_t)2 * K + 1 + kAbsmaxMaxBlocks));
    hipError_t e = hipSuccess;
    for (int k = 0; k < K && !rc && image && e == hipSuccess; ++k)
        if (cb->child[k])
            e = hipMemcpyAsync((char*)cb->frags.p + image * k, cb->child[k]->frag.p, image, hipMemcpyDeviceToDevice,
                               cb->stream);
    if (!rc && e == hipSuccess)
        e = hipMemcpyAsync(cb->ftab.p, cb->offsets.data(), sizeof(int) * ((size_t)K + 1), hipMemcpyHostToDevice, cb->stream);
    if (!rc && e == hipSuccess) e = hipStreamSynchronize(cb->stream);
    if (!rc && e != hipSuccess) rc = fail(GPAD_ERR_HIP, std::string("gpad_class_loop_fused: ") + hipGetErrorString(e));
    if (rc) {
        if (f) (void)gpad_destroy(f);
        return rc;
    }
    cb->fused = f;
    cb->start_grid = 0;
    lend_plant(cb);
    return GPAD_OK;
}

int classes_loop_fused(ClassBinding* cb, bool on, const Tuning& tune) {
    if (on && !cb->fused)
        if (const int rc = fused_create(cb, tune)) return rc;
    cb->fused_on = on;
    return GPAD_OK;
}

int classes_setup_plant(ClassBinding* cb, bool per_class, int nx, int nu, const void* PM, const void* M0,
                        const void* Pg, const void* g0, const void* A, const void* B) {
    const int rc = cb->plant.bind_plant(per_class ? "gpad_setup_plant_classes" : "gpad_setup_plant", cb->dims,
                                        per_class ? cb->K : 0, nx, nu, PM, M0, Pg, g0, A, B, cb->stream);
    lend_plant(cb);
    return rc;
}

bool classes_has_plant(const ClassBinding* cb, bool* dyn) {
    if (dyn) *dyn = cb->plant.bound() && cb->plant.dyn;
    return cb->plant.bound();
}

int classes_setup_signals(ClassBinding* cb, int ns, bool per_class, const void* SM, const void* Sg, const void* E) {
    const int rc = cb->plant.bind_signals(cb->dims.memory, ns, per_class ? cb->K : 0, SM, Sg, E, cb->stream);
    lend_plant(cb);
    return rc;
}

int classes_setup_infeasibility(ClassBinding* cb, double zbound) {
    for (gpad_handle_t c : cb->child) {
        if (!c) continue;
        if (const int rc = gpad_setup_infeasibility(c, zbound)) return rc;
    }
    if (cb->fused)  // (the fused loop then runs the certificate variant of the panel loop)
        if (const int rc = gpad_setup_infeasibility(cb->fused, zbound)) return rc;
    cb->zbound = zbound;
    return GPAD_OK;
}

// The stats of the last run from every child (each call synchronises the stream and reports that child's
// device error word); counts and codes placed in the caller's order.  After a fused loop the whole-batch
// handle is the one "child", of every sorted position.
int classes_last_stats(ClassBinding* cb, gpad_stats_t* st) {
    if (cb->last_steps <= 0) return fail(GPAD_ERR_NOT_SETUP, "gpad_last_stats: no run yet");
    const int batch = cb->dims.batch, steps = cb->last_steps;
    st->iterations = 0;
    st->converged = 0;
    st->total_iterations = 0;
    st->kernel = 0;
    st->kernel_ms = 0.0;
    st->tol_floor = 0.0;
    st->flags = 0;
    int first_err = GPAD_OK;
    std::string first_msg;
    for (int k = 0; k < (cb->last_fused ? 1 : cb->K); ++k) {
        const gpad_handle_t c = cb->last_fused ? cb->fused : cb->child[k];
        if (!c) continue;
        const int cnt = cb->last_fused ? batch : cb->count(k), off = cb->last_fused ? 0 : cb->offsets[k];
        gpad_stats_t cs{};
        if (st->iters) {
            cb->it.resize((size_t)steps * cnt);
            cs.iters = cb->it.data();
        }
        if (st->codes) {
            cb->cd.resize((size_t)steps * cnt);
            cs.codes = cb->cd.data();
        }
        const int rc = gpad_last_stats(c, &cs);
        if (rc && rc != GPAD_ERR_DEVICE) return rc;
        if (rc && !first_err) {  // every child is still asked: each reports (and clears) its own word
            first_err = rc;
            first_msg = gpad_last_error();
        }
        st->iterations = std::max(st->iterations, cs.iterations);
        st->converged += cs.converged;
        st->total_iterations += cs.total_iterations;
        if (std::isnan(cs.tol_floor) || cs.tol_floor > st->tol_floor) st->tol_floor = cs.tol_floor;
        st->flags |= cs.flags;
        if (cb->last_fused || k == cb->major) st->kernel = cs.kernel;
        for (int t = 0; t < steps; ++t)
            for (int i = 0; i < cnt; ++i) {
                const size_t to = (size_t)t * batch + cb->perm[(size_t)off + i], from = (size_t)t * cnt + i;
                if (st->iters) st->iters[to] = cb->it[from];
                if (st->codes) st->codes[to] = cb->cd[from];
            }
    }
    float ms = 0.0f;
    if (cb->timed && hipEventElapsedTime(&ms, cb->ev0, cb->ev1) == hipSuccess) st->kernel_ms = ms;
    if (first_err) return fail(first_err, "class binding: " + first_msg);
    return GPAD_OK;
}

// gpad_last_restarts: every child's counts of the last run, placed in the caller's order as the iteration counts
// are (a fused loop never runs with the restart on: its whole-batch handle reports zeros)
int classes_last_restarts(ClassBinding* cb, int* restarts, int cap) {
    const int batch = cb->dims.batch, steps = std::max(cb->last_steps, 1);
    const size_t entries = (size_t)steps * batch;
    std::vector<int> all(entries, 0);
    for (int k = 0; k < cb->K && cb->last_steps > 0 && !cb->last_fused; ++k) {
        const gpad_handle_t c = cb->child[k];
        if (!c) continue;
        const int cnt = cb->count(k), off = cb->offsets[k];
        cb->it.resize((size_t)steps * cnt);
        const int rc = gpad_last_restarts(c, cb->it.data(), steps * cnt);
        if (rc < 0) return rc;
        for (int t = 0; t < steps; ++t)
            for (int i = 0; i < cnt; ++i) all[(size_t)t * batch + cb->perm[(size_t)off + i]] = cb->it[(size_t)t * cnt + i];
    }
    const int k = (int)std::min<size_t>(entries, (size_t)cap);
    std::copy(all.begin(), all.begin() + k, restarts);
    return k;
}

// (the handles that ran last report: the children, or after a fused loop the whole-batch handle)
int classes_sync(ClassBinding* cb) {
    int first_err = GPAD_OK;
    std::string first_msg;
    for (int k = 0; k < (cb->last_fused ? 1 : cb->K); ++k) {
        const gpad_handle_t c = cb->last_fused ? cb->fused : cb->child[k];
        if (!c) continue;
        const int rc = gpad_sync(c);
        if (rc && rc != GPAD_ERR_DEVICE) return rc;
        if (rc && !first_err) {
            first_err = rc;
            first_msg = gpad_last_error();
        }
    }
    if (first_err) return fail(first_err, "class binding: " + first_msg);
    return GPAD_OK;
}

int classes_accumulate(ClassBinding* cb, long long* acc) {
    if (cb->last_steps <= 0) return fail(GPAD_ERR_NOT_SETUP, "gpad_accumulate_iterations: no run yet");
    if (cb->last_fused) return gpad_accumulate_iterations(cb->fused, acc);
    for (gpad_handle_t c : cb->child) {
        if (!c) continue;
        const int rc = gpad_accumulate_iterations(c, acc);
        if (rc) return rc;
    }
    return GPAD_OK;
}

// after the device work of a call is enqueued: stats (synchronous), or a sync for host callers
static int finish_call(ClassBinding* cb, gpad_stats_t* st) {
    if (st) return classes_last_stats(cb, st);
    if (cb->dims.memory == GPAD_MEM_HOST) return classes_sync(cb);
    return GPAD_OK;
}

template <typename T>
static int run_typed(ClassBinding* cb, T* z, T* y, const T* M, const T* g, int N, double tol, gpad_stats_t* st) {
    const gpad_dims_t& d = cb->dims;
    const size_t batch = (size_t)d.batch, zn = batch * d.n, yn = batch * d.m;
    const bool host = d.memory == GPAD_MEM_HOST;
    int rc = cb->sorted.ensure(sizeof(T) * 2 * (zn + yn));
    if (rc) return rc;
    T* sz = (T*)cb->sorted.p;
    T* sy = sz + zn;
    T* sM = sy + yn;
    T* sg = sM + zn;
    T *cz = z, *cy = y;  // the caller-order arrays on the device
    const T *cM = M, *cg = g;
    if (host) {
        if ((rc = cb->stage.ensure(sizeof(T) * 2 * (zn + yn)))) return rc;
        T* b = (T*)cb->stage.p;
        cz = b;
        cy = b + zn;
        T* wM = b + zn + yn;
        T* wg = wM + zn;
        HIP_TRY(hipMemcpyAsync(cz, z, sizeof(T) * zn, hipMemcpyHostToDevice, cb->stream));
        HIP_TRY(hipMemcpyAsync(cy, y, sizeof(T) * yn, hipMemcpyHostToDevice, cb->stream));
        HIP_TRY(hipMemcpyAsync(wM, M, sizeof(T) * zn, hipMemcpyHostToDevice, cb->stream));
        HIP_TRY(hipMemcpyAsync(wg, g, sizeof(T) * yn, hipMemcpyHostToDevice, cb->stream));
        cM = wM;
        cg = wg;
    }
    HIP_TRY(hipEventRecord(cb->ev0, cb->stream));
    RowMove<T> in{};
    in.count = 4;
    const T* isrc[4] = {cz, cy, cM, cg};
    T* idst[4] = {sz, sy, sM, sg};
    const int ilen[4] = {d.n, d.m, d.n, d.m};
    for (int a = 0; a < 4; ++a) {
        in.src[a] = isrc[a];
        in.dst[a] = idst[a];
        in.len[a] = ilen[a];
    }
    HIP_TRY(launch_class_gather<T>(in, cb->d_perm(), d.batch, cb->stream));
    cb->last_steps = 1;
    cb->last_fused = false;
    cb->timed = false;
    for (int k = 0; k < cb->K; ++k) {
        if (!cb->child[k]) continue;
        const size_t off = (size_t)cb->offsets[k];
        if ((rc = gpad_run(cb->child[k], sz + off * d.n, sy + off * d.m, sM + off * d.n, sg + off * d.m, N, tol,
                           nullptr)))
            return rc;
    }
    RowMove<T> out{};
    out.count = 2;
    out.src[0] = sz;
    out.dst[0] = cz;
    out.len[0] = d.n;
    out.src[1] = sy;
    out.dst[1] = cy;
    out.len[1] = d.m;
    HIP_TRY(launch_class_scatter<T>(out, cb->d_perm(), d.batch, cb->stream));
    HIP_TRY(hipEventRecord(cb->ev1, cb->stream));
    cb->timed = true;
    if (host) {
        HIP_TRY(hipMemcpyAsync(z, cz, sizeof(T) * zn, hipMemcpyDeviceToHost, cb->stream));
        HIP_TRY(hipMemcpyAsync(y, cy, sizeof(T) * yn, hipMemcpyDeviceToHost, cb->stream));
    }
    return finish_call(cb, st);
}

int classes_run(ClassBinding* cb, void* z, void* y, const void* M, const void* g, int N, double tol,
                gpad_stats_t* st) {
    if (!z || !y || !M || !g) return fail(GPAD_ERR_INVALID, "gpad_run: null vector");
    if (N < 0) return fail(GPAD_ERR_INVALID, "gpad_run: N < 0");
    if (!(tol <= 0.0) && !std::isfinite(tol)) return fail(GPAD_ERR_INVALID, "gpad_run: bad tol");
    if (cb->dims.dtype == GPAD_DTYPE_F64)
        return run_typed<double>(cb, (double*)z, (double*)y, (const double*)M, (const double*)g, N, tol, st);
    return run_typed<float>(cb, (float*)z, (float*)y, (const float*)M, (const float*)g, N, tol, st);
}

// The fused class loop: gpad_closed_loop of the whole-batch handle on the sorted arrays, with the class tables
// attached for the length of the call.  Grid: loop_panel_grid's rule on the classes' panels,
// min(sum_k ceil(count_k / 16), resident workgroups, kAbsmaxMaxBlocks) capped by GPAD_OPT_PANEL_MAX_GRID.
// sS: the call's signals [steps][batch][ns] in the sorted order (gpad_closed_loop_signals), or null
static int fused_loop(ClassBinding* cb, float* sx, float* sz, float* sy, const float* sS, int steps, int N, double tol,
                      int warm, float* sxs, float* sus) {
    const gpad_dims_t& d = cb->dims;
    const gpad_handle_t f = cb->fused;
    const int K = cb->K;
    std::vector<int> counts((size_t)K);
    long long panels = 0;
    for (int k = 0; k < K; ++k) panels += ((counts[k] = cb->count(k)) + 15) / 16;
    // (a batch of 16 * panels instances has exactly that many panels)
    const int grid = loop_panel_grid(d.n, d.m, (int)std::min<long long>(16 * panels, 0x7ffffff0), f->num_cus, &f->tune);
    int* tab = (int*)cb->ftab.p;  // off[K + 1] | qctr[K] | start[kAbsmaxMaxBlocks]
    if (grid != cb->start_grid) {
        cb->start.resize(kAbsmaxMaxBlocks);  // (never reallocated: a copy may still be reading it)
        if (!class_loop_deal(counts.data(), K, grid, cb->start.data()))
            return fail(GPAD_ERR_INVALID, "gpad_closed_loop: class loop: no workgroups to deal");
        HIP_TRY(hipMemcpyAsync(tab + 2 * (size_t)K + 1, cb->start.data(), sizeof(int) * (size_t)grid,
                               hipMemcpyHostToDevice, cb->stream));
        cb->start_grid = grid;
    }
    ClassLoop cl{};  // (the maps and images: the handle reads the binding's store, lend_plant)
    cl.K = K;
    cl.grid = grid;
    cl.off = tab;
    cl.qctr = tab + K + 1;
    cl.start = tab + 2 * (size_t)K + 1;
    cl.frag = cb->frags.p;
    f->cloop = &cl;
    const int rc = sS ? gpad_closed_loop_signals(f, sx, sz, sy, sS, steps, N, tol, warm, sxs, sus, nullptr)
                      : gpad_closed_loop(f, sx, sz, sy, steps, N, tol, warm, sxs, sus, nullptr);
    f->cloop = nullptr;
    return rc;
}

template <typename T>
static int state_typed(ClassBinding* cb, T* x, T* z, T* y, const T* sg, int steps, int N, double tol, int warm, T* xs,
                       T* us, gpad_stats_t* st) {
    const gpad_dims_t& d = cb->dims;
    const int nx = cb->plant.nx, nu = cb->plant.nu, ns = sg ? cb->plant.ns : 0;
    const bool loop = steps > 0, host = d.memory == GPAD_MEM_HOST;
    // gpad_class_loop_fused: a loop of a shape the panel loop takes runs as one launch over every class; any
    // other call runs class by class as if it were off (as the loop options do)
    // (GPAD_OPT_RESTART on: class by class too, on the lockstep loop -- the panel loop does not carry the restart)
    const bool fused = loop && cb->fused_on && cb->fused && sizeof(T) == sizeof(float) &&
                       cb->fused->tune.restart == 0 &&
                       loop_panel_shape(cb->fused, N, tol, nx + ns);  // (the state and the signals share a row)
    const bool zy_in = !loop || warm;  // a cold loop starts every step from z = y = 0: nothing to bring in
    const size_t batch = (size_t)d.batch, zn = batch * d.n, yn = batch * d.m, xn = batch * nx;
    const size_t xsn = loop && xs ? (size_t)steps * xn : 0, usn = loop && us ? (size_t)steps * batch * nu : 0;
    const size_t sn = (size_t)(loop ? steps : 1) * batch * ns;
    const size_t elems = xn + zn + yn + xsn + usn + sn;
    int rc = cb->sorted.ensure(sizeof(T) * elems);
    if (rc) return rc;
    T* sx = (T*)cb->sorted.p;
    T* sz = sx + xn;
    T* sy = sz + zn;
    T* sxs = xsn ? sy + yn : nullptr;
    T* sus = usn ? sy + yn + xsn : nullptr;
    T* sS = sn ? sy + yn + xsn + usn : nullptr;  // a block per class, or (fused) one array in the sorted order
    const T* cS = sg;
    T *cx = x, *cz = z, *cy = y, *cxs = xs, *cus = us;  // the caller-order arrays on the device
    if (host) {
        if ((rc = cb->stage.ensure(sizeof(T) * elems))) return rc;
        cx = (T*)cb->stage.p;
        cz = cx + xn;
        cy = cz + zn;
        cxs = xsn ? cy + yn : nullptr;
        cus = usn ? cy + yn + xsn : nullptr;
        HIP_TRY(hipMemcpyAsync(cx, x, sizeof(T) * xn, hipMemcpyHostToDevice, cb->stream));
        if (sn) {
            T* up = cy + yn + xsn + usn;
            HIP_TRY(hipMemcpyAsync(up, sg, sizeof(T) * sn, hipMemcpyHostToDevice, cb->stream));
            cS = up;
        }
        if (zy_in) {
            HIP_TRY(hipMemcpyAsync(cz, z, sizeof(T) * zn, hipMemcpyHostToDevice, cb->stream));
            HIP_TRY(hipMemcpyAsync(cy, y, sizeof(T) * yn, hipMemcpyHostToDevice, cb->stream));
        }
    }
    HIP_TRY(hipEventRecord(cb->ev0, cb->stream));
    RowMove<T> in{};
    in.count = zy_in ? 3 : 1;
    in.src[0] = cx;
    in.dst[0] = sx;
    in.len[0] = nx;
    in.src[1] = cz;
    in.dst[1] = sz;
    in.len[1] = d.n;
    in.src[2] = cy;
    in.dst[2] = sy;
    in.len[2] = d.m;
    HIP_TRY(launch_class_gather<T>(in, cb->d_perm(), d.batch, cb->stream));
    if (sn)
        HIP_TRY(launch_class_sig_gather<T>(cS, sS, ns, cb->d_perm(), fused ? nullptr : cb->d_pos_off(),
                                           fused ? nullptr : cb->d_pos_cnt(), d.batch, loop ? steps : 1, cb->stream));
    cb->last_steps = loop ? steps : 1;
    cb->timed = false;
    cb->last_fused = fused;
    if constexpr (sizeof(T) == sizeof(float)) {
        if (fused && (rc = fused_loop(cb, sx, sz, sy, sS, steps, N, tol, warm, sxs, sus))) return rc;
    }
    for (int k = 0; k < cb->K && !fused; ++k) {
        if (!cb->child[k]) continue;
        const size_t off = (size_t)cb->offsets[k];
        T *kx = sx + off * nx, *kz = sz + off * d.n, *ky = sy + off * d.m;
        // class k's trajectories and signals: one contiguous [steps][count_k][len] block each
        T* kxs = sxs ? sxs + (size_t)steps * off * nx : nullptr;
        T* kus = sus ? sus + (size_t)steps * off * nu : nullptr;
        const T* kS = sS ? sS + (size_t)(loop ? steps : 1) * off * ns : nullptr;
        if (loop && kS)
            rc = gpad_closed_loop_signals(cb->child[k], kx, kz, ky, kS, steps, N, tol, warm, kxs, kus, nullptr);
        else if (loop)
            rc = gpad_closed_loop(cb->child[k], kx, kz, ky, steps, N, tol, warm, kxs, kus, nullptr);
        else if (kS)
            rc = gpad_run_state_signals(cb->child[k], kx, kS, kz, ky, N, tol, nullptr);
        else
            rc = gpad_run_state(cb->child[k], kx, kz, ky, N, tol, nullptr);
        if (rc) return rc;
    }
    RowMove<T> out{};
    out.count = 0;
    auto add = [&](const T* src, T* dst, int len) {
        out.src[out.count] = src;
        out.dst[out.count] = dst;
        out.len[out.count] = len;
        ++out.count;
    };
    if (loop) add(sx, cx, nx);  // (gpad_run_state leaves x alone)
    add(sz, cz, d.n);
    add(sy, cy, d.m);
    HIP_TRY(launch_class_scatter<T>(out, cb->d_perm(), d.batch, cb->stream));
    if (xsn || usn) {
        TrajMove<T> tr{};
        tr.count = 0;
        if (xsn) {
            tr.src[tr.count] = sxs;
            tr.dst[tr.count] = cxs;
            tr.len[tr.count++] = nx;
        }
        if (usn) {
            tr.src[tr.count] = sus;
            tr.dst[tr.count] = cus;
            tr.len[tr.count++] = nu;
        }
        // (the fused loop wrote one [steps][batch][len] array in the sorted order, not a block per class)
        HIP_TRY(launch_class_traj_scatter<T>(tr, cb->d_perm(), fused ? nullptr : cb->d_pos_off(),
                                           fused ? nullptr : cb->d_pos_cnt(), d.batch, steps, cb->stream));
    }
    HIP_TRY(hipEventRecord(cb->ev1, cb->stream));
    cb->timed = true;
    if (host) {
        if (loop) HIP_TRY(hipMemcpyAsync(x, cx, sizeof(T) * xn, hipMemcpyDeviceToHost, cb->stream));
        HIP_TRY(hipMemcpyAsync(z, cz, sizeof(T) * zn, hipMemcpyDeviceToHost, cb->stream));
        HIP_TRY(hipMemcpyAsync(y, cy, sizeof(T) * yn, hipMemcpyDeviceToHost, cb->stream));
        if (xsn) HIP_TRY(hipMemcpyAsync(xs, cxs, sizeof(T) * xsn, hipMemcpyDeviceToHost, cb->stream));
        if (usn) HIP_TRY(hipMemcpyAsync(us, cus, sizeof(T) * usn, hipMemcpyDeviceToHost, cb->stream));
    }
    return finish_call(cb, st);
}

int classes_state(ClassBinding* cb, void* x, void* z, void* y, const void* sg, bool with_sig, const char* fn,
                  int steps, int N, double tol, int warm, void* xs, void* us, gpad_stats_t* st) {
    const std::string where(fn);
    if (with_sig && cb->plant.ns == 0) return no_classes(fn);  // (class signals: gpad_setup_class_signals)
    if (!with_sig && cb->plant.ns != 0)  // (dropping a disturbance silently is worse than an error)
        return fail(GPAD_ERR_INVALID, where + ": class signals are bound, call the _signals entry point");
    if (!cb->plant.bound()) return fail(GPAD_ERR_NOT_SETUP, where + ": call gpad_setup_plant after gpad_setup_classes");
    if (steps > 0 && !cb->plant.dyn) return fail(GPAD_ERR_NOT_SETUP, where + ": plant bound without A, B");
    if (!x || !z || !y || (with_sig && !sg)) return fail(GPAD_ERR_INVALID, where + ": null vector");
    if (N < 0 || steps < 0) return fail(GPAD_ERR_INVALID, where + ": N, steps must be >= 0");
    if (!(tol <= 0.0) && !std::isfinite(tol)) return fail(GPAD_ERR_INVALID, where + ": bad tol");
    if (cb->dims.dtype == GPAD_DTYPE_F64)
        return state_typed<double>(cb, (double*)x, (double*)z, (double*)y, (const double*)sg, steps, N, tol, warm,
                                   (double*)xs, (double*)us, st);
    return state_typed<float>(cb, (float*)x, (float*)z, (float*)y, (const float*)sg, steps, N, tol, warm, (float*)xs,
                              (float*)us, st);
}

}  // namespace gpad
