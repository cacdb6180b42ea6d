// gpad_classes.h -- the class binding (gpad_setup_classes, include/gpad.h): a fleet of K plant classes
// solved class by class as shared-matrix sub-batches.  Shared by the host runtime (gpad_host.h; the entry points branch
// here at their top), gpad_classes.cpp (the runtime) and gpad_classes.hip (the row permutations).
//
// Not here: classes running concurrently on several streams (they run one after the other on the
// handle's stream; a closed loop can run them as one launch, gpad_class_loop_fused), per-pack true plants
// under a class binding, Hessian branches.  Exogenous signals are here: gpad_setup_class_signals.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/gpad.h"
#include "gpad_internal.h"

namespace gpad {

// ---- gpad_classes.hip: row permutations between the caller's order and the class-sorted order ------
constexpr int kClassMoveArrays = 4;
// One launch moves up to four [batch][len] arrays.  perm[pos] = the caller's instance at sorted
// position pos.  gather: dst[pos][:] = src[perm[pos]][:];  scatter: dst[perm[pos]][:] = src[pos][:].
template <typename T>
struct RowMove {
    const T* src[kClassMoveArrays];
    T* dst[kClassMoveArrays];
    int len[kClassMoveArrays];
    int count;  // arrays in use
};
template <typename T>
hipError_t launch_class_gather(const RowMove<T>& mv, const int* perm, int batch, hipStream_t s);
template <typename T>
hipError_t launch_class_scatter(const RowMove<T>& mv, const int* perm, int batch, hipStream_t s);
// Trajectories: every class wrote its own contiguous [steps][count_k][len] block, class k's at element
// steps * offsets[k] * len of src; dst is the caller's [steps][batch][len].  pos_off[pos] / pos_cnt[pos]:
// offsets[k] and count_k of the class that sorted position pos belongs to.  Up to two arrays (xs, us).
template <typename T>
struct TrajMove {
    const T* src[2];
    T* dst[2];
    int len[2];
    int count;
};
// pos_off == pos_cnt == null: src is one [steps][batch][len] array in the sorted order (the fused class loop)
template <typename T>
hipError_t launch_class_traj_scatter(const TrajMove<T>& mv, const int* perm, const int* pos_off,
                                     const int* pos_cnt, int batch, int steps, hipStream_t s);
// Signals, the inverse: src is the caller's [steps][batch][ns]; dst receives class k's contiguous
// [steps][count_k][ns] block at element steps * offsets[k] * ns, or with pos_off == pos_cnt == null one
// [steps][batch][ns] array in the sorted order (the fused class loop).  steps = 1: gpad_run_state_signals' s.
template <typename T>
hipError_t launch_class_sig_gather(const T* src, T* dst, int ns, const int* perm, const int* pos_off,
                                   const int* pos_cnt, int batch, int steps, hipStream_t s);

// ---- the fused class loop (gpad_class_loop_fused) ---------------------------------------------------
// What one launch of the class-aware panel loop (gpad_loop_panel.hip) needs beyond a plain closed loop of
// the whole batch in the sorted order.  gpad_classes.cpp attaches it to the binding's whole-batch handle
// (gpad_handle_s::cloop) for the length of one gpad_closed_loop call; gpad_state.cpp reads it.  All
// pointers are device memory.  The class tables only: the maps and signal images come from the binding's
// plant store, which that handle runs with (gpad_plant_store.h), a copy per class or one for all.
struct ClassLoop {
    int K, grid;
    const int* off;    // [K + 1] offsets of the sorted order
    const int* start;  // [grid] the class each workgroup starts on (class_loop_deal)
    int* qctr;         // [K] claim counters
    const void* frag;  // K fragment images, class k's at k * 2 * T * T * 1024 bytes
};
// Host only (gpad_class_loop_deal): the class each of `grid` workgroups starts on, in proportion to the
// classes' panel counts; false on a negative count or when every class is empty
bool class_loop_deal(const int* counts, int K, int grid, int* start_class);

// ---- gpad_classes.cpp -------------------------------------------------------------------------------
// Host only: perm / offsets of the class-sorted order (gpad_class_order); false on an id outside 0..K-1
bool class_order(const int* class_of, int batch, int K, int* perm, int* offsets);

// The binding owns one child handle per non-empty class (same device, same stream, shared = 1,
// GPAD_MEM_DEVICE), perm / offsets on host and device, the workspaces, and the one plant store
// (gpad_plant_store.h) whose maps and signal images every one of its handles reads.  Every function returns a
// GPAD_* status with gpad_last_error set.
int classes_setup(ClassBinding** out, int device, hipStream_t stream, const Tuning& tune, const gpad_dims_t* dims,
                  int K, const int* class_of, const void* ML, const void* G, double L);
void classes_free(ClassBinding* cb);
int classes_set_stream(ClassBinding* cb, hipStream_t stream);
int classes_set_option(ClassBinding* cb, int option, int value);
// gpad_class_loop_fused: turns the fused class loop on or off (tune: the parent's options, for the
// whole-batch handle made the first time it is turned on)
int classes_loop_fused(ClassBinding* cb, bool on, const Tuning& tune);
// per_class: every non-NULL map holds K copies (gpad_setup_plant_classes), else one for every class
int classes_setup_plant(ClassBinding* cb, bool per_class, int nx, int nu, const void* PM, const void* M0,
                        const void* Pg, const void* g0, const void* A, const void* B);
int classes_run(ClassBinding* cb, void* z, void* y, const void* M, const void* g, int N, double tol,
                gpad_stats_t* st);
// whether a plant is bound; *dyn (nullable): with A and B
bool classes_has_plant(const ClassBinding* cb, bool* dyn);
// gpad_setup_class_signals (the handle class-bound): SM [n][ns], Sg [m][ns], E [nx][ns], per_class: K copies
// of each; ns == 0 unbinds
int classes_setup_signals(ClassBinding* cb, int ns, bool per_class, const void* SM, const void* Sg, const void* E);
// steps == 0: gpad_run_state; steps >= 1: gpad_closed_loop.  with_sig: the _signals entry points (`where`),
// sg their s [batch][ns] / S [steps][batch][ns] in the caller's order
int classes_state(ClassBinding* cb, void* x, void* z, void* y, const void* sg, bool with_sig, const char* where,
                  int steps, int N, double tol, int warm, void* xs, void* us, gpad_stats_t* st);
// gpad_setup_infeasibility on every class (and the whole-batch handle of the fused loop)
int classes_setup_infeasibility(ClassBinding* cb, double zbound);
// gpad_infeasibility_resident on every class (and the whole-batch handle)
int classes_infeasibility_resident(ClassBinding* cb, int on);
// gpad_infeasibility_loop_async likewise
int classes_infeasibility_loop_async(ClassBinding* cb, int on);
int classes_last_stats(ClassBinding* cb, gpad_stats_t* st);
// gpad_last_restarts of the binding: [steps][batch] in the caller's order; returns the entries written
int classes_last_restarts(ClassBinding* cb, int* restarts, int cap);
int classes_accumulate(ClassBinding* cb, long long* acc);
int classes_sync(ClassBinding* cb);

}  // namespace gpad
