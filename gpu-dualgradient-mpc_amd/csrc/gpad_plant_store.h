// gpad_plant_store.h -- the bound plant maps and exogenous signals, and the only place that knows their layout.
// Host only.  Included by gpad_host.h below DevBuf; gpad_plant_store.cpp is the implementation.
//
// A store holds, on the device,
//   the six maps    PM [n][nx] | M0 [n] | Pg [m][nx] | g0 [m] | A [nx][nx] | B [nx][nu], each array `copies`
//                   times over (M0, g0, A, B only when given);
//   with signals    the packed images [PM SM] | [Pg Sg] | [A E] over rows of nx + ns columns, each
//                   image_copies() = max(copies, signal copies) times over, and M0, g0, B replicated beside them
//                   where the plant holds fewer copies than the signals do -- a reader indexes all six arrays by
//                   one copy index.
// Who owns one: every handle (gpad_setup_plant: one copy; gpad_setup_plant_batch: dims.batch copies, one per
// instance) and every class binding (one copy, or K: one per class).  A handle runs with its own store or with a
// borrowed one (attach_plant, gpad_host.h): the children and the whole-batch handle of a class binding read the
// binding's.  Readers take a view at call time and keep no device pointer across a rebinding: the buffers may move.
#pragma once

namespace gpad {

// The six arrays of one copy range as a run reads them.
template <typename T>
struct PlantView {
    const T *PM, *M0, *Pg, *g0, *A, *B;  // (M0, g0: null when not bound; with signals PM, Pg, A are the images)
    int nxa;                             // columns of a PM / Pg / A row: nx, with signals nx + ns
    int copies;                          // copies behind every pointer
    bool per_copy;                       // a copy per index (LoopArgs::per_plant); else everyone reads the one
};

struct PlantStore {
    int n = 0, m = 0, dtype = -1, nx = 0, nu = 0;
    int copies = 0;      // of the six maps; 0: no plant bound
    bool stacked = false;  // the maps were bound as a stack, a copy per index (of one copy too); else one for all
    bool dyn = false;    // A and B are bound
    bool has_M0 = false, has_g0 = false;
    int ns = 0;          // signal columns; 0: none bound
    int sig_copies = 0;  // copies of SM, Sg, E that were bound
    bool sig_stacked = false;

    bool bound() const { return copies > 0; }
    bool bound_for(const gpad_dims_t& d) const { return bound() && n == d.n && m == d.m && dtype == d.dtype; }
    int image_copies() const { return copies > sig_copies ? copies : sig_copies; }
    // gpad_setup_plant*: checks the arguments (messages under `fn`), uploads every map given from d.memory --
    // stack == 0: one copy for every index, else a stack of that many, one per index -- and synchronises.  A new
    // plant unbinds the signals; a failed rebinding leaves no plant.
    int bind_plant(const char* fn, const gpad_dims_t& d, int stack, int nx, int nu, const void* PM, const void* M0,
                   const void* Pg, const void* g0, const void* A, const void* B, hipStream_t s);
    // gpad_setup_signals / gpad_setup_class_signals: SM [n][ns], Sg [m][ns], E [nx][ns] in `memory`, one copy
    // (stack == 0) or a stack as long as the plant's stack is or would be; a NULL map packs as zeros.  ns == 0
    // unbinds; a failed rebinding leaves none.  Synchronises.
    int bind_signals(int memory, int ns, int stack, const void* SM, const void* Sg, const void* E, hipStream_t s);
    void unbind() { copies = ns = 0; }
    // copy `first` (all == false), or every copy with one per index (all == true); with_sig: over [x; s]
    template <typename T>
    PlantView<T> view(int first, bool all, bool with_sig) const;
    void release() {
        maps.release();
        images.release();
    }

private:
    template <typename T>
    int pack(int memory, int ns, int ncopies, const T* const S[3], DevBuf* up, hipStream_t s);
    DevBuf maps, images;
};

}  // namespace gpad
