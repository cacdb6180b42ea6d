// gpad_loop_panel.hip -- the closed loop on the f32 MFMA panels (GPAD_OPT_LOOP_PANEL, gpad_closed_loop):
// one launch in which a panel COLUMN whose solve ends steps to its pack's next MPC solve in place.
//
// The asynchronous loop of gpad_loop.h is the two-slot register-resident kernel: right up to about one
// pack per CU.  For fleets (thousands of packs) the lockstep loop runs the MFMA panels, and pays per
// MPC step its stream operations and, with a tolerance, the whole tail of its slowest pack.  Here the
// workgroup is gpad_panel_kernel<T>'s (gpad_panel.hip): a panel of 16 packs, wave t = row tile t of both
// GEMMs over the fragment images gpad_setup packs, the same MFMA chains (every k-block, ascending,
// the zero-padding blocks included) and the same epilogues and Algorithm-1 test, operation for
// operation -- enforced, not copied: both kernels call gpad_panel.h's panel_gemm, panel_primal and
// panel_dual and gpad_panel_test.h's test.  What differs is the bookkeeping: every column carries its own pack, MPC step and
// iteration count vc, so theta / beta are per lane (theta[vc], beta[vc + 1]: the same table words,
// hence the same bits), and at a test event the columns that finished run the step boundary of
// gpad_loop.h in place -- counters, u = z*[0:nu], x+ = A x + B u, M(x+), g(x+), the u seed -- and go on
// with step t + 1 while their neighbours keep iterating.  After a pack's last step the column writes
// its results and claims the next pack from a queue counter; with none left it goes inactive, and the
// workgroup ends when no column is active.  No workgroup waits for another: every loop is bounded by
// N, by `steps` and by the finite queue.
//
// Events stay workgroup-uniform: with a tolerance the host requires N % check_every == 0, columns
// change step only at events, so every column's vc = v (mod check_every) for the workgroup's
// iteration counter v and the iteration limit falls on an event; with fixed N all columns of a
// workgroup start together and reach N together.
//
// The class loop (gpad_class_loop_fused on a class-bound handle, gpad_classes.cpp) is the same body with
// kCls set: one launch serves every plant class.  Packs are addressed in the class-sorted order, class k
// at positions off[k] .. off[k+1]-1, with one fragment image, one copy of the plant maps and one claim
// counter per class.  A workgroup serves one class kc at a time -- all 16 columns hold packs of kc, the
// two buffer descriptors are kc's -- and where the plain kernel ends (no column active) it looks for
// work in another class: the classes are scanned cyclically from kc + 1, at the first whose counter is
// below its count one lane claims 16 positions with one atomicAdd (positions past the count are empty
// columns), and all columns restart together exactly as at the kernel's start, which is the same
// mechanism on the class the host dealt (LoopArgs::cls_start).  A full cycle with nothing claimed ends
// the workgroup.  The columns restart together, so events stay workgroup-uniform by the argument above,
// and no workgroup waits for another: the scan is bounded by K.  With class signals (la.ns > 0) nothing
// else changes: S is one [steps][batch][ns] array in the sorted order, read at a column's sorted position
// with the whole batch's stride; the per-class map copies are the packed images, rows of nx + ns columns
// at (class * rows + row) * nxa; a restart reloads [x_0; S[0]] of the new columns; an empty column has no
// refill and reads neither x_in nor S.
#include <hip/hip_runtime.h>

#include <cmath>

#include "gpad_farkas.h"
#include "gpad_internal.h"
#include "gpad_panel.h"

namespace gpad {

namespace {

struct LpCol {   // a column at a step boundary, published by wave 0
    int pack;    // the pack whose solve ended (-1: the column is not at a boundary)
    int t;       // its MPC step
    int refill;  // the pack the column takes at step 0 (>= batch: none left), -1: no refill
};

template <int T>
struct __attribute__((aligned(16))) LoopPanelLds {
    float Wl[T * 256];  // [T][64][4] w    (B of GEMM 1)
    float Zh[T * 256];  // [T][64][4] zhat (B of GEMM 2)
    float Gp[T * 256];  // g_P rows of tile t
    float Pd[T * 256];  // p_D rows of tile t
    TestSlot<float> slots[T];
    LpCol col[16];
    float gmw[16];      // per wave: max |g| at the kernel's end
};

constexpr int kLpLdsPerCu = 160 * 1024;
constexpr int kLpTabMax = 32 * 1024;  // (static + dynamic LDS of the T = 16 kernel stay below 128 KiB)

// words of dynamic LDS before the schedule tables: x rows [2][16][nxa], u rows [16][nu]
__host__ __device__ inline int lp_state_words(int nxa, int nu) { return 32 * nxa + 16 * nu; }
// the schedule tables (theta | beta, N + 2 words each) go to LDS when they leave the workgroups of
// a CU resident: 32 / T workgroups for T <= 8, one above (gpad_panel.h panel_resident_grid's figure)
template <int T>
__host__ __device__ inline bool lp_tab_in_lds(int N, int nxa, int nu) {
    const long long tab = 8ll * ((long long)N + 2);
    const int wgs = T <= 8 ? 32 / T : 1;
    return tab <= kLpTabMax &&
           (long long)sizeof(LoopPanelLds<T>) + 4ll * lp_state_words(nxa, nu) + tab <= kLpLdsPerCu / wgs;
}

}  // namespace

#define GPAD_LOOP_PANEL_FK 0
#include "gpad_loop_panel_solve.inc"
#undef GPAD_LOOP_PANEL_FK
#define GPAD_LOOP_PANEL_FK 1
#include "gpad_loop_panel_solve.inc"
#undef GPAD_LOOP_PANEL_FK

// ---- host side --------------------------------------------------------------------------------
bool loop_panel_supported(int n, int m, int nx, int nu) {
    return n >= 1 && m >= 1 && panel_tiles_for(n, m) != 0 && nx >= 1 && nx <= kLoopMaxState && nu >= 1 &&
           nu <= kLoopMaxState && nu <= n;
}

int loop_panel_grid(int n, int m, int batch, int num_cus, const Tuning* tn) {
    const int panels = (batch + 15) / 16;
    const int resident = panel_resident_grid(panel_tiles_for(n, m), num_cus);
    int grid = panels < resident ? panels : resident;
    if (tn && tn->panel_max_grid > 0 && tn->panel_max_grid < grid) grid = tn->panel_max_grid;
    if (grid > kAbsmaxMaxBlocks) grid = kAbsmaxMaxBlocks;
    return grid < 1 ? 1 : grid;
}

template <int T>
static hipError_t launch_loop_panel_t(const LoopArgs& a, int grid, hipStream_t st, const FarkasArgs* fk) {
    const SolveArgs<float>& s = a.s;
    const int nxa = a.nx + a.ns;
    size_t dyn = sizeof(float) * (size_t)lp_state_words(nxa, a.nu);
    if (lp_tab_in_lds<T>(s.N, nxa, a.nu)) dyn += sizeof(float) * 2 * ((size_t)s.N + 2);
    if (fk && s.tol > 0.0) {  // the variant with the infeasibility certificate
        if (a.cls_K)
            hipLaunchKernelGGL((gpad_loop_panel_farkas_kernel<T, true>), dim3(grid), dim3(64 * T), dyn, st, a, fk->R);
        else
            hipLaunchKernelGGL((gpad_loop_panel_farkas_kernel<T, false>), dim3(grid), dim3(64 * T), dyn, st, a, fk->R);
        return hipGetLastError();
    }
    if (a.cls_K) hipLaunchKernelGGL((gpad_loop_panel_kernel<T, true>), dim3(grid), dim3(64 * T), dyn, st, a);
    else hipLaunchKernelGGL((gpad_loop_panel_kernel<T>), dim3(grid), dim3(64 * T), dyn, st, a);
    return hipGetLastError();
}

hipError_t launch_loop_panel(const LoopArgs& a, int grid, hipStream_t st, const FarkasArgs* fk) {
    const SolveArgs<float>& s = a.s;
    const int T = panel_tiles_for(s.n, s.m);
    if (!T || !s.frag || s.frag_tiles != T || s.strideA || s.strideB ||
        !loop_panel_supported(s.n, s.m, a.nx + a.ns, a.nu) || a.nx < 1 || a.ns < 0 || (a.ns && !a.S) || !s.qctr ||
        s.N < 1 || a.steps < 1 || s.batch < 1 || s.check_every < 1 || (s.tol > 0.0 && s.N % s.check_every != 0) ||
        grid < 1 || grid > kAbsmaxMaxBlocks || a.cls_K < 0)
        return hipErrorInvalidValue;
    // the class loop: at most one workgroup per panel of a class (at most batch), the tables given
    if (a.cls_K ? (!a.cls_off || !a.cls_start || grid > s.batch) : grid > (s.batch + 15) / 16)
        return hipErrorInvalidValue;
    switch (T) {
        case 1: return launch_loop_panel_t<1>(a, grid, st, fk);
        case 2: return launch_loop_panel_t<2>(a, grid, st, fk);
        case 3: return launch_loop_panel_t<3>(a, grid, st, fk);
        case 4: return launch_loop_panel_t<4>(a, grid, st, fk);
        case 5: return launch_loop_panel_t<5>(a, grid, st, fk);
        case 6: return launch_loop_panel_t<6>(a, grid, st, fk);
        case 7: return launch_loop_panel_t<7>(a, grid, st, fk);
        case 8: return launch_loop_panel_t<8>(a, grid, st, fk);
        case 9: return launch_loop_panel_t<9>(a, grid, st, fk);
        case 10: return launch_loop_panel_t<10>(a, grid, st, fk);
        case 11: return launch_loop_panel_t<11>(a, grid, st, fk);
        case 12: return launch_loop_panel_t<12>(a, grid, st, fk);
        case 13: return launch_loop_panel_t<13>(a, grid, st, fk);
        case 14: return launch_loop_panel_t<14>(a, grid, st, fk);
        case 15: return launch_loop_panel_t<15>(a, grid, st, fk);
        default: return launch_loop_panel_t<16>(a, grid, st, fk);
    }
}

}  // namespace gpad
