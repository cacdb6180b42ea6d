// gpad_phases.cpp -- the host side of phased panel solves (host only: no kernel lives here).
// A solve with a tolerance is cut into phases; between two phases the survivors are compacted
// (gpad_compact.hip) so that converged instances stop occupying MFMA columns.  This unit holds the
// schedule parameters, the phase planner, the one description of the phase workspace, and the two
// phase loops over it: the shared-matrix panels (plan, per-panel survivor lists, finisher) and the
// flat panels (ping-pong lists, geometric growth).  The kernels they launch are gpad_panel.hip
// (T <= 8), gpad_pairs.hip (T = 9..16), gpad_bigpanel.hip and gpad_flatpanel.hip.
#include <hip/hip_runtime.h>

#include <vector>

#include "gpad_farkas.h"
#include "gpad_internal.h"
#include "gpad_panel.h"  // (panel_tiles_for, panel_resident_grid, panel_handoff_shape)

namespace gpad {

// schedule parameters shared by the launcher and the host's phase hint
int panel_phase_len(int check_every, const Tuning* t) {
    // a multiple of the test period (phases end right after a test); default four tests
    int len = 4 * check_every;
    if (t && t->phase_len > 0) len = t->phase_len;
    return ((len + check_every - 1) / check_every) * check_every;
}

int panel_fin_thresh(int n, int m, int num_cus, const Tuning* t) {
    // the tail of a phased solve (survivors <= 2 per CU) goes to the latency kernel: one
    // instance per workgroup at ~1/6 of a panel's iteration time (when n, m fit it); measured
    // on C4: 2/CU 5.42e8 it/s, 4/CU 5.35e8, 8/CU 5.35e8, no finisher 5.04e8
    int f = resident_supported(n, m) ? 2 * num_cus : 0;
    if (t && t->finish_thresh >= 0 && f) f = t->finish_thresh;
    return f;
}

// ---------------------------------------------------------------------------------------------
// Phase plan from the previous solve of the same handle.
//
// A phased solve's cost is set by where its phase boundaries fall against the survival curve
// s(v) = #(instances still running past iteration v): a phase [v0, v1) costs (v1 - v0) panel
// iterations whose time depends only on how many panels s(v0) fills (columns that converge
// inside the phase idle until it ends), plus the launch, the carry traffic and the seed
// product; handing the survivors to the resident finisher at v costs the longest remaining
// solve at the latency kernel's iteration time, or the remaining instance-iterations at its
// throughput, whichever is larger.  Given s(v) from the previous solve (receding-horizon and
// scenario batches repeat it closely), a dynamic programme over the test-aligned boundaries
// picks the cheapest schedule.  The plan only moves launch boundaries: every column runs the
// same global iterations with the same tests whatever the schedule, so results are bit-identical
// (tests/test_gpu_parity.py::test_panel_phase_plan_reuse_bitexact).
//
// Cost model (us; constants from profiles/r01_timeline.txt and profiles/r01_microbench.jsonl):
//   panel iteration  = (busiest SIMD's MFMA chains) x t_chain,  t_chain = 0.055 (kb1 + kb2) + 0.2
//                      single panels: ceil(T/4) chains, pairs: ceil(2T/4) (2T/4 on the hand-off
//                      shapes, r02_handoff_ab.txt: 8192 at 10.5-10.9 us), T <= 8: co-resident
//                      panels share the CU's four SIMDs
//   phase overhead   = 2 launches (finisher + panel, 5 us each) + one seed iteration
//                      + carried z, y, w, u (16 (n + m) bytes per survivor at 5 TB/s)
//   finisher         = 1.56 t_res L + 0.70 t_res W / CUs + 2 launches,  t_res = 0.0021 (n + m) + 0.38,
//                      L the longest remaining solve, W the remaining instance-iterations (r06 refit:
//                      latency and work add, see PlanModel::finisher).
namespace {
struct PlanModel {
    int T, n, m, num_cus, grid;
    bool handoff;  // gpad_panel2_kernel's hand-off shapes (Handoff)
    bool relay;    // ... and its one-panel relay (T = 9, 13)
    static constexpr double kFinLat = 1.56;     // finisher: us per remaining iteration of the longest, / t_res
    static constexpr double kFinWork = 0.70;    // finisher: us per instance-iteration per CU, / t_res
    static constexpr double kCarryBw = 5e6;     // carried state, bytes per us
    double t_chain, t_res, t_launch = 5.0;
    double iter_time(long long panels) const {
        if (panels <= 0) return 0.0;
        double chains;
        if (T > 8) {
            if (panels <= grid) {
                // the one-panel relay (Handoff): 4 -> 3.36 chains on the busiest SIMD, measured
                // 6.02 -> 5.65-5.75 us per iteration at one CU (r02_relay_ab.txt): priced as 3.5
                chains = relay ? 3.5 : (double)((T + 3) / 4);
            } else {
                const long long pairs = (panels + 1) / 2;
                // the chain hand-off evens the pair layout's SIMD loads (7,7,6,6 -> 6.5 at T = 13)
                const double per = handoff ? 2 * T / 4.0 : (double)((2 * T + 3) / 4);
                chains = (double)((pairs + grid - 1) / grid) * per;
            }
        } else {
            const int per_cu_max = 32 / T;
            const long long rounds = (panels + (long long)grid - 1) / grid;
            const long long last = panels - (rounds - 1) * (long long)grid;
            long long q = (last + num_cus - 1) / num_cus;
            if (rounds > 1 || q > per_cu_max) q = per_cu_max;
            chains = (double)((rounds - 1) * ((per_cu_max * T + 3) / 4) + (q * T + 3) / 4);
        }
        return chains * t_chain;
    }
    double phase(int v0, int v1, long long s0) const {
        const double it = iter_time((s0 + 15) / 16);
        return 2 * t_launch + (v1 - v0 + 1) * it + (double)s0 * 16.0 * (n + m) / kCarryBw;
    }
    double finisher(int longest, long long work) const {
        // r06 refit on fresh-input C4 solves (profiles/r06_plan_refit.txt): with the queue in no
        // useful order (fresh inputs: the previous solve's counts do not rank this one's instances)
        // the longest survivor waits behind part of its CU's queue, so its latency and the CU's
        // share of the work ADD -- the duo took 341-370 us from iteration 280 (L = 110, W/CU = 181)
        // and 236-262 us from 290 (L = 90-100, W/CU = 105), where max(latency, throughput) of the
        // previous constants priced 242 / 171 us and steered ~30 % of the solves to the costlier
        // earlier takeover (+47 us per solve, profiles/r06_solve_spread.txt)
        return 2 * t_launch + kFinLat * t_res * longest + kFinWork * t_res * (double)work / num_cus;
    }
};
}  // namespace

int panel_plan(const int* iters, int batch, int n, int m, int N, int check_every, int num_cus, const Tuning* t,
               PanelPlan* out) {
    out->nph = 0;
    out->N = N;
    const int T = panel_tiles_for(n, m);
    if (!T || batch <= 0 || N <= 0 || (t && !t->plan)) return 0;
    const int K = check_every > 0 ? check_every : 1;
    int maxit = 0;
    for (int b = 0; b < batch; ++b) maxit = iters[b] > maxit ? iters[b] : maxit;
    if (maxit <= 0) return 0;
    maxit = maxit < N ? maxit : N;
    // boundaries: multiples of `step` (a multiple of the test period) up to the last iteration;
    // coarse enough that the plan fits the phase-count slots with room for the run-out phases
    const int slots = kPanelMaxPhases - 4;
    int step = K;
    while ((maxit + step - 1) / step > slots) step += K;
    const int J = (maxit + step - 1) / step;  // boundary j is iteration j*step (J*step >= maxit)
    std::vector<long long> surv(J + 1, 0), work(J + 1, 0);
    std::vector<long long> hist(maxit + 2, 0);
    for (int b = 0; b < batch; ++b) hist[iters[b] < 0 ? 0 : (iters[b] > maxit ? maxit : iters[b])]++;
    // s(v) = #(iters > v), W(v) = sum_b max(0, iters_b - v)
    std::vector<long long> s(maxit + 2, 0), W(maxit + 2, 0);
    for (int v = maxit; v >= 0; --v) {
        s[v] = s[v + 1] + hist[v + 1];
        W[v] = W[v + 1] + s[v];
    }
    for (int j = 0; j <= J; ++j) {
        const int v = j * step < maxit ? j * step : maxit;
        surv[j] = s[v];
        work[j] = W[v];
    }
    PlanModel md;
    md.T = T;
    md.n = n;
    md.m = m;
    md.num_cus = num_cus;
    md.grid = panel_resident_grid(T, num_cus);
    md.handoff = panel_handoff_shape(T, n, m);
    md.relay = md.handoff && (T == 9 || T == 13);
    md.t_chain = 0.055 * ((m + 15) / 16 + (n + 15) / 16) + 0.2;
    md.t_res = 0.0021 * (n + m) + 0.38;
    const bool fin_ok = resident_supported(n, m);
    // best[j]: cheapest finish from boundary j (survivors surv[j] in panels); nxt[j] = next
    // boundary (or -1: finisher takes over at j)
    std::vector<double> best(J + 1, 0.0);
    std::vector<int> nxt(J + 1, J);
    for (int j = J - 1; j >= 0; --j) {
        const int v = j * step;
        double c = 1e300;
        int arg = J;
        if (surv[j] == 0) {
            best[j] = 0.0;
            nxt[j] = J;
            continue;
        }
        if (fin_ok && j > 0) {
            c = md.finisher(maxit - v, work[j]);
            arg = -1;
        }
        for (int k = j + 1; k <= J; ++k) {
            const int v1 = k * step < maxit ? k * step : maxit;
            const double ck = md.phase(v, v1, surv[j]) + best[k];
            if (ck < c) {
                c = ck;
                arg = k;
            }
        }
        best[j] = c;
        nxt[j] = arg;
    }
    // walk the plan: ends of the panel phases, then the takeover (finisher) or run-out phase
    const int fin_default = panel_fin_thresh(n, m, num_cus, t);
    int j = 0, ph = 0;
    while (j < J && ph < slots) {
        const int k = nxt[j];
        if (k < 0) break;  // finisher at boundary j
        // a panel phase: the finisher may still take its list early when the survivors fall to
        // its default threshold -- unless the plan expects several times that many, where its
        // launch would only test and return (~5 us per boundary)
        out->fins[ph] = (j > 0 && surv[j] > 4 * (long long)fin_default) ? 0 : fin_default;
        out->ends[ph++] = k * step;
        j = k;
        if (surv[j] == 0) break;
    }
    // the phase starting at the last boundary runs to N; the finisher takes it when the survivors
    // fit its threshold, sized from the previous solve's survivors there (with margin)
    long long sj = j < J ? surv[j] : 0;
    long long thr = fin_default;
    if (fin_ok && sj > 0 && 2 * sj + 64 > thr) thr = 2 * sj + 64;
    if (thr > batch) thr = batch;
    if (ph > 0 && out->ends[ph - 1] >= N) {
        out->ends[ph - 1] = N;
    } else {
        out->fins[ph] = (int)thr;
        out->ends[ph++] = N;
    }
    out->nph = ph;
    out->cost_us = best[0];
    return ph;
}

// Phase schedule of a phased flat solve: 2K iterations, then a quarter of the iterations done so
// far (rounded to the test period K), so phases stay short while most columns are alive and grow
// geometrically in a long tail (O(log N) launches); past the previous solve's last iteration
// (v_pred) one phase runs to N, so an unused tail costs no empty launches.  Estimated on battery
// tol-mode batches of 8192: column utilisation ~0.9-0.96 vs 0.61-0.70 in one launch.
int flat_phase_len(int v0, int check_every, const Tuning* t) {
    const int K = check_every > 0 ? check_every : 10;
    const int base = (t && t->phase_len > 0) ? t->phase_len : 2 * K;
    const int grow = (v0 / 4) / K * K;
    return grow > base ? grow : base;
}

// ---------------------------------------------------------------------------------------------
// The phase workspace (SolveArgs::pwork), carved in one place for both phase loops:
//   idx ping-pong [2][batch] | phase counts [kPanelMaxPhases] | finisher queue counters
//   [kPanelMaxPhases] | carried w, u [batch][m] each | per-panel survivor lists: seg_idx [batch + 32],
//   seg_cnt [batch / 16 + 2] (list_survivors)
// The flat panels use the idx lists, the counts and the carried state only.  The host reads the
// counts back at int offset 2 * batch (gpad_host.cpp gpad_last_phases / gpad_phase_counts).
// ---------------------------------------------------------------------------------------------
namespace {
struct PhaseWork {
    int *idx0, *idx1, *counts, *qctrs;
    float *wc, *uc;
    int *seg_idx, *seg_cnt;
    size_t bytes;
};

// base null: only .bytes means something (panel_work_bytes)
PhaseWork phase_work(void* base, int m, int batch) {
    static_assert(sizeof(int) == 4 && sizeof(float) == 4, "the workspace is carved in 4-byte words");
    const size_t B = (size_t)batch, carried = B * (size_t)m;
    size_t words = 0;
    auto take = [&](size_t count) -> void* {  // the next `count` words
        void* p = base ? static_cast<char*>(base) + 4 * words : nullptr;
        words += count;
        return p;
    };
    PhaseWork w;
    w.idx0 = static_cast<int*>(take(B));
    w.idx1 = static_cast<int*>(take(B));
    w.counts = static_cast<int*>(take(kPanelMaxPhases));
    w.qctrs = static_cast<int*>(take(kPanelMaxPhases));
    w.wc = static_cast<float*>(take(carried));
    w.uc = static_cast<float*>(take(carried));
    w.seg_idx = static_cast<int*>(take(B + 32));
    w.seg_cnt = static_cast<int*>(take(B / 16 + 2));
    w.bytes = 4 * words;
    return w;
}
}  // namespace

size_t panel_work_bytes(int m, int batch) { return phase_work(nullptr, m, batch).bytes; }

// ---------------------------------------------------------------------------------------------
// Phase loop of the shared-matrix panels.  T = panel_tiles_for(n, m), or 0 for the big panels; it
// decides the resident grid, who zeroes the counters, and which kernel a phase launches.
// ---------------------------------------------------------------------------------------------
static hipError_t launch_panel_phase(int T, const SolveArgs<float>& a, int grid, hipStream_t s,
                                     const FarkasArgs* fk, const RestartArgs* rs) {
    if (fk || rs) return launch_panel_single(T, a, grid, s, fk, rs);  // the T-wave kernel at every T it has
    if (T == 0) {  // (its status was never looked at: the launch's own error is what counts)
        (void)launch_bigpanel(a, grid, s);
        return hipGetLastError();
    }
    return T > 8 ? launch_panel_pairs(T, a, grid, s) : launch_panel_single(T, a, grid, s);
}

// fk: the infeasibility certificate (launch_panel): the T-wave kernel's variant, no finisher; rs: the adaptive
// restart, likewise (`tw`: either)
static hipError_t launch_panel_phases(int T, SolveArgs<float> a, hipStream_t s, const FarkasArgs* fk,
                                      const RestartArgs* rs) {
    const bool tw = fk || rs;
    // Grid = resident workgroups (panel_resident_grid).  Workgroups walk their panels grid-stride.
    const int panels = (a.batch + 15) / 16;
    const int resident = tw && T > 8 ? 2 * a.num_cus : panel_resident_grid(T, a.num_cus);
    int grid = panels < resident ? panels : resident;
    const Tuning tn = a.tune ? *a.tune : Tuning{};
    if (tn.panel_max_grid > 0 && tn.panel_max_grid < grid) grid = tn.panel_max_grid;  // grid-stride panels
    const bool phased = a.tol > 0.0 && a.pwork != nullptr && tn.phased;
    a.fin_thresh = phased && !tw ? panel_fin_thresh(a.n, a.m, a.num_cus, &tn) : 0;
    if (!phased) {  // fixed N (or no workspace): one phase, nothing carried
        a.v_begin = 0;
        a.v_end = a.N;
        a.idx_in = nullptr;
        a.count_in = nullptr;
        return launch_panel_phase(T, a, grid, s, fk, rs);
    }
    // survivors listed per panel, densified at each boundary by phase_compact_kernel (one idx
    // list suffices: phase ph reads idx0 while it lists into seg_idx)
    const PhaseWork w = phase_work(a.pwork, a.m, a.batch);
    a.wc = w.wc;
    a.uc = w.uc;
    a.seg_idx = w.seg_idx;
    a.seg_cnt = w.seg_cnt;
    a.idx_out = nullptr;
    a.count_out = nullptr;
    // the phase counters and the finisher's queue counters: zeroed by the first launch's workgroup 0
    // (panel pairs), else one memset
    hipError_t e = hipSuccess;
    if (T > 8 && !tw) {
        a.zero_w = w.counts;
        a.zero_n = 2 * kPanelMaxPhases;
    } else if ((e = hipMemsetAsync(w.counts, 0, sizeof(int) * 2 * kPanelMaxPhases, s)) != hipSuccess) {
        return e;
    }
    // phase length: a multiple of the test period (phases end right after a test); default
    // four tests, doubling after 10 phases so a long tail costs O(log N) launches (a phase with
    // no survivors left costs one empty launch, ~5 us)
    const int len = panel_phase_len(a.check_every, &tn);
    const PanelPlan* plan = (a.plan && a.plan->nph > 0 && a.plan->N == a.N) ? a.plan : nullptr;
    if (a.used) {
        a.used->nph = 0;
        a.used->N = a.N;
        a.used->cost_us = plan ? plan->cost_us : 0.0;
    }
    const int fin_default = a.fin_thresh;
    int fin_prev = 0;  // the previous phase's finisher threshold
    int v0 = 0;
    for (int ph = 0; v0 < a.N; ++ph) {
        int plen = len;
        if (ph >= 10 && tn.phase_len <= 0) plen = len << (ph - 9 < 20 ? ph - 9 : 20);  // explicit: uniform
        a.fin_thresh = fin_default;
        if (plan && ph < plan->nph) {  // the previous solve's plan (panel_plan)
            plen = plan->ends[ph] - v0;
            if (ph && fin_default) a.fin_thresh = plan->fins[ph];
        }
        if (plen < 1) plen = len;
        if (ph >= kPanelMaxPhases - 1) plen = a.N;  // last slot: run to N
        const int v1 = (a.N - v0 <= plen) ? a.N : v0 + plen;
        a.v_begin = v0;
        a.v_end = v1;
        a.idx_in = ph ? w.idx0 : nullptr;
        a.count_in = ph ? w.counts + ph - 1 : nullptr;
        if (ph) {  // the boundary: phase ph-1's per-panel lists -> idx0 (LPT-ordered for the finisher)
            e = launch_phase_compact(a.seg_cnt, a.seg_idx, ph >= 2 ? w.counts + ph - 2 : nullptr, a.batch, fin_prev,
                                     w.idx0, w.counts + ph - 1, (a.pred && tn.lpt) ? a.pred : nullptr, a.fin_thresh, s);
            if (e != hipSuccess) return e;
        }
        fin_prev = a.fin_thresh;
        if (a.used && ph < kPanelMaxPhases) {  // (diagnostics: gpad_last_phases)
            a.used->ends[ph] = v1;
            a.used->fins[ph] = ph ? a.fin_thresh : 0;
            a.used->nph = ph + 1;
        }
        if (ph && a.fin_thresh) {  // few survivors left: the duo finisher takes them, runs to N --
            // two instances per CU in ping-pong, fed from the survivor list
            a.qctr = w.qctrs + ph;
            int g = a.fin_thresh < a.num_cus ? a.fin_thresh : a.num_cus;
            if (tn.duo_max_grid > 0 && tn.duo_max_grid < g) g = tn.duo_max_grid;  // more claims
            if ((e = launch_duo(a, g, s)) != hipSuccess) return e;
        }
        if ((e = launch_panel_phase(T, a, grid, s, fk, rs)) != hipSuccess) return e;
        a.zero_w = nullptr;
        v0 = v1;
    }
    return hipSuccess;
}

bool panel_folds_gmax(int n, int m) { return panel_tiles_for(n, m) > 8; }

hipError_t launch_panel(const SolveArgs<float>& a, hipStream_t s, bool* supported, const FarkasArgs* fk,
                        const RestartArgs* rs) {
    const int T = panel_tiles_for(a.n, a.m);  // 0: big panels
    if ((fk || rs) && T < 1) {  // (the big panels do not carry it)
        *supported = false;
        return hipSuccess;
    }
    // the fragment image must have been packed for this geometry at setup
    *supported = a.frag != nullptr && a.strideA == 0 && a.strideB == 0 &&
                 (T ? a.frag_tiles == T
                    : bigpanel_supported(a.n, a.m) && a.frag_tiles == panel_tiles(a.n, a.m, a.batch));
    return *supported ? launch_panel_phases(T, a, s, fk, rs) : hipSuccess;
}

// ---------------------------------------------------------------------------------------------
// Phase loop of the flat panels (gpad_flatpanel.hip): survivors appended to ping-pong lists by the
// kernel itself, phases of flat_phase_len iterations, no finisher.
// ---------------------------------------------------------------------------------------------
hipError_t launch_flatpanel(const SolveArgs<float>& a0, hipStream_t s) {
    if (!flatpanel_supported(a0.n, a0.m, a0.n_u) || !a0.frag) return hipErrorInvalidValue;
    SolveArgs<float> a = a0;
    const Tuning tn = a.tune ? *a.tune : Tuning{};
    a.v_begin = 0;
    a.v_end = a.N;
    a.idx_in = nullptr;
    a.count_in = nullptr;
    // phases pay when the batch is several resident rounds of groups (the time of a resident round
    // is its slowest column either way; compaction shortens the queue of rounds): measured on
    // battery packs, eps mode, phased vs one launch -- C1 8192: 1.91 vs 1.63 ms, 65536: 8.8 vs
    // 10.0 ms; N = 50 4096: 25.1 vs 23.9 ms, 16384: 67.7 vs 87.2 ms (profiles/r02_flat_phased.txt).
    // GPAD_OPT_PHASED: 0 never, 1 (default) from 4 panels per CU, 2 always.
    const int panels = (a.batch + 15) / 16;
    const bool phased = a.tol > 0.0 && a.pwork != nullptr &&
                        (tn.phased == 2 || (tn.phased == 1 && panels >= 4 * a.num_cus));
    if (!phased) return launch_flatpanel_once(a, s);
    const PhaseWork w = phase_work(a.pwork, a.m, a.batch);
    a.wc = w.wc;
    a.uc = w.uc;
    hipError_t e = hipMemsetAsync(w.counts, 0, sizeof(int) * kPanelMaxPhases, s);
    if (e != hipSuccess) return e;
    int v0 = 0;
    for (int ph = 0; v0 < a.N; ++ph) {
        int plen = ph >= kPanelMaxPhases - 1 ? a.N : flat_phase_len(v0, a.check_every, &tn);
        if (a0.v_pred > 0 && v0 >= a0.v_pred) plen = a.N;  // beyond the prediction: one last phase
        const int v1 = (a.N - v0 <= plen) ? a.N : v0 + plen;
        a.v_begin = v0;
        a.v_end = v1;
        a.idx_in = ph ? ((ph & 1) ? w.idx0 : w.idx1) : nullptr;
        a.count_in = ph ? w.counts + ph - 1 : nullptr;
        a.idx_out = (ph & 1) ? w.idx1 : w.idx0;
        a.count_out = w.counts + ph;
        if ((e = launch_flatpanel_once(a, s)) != hipSuccess) return e;
        v0 = v1;
    }
    return hipSuccess;
}

}  // namespace gpad
