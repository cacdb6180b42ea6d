/*
 * gpad.h -- C-ABI of the MI355X-native GPAD solver (libgpad.so).
 *
 * GPAD = accelerated dual gradient-projection for the condensed linear-MPC QP
 *     min 1/2 z'Hz + q'z   s.t.  G z <= g
 * (Bemporad & Patrinos, NMPC'12, eq. 8; reference Code/MATLAB/acceldualgrad.m).
 *
 * Plain C: pointers, sizes and status codes only; no C++ or torch types cross this boundary.
 * Every entry point names the reference interface it replaces (file:line, relative to
 * /root/reference).  Reference-side bindings (C/CUDA driver, ctypes) are in INTEGRATION.md.
 *
 * Conventions
 *   - Matrices are row-major in their mathematical orientation: ML is n x m, G is m x n.
 *   - Batches pack per-instance vectors contiguously: z [batch][n], y/g [batch][m], M [batch][n];
 *     per-instance matrices (dims.shared == 0) are packed [batch][n][m] / [batch][m][n].
 *   - dims.dtype selects float (GPAD_DTYPE_F32) or double (GPAD_DTYPE_F64) for EVERY pointer.
 *   - dims.memory says whether the caller's pointers are host or device (HIP) memory.
 *   - Status: 0 = OK, < 0 = error (gpad_strerror()).  No exceptions cross the ABI.
 *   - Thread safety: distinct handles may be used concurrently; one handle is not reentrant.
 */
#ifndef GPAD_H
#define GPAD_H

#ifdef __cplusplus
extern "C" {
#endif

#define GPAD_VERSION_MAJOR 0
#define GPAD_VERSION_MINOR 6 /* 0.3: gpad_stats_t gained tol_floor / flags, gpad_dims_t an explicit reserved
                              * word (layouts changed: rebuild callers against this header);
                              * 0.4: the condensed operator (kernel 5, option 14) removed, the device
                              * error word sticky until reported; layouts as in 0.3;
                              * 0.5: options 20, 21 removed; layouts as in 0.3;
                              * 0.6: gpad_setup_plant_batch added; layouts as in 0.3.  Added since
                              * without a new minor (no layout or behaviour of 0.6 changes):
                              * gpad_setup_signals, gpad_run_state_signals, gpad_closed_loop_signals;
                              * GPAD_OPT_LOOP_PANEL (option 23) and the reported GPAD_KERNEL_LOOP_PANEL (7);
                              * gpad_class_order, gpad_setup_classes, gpad_setup_plant_classes;
                              * gpad_class_loop_fused, gpad_class_loop_deal and the reported
                              * GPAD_KERNEL_LOOP_CLASSES (8); gpad_setup_class_signals;
                              * gpad_setup_infeasibility, gpad_farkas_margin and the termination code
                              * GPAD_CODE_INFEASIBLE (5), returned only with a bound in force;
                              * gpad_infeasibility_resident and gpad_infeasibility_loop_async (off by
                              * default: no routing changes); gpad_lipschitz, gpad_lipschitz_host;
                              * GPAD_OPT_RESTART (option 24, off by default) and gpad_last_restarts */

/* status codes */
#define GPAD_OK 0
#define GPAD_ERR_INVALID (-1)      /* bad argument / inconsistent dims                  */
#define GPAD_ERR_HIP (-2)          /* HIP runtime error (gpad_last_error() has details) */
#define GPAD_ERR_NOMEM (-3)        /* device allocation failed                          */
#define GPAD_ERR_UNSUPPORTED (-4)  /* shape/kernel combination not supported            */
#define GPAD_ERR_NOT_SETUP (-5)    /* gpad_run before gpad_setup                        */
#define GPAD_ERR_NO_DEVICE (-6)    /* no HIP device visible                             */
#define GPAD_ERR_DEVICE (-7)       /* a kernel reported a failure on the device (e.g. a chain
                                    * hand-off that never arrived): the run's z, y are invalid.
                                    * Returned by the call that collects the run's stats or
                                    * synchronises it (gpad_run with st, gpad_last_stats,
                                    * gpad_sync, host-memory runs) -- never GPAD_OK; the error
                                    * is kept on the device until one of those reports it, so
                                    * asynchronous runs queued behind a failed one do not
                                    * hide it, and once reported every later sync / stats call
                                    * on the handle returns it again until the next run starts */

/* theta/beta schedule (acceldualgrad.m:18,27,55-56 vs paper eq. 8e) */
#define GPAD_SCHEDULE_MATLAB 0 /* beta lagged one iteration, as the reference's MATLAB  */
#define GPAD_SCHEDULE_PAPER 1  /* beta_v = theta_v (1/theta_{v-1} - 1)                   */

#define GPAD_MEM_HOST 0
#define GPAD_MEM_DEVICE 1

#define GPAD_DTYPE_F32 0
#define GPAD_DTYPE_F64 1

/* kernel families (GPAD_KERNEL_AUTO picks; the others force one, for tests and benches) */
#define GPAD_KERNEL_AUTO 0
#define GPAD_KERNEL_STREAM 1   /* matrices streamed (k-major) from HBM/L2; one workgroup/instance */
#define GPAD_KERNEL_RESIDENT 2 /* matrix rows held in VGPRs; one workgroup/instance; n,m <= 208  */
#define GPAD_KERNEL_PANEL 3    /* shared ML/G, f32 MFMA 16x16x4 panels; one wave per 16 instances */
#define GPAD_KERNEL_FLAT 4     /* reported only: the flat battery path bound by gpad_setup_flat      */
/* 5: the opt-in condensed operator (not the reference's arithmetic), removed in 0.4; dims.kernel = 5
 * returns GPAD_ERR_INVALID */
#define GPAD_KERNEL_LOOP 6     /* reported only: gpad_closed_loop in one launch (GPAD_OPT_LOOP_ASYNC);
                                * dims.kernel = 6 returns GPAD_ERR_INVALID                           */
#define GPAD_KERNEL_LOOP_PANEL 7 /* reported only: gpad_closed_loop in one launch on the MFMA panels
                                * (GPAD_OPT_LOOP_PANEL); dims.kernel = 7 returns GPAD_ERR_INVALID     */
#define GPAD_KERNEL_LOOP_CLASSES 8 /* reported only: gpad_closed_loop of a class-bound handle as one launch
                                * over every class (gpad_class_loop_fused); dims.kernel = 8 returns
                                * GPAD_ERR_INVALID                                                   */

typedef struct gpad_dims {
    int n;           /* primal variables, n = n_u * N                                   */
    int m;           /* inequality constraints (battery: m = 4 n_u N + 2 N)             */
    int batch;       /* independent instances, >= 1                                     */
    int shared;      /* 1: ML, G shared by every instance; 0: per-instance matrices     */
    int dtype;       /* GPAD_DTYPE_*                                                    */
    int memory;      /* GPAD_MEM_*: where the caller's pointers live                    */
    int schedule;    /* GPAD_SCHEDULE_*                                                 */
    int check_every; /* termination test period K when tol > 0 (<= 0 -> 10)            */
    int kernel;      /* GPAD_KERNEL_*                                                   */
    int reserved;    /* must be 0 (explicit padding before tol_gap; reserved for extensions) */
    double tol_gap;  /* e_V of acceldualgrad.m:13: tolerance of test (B)'s duality-gap term
                      * -w'(G zhat - g); <= 0 (e.g. a zeroed struct): the run's tol (= e_g) */
} gpad_dims_t;

typedef struct gpad_stats {
    int iterations;              /* max iterations over the batch                       */
    int converged;               /* instances that met tol (0 when tol <= 0)            */
    long long total_iterations;  /* sum of per-instance iterations                      */
    int kernel;                  /* GPAD_KERNEL_* that ran                               */
    double kernel_ms;            /* device time of the solve launch (HIP events)        */
    int* iters;                  /* optional caller array (host) or NULL: [batch]; gpad_closed_loop:
                                  * [steps][batch]                                        */
    double tol_floor;            /* tol > 0: the certification floor of this run's data, see
                                  * gpad_run (0 when tol <= 0)                             */
    int flags;                   /* GPAD_FLAG_* of the run                                  */
    int* codes;                  /* optional caller array (host) or NULL, sized as iters:
                                  * [batch]; gpad_closed_loop: [steps][batch].  Per-instance
                                  * termination code, 0 = ran to N, 1..4 = the test that
                                  * stopped it (gpad_run), 5 = GPAD_CODE_INFEASIBLE
                                  * (gpad_setup_infeasibility)                               */
} gpad_stats_t;

/* gpad_stats_t.flags */
#define GPAD_FLAG_TOL_FLOOR 1 /* 0 < tol < tol_floor: no instance with an active constraint can be
                               * certified; expect converged == 0 (use f64 or a larger tol)   */
#define GPAD_FLAG_NONFINITE_G 2 /* tol > 0 and g holds a NaN or an infinity: tol_floor is not
                                 * finite (NaN when g has a NaN) and TOL_FLOOR is set too; the
                                 * instance holding it is never reported converged, every
                                 * other instance is solved as if it were not there           */

typedef struct gpad_handle_s* gpad_handle_t;

const char* gpad_version(void);
/* HIP devices visible to this process (>= 0), or a negative GPAD_ERR_* status; the device list
 * of gpad_group_create / gpad_solve_sharded (main.cu picks device 0, :116) */
int gpad_device_count(void);
const char* gpad_strerror(int status);
/* thread-local detail of the last failure; HIP runtime failures carry the HIP status name and
 * number ("hipErrorNoDevice (code 100): ...") */
const char* gpad_last_error(void);

/* Handle bound to one device and one HIP stream; every launch and copy of the handle is
 * ordered on that stream.  NULL = the device's default (null) stream, as in every HIP API.
 * Replaces the implicit device/default-stream state of main.cu:116-147. */
int gpad_create(gpad_handle_t* h, int device, void* hip_stream);
int gpad_destroy(gpad_handle_t h);
int gpad_set_stream(gpad_handle_t h, void* hip_stream);

/* Bind the problem shape and the (constant) matrices: ML = H^-1 G' and G, with Lipschitz L.
 * Packs them into the device layouts the kernels read (MGneg = -ML and G_L = G/L,
 * acceldualgrad.m:20-22).  Replaces the off-line precompute + H2D copy of main.cu:29-67,
 * 126-147.  Reusable across many gpad_run calls (an LTI plant has constant ML/G). */
int gpad_setup(gpad_handle_t h, const gpad_dims_t* dims, const void* ML, const void* G, double L);

/* Same, for the reference's data-file boundary (main.cu:29-67): MGneg holds -H^-1 G'
 * (sign-folded as the file does) and GL = G/L already; L only scales tol. */
int gpad_setup_scaled(gpad_handle_t h, const gpad_dims_t* dims, const void* MGneg, const void* GL,
                      double L);

/* The reference's "flat" battery data (ENABLE_FLATTEN_MATRICES, main.cu:39-56; valid for equal
 * cell capacities): MGf is the N x m flat sign-folded M_G, GLf the m x N flat G_L (row-major as
 * seq_functions.cpp:5-43 index them), n = dims.n = n_u N, m = dims.m >= 4 n_u N.  Subsequent
 * gpad_run / gpad_run_scaled use the structure-exploiting kernel with the arithmetic of
 * StepTwoGPADFlatSequential / StepFourGPADFlatSequential (f32, shared matrices only). */
int gpad_setup_flat(gpad_handle_t h, const gpad_dims_t* dims, int n_u, const float* MGf,
                    const float* GLf, double L);

/* Bind the QP Hessian H (n x n row-major; dims.shared: one for the batch, else [batch][n][n];
 * dims.dtype / dims.memory of the bound problem; symmetric positive definite) and so enable the
 * value-function branches of Algorithm 1 (acceldualgrad.m:30-33,73,76) in later gpad_run /
 * gpad_run_state calls with tol > 0.  The QP is then min 1/2 z'Hz + f'z, G z <= g with f = H M
 * (M = H^-1 f is the vector gpad_run takes).  Which kernel evaluates the value functions:
 *   f64, shared matrices, n, m <= 256: the f64 MFMA panels (gpad_panel64.hip) when forced
 *     (GPAD_KERNEL_PANEL) or under AUTO from 16 instances per CU on (gpad_host.cpp, the f64
 *     panel branch of gpad_run); bit-identical to the f64 stream kernel, codes 3 / 4 included;
 *   otherwise (f32, f64 below that batch, distinct matrices, larger n or m): the stream kernel.
 * The f32 panel and the latency (resident / duo / flat) kernels do not evaluate the value
 * functions: with H bound, forcing GPAD_KERNEL_RESIDENT, or GPAD_KERNEL_PANEL where the f64
 * panels do not apply (f32, distinct matrices, n or m > 256), returns GPAD_ERR_UNSUPPORTED.
 * H = NULL unbinds.  gpad_setup / gpad_setup_scaled unbind as well.
 * Replaces acceldualgrad.m's own H (the MATLAB function receives H, :1). */
int gpad_setup_hessian(gpad_handle_t h, const void* H);

/* ---- infeasibility certificates ------------------------------------------------------------------
 * An infeasible QP (no z with G z <= g) never meets Algorithm 1: max(G z - g) stalls at a positive
 * constant, |y| grows without bound and the solve runs to N and returns code 0, which a caller cannot
 * tell from a slow one.  The dual iterate is its own Farkas certificate: for y >= 0 and any z with
 * |z|_inf <= R,  y'(G z - g) >= -(g'y) - R |G'y|_1,  so  g'y + R |G'y|_1 < 0  proves that no z of the box
 * satisfies G z <= g.  G'y stays bounded while -g'y grows, so on an infeasible QP the test passes eventually.
 *
 * gpad_setup_infeasibility binds R = zbound > 0, the caller's bound on |z|_inf over the feasible set (the
 * battery problem: R = umax, the input box being part of G); zbound == 0 unbinds; zbound < 0 or not finite:
 * GPAD_ERR_INVALID; before gpad_setup*: GPAD_ERR_NOT_SETUP; every gpad_setup* unbinds, as for the Hessian.  On
 * a class-bound handle the binding is forwarded to every class.  It takes effect only in runs with tol > 0
 * (tol <= 0 runs exactly N iterations whatever is bound).
 *
 * The rule (one text: csrc/gpad_farkas.h), with K = dims.check_every:
 *   events     the test events at which the solve's iteration count v is a multiple of 4 K.  Stateless:
 *              nothing is kept between events.  Algorithm 1 is evaluated first and any code of its wins.
 *   nomination q = sum_i (double)y+_i (double)pD_i over the live rows, in the test's own reduction and in the
 *              order of its gap term; y+ is this iteration's projected iterate (>= 0, and what the solve
 *              returns as y*), pD = -g/L as the device holds it.  Nominated iff q > 0, i.e. g'y+ < 0.
 *   decision   fp64, on the device's G_L = G/L, pD and y+, sums ascending, products and sums unfused:
 *              t_j = sum_i y_i G_L[i][j], a = sum_j |t_j|, p = sum_i |y_i pD_i|, s = sum_i y_i r_i with
 *              r_i = sum_j |G_L[i][j]| (fp64, j ascending: the stream kernel reads them from a table made
 *              at bind time per matrix copy, the panels sum them from their own image of G_L at a decision --
 *              the same numbers either way).  Infeasible iff
 *              q - R a > mu (p + R s), mu = 16 units of 2^-24 (f32) / 2^-53 (f64) as the violation margin
 *              of gpad_run: it covers the roundings of G/L and -g/L and the fp64 sums.
 *   result     code GPAD_CODE_INFEASIBLE, z* = z (as the cap exit returns), y* = y+, the iteration count.
 *              A failed decision changes nothing.
 * Postcondition (the contract): for every instance that returns code 5, gpad_farkas_margin > 0 on the
 * caller's own G, g and the returned y.
 * Stats: code 5 counts as not converged in every aggregate; codes[] carries the 5.  A closed-loop step that
 * ends with code 5 applies u = z*[0:nu] as a capped step does, and the loop goes on.
 *
 * Engines.  Five kernel families carry the branch: gpad_stream_kernel (f32 and f64, any shape, shared or distinct
 * matrices), the f32 T-wave MFMA panel (shared matrices, n, m <= 256: every T <= 16, phased compaction as ever --
 * a code-5 instance leaves the panel like a converged one -- no pair layout, no finisher), the panel loop
 * (GPAD_OPT_LOOP_PANEL and gpad_class_loop_fused: a code-5 column takes its step boundary like any finished
 * column) and, opt-in per handle, the f32 resident kernel (gpad_infeasibility_resident below; n, m <= 208,
 * shared or distinct matrices) and the asynchronous closed loop (gpad_infeasibility_loop_async below; the
 * shapes GPAD_OPT_LOOP_ASYNC takes).  All give the same z, y, counts and codes.  With a bound in force (bound, and
 * tol > 0):
 *   - dims.kernel AUTO and GPAD_KERNEL_PANEL run those panels where they apply; AUTO else the stream kernel
 *     (f64, distinct matrices, n or m > 256), whatever the batch -- the pairs, the finisher, the big panels and
 *     the f64 panels are not used, nor by default the resident kernel;
 *   - GPAD_OPT_LOOP_ASYNC falls back to the lockstep loop, silently as for any shape it does not take
 *     (by default: gpad_infeasibility_loop_async below);
 *   - GPAD_ERR_UNSUPPORTED: a forced GPAD_KERNEL_RESIDENT (by default); a forced GPAD_KERNEL_PANEL where those
 *     panels do not apply; gpad_run_scaled with caller theta / beta tables.  Binding on a flat setup, binding
 *     with a Hessian bound and gpad_setup_hessian with a bound are GPAD_ERR_UNSUPPORTED at the bind.
 *     gpad_group_* has no binding.
 *
 * gpad_infeasibility_resident(h, 1): with a bound in force the resident kernel carries the certificate where
 * it applies.  On an f32 handle a forced GPAD_KERNEL_RESIDENT then runs (n or m > 208: GPAD_ERR_UNSUPPORTED as
 * without a bound) and AUTO takes the resident kernel exactly where it takes it without a bound -- n, m <= 208
 * and distinct matrices at any batch, or shared matrices with batch <= 4 per CU; above that AUTO runs the
 * T-wave panels as before.  Both report GPAD_KERNEL_RESIDENT.  The lockstep loops (gpad_run_state,
 * gpad_closed_loop and their _signals forms, and what GPAD_OPT_LOOP_ASYNC falls back to) follow, a class
 * binding per class; GPAD_OPT_LOOP_PANEL and gpad_class_loop_fused keep their kernels, and forced
 * GPAD_KERNEL_PANEL / GPAD_KERNEL_STREAM, f64 handles and the refusals above stay as they are.  Results are bit
 * for bit those of the other engines.  on = 0 (the default) restores the routing above; any other value, or a
 * NULL handle: GPAD_ERR_INVALID.  Valid any time after gpad_create.  A handle setting like an option: it
 * survives gpad_setup*, gpad_setup_infeasibility and unbinding, changes nothing while no bound is in force, and a
 * class-bound handle forwards it to every class whether set before or after gpad_setup_classes.  An entry
 * point rather than a GPAD_OPT_*: it selects the engine family of a run, as gpad_class_loop_fused does.
 *
 * gpad_infeasibility_loop_async(h, 1): with a bound in force GPAD_OPT_LOOP_ASYNC keeps its one-launch loop: the
 * asynchronous loop kernels (one plant, per-pack plant maps, fleets of distinct matrices) run as variants that
 * hold the certificate event after every fourth test of a pack's own solve.  A code 5 ends that solve like any
 * other termination: the pack applies u = z*[0:nu], goes on to its next step (warm from z*, y* when warm) and
 * the slot is refilled from the queue after its last step.  Reported kernel GPAD_KERNEL_LOOP; z, y, the
 * trajectories, counts and codes are bit for bit the lockstep loop's.  Every other condition of
 * GPAD_OPT_LOOP_ASYNC stands -- f32, n, m <= 208, nx + ns <= 64, AUTO or RESIDENT, no caller schedule tables;
 * GPAD_OPT_LOOP_PANEL and the fused class loop first -- and a run it does not take falls back to the lockstep
 * loop as before (on the resident certificate kernel with gpad_infeasibility_resident also on).  With tol <= 0
 * or no bound the unbound kernels run.  A separate flag from gpad_infeasibility_resident (which keeps a bound
 * GPAD_OPT_LOOP_ASYNC on the lockstep loop), with that function's rules otherwise: off by default, on = 0 / 1,
 * anything else or a NULL handle GPAD_ERR_INVALID, valid any time after gpad_create, kept across gpad_setup*,
 * gpad_setup_infeasibility and unbinding, forwarded to every class of a class-bound handle. */
#define GPAD_CODE_INFEASIBLE 5
int gpad_setup_infeasibility(gpad_handle_t h, double zbound);
int gpad_infeasibility_resident(gpad_handle_t h, int on);
int gpad_infeasibility_loop_async(gpad_handle_t h, int on);
/* host only, no device: *margin = -(g'y) - zbound |G'y|_1 in fp64 on the caller's arrays (G m x n row-major,
 * g and y of m; dtype GPAD_DTYPE_*), -inf when some y_i is negative (or NaN).  > 0 exactly when y certifies
 * that no z with |z|_inf <= zbound satisfies G z <= g: an independent check of a code 5. */
int gpad_farkas_margin(int n, int m, int dtype, const void* G, const void* g, const void* y, double zbound,
                       double* margin);

/* Run GPAD on the bound problem for every instance of the batch.
 *   z0: in z_{-1}, out z*      [batch][n]   (acceldualgrad.m:17, :83)
 *   y0: in y_0 = y_{-1}, out y* [batch][m]  (acceldualgrad.m:16)
 *   M : H^-1 q per instance    [batch][n]   (g_P, acceldualgrad.m:21)
 *   g : constraint rhs         [batch][m]   (b_i; p_D = -g/L, acceldualgrad.m:23)
 *   N : max iterations (reference: N_v = 100, main.cu:87)
 *   tol <= 0: exactly N iterations (paper Algorithm 2, main.cu behaviour);
 *   tol  > 0: Algorithm 1 test every check_every iterations (acceldualgrad.m:66-79), tol = e_g:
 *     (A) max(G z - g) <= tol                                  -> z* = z,    converged = 1
 *     (B) max(G zhat - g) <= tol, w >= 0, -w'(G zhat - g) <= e_V -> z* = zhat, converged = 2
 *     e_V = dims.tol_gap (default tol).  Both violation tests are decided on directly evaluated
 *     chains (G/L z, G/L zhat) with a rounding margin of 16 units of 2^-24 (f32) / 2^-53 (f64)
 *     of max_i |(G x)_i| + |g_i| / L, so a reported convergence holds for G z* - g evaluated
 *     exactly on the returned z*.  With H bound (gpad_setup_hessian) the value-function branches
 *     of acceldualgrad.m:73,76 follow where the MATLAB test reaches them -- after (B)'s
 *     violation part passed -- with valuefcn V(x) = (1/2 x'H + f) x and dualfcn D(y) = V(z(y)) +
 *     y'(G z(y) - g), z(y) = -ML y - M, evaluated in fp64 on the run's data:
 *     (B') w >= 0, -w'(G zhat - g) > e_V, -w'(G zhat - g) <= V(zhat) e_V/(1+e_V) -> z* = zhat, 3
 *     (B'') w not >= 0, V(zhat) - D(y+) <= e_V max(D(y+), 1)                  -> z* = zhat, 4
 *     Without H (the solve(...) surface carries no H, q) they are not evaluated.
 *   Certification floor: the margin above is at least 2^-20 max_i |g_i| (f32; f64: 2^-49), so
 *     a tol below tol_floor = 2^-20 max_{b,i} |g_{b,i}| can never certify an instance whose
 *     solution has an active constraint (G z* - g = 0 in some row) -- e.g. the reference's own
 *     e_g = 1e-6 (acceldualgrad.m:12) on data with |g| of order 10.  Such a run is not rejected
 *     (an instance with no active constraint can still pass) but flagged: st->tol_floor holds
 *     the floor of the run's data and st->flags GPAD_FLAG_TOL_FLOOR is set when tol < it.
 * Host memory: synchronous.  Device memory: enqueued on the handle's stream; synchronous only
 * when st != NULL (stats need the per-instance counters). */
int gpad_run(gpad_handle_t h, void* z0, void* y0, const void* M, const void* g, int N, double tol,
             gpad_stats_t* st);

/* gpad_run for gpad_setup_scaled problems: gP (g_P) and pD (p_D = -g/L) as in the data file,
 * optional per-iteration theta/beta tables (main.cu:61-64; float or double per dtype, length N;
 * NULL -> dims.schedule).  theta/beta are HOST arrays whatever dims.memory says (as main.cu:163,
 * 170 pass them by value per launch); the library copies them to the device. */
int gpad_run_scaled(gpad_handle_t h, void* z0, void* y0, const void* gP, const void* pD, int N,
                    double tol, const void* theta, const void* beta, gpad_stats_t* st);

/* ---- one-time QP precompute on the device ---------------------------
 * acceldualgrad.m:11,20-21 in fp64:  L = ||H||_F^2,  ML = inv(H) A' (n x m),  gP = inv(H) f' (n).
 * Replaces the MATLAB-side precompute (and the off-line data-file generator) that the reference
 * runs before main.cu:29-67 reads M_G, g_P.  shared = 1: one H (n x n) and one A (m x n) for the
 * whole batch (LTI) -> one ML, one L, and gP for each of the batch rows of f; shared = 0: H
 * [batch][n][n], A [batch][m][n] -> ML [batch][n][m], L [batch], gP [batch][n].  f (and gP) may
 * be NULL.  One workgroup per elimination of [H | A' | f'] (shared: [H | A' | I], then
 * gP = inv(H) f' row by row); H must be symmetric positive definite (no pivoting).  memory =
 * GPAD_MEM_HOST or GPAD_MEM_DEVICE for every pointer (device: on the handle's stream).
 * Synchronous.  The outputs feed gpad_setup (ML, A as G, L) and gpad_run (gP as M). */
int gpad_precompute(gpad_handle_t h, int n, int m, int batch, int shared, int memory, const double* H,
                    const double* A, const double* f, double* ML, double* gP, double* L);

/* ---- a tight step bound ------------------------------------------------------------------
 * GPAD converges for L >= lambda_max(G H^-1 G') = rho(G ML), and its iteration count grows like sqrt(L).
 * gpad_precompute's L = ||H||_F^2 is the reference's choice (acceldualgrad.m:11), not a bound on that
 * quantity.  gpad_lipschitz returns an upper bound of rho(G ML) within a factor 1 + rtol of it (for
 * ML = H^-1 G', H symmetric positive definite), in fp64 on the device: with K = min(n, m) and S = ML G
 * (n <= m) or G ML, both of which have G ML's non-zero eigenvalues,
 *     rho(S) <= ||S^p||_F^(1/p) <= K^(1/(2p)) rho(S),      p = 2^k,
 * the left inequality for every square S, the right one for S similar to a symmetric positive semi-definite
 * matrix of rank <= K.  S^p is reached by k squarings, each normalised by its Frobenius norm, k the smallest
 * count with K^(1/2^(k+1)) <= 1 + rtol (at most 16); the result is rounded up by a relative 1e-9, which
 * covers the rounding of the chain.  It is an upper bound for any pair ML, G; only its tightness needs the
 * structure above.
 *   ML n x m, G m x n, row-major, dtype GPAD_DTYPE_F32 or _F64 (widened to fp64 on load);
 *   shared = 1: one pair, L[1] (batch is not read beyond batch >= 1); shared = 0: ML [batch][n][m],
 *   G [batch][m][n], L [batch] -- a fleet that shares one gpad_setup passes the maximum;
 *   memory = GPAD_MEM_HOST or GPAD_MEM_DEVICE for ML, G and L (device: on the handle's stream);
 *   rtol in [0, 1], 0 meaning 0.01; anything else (NaN included) GPAD_ERR_INVALID;
 *   min(n, m) > 4096: GPAD_ERR_UNSUPPORTED.
 * A pair whose S, or one of its squares, is zero gives L = 0 (gpad_setup rejects it).  A norm that is not
 * finite (a NaN or infinity in ML or G, overflow) returns GPAD_ERR_INVALID, gpad_last_error naming the
 * instance.  Synchronous.  Deterministic: no floating-point atomics, so L[b] has the same bits on every run,
 * for host and device operands, and alone or at any position of a batch.  Instances are processed in chunks
 * whose workspace (kept on the handle, freed by gpad_destroy) stays within 1 GiB and 1024 instances, a single
 * instance excepted; k + 1 launches per chunk.
 * gpad_lipschitz_host: the same recursion in plain fp64 loops on host arrays, every sum ascending -- no
 * handle, no device.  It agrees with gpad_lipschitz to fp64 summation order (about 1e-13 relative). */
int gpad_lipschitz(gpad_handle_t h, int n, int m, int batch, int shared, int dtype, int memory, const void* ML,
                   const void* G, double rtol, double* L);
int gpad_lipschitz_host(int n, int m, int batch, int shared, int dtype, const void* ML, const void* G, double rtol,
                        double* L);

/* ---- per-state QP data and closed-loop MPC -------------------
 * For an LTI plant the state-dependent QP data are affine in the state x (nx):
 *   M(x) = M0 + PM x   (n;  PM = H^-1 F': the reference forms f = x0'F, gpad.m:81, and
 *                            g_P = H^-1 f', acceldualgrad.m:21, on the host every MPC step)
 *   g(x) = g0 + Pg x   (m;  b_i(x0), gpad.m:85)
 * and the receding-horizon update is x+ = A x + B u with u = z*[0:nu] (gpad.m:91-93).
 * gpad_setup_plant binds PM (n x nx), Pg (m x nx), optional M0 (n) / g0 (m) (NULL = 0) and,
 * for closed-loop runs, A (nx x nx) and B (nx x nu).  Row-major, dims.dtype / dims.memory of
 * the preceding gpad_setup, whose ML/G/L the solves use.  The fp32 evaluation order is
 * acc = c0; acc = fma(P[i][k], x[k], acc) for k = 0..nx-1 (and A then B for the update). */
int gpad_setup_plant(gpad_handle_t h, int nx, int nu, const void* PM, const void* M0, const void* Pg,
                     const void* g0, const void* A, const void* B);

/* gpad_setup_plant for a batch of distinct plants: same meaning and validation, but every non-NULL
 * array holds dims.batch consecutive per-instance copies,
 *   PM [batch][n][nx], M0 [batch][n], Pg [batch][m][nx], g0 [batch][m], A [batch][nx][nx],
 *   B [batch][nx][nu],
 * and gpad_run_state / gpad_closed_loop evaluate instance b with copy b of each map:
 *   M_b(x) = M0_b + PM_b x,  g_b(x) = g0_b + Pg_b x,  x+ = A_b x + B_b z*[0:nu].
 * The arithmetic per instance is gpad_setup_plant's, so a batch bound here gives, instance for
 * instance, the bits of `batch` separate batch-1 handles bound with gpad_setup_plant.
 * It combines with either setting of dims.shared: 0 is a fleet (every instance its own ML, G and
 * maps, all of which derive from its plant), 1 is one controller (shared ML, G) run against
 * per-instance true plants -- a plant/model mismatch study.  L stays the one scalar of gpad_setup:
 * a fleet passes an L valid for every instance, e.g. the maximum of the per-instance bounds.
 * A later gpad_setup_plant rebinds one shared plant.  The binding is for the dims.batch of the
 * preceding gpad_setup: after a gpad_setup with another batch, gpad_run_state / gpad_closed_loop
 * return GPAD_ERR_NOT_SETUP until a plant is bound again. */
int gpad_setup_plant_batch(gpad_handle_t h, int nx, int nu, const void* PM, const void* M0, const void* Pg,
                           const void* g0, const void* A, const void* B);

/* gpad_run with M = M(x), g = g(x) evaluated on the device for every instance's state
 * x [batch][nx] (no host round trip for the per-state precompute). */
int gpad_run_state(gpad_handle_t h, const void* x, void* z0, void* y0, int N, double tol,
                   gpad_stats_t* st);

/* Closed-loop simulation of gpad.m:79-95 on the device, for every instance of the batch:
 *   for t < steps:  M, g <- M(x), g(x);  z, y <- 0 (warm == 0, acceldualgrad.m:16-17) or kept
 *                   from the previous step (warm != 0);  GPAD(N, tol);
 *                   xs[t] = x;  us[t] = u = z*[0:nu];  x <- A x + B u
 * x [batch][nx]: in x_0, out x_steps.  z [batch][n], y [batch][m]: the last step's solution.
 * xs [steps][batch][nx], us [steps][batch][nu]: optional trajectories (NULL to skip).
 * st->iters and st->codes, when given, receive [steps][batch] iteration counts and termination
 * codes (size both arrays steps * batch); the other stats aggregate over every (step, instance);
 * kernel_ms times the whole loop.
 *
 * By default the steps run in lockstep: per step the affine maps, the solve of the whole batch and
 * the plant update are enqueued one after the other, so with tol > 0 every step lasts as long as its
 * slowest instance.  With GPAD_OPT_LOOP_ASYNC = 1 the loop is one launch (stats kernel =
 * GPAD_KERNEL_LOOP) in which an instance whose solve terminates applies its own plant update and
 * affine maps and starts its next step at once, no instance waiting for another.  That path is
 * taken for f32 matrices bound by gpad_setup (shared or per instance; no flat setup, no Hessian),
 * n, m <= 208, dims.kernel AUTO or RESIDENT, N >= 1, nx <= 64 and nu <= min(n, 64), with a plant
 * bound by gpad_setup_plant or gpad_setup_plant_batch; any other call runs the lockstep loop as if
 * the option were unset.  With per-instance matrices a workgroup holds one instance at a time and
 * keeps its matrix rows in registers for all `steps` steps; the grid is up to two workgroups per
 * compute unit where they fit, capped by GPAD_OPT_DUO_MAX_GRID like the shared-matrix grid.  Results are identical either way: x, z, y, xs, us and
 * every stat (per-step counts and codes included) are bit for bit those of the lockstep loop.
 *
 * GPAD_OPT_LOOP_PANEL = 1 is the same one-launch loop for fleets, on the f32 MFMA panels (stats
 * kernel = GPAD_KERNEL_LOOP_PANEL): a workgroup owns a panel of 16 instances, and a panel column whose
 * solve terminates applies its plant update and affine maps in place and goes on with its next
 * step; after an instance's last step the column takes the next instance from a queue.  It is
 * looked at before GPAD_OPT_LOOP_ASYNC and taken for f32 matrices shared by the batch
 * (dims.shared = 1; no flat setup, no Hessian), n, m <= 256, dims.kernel AUTO or PANEL, N >= 1,
 * tol <= 0 or N a multiple of dims.check_every, nx <= 64 and nu <= min(n, 64), with a plant bound
 * by gpad_setup_plant or gpad_setup_plant_batch; the grid is capped by GPAD_OPT_PANEL_MAX_GRID.  Any
 * other call goes on as if the option were unset (GPAD_OPT_LOOP_ASYNC's rules, then lockstep).
 * Results are bit for bit those of the lockstep loop here too. */
int gpad_closed_loop(gpad_handle_t h, void* x, void* z, void* y, int steps, int N, double tol, int warm,
                     void* xs, void* us, gpad_stats_t* st);

/* ---- exogenous signals: references, measured disturbances, time-varying bounds, noise ---------
 * A handle with a plant bound may bind three more maps for a signal vector s (ns), known at each
 * MPC step and not generated by the plant:
 *   M(x, s) = M0 + PM x + SM s      SM: n  x ns
 *   g(x, s) = g0 + Pg x + Sg s      Sg: m  x ns
 *   x+      = A x + E s + B u       E : nx x ns,  u = z*[0:nu]
 * Evaluation order, in dims.dtype with explicit fmas: an affine row is acc = c0[i], then
 * fma(P[i][k], x[k], acc) for k < nx, then fma(S[i][j], s[j], acc) for j < ns; a plant row is acc = 0,
 * then the A x terms, the E s terms, the B u terms.  A NULL map is a map of zeros whose terms are
 * evaluated, not a skipped chain.  Step t of a loop uses S[t] for the QP data of step t and for the
 * update from x_t to x_{t+1}.  This is, bit for bit, gpad_setup_plant on the augmented state
 * x~ = [x; s] with PM~ = [PM SM], Pg~ = [Pg Sg], A~ = [[A E]; [0 0]], B~ = [B; 0], the s rows of x~
 * replaced by the caller's S[t] before every step.  A preview of a reference over the horizon is a
 * longer s: the caller stacks r_t .. r_{t+N-1}.
 *
 * gpad_setup_signals is called after gpad_setup_plant / gpad_setup_plant_batch (GPAD_ERR_NOT_SETUP
 * before) and uses the dtype and memory of the bound problem.  After gpad_setup_plant_batch every
 * non-NULL map holds dims.batch consecutive copies -- SM [batch][n][ns], Sg [batch][m][ns],
 * E [batch][nx][ns] -- else one.  ns >= 1 binds; ns == 0 unbinds (the pointers are ignored); ns < 0
 * and a non-NULL E on a plant bound without A, B are GPAD_ERR_INVALID.  A later gpad_setup_plant,
 * gpad_setup_plant_batch or gpad_setup unbinds the signals. */
int gpad_setup_signals(gpad_handle_t h, int ns, const void* SM, const void* Sg, const void* E);

/* gpad_run_state with signals s [batch][ns], and gpad_closed_loop with S [steps][batch][ns] (in the
 * memory of dims.memory).  xs stays [steps][batch][nx]: the signals are not echoed.  Everything else
 * is as in gpad_run_state / gpad_closed_loop; tol_floor and the flags cover the g(x, s) of every step.
 * With signals bound the plain gpad_run_state / gpad_closed_loop return GPAD_ERR_INVALID (a silently
 * dropped disturbance is worse than an error); with none bound these two return GPAD_ERR_NOT_SETUP.
 * A NULL s / S is GPAD_ERR_INVALID.  GPAD_OPT_LOOP_ASYNC applies when, in addition to
 * gpad_closed_loop's conditions, nx + ns <= 64 (the state and the signals share one 64-word row); any
 * other call runs the lockstep loop, where ns is unbounded.  GPAD_OPT_LOOP_PANEL has the same extra
 * condition, nx + ns <= 64.  Results are identical either way. */
int gpad_run_state_signals(gpad_handle_t h, const void* x, const void* s, void* z0, void* y0, int N, double tol,
                           gpad_stats_t* st);
int gpad_closed_loop_signals(gpad_handle_t h, void* x, void* z, void* y, const void* S, int steps, int N,
                             double tol, int warm, void* xs, void* us, gpad_stats_t* st);

/* ---- fleets of a few plant classes: per-class matrices on the shared-matrix engines ----------------
 * A fleet of 8192 packs rarely has 8192 distinct plants: it has a handful of types (SKUs, capacity
 * bins, ageing bins).  Bound with dims.shared = 0 such a fleet carries a matrix pair per pack and runs
 * the kernels for distinct matrices (no MFMA panels); a class binding carries K pairs and solves the
 * packs of one class together as a shared-matrix sub-batch, so every class runs on the engines of
 * dims.shared = 1 -- panel pairs, phased compaction, finisher, the one-launch loops -- each class
 * picking its own engine for its own size.  Results are bit for bit those of the dims.shared = 0 binding
 * of the same fleet (ML, G of instance b = those of class class_of[b]; gpad_setup_plant_batch with the
 * maps of class class_of[b]).
 *
 * On a class-bound handle
 *   - gpad_run, gpad_run_state, gpad_closed_loop, gpad_last_stats, gpad_accumulate_iterations, gpad_sync,
 *     gpad_set_stream and gpad_set_option work unchanged for the caller, whose arrays stay in the
 *     caller's instance order (the library permutes rows to and from a class-sorted workspace on the
 *     device).  gpad_set_stream and gpad_set_option are forwarded to every class, GPAD_OPT_LOOP_ASYNC
 *     and GPAD_OPT_LOOP_PANEL included, which each class then applies by its own rules (a class that
 *     does not qualify runs the lockstep loop); gpad_class_loop_fused, where it takes the call, is
 *     looked at before the forwarded loop options.  The plain gpad_setup_plant binds the same maps for
 *     every class.
 *   - gpad_setup_hessian, gpad_setup_plant_batch, gpad_setup_signals and gpad_run_scaled return
 *     GPAD_ERR_UNSUPPORTED, gpad_last_error naming the class binding.  Signals are bound with
 *     gpad_setup_class_signals below; until they are, the _signals runs return GPAD_ERR_UNSUPPORTED too.
 *   - the phase diagnostics (gpad_phase_plan, gpad_phase_counts, gpad_last_phases) return 0.
 *   - a later gpad_setup, gpad_setup_scaled or gpad_setup_flat ends the binding and frees everything
 *     it held; a later gpad_setup_classes replaces it.
 * Stats: iterations = max over the classes, converged and total_iterations = sums, tol_floor = max,
 * flags OR-ed, iters / codes [steps][batch] in the caller's order, kernel = the kernel of the class
 * with the most instances (ties: the lowest class), kernel_ms = events on the handle's stream around the
 * whole call, row permutations included.  A GPAD_ERR_DEVICE of any class is returned, and stays sticky
 * as on any handle.
 * The classes run one after the other on the handle's stream (a loop: class 0's `steps` steps, then
 * class 1's); they are independent, so the order changes no result.  Every (class, step) so pays its own
 * launches and its own tail on a part of the GPU; gpad_class_loop_fused below runs a closed loop of every
 * class as one launch instead.  Not provided: classes running concurrently on several streams, per-pack
 * true plants under a class binding, Hessian branches. */

/* host only, no device work (for tests/tools, like gpad_plan_phases): the class-sorted order.
 * perm[batch]: sorted position -> instance, classes ascending, instances ascending inside a class
 * (stable); offsets[K + 1]: class k occupies positions offsets[k] .. offsets[k+1]-1.
 * GPAD_ERR_INVALID: NULL, batch < 1, K < 1, an id outside 0..K-1. */
int gpad_class_order(const int* class_of, int batch, int K, int* perm, int* offsets);

/* gpad_setup for a fleet of K plant classes: ML [K][n][m], G [K][m][n] (dims.dtype / dims.memory),
 * class_of [batch] HOST ints in 0..K-1 (as theta/beta: host whatever dims.memory says), one L.
 * dims.shared must be 1 (matrices are shared inside a class); 1 <= K <= dims.batch; a class may be empty. */
int gpad_setup_classes(gpad_handle_t h, const gpad_dims_t* dims, int K, const int* class_of,
                       const void* ML, const void* G, double L);

/* gpad_setup_plant with one copy of every non-NULL map per class: PM [K][n][nx], M0 [K][n], Pg [K][m][nx],
 * g0 [K][m], A [K][nx][nx], B [K][nx][nu]; instance b uses copy class_of[b].  GPAD_ERR_NOT_SETUP unless
 * the handle is class-bound. */
int gpad_setup_plant_classes(gpad_handle_t h, int nx, int nu, const void* PM, const void* M0,
                             const void* Pg, const void* g0, const void* A, const void* B);

/* gpad_setup_signals for a class-bound handle with a plant bound (gpad_setup_plant or
 * gpad_setup_plant_classes; either combines with either per_class).  per_class = 1: every non-NULL map holds
 * K copies, SM [K][n][ns], Sg [K][m][ns], E [K][nx][ns], and instance b uses copy class_of[b] (an empty
 * class's copy is present and ignored); per_class = 0: one copy serves every class.  dtype and memory follow
 * dims; a NULL map is a map of zeros whose terms are evaluated; the evaluation order is gpad_setup_signals'.
 * ns >= 1 binds, ns == 0 unbinds, ns < 0 and per_class outside {0, 1} are GPAD_ERR_INVALID, as is a non-NULL
 * E on a plant bound without A, B; GPAD_ERR_NOT_SETUP on a handle that is not class-bound or has no plant.
 * A later gpad_setup_plant, gpad_setup_plant_classes, gpad_setup_classes or any gpad_setup* unbinds.
 * With class signals bound, gpad_run_state_signals and gpad_closed_loop_signals take s [batch][ns] and
 * S [steps][batch][ns] in the caller's instance order (dims.memory), a NULL s / S is GPAD_ERR_INVALID, and
 * the plain gpad_run_state / gpad_closed_loop return GPAD_ERR_INVALID as on a plain handle.  Class k binds
 * its copy with gpad_setup_signals and runs on its own rows of S; the forwarded GPAD_OPT_LOOP_ASYNC /
 * GPAD_OPT_LOOP_PANEL apply by each class's own rules (nx + ns <= 64; ns is unbounded on the lockstep loop),
 * and gpad_class_loop_fused takes a gpad_closed_loop_signals call by its rules below with nx + ns in the
 * place of nx.  Results are bit for bit those of the dims.shared = 0 binding of the expanded fleet
 * (gpad_setup_plant_batch + gpad_setup_signals, instance b holding the copies of class class_of[b]):
 * outputs, trajectories, per-step counts and codes, stats by the rules above; tol_floor and the flags cover
 * g(x, s) of every step of every class. */
int gpad_setup_class_signals(gpad_handle_t h, int ns, int per_class, const void* SM, const void* Sg,
                             const void* E);

/* The fused class loop (opt-in, off by default): gpad_closed_loop of a class-bound handle as ONE launch of
 * the class-aware MFMA panel loop (the kernel of GPAD_OPT_LOOP_PANEL; reported kernel =
 * GPAD_KERNEL_LOOP_CLASSES).  A workgroup serves one class at a time -- its 16 panel columns hold packs of
 * that class, claimed from the class's own queue -- and moves on to another class with unclaimed packs when
 * its own has none left, so the call pays one tail and no per-class launch trains.  No workgroup waits for
 * another.  Results (outputs, trajectories, per-step counts and codes, stats, tol_floor, flags) are bit
 * for bit those of the binding without it.
 * on = 0 or 1 (anything else: GPAD_ERR_INVALID); GPAD_ERR_NOT_SETUP unless the handle is class-bound;
 * cleared by a later gpad_setup_classes and by every gpad_setup*.
 * It is looked at before the forwarded loop options, and takes a call when steps >= 1 and the shape
 * meets the rules of GPAD_OPT_LOOP_PANEL (the same for every class, which share dims): f32, n, m <= 256,
 * dims.kernel AUTO or PANEL, N >= 1, tol <= 0 or N % check_every == 0, nx <= 64 (with class signals
 * nx + ns <= 64), nu <= min(n, 64), the plant bound with A and B.  Any other call (f64, gpad_run, gpad_run_state, ...) runs class by class exactly as
 * if it were off, with that path's results and reported kernel, silently, as the loop options do.
 * Grid: min(sum_k ceil(count_k / 16), resident workgroups, 1024), capped by GPAD_OPT_PANEL_MAX_GRID; the
 * workgroups start on the classes gpad_class_loop_deal gives them.
 * gpad_last_stats, gpad_accumulate_iterations, gpad_sync and the sticky GPAD_ERR_DEVICE work after a fused
 * run as after any run, the stats by the rules above with kernel = GPAD_KERNEL_LOOP_CLASSES.  The binding
 * makes one more handle of the whole batch the first time the loop is turned on (f32 bindings only). */
int gpad_class_loop_fused(gpad_handle_t h, int on);

/* host only, no device work (for tests/tools, like gpad_class_order): the class each of `grid` workgroups
 * of the fused class loop starts on, start_class[grid], class 0's workgroups first.  Workgroups are dealt
 * in proportion to the classes' panel counts ceil(counts[k] / 16); none goes to an empty class; with grid
 * at least the number of non-empty classes each of those gets one, else the classes with the most panels
 * are dealt first (ties: the lowest) and the others are reached by switching.
 * GPAD_ERR_INVALID: NULL, K < 1, grid < 1, a negative count, every count zero. */
int gpad_class_loop_deal(const int* counts, int K, int grid, int* start_class);

/* ---- reference data-file boundary (main.cu:29-67 readData) ------------------------------
 * Text file: "n_u N m num_iterations L", then M_G (n*m), g_P (n), G_L (n*m), p_D (m),
 * theta (num_iterations), beta (num_iterations), n = n_u*N, whitespace-separated floats.
 * M_G = -H^-1 G' (sign-folded), G_L = G/L, p_D = -g/L: the gpad_setup_scaled/run_scaled
 * inputs.  The file's matrix layout is the reference build's choice: GPAD_FILE_ROWMAJOR is
 * seq_functions.cpp's (M_G[i*m+j], G_L[i*n+j]); GPAD_FILE_FLIPPED is kernel_functions.cu's
 * ENABLE_FLIPPING layout (M_G[j*n+i], G_L[j*m+i]).  The struct always holds the row-major
 * mathematical orientation (M_G n x m, G_L m x n). */
#define GPAD_FILE_ROWMAJOR 0
#define GPAD_FILE_FLIPPED 1
#define GPAD_FILE_FLAT 2 /* ENABLE_FLATTEN_MATRICES files: M_G is N x m, G_L is m x N (flat) */

typedef struct gpad_datafile {
    int n_u, N, m, num_iterations;
    float L;
    float* M_G;   /* n x m  (GPAD_FILE_FLAT: N x m) */
    float* g_P;   /* n */
    float* G_L;   /* m x n  (GPAD_FILE_FLAT: m x N) */
    float* p_D;   /* m */
    float* theta; /* num_iterations */
    float* beta;  /* num_iterations */
} gpad_datafile_t;

/* Allocates the arrays (release with gpad_datafile_free).  GPAD_ERR_INVALID on a malformed or
 * truncated file (the reference's readData only perror()s and continues). */
int gpad_datafile_read(const char* path, int layout, gpad_datafile_t* out);
int gpad_datafile_write(const char* path, int layout, const gpad_datafile_t* f);
void gpad_datafile_free(gpad_datafile_t* f);

/* Per-instance iteration counts / convergence flags of the last run (device work finished). */
int gpad_last_stats(gpad_handle_t h, gpad_stats_t* st);

/* Enqueue, on the handle's stream, acc[0] += the sum of the last run's per-instance iteration
 * counts (acc: one device int64).  Lets a caller count the work of back-to-back asynchronous
 * runs without a host synchronisation per run (bench.py's timed loop). */
int gpad_accumulate_iterations(gpad_handle_t h, long long* acc);

/* Diagnostics (no reference counterpart): the phase plan the next phased panel solve of this
 * handle will follow, made from the previous solve's iteration counts by gpad_last_stats / a
 * stats-collecting run.  Writes up to cap phase ends (iterations; the last is N) and finisher
 * thresholds, and the modelled solve time in us; returns the number of phases (0: no plan,
 * the default schedule applies). */
int gpad_phase_plan(gpad_handle_t h, int* ends, int* fins, int cap, double* cost_us);
/* Diagnostics: the survivors each boundary of the last phased panel solve listed -- counts[ph] =
 * instances still running after phase ph (the next phase's input) -- for up to cap phases
 * (synchronises the handle's stream).  Returns the number written, 0 when the last run was not a
 * phased panel solve. */
int gpad_phase_counts(gpad_handle_t h, int* counts, int cap);
/* Diagnostics: the phases the last phased panel solve of this handle actually launched -- ends[ph]
 * (iterations), fins[ph] (the finisher threshold at the start of phase ph: the finisher takes phase
 * ph's list when counts[ph - 1] <= fins[ph]; 0 = none) and counts[ph] (survivors after phase ph, as
 * gpad_phase_counts) -- for up to cap phases (any array may be NULL; counts synchronises the stream);
 * *prior (may be NULL) = 1 when the solve followed the shape's plan prior (a handle without a plan
 * of its own: gpad_run).  Returns the number of phases written, 0 when the last run was not a phased
 * panel solve. */
int gpad_last_phases(gpad_handle_t h, int* ends, int* fins, int* counts, int cap, int* prior);
/* The planner itself on given iteration counts (host only, no device work; for tests/tools). */
int gpad_plan_phases(const int* iters, int batch, int n, int m, int N, int check_every, int num_cus,
                     int* ends, int* fins, int cap, double* cost_us);

/* One-shot north-star surface: solve(z0, y0, ML, M, G, g, N, L, tol).  Equivalent to
 * create + setup + run + destroy (the handle is cached per thread and device). */
int gpad_solve(void* z0, void* y0, const void* ML, const void* M, const void* G, const void* g,
               int N, double L, double tol, const gpad_dims_t* dims, gpad_stats_t* st);
/* Free the calling thread's cached gpad_solve handle and gpad_solve_sharded group (device memory,
 * streams, RCCL communicators).  Call it before a thread that used them exits; the caches are
 * never freed from a thread-exit destructor (at process exit the OS reclaims them). */
void gpad_release_cached(void);

/* ---- multi-device: instance shards, RCCL scatter/gather ------------------
 * A group drives several devices from ONE C process (the reference's caller is a single C
 * program, main.cu:79-203; north_star: "partition across the 8 GPUs of one node by sharding
 * independent MPC problem instances with a single RCCL gather of solutions").  One handle and
 * HIP stream per device; the batch splits into contiguous shards (sizes differ by at most one,
 * larger first) solved with no communication.  dims.memory == GPAD_MEM_DEVICE: every pointer is
 * device memory on devices[0] (the root); shared ML/G are broadcast at setup (ncclBroadcast),
 * per-instance matrices and each non-root shard of M, g, z0, y0 go out by one grouped
 * ncclSend/ncclRecv, and (z*, y*) come back into the root buffers by another.  GPAD_MEM_HOST:
 * every device copies its own shard in and out.  With distinct devices the group holds one RCCL
 * clique (ncclCommInitAll); a device listed twice (one GPU standing in for several) moves the
 * same bytes by peer copies instead (gpad_group_transport tells which).  librccl is loaded on the
 * first group over distinct devices (not linked: single-GPU users need no RCCL); when it cannot
 * be loaded such a group uses the peer copies too. */
typedef struct gpad_group_s* gpad_group_t;
#define GPAD_GROUP_RCCL 1
#define GPAD_GROUP_PEER 2
int gpad_group_create(gpad_group_t* g, int ndev, const int* devices);
int gpad_group_destroy(gpad_group_t g);
int gpad_group_transport(gpad_group_t g); /* GPAD_GROUP_RCCL or GPAD_GROUP_PEER */
/* Integration / test hook: groups created after this call (gpad_group_create, gpad_solve_sharded)
 * take their RCCL entry points (ncclCommInitAll, ncclCommDestroy, ncclGroupStart / End, ncclSend,
 * ncclRecv, ncclBroadcast, ncclGetErrorString) from the shared library at `path` (NULL: the default
 * librccl).  force_rccl != 0: they use the RCCL transport even when a device is listed twice (for a
 * library that accepts it -- real RCCL refuses duplicate devices, so the group creation then fails).
 * Returns GPAD_OK, or GPAD_ERR_UNSUPPORTED when the library or one of the symbols cannot be loaded;
 * such groups then use the peer copies.  Existing groups keep the library they were created with. */
int gpad_group_rccl_library(const char* path, int force_rccl);
/* Device memory: the stream of devices[0] on which the caller produces / consumes the buffers it
 * passes (NULL, the default: the null stream).  Setup and run first make every device stream of
 * the group wait for the work queued on it so far; runs are synchronous, so the results are
 * complete when gpad_group_run returns. */
int gpad_group_set_stream(gpad_group_t g, void* hip_stream);
/* dims.batch is the WHOLE batch (as for gpad_setup); ML, G as gpad_setup's. */
int gpad_group_setup(gpad_group_t g, const gpad_dims_t* dims, const void* ML, const void* G, double L);
/* The whole batch's vectors (gpad_run's meaning).  Synchronous.  st aggregates every shard
 * (kernel_ms: the slowest shard's device time); st->iters, when given, receives [batch] counts. */
int gpad_group_run(gpad_group_t g, void* z0, void* y0, const void* M, const void* g_rhs, int N, double tol,
                   gpad_stats_t* st);
/* One-shot solve(...) over several devices (the group is cached per thread and device list). */
int gpad_solve_sharded(int ndev, const int* devices, void* z0, void* y0, const void* ML, const void* M,
                       const void* G, const void* g, int N, double L, double tol, const gpad_dims_t* dims,
                       gpad_stats_t* st);

/* ---- per-step device entry points (float, device pointers, handle stream) ---------------
 * Mirror the reference kernels of kernel_functions.h:9-41 one for one, with the CPU
 * semantics of seq_functions.h:4-17 (row-major matrices).  For integration and per-step
 * known-answer tests; the fused gpad_run path is the fast one. */
/* 8a: w = y + beta (y - ym1)               -- StepOneGPADKernel, kernel_functions.cu:7-14   */
int gpad_step1_extrapolate(gpad_handle_t h, const float* y, const float* ym1, float* w, float beta,
                           int m);
/* 8b: zhat = MGneg w - gP (MGneg n x m)    -- StepTwoGPADKernel, kernel_functions.cu:16-64  */
int gpad_step2_primal(gpad_handle_t h, const float* MGneg, const float* w, const float* gP,
                      float* zhat, int n, int m);
/* 8c: z = (1-theta) zm1 + theta zhat        -- StepThreeGPADKernel, kernel_functions.cu:66-72 */
int gpad_step3_average(gpad_handle_t h, float theta, const float* zm1, const float* zhat, float* z,
                       int n);
/* 8d: yp1 = max(0, w + GL zhat + pD)        -- StepFourGPADFlippedParRows, kernel_functions.cu:142-200 */
int gpad_step4_project(gpad_handle_t h, const float* GL, float* yp1, const float* w,
                       const float* pD, const float* zhat, int n, int m);
/* flat battery steps (device pointers; MGf N x m, GLf m x N):
 * StepTwoGPADFlatSequential seq_functions.cpp:5-20 / StepFourGPADFlatParRows kernel_functions.cu:74-109
 * (with the CPU step's projection y < 0 -> 0, seq_functions.cpp:40-42). */
int gpad_step2_primal_flat(gpad_handle_t h, const float* MGf, const float* w, const float* gP,
                           float* zhat, int N, int n_u, int m);
int gpad_step4_project_flat(gpad_handle_t h, const float* GLf, float* yp1, const float* w,
                            const float* pD, const float* zhat, int N, int n_u, int m);
/* 8e (host): theta[v], beta[v] for v < N   -- acceldualgrad.m:18,27,55-56 / main.cu:61-64    */
int gpad_schedule(int N, int kind, double* theta, double* beta);

/* ---- schedule / launch tuning (no reference counterpart) ---------------------------------
 * Per-handle options for tests, diagnostics and A/B tools.  None changes any result: they move
 * phase boundaries, cap grids, reorder the finisher's queue or choose where operands are staged.
 * value GPAD_OPT_DEFAULT restores the default.  Returns GPAD_ERR_INVALID for an unknown option
 * or an out-of-range value. */
#define GPAD_OPT_DEFAULT (-1)
#define GPAD_OPT_PHASE_LEN 1       /* panel phase length in iterations (default 4 * check_every,
                                    * doubling after the 10th phase; set: uniform, with PLAN 0);
                                    * flat panels: the first phase                                  */
#define GPAD_OPT_FINISH_THRESH 2   /* survivors at which the finisher takes over (default 2/CU)    */
#define GPAD_OPT_PLAN 3            /* 1: plan phases from the previous solve's counts (default)    */
#define GPAD_OPT_PHASED 4          /* 1: phased compaction of tol > 0 panel solves (default; flat
                                    * panels: from 4 panels per CU), 2: always, 0: one launch       */
/* 5 (finisher kind), 13 (solo finisher workgroups), 15 (plan finisher cost): retired in 0.3 after
 * measuring no gain; 14 (condensed panels): removed with the condensed operator in
 * 0.4; 17: the round-4 pair layouts (W32, TailPair) measured slower and left out of 0.4; 20 (panel
 * dataflow GEMM boundaries, 2-4 % slower) and 21 (finisher slot hand-off mailbox, even at the step
 * level): built and measured in round 5, removed in 0.5; setting any of them
 * returns GPAD_ERR_INVALID                                                                       */
#define GPAD_OPT_LPT 6             /* 1: longest-predicted-first finisher queue (default)          */
#define GPAD_OPT_PANEL_MAX_GRID 7  /* cap on the panel grid, workgroups (0 = none, default)        */
#define GPAD_OPT_DUO_MAX_GRID 8    /* cap on the finisher grid (0 = none, default)                 */
#define GPAD_OPT_FLAT_PANEL_MIN 9  /* batch from which flat setups run the flat panels (default 8/CU) */
#define GPAD_OPT_FLAT_PANELS 10    /* panels per flat-panel workgroup, 1..4 (0 = auto, default)    */
#define GPAD_OPT_FLAT_WAVES 11     /* flat-panel workgroup waves: 0 auto (default), 8 or 16         */
#define GPAD_OPT_FLAT_A_LDS 12     /* 1: flat fragment image staged in LDS when it fits (default)  */
#define GPAD_OPT_DEBUG_DROP_HANDOFF 16 /* test only (fault injection): 1 = every panel solve that
                                    * uses the chain hand-off withholds its first post, so the
                                    * receiver's bounded wait expires and the run ends in
                                    * GPAD_ERR_DEVICE; 0 (default) = off.  Honoured by the
                                    * 193..208-row shapes (the C3/C4 tiling, T = 13), which run
                                    * a separate test-only kernel instantiation while it is set */
#define GPAD_OPT_P64_RELAY 18      /* 1: f64 panels at T = 9, 13 (n, m in (128, 144], (192, 208]) run
                                    * the 16-wave relay layout (default); 0: one wave per tile */
#define GPAD_OPT_P64_REFILL 19     /* 1: f64 panel solves with tol > 0, N a multiple of check_every and
                                    * more panels than workgroups refill a finished column with the
                                    * next instance (default); 0: each panel runs to its slowest column */
#define GPAD_OPT_LOOP_ASYNC 22     /* 1: gpad_closed_loop runs the whole loop in one launch in which
                                    * every instance steps on its own (see gpad_closed_loop) where that
                                    * kernel applies, else the lockstep loop; 0 (default): lockstep */
#define GPAD_OPT_LOOP_PANEL 23     /* 1: gpad_closed_loop runs the whole loop in one launch on the MFMA
                                    * panels, every panel column stepping on its own (see
                                    * gpad_closed_loop), where that kernel applies, else as without
                                    * the option; 0 (default): off */
int gpad_set_option(gpad_handle_t h, int option, int value);

/* ---- adaptive restart of the momentum (O'Donoghue & Candes; no reference counterpart) ------------
 * gpad_set_option(h, GPAD_OPT_RESTART, R), option 24 -- set through gpad_set_option and kept, like every
 * option, across gpad_setup*, but unlike the tuning options above it CHANGES RESULTS (fewer iterations to
 * the same tolerance; other z*, y* bits), which is why it is defined apart from them.
 *   R = 0 (default): off -- every kernel and every result as without the option.
 *   R >= 1: after every iteration k of an instance's own solve (counted from 1) with k % R == 0 and k < the
 *     solve's final count, the instance decides on a restart.  Algorithm 1 and the iteration cap come first:
 *     an iteration that ends the solve decides nothing.  With tol > 0 and at fixed N alike.
 *   GPAD_OPT_DEFAULT (-1) restores 0, as for every option; any other R < 0 is GPAD_ERR_INVALID.
 * The decision uses iteration k's own vectors: q = sum_i (double)(w_i - y+_i) * (double)(y+_i - y_i), the two
 * differences each rounded once in the handle's dtype, the products and the sum in fp64 (f32 products are
 * exact there), summed in the engine's own order.  The instance restarts iff q > 0: its next iteration runs
 * with w = y+ exactly and reads theta / beta from position 0 of the schedule, the one after from position 1,
 * and so on -- each instance has its own position.  z, y and the recursions of Algorithm 1 go on untouched
 * (theta_0 = 1 makes the average forget z_{-1} by itself).  While the iterates are finite this is, bit for
 * bit, the plain solve with the per-instance tables theta'[k + 1 + i] = theta[i], beta'[k + 1] = 0,
 * beta'[k + 1 + i] = beta[i] (i >= 1) spliced in at every restart after the iteration of index k
 * (tests/restart_ref.py).
 * Routing with R > 0.  A forced GPAD_KERNEL_PANEL, and GPAD_KERNEL_AUTO where it runs panels without the
 * option (shared matrices, more instances than the latency kernel serves), run the f32 T-wave MFMA panels'
 * restart variant where the plain T-wave panels apply -- shared f32 matrices, n, m <= 256; every column has
 * its own position in the schedule; no pair layout and no finisher, as with a certificate bound; phased
 * compaction stays, a parked instance keeps its position and count (stats kernel = GPAD_KERNEL_PANEL).
 * GPAD_KERNEL_AUTO otherwise (f64, per-instance matrices, n or m > 256, small batches) and a forced
 * GPAD_KERNEL_STREAM run the stream kernel's restart variant (GPAD_KERNEL_STREAM), f32 and f64.  Both give
 * the same bits.  gpad_run_state and the lockstep gpad_closed_loop (with signals or without) reach them solve
 * by solve; GPAD_OPT_LOOP_ASYNC, GPAD_OPT_LOOP_PANEL and gpad_class_loop_fused fall back to the lockstep loop
 * while R > 0, and a class binding forwards the option to its classes.  GPAD_ERR_UNSUPPORTED, with a message
 * that names the restart, from the run (the handle then still runs with R = 0): a forced
 * GPAD_KERNEL_RESIDENT, a forced GPAD_KERNEL_PANEL on f64 or with n or m > 256 (the f64 and the big panels),
 * flat setups, a bound Hessian, caller theta / beta tables in gpad_run_scaled, an infeasibility bound in
 * force together with tol > 0.  Follow-ups, not built: the restart on the resident kernel, in the panel
 * loops, on the pairs and the finisher, together with the certificate, and in groups (gpad_group_* take no
 * options, so a group never runs with the restart on). */
#define GPAD_OPT_RESTART (24)
/* The restarts of every solve of the last run, as the iteration counts are laid out: [batch], after
 * gpad_closed_loop [steps][batch]; a class-bound handle reports them in the caller's order.  Zeros when
 * that run had the restart off, or before any run.  Writes up to cap entries (synchronises the stream) and
 * returns the number written, or GPAD_ERR_INVALID (NULL, cap < 0). */
int gpad_last_restarts(gpad_handle_t h, int* restarts, int cap);

/* Synchronise the handle's stream (for callers using device memory + async runs). */
int gpad_sync(gpad_handle_t h);

#ifdef __cplusplus
}
#endif
#endif /* GPAD_H */
