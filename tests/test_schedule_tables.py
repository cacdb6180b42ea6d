"""Caller theta/beta tables with theta[0] < 1 (gpad_run_scaled; the reference's data-file columns,
main.cu:61-64), on every engine, against the oracle.

Both built-in schedules start at theta[0] = 1, so in every other test the first iteration's 8c,
z = fma(1 - theta[0], z_{-1}, theta[0] zhat), multiplies the caller's z0 by zero, and so does the
violation recursion u = fma(1 - theta[0], u, theta[0] G_L zhat) with its seed u = G_L z_{-1}: neither
the z0 load nor the seed GEMM can reach an asserted value.  A table entered late does both:

* fixed N (tol = 0): z* depends on z0 from the first iteration on -- the z0 load of every engine;
  at N = 1 with y0 = 0, z* = fma(1 - theta[0], z0, theta[0] (-g_P)) is also checked against numpy;
* tol = 1e-4 from z0 = z_f, the generator's strictly feasible point: G z0 - g < 0 in every row, so
  with the right seed test (A) is nominated and passes within a few tests (code 1), while a seed
  that is dropped or wrong in some rows (u + p_D = p_D = -g / L there, positive where g < 0) keeps (A)
  from being nominated for hundreds of iterations -- the seed sites of every engine.

The tables: the default schedule entered s iterations late, theta[v] = theta_std[v + s] (the
schedule of a solve that was interrupted and resumed), and a table of arbitrary values in (0, 1).
f32 results are bit-identical to the oracle's; f64 counts and codes are equal and z*, y* agree to
1e-11 norm-relative (and the f64 panels equal the f64 stream kernel bit for bit).

Where each seed u = G_L z_{-1} and z0 load is observed (the engine that ran is st["kernel"], with the
option that selects the variant):

* gpad_stream.hip (f32 and f64): test_seed[*-stream], test_seed_f64 ("stream");
  gpad_resident.hip: test_seed[*-resident] ("resident");
* gpad_panel.hip small panels (T <= 8): test_seed[37x53-panel]; gpad_pairs.hip panel pairs (T > 8), one panel per
  workgroup: test_seed[*-panel-onepanel]; pair layout (panel_max_grid = 2 for three panels):
  test_seed[*-panel-pair] and test_seed_mixed_batches, whose case (iii) depends on the per-wave znz
  flags being combined ("panel");
* gpad_bigpanel.hip: test_seed[300x280-bigpanel] ("panel", n, m > 256);
* gpad_flatpanel.hip (operand staging and GEMM), gpad_flat.hip, the flat resident chains:
  test_flat_seed[*-panels*], [*-lds], [*-chains] ("flat"; gpad_phase_counts has entries for the panels only);
* gpad_panel64.hip first columns: test_seed_f64 ("panel", p64_relay 1 and 0); refilled columns:
  test_seed_f64_refilled_columns (differs from the p64_refill = 0 run if that seed is wrong);
* every engine's z0 load: test_fixed_n_z0_load / test_flat_fixed_n_z0_load;
* not reachable through a caller table: gpad_duo.hip's fresh start (gpad_run launches the duo finisher
  only for phases after the first, v_begin > 0; it starts fresh only inside the closed-loop kernel)
  and gpad_loop.h (gpad_closed_loop takes no table) -- DESIGN.md section 5b.

test_inputs_depend_on_the_start (CPU) keeps the tol > 0 inputs meaningful on the oracle alone: at
least half of the instances with z0 != 0 end with code 1, and at least half of them end at another
iteration count from z0 = 0.
"""
from __future__ import annotations

import functools
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import pytest

SEED = 21          # problems.synthetic_qp seed of every case
TOL = 1e-4
NMAX = 3000        # iteration cap of the tol > 0 cases
S_FIXED = 7        # the shifted table of the fixed-N cases
F32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))  # noqa: E731
F64 = lambda a: np.ascontiguousarray(np.asarray(a, np.float64))  # noqa: E731


@functools.lru_cache(maxsize=None)
def orc():
    import pyoracle
    return pyoracle.Oracle()


def pmap(fn, items):
    """fn over items on a few threads (the oracle's C solves release the GIL)."""
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(fn, items))


# ------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def problem(n, m, B, shared=True, f64=False):
    """synthetic_qp(n, m, B, seed 21) in the scaled form gpad_setup_scaled / gpad_run_scaled take
    (MGneg = -ML, GL = G / L, PD = -g / L; oracle.scale's roundings in f32, acceldualgrad.m:22-23's in
    f64), the unscaled f64-oracle inputs, H, and zf [B][n]: every instance's strictly feasible point
    (the generator's first draw of its right-hand side)."""
    from gpad_mpc import problems
    O = orc()
    qp = problems.synthetic_qp(n, m, batch=B, seed=SEED, shared=shared)
    p = SimpleNamespace(n=n, m=m, B=B, shared=shared, f64=f64)
    if f64:
        p.ML, p.G, p.M, p.g, p.L = F64(qp.ML), F64(qp.G), F64(qp.M).reshape(B, n), F64(qp.g).reshape(B, m), float(qp.L)
        p.H = F64(qp.H)
        p.MGneg, p.GL, p.PD = -p.ML, (1.0 / p.L) * p.G, (-1.0 / p.L) * p.g
    else:
        ML, G, g = F32(qp.ML), F32(qp.G), F32(qp.g).reshape(B, m)
        p.M, p.L = F32(qp.M).reshape(B, n), np.float32(qp.L)
        if shared:
            p.MGneg, p.GL, _ = O.scale(ML, G, g[0], p.L)
        else:
            sc = [O.scale(ML[b], G[b], g[b], p.L) for b in range(B)]
            p.MGneg, p.GL = np.stack([a[0] for a in sc]), np.stack([a[1] for a in sc])
        p.PD = np.ascontiguousarray(O.scale_vec(g, p.L))
        p.g = g
    if shared:
        zf = np.stack([np.random.default_rng(SEED + 1 + b).uniform(-0.5, 0.5, n) for b in range(B)])
        G64, g64 = np.asarray(qp.G), np.asarray(qp.g).reshape(B, m)
        assert ((zf @ G64.T - g64).max(axis=1) < -0.09).all(), "zf is not the generator's feasible point"
        p.zf = F64(zf) if f64 else F32(zf)
    for a in vars(p).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def tables(kind, N, f64=False, schedule=0):
    """'shiftS': the schedule entered S iterations late; 'arb': arbitrary values in (0, 1) with
    theta[0] = 0.3 (beta < 1 keeps 8a an extrapolation); 'default': the schedule itself."""
    O = orc()
    if kind == "arb":
        rng = np.random.default_rng(1234)
        th, be = rng.uniform(0.05, 0.95, N), rng.uniform(0.0, 0.9, N)
        th[0] = 0.3
    else:
        s = 0 if kind == "default" else int(kind[5:])
        th, be = O.schedule(N + s, schedule)
        th, be = th[s:], be[s:]
    out = tuple((F64 if f64 else F32)(t) for t in (th, be))
    for t in out:
        t.setflags(write=False)
    return out


def random_z0(B, n, f64=False):
    z0 = np.random.default_rng(77).uniform(-0.5, 0.5, (B, n))
    return F64(z0) if f64 else F32(z0)


def oracle_solves(p, z0, N, tol, K, th, be, H=None, pick=None):
    """(z*, y*, iterations, codes) of p's instances `pick` (default: z0's rows) from z0, y0 = 0, one
    oracle solve each with the tables th / be."""
    O = orc()
    pick = list(range(z0.shape[0])) if pick is None else list(pick)

    def one(b):
        if p.f64:
            if H is not None:
                return O.solve_value_f64(z0[b], np.zeros(p.m), p.ML, p.M[b], p.G, p.g[b], H, N, p.L, tol, K,
                                         theta=th, beta=be)
            return O.solve_f64(z0[b], np.zeros(p.m), p.ML, p.M[b], p.G, p.g[b], N, p.L, tol, K, theta=th, beta=be,
                               code=True)
        mg, gl = (p.MGneg, p.GL) if p.shared else (p.MGneg[b], p.GL[b])
        return O.solve_scaled_f32(z0[b], np.zeros(p.m), mg, p.M[b], gl, p.PD[b], N, p.L, tol, K, theta=th, beta=be,
                                  code=True)
    r = pmap(one, pick)
    out = (np.stack([a[0] for a in r]), np.stack([a[1] for a in r]), np.array([a[2] for a in r], np.int32),
           np.array([a[3] for a in r], np.int32))
    for a in out:
        a.setflags(write=False)
    return out


# The tol > 0 cases: (shape, batch, shift, test period).  Every one (the mixed and the flat ones below
# too) was chosen with a scratch copy of the oracle whose seed lines write 0 (never committed): it ends
# each seeded instance that the oracle ends with code 1 at another (iterations, code), most of them
# with code 2 after 230-500 iterations instead of code 1 at 10-30.
# The three pair-kernel shapes hold 40 instances: three panels, the last ragged, which two workgroups
# run as a pair and a single panel (the pair layout) and three workgroups one each; resident and stream
# run the first SEED_B_SMALL of them.
SEED_CASES = {"136x136": (136, 136, 40, 30, 10), "200x200": (200, 200, 40, 30, 10), "208x180": (208, 180, 40, 30, 10),
              "300x280": (300, 280, 16, 30, 10), "37x53": (37, 53, 16, 10, 1)}
SEED_B_SMALL = 16
MIXED_SHAPE, MIXED_B, MIXED_S, MIXED_K = (200, 200), 48, 30, 10
F64_CASES = {"136x136": (136, 136, 40, 30, 10), "40x64": (40, 64, 40, 30, 10)}


@functools.lru_cache(maxsize=None)
def masked_start(b, lo=64, margin=0.3):
    """A strictly feasible z0 of the mixed shape's instance b that is zero in components < lo: the
    minimum-norm x with G[:, lo:] x <= g - margin, solved by the fp64 oracle itself (GPAD on H = I)."""
    n, m = MIXED_SHAPE
    p = problem(n, m, MIXED_B, f64=True)
    G2 = np.ascontiguousarray(p.G[:, lo:])
    ML = np.ascontiguousarray(G2.T)
    x, _, _, conv = orc().solve_f64(np.zeros(n - lo), np.zeros(m), ML, np.zeros(n - lo), G2, p.g[b] - margin, 20000,
                                    float(np.linalg.norm(G2 @ ML, "fro")), 1e-3)
    z0 = np.zeros(n)
    z0[lo:] = x
    assert conv and (p.G @ z0 - p.g[b]).max() < -0.25
    return F32(z0)


@functools.lru_cache(maxsize=None)
def mixed_start(kind):
    """z0 [48][200] of the mixed batches: (i) only instance 5 is seeded; (ii) every instance of the
    second panel and none of the first (nor the third); (iii) eight instances of the second panel
    start from a feasible point that is zero in components < 64 -- in the panel-pair kernel those are
    the rows of waves 0..3, whose own rows are then all zero while the seed GEMM is still needed."""
    n, m = MIXED_SHAPE
    p = problem(n, m, MIXED_B)
    z0 = np.zeros((MIXED_B, n), np.float32)
    if kind == "i":
        z0[5] = p.zf[5]
    elif kind == "ii":
        z0[16:32] = p.zf[16:32]
    else:
        for b in range(16, 24):
            z0[b] = masked_start(b)
    z0.setflags(write=False)
    return z0


@functools.lru_cache(maxsize=None)
def mixed_reference(kind):
    """The mixed batch's oracle solves, assembled from one cold solve of every instance (shared by
    the three batches) and the solves of the seeded ones."""
    n, m = MIXED_SHAPE
    p = problem(n, m, MIXED_B)
    th, be = tables(f"shift{MIXED_S}", NMAX)
    cold = _mixed_cold()
    z0 = mixed_start(kind)
    seeded = np.flatnonzero(np.abs(z0).max(axis=1) > 0)
    warm = oracle_solves(p, z0, NMAX, TOL, MIXED_K, th, be, pick=seeded)
    out = [a.copy() for a in cold]
    for a, w in zip(out, warm):
        a[seeded] = w
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _mixed_cold():
    n, m = MIXED_SHAPE
    p = problem(n, m, MIXED_B)
    th, be = tables(f"shift{MIXED_S}", NMAX)
    return oracle_solves(p, np.zeros((MIXED_B, n), np.float32), NMAX, TOL, MIXED_K, th, be)


# ---- flat battery data ------------------------------------------------------------------------
FLAT_GOLDEN = ["battery_flat_3x4", "battery_flat_4x10"]
FLAT_TOL = {"3x4": (3, 4, 16, 30, 10), "4x10": (4, 10, 16, 30, 10)}  # n_u, horizon, batch, shift, test period


@functools.lru_cache(maxsize=None)
def flat_golden(name, B):
    """The golden's flat plant and its one (g_P, p_D), repeated for B instances."""
    from conftest import load_golden
    gd = load_golden(name)
    rep = lambda v: np.ascontiguousarray(np.tile(v.astype(np.float32), (B, 1)))  # noqa: E731
    return SimpleNamespace(MGf=F32(gd["MGf"]), GLf=F32(gd["GLf"]), GP=rep(gd["gP"]), PD=rep(gd["pD"]),
                           L=np.float32(gd["L"]), n_u=int(gd["n_u"]), n=gd["gP"].size, m=gd["pD"].size, B=B)


@functools.lru_cache(maxsize=None)
def flat_feasible(n_u, Nh, B):
    """The battery plant's flat matrices (problems.flatten_battery of a battery_scenarios batch, its
    g_P per state of charge) with right-hand sides that have a strictly feasible point, as
    synthetic_qp draws them: g = G zf + U(0.1, 1), zf ~ U(-0.5, 0.5).  The battery's own g holds exact
    zeros (no interior point), so on the goldens and on scenario batches no start -- half a previous
    solution included -- lets test (A) pass before test (B): measured 0 of 16 instances with code 1
    and no count that depends on z0, at shifts 10 and 30, tests every 1 and 10 iterations."""
    from gpad_mpc import problems
    qp = problems.battery_scenarios(n_u, Nh, B, seed=SEED)
    MGf, GLf, L = problems.flatten_battery(qp, n_u, Nh)
    rng = np.random.default_rng(SEED)
    zf = rng.uniform(-0.5, 0.5, (B, qp.n))
    g = zf @ np.asarray(qp.G).T + rng.uniform(0.1, 1.0, (B, qp.m))
    L32 = np.float32(L)
    return SimpleNamespace(MGf=F32(MGf), GLf=F32(GLf), GP=F32(qp.M).reshape(B, qp.n),
                           PD=np.ascontiguousarray(orc().scale_vec(F32(g), L32)), L=L32, n_u=n_u, n=qp.n, m=qp.m, B=B,
                           zf=F32(zf))


def flat_oracle_solves(f, z0, N, tol, K, th, be):
    O = orc()
    r = pmap(lambda b: O.solve_flat_f32(z0[b], np.zeros(f.m), f.MGf, f.GP[b], f.GLf, f.PD[b], f.n_u, N, f.L, tol, K,
                                        theta=th, beta=be), range(z0.shape[0]))
    return (np.stack([a[0] for a in r]), np.stack([a[1] for a in r]), np.array([a[2] for a in r], np.int32),
            np.array([a[3] for a in r], np.int32))


@functools.lru_cache(maxsize=None)
def seed_reference(name, f64=False, hessian=False):
    n, m, B, s, K = (F64_CASES if f64 else SEED_CASES)[name]
    p = problem(n, m, B, f64=f64)
    th, be = tables(f"shift{s}", NMAX, f64)
    return oracle_solves(p, p.zf, NMAX, TOL, K, th, be, H=p.H if hessian else None)


@functools.lru_cache(maxsize=None)
def flat_tol_reference(name):
    n_u, Nh, B, s, K = FLAT_TOL[name]
    f = flat_feasible(n_u, Nh, B)
    th, be = tables(f"shift{s}", NMAX)
    return flat_oracle_solves(f, f.zf, NMAX, TOL, K, th, be)


# Both codes in one batch of the row kernels (csrc/gpad_chain.h lists the cases per kernel): eight
# instances of a case above, the even ones from z_f -- test (A) nominated by the recursion, verified on
# the direct chain, code 1 -- and the odd ones from z0 = 0 -- test (B), code 2 -- under the case's table.
BOTH_B = 8


def _both_starts(zf):
    z0 = np.array(zf[:BOTH_B])
    z0[1::2] = 0.0
    z0.setflags(write=False)
    return z0


def _both_codes_checked(what, ref):
    """At least three instances of the oracle's batch end with each code."""
    codes = ref[3]
    assert int((codes == 1).sum()) >= 3 and int((codes == 2).sum()) >= 3, (what, codes.tolist(), ref[2].tolist())
    assert ref[2].max() < NMAX


@functools.lru_cache(maxsize=None)
def both_codes_reference(name):
    n, m, Bp, s, K = SEED_CASES[name]
    p = problem(n, m, Bp)
    th, be = tables(f"shift{s}", NMAX)
    z0 = _both_starts(p.zf)
    return z0, oracle_solves(p, z0, NMAX, TOL, K, th, be)


@functools.lru_cache(maxsize=None)
def flat_both_codes_reference(name):
    n_u, Nh, B, s, K = FLAT_TOL[name]
    f = flat_feasible(n_u, Nh, B)
    th, be = tables(f"shift{s}", NMAX)
    z0 = _both_starts(f.zf)
    return z0, flat_oracle_solves(f, z0, NMAX, TOL, K, th, be)


# ------------------------------------------------------------------------------------ CPU
def test_f64_table_entries_return_the_schedule_entries_bits(oracle):
    """orc_solve_tables_f64 / orc_solve_value_tables_f64 with orc_schedule's tables return the bits of
    orc_solve_f64 / orc_solve_value_f64, fixed N and to a tolerance, both schedules."""
    p = problem(40, 64, 40, f64=True)
    z0 = p.zf[3]
    for kind in (0, 1):
        for N, tol in ((37, 0.0), (2000, 1e-4)):
            th, be = oracle.schedule(N, kind)
            for H in (None, p.H):
                if H is None:
                    a = oracle.solve_f64(z0, np.zeros(64), p.ML, p.M[3], p.G, p.g[3], N, p.L, tol, schedule=kind, code=True)
                    b = oracle.solve_f64(z0, np.zeros(64), p.ML, p.M[3], p.G, p.g[3], N, p.L, tol, theta=th, beta=be,
                                         code=True)
                else:
                    a = oracle.solve_value_f64(z0, np.zeros(64), p.ML, p.M[3], p.G, p.g[3], H, N, p.L, tol, schedule=kind)
                    b = oracle.solve_value_f64(z0, np.zeros(64), p.ML, p.M[3], p.G, p.g[3], H, N, p.L, tol, theta=th,
                                               beta=be)
                assert a[2:] == b[2:] and (tol == 0.0 or a[3] > 0)
                np.testing.assert_array_equal(a[0], b[0])
                np.testing.assert_array_equal(a[1], b[1])
    with pytest.raises(ValueError):
        oracle.solve_f64(z0, np.zeros(64), p.ML, p.M[3], p.G, p.g[3], 5, p.L, theta=np.ones(5))


def test_f32_code_keyword_keeps_the_existing_return(oracle):
    p = problem(37, 53, 16)
    th, be = tables("shift10", NMAX)
    args = (p.zf[0], np.zeros(53), p.MGneg, p.M[0], p.GL, p.PD[0], NMAX, p.L, TOL, 1)
    a = oracle.solve_scaled_f32(*args, theta=th, beta=be)
    b = oracle.solve_scaled_f32(*args, theta=th, beta=be, code=True)
    assert a[3] is True and b[3] in (1, 2) and a[2] == b[2]
    np.testing.assert_array_equal(a[0], b[0])


def _shares(name, codes, its, its_cold, seeded):
    k = int(seeded.sum())
    a, b = int((codes[seeded] == 1).sum()), int((its[seeded] != its_cold[seeded]).sum())
    print(f"{name}: {k} seeded, (a) code 1: {a}/{k}, (b) count differs from z0 = 0: {b}/{k}, "
          f"iterations {its.min()}..{its.max()}")
    assert k > 0 and 2 * a >= k, f"{name}: only {a} of {k} seeded instances end with code 1"
    assert 2 * b >= k, f"{name}: only {b} of {k} seeded instances depend on z0"
    assert its.max() < NMAX and its_cold.max() < NMAX


def test_inputs_depend_on_the_start(oracle):
    """Conditions (a) and (b) of the module docstring for every tol > 0 case of the GPU tests, on the
    oracle alone."""
    for name, (n, m, B, s, K) in SEED_CASES.items():
        p = problem(n, m, B)
        th, be = tables(f"shift{s}", NMAX)
        _, _, its, codes = seed_reference(name)
        cold = oracle_solves(p, np.zeros((B, n), np.float32), NMAX, TOL, K, th, be)
        _shares(f"f32 {name} s={s} K={K}", codes, its, cold[2], np.ones(B, bool))
    for kind in ("i", "ii", "iii"):
        z0 = mixed_start(kind)
        seeded = np.abs(z0).max(axis=1) > 0
        _, _, its, codes = mixed_reference(kind)
        _shares(f"mixed ({kind})", codes, its, _mixed_cold()[2], seeded)
        # the cold instances run on through several phases of 20 iterations
        assert (its[~seeded] > 100).all()
        if kind == "iii":  # a seed left at zero in the rows of waves 0..3 would sit above the tolerance
            p = problem(*MIXED_SHAPE, MIXED_B)
            assert (z0[seeded][:, :64] == 0).all() and (np.abs(z0[seeded][:, 64:]).max(axis=1) > 0).all()
            assert (p.g[seeded][:, :64].min(axis=1) < 0).all()
    for name, (n_u, Nh, B, s, K) in FLAT_TOL.items():
        f = flat_feasible(n_u, Nh, B)
        th, be = tables(f"shift{s}", NMAX)
        _, _, its, codes = flat_tol_reference(name)
        cold = flat_oracle_solves(f, np.zeros((B, f.n), np.float32), NMAX, TOL, K, th, be)
        _shares(f"flat {name} s={s} K={K}", codes, its, cold[2], np.ones(B, bool))
    for name, (n, m, B, s, K) in F64_CASES.items():
        p = problem(n, m, B, f64=True)
        th, be = tables(f"shift{s}", NMAX, True)
        for hessian in (False, True):
            _, _, its, codes = seed_reference(name, True, hessian)
            cold = oracle_solves(p, np.zeros((B, n)), NMAX, TOL, K, th, be, H=p.H if hessian else None)
            _shares(f"f64 {name} hessian={hessian}", codes, its, cold[2], np.ones(B, bool))


# ------------------------------------------------------------------------------------ GPU
KERNELS = {"auto": 0, "stream": 1, "resident": 2, "panel": 3}


def gpu_solve(p, B, kernel, z0, N, tol, K, th, be, *, opts=None, hessian=False, schedule=0, solver=None):
    """One run on p's first B instances from z0, y0 = 0 through gpad_setup_scaled / gpad_run_scaled
    (host arrays); returns (z, y, iterations, codes, stats).  `solver`: a handle set up already."""
    import gpad_mpc
    dt = np.float64 if p.f64 else np.float32
    z, y = np.ascontiguousarray(z0[:B], dt).copy(), np.zeros((B, p.m), dt)
    its, codes = np.full(B, -1, np.int32), np.full(B, -1, np.int32)
    s = solver or gpad_mpc.GpadSolver(0)
    try:
        if solver is None:
            mg, gl = (p.MGneg, p.GL) if p.shared else (p.MGneg[:B], p.GL[:B])
            s.setup(np.ascontiguousarray(mg), np.ascontiguousarray(gl), float(p.L), n=p.n, m=p.m, batch=B,
                    shared=p.shared, schedule=schedule, check_every=K, kernel=KERNELS[kernel], scaled=True)
            if hessian:
                s.setup_hessian(p.H)
            s.set_options(**(opts or {}))
        st = s.run(z, y, np.ascontiguousarray(p.M[:B]), np.ascontiguousarray(p.PD[:B]), N, tol, scaled=True,
                   theta=None if th is None else np.ascontiguousarray(th[:N]),
                   beta=None if be is None else np.ascontiguousarray(be[:N]), iters=its, codes=codes)
    finally:
        if solver is None:
            s.close()
    return z, y, its, codes, st


def same(got, ref, what, f64=False, counts=True):
    """got = (z, y, iterations, codes, ...) against the oracle's (z, y, iterations, codes)."""
    B = got[0].shape[0]
    if counts:
        bad = np.flatnonzero((got[2] != ref[2][:B]) | (got[3] != ref[3][:B]))
        assert bad.size == 0, (f"{what}: (iterations, code) differ at {bad[:8]}: "
                               f"{list(zip(got[2][bad[:8]], got[3][bad[:8]]))} vs oracle "
                               f"{list(zip(ref[2][bad[:8]], ref[3][bad[:8]]))}")
    for name, a, r in (("z", got[0], ref[0][:B]), ("y", got[1], ref[1][:B])):
        if f64:
            e = np.linalg.norm(a - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-300)
            assert e.max() <= 1e-11, f"{what} {name}: norm-relative {e.max():.3g} at instance {int(e.argmax())}"
        elif not np.array_equal(a, r):
            d = np.abs(a.astype(np.float64) - r.astype(np.float64))
            rows = np.flatnonzero(d.max(axis=1) > 0)
            raise AssertionError(f"{what} {name}: {rows.size} of {B} instances differ (first {rows[:8]}), "
                                 f"max |d| = {d.max():.3g}")


def closed_form_n1(p, B, z0, th):
    """N = 1 from y0 = 0: w = 0, every 8b chain is +0, zhat = -g_P, and 8c is one fma: fp64 numpy
    on the f32 operands.  The product (1 - theta) z0 is exact in fp64, but the sum is rounded to fp64
    and then to f32 -- twice, where the fma rounds once; the two differ only when the fp64 sum falls
    within 2^-29 relative of an f32 tie, which no input used here does
    (test_fixed_n_closed_form_on_the_oracle)."""
    omt = np.float32(1.0) - np.float32(th[0])
    t = np.float32(th[0]) * (-p.M[:B])  # the oracle's rounded product theta * zhat
    return (np.float64(omt) * z0[:B].astype(np.float64) + t.astype(np.float64)).astype(np.float32)


FIXED_N = (1, 2, 25)
FIXED_TABLES = (f"shift{S_FIXED}", "arb")
FIXED_SHAPES = [(1, 5), (5, 1), (37, 53), (65, 129), (136, 136), (200, 200), (208, 180)]
FIXED_BMAX = 35


@functools.lru_cache(maxsize=None)
def fixed_reference(n, m, B, shared, table, N):
    p = problem(n, m, B, shared)
    th, be = tables(table, N)
    return oracle_solves(p, random_z0(B, n), N, 0.0, 10, th, be)


def _fixed_cases():
    for n, m in FIXED_SHAPES:
        for kernel in ("stream", "resident", "panel"):
            for B in (1, 19) + ((35,) if kernel == "panel" else ()):
                yield pytest.param(n, m, B, True, kernel, id=f"{n}x{m}-{kernel}-B{B}")
    yield pytest.param(300, 280, 20, True, "panel", id="300x280-bigpanel-B20")
    yield pytest.param(37, 53, 5, False, "stream", id="37x53-perinstance-stream-B5")
    yield pytest.param(37, 53, 5, False, "resident", id="37x53-perinstance-resident-B5")


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,B,shared,kernel", list(_fixed_cases()))
def test_fixed_n_z0_load(gpu, oracle, n, m, B, shared, kernel):
    """Fixed N in {1, 2, 25} under a shifted and an arbitrary table from a random z0 that differs per
    instance: z*, y* bit-identical to the oracle, on one handle (six runs, six tables).  The panel
    cases of 35 instances (three panels) run twice: one panel per workgroup, and on one workgroup
    (panel_max_grid = 1), which on the pair kernel (n or m > 128) is the pair layout -- a pair and a
    single panel -- and on the smaller panels a workgroup walking its panels."""
    import gpad_mpc
    Bp = FIXED_BMAX if (shared and (n, m) != (300, 280)) else B
    p = problem(n, m, Bp, shared)
    z0 = random_z0(Bp, n)
    with gpad_mpc.GpadSolver(0) as s:
        mg, gl = (p.MGneg, p.GL) if shared else (p.MGneg[:B], p.GL[:B])
        s.setup(np.ascontiguousarray(mg), np.ascontiguousarray(gl), float(p.L), n=n, m=m, batch=B, shared=shared,
                kernel=KERNELS[kernel], scaled=True)
        for grid in ((0, 1) if (kernel == "panel" and B == FIXED_BMAX) else (None,)):
            if grid is not None:
                s.set_option("panel_max_grid", grid)
            for table in FIXED_TABLES:
                for N in FIXED_N:
                    th, be = tables(table, N)
                    got = gpu_solve(p, B, kernel, z0, N, 0.0, 10, th, be, solver=s)
                    what = f"{table} N={N} grid cap {grid}"
                    assert got[4]["kernel"] == kernel
                    assert (got[2] == N).all() and (got[3] == 0).all()
                    same(got, fixed_reference(n, m, Bp, shared, table, N), what, counts=False)
                    if N == 1:
                        np.testing.assert_array_equal(got[0], closed_form_n1(p, B, z0, th), err_msg=f"{what} closed form")


def test_fixed_n_closed_form_on_the_oracle(oracle):
    """The N = 1 closed form agrees with the oracle (CPU): the check above is not vacuous."""
    p = problem(37, 53, FIXED_BMAX)
    z0 = random_z0(FIXED_BMAX, 37)
    for table in FIXED_TABLES:
        th, _ = tables(table, 1)
        ref = fixed_reference(37, 53, FIXED_BMAX, True, table, 1)
        np.testing.assert_array_equal(ref[0], closed_form_n1(p, FIXED_BMAX, z0, th))
        assert not np.array_equal(ref[0], -p.M)  # z0 is in z*


def flat_solve(f, B, kernel, opts, z0, N, tol, K, th, be):
    import gpad_mpc
    z, y = z0[:B].copy(), np.zeros((B, f.m), np.float32)
    its, codes = np.full(B, -1, np.int32), np.full(B, -1, np.int32)
    with gpad_mpc.GpadSolver(0) as s:
        s.setup_flat(f.MGf, f.GLf, float(f.L), n_u=f.n_u, batch=B, kernel=kernel, check_every=K)
        s.set_options(**opts)
        st = s.run(z, y, np.ascontiguousarray(f.GP[:B]), np.ascontiguousarray(f.PD[:B]), N, tol, scaled=True,
                   theta=np.ascontiguousarray(th[:N]), beta=np.ascontiguousarray(be[:N]), iters=its, codes=codes)
        # gpad_phase_counts reports entries only after a tol > 0 solve on the flat panels (their phase
        # workspace): the one thing that tells the flat engines apart, st["kernel"] being "flat" for all
        import ctypes
        phase_entries = s.lib.gpad_phase_counts(s.h, (ctypes.c_int * 64)(), 64)
    return z, y, its, codes, st, phase_entries


# register-resident flat chains (AUTO at these sizes), the LDS flat kernel (STREAM), the flat panels
FLAT_ENGINES = {"chains": (0, {}), "lds": (1, {}), "panels": (0, {"flat_panel_min": 0})}


@pytest.mark.gpu
@pytest.mark.parametrize("engine", list(FLAT_ENGINES))
@pytest.mark.parametrize("B", [1, 19])
@pytest.mark.parametrize("name", FLAT_GOLDEN)
def test_flat_fixed_n_z0_load(gpu, oracle, name, B, engine):
    """The flat engines at fixed N.  Every flat engine reports st["kernel"] == "flat" and a fixed-N run
    leaves no other trace, so here the kernel / flat_panel_min setting alone says which engine ran;
    test_flat_seed shows for the same settings and plant sizes that the flat panels take them."""
    f = flat_golden(name, 19)
    z0 = random_z0(19, f.n)
    kernel, opts = FLAT_ENGINES[engine]
    for table in FIXED_TABLES:
        for N in FIXED_N:
            th, be = tables(table, N)
            got = flat_solve(f, B, kernel, opts, z0, N, 0.0, 10, th, be)
            assert got[4]["kernel"] == "flat" and (got[2] == N).all()
            ref = flat_oracle_solves(f, z0[:B], N, 0.0, 10, th, be)
            same(got, ref, f"{table} N={N}", counts=False)
            if N == 1:  # (f.GP plays p.M's part)
                cf = closed_form_n1(SimpleNamespace(M=f.GP), B, z0, th)
                np.testing.assert_array_equal(got[0], cf, err_msg=f"{table} closed form")


@pytest.mark.gpu
@pytest.mark.parametrize("engine", list(FLAT_ENGINES) + ["panels-phased"])
@pytest.mark.parametrize("name", list(FLAT_TOL))
def test_flat_seed(gpu, oracle, name, engine):
    """tol = 1e-4 from the feasible point on the flat engines (flat_feasible's data): counts, codes,
    z*, y* of every instance.  panels-phased: phases of 20 iterations forced (phased = 2)."""
    n_u, Nh, B, s, K = FLAT_TOL[name]
    f = flat_feasible(n_u, Nh, B)
    th, be = tables(f"shift{s}", NMAX)
    kernel, opts = FLAT_ENGINES[engine.split("-")[0]]
    if engine == "panels-phased":
        opts = dict(opts, phased=2, phase_len=20)
    got = flat_solve(f, B, kernel, opts, f.zf, NMAX, TOL, K, th, be)
    assert got[4]["kernel"] == "flat"
    assert (got[5] > 0) == engine.startswith("panels"), (engine, got[5])
    same(got, flat_tol_reference(name), f"flat {name} {engine}")


# panel_max_grid, as tests/test_panel_loop_diet.py: the pair kernel pairs its panels when there are more
# of them than workgroups -- 2 workgroups for the 3 panels of a batch of 40 or 48; no cap: one panel each
LAYOUTS = {"pair": 2, "onepanel": 0}


def _seed_cases():
    for name in ("136x136", "200x200", "208x180"):
        for layout in LAYOUTS:
            yield pytest.param(name, "panel", {"panel_max_grid": LAYOUTS[layout]}, id=f"{name}-panel-{layout}")
        yield pytest.param(name, "resident", {}, id=f"{name}-resident")
        yield pytest.param(name, "stream", {}, id=f"{name}-stream")
    yield pytest.param("300x280", "panel", {}, id="300x280-bigpanel")
    yield pytest.param("300x280", "stream", {}, id="300x280-stream")
    for kernel in ("panel", "resident", "stream"):
        yield pytest.param("37x53", kernel, {}, id=f"37x53-{kernel}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,kernel,opts", list(_seed_cases()))
def test_seed(gpu, oracle, name, kernel, opts):
    """tol = 1e-4 from z0 = z_f under the shifted table: counts, codes, z*, y* of every instance."""
    n, m, Bp, s, K = SEED_CASES[name]
    p = problem(n, m, Bp)
    B = Bp if kernel == "panel" else min(Bp, SEED_B_SMALL)
    if "panel_max_grid" in opts:  # the layouts differ only with more panels than the capped grid
        assert (B + 15) // 16 > 2
    th, be = tables(f"shift{s}", NMAX)
    got = gpu_solve(p, B, kernel, p.zf, NMAX, TOL, K, th, be, opts=opts)
    assert got[4]["kernel"] == kernel
    same(got, seed_reference(name), f"{name} {kernel}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,kernel", [("37x53", "stream"), ("37x53", "resident"), ("136x136", "resident")],
                         ids=["37x53-stream", "37x53-resident", "136x136-resident"])
def test_both_codes_in_one_batch(gpu, oracle, name, kernel):
    """The row kernels on one batch that the oracle ends with code 1 and with code 2 (test_seed's
    instances all end with code 1 on them): stage 1, the verification of a nominated (A) and both codes
    in one launch.  Counts, codes, z*, y* bit-identical to the oracle."""
    n, m, Bp, s, K = SEED_CASES[name]
    z0, ref = both_codes_reference(name)
    _both_codes_checked(name, ref)
    th, be = tables(f"shift{s}", NMAX)
    got = gpu_solve(problem(n, m, Bp), BOTH_B, kernel, z0, NMAX, TOL, K, th, be)
    assert got[4]["kernel"] == kernel
    same(got, ref, f"both codes {name} {kernel}")


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["lds", "chains"])
def test_flat_both_codes_in_one_batch(gpu, oracle, engine):
    """As test_both_codes_in_one_batch on the LDS flat kernel and the register-resident flat chains
    (flat 3x4; test_flat_seed's instances all end with code 1 on them)."""
    n_u, Nh, _, s, K = FLAT_TOL["3x4"]
    z0, ref = flat_both_codes_reference("3x4")
    _both_codes_checked("flat 3x4", ref)
    th, be = tables(f"shift{s}", NMAX)
    kernel, opts = FLAT_ENGINES[engine]
    got = flat_solve(flat_feasible(n_u, Nh, FLAT_TOL["3x4"][2]), BOTH_B, kernel, opts, z0, NMAX, TOL, K, th, be)
    assert got[4]["kernel"] == "flat" and got[5] == 0
    same(got, ref, f"flat both codes 3x4 {engine}")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kind", ["i", "ii", "iii"])
def test_seed_mixed_batches(gpu, oracle, kind, layout):
    """Seeded and cold instances in one batch of 48 on the panel pairs (the per-wave test that skips
    the seed GEMM of an all-cold panel), in phases of 20 iterations with the duo finisher taking the
    last survivors: the cold instances cross phase boundaries under the caller's table."""
    n, m = MIXED_SHAPE
    p = problem(n, m, MIXED_B)
    th, be = tables(f"shift{MIXED_S}", NMAX)
    z0 = mixed_start(kind)
    import gpad_mpc
    with gpad_mpc.GpadSolver(0) as s:
        s.setup(p.MGneg, p.GL, float(p.L), n=n, m=m, batch=MIXED_B, check_every=MIXED_K, kernel=KERNELS["panel"],
                scaled=True)
        # plan = 0: uniform phases of 20 (no plan from an earlier solve of the shape); finish_thresh = 16: the
        # panels carry the survivors over several boundaries before the finisher
        s.set_options(phased=2, phase_len=20, plan=0, finish_thresh=16, panel_max_grid=LAYOUTS[layout])
        got = gpu_solve(p, MIXED_B, "panel", z0, NMAX, TOL, MIXED_K, th, be, solver=s)
        phases = s.last_phases()
    assert got[4]["kernel"] == "panel"
    assert len(phases["ends"]) > 2 and phases["ends"][0] == 20, phases
    # carried panel phases first, then the finisher: both run under the caller's table
    assert phases["takeover"] is not None and phases["takeover"]["phase"] > 2, phases
    same(got, mixed_reference(kind), f"mixed ({kind}) {layout}")


def _f64_cases():
    for name in F64_CASES:
        for hessian in (False, True):
            yield pytest.param(name, hessian, {}, id=f"{name}-{'H' if hessian else 'noH'}")
    yield pytest.param("136x136", False, {"p64_relay": 0}, id="136x136-noH-relay0")
    yield pytest.param("136x136", True, {"p64_relay": 0}, id="136x136-H-relay0")


@pytest.mark.gpu
@pytest.mark.parametrize("name,hessian,opts", list(_f64_cases()))
def test_seed_f64(gpu, oracle, name, hessian, opts):
    """f64: the stream kernel and the f64 panels from z0 = z_f under the shifted table, with and without
    the Hessian bound: counts and codes equal to the fp64 oracle, z*, y* to 1e-11; panels bit-identical
    to the stream kernel."""
    n, m, B, s, K = F64_CASES[name]
    p = problem(n, m, B, f64=True)
    th, be = tables(f"shift{s}", NMAX, True)
    ref = seed_reference(name, True, hessian)
    a = gpu_solve(p, B, "panel", p.zf, NMAX, TOL, K, th, be, opts=opts, hessian=hessian)
    b = gpu_solve(p, B, "stream", p.zf, NMAX, TOL, K, th, be, hessian=hessian)
    assert a[4]["kernel"] == "panel" and b[4]["kernel"] == "stream"
    same(b, ref, f"f64 {name} stream", f64=True)
    same(a, ref, f"f64 {name} panel", f64=True)
    for x, y_ in zip(a[:4], b[:4]):
        np.testing.assert_array_equal(x, y_)


@pytest.mark.gpu
def test_seed_f64_both_codes_in_one_panel(gpu, oracle):
    """The f64 panels on one panel that the oracle ends with code 1 and with code 2 (test_seed_f64's
    instances all end with code 1): stage 1, the verification GEMM and the code selection in one
    workgroup, with the Hessian bound (the value-function branches read stage 1's parts).  Sixteen
    instances of the 40x64 case, the even ones from z_f -- test (A) within two tests -- and the odd ones
    from z0 = 0 -- test (B).  Counts and codes equal to the fp64 oracle, z*, y* to 1e-11, bit-identical
    to the f64 stream kernel."""
    n, m, _, s, K = F64_CASES["40x64"]
    p = problem(n, m, 40, f64=True)
    th, be = tables(f"shift{s}", NMAX, True)
    z0 = np.array(p.zf[:16])
    z0[1::2] = 0.0
    ref = oracle_solves(p, z0, NMAX, TOL, K, th, be, H=p.H)
    assert (ref[3][0::2] == 1).all() and (ref[3][1::2] == 2).all(), ref[3]
    a = gpu_solve(p, 16, "panel", z0, NMAX, TOL, K, th, be, hessian=True)
    b = gpu_solve(p, 16, "stream", z0, NMAX, TOL, K, th, be, hessian=True)
    assert a[4]["kernel"] == "panel" and b[4]["kernel"] == "stream"
    same(a, ref, "f64 mixed panel", f64=True)
    for x, y_ in zip(a[:4], b[:4]):
        np.testing.assert_array_equal(x, y_)


@pytest.mark.gpu
def test_seed_f64_refilled_columns(gpu, oracle):
    """More f64 panels than workgroups with N a multiple of the test period: columns that finish take
    the next instances, whose seed is the refill path's GEMM over the new columns, here with
    z0 = z_f != 0 and theta[0] < 1.  (The f64 panels' grid follows the device's occupancy and takes no
    cap from panel_max_grid, so the batch is sized past two workgroups on every CU of the device; the
    library reports no refill count, the sizing is the evidence.)  Bit-identical to the
    run without refills and to the f64 stream kernel; a sample equal to the fp64 oracle."""
    import torch
    n, m, _, s, K = F64_CASES["136x136"]
    # n = m = 136 runs the 1024-thread relay layout: at most two workgroups fit a CU (2048 threads), and
    # columns are refilled when there are more panels than resident workgroups (launch_p64)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 16 * (2 * cus + 8)
    p = problem(n, m, B, f64=True)
    th, be = tables(f"shift{s}", NMAX, True)
    a = gpu_solve(p, B, "panel", p.zf, NMAX, TOL, K, th, be)
    b = gpu_solve(p, B, "panel", p.zf, NMAX, TOL, K, th, be, opts={"p64_refill": 0})
    c = gpu_solve(p, B, "stream", p.zf, NMAX, TOL, K, th, be)
    assert a[4]["kernel"] == "panel" and b[4]["kernel"] == "panel" and c[4]["kernel"] == "stream"
    for x, y_, w in zip(a[:4], b[:4], c[:4]):
        np.testing.assert_array_equal(x, y_)
        np.testing.assert_array_equal(x, w)
    pick = sorted(set(list(range(0, B, 397)) + [B - 1, int(np.argmax(a[2])), int(np.argmin(a[2]))]))
    ref = oracle_solves(p, p.zf, NMAX, TOL, K, th, be, pick=pick)
    same(tuple(x[pick] for x in a[:4]), ref, "f64 refill sample", f64=True)
    assert 2 * int((a[3] == 1).sum()) >= B  # test (A) from the seed, as in the small cases


# ---- table caching: default, custom A, custom B, default on one handle at one N ---------------
def _caching_run(p, B, kernel, schedule, N, z0):
    import gpad_mpc
    f64 = p.f64
    seq = [("default", None), ("custom A", tables(f"shift{S_FIXED}", N, f64)), ("custom B", tables("arb", N, f64)),
           ("default again", None)]
    with gpad_mpc.GpadSolver(0) as s:
        s.setup(p.MGneg, p.GL, float(p.L), n=p.n, m=p.m, batch=B, schedule=schedule, kernel=KERNELS[kernel], scaled=True)
        for what, tab in seq:
            th, be = tab if tab is not None else (None, None)
            got = gpu_solve(p, B, kernel, z0, N, 0.0, 10, th, be, solver=s)
            assert got[4]["kernel"] == kernel
            rt = tab if tab is not None else tables("default", N, f64, schedule)
            ref = oracle_solves(p, z0[:B], N, 0.0, 10, rt[0], rt[1])
            same(got, ref, f"{what} (schedule {schedule})", f64=f64, counts=False)


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", [0, 1])
@pytest.mark.parametrize("kernel", ["stream", "resident", "panel"])
def test_table_caching(gpu, oracle, kernel, schedule):
    """A custom table must not be reused by the next run (another custom table of the same length, or
    the schedule of dims.schedule): every run equals the oracle under its own table."""
    p = problem(37, 53, FIXED_BMAX)
    _caching_run(p, 19, kernel, schedule, 25, random_z0(FIXED_BMAX, 37))


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", [0, 1])
@pytest.mark.parametrize("kernel", ["stream", "panel"])
def test_table_caching_f64(gpu, oracle, kernel, schedule):
    p = problem(40, 64, 40, f64=True)
    _caching_run(p, 40, kernel, schedule, 25, random_z0(40, 40, True))


# ---- GPAD_SCHEDULE_PAPER beyond one battery shape ----------------------------------------------
@functools.lru_cache(maxsize=None)
def paper_reference(n, m, B, f64=False):
    p = problem(n, m, B, f64=f64)
    O = orc()
    if f64:
        r = pmap(lambda b: O.solve_f64(np.zeros(n), np.zeros(m), p.ML, p.M[b], p.G, p.g[b], NMAX, p.L, TOL, schedule=1,
                                       code=True), range(B))
    else:
        r = pmap(lambda b: O.solve_scaled_f32(np.zeros(n), np.zeros(m), p.MGneg, p.M[b], p.GL, p.PD[b], NMAX, p.L, TOL,
                                              schedule=1, code=True), range(B))
    return (np.stack([a[0] for a in r]), np.stack([a[1] for a in r]), np.array([a[2] for a in r], np.int32),
            np.array([a[3] for a in r], np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["stream", "resident", "panel"])
@pytest.mark.parametrize("n,m,B", [(37, 53, 19), (200, 200, 35)])
def test_paper_schedule(gpu, oracle, n, m, B, kernel):
    """schedule = 1 to tol = 1e-4 from z0 = 0: counts, codes, z*, y* of every instance equal the
    oracle's solve with schedule = 1."""
    p = problem(n, m, B)
    got = gpu_solve(p, B, kernel, np.zeros((B, n), np.float32), NMAX, TOL, 10, None, None, schedule=1)
    assert got[4]["kernel"] == kernel
    ref = paper_reference(n, m, B)
    assert ref[2].max() < NMAX and (ref[3] > 0).all()
    same(got, ref, f"paper {n}x{m} {kernel}")


@pytest.mark.gpu
def test_paper_schedule_f64_panels(gpu, oracle):
    n, m, B = 136, 136, 40
    p = problem(n, m, B, f64=True)
    a = gpu_solve(p, B, "panel", np.zeros((B, n)), NMAX, TOL, 10, None, None, schedule=1)
    b = gpu_solve(p, B, "stream", np.zeros((B, n)), NMAX, TOL, 10, None, None, schedule=1)
    assert a[4]["kernel"] == "panel" and b[4]["kernel"] == "stream"
    ref = paper_reference(n, m, B, True)
    assert ref[2].max() < NMAX and (ref[3] > 0).all()
    same(a, ref, "paper f64 panel", f64=True)
    for x, y_ in zip(a[:4], b[:4]):
        np.testing.assert_array_equal(x, y_)
