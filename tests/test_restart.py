"""Adaptive restart of the momentum (GPAD_OPT_RESTART, include/gpad.h) on the stream kernel, f32 and f64.

The contract is bit identity with the spliced-table solve (tests/restart_ref.py): a restarted solve is the plain
solve with per-instance theta' / beta' tables, so the unchanged oracle gives z*, y*, counts and codes once the
reference has reproduced the decisions, and the restart counts come from the same decisions.  f32 runs are
compared with the oracle bit for bit.  The f64 oracle restates the MATLAB arithmetic, not the kernels' (it adds
(w + G_L zhat) + p_D, they (w + p_D) + G_L zhat; tests/test_gpu_parity.py holds the plain f64 kernel to 1e-12 of
it), so f64 runs are compared with it in counts, codes and restart counts exactly and in z*, y* to that 1e-12,
and bit for bit with the plain f64 stream kernel given each instance's spliced tables through gpad_run_scaled.

Inputs: synthetic_qp(12, 16), synthetic_qp(80, 48) and the C1 battery plant (40 x 180) at random states, batch 5,
with the tight step bound L = 1.01 lambda_max(G ML); instance 0 of every batch has its constraints far away
(y stays 0: q = 0 at every decision, no restart).  tol = 1e-4 with N = 400, and fixed N = 37 (short of
convergence, where q decays to rounding noise).  An ambiguous decision (restart_ref.AMBIGUOUS) takes its instance
out of a comparison; more than 2 % of a test's instances left out fails it.  The CPU part asserts that the
reference leaves out none.

The restart on the MFMA panels, its phase-boundary cases and the panel / stream cross-check are in
tests/test_restart_panels.py.
"""
from __future__ import annotations

import functools
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import restart_ref
from conftest import ROOT
from test_loop_async import F32, F64, battery, same_bits, states

R_SET = (1, 3, 4, 10)  # 3 does not divide check_every = 10; 10 coincides with every test event
SHAPES = ("s12x16", "s80x48", "c1")
MODES = {"tol": (400, 1e-4), "fixed": (37, 0.0)}
BATCH = 5
F64_RTOL = 1e-12


# ------------------------------------------------------------------------------ problems
def tight_L(ML, G):
    """1.01 lambda_max(G ML) over every instance (G ML = G H^-1 G' is symmetric)."""
    ML, G = np.atleast_3d(ML.T).T, np.atleast_3d(G.T).T
    top = 0.0
    for a, b in zip(ML, G):
        S = b.astype(np.float64) @ a.astype(np.float64)
        top = max(top, float(np.linalg.eigvalsh(0.5 * (S + S.T))[-1]))
    return 1.01 * top


@functools.lru_cache(maxsize=None)
def problem(shape, shared):
    """fp64 data of a batch: ML [B or 1][n][m], G likewise, M [B][n], g [B][m], L."""
    from gpad_mpc import problems
    if shape == "c1":
        p = battery(4, 10)
        X = states(p, BATCH, 31).astype(np.float64)
        X[0] = 0.0
        M = X @ p.PM.T
        g = p.g0[None, :] + X @ p.Pg.T
        ML, G = p.qp.ML[None], p.qp.G[None]
        if not shared:
            ML, G = np.repeat(ML, BATCH, 0), np.repeat(G, BATCH, 0)
    else:
        n, m = (12, 16) if shape == "s12x16" else (80, 48)
        qp = problems.synthetic_qp(n, m, batch=BATCH, seed=7, shared=bool(shared))
        ML, G = (qp.ML[None], qp.G[None]) if shared else (qp.ML, qp.G)
        M, g = qp.M.copy(), qp.g.copy()
        g[0] = 1e3
    return SimpleNamespace(ML=ML, G=G, M=M, g=g, L=tight_L(ML, G), n=ML.shape[1], m=ML.shape[2], shared=shared)


def typed(pr, dtype):
    c = F64 if dtype == np.float64 else F32
    L = float(pr.L) if dtype == np.float64 else np.float32(pr.L)
    return SimpleNamespace(ML=c(pr.ML), G=c(pr.G), M=c(pr.M), g=c(pr.g), L=L, n=pr.n, m=pr.m, shared=pr.shared)


def scaled(oracle, t, b, dtype):
    """Instance b's scaled operands as its kernel holds them: MGneg, GL, pD."""
    i = 0 if t.shared else b
    if dtype == np.float64:
        return -t.ML[i], (1.0 / t.L) * t.G[i], (-1.0 / t.L) * t.g[b]
    MGneg, GL, pD = oracle.scale(t.ML[i], t.G[i], t.g[b], t.L)
    return MGneg, GL, pD


_ref_cache = {}


def reference(oracle, shape, shared, dtype, mode, R, start=None):
    """restart_ref.expected of every instance of a case, once per session.  start: (Z0, Y0) or None (zeros)."""
    key = (shape, shared, np.dtype(dtype).name, mode, R, None if start is None else start[1].tobytes())
    if key not in _ref_cache:
        t = typed(problem(shape, shared), dtype)
        N, tol = MODES[mode]
        th, be = oracle.schedule(N) if dtype == np.float64 else oracle.schedule_f32(N)
        rows = []
        for b in range(BATCH):
            MGneg, GL, pD = scaled(oracle, t, b, dtype)
            z0 = np.zeros(t.n, dtype) if start is None else start[0][b]
            y0 = np.zeros(t.m, dtype) if start is None else start[1][b]
            i = 0 if t.shared else b
            rows.append(restart_ref.expected(oracle, z0, y0, MGneg, t.M[b], GL, pD, N, t.L, tol, R, th, be,
                                             f64_problem=(t.ML[i], t.M[b], t.G[i], t.g[b]) if dtype == np.float64
                                             else None))
        _ref_cache[key] = rows
    return _ref_cache[key]


def warm_start(oracle, shape, dtype):
    """z*, y* of the plain tolerance solves of the batch rolled by one instance: a previous, nearby solve."""
    rows = reference(oracle, shape, 1, dtype, "tol", 0)
    order = [0] + [1 + (b % (BATCH - 1)) for b in range(1, BATCH)]  # (instance 0 keeps its own: y* = 0)
    return np.stack([rows[j].z for j in order]), np.stack([rows[j].y for j in order])


# ------------------------------------------------------------------------------ GPU runs
_handles = {}


def handle(shape, shared, dtype, kernel=None):
    from gpad_mpc import GpadSolver, _lib
    key = (shape, shared, np.dtype(dtype).name, kernel)
    if key not in _handles:
        t = typed(problem(shape, shared), dtype)
        s = GpadSolver(0)
        s.setup(t.ML if not shared else t.ML[0], t.G if not shared else t.G[0], float(t.L), n=t.n, m=t.m, batch=BATCH,
                shared=bool(shared), kernel=_lib.KERNEL_AUTO if kernel is None else kernel)
        _handles[key] = (s, t)
    return _handles[key]


def solve(s, t, N, tol, R, start=None):
    dtype = t.M.dtype
    Z = np.zeros((BATCH, t.n), dtype) if start is None else start[0].astype(dtype).copy()
    Y = np.zeros((BATCH, t.m), dtype) if start is None else start[1].astype(dtype).copy()
    it, cd = np.full(BATCH, -1, np.int32), np.full(BATCH, -1, np.int32)
    s.set_option("restart", R)
    try:
        st = s.run(Z, Y, t.M, t.g, N, tol, iters=it, codes=cd)
        rs = s.last_restarts()
    finally:
        s.set_option("restart", 0)
    return SimpleNamespace(z=Z, y=Y, it=it, cd=cd, rs=rs, st=st)


def compare(r, rows, dtype, what):
    """r against the reference rows; ambiguous instances left out, at most 2 % of them."""
    keep = [b for b, e in enumerate(rows) if not e.ambiguous]
    assert len(rows) - len(keep) <= restart_ref.MAX_LEFT_OUT * len(rows), f"{what}: ambiguous {len(rows) - len(keep)}"
    for b in keep:
        e = rows[b]
        got = (int(r.it[b]), int(r.cd[b]), int(r.rs[b]))
        assert got == (e.it, e.code, e.restarts), f"{what} instance {b}: (it, code, restarts) {got} != " \
                                                  f"{(e.it, e.code, e.restarts)}, min ratio {e.min_ratio:.3g}"
        if dtype == np.float64:
            for a, o, k in ((r.z[b], e.z, "z"), (r.y[b], e.y, "y")):
                rel = np.linalg.norm(a - o) / max(np.linalg.norm(o), 1e-300)
                print(f"{what} instance {b} {k}: rel {rel:.3g}")
                assert rel < F64_RTOL, f"{what} instance {b} {k}: rel {rel:.3g}"
        else:
            same_bits(r.z[b], e.z, f"{what} instance {b} z")
            same_bits(r.y[b], e.y, f"{what} instance {b} y")
    return keep


def spliced_gpu(oracle, t, b, e, N, tol, start=None):
    """Instance b on the plain stream kernel with its spliced tables (gpad_run_scaled, caller tables)."""
    from gpad_mpc import GpadSolver, _lib
    dtype = t.M.dtype
    MGneg, GL, pD = scaled(oracle, t, b, dtype)
    z = np.zeros(t.n, dtype) if start is None else start[0][b].astype(dtype).copy()
    y = np.zeros(t.m, dtype) if start is None else start[1][b].astype(dtype).copy()
    it, cd = np.full(1, -1, np.int32), np.full(1, -1, np.int32)
    with GpadSolver(0) as s:
        s.setup(np.ascontiguousarray(MGneg), np.ascontiguousarray(GL), float(t.L), n=t.n, m=t.m, batch=1, shared=True,
                kernel=_lib.KERNEL_STREAM, scaled=True)
        s.run(z, y, np.ascontiguousarray(t.M[b]), np.ascontiguousarray(pD), N, tol, scaled=True,
              theta=np.ascontiguousarray(e.theta), beta=np.ascontiguousarray(e.beta), iters=it, codes=cd)
    return z, y, int(it[0]), int(cd[0])


# ------------------------------------------------------------------------------ CPU
def test_option_number_and_exports():
    from gpad_mpc import _lib
    hdr = open(os.path.join(ROOT, "include", "gpad.h")).read()
    assert int(re.search(r"#define GPAD_OPT_RESTART \((\d+)\)", hdr).group(1)) == 24 == _lib.OPT_RESTART
    assert _lib.SOLVE_OPTIONS == {"restart": 24} and "restart" not in _lib.OPTIONS
    assert 24 not in _lib.OPTIONS.values() and 24 not in _lib.OPT_RETIRED
    assert "gpad_last_restarts" in _lib.EXPORTS and hasattr(_lib.load(), "gpad_last_restarts")
    assert not re.search(r"restart", open(os.path.join(ROOT, "bench.py")).read())  # (off in the benchmark)


def test_validation_without_a_gpu():
    """A null handle, a null array and a negative cap are GPAD_ERR_INVALID, on the option and on the counts."""
    import ctypes as C
    from gpad_mpc import _lib
    lib = _lib.load()
    buf = (C.c_int * 4)()
    assert lib.gpad_set_option(None, _lib.OPT_RESTART, 4) == _lib.ERR_INVALID
    assert lib.gpad_last_restarts(None, buf, 4) == _lib.ERR_INVALID
    assert b"gpad_last_restarts" in lib.gpad_last_error()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_R0_tables_are_the_schedule(oracle, dtype):
    t = typed(problem("s12x16", 1), dtype)
    th, be = oracle.schedule(60) if dtype == np.float64 else oracle.schedule_f32(60)
    MGneg, GL, pD = scaled(oracle, t, 1, dtype)
    th2, be2, restarts, decisions = restart_ref.restart_tables(oracle, np.zeros(t.n), np.zeros(t.m), MGneg, t.M[1], GL,
                                                               pD, 60, 0, th, be)
    assert restarts == [] and decisions == []
    same_bits(th2, th, "theta")
    same_bits(be2, be, "beta")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("R", R_SET)
def test_splice_identity_on_the_oracle(oracle, shape, R):
    """A step loop over Oracle.step1..4 that restarts in place -- w = y+, position 0 -- gives the bits of the
    table solve with the spliced tables."""
    t = typed(problem(shape, 1), np.float32)
    N = 120
    th, be = oracle.schedule_f32(N)
    seen = 0
    for b in (1, 2):
        MGneg, GL, pD = scaled(oracle, t, b, np.float32)
        z, y = np.zeros(t.n, np.float32), np.zeros(t.m, np.float32)
        ym1, pos, count = y.copy(), 0, 0
        for v in range(N):
            w = oracle.step1(y, ym1, be[pos])
            zh = oracle.step2(MGneg, w, t.M[b])
            z = oracle.step3(th[pos], z, zh)
            yp = oracle.step4(GL, w, pD, zh)
            pos += 1
            if (v + 1) % R == 0 and v + 1 < N:
                q = math.fsum((w - yp).astype(np.float64) * (yp - y).astype(np.float64))
                if q > 0.0:
                    ym1, y, pos, count = yp, yp, 0, count + 1  # (y - ym1 = 0: the next w is y+ whatever beta)
                    continue
            ym1, y = y, yp
        e = restart_ref.expected(oracle, np.zeros(t.n), np.zeros(t.m), MGneg, t.M[b], GL, pD, N, t.L, 0.0, R, th, be)
        assert e.it == N and e.restarts == count
        seen += count
        same_bits(z, e.z, f"{shape} R={R} instance {b} z")
        same_bits(y, e.y, f"{shape} R={R} instance {b} y")
    assert seen >= 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shared", [1, 0])
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_is_decided(oracle, shape, shared, dtype):
    """For the GPU cases of this shape, case by case: no ambiguous instance; an instance with no restart (instance
    0); with R <= 4 and a tolerance an instance with >= 2 restarts; and the restarted tolerance solves take fewer
    iterations in total than the plain ones.  Where ">= 2 restarts" is not asserted it cannot hold for these
    inputs: with R = 10 a solve that ends after 30 - 50 iterations has two to four decisions and takes one of
    them (12 x 16: restarts [0, 1, 1, 1, 1]), and at fixed N = 37 with R = 10 there are three decisions in all;
    every case still asserts that something restarts, and prints its counts."""
    worst = math.inf
    for mode in MODES:
        for R in R_SET:
            rows = reference(oracle, shape, shared, dtype, mode, R)
            assert not any(e.ambiguous for e in rows), (mode, R)
            worst = min(worst, min(e.min_ratio for e in rows))
            rst = [e.restarts for e in rows]
            print(f"{shape} shared={shared} {np.dtype(dtype).name} {mode} R={R}: restarts {rst}")
            assert min(rst) == 0 and max(rst) >= (2 if R <= 4 and mode == "tol" else 1), (mode, R, rst)
            if mode == "tol":
                plain = reference(oracle, shape, shared, dtype, mode, 0)
                total, total0 = sum(e.it for e in rows), sum(e.it for e in plain)
                print(f"{shape} shared={shared} {np.dtype(dtype).name} R={R}: iterations {total0} -> {total}, "
                      f"restarts {[e.restarts for e in rows]}")
                assert total < total0, (R, total, total0)
                assert all(e.code != 0 for e in rows), (R, [e.code for e in rows])
    print(f"{shape} shared={shared} {np.dtype(dtype).name}: smallest |q| / sum|terms| before termination {worst:.3g}")
    assert worst > 1e3 * restart_ref.AMBIGUOUS


# ------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("R", R_SET)
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shared", [1, 0])
@pytest.mark.parametrize("shape", SHAPES)
def test_stream(gpu, oracle, shape, shared, dtype, mode, R):
    N, tol = MODES[mode]
    s, t = handle(shape, shared, dtype)
    rows = reference(oracle, shape, shared, dtype, mode, R)
    r = solve(s, t, N, tol, R)
    assert r.st["kernel"] == "stream"
    what = f"{shape} shared={shared} {np.dtype(dtype).name} {mode} R={R}"
    keep = compare(r, rows, dtype, what)
    plain = solve(s, t, N, tol, 0)  # the same data with the restart off: its floor and flags, zero restart counts
    assert not plain.rs.any()
    assert np.array_equal(r.st["tol_floor"], plain.st["tol_floor"], equal_nan=True)
    assert (r.st["below_tol_floor"], r.st["nonfinite_g"]) == (plain.st["below_tol_floor"], plain.st["nonfinite_g"])
    assert r.st["total_iterations"] == int(r.it.sum()) and r.st["iterations"] == int(r.it.max())
    if dtype == np.float64 and R == 4:  # the device's own splice identity, bit for bit
        for b in keep:
            z, y, it, cd = spliced_gpu(oracle, t, b, rows[b], N, tol)
            assert (it, cd) == (int(r.it[b]), int(r.cd[b]))
            same_bits(r.z[b], z, f"{what} instance {b} z vs the plain kernel on the spliced tables")
            same_bits(r.y[b], y, f"{what} instance {b} y vs the plain kernel on the spliced tables")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES)
def test_stream_warm_start(gpu, oracle, shape, dtype):
    """From a previous solve's z*, y* (a neighbouring instance's), tol = 1e-4, R = 4."""
    s, t = handle(shape, 1, dtype)
    start = warm_start(oracle, shape, dtype)
    rows = reference(oracle, shape, 1, dtype, "tol", 4, start=start)
    r = solve(s, t, *MODES["tol"], 4, start=start)
    compare(r, rows, dtype, f"{shape} warm {np.dtype(dtype).name}")
    assert any(e.restarts for e in rows)


@pytest.mark.gpu
def test_R0_after_R4_is_the_plain_solve(gpu, oracle):
    s, t = handle("c1", 1, np.float32)
    N, tol = MODES["tol"]
    before = solve(s, t, N, tol, 0)
    on = solve(s, t, N, tol, 4)
    after = solve(s, t, N, tol, 0)
    assert on.rs.any() and not after.rs.any() and not before.rs.any()
    for k in ("z", "y", "it", "cd"):
        same_bits(getattr(after, k), getattr(before, k), k)
    compare(after, reference(oracle, "c1", 1, np.float32, "tol", 0), np.float32, "R = 0 after R = 4")
    assert int(on.it.sum()) < int(before.it.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain", "classes"])
def test_option_bounds(gpu, kind):
    """0 .. 2^30 and GPAD_OPT_DEFAULT (restores 0) are accepted; any other negative and 2^30 + 1 are not."""
    from gpad_mpc import _lib
    from test_options import _handle
    s = _handle(kind)
    set_ = lambda v: s.lib.gpad_set_option(s.h, _lib.OPT_RESTART, v)  # noqa: E731
    try:
        for v in (-2, -7, (1 << 30) + 1):
            assert set_(v) == _lib.ERR_INVALID, v
        for v in (0, 1, 1 << 30, _lib.OPT_DEFAULT):
            assert set_(v) == _lib.GPAD_OK, v
    finally:
        assert set_(0) == _lib.GPAD_OK


@pytest.mark.gpu
def test_no_run_yet_reports_zeros(gpu):
    from gpad_mpc import GpadSolver
    t = typed(problem("s12x16", 1), np.float32)
    with GpadSolver(0) as s:
        s.setup(t.ML[0], t.G[0], float(t.L), n=t.n, m=t.m, batch=BATCH, shared=True)
        s.set_option("restart", 4)
        rs = s.last_restarts()
        assert rs.shape == (BATCH,) and not rs.any()


# ---- run_state and the lockstep closed loop of the C1 plant -------------------------------------------
def loop_reference(oracle, p, L, X0, steps, N, tol, warm, R, S=None):
    """The closed loop driven step by step on the CPU: affine maps, restart_ref.expected, plant step.  S
    [steps][batch][ns]: p has signals bound -- the same loop on the augmented plant over [x; S[t]]
    (test_signals.augmented), of whose state the first nx rows are the plant's."""
    import ctypes as C
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    qp, nx = p.qp, p.nx
    if S is not None:
        from test_signals import augmented
        p = augmented(p)
    MGneg, GL, _ = oracle.scale(F32(qp.ML), F32(qp.G), F32(np.zeros(qp.m)), L)
    th, be = oracle.schedule_f32(N)
    A, B = F32(p.A), F32(p.B)
    batch = X0.shape[0]
    out = SimpleNamespace(x=X0.copy(), z=np.zeros((batch, qp.n), np.float32), y=np.zeros((batch, qp.m), np.float32),
                          it=np.zeros((steps, batch), np.int32), cd=np.zeros((steps, batch), np.int32),
                          rs=np.zeros((steps, batch), np.int32), xs=np.zeros((steps, batch, nx), np.float32),
                          us=np.zeros((steps, batch, p.nu), np.float32), ambiguous=np.zeros(batch, bool))
    for b in range(batch):
        x, z, y = X0[b].copy(), out.z[b], out.y[b]
        for t in range(steps):
            if S is not None:
                x = np.concatenate([x[:nx], S[t, b]]).astype(np.float32)
            gP = oracle.affine(p.PM, p.M0, x)
            pD = oracle.scale_vec(oracle.affine(p.Pg, p.g0, x), L)
            if not warm:
                z, y = np.zeros(qp.n, np.float32), np.zeros(qp.m, np.float32)
            e = restart_ref.expected(oracle, z, y, MGneg, gP, GL, pD, N, L, tol, R, th, be)
            z, y = e.z, e.y
            out.it[t, b], out.cd[t, b], out.rs[t, b] = e.it, e.code, e.restarts
            out.ambiguous[b] |= e.ambiguous
            out.xs[t, b], out.us[t, b] = x[:nx], z[:p.nu]
            xn = np.empty(p.nx, np.float32)
            oracle.lib.orc_plant_step_f32(fp(A), fp(B), fp(np.ascontiguousarray(x)), fp(np.ascontiguousarray(z[:p.nu])),
                                          fp(xn), p.nx, p.nu)
            x = xn
        out.x[b], out.z[b], out.y[b] = x[:nx], z, y
    return out


def c1_loop_solver(batch, L, **options):
    from gpad_mpc import GpadSolver
    p = battery(4, 10)
    s = GpadSolver(0)
    s.setup(F32(p.qp.ML), F32(p.qp.G), float(L), n=p.qp.n, m=p.qp.m, batch=batch, shared=True)
    s.setup_plant(F32(p.PM), F32(p.Pg), g0=F32(p.g0), A=F32(p.A), B=F32(p.B))
    s.set_options(**options)
    return s, p


def run_loop(s, p, X0, steps, N, tol, warm):
    from test_loop_async import loop
    r = loop(s, p, X0, steps, N, tol, warm)
    r.rs = s.last_restarts()
    return r


def assert_loop(r, ref, what):
    keep = np.flatnonzero(~ref.ambiguous)
    assert len(ref.ambiguous) - len(keep) <= restart_ref.MAX_LEFT_OUT * len(ref.ambiguous), what
    assert r.rs.shape == ref.rs.shape, what
    for k in ("x", "z", "y"):
        same_bits(getattr(r, k)[keep], getattr(ref, k)[keep], f"{what} {k}")
    for k in ("xs", "us", "it", "cd", "rs"):
        same_bits(getattr(r, k)[:, keep], getattr(ref, k)[:, keep], f"{what} {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("option", [None, "loop_async", "loop_panel"])
def test_lockstep_closed_loop(gpu, oracle, warm, option):
    """Four steps of the C1 plant, tol = 1e-4, R = 4, against the loop driven step by step; with loop_async /
    loop_panel set the run reports a lockstep engine and the same bits."""
    p = battery(4, 10)
    L = np.float32(tight_L(p.qp.ML, p.qp.G))
    X0 = states(p, 6, 41)
    steps, N, tol = 4, 400, 1e-4
    ref = loop_reference(oracle, p, L, X0, steps, N, tol, warm, 4)
    assert ref.rs.max() >= 2 and not ref.ambiguous.any()
    s, _ = c1_loop_solver(6, L, restart=4, **({option: 1} if option else {}))
    with s:
        r = run_loop(s, p, X0, steps, N, tol, warm)
        assert r.st["kernel"] == "stream"
        assert_loop(r, ref, f"loop warm={warm} {option}")
        if option:  # the same handle with the restart off takes its one-launch engine again
            s.set_option("restart", 0)
            off = run_loop(s, p, X0, steps, N, tol, warm)
            assert off.st["kernel"] == {"loop_async": "loop", "loop_panel": "loop_panel"}[option]
            assert not off.rs.any() and off.rs.shape == (steps, 6)


@pytest.mark.gpu
def test_lockstep_closed_loop_with_signals(gpu, oracle):
    """The loaded C1 plant (test_signals' mild loads and references), four steps, warm, R = 4."""
    import test_signals as TS
    p = TS.battery(4, 10)
    X0, S = TS.inputs(4, 5, 4, **TS.MILD)
    L = np.float32(tight_L(p.qp.ML, p.qp.G))
    steps, N, tol = 4, 400, 1e-4
    ref = loop_reference(oracle, p, L, X0, steps, N, tol, True, 4, S=S)
    print("signals: restarts", ref.rs.tolist(), "counts", ref.it.tolist(), "ambiguous", ref.ambiguous.tolist())
    assert ref.rs.max() >= 2
    from gpad_mpc import GpadSolver
    with GpadSolver(0) as s:
        s.setup(F32(p.qp.ML), F32(p.qp.G), float(L), n=p.qp.n, m=p.qp.m, batch=5, shared=True)
        s.setup_plant(F32(p.PM), F32(p.Pg), g0=F32(p.g0), A=F32(p.A), B=F32(p.B))
        s.setup_signals(F32(p.SM), F32(p.Sg), F32(p.E), ns=p.ns)
        s.set_option("restart", 4)
        r = TS.loop(s, p, X0, S, steps, N, tol, True)
        r.rs = s.last_restarts()
    assert r.st["kernel"] == "stream"
    assert_loop(r, ref, "loop with signals")


@pytest.mark.gpu
def test_fused_class_loop_falls_back(gpu):
    """A class binding with gpad_class_loop_fused on: with R = 4 its closed loop runs class by class on the
    lockstep loop -- the bits and the [steps][batch] restart counts, in the caller's order, of the binding with the
    fused loop off -- and with R = 0 again the fused loop."""
    from test_classes import inputs
    from test_loop_async import loop
    from test_options import _classes
    I = inputs("A")
    steps, N, tol = 3, 400, 1e-4
    runs = {}
    for fused in (True, False):
        with _classes(after=dict(restart=4)) as s:
            s.set_class_loop_fused(fused)
            r = runs[fused] = loop(s, I.C, I.X0, steps, N, tol, False)
            r.rs = s.last_restarts()
            assert r.st["kernel"] not in ("loop_classes", "loop", "loop_panel"), r.st["kernel"]
            if fused:
                s.set_option("restart", 0)
                off = loop(s, I.C, I.X0, steps, N, tol, False)
                assert off.st["kernel"] == "loop_classes" and not s.last_restarts().any()
                assert int(off.it.sum()) > int(r.it.sum())
    a, b = runs[True], runs[False]
    assert a.rs.shape == (steps, I.X0.shape[0]) and a.rs.max() >= 2 and len(set(a.rs[0].tolist())) > 1
    for k in ("x", "z", "y", "xs", "us", "it", "cd", "rs"):
        same_bits(getattr(a, k), getattr(b, k), k)
    # every class's counts sit at its members' places: a member's count is its class child's (classes of one
    # instance each would hide a permutation, so the per-class multisets are compared as well)
    for k in np.unique(I.class_of):
        sel = np.flatnonzero(I.class_of == k)
        assert sorted(a.rs[:, sel].ravel().tolist()) == sorted(b.rs[:, sel].ravel().tolist())


@pytest.mark.gpu
def test_run_state(gpu, oracle):
    p = battery(4, 10)
    L = np.float32(tight_L(p.qp.ML, p.qp.G))
    X0 = states(p, 6, 43)
    ref = loop_reference(oracle, p, L, X0, 1, 400, 1e-4, False, 3)
    s, _ = c1_loop_solver(6, L, restart=3)
    with s:
        Z, Y = np.zeros((6, p.qp.n), np.float32), np.zeros((6, p.qp.m), np.float32)
        st = s.run_state(X0.copy(), Z, Y, 400, 1e-4)
        rs = s.last_restarts()
    assert st["kernel"] == "stream" and rs.shape == (6,) and not ref.ambiguous.any()
    same_bits(Z, ref.z, "z")
    same_bits(Y, ref.y, "y")
    same_bits(rs, ref.rs[0], "restarts")
    assert st["total_iterations"] == int(ref.it.sum())


# ---- a class binding forwards the option and gathers the counts -----------------------------------------
@pytest.mark.gpu
def test_class_binding_equals_its_expansion(gpu):
    """K = 2 classes, 20 instances: the class-bound handle with R = 4 equals the shared = 0 handle holding every
    instance's own copy of its class's matrices, restart counts in the caller's order."""
    from gpad_mpc import GpadSolver, problems
    K, batch, n, m = 2, 20, 12, 16
    qp = problems.synthetic_qp(n, m, batch=batch, seed=7, shared=False)
    class_of = (np.arange(batch) * 7 % 3 % K).astype(np.int32)
    ML, G = F32(qp.ML[:K]), F32(qp.G[:K])
    L = float(np.float32(tight_L(qp.ML[:K], qp.G[:K])))
    M, g = F32(qp.M), F32(qp.g)
    runs = []
    for bound in (True, False):
        with GpadSolver(0) as s:
            if bound:
                s.set_option("restart", 4)  # (before the binding: forwarded to the new children)
                s.setup_classes(ML, G, L, class_of, n=n, m=m)
            else:
                s.setup(np.ascontiguousarray(ML[class_of]), np.ascontiguousarray(G[class_of]), L, n=n, m=m,
                        batch=batch, shared=False)
                s.set_option("restart", 4)
            Z, Y = np.zeros((batch, n), np.float32), np.zeros((batch, m), np.float32)
            it, cd = np.zeros(batch, np.int32), np.zeros(batch, np.int32)
            s.run(Z, Y, M, g, 400, 1e-4, iters=it, codes=cd)
            runs.append(SimpleNamespace(z=Z, y=Y, it=it, cd=cd, rs=s.last_restarts()))
            if bound:  # turned off after the binding: forwarded call by call
                s.set_option("restart", 0)
                s.run(Z.copy(), Y.copy(), M, g, 400, 1e-4)
                assert not s.last_restarts().any()
    a, b = runs
    assert a.rs.shape == (batch,) and a.rs.max() >= 2 and len(set(a.rs.tolist())) > 1
    for k in ("z", "y", "it", "cd", "rs"):
        same_bits(getattr(a, k), getattr(b, k), k)


# ---- what the restart kernels do not carry ---------------------------------------------------------------
def _unsupported_cases():
    from gpad_mpc import _lib
    return {"resident": dict(kernel=_lib.KERNEL_RESIDENT), "panel_big": dict(kernel=_lib.KERNEL_PANEL, big=True),
            "panel_f64": dict(kernel=_lib.KERNEL_PANEL, dtype=np.float64), "hessian": dict(hessian=True),
            "infeasibility": dict(zbound=10.0), "tables": dict(tables=True), "flat": dict(flat=True)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["resident", "panel_big", "panel_f64", "hessian", "infeasibility", "tables", "flat"])
def test_unsupported_combinations(gpu, oracle, case):
    """GPAD_ERR_UNSUPPORTED with a message that names the restart; the handle then runs with R = 0, and the plain
    bits where the oracle has them."""
    from gpad_mpc import GpadError, GpadSolver, _lib, problems
    c = _unsupported_cases()[case]
    dtype = c.get("dtype", np.float32)
    cv = F64 if dtype == np.float64 else F32
    N, tol = 40, 1e-4
    kw = {}
    with GpadSolver(0) as s:
        if c.get("flat"):
            qp = problems.battery_mpc(4, 10, seed=0)
            MGf, GLf, L = problems.flatten_battery(qp, 4, 10)
            s.setup_flat(F32(MGf), F32(GLf), float(np.float32(L)), n_u=4, batch=BATCH)
            n, m = qp.n, qp.m
            M, g = F32(np.tile(qp.M, (BATCH, 1))), F32(np.tile(-qp.g / L, (BATCH, 1)))  # (g_P, p_D)
            kw = dict(scaled=True)
        else:
            t = typed(problem("s12x16", 1), dtype)
            if c.get("big"):  # n > 256: the big panels, which do not carry the restart
                qp = problems.synthetic_qp(260, 16, batch=BATCH, seed=3)
                t = SimpleNamespace(ML=F32(qp.ML)[None], G=F32(qp.G)[None], M=F32(qp.M), g=F32(qp.g),
                                    L=np.float32(qp.L), n=260, m=16)
            n, m, M, g = t.n, t.m, t.M, t.g
            s.setup(t.ML[0], t.G[0], float(t.L), n=n, m=m, batch=BATCH, shared=True,
                    kernel=c.get("kernel", _lib.KERNEL_AUTO), scaled=bool(c.get("tables")))
            if c.get("hessian"):
                s.setup_hessian(cv(problems.synthetic_qp(12, 16, batch=BATCH, seed=7).H))
            if c.get("zbound"):
                s.setup_infeasibility(c["zbound"])
        if c.get("tables"):
            th, be = oracle.schedule_f32(N)
            kw = dict(scaled=True, theta=th, beta=be)
        run = lambda: s.run(np.zeros((BATCH, n), dtype), np.zeros((BATCH, m), dtype), M, g, N, tol, **kw)  # noqa: E731
        s.set_option("restart", 4)
        with pytest.raises(GpadError) as err:
            run()
        assert err.value.code == _lib.ERR_UNSUPPORTED and "restart" in str(err.value).lower(), str(err.value)
        assert not s.last_restarts().any()
        s.set_option("restart", 0)
        st = run()
        assert st["iterations"] >= 1 and not s.last_restarts().any()
