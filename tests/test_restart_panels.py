"""Adaptive restart (GPAD_OPT_RESTART) on the f32 T-wave MFMA panels: gpad_panel_restart_kernel<T>.

Shared matrices, a forced PANEL kernel, batches of 37 (ragged last panel) and 16 (the first 16 instances of the
same data).  Shapes: T = 1 (12 x 16), T = 3 with n > m (48 x 20) and m > n (20 x 48), C1 (40 x 180: T = 12, ragged
last tiles in both operands), the tile edges 16 x 256 and 256 x 16 (T = 16).  R in {1, 3, 4, 10}; tol = 1e-4 with
N = 400 on the default phases and with phase_len = 10; fixed N = 37.  Every run is compared bit for bit -- z*, y*,
counts, codes, restart counts -- with the reference (tests/restart_ref.py: the unchanged oracle on each instance's
spliced tables) and with the restart stream kernel on the same inputs; floor and flags with the stream run's.

Phase boundaries fall on test events only (panel_phase_len rounds the length up to a multiple of check_every), so
"between a restart and the next test event" cannot be had at check_every = 10; phase_len = 10 puts a boundary after
every test event instead: with R = 3 and 4 a column is parked with a position that differs from its count (the
carried phase restores it and goes on counting v % R in the instance's own iterations), and with R = 1 and 10
every boundary falls on a decision iteration itself, whose restart -- with R = 10 every restart there is -- is
applied before the column is parked.

Instance 0 has its constraints far away (no restart); an ambiguous decision (restart_ref.AMBIGUOUS) takes its
instance out of a comparison, and more than 2 % left out fails the test; the CPU part asserts that none is.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import pytest

import restart_ref
from test_loop_async import F32, battery, same_bits, states
from test_restart import MODES, R_SET, tight_L

SHAPES = {"T1_12x16": (12, 16), "T3_48x20": (48, 20), "T3_20x48": (20, 48), "c1": (40, 180),
          "T16_16x256": (16, 256), "T16_256x16": (256, 16)}
BATCH = 37


@functools.lru_cache(maxsize=None)
def problem(shape):
    from gpad_mpc import problems
    if shape == "c1":
        p = battery(4, 10)
        X = states(p, BATCH, 53).astype(np.float64)
        X[0] = 0.0
        ML, G, M, g = p.qp.ML, p.qp.G, X @ p.PM.T, p.g0[None, :] + X @ p.Pg.T
        L = tight_L(ML, G)
    else:
        n, m = SHAPES[shape]
        qp = problems.synthetic_qp(n, m, batch=BATCH, seed=20)
        ML, G, M, g = qp.ML, qp.G, qp.M.copy(), qp.g.copy()
        g[0] = 1e3
        L = qp.L  # synthetic_qp's own bound ||G ML||_F: with the tight one these solves are over well before 37
    return SimpleNamespace(ML=F32(ML), G=F32(G), M=F32(M), g=F32(g), L=np.float32(L), n=ML.shape[0], m=ML.shape[1])


_refs = {}


def reference(oracle, shape, mode, R):
    if (shape, mode, R) not in _refs:
        t = problem(shape)
        N, tol = MODES[mode]
        th, be = oracle.schedule_f32(N)
        rows = []
        for b in range(BATCH):
            MGneg, GL, pD = oracle.scale(t.ML, t.G, t.g[b], t.L)
            rows.append(restart_ref.expected(oracle, np.zeros(t.n), np.zeros(t.m), MGneg, t.M[b], GL, pD, N, t.L, tol,
                                             R, th, be))
        _refs[shape, mode, R] = rows
    return _refs[shape, mode, R]


_handles = {}


def handle(shape, batch, kernel):
    from gpad_mpc import GpadSolver
    if (shape, batch, kernel) not in _handles:
        t = problem(shape)
        s = GpadSolver(0)
        s.setup(t.ML, t.G, float(t.L), n=t.n, m=t.m, batch=batch, shared=True, kernel=kernel)
        _handles[shape, batch, kernel] = s
    return _handles[shape, batch, kernel]


def solve(shape, batch, kernel, mode, R, phase_len=0):
    t = problem(shape)
    N, tol = MODES[mode]
    s = handle(shape, batch, kernel)
    Z, Y = np.zeros((batch, t.n), np.float32), np.zeros((batch, t.m), np.float32)
    it, cd = np.full(batch, -1, np.int32), np.full(batch, -1, np.int32)
    s.set_options(restart=R, phase_len=phase_len)
    try:
        st = s.run(Z, Y, np.ascontiguousarray(t.M[:batch]), np.ascontiguousarray(t.g[:batch]), N, tol, iters=it,
                   codes=cd)
        rs = s.last_restarts()
        phases = s.last_phases() if tol > 0.0 and st["kernel"] == "panel" else None
    finally:
        s.set_options(restart=0, phase_len=0)
    return SimpleNamespace(z=Z, y=Y, it=it, cd=cd, rs=rs, st=st, phases=phases)


def check(oracle, shape, batch, mode, R, phase_len=0):
    from gpad_mpc import _lib
    what = f"{shape} batch={batch} {mode} R={R} phase_len={phase_len}"
    rows = reference(oracle, shape, mode, R)[:batch]
    keep = [b for b, e in enumerate(rows) if not e.ambiguous]
    assert batch - len(keep) <= restart_ref.MAX_LEFT_OUT * batch, f"{what}: {batch - len(keep)} ambiguous"
    r = solve(shape, batch, _lib.KERNEL_PANEL, mode, R, phase_len)
    q = solve(shape, batch, _lib.KERNEL_STREAM, mode, R)
    assert r.st["kernel"] == "panel" and q.st["kernel"] == "stream", (r.st["kernel"], q.st["kernel"])
    for b in keep:
        e = rows[b]
        got = (int(r.it[b]), int(r.cd[b]), int(r.rs[b]))
        assert got == (e.it, e.code, e.restarts), f"{what} instance {b}: (it, code, restarts) {got} != " \
                                                  f"{(e.it, e.code, e.restarts)}, min ratio {e.min_ratio:.3g}"
        same_bits(r.z[b], e.z, f"{what} instance {b} z")
        same_bits(r.y[b], e.y, f"{what} instance {b} y")
    for k in ("z", "y", "it", "cd", "rs"):
        same_bits(getattr(r, k)[keep], getattr(q, k)[keep], f"{what} panel against stream: {k}")
    assert np.array_equal(r.st["tol_floor"], q.st["tol_floor"], equal_nan=True)
    assert (r.st["below_tol_floor"], r.st["nonfinite_g"]) == (q.st["below_tol_floor"], q.st["nonfinite_g"])
    assert r.st["total_iterations"] == int(r.it.sum()) and r.st["iterations"] == int(r.it.max())
    return r, rows


# ------------------------------------------------------------------------------ CPU
# The cases in which no instance restarts twice, with the largest restart count the reference gives.  Within 37
# iterations the 16 x 256 problem (16 variables under 256 constraints, slow on this L) turns its momentum once or
# not at all, and with R = 10 there are three decisions, of which 20 x 48 and C1 take one.
FEWER = {("T16_16x256", "fixed", 1): 1, ("T16_16x256", "fixed", 3): 1, ("T16_16x256", "fixed", 4): 0,
         ("T16_16x256", "fixed", 10): 0, ("T3_20x48", "fixed", 10): 1, ("c1", "fixed", 10): 1}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_reference_is_decided(oracle, shape):
    """Case by case: no ambiguous instance, an instance without a restart (instance 0), an instance with >= 2
    restarts -- but the cases of FEWER, whose most restarted instance has exactly the count given there -- and fewer
    iterations in total than the plain tolerance solve."""
    plain = sum(e.it for e in reference(oracle, shape, "tol", 0))
    for mode in MODES:
        for R in R_SET:
            rows = reference(oracle, shape, mode, R)
            rst = [e.restarts for e in rows]
            print(f"{shape} {mode} R={R}: restarts {rst}, smallest |q| / sum|terms| "
                  f"{min(e.min_ratio for e in rows):.3g}")
            assert not any(e.ambiguous for e in rows), (mode, R)
            need = FEWER.get((shape, mode, R), 2)
            assert min(rst) == 0 and (max(rst) >= 2 if need == 2 else max(rst) == need), (mode, R, rst)
            if mode == "tol":
                assert sum(e.it for e in rows) < plain, (R, sum(e.it for e in rows), plain)


# ------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("R", R_SET)
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("batch", [37, 16])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_panels(gpu, oracle, shape, batch, mode, R):
    check(oracle, shape, batch, mode, R)


@pytest.mark.gpu
@pytest.mark.parametrize("R", R_SET)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_panels_phase_boundaries(gpu, oracle, shape, R):
    """phase_len = 10: a boundary after every test event, columns parked with their position and count."""
    r, rows = check(oracle, shape, BATCH, "tol", R, phase_len=10)
    ends = r.phases["ends"]
    assert len(ends) >= 3 and ends[:3] == [10, 20, 30], ends
    # some column crossed a boundary after a restart: parked at a position that is not its count ...
    assert any(e.it > 10 * (c // 10 + 1) for e in rows for c in e.restart_counts)
    if R == 10:  # ... and every restart was taken on a boundary iteration itself
        assert any(c % 10 == 0 and e.it > c for e in rows for c in e.restart_counts)


@pytest.mark.gpu
def test_auto_routes_fleets_to_the_panels(gpu):
    """AUTO with R > 0: a shared f32 fleet above the panel threshold runs the restart panels, a batch below it the
    restart stream kernel, and big panels (n > 256) the stream kernel."""
    import torch
    from gpad_mpc import GpadSolver, problems
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for n, m, batch, want in ((12, 16, 4 * cus + 16, "panel"), (12, 16, 8, "stream"), (260, 16, 80, "stream")):
        qp = problems.synthetic_qp(n, m, batch=batch, seed=5)
        with GpadSolver(0) as s:
            s.setup(F32(qp.ML), F32(qp.G), float(np.float32(qp.L)), n=n, m=m, batch=batch, shared=True)
            s.set_option("restart", 4)
            Z, Y = np.zeros((batch, n), np.float32), np.zeros((batch, m), np.float32)
            st = s.run(Z, Y, F32(qp.M), F32(qp.g), 400, 1e-4)
            assert st["kernel"] == want, (n, m, batch, st["kernel"])
            assert s.last_restarts().max() >= 1
