"""The panel-pair solve loop (gpad_pairs.h panel2_run) against the f32 oracle, bit for bit.

The loop's epilogues are scheduled for the fewest vector instructions beside the MFMA chains
(the schedule load, the splats, the stage order of 8d / 8a, the u recursion and the test's
partials); none of that may change a result.  Every case compares z*, y*, the iteration count
and the termination code of every instance with its own oracle solve:

* layouts: panel pairs (the grid capped below the panel count) and one panel per workgroup
  (no cap), at 96 instances (6 full panels) and 40 (a ragged third panel, a pair item with one
  panel);
* shapes: n = m = 200 (T = 13, the hand-off deal, last k-block of 2 steps), n = m = 136 (T = 9,
  the other hand-off shape), n = 184 with m = 200 (a runtime-length GEMM, no hand-off);
* modes: fixed N = 23; to a tolerance with the test every 10 and every iteration, in phases of
  20 so that the first launch ends in a park and a carried phase follows;
* starts: cold (z0 = y0 = 0), warm (non-zero z0, y0), and y0 = 0 on some columns only.

The oracle solves of a (shape, start, mode) are computed once and shared by its layouts.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BMAX = 96
PHASE = 20
SHAPES = [(200, 200), (136, 136), (184, 200)]
MODES = {"fixedN23": (0.0, 23, 10), "epsK10": (1e-4, 3000, 10), "epsK1": (1e-4, 3000, 1)}
STARTS = ["cold", "warm", "partial"]
LAYOUTS = {"pair": 2, "onepanel": 0}  # panel_max_grid: 2 workgroups for 3 or 6 panels; no cap


@functools.lru_cache(maxsize=None)
def problem(nm):
    from gpad_mpc import problems
    n, m = nm
    qp = problems.synthetic_qp(n, m, batch=BMAX, seed=31)
    f = lambda a: np.ascontiguousarray(np.asarray(a).astype(np.float32))  # noqa: E731
    return f(qp.ML), f(qp.M), f(qp.G), f(qp.g), np.float32(qp.L)


@functools.lru_cache(maxsize=None)
def start(nm, kind):
    n, m = nm
    rng = np.random.default_rng(5)
    z0 = (0.1 * rng.normal(size=(BMAX, n))).astype(np.float32)
    y0 = np.abs(0.1 * rng.normal(size=(BMAX, m))).astype(np.float32)
    if kind == "cold":
        z0[:] = 0.0
        y0[:] = 0.0
    elif kind == "partial":  # y0 = 0 on two columns of three, in every panel; z0 = 0 on half of those
        cols = np.arange(BMAX)
        y0[cols % 3 != 1] = 0.0
        z0[cols % 6 == 0] = 0.0
    return z0, y0


@functools.lru_cache(maxsize=None)
def reference(nm, kind, mode):
    """(z*, y*, iterations, termination code) of the BMAX instances, one oracle solve each (the
    oracle's C entry point, which reports the code; pyoracle's wrapper folds it to a bool)."""
    import pyoracle
    O = pyoracle.Oracle()
    ML, M, G, g, L = problem(nm)
    z0, y0 = start(nm, kind)
    tol, N, K = MODES[mode]
    n, m = nm
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    th, be = (np.ascontiguousarray(t, np.float32) for t in O.schedule_f32(max(N, 1)))
    z, y = z0.copy(), y0.copy()
    its, codes = np.zeros(BMAX, np.int32), np.zeros(BMAX, np.int32)
    MGneg = GL = None
    for b in range(BMAX):
        Mn, Gl, pD = (np.ascontiguousarray(a, np.float32) for a in O.scale(ML, G, g[b], L))
        if MGneg is None:
            MGneg, GL = Mn, Gl  # (the scaled matrices do not depend on g)
        code = C.c_int(0)
        its[b] = O.lib.orc_solve_f32(fp(z[b]), fp(y[b]), fp(MGneg), fp(M[b]), fp(GL), fp(pD), n, m, N, L,
                                     float(tol), 0.0, K, fp(th), fp(be), C.byref(code))
        codes[b] = code.value
    for a in (z, y, its, codes):
        a.setflags(write=False)
    return z, y, its, codes


def cases():
    for nm in SHAPES:
        for mode in MODES:
            for kind in STARTS:
                # the columns-apart start: once per shape and layout, in the tolerance mode
                if kind == "partial" and mode != "epsK10":
                    continue
                for layout in LAYOUTS:
                    for B in (96, 40):
                        yield pytest.param(nm, mode, kind, layout, B, id=f"{nm[0]}x{nm[1]}-{mode}-{kind}-{layout}-B{B}")


@pytest.mark.parametrize("nm,mode,kind,layout,B", list(cases()))
def test_panel_loop_bitexact(gpu, oracle, nm, mode, kind, layout, B):
    import gpad_mpc
    from gpad_mpc import _lib
    n, m = nm
    ML, M, G, g, L = problem(nm)
    z0, y0 = start(nm, kind)
    tol, N, K = MODES[mode]
    zr, yr, itr, cvr = reference(nm, kind, mode)
    z, y = z0[:B].copy(), y0[:B].copy()
    iters = np.zeros(B, np.int32)
    codes = np.full(B, -1, np.int32)
    with gpad_mpc.GpadSolver(0) as s:
        s.setup(ML, G, float(L), n=n, m=m, batch=B, shared=True, kernel=_lib.KERNEL_PANEL, check_every=K)
        # finish_thresh = 0: the carried phases stay on the panel kernel
        s.set_options(panel_max_grid=LAYOUTS[layout], phase_len=PHASE, finish_thresh=0)
        st = s.run(z, y, np.ascontiguousarray(M[:B]), np.ascontiguousarray(g[:B]), N, tol, iters=iters, codes=codes)
    assert st["kernel"] == "panel"
    if tol > 0.0:
        assert itr[:B].max() > PHASE, "no instance was carried into a second phase"
        assert itr[:B].max() < N and (cvr[:B] > 0).all(), "the reference did not converge"
    bad = np.flatnonzero(iters != itr[:B])
    assert bad.size == 0, f"iteration counts differ at {bad[:8]}: {iters[bad[:8]]} vs {itr[bad[:8]]}"
    assert np.array_equal(codes, cvr[:B]), f"termination codes differ at {np.flatnonzero(codes != cvr[:B])[:8]}"
    for name, a, r in (("z", z, zr[:B]), ("y", y, yr[:B])):
        if not np.array_equal(a, r):
            d = np.abs(a.astype(np.float64) - r.astype(np.float64))
            rows = np.flatnonzero(d.max(axis=1) > 0)
            raise AssertionError(f"{name}: {rows.size} of {B} instances differ (first {rows[:8]}), max |d| = {d.max():.3g}")
