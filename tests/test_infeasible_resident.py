"""Infeasibility certificates on the resident kernel (include/gpad.h gpad_infeasibility_resident): the surface,
the routing rules of the per-handle flag, one answer against the stream kernel, no false alarm, and the loops.

gpad_resident_farkas_kernel is the resident kernel's text with the rule of csrc/gpad_farkas.h; it must give the
stream kernel's bits.  The flag is off by default, and tests/test_infeasible.py pins what runs then.

Inputs: tests/infeas_cases.py (asserted on the reference by tests/test_infeasible_cpu.py) and the helpers of
tests/test_infeasible.py; reference: tests/infeas_ref64.py.  The wide cases (WIDE) are ``problems.synthetic_qp``
draws and the same draws with two contradictory rows: n = 72, where two waves own -ML rows, so that the G/L
waves' slots start at wave 2, and n = 204, m = 208, the largest bucket pair (208 row registers, eight waves).
Seeds and bounds were chosen on the CPU and are asserted there (test_wide_cases_cpu).
"""
from __future__ import annotations

import functools
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import gpad_mpc
import infeas_cases as cases
import infeas_ref64 as ref
from conftest import ROOT
from gpad_mpc import _lib, problems
from test_infeasible import F32, F64, _L, _code, _feasible, _loop, bound_solver, run, same

N, TOL, R = cases.N, cases.TOL, cases.R
SHAPES = ["1x2", "2x4", "4x10"]  # one G/L wave with 12 live rows, one with 40, three with the last ragged
NAME = "gpad_infeasibility_resident"

# the wide cases: n = 72 (two -ML waves), m = 100 (two G/L waves, the second ragged); n = 204, m = 208 (four and
# four, the 208 / 208 bucket pair).  R bounds |z|_inf of the feasible draws' solutions (below 2) with room
WIDE = {"n72": SimpleNamespace(n=72, m=100, batch=4, seed=1, R=1e3, rows=(3, 70)),
        "n204": SimpleNamespace(n=204, m=208, batch=2, seed=1, R=10.0, rows=(3, 150))}


def flagged(qp, c, batch, *, on=True, **kw):
    """bound_solver with the flag set (before the bound: it must survive the binding)."""
    s = bound_solver(qp, c, batch, bound=None, **{k: v for k, v in kw.items() if k != "bound"})
    s.set_infeasibility_resident(on)
    if kw.get("bound", R) is not None:
        s.setup_infeasibility(kw.get("bound", R))
    return s


@functools.lru_cache(maxsize=None)
def wide(key, infeasible):
    """A wide synthetic QP; infeasible: rows i, j made contradictory (G_j = -G_i, g_j = -g_i - 1: no z meets
    both, and y = e_i + e_j certifies it for any R), with ML and L recomputed from the new G."""
    w = WIDE[key]
    qp = problems.synthetic_qp(w.n, w.m, batch=w.batch, seed=w.seed)
    if not infeasible:
        return qp
    i, j = w.rows
    G, g = qp.G.copy(), qp.g.copy()
    G[j], g[:, j] = -G[i], -g[:, i] - 1.0
    ML = np.linalg.inv(qp.H) @ G.T
    return problems.QP(ML=ML, M=qp.M, G=G, g=g, L=float(np.linalg.norm(G @ ML, "fro")), H=qp.H, q=qp.q)


# ------------------------------------------------------------------------------------------ 1. surface (no GPU)
def test_surface():
    header = open(os.path.join(ROOT, "include", "gpad.h")).read()
    assert re.search(r"^int\s+gpad_infeasibility_resident\s*\(\s*gpad_handle_t\s+h\s*,\s*int\s+on\s*\)\s*;", header, re.M)
    lib = _lib.load()
    assert hasattr(lib, NAME) and NAME in _lib.EXPORTS
    assert callable(gpad_mpc.GpadSolver.set_infeasibility_resident)
    for on in (0, 1):
        assert lib.gpad_infeasibility_resident(None, on) == _lib.ERR_INVALID
        assert NAME in lib.gpad_last_error().decode()


@pytest.mark.parametrize("key", list(WIDE))
def test_wide_cases_cpu(oracle, key):
    """The wide draws do what the GPU tests take them for: the feasible one converges with codes in {1, 2} after
    at least 40 iterations (the CPU oracle, f32) to a z inside the bound, the contradictory one is certified
    before N by the reference in both precisions, and the reference never nominates the feasible one."""
    w, f, b = WIDE[key], wide(key, False), wide(key, True)
    for i in range(w.batch):
        z, _, it, code = oracle.solve_f32(np.zeros(w.n), np.zeros(w.m), F32(f.ML), F32(f.M[i]), F32(f.G),
                                          F32(f.g[i]), 2000, np.float32(f.L), tol=TOL, code=True)
        assert code in (1, 2) and 40 <= it < 2000 and np.abs(z).max() < min(w.R, 2.0), (i, it, code)
        for dt in (np.float32, np.float64):
            r = ref.solve(f.ML, f.M[i], f.G, f.g[i], f.L, 2000, TOL, w.R, dt)
            assert r.code in (1, 2) and r.nominated == 0, (i, dt, r.code, r.nominated)
            r = ref.solve(b.ML, b.M[i], b.G, b.g[i], b.L, N, TOL, w.R, dt)
            assert r.code == 5 and r.it < N and ref.farkas_margin(b.G, b.g[i], r.y, w.R) > 0.0, (i, dt, r.code, r.it)


# ---------------------------------------------------------------------------------------------------- 2. rules
@pytest.mark.gpu
def test_rules(gpu):
    p, b = cases.pack("2x4"), cases.batch("2x4", cases.BATCH, 2)
    qp, M, g = p.qp, b.M[:16], b.g[:16]
    RES, PAN, STR = _lib.KERNEL_RESIDENT, _lib.KERNEL_PANEL, _lib.KERNEL_STREAM
    with bound_solver(qp, F32, 16, kernel=STR) as s:
        want = run(s, F32, M, g)  # the stream kernel with the bound: what every engine must give
    assert 5 in want.cd and want.st["kernel"] == "stream"
    with gpad_mpc.GpadSolver(0) as s:  # valid any time after gpad_create; on outside 0 / 1 is refused
        for bad in (2, -1):
            assert s.lib.gpad_infeasibility_resident(s.h, bad) == _lib.ERR_INVALID
            assert NAME in s.lib.gpad_last_error().decode()
        assert s.lib.gpad_infeasibility_resident(s.h, 1) == _lib.GPAD_OK
        assert s.lib.gpad_infeasibility_resident(s.h, 0) == _lib.GPAD_OK
    # flag off: today's routing
    with flagged(qp, F32, 16, on=False, kernel=RES) as s:
        assert _code(lambda: run(s, F32, M, g))[0] == _lib.ERR_UNSUPPORTED
    with flagged(qp, F32, 16, on=False) as s:
        assert run(s, F32, M, g).st["kernel"] == "panel"
    with flagged(qp, F32, 16, on=False, shared=False) as s:
        assert run(s, F32, M, g).st["kernel"] == "stream"
    # flag on
    with flagged(qp, F32, 16, kernel=RES) as s:
        r = run(s, F32, M, g)
        assert r.st["kernel"] == "resident"
        same(r, want)
        assert s.last_phases()["ends"] == []  # last_phased is false on this path
    for shared in (True, False):
        with flagged(qp, F32, 16, shared=shared) as s:
            r = run(s, F32, M, g)
            assert r.st["kernel"] == "resident", shared
            same(r, want)
    with flagged(qp, F32, 16, kernel=PAN) as s:
        r = run(s, F32, M, g)
        assert r.st["kernel"] == "panel"
        same(r, want)
    with flagged(qp, F32, 16, kernel=PAN, shared=False) as s:
        assert _code(lambda: run(s, F32, M, g))[0] == _lib.ERR_UNSUPPORTED
    with flagged(qp, F32, 16, kernel=STR) as s:
        r = run(s, F32, M, g)
        assert r.st["kernel"] == "stream"
        same(r, want)
    with flagged(qp, F64, 16) as s:
        assert run(s, F64, M, g).st["kernel"] == "stream"
    with flagged(qp, F64, 16, kernel=RES) as s:
        assert _code(lambda: run(s, F64, M, g))[0] == _lib.ERR_UNSUPPORTED
    with flagged(qp, F32, 16, kernel=STR) as s:  # caller tables with a bound in force: refused as before
        th, be = gpad_mpc.schedule(N)
        z, y = np.zeros((16, p.n), np.float32), np.zeros((16, p.m), np.float32)
        pD = F32(-g / _L(qp, F32))
        assert _code(lambda: s.run(z, y, F32(M), pD, N, TOL, scaled=True, theta=F32(th), beta=F32(be)))[0] == \
            _lib.ERR_UNSUPPORTED
    # tol <= 0: exactly N iterations with codes 0, on the unbound run's kernel, whatever is bound and set
    with bound_solver(qp, F32, 16, bound=None) as s:
        plain = run(s, F32, M, g, 130, 0.0)
        never = run(s, F32, M, g)  # a handle that never saw the flag, no bound
    with flagged(qp, F32, 16) as s:
        fixed = run(s, F32, M, g, 130, 0.0)
        assert (fixed.it == 130).all() and (fixed.cd == 0).all() and fixed.st["kernel"] == plain.st["kernel"]
        same(fixed, plain)
        # the flag survives a second gpad_setup (which unbinds R) and the rebinding of R
        s.setup(F32(qp.ML), F32(qp.G), _L(qp, F32), n=p.n, m=p.m, batch=16)
        same(run(s, F32, M, g), never)  # no bound in force: today's run
        s.setup_infeasibility(R)
        r = run(s, F32, M, g)
        assert r.st["kernel"] == "resident"
        same(r, want)
        # R = 0 unbinds: bit for bit the run of a handle that never saw the flag
        s.setup_infeasibility(0.0)
        r = run(s, F32, M, g)
        assert r.st["kernel"] == never.st["kernel"]
        same(r, never)
    # m > 208: a forced RESIDENT stays unsupported (the resident kernel's own refusal), AUTO runs as with the flag off
    big = problems.synthetic_qp(24, 212, batch=2, seed=1)
    with flagged(big, F32, 2, bound=1e3, kernel=RES) as s:
        code, msg = _code(lambda: run(s, F32, big.M, big.g, 40, 1e-3))
        assert code == _lib.ERR_UNSUPPORTED and "208" in msg
    with flagged(big, F32, 2, bound=1e3, on=False) as s:
        off = run(s, F32, big.M, big.g, 40, 1e-3)
    with flagged(big, F32, 2, bound=1e3) as s:
        on = run(s, F32, big.M, big.g, 40, 1e-3)
    assert on.st["kernel"] == off.st["kernel"] != "resident"
    same(on, off)
    # a class binding forwards the flag to every class, set before or after gpad_setup_classes
    args = (F32(np.stack([qp.ML, qp.ML])), F32(np.stack([qp.G, qp.G])), _L(qp, F32), np.arange(16) % 2)
    for before in (True, False):
        with gpad_mpc.GpadSolver(0) as t:
            if before:
                t.set_infeasibility_resident(True)
            t.setup_classes(*args, n=p.n, m=p.m)
            if not before:
                t.set_infeasibility_resident(True)
            t.setup_infeasibility(R)
            r = run(t, F32, M, g)
            assert r.st["kernel"] == "resident", before
            same(r, want)
            t.set_infeasibility_resident(False)
            r = run(t, F32, M, g)
            assert r.st["kernel"] == "panel", before
            same(r, want)


# ----------------------------------------------------------------------------------------------- 3. one answer
@pytest.mark.gpu
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "distinct"])
@pytest.mark.parametrize("batch", [16, 33])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_answer(gpu, shape, batch, shared):
    """The certificate resident kernel, forced and by AUTO, against the forced stream kernel with the same bound:
    z, y, counts and codes byte-equal; and the contract of a code 5 on its results."""
    p, b, rf = cases.pack(shape), cases.batch(shape, cases.BATCH, 2), cases.reference(shape)
    M, g = b.M[:batch], b.g[:batch]
    with bound_solver(p.qp, F32, batch, kernel=_lib.KERNEL_STREAM, shared=shared) as s:
        want = run(s, F32, M, g)
    with flagged(p.qp, F32, batch, kernel=_lib.KERNEL_RESIDENT, shared=shared) as s:
        forced = run(s, F32, M, g)
    with flagged(p.qp, F32, batch, shared=shared) as s:
        auto = run(s, F32, M, g)
    print(shape, batch, "codes", forced.cd.tolist(), "counts", forced.it.tolist())
    assert (want.st["kernel"], forced.st["kernel"], auto.st["kernel"]) == ("stream", "resident", "resident")
    assert 5 in want.cd and (1 in want.cd or 2 in want.cd)
    same(forced, want)
    same(auto, want)
    G32, g32 = F32(p.qp.G), F32(g)
    margins = {i: gpad_mpc.farkas_margin(G32, g32[i], forced.y[i], R) for i in range(batch) if forced.cd[i] == 5}
    assert margins and all(v > 0.0 for v in margins.values()), margins
    for i in range(batch):
        if rf[i].code == 5:
            assert forced.cd[i] == 5 and forced.it[i] < N, (i, forced.cd[i], forced.it[i])
        else:
            assert forced.cd[i] in (1, 2), (i, forced.cd[i])
    for r in (forced, auto):  # aggregates: a certificate is no convergence
        assert r.st["converged"] == int(np.isin(r.cd, (1, 2)).sum())
        assert r.st["total_iterations"] == int(r.it.sum()) and r.st["iterations"] == int(r.it.max())


# -------------------------------------------------------------------------------------------- 4. no false alarm
def _quiet(qp, tol, bnd):
    """Forced RESIDENT unbound against flag on + bound on: the same bytes, converged past a certificate event."""
    batch = qp.M.shape[0]
    with bound_solver(qp, F32, batch, bound=None, kernel=_lib.KERNEL_RESIDENT) as s:
        off = run(s, F32, qp.M, qp.g, 2000, tol)
    with flagged(qp, F32, batch, bound=bnd, kernel=_lib.KERNEL_RESIDENT) as s:
        on = run(s, F32, qp.M, qp.g, 2000, tol)
    print("codes", sorted(set(off.cd.tolist())), "counts", off.it.min(), off.it.max())
    assert on.st["kernel"] == off.st["kernel"] == "resident"
    assert set(off.cd.tolist()) <= {1, 2}
    same(on, off)
    return off


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["battery_c1", "synth_small", "scenarios", "synthetic"])
def test_no_false_alarm(gpu, name):
    qp, tol = _feasible(name)
    off = _quiet(qp, tol, 1e3 if name in ("synth_small", "synthetic") else R)
    assert off.it.min() >= 40  # (every instance past a certificate event)


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(WIDE))
def test_no_false_alarm_wide(gpu, key):
    """n = 72: waves 0 and 1 own the -ML rows, the G/L waves' partials of q sit in slots 2 and 3; n = 204,
    m = 208: the largest bucket pair launches (kResidentMaxThreads) and is the unbound kernel's twin."""
    off = _quiet(wide(key, False), TOL, WIDE[key].R)
    assert off.it.min() >= 40


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(WIDE))
def test_infeasible_wide(gpu, key):
    """The contradictory rows at those widths: 5 before N on every instance, the stream kernel's bytes, shared
    and distinct matrices, and the certificate holds on the caller's f32 data."""
    qp, w = wide(key, True), WIDE[key]
    for shared in (True, False):
        with bound_solver(qp, F32, w.batch, bound=w.R, kernel=_lib.KERNEL_STREAM, shared=shared) as s:
            want = run(s, F32, qp.M, qp.g)
        with flagged(qp, F32, w.batch, bound=w.R, shared=shared) as s:
            r = run(s, F32, qp.M, qp.g)
        print("shared" if shared else "distinct", "codes", r.cd.tolist(), "counts", r.it.tolist())
        assert (want.st["kernel"], r.st["kernel"]) == ("stream", "resident")
        assert (r.cd == 5).all() and r.it.max() < N
        same(r, want)
        for i in range(w.batch):
            assert gpad_mpc.farkas_margin(F32(qp.G), F32(qp.g[i]), r.y[i], w.R) > 0.0


# --------------------------------------------------------------------------------------------------- 5. loops
def _loop_solver(mode, flag):
    """The loop modes of tests/test_infeasible.py with the bound bound and the flag as given; "fleet": a
    shared = 0 fleet of copies through setup_plant_batch + setup_signals."""
    p, I = cases.pack("4x10"), cases.loop_inputs()
    qp, pl, B = p.qp, p.pl, I.batch
    s = gpad_mpc.GpadSolver(0)
    if flag:
        s.set_infeasibility_resident(True)
    if mode in ("classes", "fused"):  # two classes of the same pack type, interleaved
        s.setup_classes(F32(np.stack([qp.ML, qp.ML])), F32(np.stack([qp.G, qp.G])), _L(qp, F32), np.arange(B) % 2,
                        n=p.n, m=p.m)
        s.setup_plant(F32(pl.PM), F32(pl.Pg), g0=F32(pl.g0), A=F32(pl.A), B=F32(pl.B))
        s.setup_class_signals(F32(pl.SM), F32(pl.Sg), F32(pl.E))
        if mode == "fused":
            s.set_class_loop_fused(True)
    elif mode == "fleet":
        st = lambda a: np.ascontiguousarray(np.broadcast_to(F32(a), (B,) + np.shape(a)))  # noqa: E731
        s.setup(st(qp.ML), st(qp.G), _L(qp, F32), n=p.n, m=p.m, batch=B, shared=False)
        s.setup_plant(st(pl.PM), st(pl.Pg), g0=st(pl.g0), A=st(pl.A), B=st(pl.B))
        s.setup_signals(st(pl.SM), st(pl.Sg), st(pl.E))
    else:
        s.setup(F32(qp.ML), F32(qp.G), _L(qp, F32), n=p.n, m=p.m, batch=B,
                kernel=_lib.KERNEL_STREAM if mode == "stream" else _lib.KERNEL_AUTO)
        s.setup_plant(F32(pl.PM), F32(pl.Pg), g0=F32(pl.g0), A=F32(pl.A), B=F32(pl.B))
        s.setup_signals(F32(pl.SM), F32(pl.Sg), F32(pl.E))
        if mode in ("loop_panel", "loop_async"):
            s.set_option(mode, 1)
    s.setup_infeasibility(R)
    return s


# the kernel each loop mode must report with the bound in force and the flag on
ENGINE = {"lockstep": "resident", "loop_async": "resident", "classes": "resident", "fleet": "resident",
          "loop_panel": "loop_panel", "fused": "loop_classes"}


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_loops(gpu, warm):
    """Flag on: the lockstep loop, loop_async (which falls back to it), a 2-class binding and a shared = 0 fleet
    run the certificate resident kernel, loop_panel and the fused class loop keep theirs; all give the bytes of
    the flag-off lockstep loop on the stream kernel, the 5s stand exactly at I.bad, and no solve runs to N."""
    I = cases.loop_inputs()
    with _loop_solver("stream", False) as s:
        base = _loop(s, I, warm)
    assert base.st["kernel"] == "stream"
    print("warm" if warm else "cold", "codes\n", base.cd, "\ncounts\n", base.it)
    for mode, engine in ENGINE.items():
        with _loop_solver(mode, True) as s:
            r = _loop(s, I, warm)
        assert r.st["kernel"] == engine, (mode, r.st["kernel"])
        for k in ("x", "z", "y", "xs", "us", "it", "cd"):
            assert getattr(r, k).tobytes() == getattr(base, k).tobytes(), (mode, k)
        assert r.st["converged"] == base.st["converged"], mode
    want = np.zeros_like(base.cd, dtype=bool)
    for b, t0 in I.bad.items():
        want[t0:, b] = True
    assert ((base.cd == 5) == want).all() and (base.cd[~want] > 0).all()
    assert base.it.max() < N
    assert base.st["converged"] == int((~want).sum())
