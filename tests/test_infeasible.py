"""Infeasibility certificates on the GPU (include/gpad.h gpad_setup_infeasibility): the contract of a code 5,
no false alarm on feasible batches, one answer whatever the matrices' layout and against the fp64 reference,
the closed loops, and the rules of the surface.  The branch lives in the stream kernel (any shape, f32 / f64,
shared or distinct matrices) and in the f32 T-wave panels (shared matrices), which AUTO runs with a bound in
force.

Inputs: tests/infeas_cases.py (asserted on the reference itself by tests/test_infeasible_cpu.py); reference:
tests/infeas_ref64.py.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest

import gpad_mpc
import infeas_cases as cases
from conftest import load_golden
from gpad_mpc import _lib, problems

pytestmark = pytest.mark.gpu

N, TOL, R = cases.N, cases.TOL, cases.R
F32 = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))  # noqa: E731
F64 = lambda a: None if a is None else np.ascontiguousarray(a, np.float64)  # noqa: E731


def _L(qp, c):
    return float(np.float32(qp.L)) if c is F32 else float(qp.L)


def bound_solver(qp, c, batch, *, bound=R, kernel=_lib.KERNEL_AUTO, shared=True):
    """A handle with qp's matrices bound (shared=False: a copy per instance) and the certificate's bound."""
    s = gpad_mpc.GpadSolver(0)
    ML, G = c(qp.ML), c(qp.G)
    if not shared:
        ML, G = np.ascontiguousarray(np.broadcast_to(ML, (batch,) + ML.shape)), np.ascontiguousarray(
            np.broadcast_to(G, (batch,) + G.shape))
    s.setup(ML, G, _L(qp, c), n=qp.n, m=qp.m, batch=batch, shared=shared, kernel=kernel)
    if bound is not None:
        s.setup_infeasibility(bound)
    return s


def run(s, c, M, g, N=N, tol=TOL):
    batch = M.shape[0]
    z, y = c(np.zeros_like(M)), c(np.zeros_like(g))
    it, cd = np.full(batch, -1, np.int32), np.full(batch, -1, np.int32)
    st = s.run(z, y, c(M), c(g), N, tol, iters=it, codes=cd)
    return SimpleNamespace(z=z, y=y, it=it, cd=cd, st=st)


def same(a, b):
    for k in ("z", "y", "it", "cd"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


def _code(fn):
    try:
        fn()
    except _lib.GpadError as e:
        return e.code, str(e)
    return _lib.GPAD_OK, ""


# the instances the reference certifies, by the fixed seeds of tests/infeas_cases.py
INFEASIBLE = {"2x4": [i for i in range(1, 33, 2) if i != 27], "4x10": list(range(1, 33, 2))}


# ---------------------------------------------------------------------------------------------- 1. contract
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "distinct"])
@pytest.mark.parametrize("batch", [16, 33])
@pytest.mark.parametrize("shape", ["2x4", "4x10"])
def test_contract(gpu, shape, batch, shared):
    """Every code 5 is a certificate on the caller's own f32 G, g and the returned y, and every instance the
    reference calls infeasible returns 5 before N."""
    p, b, ref = cases.pack(shape), cases.batch(shape, cases.BATCH, 2), cases.reference(shape)
    with bound_solver(p.qp, F32, batch, shared=shared) as s:
        r = run(s, F32, b.M[:batch], b.g[:batch])
    G32, g32 = F32(p.qp.G), F32(b.g[:batch])
    margins = {i: gpad_mpc.farkas_margin(G32, g32[i], r.y[i], R) for i in range(batch) if r.cd[i] == 5}
    print(shape, batch, r.st["kernel"], "codes", r.cd.tolist(), "counts", r.it.tolist(), "margins", margins)
    assert r.st["kernel"] == ("panel" if shared else "stream")
    assert all(v > 0.0 for v in margins.values()), margins
    infeasible = [i for i in range(batch) if ref[i].code == 5]
    assert infeasible == INFEASIBLE[shape][:len(infeasible)] and len(infeasible) == sum(
        i < batch for i in INFEASIBLE[shape])
    for i in infeasible:
        assert r.cd[i] == 5 and r.it[i] < N, (i, r.cd[i], r.it[i])
    for i in range(batch):
        if ref[i].code != 5:
            assert r.cd[i] in (1, 2), (i, r.cd[i])
    # aggregates: a certificate is no convergence
    assert r.st["converged"] == int(np.isin(r.cd, (1, 2)).sum())
    assert r.st["total_iterations"] == int(r.it.sum()) and r.st["iterations"] == int(r.it.max())


# ------------------------------------------------------------------------------ 2. no false alarm, bit for bit
def _feasible(name):
    if name in ("battery_c1", "synth_small"):
        gd = load_golden(name)
        return problems.QP(ML=gd["ML"], M=gd["M"][None], G=gd["G"], g=gd["g"][None], L=float(gd["L"])), 1e-3
    if name == "scenarios":
        return problems.battery_scenarios(4, 10, 33, seed=3), TOL
    return problems.synthetic_qp(24, 52, batch=33, seed=9), TOL


@pytest.mark.parametrize("engine", ["stream-f32", "stream-f64", "panel-f32"])
@pytest.mark.parametrize("name", ["battery_c1", "synth_small", "scenarios", "synthetic"])
def test_no_false_alarm(gpu, name, engine):
    """A feasible batch, per engine: bound on and off, z, y, counts and codes are identical (R = 1e3 for the
    synthetic QPs, whose z is not boxed by G; the battery bound for the others).  The panel runs of the batches of
    33 are phased (three panels, compaction at the phase ends); unbound, battery_c1 and scenarios (T = 12) run
    the pair layout, so that case also sets the T-wave variant against the pairs."""
    qp, tol = _feasible(name)
    batch = qp.M.shape[0]
    c = F64 if engine.endswith("f64") else F32
    kernel = _lib.KERNEL_PANEL if engine.startswith("panel") else _lib.KERNEL_STREAM
    bnd = 1e3 if name in ("synth_small", "synthetic") else R
    with bound_solver(qp, c, batch, bound=None, kernel=kernel) as s:
        off = run(s, c, qp.M, qp.g, 2000, tol)
        s.setup_infeasibility(bnd)
        on = run(s, c, qp.M, qp.g, 2000, tol)
        phases = s.last_phases()["ends"] if kernel == _lib.KERNEL_PANEL else None
    with bound_solver(qp, c, batch, bound=bnd) as s:  # AUTO: the panels for shared f32 matrices, else the stream kernel
        auto = run(s, c, qp.M, qp.g, 2000, tol)
    print(name, engine, "codes", sorted(set(off.cd.tolist())), "counts", off.it.min(), off.it.max(), "phases", phases)
    assert on.st["kernel"] == off.st["kernel"] == engine.split("-")[0]
    assert auto.st["kernel"] == ("panel" if c is F32 else "stream")
    assert set(off.cd.tolist()) <= {1, 2} and off.it.max() >= 40  # (converged, past a certificate event)
    if phases is not None and batch > 16:
        assert len(phases) >= 2
    same(on, off)
    same(auto, off)


# --------------------------------------------------------------------------------------------- 3. one answer
@pytest.mark.parametrize("batch", [16, 33])
@pytest.mark.parametrize("shape", ["2x4", "4x10"])
def test_stream_and_panel_agree(gpu, shape, batch):
    """Stream f32 against panel f32 on the mixed batches: z, y, counts and codes identical (one panel; three,
    the last ragged, phased)."""
    p, b = cases.pack(shape), cases.batch(shape, cases.BATCH, 2)
    with bound_solver(p.qp, F32, batch, kernel=_lib.KERNEL_STREAM) as s:
        a = run(s, F32, b.M[:batch], b.g[:batch])
    with bound_solver(p.qp, F32, batch, kernel=_lib.KERNEL_PANEL) as s:
        d = run(s, F32, b.M[:batch], b.g[:batch])
        phases = s.last_phases()
        s.set_option("phased", 0)  # one launch instead of phases: the same bits
        one = run(s, F32, b.M[:batch], b.g[:batch])
    print(shape, batch, "phases", phases["ends"], "codes", a.cd.tolist())
    assert (a.st["kernel"], d.st["kernel"], one.st["kernel"]) == ("stream", "panel", "panel")
    assert 5 in a.cd and 2 in a.cd and len(phases["ends"]) >= 2
    same(d, a)
    same(one, a)


@pytest.mark.parametrize("shape", ["2x4", "4x10"])
def test_shared_and_distinct_matrices_agree(gpu, shape):
    p, b = cases.pack(shape), cases.batch(shape, cases.BATCH, 2)
    with bound_solver(p.qp, F32, 33) as s:
        a = run(s, F32, b.M, b.g)
    with bound_solver(p.qp, F32, 33, shared=False) as s:
        d = run(s, F32, b.M, b.g)
    assert 5 in a.cd
    same(a, d)


@pytest.mark.parametrize("shape", ["1x2", "2x4", "4x10"])
def test_f64_matches_reference(gpu, shape):
    """f64 stream kernel against infeas_ref64: counts and codes equal, every entry of z and y within 1e-9
    (absolute; the figure tests/test_loop_f64.py asks of the f64 loop against its reference).  Measured on an
    MI355X: below 1e-12, with |y| up to 40."""
    p, b, ref = cases.pack(shape), cases.batch(shape, cases.BATCH, 2), cases.reference(shape)
    batch = 16
    with bound_solver(p.qp, F64, batch) as s:
        r = run(s, F64, b.M[:batch], b.g[:batch])
    far = lambda x, y: float(np.abs(x - y).max())  # noqa: E731
    devs = [max(far(r.z[i], ref[i].z), far(r.y[i], ref[i].y)) for i in range(batch)]
    dev = max(devs)
    print(shape, "codes", r.cd.tolist(), "counts", r.it.tolist(), "z / y deviation per instance",
          ["%.2g" % d for d in devs], "largest |y|", max(float(np.abs(x.y).max()) for x in ref[:batch]))
    assert r.st["kernel"] == "stream"
    assert r.it.tolist() == [ref[i].it for i in range(batch)]
    assert r.cd.tolist() == [ref[i].code for i in range(batch)]
    assert 5 in r.cd and dev <= 1e-9
    for i in range(batch):
        if r.cd[i] == 5:
            assert gpad_mpc.farkas_margin(F64(p.qp.G), F64(b.g[i]), r.y[i], R) > 0.0


# --------------------------------------------------------------------------------------------------- 4. loops
def _loop(s, I, warm, N=N, tol=TOL):
    n, m, B, steps = cases.pack("4x10").n, cases.pack("4x10").m, I.batch, I.steps
    x, z, y = F32(I.X0), np.zeros((B, n), np.float32), np.zeros((B, m), np.float32)
    xs, us = np.zeros((steps, B, 4), np.float32), np.zeros((steps, B, 4), np.float32)
    it, cd = np.full(steps * B, -1, np.int32), np.full(steps * B, -1, np.int32)
    st = s.closed_loop(x, z, y, steps, N, tol, warm=warm, xs=xs, us=us, iters=it, codes=cd, signals=F32(I.S))
    return SimpleNamespace(x=x, z=z, y=y, xs=xs, us=us, it=it.reshape(steps, B), cd=cd.reshape(steps, B), st=st)


def _loop_solver(mode, bound=R):
    p, I = cases.pack("4x10"), cases.loop_inputs()
    qp, pl = p.qp, p.pl
    s = gpad_mpc.GpadSolver(0)
    if mode in ("classes", "fused"):  # two classes of the same pack type, interleaved
        s.setup_classes(F32(np.stack([qp.ML, qp.ML])), F32(np.stack([qp.G, qp.G])), _L(qp, F32),
                        np.arange(I.batch) % 2, n=p.n, m=p.m)
        s.setup_plant(F32(pl.PM), F32(pl.Pg), g0=F32(pl.g0), A=F32(pl.A), B=F32(pl.B))
        s.setup_class_signals(F32(pl.SM), F32(pl.Sg), F32(pl.E))
        if mode == "fused":
            s.set_class_loop_fused(True)
    else:
        s.setup(F32(qp.ML), F32(qp.G), _L(qp, F32), n=p.n, m=p.m, batch=I.batch,
                kernel=_lib.KERNEL_STREAM if mode == "stream" else _lib.KERNEL_AUTO)
        s.setup_plant(F32(pl.PM), F32(pl.Pg), g0=F32(pl.g0), A=F32(pl.A), B=F32(pl.B))
        s.setup_signals(F32(pl.SM), F32(pl.Sg), F32(pl.E))
        if mode in ("loop_panel", "loop_async"):
            s.set_option(mode, 1)
    if bound:
        s.setup_infeasibility(bound)
    return s


# the kernel each loop mode must report with a bound in force: the asynchronous loop alone falls back to lockstep
ENGINE = {"lockstep": "panel", "stream": "stream", "loop_panel": "loop_panel", "loop_async": "panel", "classes": "panel",
          "fused": "loop_classes"}


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_loops(gpu, warm):
    """Six steps, two of 16 packs infeasible from steps 3 and 2 on: the lockstep loop, the loop options, a
    2-class binding and the fused class loop, each on its own engine (ENGINE), and a lockstep loop on the stream
    kernel give the same bits; the 5s stand where the load makes the step infeasible, and no solve runs to N."""
    I = cases.loop_inputs()
    runs = {}
    for mode in ("lockstep", "stream", "loop_panel", "loop_async", "classes", "fused"):
        with _loop_solver(mode) as s:
            runs[mode] = _loop(s, I, warm)
        assert runs[mode].st["kernel"] == ENGINE[mode], (mode, runs[mode].st["kernel"])
    base = runs["lockstep"]
    print("warm" if warm else "cold", "codes\n", base.cd, "\ncounts\n", base.it)
    for mode, r in runs.items():
        for k in ("x", "z", "y", "xs", "us", "it", "cd"):
            assert getattr(r, k).tobytes() == getattr(base, k).tobytes(), (mode, k)
    want = np.zeros_like(base.cd, dtype=bool)
    for b, t0 in I.bad.items():
        want[t0:, b] = True
    assert ((base.cd == 5) == want).all() and (base.cd[~want] > 0).all()
    assert base.it.max() < N
    assert base.st["converged"] == int((~want).sum())
    G32 = F32(cases.pack("4x10").qp.G)
    for b in I.bad:  # the last step's y is returned: its certificate holds on g(x, s) of that step
        xa = np.concatenate([base.xs[-1, b], F32(I.S)[-1, b]]).astype(np.float64)
        pl = cases.pack("4x10").pl
        g = F32(pl.g0).astype(np.float64) + np.hstack([F32(pl.Pg), F32(pl.Sg)]).astype(np.float64) @ xa
        assert gpad_mpc.farkas_margin(G32, F32(g), base.y[b], R) > 0.0
    # without the bound the same loop is today's: the infeasible steps run to N with code 0
    if not warm:
        with _loop_solver("lockstep", bound=None) as s:
            r = _loop(s, I, warm)
        assert ((r.cd == 0) == want).all() and (r.it[want] == N).all()
        assert r.it[~want].tobytes() == base.it[~want].tobytes()


# --------------------------------------------------------------------------------------------------- 5. rules
def test_rules(gpu):
    p, b = cases.pack("2x4"), cases.batch("2x4", cases.BATCH, 2)
    qp, M, g = p.qp, b.M[:16], b.g[:16]
    s = gpad_mpc.GpadSolver(0)
    lib = s.lib
    assert lib.gpad_setup_infeasibility(s.h, R) == _lib.ERR_NOT_SETUP
    s.setup(F32(qp.ML), F32(qp.G), _L(qp, F32), n=p.n, m=p.m, batch=16)
    for bad in (-0.1, float("inf"), float("nan")):
        assert lib.gpad_setup_infeasibility(s.h, bad) == _lib.ERR_INVALID
    before = run(s, F32, M, g)                     # today's engines: the infeasible instances run to N
    assert before.st["kernel"] != "stream" and 5 not in before.cd and before.it.max() == N
    s.setup_infeasibility(R)
    on = run(s, F32, M, g)
    assert 5 in on.cd and on.it.max() < N and on.st["kernel"] == "panel"
    fixed = run(s, F32, M, g, 130, 0.0)            # tol <= 0: exactly N iterations, bound or not
    assert (fixed.it == 130).all() and (fixed.cd == 0).all() and fixed.st["kernel"] == before.st["kernel"]
    s.setup_infeasibility(0.0)                     # unbinds: today's results, bit for bit
    same(run(s, F32, M, g), before)
    s.setup_infeasibility(R)
    s.setup(F32(qp.ML), F32(qp.G), _L(qp, F32), n=p.n, m=p.m, batch=16)  # every gpad_setup* unbinds
    same(run(s, F32, M, g), before)
    # a Hessian and a bound exclude each other, either way round
    s.setup_infeasibility(R)
    assert _code(lambda: s.setup_hessian(F32(qp.H)))[0] == _lib.ERR_UNSUPPORTED
    s.setup_hessian(None)
    s.setup_infeasibility(0.0)
    s.setup_hessian(F32(qp.H))
    assert _code(lambda: s.setup_infeasibility(R))[0] == _lib.ERR_UNSUPPORTED
    s.setup_infeasibility(0.0)
    s.close()
    # forced engines without the branch, with a bound in force (tol > 0); with tol <= 0 they run
    with bound_solver(qp, F32, 16, kernel=_lib.KERNEL_RESIDENT) as t:
        assert _code(lambda: run(t, F32, M, g))[0] == _lib.ERR_UNSUPPORTED
        assert (run(t, F32, M, g, 50, 0.0).it == 50).all()
    with bound_solver(qp, F32, 16, kernel=_lib.KERNEL_PANEL) as t:  # the T-wave panels carry it
        same(run(t, F32, M, g), on)
    with bound_solver(qp, F32, 16, kernel=_lib.KERNEL_PANEL, shared=False) as t:  # ... for shared matrices
        assert _code(lambda: run(t, F32, M, g))[0] == _lib.ERR_UNSUPPORTED
    with bound_solver(qp, F64, 16, kernel=_lib.KERNEL_PANEL) as t:  # ... in f32
        assert _code(lambda: run(t, F64, M, g))[0] == _lib.ERR_UNSUPPORTED
    big = problems.synthetic_qp(24, 260, batch=2, seed=1)  # m > 256: the big panels do not carry it
    with bound_solver(big, F32, 2, bound=1e3, kernel=_lib.KERNEL_PANEL) as t:
        assert _code(lambda: run(t, F32, big.M, big.g, 40, 1e-3))[0] == _lib.ERR_UNSUPPORTED
    with bound_solver(big, F32, 2, bound=1e3) as t:
        assert run(t, F32, big.M, big.g, 40, 1e-3).st["kernel"] == "stream"
    with bound_solver(qp, F32, 16, kernel=_lib.KERNEL_STREAM) as t:
        same(run(t, F32, M, g), on)
        # gpad_run_scaled with caller tables
        th, be = gpad_mpc.schedule(N)
        z, y = np.zeros((16, p.n), np.float32), np.zeros((16, p.m), np.float32)
        pD = F32(-g / _L(qp, F32))
        assert _code(lambda: t.run(z, y, F32(M), pD, N, TOL, scaled=True, theta=F32(th), beta=F32(be)))[0] == \
            _lib.ERR_UNSUPPORTED
        t.run(z, y, F32(M), pD, N, TOL, scaled=True)  # the library's own schedule: served
    # a flat setup has no binding
    fq = problems.battery_mpc(2, 4)
    MGf, GLf, Lf = problems.flatten_battery(fq, 2, 4)
    with gpad_mpc.GpadSolver(0) as t:
        t.setup_flat(F32(MGf), F32(GLf), Lf, n_u=2, batch=4)
        assert _code(lambda: t.setup_infeasibility(R))[0] == _lib.ERR_UNSUPPORTED
        t.setup_infeasibility(0.0)
    # a class binding forwards the bound to every class, and a new binding drops it
    with gpad_mpc.GpadSolver(0) as t:
        args = (F32(np.stack([qp.ML, qp.ML])), F32(np.stack([qp.G, qp.G])), _L(qp, F32), np.arange(16) % 2)
        t.setup_classes(*args, n=p.n, m=p.m)
        plain = run(t, F32, M, g)
        assert 5 not in plain.cd
        t.setup_infeasibility(R)
        same(run(t, F32, M, g), on)
        t.setup_classes(*args, n=p.n, m=p.m)
        same(run(t, F32, M, g), plain)
