"""Infeasibility certificates in the asynchronous closed loop (include/gpad.h gpad_infeasibility_loop_async): the
surface, the routing rules of the per-handle flag, the loops bit for bit against the bound lockstep loop on the
stream kernel, a wide plant, and no false alarm.

gpad_loop_farkas_kernel (one plant, per-pack plant maps) and gpad_loop_fleet_farkas_kernel (distinct matrices) are
the asynchronous loop kernels' text with the rule of csrc/gpad_farkas.h after every fourth test of a pack's own
solve; a code 5 is a termination like any other at the step boundary.  The flag is off by default, and
tests/test_infeasible.py and tests/test_infeasible_resident.py pin what runs then.

Inputs: tests/infeas_cases.py and the helpers of tests/test_infeasible.py; reference: tests/infeas_ref64.py.  The
wide plant is test_loop_async.synthetic(70, 130, 5, 2) -- two -ML waves, three G/L waves with the last ragged --
and the same plant with two contradictory rows in the matrices and in the maps, so that every step of every pack
is infeasible.  Its rows and bound are asserted on the CPU (test_wide_plant_cpu).
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
import test_loop_async as tla
from conftest import ROOT
from gpad_mpc import _lib, problems
from test_infeasible import F32, _L, _loop

N, TOL, R = cases.N, cases.TOL, cases.R
NAME = "gpad_infeasibility_loop_async"
KEYS = ("x", "z", "y", "xs", "us", "it", "cd")
# the wide plant: rows i (wave 0) and j (the ragged third G/L wave) contradict each other; R bounds |z|_inf of
# the feasible twin's solutions (below 2) with room
WIDE = SimpleNamespace(rows=(3, 129), R=1e3, N=3000, packs=6, steps=3)


@functools.lru_cache(maxsize=None)
def wide(infeasible):
    """test_loop_async.synthetic(70, 130, 5, 2); infeasible: G_j = -G_i in the matrices (ML and L recomputed from
    the new G) and Pg_j = -Pg_i, g0_j = -g0_i - 1 in the maps, so g_j(x) = -g_i(x) - 1 at every state: no z meets
    both rows, and y = e_i + e_j certifies it for any R."""
    p = tla.synthetic(70, 130, 5, 2)
    if not infeasible:
        return p
    i, j = WIDE.rows
    qp = p.qp
    G, g0, Pg = qp.G.copy(), np.array(p.g0, np.float64), p.Pg.copy()
    G[j], Pg[j] = -G[i], -Pg[i]
    g0[..., j] = -g0[..., i] - 1.0
    ML = np.linalg.inv(qp.H) @ G.T
    nq = problems.QP(ML=ML, M=qp.M, G=G, g=g0.reshape(qp.g.shape), L=float(np.linalg.norm(G @ ML, "fro")), H=qp.H,
                     q=qp.q)
    return SimpleNamespace(qp=nq, PM=p.PM, Pg=Pg, M0=p.M0, g0=g0.reshape(np.shape(p.g0)), A=p.A, B=p.B, nx=p.nx,
                           nu=p.nu, X0=p.X0)


def _same(r, base, what):
    for k in KEYS:
        assert getattr(r, k).tobytes() == getattr(base, k).tobytes(), (what, k)
    assert r.st["converged"] == base.st["converged"], what


# ------------------------------------------------------------------------------------------ 1. surface (no GPU)
def test_surface():
    header = open(os.path.join(ROOT, "include", "gpad.h")).read()
    assert re.search(r"^int\s+gpad_infeasibility_loop_async\s*\(\s*gpad_handle_t\s+h\s*,\s*int\s+on\s*\)\s*;", header,
                     re.M)
    lib = _lib.load()
    assert hasattr(lib, NAME) and NAME in _lib.EXPORTS
    assert lib.gpad_infeasibility_loop_async.argtypes is not None and len(lib.gpad_infeasibility_loop_async.argtypes) == 2
    assert callable(gpad_mpc.GpadSolver.set_infeasibility_loop_async)
    for on in (0, 1, 2, -1):
        assert lib.gpad_infeasibility_loop_async(None, on) == _lib.ERR_INVALID
        assert NAME in lib.gpad_last_error().decode()


# ------------------------------------------------------------------------------- 2. the wide plant on the CPU
def test_wide_plant_cpu(oracle):
    """At the initial states the contradictory plant is certified before N by the reference in f32 and f64, and
    its feasible twin converges with codes in {1, 2} after at least 40 iterations (the CPU oracle, f32) to a z
    inside the bound, without a nomination."""
    f, b = wide(False), wide(True)
    assert (len(f.X0), f.qp.n, f.qp.m) == (WIDE.packs, 70, 130)
    for k in range(WIDE.packs):
        x = f.X0[k].astype(np.float64)
        Mf, gf = np.ravel(f.M0) + f.PM @ x, np.ravel(f.g0) + f.Pg @ x
        Mb, gb = np.ravel(b.M0) + b.PM @ x, np.ravel(b.g0) + b.Pg @ x
        i, j = WIDE.rows
        assert abs(gb[j] + gb[i] + 1.0) < 1e-12
        z, _, it, code = oracle.solve_f32(np.zeros(70), np.zeros(130), F32(f.qp.ML), F32(Mf), F32(f.qp.G), F32(gf),
                                          WIDE.N, np.float32(f.qp.L), tol=TOL, code=True)
        assert code in (1, 2) and 40 <= it < WIDE.N and np.abs(z).max() < min(WIDE.R, 2.0), (k, it, code)
        for dt in (np.float32, np.float64):
            r = ref.solve(f.qp.ML, Mf, f.qp.G, gf, f.qp.L, WIDE.N, TOL, WIDE.R, dt)
            assert r.code in (1, 2) and r.it >= 40 and r.nominated == 0, (k, dt, r.code, r.it, r.nominated)
            r = ref.solve(b.qp.ML, Mb, b.qp.G, gb, b.qp.L, WIDE.N, TOL, WIDE.R, dt)
            assert r.code == 5 and r.it < WIDE.N and ref.farkas_margin(b.qp.G, gb, r.y, WIDE.R) > 0.0, \
                (k, dt, r.code, r.it)
    # the feasible twin's cold closed loop (the CPU oracle, whose counts the loop kernels reproduce): every solve of
    # the GPU test's steps passes a certificate event and ends before N
    orc = tla.oracle_loop(oracle, "s70-infeasible-loop", f, f.X0, WIDE.steps, WIDE.N, TOL, False)
    assert 40 <= orc.it.min() and orc.it.max() < WIDE.N, (orc.it.min(), orc.it.max())


# ---------------------------------------------------------------------------------------------------- solvers
def _loop_solver(mode, I, *, flag=True, grid=0, bound=R, async_=True):
    """A bound closed loop of 4x10 packs: "stream" (the lockstep loop on the stream kernel, the base), "shared"
    (one plant), "plant" (per-pack copies of the maps through the stacked setup_plant on shared matrices), "fleet"
    (shared = 0, copies of the matrices and the maps) and "classes" (a 2-class binding, the option forwarded)."""
    p = cases.pack("4x10")
    qp, pl, B = p.qp, p.pl, I.batch
    st = lambda a: np.ascontiguousarray(np.broadcast_to(F32(a), (B,) + np.shape(a)))  # noqa: E731
    s = gpad_mpc.GpadSolver(0)
    if flag:
        s.set_infeasibility_loop_async(True)  # (before every setup: it must survive them)
    if mode == "classes":
        s.setup_classes(F32(np.stack([qp.ML, qp.ML])), F32(np.stack([qp.G, qp.G])), _L(qp, F32), np.arange(B) % 2,
                        n=p.n, m=p.m)
        s.setup_plant(F32(pl.PM), F32(pl.Pg), g0=F32(pl.g0), A=F32(pl.A), B=F32(pl.B))
        s.setup_class_signals(F32(pl.SM), F32(pl.Sg), F32(pl.E))
    elif mode == "fleet":
        s.setup(st(qp.ML), st(qp.G), _L(qp, F32), n=p.n, m=p.m, batch=B, shared=False)
        s.setup_plant(st(pl.PM), st(pl.Pg), g0=st(pl.g0), A=st(pl.A), B=st(pl.B))
        s.setup_signals(st(pl.SM), st(pl.Sg), st(pl.E))
    else:
        s.setup(F32(qp.ML), F32(qp.G), _L(qp, F32), n=p.n, m=p.m, batch=B,
                kernel=_lib.KERNEL_STREAM if mode == "stream" else _lib.KERNEL_AUTO)
        if mode == "plant":
            s.setup_plant(st(pl.PM), st(pl.Pg), g0=st(pl.g0), A=st(pl.A), B=st(pl.B))
            s.setup_signals(st(pl.SM), st(pl.Sg), st(pl.E))
        else:
            s.setup_plant(F32(pl.PM), F32(pl.Pg), g0=F32(pl.g0), A=F32(pl.A), B=F32(pl.B))
            s.setup_signals(F32(pl.SM), F32(pl.Sg), F32(pl.E))
    if async_ and mode != "stream":
        s.set_option("loop_async", 1)
    if grid:
        s.set_option("duo_max_grid", grid)
    if bound:
        s.setup_infeasibility(bound)
    return s


_base = {}


def base_of(I, warm):
    """The bound lockstep loop on the stream kernel, once per input set and start."""
    k = (I.batch, I.steps, warm)
    if k not in _base:
        with _loop_solver("stream", I, flag=False) as s:
            _base[k] = _loop(s, I, warm)
        assert _base[k].st["kernel"] == "stream"
    return _base[k]


# ---------------------------------------------------------------------------------------------------- 3. rules
@pytest.mark.gpu
def test_rules(gpu):
    I = cases.loop_inputs()
    base = base_of(I, False)
    with gpad_mpc.GpadSolver(0) as s:  # valid any time after gpad_create; on outside 0 / 1 is refused
        for bad in (2, -1):
            assert s.lib.gpad_infeasibility_loop_async(s.h, bad) == _lib.ERR_INVALID
            assert NAME in s.lib.gpad_last_error().decode()
        assert s.lib.gpad_infeasibility_loop_async(s.h, 1) == _lib.GPAD_OK
        assert s.lib.gpad_infeasibility_loop_async(s.h, 0) == _lib.GPAD_OK
    with _loop_solver("shared", I, flag=False) as s:  # flag off: the lockstep loop, as today
        r = _loop(s, I, False)
        assert r.st["kernel"] == "panel"
        _same(r, base, "flag off")
    with _loop_solver("shared", I, bound=None, flag=False) as s:  # the unbound loop_async runs of a handle that never saw the flag
        never = _loop(s, I, False)
        fixed0 = _loop(s, I, False, 130, 0.0)
    assert never.st["kernel"] == fixed0.st["kernel"] == "loop"
    with _loop_solver("shared", I) as s:  # the flag was set before setup, setup_plant, setup_signals and the bound
        r = _loop(s, I, False)
        assert r.st["kernel"] == "loop"
        _same(r, base, "flag on")
        fixed = _loop(s, I, False, 130, 0.0)  # tol = 0: the unbound kernel, N iterations, codes 0
        assert fixed.st["kernel"] == "loop" and (fixed.it == 130).all() and (fixed.cd == 0).all()
        _same(fixed, fixed0, "tol = 0")
        s.setup_infeasibility(0.0)  # no bound: the unbound loop_async run
        r = _loop(s, I, False)
        assert r.st["kernel"] == "loop"
        _same(r, never, "unbound")
        s.setup_infeasibility(R)  # the flag survives the rebinding of the bound
        r = _loop(s, I, False)
        assert r.st["kernel"] == "loop"
        _same(r, base, "rebound")
        s.set_infeasibility_loop_async(False)
        assert _loop(s, I, False).st["kernel"] == "panel"
    p = cases.pack("4x10")
    with gpad_mpc.GpadSolver(0) as s:  # a forced stream kernel is no shape of the loop
        s.set_infeasibility_loop_async(True)
        s.setup(F32(p.qp.ML), F32(p.qp.G), _L(p.qp, F32), n=p.n, m=p.m, batch=I.batch, kernel=_lib.KERNEL_STREAM)
        s.setup_plant(F32(p.pl.PM), F32(p.pl.Pg), g0=F32(p.pl.g0), A=F32(p.pl.A), B=F32(p.pl.B))
        s.setup_signals(F32(p.pl.SM), F32(p.pl.Sg), F32(p.pl.E))
        s.set_option("loop_async", 1)
        s.setup_infeasibility(R)
        r = _loop(s, I, False)
        assert r.st["kernel"] == "stream"
        _same(r, base, "forced stream")


# ---------------------------------------------------------------------------------------------------- 4. loops
MODES = ["shared", "plant", "fleet", "classes"]


def _check_bad(I, base):
    want = np.zeros_like(base.cd, dtype=bool)
    for b, t0 in I.bad.items():
        if b < I.batch:
            want[t0:, b] = True
    assert ((base.cd == 5) == want).all() and (base.cd[~want] > 0).all()
    assert base.it.max() < N
    assert base.st["converged"] == int((~want).sum())
    p = cases.pack("4x10")
    G32, pl = F32(p.qp.G), p.pl
    for b in I.bad:  # the last step's y is returned: its certificate holds on g(x, s) of that step
        if b >= I.batch:
            continue
        xa = np.concatenate([base.xs[-1, b], F32(I.S)[-1, b]]).astype(np.float64)
        g = F32(pl.g0).astype(np.float64) + np.hstack([F32(pl.Pg), F32(pl.Sg)]).astype(np.float64) @ xa
        assert gpad_mpc.farkas_margin(G32, F32(g), base.y[b], R) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [0, 2], ids=["grid0", "grid2"])
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("mode", MODES)
def test_loops(gpu, mode, warm, grid):
    """16 packs, six steps, packs 3 and 10 infeasible from steps 3 and 2 on: every mode of the asynchronous loop
    with the flag on gives the bytes of the bound lockstep loop on the stream kernel.  With two workgroups every
    one claims from the queue: a slot certifies, steps on and refills while its neighbour is mid-solve, and the
    solo tail runs."""
    I = cases.loop_inputs()
    base = base_of(I, warm)
    with _loop_solver(mode, I, grid=grid) as s:
        r = _loop(s, I, warm)
    print(mode, "warm" if warm else "cold", grid, "codes\n", r.cd, "\ncounts\n", r.it)
    assert r.st["kernel"] == "loop", (mode, r.st["kernel"])
    _same(r, base, mode)
    _check_bad(I, r)


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("mode", MODES)
def test_loops_odd_batch(gpu, mode, warm):
    """11 packs on four workgroups: the second slots are partly empty from the start."""
    I = cases.loop_inputs(batch_size=11)
    base = base_of(I, warm)
    with _loop_solver(mode, I, grid=4) as s:
        r = _loop(s, I, warm)
    assert r.st["kernel"] == "loop", (mode, r.st["kernel"])
    _same(r, base, mode)
    _check_bad(I, r)


# ------------------------------------------------------------------------------------------------ 5. wide loop
def _wide_solver(p, mode, *, bound, flag=True, grid=2):
    B = len(p.X0)
    qp = p.qp
    st = lambda a: np.ascontiguousarray(np.broadcast_to(F32(a), (B,) + np.shape(a)))  # noqa: E731
    s = gpad_mpc.GpadSolver(0)
    if flag:
        s.set_infeasibility_loop_async(True)
    if mode == "fleet":
        s.setup(st(qp.ML), st(qp.G), _L(qp, F32), n=qp.n, m=qp.m, batch=B, shared=False)
        s.setup_plant(st(p.PM), st(p.Pg), M0=st(np.ravel(p.M0)), g0=st(np.ravel(p.g0)), A=st(p.A), B=st(p.B))
    else:
        s.setup(F32(qp.ML), F32(qp.G), _L(qp, F32), n=qp.n, m=qp.m, batch=B,
                kernel=_lib.KERNEL_STREAM if mode == "stream" else _lib.KERNEL_AUTO)
        s.setup_plant(F32(p.PM), F32(p.Pg), M0=F32(np.ravel(p.M0)), g0=F32(np.ravel(p.g0)), A=F32(p.A), B=F32(p.B))
    if mode != "stream":
        s.set_option("loop_async", 1)
        s.set_option("duo_max_grid", grid)
    if bound:
        s.setup_infeasibility(bound)
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_wide_loop(gpu, warm):
    """The contradictory plant: two -ML waves, so the G/L waves' rows and partials are found behind them; every
    step of every pack ends with a 5 before N, on the shared plant and as a shared = 0 fleet, with the bytes of
    the bound lockstep loop on the stream kernel."""
    p = wide(True)
    with _wide_solver(p, "stream", bound=WIDE.R, flag=False) as s:
        base = tla.loop(s, p, p.X0, WIDE.steps, WIDE.N, TOL, warm)
    assert base.st["kernel"] == "stream"
    print("codes\n", base.cd, "\ncounts\n", base.it)
    assert (base.cd == 5).all() and base.it.max() < WIDE.N
    for mode in ("shared", "fleet"):
        with _wide_solver(p, mode, bound=WIDE.R) as s:
            r = tla.loop(s, p, p.X0, WIDE.steps, WIDE.N, TOL, warm)
        assert r.st["kernel"] == "loop", mode
        _same(r, base, mode)


# -------------------------------------------------------------------------------------------- 6. no false alarm
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["shared", "fleet"])
def test_no_false_alarm(gpu, mode):
    """Two steps, before any pack turns infeasible: flag on, bound on against bound off, the same bytes from the
    same engine, every solve converged past a certificate event."""
    I = cases.loop_inputs(steps=2)
    with _loop_solver(mode, I, bound=None, grid=2) as s:
        off = _loop(s, I, False)
        s.setup_infeasibility(R)
        on = _loop(s, I, False)
    print("codes", sorted(set(off.cd.ravel().tolist())), "counts", off.it.min(), off.it.max())
    assert on.st["kernel"] == off.st["kernel"] == "loop"
    assert set(off.cd.ravel().tolist()) <= {1, 2} and off.it.min() >= 40
    _same(on, off, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["shared", "fleet"])
def test_no_false_alarm_wide(gpu, mode):
    p = wide(False)
    with _wide_solver(p, mode, bound=None) as s:
        off = tla.loop(s, p, p.X0, WIDE.steps, WIDE.N, TOL, False)
        s.setup_infeasibility(WIDE.R)
        on = tla.loop(s, p, p.X0, WIDE.steps, WIDE.N, TOL, False)
    print("codes", sorted(set(off.cd.ravel().tolist())), "counts", off.it.min(), off.it.max())
    assert on.st["kernel"] == off.st["kernel"] == "loop"
    assert set(off.cd.ravel().tolist()) <= {1, 2} and off.it.min() >= 40
    _same(on, off, mode)
