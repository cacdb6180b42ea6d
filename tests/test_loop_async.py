"""The asynchronous closed loop (GPAD_OPT_LOOP_ASYNC, csrc/gpad_loop.hip): one launch in which every
pack advances to its next MPC step as soon as its own solve ends.

The contract is bit identity: with the option on, x, z, y, xs, us, the per-step counts and codes and
every aggregate stat equal gpad_closed_loop with the option off, and the trajectories and counts
equal the CPU oracle's closed loop.  Inputs follow test_plant_io.test_closed_loop_bitexact.  The
oracle and the lockstep run of a configuration are computed once and shared by the cases that vary
only the grid.
"""
from __future__ import annotations

import functools
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT

F32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))  # noqa: E731
F64 = lambda a: np.ascontiguousarray(a, np.float64)  # noqa: E731
STAT_KEYS = ("iterations", "converged", "total_iterations", "below_tol_floor", "nonfinite_g")


# ------------------------------------------------------------------------------ problems
@functools.lru_cache(maxsize=None)
def battery(n_u, Nh):
    from gpad_mpc import problems
    qp, pl = problems.battery_plant(n_u, Nh)
    return SimpleNamespace(qp=qp, PM=pl.PM, Pg=pl.Pg, M0=None, g0=pl.g0, A=pl.A, B=pl.B, nx=n_u, nu=n_u,
                           X0=None)


@functools.lru_cache(maxsize=None)
def synthetic(n, m, nx, nu, packs=6, seed=11):
    """A generic plant on a synthetic QP: both affine maps with a constant term (M0, g0 bound),
    nx != nu, a contracting A (0.9 x orthogonal).  seed: of the maps and X0 (the QP is seed 1's)."""
    from gpad_mpc import problems
    qp = problems.synthetic_qp(n, m, batch=1, seed=1)
    rng = np.random.default_rng(seed)
    PM = 0.1 * rng.standard_normal((n, nx))
    Pg = 0.05 * rng.standard_normal((m, nx))
    Q, _ = np.linalg.qr(rng.standard_normal((nx, nx)))
    A = 0.9 * Q
    B = 0.1 * rng.standard_normal((nx, nu))
    X0 = np.stack([rng.uniform(-1, 1, nx) for _ in range(packs)]).astype(np.float32)
    return SimpleNamespace(qp=qp, PM=PM, Pg=Pg, M0=qp.M, g0=qp.g, A=A, B=B, nx=nx, nu=nu, X0=X0)


def states(p, batch, seed):
    return (np.random.default_rng(seed).random((batch, p.nx)) - 0.5).astype(np.float32)


# ------------------------------------------------------------------------------ runs
def make_solver(p, batch, kernel=None, dtype=np.float32):
    import gpad_mpc
    from gpad_mpc import _lib
    c = F64 if dtype == np.float64 else F32
    qp = p.qp
    L = float(qp.L) if dtype == np.float64 else float(np.float32(qp.L))
    s = gpad_mpc.GpadSolver(0)
    s.setup(c(qp.ML), c(qp.G), L, n=qp.n, m=qp.m, batch=batch, shared=True,
            kernel=_lib.KERNEL_AUTO if kernel is None else kernel)
    opt = lambda a: None if a is None else c(a)  # noqa: E731
    s.setup_plant(c(p.PM), c(p.Pg), M0=opt(p.M0), g0=opt(p.g0), A=c(p.A), B=c(p.B))
    return s


def loop(s, p, X0, steps, N, tol, warm, dtype=np.float32):
    """One closed loop on host arrays from Z = Y = 0; returns every output and the stats."""
    batch = X0.shape[0]
    X = X0.astype(dtype).copy()
    Z = np.zeros((batch, p.qp.n), dtype)
    Y = np.zeros((batch, p.qp.m), dtype)
    XS = np.zeros((steps, batch, p.nx), dtype)
    US = np.zeros((steps, batch, p.nu), dtype)
    IT = np.full(steps * batch, -1, np.int32)
    CD = np.full(steps * batch, -1, np.int32)
    st = s.closed_loop(X, Z, Y, steps, N, tol, warm=warm, xs=XS, us=US, iters=IT, codes=CD)
    return SimpleNamespace(x=X, z=Z, y=Y, xs=XS, us=US, it=IT.reshape(steps, batch), cd=CD.reshape(steps, batch),
                           st=st)


def run(p, X0, steps, N, tol, warm, *, async_=False, grid=0, kernel=None, dtype=np.float32):
    s = make_solver(p, X0.shape[0], kernel=kernel, dtype=dtype)
    if async_:
        s.set_option("loop_async", 1)
    if grid:
        s.set_option("duo_max_grid", grid)
    return loop(s, p, X0, steps, N, tol, warm, dtype)


_lockstep_cache = {}


def lockstep(key, p, X0, steps, N, tol, warm):
    """The lockstep run of a configuration, once per session."""
    k = (key, X0.tobytes(), steps, N, tol, warm)
    if k not in _lockstep_cache:
        _lockstep_cache[k] = run(p, X0, steps, N, tol, warm)
        assert _lockstep_cache[k].st["kernel"] != "loop"
    return _lockstep_cache[k]


_oracle_cache = {}


def oracle_loop(oracle, key, p, X0, steps, N, tol, warm):
    """The CPU oracle's closed loop of every pack, once per session: (x, z, y, xs, us, it)."""
    k = (key, X0.tobytes(), steps, N, tol, warm)
    if k not in _oracle_cache:
        qp = p.qp
        L = np.float32(qp.L)
        MGneg, GL, _ = oracle.scale(F32(qp.ML), F32(qp.G), F32(np.zeros(qp.m)), L)
        rows = [oracle.closed_loop_f32(X0[b], MGneg, GL, L, p.PM, p.Pg, p.A, p.B, steps, N, tol, M0=p.M0,
                                       g0=p.g0, warm=warm) for b in range(X0.shape[0])]
        _oracle_cache[k] = SimpleNamespace(
            x=np.stack([r[0] for r in rows]), z=np.stack([r[1] for r in rows]), y=np.stack([r[2] for r in rows]),
            xs=np.stack([r[3] for r in rows], axis=1), us=np.stack([r[4] for r in rows], axis=1),
            it=np.stack([r[5] for r in rows], axis=1))
    return _oracle_cache[k]


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert a.tobytes() == b.tobytes(), f"{what}: {int((a.view(np.uint8) != b.view(np.uint8)).sum())} bytes differ"


def assert_same_run(r, ref, packs=None):
    """Outputs, per-step counts and codes, aggregate stats: r == ref bit for bit."""
    sel = slice(None) if packs is None else packs
    for k in ("x", "z", "y"):
        same_bits(getattr(r, k)[sel], getattr(ref, k)[sel], k)
    for k in ("xs", "us", "it", "cd"):
        same_bits(getattr(r, k)[:, sel], getattr(ref, k)[:, sel], k)
    if packs is None:
        for k in STAT_KEYS:
            assert r.st[k] == ref.st[k], k
        assert np.array_equal(r.st["tol_floor"], ref.st["tol_floor"], equal_nan=True), "tol_floor"


def assert_matches_oracle(r, orc, packs=None):
    sel = slice(None) if packs is None else packs
    for k in ("x", "z", "y"):
        same_bits(getattr(r, k)[sel], getattr(orc, k)[sel], "oracle " + k)
    for k in ("xs", "us", "it"):
        same_bits(getattr(r, k)[:, sel], getattr(orc, k)[:, sel], "oracle " + k)


def check_async(oracle, key, p, X0, steps, N, tol, warm, grid):
    orc = oracle_loop(oracle, key, p, X0, steps, N, tol, warm)
    ref = lockstep(key, p, X0, steps, N, tol, warm)
    r = run(p, X0, steps, N, tol, warm, async_=True, grid=grid)
    assert r.st["kernel"] == "loop"
    assert_same_run(r, ref)
    assert_matches_oracle(r, orc)
    assert r.st["total_iterations"] == int(orc.it.sum())
    return r, orc


# ------------------------------------------------------------------------------ CPU
def test_option_and_kernel_numbers_match_the_header():
    """_lib's loop_async option and the kernel names agree with include/gpad.h."""
    from gpad_mpc import _lib
    hdr = open(os.path.join(ROOT, "include", "gpad.h")).read()
    opt = dict(re.findall(r"#define GPAD_OPT_(\w+) +\(?(-?\d+)\)?", hdr))
    ker = {k: int(v) for k, v in re.findall(r"#define GPAD_KERNEL_(\w+) +(\d+)", hdr)}
    assert int(opt["LOOP_ASYNC"]) == 22 == _lib.OPTIONS["loop_async"] == _lib.OPT_LOOP_ASYNC
    assert ker["LOOP"] == 6 == _lib.KERNEL_LOOP
    assert {v: k.lower() for k, v in ker.items()} == _lib.KERNEL_NAMES


# ------------------------------------------------------------------------------ GPU
# plant -> (batch, seed, steps, N with a tolerance)
PLANTS = {(3, 4): (7, 7, 6, 2000), (4, 10): (5, 5, 4, 3000)}


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [0, 2], ids=["solo", "grid2"])
@pytest.mark.parametrize("tol", [0.0, 1e-4])
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("plant", sorted(PLANTS), ids=["b3x4", "b4x10"])
def test_bit_identity(gpu, oracle, plant, warm, tol, grid):
    """Async == lockstep == oracle.  The default grid runs every pack solo; a grid of 2 workgroups
    gives static pairs, queue claims, an odd tail and the pair -> solo switch.  With a tolerance the
    packs must really be ragged: some step with >= 3 distinct counts, unequal totals."""
    batch, seed, steps, Ntol = PLANTS[plant]
    p = battery(*plant)
    N = Ntol if tol else 100
    r, orc = check_async(oracle, plant, p, states(p, batch, seed), steps, N, tol, warm, grid)
    if tol:
        assert max(len(set(row)) for row in orc.it.tolist()) >= 3
        assert len(set(orc.it.sum(axis=0).tolist())) > 1
        assert orc.it.max() < N
        if warm:  # (csrc/gpad_chain.h names this case: test (B) at step 0, a verified (A) on the warm steps;
            # the oracle's loop returns no codes, the run's are bit-identical to the lockstep loop's)
            assert {1, 2} <= set(r.cd.ravel().tolist())
    else:
        assert (r.it == N).all() and (r.cd == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("plant", sorted(PLANTS), ids=["b3x4", "b4x10"])
def test_batch_of_one(gpu, oracle, plant):
    batch, seed, steps, N = PLANTS[plant]
    p = battery(*plant)
    check_async(oracle, plant, p, states(p, batch, seed)[:1], steps, N, 1e-4, False, 0)


@pytest.mark.gpu
def test_iteration_cap_inside_a_step(gpu, oracle):
    """N = 60: some solves stop at the cap and some earlier, inside one run."""
    p = battery(3, 4)
    r, orc = check_async(oracle, (3, 4), p, states(p, 7, 7), 6, 60, 1e-4, False, 2)
    assert (orc.it == 60).any() and (orc.it < 60).any()
    np.testing.assert_array_equal(r.cd > 0, r.it < 60)


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_two_ml_waves_m0_bound(gpu, oracle, warm):
    """n = 70 (two -ML waves), m = 130, M0 and g0 bound, nx = 5 != nu = 2."""
    p = synthetic(70, 130, 5, 2)
    r, orc = check_async(oracle, "s70", p, p.X0, 5, 1500, 1e-4, warm, 2)
    assert np.isfinite(orc.xs).all() and np.isfinite(orc.z).all() and orc.it.max() < 1500


@pytest.mark.gpu
def test_nx_at_the_bound(gpu, oracle):
    """nx = 64 (the whole LDS state row), nu = 1."""
    p = synthetic(70, 130, 64, 1)
    orc = oracle_loop(oracle, "s70x64", p, p.X0, 5, 1500, 1e-4, False)
    assert all(np.isfinite(getattr(orc, k)).all() for k in ("x", "z", "y", "xs", "us"))
    check_async(oracle, "s70x64", p, p.X0, 5, 1500, 1e-4, False, 2)


@pytest.mark.gpu
def test_nx_past_the_bound_runs_lockstep(gpu):
    p = synthetic(70, 130, 65, 1)
    ref = lockstep("s70x65", p, p.X0, 3, 200, 1e-4, False)
    r = run(p, p.X0, 3, 200, 1e-4, False, async_=True, grid=2)
    assert r.st["kernel"] not in (None, "loop")
    assert_same_run(r, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["f64", "panel", "n300"])
def test_fallbacks(gpu, case):
    """Where the kernel does not apply the option is accepted and the lockstep loop runs."""
    from gpad_mpc import _lib
    if case == "n300":
        p = synthetic(300, 64, 3, 2, packs=2)
        X0, kw = p.X0, {}
    else:
        p = battery(3, 4)
        X0 = states(p, 7, 7)
        kw = dict(dtype=np.float64) if case == "f64" else dict(kernel=_lib.KERNEL_PANEL)
    ref = run(p, X0, 2, 50, 0.0, False, **kw)
    r = run(p, X0, 2, 50, 0.0, False, async_=True, **kw)
    assert r.st["kernel"] == ref.st["kernel"] != "loop"
    assert_same_run(r, ref)


@pytest.mark.gpu
def test_option_range(gpu):
    from gpad_mpc._lib import GpadError
    s = make_solver(battery(3, 4), 1)
    with pytest.raises(GpadError):
        s.set_option("loop_async", 2)
    s.set_option("loop_async", 1)
    s.set_option("loop_async", -1)  # back to the default: lockstep
    p = battery(3, 4)
    assert loop(s, p, states(p, 1, 7), 2, 20, 0.0, False).st["kernel"] != "loop"


@pytest.mark.gpu
def test_nonfinite_state(gpu, oracle):
    """An infinite state poisons its own pack only: N bounded iterations of NaN arithmetic per step,
    the run flagged NONFINITE_G in both modes, the other packs untouched."""
    p = battery(3, 4)
    X0 = states(p, 3, 7)
    X0[1, 0] = np.inf
    ref = lockstep((3, 4), p, X0, 2, 60, 1e-4, False)
    r = run(p, X0, 2, 60, 1e-4, False, async_=True)
    assert r.st["kernel"] == "loop"
    assert r.st["nonfinite_g"] and ref.st["nonfinite_g"]
    assert r.st["below_tol_floor"] == ref.st["below_tol_floor"]
    assert np.array_equal(r.st["tol_floor"], ref.st["tol_floor"], equal_nan=True)
    same_bits(r.it, ref.it, "it")
    same_bits(r.cd, ref.cd, "cd")
    assert_same_run(r, ref, packs=[0, 2])
    Xf = X0.copy()
    Xf[1] = 0.0
    assert_matches_oracle(r, oracle_loop(oracle, (3, 4), p, Xf, 2, 60, 1e-4, False), packs=[0, 2])


@pytest.mark.gpu
def test_device_tensors_without_stats(gpu):
    """Device memory, stats=False: the loop is only enqueued; sync, then compare with lockstep."""
    import torch
    import gpad_mpc
    p = battery(3, 4)
    qp = p.qp
    batch, steps, N = 7, 6, 2000
    t = lambda a: torch.from_numpy(F32(a)).to(gpu)  # noqa: E731
    X0 = states(p, batch, 7)
    out = []
    for async_ in (False, True):
        s = gpad_mpc.GpadSolver(0)
        s.setup(t(qp.ML), t(qp.G), float(np.float32(qp.L)), n=qp.n, m=qp.m, batch=batch)
        s.setup_plant(t(p.PM), t(p.Pg), g0=t(p.g0), A=t(p.A), B=t(p.B))
        if async_:
            s.set_options(loop_async=1, duo_max_grid=2)
        X = torch.from_numpy(X0).to(gpu)
        Z = torch.zeros(batch, qp.n, device=gpu)
        Y = torch.zeros(batch, qp.m, device=gpu)
        XS = torch.zeros(steps, batch, p.nx, device=gpu)
        US = torch.zeros(steps, batch, p.nu, device=gpu)
        assert s.closed_loop(X, Z, Y, steps, N, 1e-4, xs=XS, us=US, stats=False) is None
        s.sync()
        st = s.last_stats()
        assert (st["kernel"] == "loop") == async_
        out.append(([a.cpu().numpy() for a in (X, Z, Y, XS, US)], st))
    for a, b, k in zip(out[0][0], out[1][0], "x z y xs us".split()):
        same_bits(b, a, k)
    for k in STAT_KEYS + ("tol_floor",):
        assert out[0][1][k] == out[1][1][k], k


@pytest.mark.gpu
def test_handle_reuse(gpu):
    """Async twice, the option off, async again on one handle: four identical results (the queue
    counter and the status words are reset per run)."""
    p = battery(3, 4)
    X0 = states(p, 7, 7)
    s = make_solver(p, 7)
    s.set_options(loop_async=1, duo_max_grid=2)
    runs = [loop(s, p, X0, 6, 2000, 1e-4, False) for _ in range(2)]
    s.set_option("loop_async", 0)
    runs.append(loop(s, p, X0, 6, 2000, 1e-4, False))
    s.set_option("loop_async", 1)
    runs.append(loop(s, p, X0, 6, 2000, 1e-4, False))
    assert [r.st["kernel"] == "loop" for r in runs] == [True, True, False, True]
    for r in runs[1:]:
        assert_same_run(r, runs[0])
