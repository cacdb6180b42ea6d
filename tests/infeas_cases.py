"""Inputs of the infeasibility tests (tests/test_infeasible_cpu.py, tests/test_infeasible.py).  TEST
INFRASTRUCTURE ONLY.

Packs of ``problems.battery_plant_signals`` under a 5 A load.  A draw puts every cell's state of charge
inside the box; an ``edge`` draw moves one cell to within 0.05 of a bound and points the load outward, so
that the horizon cannot keep xmin <= x <= xmax with |u| <= 0.3: the QP is infeasible.  The other draws keep
every cell at least 0.25 away from the bound the load pushes to, which the horizon cannot reach (a step
under load moves a cell by 0.0126), so they are feasible.  R = 0.3 = problems.battery_zbound().
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import infeas_ref64 as ref
from gpad_mpc import problems

R, N, TOL, LOAD = 0.3, 3000, 1e-4, 5.0
BATCH = 33  # the largest batch of the GPU tests; the smaller ones take its first instances
SHAPES = {"1x2": (1, 2), "2x4": (2, 4), "4x10": (4, 10)}
SEEDS = {"1x2": 11, "2x4": 14, "4x10": 13}


@functools.lru_cache(maxsize=None)
def pack(shape):
    n_u, Nh = SHAPES[shape]
    qp, pl = problems.battery_plant_signals(n_u, Nh)
    return SimpleNamespace(n_u=n_u, Nh=Nh, qp=qp, pl=pl, n=qp.n, m=qp.m, ns=1 + n_u)


def draw(shape, rng, edge):
    """(x0, s) of one instance: s = [i_load, r_1 .. r_nu]."""
    n_u = SHAPES[shape][0]
    up = rng.random() < 0.5                       # the load pushes towards xmax (i_load < 0) or xmin
    x = rng.uniform(-0.2, 0.2, n_u)
    if edge:
        d = rng.uniform(0.0, 0.05)
        x[rng.integers(n_u)] = 0.5 - d if up else -0.5 + d
    s = np.concatenate([[-LOAD if up else LOAD], rng.uniform(-0.1, 0.1, n_u)])
    return x, s


def qp_data(shape, x, s):
    """M(x, s), g(x, s) in fp64 (the affine maps of gpad_setup_signals)."""
    pl = pack(shape).pl
    return pl.PM @ x + pl.SM @ s, pl.g0 + pl.Pg @ x + pl.Sg @ s


@functools.lru_cache(maxsize=None)
def batch(shape, count, edge_every, seed=None):
    """``count`` instances, every ``edge_every``-th an edge draw: X [count][nu], S [count][ns], M, g and the
    mask of the edge draws."""
    rng = np.random.default_rng(SEEDS[shape] if seed is None else seed)
    edge = np.array([b % edge_every == edge_every - 1 for b in range(count)])
    xs = [draw(shape, rng, e) for e in edge]
    X, S = np.stack([x for x, _ in xs]), np.stack([s for _, s in xs])
    Mg = [qp_data(shape, x, s) for x, s in xs]
    return SimpleNamespace(X=X, S=S, M=np.stack([a for a, _ in Mg]), g=np.stack([b for _, b in Mg]), edge=edge)


@functools.lru_cache(maxsize=None)
def reference(shape, dtype=np.float64, bound=True):
    """infeas_ref64.solve of every instance of batch(shape, BATCH, 2), from z = y = 0 (computed once, shared by
    the tests, never modified)."""
    p, b = pack(shape), batch(shape, BATCH, 2)
    return [ref.solve(p.qp.ML, b.M[i], p.qp.G, b.g[i], p.qp.L, N, TOL, R if bound else 0.0, dtype) for i in range(BATCH)]


@functools.lru_cache(maxsize=None)
def loop_inputs(batch_size=16, steps=6):
    """A closed loop of 4x10 packs under small loads, two of which get the 5 A load switched on at steps 3 and 2
    while a cell sits 0.06 / 0.05 from the bound it pushes to: feasible before, infeasible from then on (far
    enough inside for the certificate to pass within a few hundred iterations).  X0 [batch][nu],
    S [steps][batch][ns], bad = {pack: first infeasible step}."""
    rng = np.random.default_rng(5)
    X = rng.uniform(-0.2, 0.2, (batch_size, 4))
    S = np.zeros((steps, batch_size, 5))
    S[:, :, 0] = rng.uniform(-0.5, 0.5, batch_size)[None, :]
    S[:, :, 1:] = rng.uniform(-0.1, 0.1, (batch_size, 4))[None]
    bad = {3: 3, 10: 2}
    for b, off, sg in ((3, 0.06, 1.0), (10, 0.05, -1.0)):
        X[b, 1] = sg * (-0.5 + off)
        S[:, b, 0] = 0.0
        S[bad[b]:, b, 0] = sg * LOAD
    return SimpleNamespace(X0=X, S=S, bad=bad, steps=steps, batch=batch_size)
