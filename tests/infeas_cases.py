"""Inputs of the infeasibility tests (tests/test_infeasible_cpu.py, tests/test_infeasible.py).  TEST
INFRASTRUCTURE ONLY.

Packs of ``problems.battery_plant_signals`` under a 5 A load.  A draw puts every cell's state of charge
inside the box; an ``edge`` draw moves one cell to within 0.05 of a bound and points the load outward, so
that the horizon cannot keep xmin <= x <= xmax with |u| <= 0.3: the QP is infeasible.  The other draws keep
every cell at least 0.25 away from the bound the load pushes to, which the horizon cannot reach (a step
under load moves a cell by 0.0126), so they are feasible.  R = 0.3 = problems.battery_zbound().

The wide inputs of tests/test_infeasible_panels.py (slab_*) are synthetic QPs of any shape in which two rows of G
are opposite: their right-hand sides make a slab around a witness or contradict each other (R = SLAB_R).
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


# ------------------------------------------------- wide mixed batches (tests/test_infeasible_panels.py)
SLAB_R = 10.0  # |zf|_inf <= 0.5, and the feasible instances' solutions stay below it (asserted on the CPU)


def slab_rows(m):
    """Row i in row tile 0 and row j in the last row tile of G."""
    return (min(3, m - 3), m - 2 if (m - 2) // 16 == (m - 1) // 16 else m - 1)


@functools.lru_cache(maxsize=None)
def slab_qp(n, m, seed, rows=None):
    """problems.synthetic_qp(n, m, seed=seed) with G[j] = -G[i]; ML and L recomputed from the new G."""
    i, j = rows or slab_rows(m)
    qp = problems.synthetic_qp(n, m, seed=seed)
    G = qp.G.copy()
    G[j] = -G[i]
    ML = np.linalg.inv(qp.H) @ G.T
    return problems.QP(ML=ML, M=None, G=G, g=None, L=float(np.linalg.norm(G @ ML, "fro")), H=qp.H)


@functools.lru_cache(maxsize=None)
def slab_batch(n, m, batch, seed, rows=None, bad=None):
    """A mixed batch with a known answer on the matrices of slab_qp: rows i and j of G are opposite, so the two
    of them bound G[i] z from both sides.  Every instance draws zf ~ U(-0.5, 0.5)^n, q ~ N(0, 1)^n and
    g = G zf + U(0.1, 1).  A feasible instance's row j is -G[i] zf + U(0.1, 1): a slab of positive width with the
    witness zf inside the box.  An infeasible one's (``bad``: a tuple of instances, default every second) is
    g[j] = -g[i] - 1: no z meets both rows, and y = e_i + e_j certifies it for any R.  Returns the QP (ML, G, L
    shared), zf [batch][n], the infeasible mask, M = inv(H) q [batch][n] and g [batch][m], all fp64."""
    i, j = rows or slab_rows(m)
    qp = slab_qp(n, m, seed, (i, j))
    mask = np.zeros(batch, bool)
    mask[list(range(1, batch, 2)) if bad is None else list(bad)] = True
    Hinv = np.linalg.inv(qp.H)
    zf, M, g = np.empty((batch, n)), np.empty((batch, n)), np.empty((batch, m))
    for k in range(batch):  # a generator per instance: a smaller batch is a prefix of a larger one
        rng = np.random.default_rng([seed, n, m, k])
        zf[k], M[k] = rng.uniform(-0.5, 0.5, n), Hinv @ rng.normal(0.0, 1.0, n)
        g[k] = qp.G @ zf[k] + rng.uniform(0.1, 1.0, m)  # (row j: G[j] zf = -G[i] zf)
    g[mask, j] = -g[mask, i] - 1.0
    return SimpleNamespace(qp=qp, n=n, m=m, rows=(i, j), zf=zf, bad=mask, M=M, g=g)


@functools.lru_cache(maxsize=None)
def slab_plant(n=70, m=130, nx=5, nu=2, rows=None, packs=16):
    """test_loop_async.synthetic(n, m, nx, nu) with rows i, j opposite in the matrices and the maps (G[j] = -G[i],
    Pg[j] = -Pg[i], g0[j] = -g0[i]; ML and L recomputed from the new G) and one signal on row j (ns = 1,
    Sg[j, 0] = 1, no other signal map), so that g_i(x, s) + g_j(x, s) = s at every state: a positive s is the
    width of a slab, s = -1 leaves no z for the two rows, and y = e_i + e_j certifies that for any R."""
    import test_loop_async as tla
    i, j = rows or slab_rows(m)
    p = tla.synthetic(n, m, nx, nu, packs=packs)
    qp = p.qp
    G, Pg, g0 = qp.G.copy(), p.Pg.copy(), np.array(p.g0, np.float64).reshape(m)
    G[j], Pg[j], g0[j] = -G[i], -Pg[i], -g0[i]
    Sg = np.zeros((m, 1))
    Sg[j, 0] = 1.0
    ML = np.linalg.inv(qp.H) @ G.T
    nq = problems.QP(ML=ML, M=None, G=G, g=None, L=float(np.linalg.norm(G @ ML, "fro")), H=qp.H)
    return SimpleNamespace(qp=nq, n=n, m=m, rows=(i, j), PM=p.PM, Pg=Pg, M0=np.array(p.M0, np.float64).reshape(n),
                           g0=g0, Sg=Sg, A=p.A, B=p.B, nx=nx, nu=nu, ns=1, X0=p.X0)


SLAB_BAD = {3: (2, 5), 10: (3, 5), 6: (0, 1)}  # pack: the steps [from, to) at which its signal is -1


def slab_loop_inputs(width, batch_size=16, steps=5):
    """The script of the slab plant's closed loop: S[t, b, 0] = width, a slab every pack can stay in, except
    S = -1 where SLAB_BAD says so: packs 3 and 10 turn infeasible at steps 2 and 3 and stay so, pack 6 is
    infeasible at step 0 only.  S [steps][batch][1], want [steps][batch]: the solves that must end 5."""
    S = np.full((steps, batch_size, 1), float(width))
    want = np.zeros((steps, batch_size), bool)
    for b, (t0, t1) in SLAB_BAD.items():
        if b < batch_size:
            want[t0:t1, b] = True
    S[want, 0] = -1.0
    return SimpleNamespace(S=S, want=want, steps=steps, batch=batch_size)


def slab_loop_reference(pl, L, X0, S, N=N, tol=TOL, R=SLAB_R, warm=False):
    """The fp64 reference closed loop of every pack: loop_ref64's plant arithmetic around infeas_ref64.solve.
    ``pl``: one slab_plant, or a list with every pack's own (a class fleet).
    -> x, z, y [batch][.], xs, us [steps][batch][.], it, cd, nominated [steps][batch]."""
    import loop_ref64 as lr
    steps, batch = S.shape[:2]
    plants = list(pl) if isinstance(pl, (list, tuple)) else [pl] * batch
    pl = plants[0]
    out = SimpleNamespace(x=np.zeros((batch, pl.nx)), z=np.zeros((batch, pl.n)), y=np.zeros((batch, pl.m)),
                          xs=np.zeros((steps, batch, pl.nx)), us=np.zeros((steps, batch, pl.nu)),
                          it=np.zeros((steps, batch), np.int32), cd=np.zeros((steps, batch), np.int32),
                          nominated=np.zeros((steps, batch), np.int32))
    for b in range(batch):
        pl = plants[b]
        x, z, y = np.asarray(X0[b], np.float64), None, None
        for t in range(steps):
            s = np.asarray(S[t, b], np.float64)
            M = lr.affine(pl.PM, pl.M0, x, None, s)
            g = lr.affine(pl.Pg, pl.g0, x, pl.Sg, s)
            r = ref.solve(pl.qp.ML, M, pl.qp.G, g, L, N, tol, R, np.float64, z0=z if warm else None,
                          y0=y if warm else None)
            z, y = r.z, r.y
            out.xs[t, b], out.us[t, b] = x, z[:pl.nu]
            out.it[t, b], out.cd[t, b], out.nominated[t, b] = r.it, r.code, r.nominated
            x = lr.plant_step(pl.A, pl.B, x, z[:pl.nu], None, s)
        out.x[b], out.z[b], out.y[b] = x, z, y
    return out


@functools.lru_cache(maxsize=None)
def slab_reference(n, m, batch, seed, dtype=np.float64):
    """infeas_ref64.solve of every instance of slab_batch(n, m, batch, seed) with R = SLAB_R (computed once, shared
    by the tests, never modified)."""
    b = slab_batch(n, m, batch, seed)
    return [ref.solve(b.qp.ML, b.M[k], b.qp.G, b.g[k], b.qp.L, N, TOL, SLAB_R, dtype) for k in range(batch)]
