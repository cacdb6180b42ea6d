"""The certification floor and the run flags (include/gpad.h gpad_stats_t: tol_floor,
GPAD_FLAG_TOL_FLOOR, GPAD_FLAG_NONFINITE_G) on every engine and entry point.

Reference: plain fp64 numpy, floor = margin * max |g| over the run's whole g (margin 2^-20 for f32,
2^-49 for f64; margin * L * max |p_D| for scaled runs).

Planted maximum: one entry of a finite problem's g is overwritten with -4 max |g| (negative on
purpose), one run per planted position.  A reduction that drops that lane, row, panel or workgroup
then reports a floor 4x too small, and a tol of half the true floor is no longer flagged -- while no
solve result changes.  The positions are the corners of the batch, the first column of the second
16-instance panel, the last instance of the last full panel and the rows on each side of the last
16-row tile boundary.

gpad_run / gpad_run_scaled scale the maximum by margin * L * (1/L), which is not exactly margin:
rel = 1e-6 (as tests/test_errors.py).  gpad_run_state / gpad_closed_loop scale by margin itself, a
power of two: their floor must be exactly equal.

Non-finite g: an instance with a NaN / infinity in g must flag the run, give a NaN / inf floor, not
converge -- and leave every other instance of its 16-column MFMA panel bit-equal to the oracle.
"""
from __future__ import annotations

import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MARGIN = {np.float32: 2.0 ** -20, np.float64: 2.0 ** -49}
F32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))  # noqa: E731
F64 = lambda a: np.ascontiguousarray(a, np.float64)  # noqa: E731


def _qp(n, m, B, dtype=np.float32, shared=True):
    """(ML, M [B][n], G, g [B][m], L) of problems.synthetic_qp, g of order 0.1 .. 2."""
    from gpad_mpc import problems
    qp = problems.synthetic_qp(n, m, batch=B, seed=n + m + B)
    c = F32 if dtype == np.float32 else F64
    ML, G = c(qp.ML), c(qp.G)
    if not shared:
        rng = np.random.default_rng(B)
        ML = c(ML[None] * (1 + 0.02 * rng.random((B, 1, 1))))
        G = c(G[None] * (1 + 0.02 * rng.random((B, 1, 1))))
    L = float(np.float32(qp.L)) if dtype == np.float32 else float(qp.L)
    return ML, c(qp.M).reshape(B, n), G, c(qp.g).reshape(B, m), L


def _positions(B, m):
    r = 16 * ((m - 1) // 16)  # first row of the last 16-row tile
    full = 16 * (B // 16) - 1  # last instance of the last full panel
    cand = [(0, 0), (0, m - 1), (B - 1, 0), (B - 1, m - 1), (16, m - 1), (full, m // 2), (B // 2, r - 1),
            (B // 2, r)]
    out = []
    for b, i in cand:
        if 0 <= b < B and 0 <= i < m and (b, i) not in out:
            out.append((b, i))
    return out


def _plant(g, b, i):
    """g with entry (b, i) = -4 max |g|, and the fp64 max |.| of the result."""
    gp = g.copy()
    gp[b, i] = -4 * np.abs(g).max()
    return gp, float(np.abs(gp.astype(np.float64)).max())


def _check(st, floor, tol, kernel, exact, what):
    if exact:
        assert st["tol_floor"] == floor, (what, st["tol_floor"], floor)
    else:
        assert st["tol_floor"] == pytest.approx(floor, rel=1e-6), (what, st["tol_floor"], floor)
    assert st["below_tol_floor"] is (tol < floor), (what, tol, floor, st)
    assert not st["nonfinite_g"], (what, st)
    assert st["kernel"] == kernel, (what, st)


def _sweep(s, M, g, *, kernel, N=20, scaled=False, L=None, run=None, positions=None):
    """One run per planted position and tol side on the solver `s`; every run and the last_stats()
    right after it must report the planted floor and the flags."""
    B, m = g.shape
    margin = MARGIN[g.dtype.type]

    def host_run(gp, tol):
        z = np.zeros_like(M)
        y = np.zeros_like(g)
        return s.run(z, y, M, gp, N, tol, scaled=scaled)

    run = run or host_run
    for b, i in positions or _positions(B, m):
        gp, gmax = _plant(g, b, i)
        floor = margin * L * gmax if scaled else margin * gmax
        assert floor < 1e-4
        for tol in (1e-4, 0.5 * floor):
            st = run(gp, tol)
            _check(st, floor, tol, kernel, False, (b, i, tol))
            _check(s.last_stats(), floor, tol, kernel, False, ("last_stats", b, i, tol))


def _solver(ML, G, L, M, g, kernel=0, shared=True, **opts):
    import gpad_mpc
    s = gpad_mpc.GpadSolver(0)
    s.setup(ML, G, L, n=M.shape[1], m=g.shape[1], batch=g.shape[0], shared=shared, kernel=kernel)
    s.set_options(**opts)
    return s


# ------------------------------------------------------------------ gpad_run, every engine
@pytest.mark.parametrize("n,m,B", [(40, 64, 5), (208, 180, 3)])
def test_floor_resident(gpu, n, m, B):
    """The resident kernel, then absmax_kernel over g."""
    ML, M, G, g, L = _qp(n, m, B)
    with _solver(ML, G, L, M, g) as s:
        _sweep(s, M, g, kernel="resident")


@pytest.mark.parametrize("n,m,B,shared,kernel", [(37, 53, 3, True, 1), (37, 53, 3, False, 1), (300, 260, 2, True, 0)])
def test_floor_stream(gpu, n, m, B, shared, kernel):
    """The stream kernel: forced (shared and per-instance matrices), and chosen (past the resident
    kernel's 208 rows at a batch below the panels')."""
    ML, M, G, g, L = _qp(n, m, B, shared=shared)
    with _solver(ML, G, L, M, g, kernel=kernel, shared=shared) as s:
        _sweep(s, M, g, kernel="stream")


@pytest.mark.parametrize("n,m,B", [(37, 53, 40), (128, 100, 40), (40, 257, 20)])
def test_floor_small_and_big_panels(gpu, n, m, B):
    """T <= 8 panels and the big panels (max(n, m) just above 256: 17 tiles) leave the maximum to
    absmax_kernel."""
    from gpad_mpc import _lib
    ML, M, G, g, L = _qp(n, m, B)
    with _solver(ML, G, L, M, g, kernel=_lib.KERNEL_PANEL) as s:
        _sweep(s, M, g, kernel="panel")


# (n, m): T = 9; T = 13 KQ = 2; T = 13 KQ = 4; scalar rows4 I/O (n, m not multiples of 4), twice;
# tiles past the last row (n << m, m << n); T = 16
FOLDED = [(144, 129), (200, 200), (208, 208), (199, 201), (193, 201), (8, 196), (200, 8), (256, 250)]
# (B, panel_max_grid): one panel per workgroup (3 panels, default grid); 3 panels on one workgroup
# (pairs, two items walked grid-stride, the last a lone ragged panel); 5 panels on two workgroups
# (workgroup 0 takes items 0 and 2)
LAYOUTS = [(40, 0), (40, 1), (72, 2)]


@pytest.mark.parametrize("B,grid", LAYOUTS)
@pytest.mark.parametrize("n,m", FOLDED)
def test_floor_folded_panels(gpu, n, m, B, grid):
    """The panel pairs (T = 9 .. 16) fold max |g| into their own operand loads."""
    from gpad_mpc import _lib
    ML, M, G, g, L = _qp(n, m, B)
    with _solver(ML, G, L, M, g, kernel=_lib.KERNEL_PANEL) as s:
        if grid:
            s.set_option("panel_max_grid", grid)
        _sweep(s, M, g, kernel="panel")


def test_floor_folded_panels_scaled(gpu, oracle):
    """gpad_setup_scaled + gpad_run_scaled: floor = margin * L * max |p_D|."""
    import gpad_mpc
    from gpad_mpc import _lib
    n = m = 200
    B = 40
    ML, M, G, g, L = _qp(n, m, B)
    MGneg, GL, _ = oracle.scale(ML, G, g[0], np.float32(L))
    pD = np.ascontiguousarray(oracle.scale_vec(g, np.float32(L)))
    with gpad_mpc.GpadSolver(0) as s:
        s.setup(MGneg, GL, L, n=n, m=m, batch=B, kernel=_lib.KERNEL_PANEL, scaled=True)
        _sweep(s, M, pD, kernel="panel", scaled=True, L=L)


def test_floor_folded_panels_phased(gpu):
    """A phased solve: only the first launch stores the per-workgroup maxima, the later phases max
    in.  The planted instance converges in phase 0 (its M = 0 and a tol its planted row meets at the
    first test), the others (M scaled up) survive into the later phases, which therefore load their
    g but never the planted one: a later phase that stored would lose the planted maximum."""
    from gpad_mpc import _lib
    n = m = 200
    B, N = 40, 100
    ML, M, G, g, L = _qp(n, m, B)
    M = (M * np.float32(1000.0)).astype(np.float32)
    margin = MARGIN[np.float32]
    with _solver(ML, G, L, M, g, kernel=_lib.KERNEL_PANEL, panel_max_grid=1) as s:
        for b, i in [(3, 7), (17, m - 1), (B - 2, 100)]:
            Mb = M.copy()
            Mb[b] = 0.0
            gp, gmax = _plant(g, b, i)
            floor = margin * gmax
            tol = 2.0 * gmax  # the first test passes near z = 0: L * viol ~ the planted 4 max |g| <= tol
            it = np.zeros(B, np.int32)
            st = s.run(np.zeros_like(M), np.zeros_like(g), Mb, gp, N, tol, iters=it)
            ph = s.last_phases()
            assert len(ph["ends"]) >= 2, ph
            assert it[b] <= ph["ends"][0] < it.max(), (b, it[b], it.max(), ph)
            _check(st, floor, tol, "panel", False, (b, i))
            _check(s.last_stats(), floor, tol, "panel", False, ("last_stats", b, i))


def test_floor_without_iterations(gpu):
    """N = 0 with a tolerance: nothing is launched but the floor is still reported (absmax path)."""
    from gpad_mpc import _lib
    ML, M, G, g, L = _qp(200, 200, 40)
    with _solver(ML, G, L, M, g, kernel=_lib.KERNEL_PANEL) as s:
        _sweep(s, M, g, kernel="panel", N=0)


@pytest.mark.parametrize("engine", ["lds", "resident", "panels"])
def test_floor_flat(gpu, oracle, engine):
    """The flat battery path (scaled data): the LDS flat kernel, the register-resident flat chains
    and the flat panels (tol > 0: phased, the solve runs past its first phase)."""
    import gpad_mpc
    from gpad_mpc import _lib, problems
    n_u, Nh = 4, 10
    B = 40 if engine == "panels" else 5
    qp = problems.battery_scenarios(n_u, Nh, B, seed=4)
    MGf, GLf, L = problems.flatten_battery(qp, n_u, Nh)
    L32 = np.float32(L)
    GP = F32(qp.M)
    PD = np.ascontiguousarray(oracle.scale_vec(F32(qp.g), L32))
    kernel = {"lds": _lib.KERNEL_STREAM, "resident": _lib.KERNEL_AUTO, "panels": _lib.KERNEL_PANEL}[engine]
    with gpad_mpc.GpadSolver(0) as s:
        s.setup_flat(F32(MGf), F32(GLf), float(L32), n_u=n_u, batch=B, kernel=kernel)
        if engine == "panels":
            s.set_option("phased", 2)
        _sweep(s, GP, PD, kernel="flat", scaled=True, L=float(L32), N=60 if engine == "panels" else 20)


@pytest.mark.parametrize("n,m,B,kernel,name", [(40, 64, 3, 1, "stream"), (40, 64, 20, 3, "panel"),
                                               (200, 200, 20, 3, "panel")])
def test_floor_f64(gpu, n, m, B, kernel, name):
    """f64: the stream kernel and the f64 panels, margin 2^-49."""
    ML, M, G, g, L = _qp(n, m, B, dtype=np.float64)
    with _solver(ML, G, L, M, g, kernel=kernel) as s:
        _sweep(s, M, g, kernel=name)


@pytest.mark.parametrize("n,m,B,kernel,name", [(40, 64, 5, 0, "resident"), (200, 200, 40, 3, "panel")])
def test_floor_async_run(gpu, n, m, B, kernel, name):
    """Device tensors without a stats struct (asynchronous), gpad_sync, then gpad_last_stats."""
    import torch
    ML, M, G, g, L = _qp(n, m, B)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    dM = t(M)
    with _solver(t(ML), t(G), L, M, g, kernel=kernel) as s:
        def run(gp, tol):
            z = torch.zeros(B, n, device=gpu)
            y = torch.zeros(B, m, device=gpu)
            assert s.run(z, y, dM, t(gp), 20, tol, stats=False) is None
            s.sync()
            return s.last_stats()

        _sweep(s, M, g, kernel=name, run=run, positions=_positions(B, m)[:5])


# ------------------------------------------------------------------ gpad_run_state
def _plant_solver(qp, pl, batch, kernel=0, dtype=np.float32, dyn=True):
    import gpad_mpc
    c = F32 if dtype == np.float32 else F64
    L = float(np.float32(qp.L)) if dtype == np.float32 else float(qp.L)
    s = gpad_mpc.GpadSolver(0)
    s.setup(c(qp.ML), c(qp.G), L, n=qp.n, m=qp.m, batch=batch, kernel=kernel)
    s.setup_plant(c(pl.PM), c(pl.Pg), g0=c(pl.g0), A=c(pl.A) if dyn else None, B=c(pl.B) if dyn else None)
    return s


@pytest.mark.parametrize("batch", [5, 96])
def test_floor_run_state(gpu, oracle, batch):
    """gpad_run_state: g(x) = g0 + Pg x formed on the device; one pack's state is pushed out so that
    its g(x) holds the maximum.  floor_scale is margin itself: exact equality."""
    from gpad_mpc import problems
    qp, pl = problems.battery_plant(4, 10)
    margin = MARGIN[np.float32]
    X0 = np.random.default_rng(3).uniform(-0.45, 0.45, (batch, 4)).astype(np.float32)
    with _plant_solver(qp, pl, batch, dyn=False) as s:
        for b, j in [(0, 0), (batch - 1, 3), (16, 1), (batch // 2, 2)]:
            if b >= batch:
                continue
            X = X0.copy()
            X[b, j] = -8.0
            gx = np.stack([oracle.affine(pl.Pg, pl.g0, X[k]) for k in range(batch)]).astype(np.float64)
            assert int(np.argmax(np.abs(gx).max(axis=1))) == b
            floor = margin * float(np.abs(gx).max())
            for tol in (1e-4, 0.5 * floor):
                Z = np.zeros((batch, qp.n), np.float32)
                Y = np.zeros((batch, qp.m), np.float32)
                st = s.run_state(X, Z, Y, 20, tol)
                _check(st, floor, tol, "resident", True, (b, j, tol))
                _check(s.last_stats(), floor, tol, "resident", True, ("last_stats", b, j, tol))


# ------------------------------------------------------------------ gpad_closed_loop
class _Plant:
    """Synthetic plant on synthetic_qp(40, 64): nx = 3, nu = 2; g(x) = (|g| + 1) + Pg x with
    Pg ~ N(0, 1), so max |g(x_t)| follows |x_t|; PM and B are small, so x_t follows A."""

    def __init__(self, A):
        from gpad_mpc import problems
        self.qp = problems.synthetic_qp(40, 64, batch=1, seed=0)
        rng = np.random.default_rng(11)
        self.PM = 0.01 * rng.standard_normal((40, 3))
        self.Pg = rng.standard_normal((64, 3))
        self.g0 = np.abs(self.qp.g) + 1.0
        self.B = 0.01 * rng.standard_normal((3, 2))
        self.A = np.asarray(A, np.float64)


DYNAMICS = {"decay": 0.5 * np.eye(3), "rise": 2.0 * np.eye(3), "mixed": np.diag([0.5, 2.0, 1.0])}
STEPS, CL_N = 5, 30


def _x0(dyn, batch):
    """Initial states of order (40, -30, 20).  mixed: A = diag(0.5, 2, 1) is shared, so the packs start
    along different axes -- pack b along axis b % 3: axis 0 decays (large start, the run's maximum at
    step 0), axis 1 rises (small start, its own maximum at the last step), axis 2 stays."""
    s = 1.0 + 0.01 * np.arange(batch)[:, None]
    if dyn != "mixed":
        return (s * np.array([40.0, -30.0, 20.0])).astype(np.float32)
    amp = np.array([400.0, -2.0, 20.0])
    X = np.zeros((batch, 3))
    for b in range(batch):
        X[b, b % 3] = amp[b % 3] * s[b, 0]
    return X.astype(np.float32)


def _affine_f64(P, c0, x):
    """orc_affine's chain acc = fma(P[i][k], x[k], acc) from c0[i], in fp64 with exact fma."""
    out = np.empty(P.shape[0])
    for i in range(P.shape[0]):
        acc = float(c0[i])
        for k in range(P.shape[1]):
            acc = float(Fraction(float(P[i, k])) * Fraction(float(x[k])) + Fraction(acc))
        out[i] = acc
    return out


def _cl_oracle(oracle, p, X0, tol):
    """Per pack: the oracle's closed loop -> (x, z, y, xs, us, iters)."""
    L = np.float32(p.qp.L)
    MGneg, GL, _ = oracle.scale(F32(p.qp.ML), F32(p.qp.G), F32(p.qp.g), L)
    return [oracle.closed_loop_f32(X0[b], MGneg, GL, L, p.PM, p.Pg, p.A, p.B, STEPS, CL_N, tol, g0=p.g0)
            for b in range(X0.shape[0])]


def _step_maxima_f32(oracle, p, ref):
    """max |g(x_t)| over the packs and rows, per step, from the oracle's trajectories."""
    return np.array([max(float(np.abs(oracle.affine(p.Pg, p.g0, r[3][t]).astype(np.float64)).max()) for r in ref)
                     for t in range(STEPS)])


def _cl_run(s, p, X0, tol, dtype=np.float32):
    batch = X0.shape[0]
    out = dict(X=X0.astype(dtype), Z=np.zeros((batch, 40), dtype), Y=np.zeros((batch, 64), dtype),
               XS=np.zeros((STEPS, batch, 3), dtype), US=np.zeros((STEPS, batch, 2), dtype),
               IT=np.zeros(STEPS * batch, np.int32))
    out["st"] = s.closed_loop(out["X"], out["Z"], out["Y"], STEPS, CL_N, tol, xs=out["XS"], us=out["US"],
                              iters=out["IT"])
    out["IT"] = out["IT"].reshape(STEPS, batch)
    return out


@pytest.mark.parametrize("batch", [5, 80])
@pytest.mark.parametrize("kernel,name", [(0, "resident"), (3, "panel")])
@pytest.mark.parametrize("dyn", ["decay", "rise", "mixed"])
def test_floor_closed_loop_covers_every_step(gpu, oracle, dyn, kernel, name, batch):
    """include/gpad.h: the stats of gpad_closed_loop aggregate over every (step, instance).  Every
    step's solve stores its own per-workgroup maxima, so the run's floor must be folded over the
    steps: with decaying dynamics the maximum is at step 0, with rising ones at the last step, and
    the mixed batch has packs of both kinds.  Exact equality (floor_scale = margin); TOL_FLOOR
    follows the aggregated floor for a tol between the last step's floor and the run's."""
    p = _Plant(DYNAMICS[dyn])
    margin = MARGIN[np.float32]
    X0 = _x0(dyn, batch)
    probe = margin * _step_maxima_f32(oracle, p, _cl_oracle(oracle, p, X0, 1e-4))
    between = float(np.sqrt(probe[-1] * probe.max())) if probe[-1] < probe.max() else 0.5 * float(probe.max())
    with _plant_solver(p.qp, p, batch, kernel=kernel) as s:
        for tol in (between, 2.0 * float(probe.max())):
            ref = _cl_oracle(oracle, p, X0, tol)
            steps = margin * _step_maxima_f32(oracle, p, ref)
            floor = float(steps.max())
            assert np.isfinite(steps).all()
            if dyn != "rise":  # the run's maximum is not the last step's
                assert steps[-1] < 0.5 * floor
                if tol == between:
                    assert steps[-1] < tol < floor
            out = _cl_run(s, p, X0, tol)
            for b, r in enumerate(ref):  # (the trajectories the reference floor was taken from)
                np.testing.assert_array_equal(out["XS"][:, b], r[3], err_msg=f"xs[{b}]")
            _check(out["st"], floor, tol, name, True, (dyn, tol, steps))
            _check(s.last_stats(), floor, tol, name, True, ("last_stats", dyn, tol))


@pytest.mark.parametrize("dyn", ["decay", "rise", "mixed"])
def test_floor_closed_loop_f64(gpu, dyn):
    """f64 closed loop (stream kernel): the reference g(x_t) is the affine fma chain, evaluated
    exactly, on the trajectory the run returned; margin 2^-49, exact equality."""
    p = _Plant(DYNAMICS[dyn])
    margin = MARGIN[np.float64]
    batch = 5
    X0 = _x0(dyn, batch).astype(np.float64)
    def step_floors(out):
        return margin * np.array([max(np.abs(_affine_f64(p.Pg, p.g0, out["XS"][t, b])).max() for b in range(batch))
                                  for t in range(STEPS)])

    with _plant_solver(p.qp, p, batch, dtype=np.float64) as s:
        first = float(step_floors(_cl_run(s, p, X0, 1e-4, dtype=np.float64)).max())
        for tol in (1e-4, 0.5 * first, 2.0 * first):  # (the trajectory, so the floor, moves a little with tol)
            out = _cl_run(s, p, X0, tol, dtype=np.float64)
            steps = step_floors(out)
            floor = float(steps.max())
            if dyn != "rise":
                assert steps[-1] < 0.5 * floor
            _check(out["st"], floor, tol, "stream", True, (dyn, tol, steps))
            _check(s.last_stats(), floor, tol, "stream", True, ("last_stats", dyn, tol))


@pytest.mark.parametrize("batch,bad", [(5, 3), (80, 78)])
@pytest.mark.parametrize("kernel,name", [(0, "resident"), (3, "panel")])
def test_closed_loop_nan_state_is_isolated(gpu, oracle, kernel, name, batch, bad):
    """One pack starts from a NaN state: the run is flagged, the floor is NaN, and every other pack
    -- the ones sharing its 16-column panel included -- equals the oracle bit for bit."""
    p = _Plant(DYNAMICS["decay"])
    X0 = _x0("decay", batch)
    X0[bad, 1] = np.nan
    tol = 1e-2
    ref = _cl_oracle(oracle, p, X0, tol)
    with _plant_solver(p.qp, p, batch, kernel=kernel) as s:
        out = _cl_run(s, p, X0, tol)
        st = out["st"]
        assert st["kernel"] == name
        assert st["nonfinite_g"] and st["below_tol_floor"] and np.isnan(st["tol_floor"]), st
        ls = s.last_stats()
        assert ls["nonfinite_g"] and ls["below_tol_floor"] and np.isnan(ls["tol_floor"]), ls
    for b, (x, z, y, xs, us, its) in enumerate(ref):
        if b == bad:
            continue
        np.testing.assert_array_equal(out["XS"][:, b], xs, err_msg=f"xs[{b}]")
        np.testing.assert_array_equal(out["US"][:, b], us, err_msg=f"us[{b}]")
        np.testing.assert_array_equal(out["X"][b], x, err_msg=f"x[{b}]")
        np.testing.assert_array_equal(out["Z"][b], z, err_msg=f"z[{b}]")
        np.testing.assert_array_equal(out["Y"][b], y, err_msg=f"y[{b}]")
        np.testing.assert_array_equal(out["IT"][:, b], its, err_msg=f"iters[{b}]")


def test_closed_loop_nan_state_is_isolated_f64(gpu):
    """f64: the packs beside the NaN one equal, bit for bit, the same run with a healthy pack in its
    place; the floor is NaN and the run flagged."""
    p = _Plant(DYNAMICS["decay"])
    batch, bad, tol = 5, 3, 1e-6
    X0 = _x0("decay", batch).astype(np.float64)
    XN = X0.copy()
    XN[bad, 1] = np.nan
    with _plant_solver(p.qp, p, batch, dtype=np.float64) as s:
        good = _cl_run(s, p, X0, tol, dtype=np.float64)
        out = _cl_run(s, p, XN, tol, dtype=np.float64)
    assert not good["st"]["nonfinite_g"] and np.isfinite(good["st"]["tol_floor"])
    st = out["st"]
    assert st["nonfinite_g"] and st["below_tol_floor"] and np.isnan(st["tol_floor"]), st
    keep = [b for b in range(batch) if b != bad]
    for k in ("XS", "US", "IT"):
        np.testing.assert_array_equal(out[k][:, keep], good[k][:, keep], err_msg=k)
    for k in ("X", "Z", "Y"):
        np.testing.assert_array_equal(out[k][keep], good[k][keep], err_msg=k)


# ------------------------------------------------------------------ groups
def _sharded(devices, Z, Y, ML, M, G, g, N, L, tol):
    from gpad_mpc import _lib
    lib = _lib.load()
    B, n = M.shape
    d = _lib.Dims(n=n, m=g.shape[1], batch=B, shared=1, dtype=_lib.DTYPE_F32, memory=_lib.MEM_HOST,
                  schedule=_lib.SCHEDULE_MATLAB, check_every=10, kernel=_lib.KERNEL_AUTO)
    st = _lib.Stats()
    devs = (C.c_int * len(devices))(*devices)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    _lib.check(lib.gpad_solve_sharded(len(devices), devs, p(Z), p(Y), p(ML), p(M), p(G), p(g), N, float(L), tol,
                                      C.byref(d), C.byref(st)), "gpad_solve_sharded")
    import gpad_mpc
    return gpad_mpc.GpadSolver._stats_dict(st)


def _group_runs(ML, M, G, g, L):
    """[(label, run(gp, tol) -> stats)] for GpadGroup.run and gpad_solve_sharded, two shards on device 0."""
    import gpad_mpc
    B, n = M.shape
    m = g.shape[1]
    grp = gpad_mpc.GpadGroup([0, 0])
    grp.setup(ML, G, L, n=n, m=m, batch=B)

    def group(gp, tol):
        return grp.run(np.zeros_like(M), np.zeros_like(g), M, gp, 20, tol)

    def sharded(gp, tol):
        return _sharded([0, 0], np.zeros_like(M), np.zeros_like(g), ML, M, G, gp, 20, L, tol)

    return grp, [("group", group), ("sharded", sharded)]


def test_floor_group_shards(gpu):
    """Two shards: the maximum planted in the first shard, then in the last."""
    from gpad_mpc import _lib
    n, m, B = 40, 72, 37
    ML, M, G, g, L = _qp(n, m, B)
    margin = MARGIN[np.float32]
    grp, runs = _group_runs(ML, M, G, g, L)
    with grp:
        for b, i in [(0, 0), (5, m - 1), (B - 1, m - 1), (B - 3, 0)]:
            gp, gmax = _plant(g, b, i)
            floor = margin * gmax
            for tol in (1e-4, 0.5 * floor):
                for label, run in runs:
                    _check(run(gp, tol), floor, tol, "resident", False, (label, b, i, tol))
    _lib.load().gpad_release_cached()  # (gpad_solve_sharded's cached group)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_group_keeps_a_nonfinite_floor(gpu, bad):
    """include/gpad.h: the floor is NaN when g holds a NaN.  A shard's NaN floor must dominate the
    fold over the shards (std::max drops a NaN), an infinite one must be kept."""
    from gpad_mpc import _lib
    n, m, B = 40, 72, 37
    ML, M, G, g, L = _qp(n, m, B)
    grp, runs = _group_runs(ML, M, G, g, L)
    with grp:
        for b in (2, B - 2):  # first shard, last shard
            gp = g.copy()
            gp[b, 7] = bad
            for label, run in runs:
                st = run(gp, 1e-4)
                assert st["nonfinite_g"] and st["below_tol_floor"], (label, b, st)
                assert (np.isnan(st["tol_floor"]) if np.isnan(bad) else np.isinf(st["tol_floor"])), (label, b, st)
    _lib.load().gpad_release_cached()


# ------------------------------------------------------------------ non-finite g inside a panel
def _oracle_f32(oracle, ML, M, G, g, N, L, tol):
    """oracle.solve_f32 returning the termination code (pyoracle returns it as a bool)."""
    MGneg, GL, pD = oracle.scale(ML, G, g, np.float32(L))
    return _oracle_scaled(oracle, MGneg, M, GL, pD, N, L, tol)


def _oracle_scaled(oracle, MGneg, gP, GL, pD, N, L, tol):
    fp = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    n, m = MGneg.shape
    z = np.zeros(n, np.float32)
    y = np.zeros(m, np.float32)
    th, be = oracle.schedule_f32(max(N, 1))
    MGneg, gP, GL, pD = (np.ascontiguousarray(a, np.float32) for a in (MGneg, gP, GL, pD))
    code = C.c_int(0)
    it = oracle.lib.orc_solve_f32(fp(z), fp(y), fp(MGneg), fp(gP), fp(GL), fp(pD), n, m, N, np.float32(L), float(tol),
                                  0.0, 10, fp(th), fp(be), C.byref(code))
    return z, y, it, code.value


NAN_N, NAN_TOL = 60, 1e-2  # (the healthy instances: some converge within N, most do not)


def _assert_isolated(st, Z, Y, it, codes, bstar, bad, ref, exact=True):
    """The run is flagged with a NaN / inf floor, instance bstar did not converge, every other
    instance equals ref(b) -> (z, y, iterations, code)."""
    assert st["nonfinite_g"] and st["below_tol_floor"], st
    assert (np.isnan(st["tol_floor"]) if np.isnan(bad) else np.isinf(st["tol_floor"])), st
    assert it[bstar] == NAN_N and codes[bstar] == 0, (bstar, it[bstar], codes[bstar])
    for b in range(Z.shape[0]):
        if b == bstar:
            continue
        z, y, its, code = ref(b)
        assert (it[b], codes[b]) == (its, code), (b, it[b], codes[b], its, code)
        if exact:
            np.testing.assert_array_equal(Z[b], z, err_msg=f"z[{b}]")
            np.testing.assert_array_equal(Y[b], y, err_msg=f"y[{b}]")
        else:
            np.testing.assert_allclose(Z[b], z, rtol=1e-12, atol=1e-14, err_msg=f"z[{b}]")
            np.testing.assert_allclose(Y[b], y, rtol=1e-12, atol=1e-14, err_msg=f"y[{b}]")


@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("n,m,B,kernel,name,grid", [(40, 64, 6, 0, "resident", 0), (37, 53, 40, 3, "panel", 0),
                                                    (200, 200, 40, 3, "panel", 0), (200, 200, 40, 3, "panel", 1)])
def test_nonfinite_g_is_isolated(gpu, oracle, n, m, B, kernel, name, grid, bad):
    """g[b*, 7] = NaN / +inf for b* = 3 and b* = B - 2 (in the ragged last panel): the resident
    kernel, the small panels and the folded panels (one panel per workgroup; three on one)."""
    ML, M, G, g, L = _qp(n, m, B)
    good = {}

    def ref(b):
        if b not in good:
            good[b] = _oracle_f32(oracle, ML, M[b], G, g[b], NAN_N, L, NAN_TOL)
        return good[b]

    with _solver(ML, G, L, M, g, kernel=kernel) as s:
        if grid:
            s.set_option("panel_max_grid", grid)
        for bstar in (3, B - 2):
            gp = g.copy()
            gp[bstar, 7] = bad
            Z, Y = np.zeros_like(M), np.zeros_like(g)
            it, codes = np.zeros(B, np.int32), np.full(B, -1, np.int32)
            st = s.run(Z, Y, M, gp, NAN_N, NAN_TOL, iters=it, codes=codes)
            assert st["kernel"] == name
            _assert_isolated(st, Z, Y, it, codes, bstar, bad, ref)
            ls = s.last_stats()
            assert ls["nonfinite_g"] and ls["below_tol_floor"], ls
            assert (np.isnan(ls["tol_floor"]) if np.isnan(bad) else np.isinf(ls["tol_floor"])), ls


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_nonfinite_g_is_isolated_flat_panels(gpu, oracle, bad):
    """The flat panels (phased): p_D[b*, 7] = NaN / +inf, every other instance equals the oracle's
    flat solve."""
    import gpad_mpc
    from gpad_mpc import _lib, problems
    n_u, Nh, B = 4, 10, 40
    qp = problems.battery_scenarios(n_u, Nh, B, seed=4)
    MGf, GLf, L = problems.flatten_battery(qp, n_u, Nh)
    L32 = np.float32(L)
    MGf, GLf, GP = F32(MGf), F32(GLf), F32(qp.M)
    PD = np.ascontiguousarray(oracle.scale_vec(F32(qp.g), L32))
    good = {}

    def ref(b):
        if b not in good:
            good[b] = oracle.solve_flat_f32(np.zeros(qp.n), np.zeros(qp.m), MGf, GP[b], GLf, PD[b], n_u, NAN_N, L32,
                                            NAN_TOL)
        return good[b]

    with gpad_mpc.GpadSolver(0) as s:
        s.setup_flat(MGf, GLf, float(L32), n_u=n_u, batch=B, kernel=_lib.KERNEL_PANEL)
        s.set_option("phased", 2)
        for bstar in (3, B - 2):
            pd = PD.copy()
            pd[bstar, 7] = bad
            Z, Y = np.zeros_like(GP), np.zeros_like(PD)
            it, codes = np.zeros(B, np.int32), np.full(B, -1, np.int32)
            st = s.run(Z, Y, GP, pd, NAN_N, NAN_TOL, scaled=True, iters=it, codes=codes)
            assert st["kernel"] == "flat"
            _assert_isolated(st, Z, Y, it, codes, bstar, bad, ref)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_nonfinite_g_is_isolated_f64_panels(gpu, oracle, bad):
    """The f64 panels: every other instance within 1e-12 of the fp64 oracle, counts and convergence
    equal."""
    n, m, B = 40, 64, 20
    ML, M, G, g, L = _qp(n, m, B, dtype=np.float64)
    good = {}

    def ref(b):
        if b not in good:
            z, y, its, conv = oracle.solve_f64(np.zeros(n), np.zeros(m), ML, M[b], G, g[b], NAN_N, L, NAN_TOL)
            good[b] = (z, y, its, conv)
        return good[b]

    with _solver(ML, G, L, M, g, kernel=3) as s:
        for bstar in (3, B - 2):
            gp = g.copy()
            gp[bstar, 7] = bad
            Z, Y = np.zeros_like(M), np.zeros_like(g)
            it, codes = np.zeros(B, np.int32), np.full(B, -1, np.int32)
            st = s.run(Z, Y, M, gp, NAN_N, NAN_TOL, iters=it, codes=codes)
            assert st["kernel"] == "panel"
            _assert_isolated(st, Z, Y, it, (codes > 0).astype(np.int32), bstar, bad, ref, exact=False)


# ------------------------------------------------------------------ gpad_last_phases
def test_last_phases_prior_is_the_last_runs(gpu):
    """A handle that followed the shape's plan prior and then runs non-phased (fixed N): the last run
    has no phases and followed no prior."""
    from gpad_mpc import _lib
    n = m = 200
    B, N, tol = 40, 137, 1e-4
    ML, M, G, g, L = _qp(n, m, B)

    def solve(s, N, tol):
        s.run(np.zeros_like(M), np.zeros_like(g), M, g, N, tol)
        return s.last_phases()

    with _solver(ML, G, L, M, g, kernel=_lib.KERNEL_PANEL) as a, _solver(ML, G, L, M, g, kernel=_lib.KERNEL_PANEL) as b:
        solve(a, N, tol)  # a's plan becomes the shape's prior
        pb = solve(b, N, tol)
        assert pb["prior"] and len(pb["ends"]) >= 1, pb
        pf = solve(b, 30, 0.0)
        assert pf["ends"] == [] and pf["prior"] is False, pf
