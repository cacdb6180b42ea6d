"""The infeasibility certificate on the MFMA panel carriers at every tile count and shape:
gpad_panel_farkas_kernel<T> (T = 1..16, the T-wave panels a bound handle runs) and
gpad_loop_panel_farkas_kernel<T, kCls> (the panel loop and the fused class loop), csrc/gpad_farkas.h.

The battery packs and small goldens of tests/test_infeasible.py reach T = 1, 3, 4 and 12 and column tiles 0..2 of
the G/L image.  Here every T runs, with n > m, m > n, the exact tile edges 16 and 256, and both dimensions ragged
in the last tile, on mixed batches whose answer is known by construction (tests/infeas_cases.py slab_batch): rows
i (row tile 0) and j (the last row tile) of G are opposite, a feasible instance carries a witness zf inside the
box, and an infeasible one has g_j = -g_i - 1.  The same construction with one signal on row j gives a wide plant
whose packs turn infeasible by script (slab_plant, slab_loop_inputs).

What the GPU tests take for granted is asserted on the reference itself by the CPU tests below: the codes of
every instance, the nominated-but-not-certified columns, the columns certified at the same event, the cap cases
and the loop scripts.  Seeds were chosen there.  Reference: tests/infeas_ref64.py (fp64, and its f32 emulation);
the closed loops: tests/loop_ref64.py's plant arithmetic around it.

test_loop_async.loop takes no signals, so the loops here run through _loop below (the generic form of
test_infeasible._loop).
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import pytest

import gpad_mpc
import infeas_cases as cases
import infeas_ref64 as ref
from gpad_mpc import _lib, problems
from test_infeasible import F32, F64, _L, bound_solver, run, same

N, TOL, R = cases.N, cases.TOL, cases.SLAB_R
SEED, BATCH = 1, 6
# (T, n, m): every tile count of the panels.  T = 1 and T = 16 hold more than one shape: the one-tile shape
# with m < 8 and the exact edge 16 x 16; n > m and m > n by twelve tiles, the exact edge 256 x 256 and both
# dimensions ragged.  T = 9, 13 and 16 are ragged in both dimensions; T = 10 and 15 have n > m, T = 11 m > n.
SHAPES = [(1, 1, 5), (1, 16, 16), (2, 17, 31), (3, 33, 48), (4, 40, 64), (5, 80, 65), (6, 50, 96), (7, 72, 100),
          (8, 128, 120), (9, 130, 137), (10, 150, 40), (11, 40, 170), (12, 192, 177), (13, 200, 193), (14, 144, 220),
          (15, 233, 60), (16, 241, 250), (16, 256, 256), (16, 250, 40), (16, 40, 250)]
IDS = ["T%d-%dx%d" % s for s in SHAPES]
MULTI = [(4, 40, 64), (9, 130, 137), (16, 241, 250)]  # batches of 37: three panels, the last ragged
CAPS = [(4, 40, 64), (16, 250, 40)]                   # the cap at a certificate event
WIDE64 = [(9, 130, 137), (16, 250, 40), (16, 256, 256)]  # the fp64 reference against the f64 engine
KEYS = ("x", "z", "y", "xs", "us", "it", "cd")


def _ids(shapes):
    return ["T%d-%dx%d" % s for s in shapes]


def v_star(n, m):
    """The smallest count at which the fp64 reference certifies an instance of the batch, and the instances."""
    r64 = cases.slab_reference(n, m, BATCH, SEED)
    v = min(r.it for r in r64 if r.code == 5)
    return v, [k for k, r in enumerate(r64) if r.code == 5 and r.it == v]


# ------------------------------------------------------------------------------------ 1. the inputs (no GPU)
def _check_instances(b, refs, count):
    G32 = F32(b.qp.G)
    for k in range(count):
        g32, r = F32(b.g[k]), refs[k]
        if b.bad[k]:
            assert r.code == 5 and r.it < N, (k, r.code, r.it)
            assert ref.farkas_margin(G32, g32, r.y, R) > 0.0, k
        else:
            assert r.code in (1, 2) and np.abs(r.z).max() < R, (k, r.code, np.abs(r.z).max())
            zf = b.zf[k]
            assert (G32.astype(np.float64) @ zf <= g32.astype(np.float64)).all() and np.abs(zf).max() <= R, k


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_slab_batches_cpu(shape):
    """Every infeasible instance ends 5 before N with a positive margin on the f32-rounded G, g, every feasible
    one ends 1 or 2 inside the bound, and its witness zf meets the f32-rounded constraints: in fp64 and in the
    f32 emulation.  Row i lies in row tile 0 and row j in the last one."""
    T, n, m = shape
    assert T == (max(n, m) + 15) // 16
    b = cases.slab_batch(n, m, BATCH, SEED)
    i, j = b.rows
    assert i != j and i < 16 and j // 16 == (m - 1) // 16
    assert 0 < b.bad.sum() < BATCH
    for dt in (np.float64, np.float32):
        _check_instances(b, cases.slab_reference(n, m, BATCH, SEED, dt), BATCH)


def test_slab_event_paths_cpu():
    """The event paths the GPU tests lean on exist in these inputs: a feasible instance that is nominated and not
    certified at T <= 8 and at T > 8, infeasible instances of one panel certified at the same count (several
    columns decided at one event), and the cap cases: v* is a certificate event past the first one, some instance
    is still running at v* - 40, and some feasible one has converged before it."""
    nominated = {T: 0 for T, _, _ in SHAPES}
    together = 0
    for T, n, m in SHAPES:
        b, r64 = cases.slab_batch(n, m, BATCH, SEED), cases.slab_reference(n, m, BATCH, SEED)
        nominated[T] += sum(r.nominated > 0 for k, r in enumerate(r64) if not b.bad[k])
        counts = [r.it for r in r64 if r.code == 5]
        together += len(counts) > len(set(counts))
    assert any(v > 0 for T, v in nominated.items() if T <= 8) and any(v > 0 for T, v in nominated.items() if T > 8)
    assert together >= 1
    for T, n, m in CAPS:
        v, who = v_star(n, m)
        r64 = cases.slab_reference(n, m, BATCH, SEED)
        assert v % 40 == 0 and v >= 80 and who
        assert any(r.code in (1, 2) and r.it < v - 40 for r in r64)
        for dt in (np.float64, np.float32):  # the capped runs of the reference: (5, v*) and (0, v* - 40)
            b = cases.slab_batch(n, m, BATCH, SEED)
            for k in who:
                at = ref.solve(b.qp.ML, b.M[k], b.qp.G, b.g[k], b.qp.L, v, TOL, R, dt)
                under = ref.solve(b.qp.ML, b.M[k], b.qp.G, b.g[k], b.qp.L, v - 40, TOL, R, dt)
                assert (at.code, at.it, under.code, under.it) == (5, v, 0, v - 40), (n, m, k, dt)


@pytest.mark.parametrize("shape", MULTI, ids=_ids(MULTI))
def test_slab_batches_of_37_cpu(shape):
    """The batches of three panels: the mask holds on every instance (fp64 reference)."""
    T, n, m = shape
    b = cases.slab_batch(n, m, 37, SEED)
    assert np.array_equal(b.M[:BATCH], cases.slab_batch(n, m, BATCH, SEED).M)  # (a smaller batch is a prefix)
    _check_instances(b, [ref.solve(b.qp.ML, b.M[k], b.qp.G, b.g[k], b.qp.L, N, TOL, R) for k in range(37)], 37)


# the plants of the panel loops: (n, m, nx, nu) -> the feasible width of the slab, chosen on the CPU
PLANTS = {"T9": (70, 130, 5, 2), "T16": (200, 250, 4, 3)}
WIDTH = 2.0
TWIN_ROWS = (7, 100)  # class 1 of the fused class loop: the T9 plant with another pair of opposite rows


@functools.lru_cache(maxsize=None)
def loop_reference(key, warm, batch=16):
    n, m, nx, nu = PLANTS[key]
    pl, I = cases.slab_plant(n, m, nx, nu, packs=batch), cases.slab_loop_inputs(WIDTH, batch)
    return cases.slab_loop_reference(pl, pl.qp.L, pl.X0, I.S, warm=warm)


def _check_script(r, I):
    assert ((r.cd == 5) == I.want).all(), r.cd
    assert np.isin(r.cd[~I.want], (1, 2)).all() and r.it.max() < N, (r.cd, r.it.max())


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("key", list(PLANTS))
def test_slab_plant_cpu(key, warm):
    """The reference closed loop of the slab plants: the 5s stand exactly where the script puts them, every other
    solve ends 1 or 2 before N inside the bound; the plant keeps the panel loop's shape rules; the packs of one
    panel end their solves at different counts (the columns of a loop panel sit at different counts)."""
    n, m, nx, nu = PLANTS[key]
    pl, I = cases.slab_plant(n, m, nx, nu), cases.slab_loop_inputs(WIDTH)
    assert (max(n, m) + 15) // 16 == int(key[1:]) and pl.nx + pl.ns <= 64 and N % 10 == 0
    i, j = pl.rows
    assert i < 16 and j // 16 == (m - 1) // 16 and I.want.sum() == 6 and I.want[:, 6].tolist() == [True] + [False] * 4
    r = loop_reference(key, warm)
    _check_script(r, I)
    assert np.abs(r.z).max() < R and np.abs(r.us).max() < R
    assert all(len(set(row)) >= 3 for row in r.it.tolist())


def test_slab_plant_37_cpu():
    """The 37 packs of the grid-stride loop case (cold): the same script, the further packs feasible throughout."""
    _check_script(loop_reference("T9", False, 37), cases.slab_loop_inputs(WIDTH, 37))


@functools.lru_cache(maxsize=None)
def class_fleet():
    """Two classes of the T9 plant with distinct G/L images: class 0 the slab plant, class 1 its twin with rows
    TWIN_ROWS opposite; packs interleaved, one L (the larger).  -> the per-class stacks (QP, Plant), class_of."""
    n, m, nx, nu = PLANTS["T9"]
    cls = [cases.slab_plant(n, m, nx, nu), cases.slab_plant(n, m, nx, nu, TWIN_ROWS)]
    st = lambda k: np.stack([getattr(c, k) if hasattr(c, k) else getattr(c.qp, k) for c in cls])  # noqa: E731
    qp = problems.QP(ML=st("ML"), M=None, G=st("G"), g=None, L=max(c.qp.L for c in cls), H=st("H"))
    plant = problems.Plant(PM=st("PM"), Pg=st("Pg"), A=st("A"), B=st("B"), M0=st("M0"), g0=st("g0"), Sg=st("Sg"))
    return SimpleNamespace(cls=cls, qp=qp, plant=plant, class_of=np.arange(16) % 2, X0=cls[0].X0)


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_class_fleet_cpu(warm):
    """The two classes' G/L differ where it matters: class 0's opposite rows are not opposite in class 1 and the
    other way round, so a decision on the wrong class's image certifies nothing.  The reference loop of the
    interleaved fleet puts each class's 5s where the script does: packs 6 and 10 are class 0, pack 3 is
    class 1."""
    f, I = class_fleet(), cases.slab_loop_inputs(WIDTH)
    (i0, j0), (i1, j1) = f.cls[0].rows, f.cls[1].rows
    G = f.qp.G
    assert np.array_equal(G[0][j0], -G[0][i0]) and not np.array_equal(G[1][j0], -G[1][i0])
    assert np.array_equal(G[1][j1], -G[1][i1]) and not np.array_equal(G[0][j1], -G[0][i1])
    assert {int(f.class_of[b]) for b in cases.SLAB_BAD} == {0, 1}
    r = cases.slab_loop_reference([f.cls[k] for k in f.class_of], f.qp.L, f.X0, I.S, warm=warm)
    _check_script(r, I)


# ------------------------------------------------------------------------------------ 2. GPU: the solve panels
@functools.lru_cache(maxsize=None)
def device_runs(n, m):
    """The bound f32 runs of slab_batch(n, m, BATCH): the forced panel and the forced stream kernel, once."""
    b = cases.slab_batch(n, m, BATCH, SEED)
    with bound_solver(b.qp, F32, BATCH, bound=R, kernel=_lib.KERNEL_PANEL) as s:
        pan = run(s, F32, b.M, b.g)
    with bound_solver(b.qp, F32, BATCH, bound=R, kernel=_lib.KERNEL_STREAM) as s:
        stm = run(s, F32, b.M, b.g)
    return pan, stm


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_every_tile_count(gpu, shape):
    """gpad_panel_farkas_kernel<T> against the stream kernel: the same bytes; every infeasible instance ends 5
    before N with a positive margin from the library's evaluator and from numpy's on the caller's f32 G, g and
    the returned y; every other instance ends 1 or 2; no instance with a witness returns 5; the stats agree with
    the per-instance arrays."""
    T, n, m = shape
    assert T == (max(n, m) + 15) // 16  # panel_tiles_for (csrc/gpad_panel.h): the instantiation the id names
    b = cases.slab_batch(n, m, BATCH, SEED)
    pan, stm = device_runs(n, m)
    print(IDS[SHAPES.index(shape)], "codes", pan.cd.tolist(), "counts", pan.it.tolist(), "stream", stm.cd.tolist(),
          stm.it.tolist())
    assert (pan.st["kernel"], stm.st["kernel"]) == ("panel", "stream")
    same(pan, stm)
    G32, g32 = F32(b.qp.G), F32(b.g)
    for r in (pan, stm):
        for k in range(BATCH):
            if b.bad[k]:
                assert r.cd[k] == 5 and r.it[k] < N, (k, r.cd[k], r.it[k])
            else:  # a witness zf exists: a 5 here is a proof of a bug, whatever any reference says
                assert r.cd[k] in (1, 2), (k, r.cd[k])
            if r.cd[k] == 5:
                assert gpad_mpc.farkas_margin(G32, g32[k], r.y[k], R) > 0.0, k
                assert ref.farkas_margin(G32, g32[k], r.y[k], R) > 0.0, k
        assert r.st["converged"] == int(np.isin(r.cd, (1, 2)).sum())
        assert r.st["total_iterations"] == int(r.it.sum()) and r.st["iterations"] == int(r.it.max())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_f32_codes_match_reference(gpu, shape):
    """The codes of the f32 runs equal the fp64 reference's, instance for instance.  Counts are not compared:
    numpy's f32 products sum in another order, and the two precisions of the reference already differ by up to
    20 iterations on these inputs."""
    T, n, m = shape
    want = [r.code for r in cases.slab_reference(n, m, BATCH, SEED)]
    for r in device_runs(n, m):
        assert r.cd.tolist() == want, (r.st["kernel"], r.cd.tolist(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MULTI, ids=_ids(MULTI))
def test_three_panels(gpu, shape):
    """Batch 37: three panels with the last ragged.  The phased run, a grid of one workgroup walking the panels
    (survivor lists read through idx_in), phases that end on a certificate event (40) and phases that do not
    (30), and one launch (phased 0) give the forced stream kernel's bytes."""
    T, n, m = shape
    b = cases.slab_batch(n, m, 37, SEED)
    with bound_solver(b.qp, F32, 37, bound=R, kernel=_lib.KERNEL_STREAM) as s:
        stm = run(s, F32, b.M, b.g)
    assert stm.st["kernel"] == "stream"
    for k in range(37):
        assert stm.cd[k] == 5 and stm.it[k] < N if b.bad[k] else stm.cd[k] in (1, 2), (k, stm.cd[k], stm.it[k])
    print(_ids([shape])[0], "codes", stm.cd.tolist(), "counts", stm.it.tolist())
    # (plan 0: the phase ends are phase_len's, not those of the plan an earlier run of the shape left behind)
    for opts in (dict(panel_max_grid=0), dict(panel_max_grid=1), dict(phase_len=40, plan=0), dict(phase_len=30, plan=0),
                 dict(phase_len=40, plan=0, panel_max_grid=1), dict(phased=0)):
        with bound_solver(b.qp, F32, 37, bound=R, kernel=_lib.KERNEL_PANEL) as s:
            s.set_options(**opts)
            r = run(s, F32, b.M, b.g)
            ends = s.last_phases()["ends"]
        print(opts, "phases", ends[:8])
        assert r.st["kernel"] == "panel", opts
        if opts.get("phased", 1):
            assert len(ends) >= 2, (opts, ends)
            if "phase_len" in opts:
                assert ends[:2] == [opts["phase_len"], 2 * opts["phase_len"]], (opts, ends)
        same(r, stm)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", CAPS, ids=_ids(CAPS))
def test_cap_at_a_certificate_event(gpu, shape):
    """N = v*, the smallest count at which the reference certifies an instance: that column reaches N at a
    certificate event and ends (5, v*); with N = v* - 40 it ends (0, N).  Panel and stream give the same bytes
    in both runs, and the feasible instances that converge before the cap keep their counts of the N = 3000
    run."""
    T, n, m = shape
    b = cases.slab_batch(n, m, BATCH, SEED)
    v, who = v_star(n, m)
    full = device_runs(n, m)[1]
    for cap in (v, v - 40):
        with bound_solver(b.qp, F32, BATCH, bound=R, kernel=_lib.KERNEL_PANEL) as s:
            pan = run(s, F32, b.M, b.g, cap)
        with bound_solver(b.qp, F32, BATCH, bound=R, kernel=_lib.KERNEL_STREAM) as s:
            stm = run(s, F32, b.M, b.g, cap)
        print(_ids([shape])[0], "N", cap, "codes", pan.cd.tolist(), "counts", pan.it.tolist())
        assert (pan.st["kernel"], stm.st["kernel"]) == ("panel", "stream")
        same(pan, stm)
        for k in who:
            assert (pan.cd[k], pan.it[k]) == ((5, v) if cap == v else (0, cap)), (cap, k, pan.cd[k], pan.it[k])
        early = [k for k in range(BATCH) if not b.bad[k] and full.it[k] < cap]
        assert early or cap != v
        for k in early:
            assert (pan.cd[k], pan.it[k]) == (full.cd[k], full.it[k]), (cap, k)
            assert pan.z[k].tobytes() == full.z[k].tobytes() and pan.y[k].tobytes() == full.y[k].tobytes(), (cap, k)
        for k in range(BATCH):
            if pan.cd[k] == 5:
                assert gpad_mpc.farkas_margin(F32(b.qp.G), F32(b.g[k]), pan.y[k], R) > 0.0, (cap, k)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", WIDE64, ids=_ids(WIDE64))
def test_f64_matches_reference_wide(gpu, shape):
    """The f64 stream kernel with the bound against infeas_ref64.solve(dtype=float64) at wide shapes: counts and
    codes equal, every entry of z and y within 1e-9 absolute (the figure test_infeasible.test_f64_matches_reference
    and tests/test_loop_f64.py ask of the f64 engine)."""
    T, n, m = shape
    b, r64 = cases.slab_batch(n, m, BATCH, SEED), cases.slab_reference(n, m, BATCH, SEED)
    with bound_solver(b.qp, F64, BATCH, bound=R, kernel=_lib.KERNEL_STREAM) as s:
        r = run(s, F64, b.M, b.g)
    far = lambda x, y: float(np.abs(x - y).max())  # noqa: E731
    devs = [max(far(r.z[k], r64[k].z), far(r.y[k], r64[k].y)) for k in range(BATCH)]
    print(_ids([shape])[0], "codes", r.cd.tolist(), "counts", r.it.tolist(), "reference", [x.it for x in r64],
          "z / y deviation per instance", ["%.2g" % d for d in devs],
          "largest |y|", max(float(np.abs(x.y).max()) for x in r64))
    assert r.st["kernel"] == "stream"
    assert r.it.tolist() == [x.it for x in r64]
    assert r.cd.tolist() == [x.code for x in r64]
    assert 5 in r.cd and max(devs) <= 1e-9
    for k in range(BATCH):
        if r.cd[k] == 5:
            assert gpad_mpc.farkas_margin(F64(b.qp.G), F64(b.g[k]), r.y[k], R) > 0.0


# ------------------------------------------------------------------------------------ 3. GPU: the panel loops
def _loop(s, pl, X0, I, warm, N=N, tol=TOL):
    B, steps = I.batch, I.steps
    x, z, y = F32(X0), np.zeros((B, pl.n), np.float32), np.zeros((B, pl.m), np.float32)
    xs, us = np.zeros((steps, B, pl.nx), np.float32), np.zeros((steps, B, pl.nu), np.float32)
    it, cd = np.full(steps * B, -1, np.int32), np.full(steps * B, -1, np.int32)
    st = s.closed_loop(x, z, y, steps, N, tol, warm=warm, xs=xs, us=us, iters=it, codes=cd, signals=F32(I.S))
    return SimpleNamespace(x=x, z=z, y=y, xs=xs, us=us, it=it.reshape(steps, B), cd=cd.reshape(steps, B), st=st)


def _plant_solver(pl, batch, mode, grid=None):
    """The slab plant bound with R: "stream" (the lockstep loop on the forced stream kernel, the base), "lockstep"
    (AUTO: the T-wave certificate panels) and "loop_panel"."""
    qp = pl.qp
    s = gpad_mpc.GpadSolver(0)
    s.setup(F32(qp.ML), F32(qp.G), _L(qp, F32), n=pl.n, m=pl.m, batch=batch,
            kernel=_lib.KERNEL_STREAM if mode == "stream" else _lib.KERNEL_AUTO)
    s.setup_plant(F32(pl.PM), F32(pl.Pg), M0=F32(pl.M0), g0=F32(pl.g0), A=F32(pl.A), B=F32(pl.B))
    s.setup_signals(None, F32(pl.Sg), None)
    if mode == "loop_panel":
        s.set_option("loop_panel", 1)
    if grid is not None:
        s.set_option("panel_max_grid", grid)
    s.setup_infeasibility(R)
    return s


def _same_loop(r, base, what):
    for k in KEYS:
        assert getattr(r, k).tobytes() == getattr(base, k).tobytes(), (what, k)
    assert r.st["converged"] == base.st["converged"], what


def _check_loop(r, pl, I):
    """The 5s stand where the script puts them, no solve runs to N, and the last step's y of a pack that ends
    with a 5 certifies on g(x, s) of that step."""
    assert ((r.cd == 5) == I.want).all() and np.isin(r.cd[~I.want], (1, 2)).all(), r.cd
    assert r.it.max() < N and r.st["converged"] == int((~I.want).sum())
    G32 = F32(pl.qp.G)
    last = np.flatnonzero(I.want[-1])
    assert len(last)
    for b in last:
        xa = np.concatenate([r.xs[-1, b], F32(I.S)[-1, b]]).astype(np.float64)
        g = F32(pl.g0).astype(np.float64) + np.hstack([F32(pl.Pg), F32(pl.Sg)]).astype(np.float64) @ xa
        assert gpad_mpc.farkas_margin(G32, F32(g), r.y[b], R) > 0.0, b
        assert ref.farkas_margin(G32, F32(g), r.y[b], R) > 0.0, b


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_loop_engines(gpu, warm):
    """The T = 9 slab plant (two -ML waves, ragged last G/L tile), 16 packs, five steps: the panel loop
    (gpad_loop_panel_farkas_kernel<9>), also with panel_max_grid 1, and the bound lockstep loop on AUTO
    (gpad_panel_farkas_kernel<9> step by step) give the bytes of the bound lockstep loop on the stream kernel."""
    n, m, nx, nu = PLANTS["T9"]
    pl, I = cases.slab_plant(n, m, nx, nu), cases.slab_loop_inputs(WIDTH)
    with _plant_solver(pl, I.batch, "stream") as s:
        base = _loop(s, pl, pl.X0, I, warm)
    assert base.st["kernel"] == "stream"
    print("warm" if warm else "cold", "codes\n", base.cd, "\ncounts\n", base.it)
    _check_loop(base, pl, I)
    for mode, grid, engine in (("loop_panel", None, "loop_panel"), ("loop_panel", 1, "loop_panel"),
                               ("lockstep", None, "panel")):
        with _plant_solver(pl, I.batch, mode, grid) as s:
            r = _loop(s, pl, pl.X0, I, warm)
        assert r.st["kernel"] == engine, (mode, r.st["kernel"])
        _same_loop(r, base, (mode, grid))


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [0, 1], ids=["grid0", "grid1"])
def test_loop_three_panels(gpu, grid):
    """37 packs of the T = 9 plant: three loop panels with the last ragged, and one workgroup that claims the
    packs beyond its first 16 from the queue as its columns finish."""
    n, m, nx, nu = PLANTS["T9"]
    pl, I = cases.slab_plant(n, m, nx, nu, packs=37), cases.slab_loop_inputs(WIDTH, 37)
    with _plant_solver(pl, 37, "stream") as s:
        base = _loop(s, pl, pl.X0, I, False)
    assert base.st["kernel"] == "stream"
    _check_loop(base, pl, I)
    with _plant_solver(pl, 37, "loop_panel", grid) as s:
        r = _loop(s, pl, pl.X0, I, False)
    assert r.st["kernel"] == "loop_panel"
    _same_loop(r, base, grid)


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_loop_sixteen_tiles(gpu, warm):
    """The same through the panel loop at T = 16: test_loop_async.synthetic(200, 250, 4, 3), workgroups of 1024
    threads (gpad_loop_panel_farkas_kernel<16>)."""
    n, m, nx, nu = PLANTS["T16"]
    pl, I = cases.slab_plant(n, m, nx, nu), cases.slab_loop_inputs(WIDTH)
    with _plant_solver(pl, I.batch, "stream") as s:
        base = _loop(s, pl, pl.X0, I, warm)
    assert base.st["kernel"] == "stream"
    print("warm" if warm else "cold", "codes\n", base.cd, "\ncounts\n", base.it)
    _check_loop(base, pl, I)
    with _plant_solver(pl, I.batch, "loop_panel") as s:
        r = _loop(s, pl, pl.X0, I, warm)
    assert r.st["kernel"] == "loop_panel"
    _same_loop(r, base, "loop_panel")


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_fused_class_loop_distinct_classes(gpu, warm):
    """The fused class loop (gpad_loop_panel_farkas_kernel<9, true>) on two classes whose G/L images differ:
    the bytes of the shared = 0 fleet (problems.expand_classes) on the bound lockstep stream loop, and each
    class's 5s where its own script puts them.  A decision that read the wrong class's image would certify the
    wrong packs or none."""
    f, I = class_fleet(), cases.slab_loop_inputs(WIDTH)
    pl, L = f.cls[0], float(np.float32(f.qp.L))
    eq, ep = problems.expand_classes(f.qp, f.plant, f.class_of)
    with gpad_mpc.GpadSolver(0) as s:
        s.setup(F32(eq.ML), F32(eq.G), L, n=pl.n, m=pl.m, batch=I.batch, shared=False, kernel=_lib.KERNEL_STREAM)
        s.setup_plant(F32(ep.PM), F32(ep.Pg), M0=F32(ep.M0), g0=F32(ep.g0), A=F32(ep.A), B=F32(ep.B))
        s.setup_signals(None, F32(ep.Sg), None)
        s.setup_infeasibility(R)
        base = _loop(s, pl, f.X0, I, warm)
    assert base.st["kernel"] == "stream"
    print("warm" if warm else "cold", "codes\n", base.cd, "\ncounts\n", base.it)
    assert ((base.cd == 5) == I.want).all() and np.isin(base.cd[~I.want], (1, 2)).all(), base.cd
    assert base.it.max() < N
    with gpad_mpc.GpadSolver(0) as s:
        s.setup_classes(F32(f.qp.ML), F32(f.qp.G), L, f.class_of, n=pl.n, m=pl.m)
        s.setup_plant(F32(f.plant.PM), F32(f.plant.Pg), M0=F32(f.plant.M0), g0=F32(f.plant.g0), A=F32(f.plant.A),
                      B=F32(f.plant.B))
        s.setup_class_signals(None, F32(f.plant.Sg), None)
        s.set_class_loop_fused(True)
        s.setup_infeasibility(R)
        r = _loop(s, pl, f.X0, I, warm)
    assert r.st["kernel"] == "loop_classes", r.st["kernel"]
    _same_loop(r, base, "fused")
    for b in np.flatnonzero(I.want[-1]):  # the last step's certificate, on the pack's own class
        c = f.cls[f.class_of[b]]
        xa = np.concatenate([r.xs[-1, b], F32(I.S)[-1, b]]).astype(np.float64)
        g = F32(c.g0).astype(np.float64) + np.hstack([F32(c.Pg), F32(c.Sg)]).astype(np.float64) @ xa
        assert gpad_mpc.farkas_margin(F32(c.qp.G), F32(g), r.y[b], R) > 0.0, b
