"""The closed loop on the MFMA panels (GPAD_OPT_LOOP_PANEL, csrc/gpad_loop_panel.hip): one launch in
which a panel column whose solve ends steps to its pack's next MPC solve in place, and takes the next
pack from a queue after the last step.

The contract is test_loop_async's: with the option on, x, z, y, xs, us, the per-step counts and codes,
every aggregate stat and tol_floor equal gpad_closed_loop with the option off bit for bit, and the
trajectories and counts equal the CPU oracle's closed loop.  Every GPU case asserts on the reported
kernel.  Shapes are the smallest that reach each mechanism: T = 4, 9 and 12 waves, full panels plus a
ragged tail, one workgroup refilling its columns from the queue (panel_max_grid = 1), the schedule
tables in LDS (N = 100 at T = 4; every N at T >= 9) and read from global memory (N = 2000 at T = 4).
"""
from __future__ import annotations

import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import test_fleet as TF
import test_signals as TS
from conftest import ROOT
from test_loop_async import (F32, STAT_KEYS, assert_matches_oracle, assert_same_run, battery, lockstep, loop,
                             make_solver, oracle_loop, same_bits, states, synthetic)

NAME = "loop_panel"


# ------------------------------------------------------------------------------ CPU
def test_option_and_kernel_numbers_match_the_header():
    from gpad_mpc import _lib
    hdr = open(os.path.join(ROOT, "include", "gpad.h")).read()
    opt = dict(re.findall(r"#define GPAD_OPT_(\w+) +\(?(-?\d+)\)?", hdr))
    ker = {k: int(v) for k, v in re.findall(r"#define GPAD_KERNEL_(\w+) +(\d+)", hdr)}
    assert int(opt["LOOP_PANEL"]) == 23 == _lib.OPTIONS["loop_panel"] == _lib.OPT_LOOP_PANEL
    assert ker["LOOP_PANEL"] == 7 == _lib.KERNEL_LOOP_PANEL
    assert _lib.KERNEL_NAMES[7] == NAME
    assert all(_lib.KERNEL_NAMES[v] == k.lower() for k, v in ker.items())


# ------------------------------------------------------------------------------ runs
def panel_run(p, X0, steps, N, tol, warm, *, grid=0, **kw):
    s = make_solver(p, X0.shape[0], **kw)
    s.set_option("loop_panel", 1)
    if grid:
        s.set_option("panel_max_grid", grid)
    return loop(s, p, X0, steps, N, tol, warm)


def check_panel(oracle, key, p, X0, steps, N, tol, warm, grid):
    orc = oracle_loop(oracle, key, p, X0, steps, N, tol, warm)
    ref = lockstep(key, p, X0, steps, N, tol, warm)
    assert ref.st["kernel"] != NAME
    r = panel_run(p, X0, steps, N, tol, warm, grid=grid)
    assert r.st["kernel"] == NAME
    assert_same_run(r, ref)
    assert_matches_oracle(r, orc)
    assert r.st["total_iterations"] == int(orc.it.sum())
    return r, orc


GRIDS = pytest.mark.parametrize("grid", [0, 1], ids=["grid0", "grid1"])
WARM = pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])


# ------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@GRIDS
@pytest.mark.parametrize("tol", [0.0, 1e-4])
@WARM
def test_bit_identity_t4(gpu, oracle, warm, tol, grid):
    """battery(3, 4): n = 12, m = 56, T = 4.  37 packs = two full panels and a tail of 5; with
    grid 1 one workgroup refills finished columns from the queue.  With a tolerance the columns of a
    panel must really be ragged."""
    p = battery(3, 4)
    N = 2000 if tol else 100
    r, orc = check_panel(oracle, "lp34", p, states(p, 37, 7), 6, N, tol, warm, grid)
    if tol:
        assert max(len(set(row[:16])) for row in orc.it.tolist()) >= 3
        assert orc.it.max() < N
    else:
        assert (r.it == N).all() and (r.cd == 0).all()


@pytest.mark.gpu
@GRIDS
@WARM
def test_bit_identity_t12(gpu, oracle, warm, grid):
    """battery(4, 10): n = 40, m = 180, T = 12 (768 threads).  21 packs."""
    p = battery(4, 10)
    r, orc = check_panel(oracle, "lp410", p, states(p, 21, 5), 4, 3000, 1e-4, warm, grid)
    assert max(len(set(row[:16])) for row in orc.it.tolist()) >= 3
    assert orc.it.max() < 3000


@pytest.mark.gpu
@WARM
def test_synthetic_plant(gpu, oracle, warm):
    """synthetic(70, 130, 5, 2): T = 9, M0 and g0 bound, nx != nu.  19 packs on one workgroup."""
    p = synthetic(70, 130, 5, 2, packs=19)
    r, orc = check_panel(oracle, "lps70", p, p.X0, 5, 1500, 1e-4, warm, 1)
    assert all(np.isfinite(getattr(orc, k)).all() for k in ("x", "z", "y", "xs", "us"))
    assert orc.it.max() < 1500


@pytest.mark.gpu
def test_iteration_cap_inside_a_step(gpu, oracle):
    """N = 60: some solves stop at the cap and some earlier, inside one run.  N is a multiple of
    check_every, so the test also runs at iteration 60: of these 37 packs a few pass it exactly there
    (a count of 60 with a code > 0, in the lockstep run as well -- check_panel compares the codes), so
    the codes are > 0 everywhere below the cap, and at the cap both outcomes occur."""
    p = battery(3, 4)
    r, orc = check_panel(oracle, "lp34", p, states(p, 37, 7), 6, 60, 1e-4, False, 1)
    assert (orc.it == 60).any() and (orc.it < 60).any()
    assert (r.cd[r.it < 60] > 0).all()
    at_cap = r.cd[r.it == 60]
    assert (at_cap == 0).any() and (at_cap > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 16])
def test_one_panel(gpu, oracle, batch):
    """A batch of one, and 16 packs exactly: one full panel, no tail, no queue."""
    p = battery(3, 4)
    check_panel(oracle, "lp34", p, states(p, 37, 7)[:batch], 6, 2000, 1e-4, False, 0)


def both_codes_plant(packs=16):
    """synthetic(12, 56, 3, 3) -- battery(3, 4)'s sizes, T = 4 -- with M0 = -z_f, the generator's strictly
    feasible point (its first draw; G z_f - g <= -0.1 in every row).  At x = 0 the unconstrained minimiser
    zhat = -g_P is z_f, so packs with a small state end by test (A) at the first event (code 1), while a
    large state pushes the minimiser out of the feasible set: active constraints, test (B), code 2."""
    base = synthetic(12, 56, 3, 3, packs=packs)
    qp = base.qp
    zf = np.random.default_rng(2).uniform(-0.5, 0.5, qp.n)  # synthetic_qp(seed=1) draws it from seed + 1
    assert (np.asarray(qp.G) @ zf - np.asarray(qp.g).reshape(-1)).max() < -0.09, "zf is not the generator's feasible point"
    scale = np.where(np.arange(packs) % 2 == 0, 0.05, 4.0)
    X0 = (np.random.default_rng(5).uniform(-1, 1, (packs, 3)) * scale[:, None]).astype(np.float32)
    return SimpleNamespace(**dict(vars(base), M0=-zf, X0=X0))


@pytest.mark.gpu
def test_both_codes_in_one_panel(gpu, oracle):
    """One panel of 16 packs whose solves end by test (A) and by test (B) side by side: stage 1, the
    verification GEMM on the direct G_L z and the code selection of gpad_loop_panel_kernel in one
    workgroup (the other cases of this module end every solve with code 2).  The reference's own codes
    -- the lockstep loop's -- hold both in every step."""
    p = both_codes_plant()
    cfg = (3, 2000, 1e-4, False)
    ref = lockstep("lp-codes", p, p.X0, *cfg)
    for t in range(cfg[0]):
        assert {1, 2} <= set(ref.cd[t].tolist()), ref.cd[t]
    assert ref.it.max() < cfg[1]
    r, _ = check_panel(oracle, "lp-codes", p, p.X0, *cfg, 0)
    assert {1, 2} <= set(r.cd[0].tolist())


@pytest.mark.gpu
@WARM
def test_per_pack_plants(gpu, warm):
    """One controller (shared matrices) against 19 per-pack plants (test_fleet.mismatch's construction):
    equal to the lockstep loop, and pack for pack to batch-1 handles."""
    from gpad_mpc import problems
    packs = 19
    caps = 0.027 * 4.1 * np.random.default_rng(119).uniform(0.6, 1.4, (packs, 3))
    qp, pl = problems.battery_fleet(3, 4, caps)
    q0 = SimpleNamespace(ML=qp.ML[0], G=qp.G[0], L=qp.L, n=qp.n, m=qp.m)
    F = SimpleNamespace(qp=q0, nx=3, nu=3, X0=states(battery(3, 4), packs, 19), PM=np.stack([pl.PM[0]] * packs),
                        Pg=pl.Pg, M0=None, g0=pl.g0, A=pl.A, B=pl.B)
    cfg = (6, 2000, 1e-4, warm)
    ref = loop(TF.make_solver(F), F, F.X0, *cfg)
    assert ref.st["kernel"] not in (NAME, "loop")
    s = TF.make_solver(F)
    s.set_options(loop_panel=1, panel_max_grid=1)
    r = loop(s, F, F.X0, *cfg)
    assert r.st["kernel"] == NAME
    assert_same_run(r, ref)
    assert_same_run(r, TF.singles("lp-mismatch19", F, *cfg))
    assert len({F.B[b].tobytes() for b in range(packs)}) == packs  # the plants do differ (A = I in all)


def signals_run(p, X0, S, steps, N, tol, warm, grid=1):
    s = TS.make_solver(p, X0.shape[0])
    s.set_option("loop_panel", 1)
    if grid:
        s.set_option("panel_max_grid", grid)
    return TS.loop(s, p, X0, S, steps, N, tol, warm)


@pytest.mark.gpu
@WARM
def test_signals(gpu, warm):
    """battery_plant_signals(3, 4) under test_signals' mild load set, 19 packs on one workgroup."""
    p = TS.battery(3, 4)
    X0, S = TS.inputs(3, 19, 6, **TS.MILD)
    ref = TS.lockstep("lp-sig34", p, X0, S, 6, 2000, 1e-4, warm)
    assert ref.st["kernel"] != NAME
    r = signals_run(p, X0, S, 6, 2000, 1e-4, warm)
    assert r.st["kernel"] == NAME
    TS.assert_same_run(r, ref)
    assert len(set(r.it.ravel().tolist())) >= 3


@pytest.mark.gpu
def test_state_and_signals_fill_the_row(gpu):
    """nx + ns = 64 on the synthetic plant: the whole state row."""
    p = TS.synth(70, 130, 40, 1, 24)
    X0, S = TS.synth_inputs(p, 4)
    ref = TS.lockstep("lp-s70x64", p, X0, S, 4, 300, 1e-4, False)
    assert all(np.isfinite(getattr(ref, k)).all() for k in ("x", "z", "y", "xs", "us"))
    r = signals_run(p, X0, S, 4, 300, 1e-4, False)
    assert r.st["kernel"] == NAME
    TS.assert_same_run(r, ref)


# ---- fallbacks: the option is accepted and the call goes on as without it
def _battery_case(**kw):
    p = battery(3, 4)
    X0 = states(p, 7, 7)
    return lambda opts: _with(make_solver(p, 7, **kw), opts), lambda s: loop(s, p, X0, 2, 50, 0.0, False,
                                                                          kw.get("dtype", np.float32))


def _with(s, opts):
    s.set_options(**opts)
    return s


def _fallback_case(case):
    from gpad_mpc import _lib, problems
    import gpad_mpc
    if case == "f64":
        return _battery_case(dtype=np.float64)
    if case == "resident":
        return _battery_case(kernel=_lib.KERNEL_RESIDENT)
    if case == "unshared":
        F = TF.fleet(3, 4)
        return lambda opts: _with(TF.make_solver(F), opts), lambda s: loop(s, F, F.X0, 2, 50, 0.0, False)
    if case == "n300":
        p = synthetic(300, 64, 3, 2, packs=2)
        return lambda opts: _with(make_solver(p, 2), opts), lambda s: loop(s, p, p.X0, 2, 50, 0.0, False)
    if case == "flat":
        qp, pl = problems.battery_plant(4, 10)
        MGf, GLf, L = problems.flatten_battery(qp, 4, 10)
        p = SimpleNamespace(qp=qp, nx=4, nu=4)

        def make(opts):
            s = gpad_mpc.GpadSolver(0)
            s.setup_flat(F32(MGf), F32(GLf), float(np.float32(L)), n_u=4, batch=20)
            s.setup_plant(F32(pl.PM), F32(pl.Pg), g0=F32(pl.g0), A=F32(pl.A), B=F32(pl.B))
            return _with(s, opts)
        return make, lambda s: loop(s, p, states(p, 20, 7), 2, 50, 0.0, False)
    if case == "hessian":
        p = battery(3, 4)
        H = F32(problems.battery_matrices(3, 4)["H"])
        X0 = states(p, 7, 7)

        def make(opts):
            s = make_solver(p, 7)
            s.setup_hessian(H)
            return _with(s, opts)
        return make, lambda s: loop(s, p, X0, 2, 50, 0.0, False)
    if case == "N55":  # with a tolerance the iteration limit must fall on a test (check_every = 10)
        p = battery(3, 4)
        X0 = states(p, 7, 7)
        return lambda opts: _with(make_solver(p, 7), opts), lambda s: loop(s, p, X0, 2, 55, 1e-4, False)
    assert case == "row65"  # nx + ns = 65
    p = TS.synth(70, 130, 40, 1, 25)
    X0, S = TS.synth_inputs(p, 3)
    return lambda opts: _with(TS.make_solver(p, X0.shape[0]), opts), lambda s: TS.loop(s, p, X0, S, 3, 200, 1e-4, False)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["f64", "unshared", "n300", "flat", "hessian", "resident", "N55", "row65"])
def test_fallbacks(gpu, case):
    make, go = _fallback_case(case)
    ref = go(make({}))
    r = go(make(dict(loop_panel=1)))
    assert r.st["kernel"] == ref.st["kernel"] != NAME
    assert r.st["kernel"] is not None
    assert_same_run(r, ref)


@pytest.mark.gpu
def test_both_options_without_the_panel_path(gpu):
    """loop_panel and loop_async both set, the panel path not applicable: the asynchronous kernel."""
    make, go = _fallback_case("N55")
    r = go(make(dict(loop_panel=1, loop_async=1)))
    assert r.st["kernel"] == "loop"
    assert_same_run(r, go(make({})))


@pytest.mark.gpu
def test_option_range(gpu):
    from gpad_mpc._lib import GpadError
    p = battery(3, 4)
    s = make_solver(p, 1)
    with pytest.raises(GpadError):
        s.set_option("loop_panel", 2)
    s.set_option("loop_panel", 1)
    assert loop(s, p, states(p, 1, 7), 2, 20, 0.0, False).st["kernel"] == NAME
    s.set_option("loop_panel", -1)  # back to the default: lockstep
    assert loop(s, p, states(p, 1, 7), 2, 20, 0.0, False).st["kernel"] not in (NAME, "loop")


@pytest.mark.gpu
def test_nonfinite_state(gpu, oracle):
    """An infinite state poisons its own pack only: N bounded iterations of NaN arithmetic per step,
    the run flagged as the lockstep run is, the other packs untouched, and the run ends."""
    p = battery(3, 4)
    X0 = states(p, 19, 7)
    X0[1, 0] = np.inf
    ref = lockstep("lp34", p, X0, 2, 60, 1e-4, False)
    r = panel_run(p, X0, 2, 60, 1e-4, False, grid=1)
    assert r.st["kernel"] == NAME
    assert r.st["nonfinite_g"] and ref.st["nonfinite_g"]
    assert r.st["below_tol_floor"] == ref.st["below_tol_floor"]
    assert np.array_equal(r.st["tol_floor"], ref.st["tol_floor"], equal_nan=True)
    same_bits(r.it, ref.it, "it")
    same_bits(r.cd, ref.cd, "cd")
    others = [b for b in range(19) if b != 1]
    assert_same_run(r, ref, packs=others)
    Xf = X0.copy()
    Xf[1] = 0.0
    assert_matches_oracle(r, oracle_loop(oracle, "lp34", p, Xf, 2, 60, 1e-4, False), packs=others)


@pytest.mark.gpu
def test_device_tensors_without_stats(gpu):
    """Device memory, stats=False: the loop is only enqueued; sync, then compare with lockstep."""
    import torch
    import gpad_mpc
    p = battery(3, 4)
    qp = p.qp
    batch, steps, N = 37, 6, 2000
    t = lambda a: torch.from_numpy(F32(a)).to(gpu)  # noqa: E731
    X0 = states(p, batch, 7)
    out = []
    for panel in (False, True):
        s = gpad_mpc.GpadSolver(0)
        s.setup(t(qp.ML), t(qp.G), float(np.float32(qp.L)), n=qp.n, m=qp.m, batch=batch)
        s.setup_plant(t(p.PM), t(p.Pg), g0=t(p.g0), A=t(p.A), B=t(p.B))
        if panel:
            s.set_options(loop_panel=1, panel_max_grid=1)
        X = torch.from_numpy(X0).to(gpu)
        Z = torch.zeros(batch, qp.n, device=gpu)
        Y = torch.zeros(batch, qp.m, device=gpu)
        XS = torch.zeros(steps, batch, p.nx, device=gpu)
        US = torch.zeros(steps, batch, p.nu, device=gpu)
        assert s.closed_loop(X, Z, Y, steps, N, 1e-4, xs=XS, us=US, stats=False) is None
        s.sync()
        st = s.last_stats()
        assert (st["kernel"] == NAME) == panel
        out.append(([a.cpu().numpy() for a in (X, Z, Y, XS, US)], st))
    for a, b, k in zip(out[0][0], out[1][0], "x z y xs us".split()):
        same_bits(b, a, k)
    for k in STAT_KEYS + ("tol_floor",):
        assert out[0][1][k] == out[1][1][k], k


@pytest.mark.gpu
def test_handle_reuse(gpu):
    """The panel loop twice, the option off, on again on one handle: four identical results (the
    queue counter and the status words are reset per run)."""
    p = battery(3, 4)
    X0 = states(p, 37, 7)
    s = make_solver(p, 37)
    s.set_options(loop_panel=1, panel_max_grid=1)
    runs = [loop(s, p, X0, 6, 2000, 1e-4, False) for _ in range(2)]
    s.set_option("loop_panel", 0)
    runs.append(loop(s, p, X0, 6, 2000, 1e-4, False))
    s.set_option("loop_panel", 1)
    runs.append(loop(s, p, X0, 6, 2000, 1e-4, False))
    assert [r.st["kernel"] == NAME for r in runs] == [True, True, False, True]
    for r in runs[1:]:
        assert_same_run(r, runs[0])
