"""The one-launch closed loops at every row bucket and tile count: the asynchronous loop kernels
(GPAD_OPT_LOOP_ASYNC, csrc/gpad_loop_kernels.inc) and the panel loops (GPAD_OPT_LOOP_PANEL and the fused class
loop, csrc/gpad_loop_panel.hip), swept over shapes; the state and input sizes nu > nx, nu = 64 and nu = n on
every loop engine.  The contract is the neighbouring files': bit identity with the lockstep loop of the same
handle configuration and with the CPU oracle, pack by pack.  Inputs: tests/loop_shape_cases.py.

Plants: test_loop_async.synthetic(n, m, nx, nu, packs), (nx, nu) = STATE[i % 5] over the shape index i with nu
clipped to n.  Three steps.  Modes of every shape, in one test body: (a) warm, tol 1e-4, N = 1000; (b) cold, tol
1e-4, a second N; (c) cold, fixed N = 30.

What the sweep reaches
  asynchronous loops (18 shapes, 5 packs on duo_max_grid = 2: the two-slot kernels start four packs and claim
  one from the queue, the one-slot fleet kernel claims three):
    gpad_loop_kernel<KA, KB, shared>, gpad_loop_kernel<KA, KB, per-pack plant> and gpad_loop_fleet_kernel<KA, KB>
    at every bucket of KA = res_bucket(m) and every bucket of KB = res_bucket(n) (each of the 16 edge values
    1, 32, 33, ..., 201, 208 once as n and once as m; 208 x 208 is the 512-thread workgroup; 20 x 30 both small),
    and the certificate twin of each (gpad_loop_farkas_kernel, gpad_loop_fleet_farkas_kernel) under a bound that
    cannot fire, in modes (a) and (b).  18 of the 64 bucket pairs per kernel; the other 46 pair row sets that are
    tested here one by one (KA and KB select independent chains) and stay unreached as pairs.
  panel loops (test_infeasible_panels.SHAPES: T = 1..16, 20 shapes, 37 packs on panel_max_grid = 2: three panels,
  the last ragged, so columns refill from the queue):
    gpad_loop_panel_kernel<T, false> (loop_panel) and <T, true> (the fused class loop on two classes of 24 and 13
    packs) at every T, and gpad_loop_panel_farkas_kernel<T, false / true> under a bound that cannot fire in modes
    (a) and (b); per-pack plant maps on loop_panel at T = 1, 8, 13, 16.
    The schedule tables (lp_tab_in_lds<T>(N, nx, nu): 8 (N + 2) <= 32768 and sizeof(LoopPanelLds<T>) + 4 (32 nx +
    16 nu) + 8 (N + 2) <= 163840 / (T <= 8 ? 32 / T : 1), sizeof = 4480 T + 256) per T and mode:

       T   state    (a) N = 1000   (b) N      placement   (c) N = 30   largest N in LDS
       1   (2, 1)   global         4100       global      global       0 (budget 5120 - 4736 - 320 = 64 B)
       1   (5, 2)   global         4100       global      global       0 (the state rows alone pass the budget)
       2   (1, 1)   global         4100       global      LDS          100 (a cold solve needs 120: not reachable)
       3   (64, 1)  global         4100       global      global       0 (the state rows alone pass the budget)
       4   (3, 40)  global         4100       global      global       0 (the state rows alone pass the budget)
       5   (2, 3)   global          520       LDS         LDS          520
       6   (5, 2)   global          600       LDS         LDS          600
       7   (1, 1)   LDS            4100       global      LDS          1140
       8   (64, 1)  global         4100       global      global       0 (the state rows alone pass the budget)
       9 .. 16      LDS            4100       global      LDS          4090 (the 32 KiB cap alone)

    Both placements run through modes (a) and (b) at T = 5, 6, 7 and 9 .. 16; at T = 2 the LDS side runs in mode
    (c) only; at T = 1, 3, 4 and 8 no multiple of check_every reaches LDS with these state sizes
    (test_table_placement_cpu asserts every line).
  state and input sizes on 70 x 130: the five STATE entries on the lockstep loop and gpad_run_state (max(nx, nu)
    and the `i < nu` tail of plant_step_kernel with nu the larger), signals with nu > nx + ns and with nx + ns =
    nu = 64 on the lockstep loop, loop_async and loop_panel (plant_step_sig_kernel), (2, 3) on the f64 loop.
  the closed-loop fuzz draws the engine as well (fuzz_util.draw_loop_case(engines=LOOP_ENGINES)).

What stays unreached: the other 46 bucket pairs of each asynchronous kernel (above); the LDS placement at T = 1, 3,
4, 8 (it needs smaller states than STATE deals those shapes; tests/test_loop_panel.py runs it at T = 4 with
nx = nu = 3); handles bound to another stream.

One input departs from synthetic's defaults: at 40 x 250 the shared plant of 37 packs is drawn from seed 12,
because four of the default's packs need 1000 to 1040 iterations and would stop at the cap (loop_shape_cases
SHARED_SEED).  Checked on the CPU oracle (the *_cpu tests assert it): no solve of modes (a) and (b) reaches N in
any binding (0 of 11388 solves; counts 10 .. 970), every output is finite, and every shape with m > 1 has a step
whose packs stop at two or more different counts in mode (a); in mode (b) the five cold packs of 161 x 32 all stop
at 70 on the shared plant and on the per-pack plants (asserted as the only flat cases).

Measured on an MI355X: the 115 GPU cases of this file take 17 s together, the CPU oracle's loops included; the
slowest, the panel sweep at 241 x 250, takes 1.6 s.  A kernel trace of the three sweeps shows 172 distinct loop
kernels launched: the 18 bucket pairs of gpad_loop_kernel<KA, KB, 0>, <KA, KB, 1> and gpad_loop_fleet_kernel<KA, KB>
and of their three certificate twins (108), and gpad_loop_panel_kernel<T, false / true> and its certificate twin
at T = 1 .. 16 (64).
"""
from __future__ import annotations

import json

import numpy as np
import pytest

import fuzz_util
import loop_ref64 as R64
import loop_shape_cases as C
import test_class_loop as TC
import test_classes as TK
import test_fleet as TF
import test_loop_async as T
import test_loop_f64 as T64
import test_loop_panel as TP
import test_signals as TS
from test_loop_async import F32, assert_matches_oracle, assert_same_run, same_bits

ASYNC_IDS = ["%dx%d" % s for s in C.ASYNC_SHAPES]
PANEL_IDS = ["T%d-%dx%d" % s for s in C.PANEL_SHAPES]
BINDINGS = ("shared", "plants", "fleet")
WIDE = (70, 130)  # the shape of the state-size cases: two -ML waves, three G/L waves with the last ragged
FLAT_COLD = {("shared", 161, 32), ("plants", 161, 32)}  # mode (b): every pack stops at the same count


# ------------------------------------------------------------------------------ inputs
def async_binding(binding, shape):
    n, m = shape
    nx, nu = C.state_of(C.async_index(shape), n)
    make = {"shared": C.shared_plant, "plants": C.per_pack_plants, "fleet": C.fleet}[binding]
    return make(n, m, nx, nu, C.ASYNC_PACKS)


def panel_state(shape):
    return C.state_of(C.panel_index(shape), shape[1])


def panel_plant(shape):
    _, n, m = shape
    return C.shared_plant(n, m, *panel_state(shape), C.PANEL_PACKS)


def panel_classes(shape):
    _, n, m = shape
    return C.class_input(n, m, *panel_state(shape))


def panel_per_pack(shape):
    _, n, m = shape
    return C.per_pack_plants(n, m, *panel_state(shape), C.PANEL_PACKS)


PLANT_SHAPES = [next(s for s in C.PANEL_SHAPES if s[0] == t) for t in C.PLANT_TILES]


def distinct(orc):
    return max(len(set(row)) for row in orc.it.tolist())


def check_conditions(oracle, key, F, modes, m, flat_cold=False):
    """Modes (a) and (b) of an input on the oracle alone: loop_shape_cases.assert_conditions, and the raggedness
    rule of the module docstring."""
    for name in ("a", "b"):
        cfg = C.cfg_of(modes[name])
        orc = C.oracle_run(oracle, key, F, cfg)
        C.assert_conditions(orc, cfg, m)
        if m > 1 and name == "a":
            assert distinct(orc) >= 2, (key, orc.it.tolist())
        if m > 1 and name == "b":
            assert (distinct(orc) == 1) == flat_cold, (key, orc.it.tolist())
    cfg = C.cfg_of(modes["c"])
    C.assert_conditions(C.oracle_run(oracle, key, F, cfg), cfg, m)


# ------------------------------------------------------------------------------ CPU: the lists
def test_shape_lists_cpu():
    """Every edge value once as n and once as m, every bucket of KA and of KB, the corners; T = 1..16 as
    (max(n, m) + 15) // 16 gives it; the state sizes the sweep is about occur."""
    head = C.ASYNC_SHAPES[:16]
    assert sorted(n for n, _ in head) == C.EDGES == sorted(m for _, m in head)
    assert C.ASYNC_SHAPES[16:] == [(208, 208), (20, 30)] and len(set(C.ASYNC_SHAPES)) == 18
    assert sorted({C.res_bucket(m) for _, m in C.ASYNC_SHAPES}) == C.BUCKETS  # KA
    assert sorted({C.res_bucket(n) for n, _ in C.ASYNC_SHAPES}) == C.BUCKETS  # KB
    assert [C.res_bucket(v) for v in (1, 32, 33, 192, 193, 200, 201, 208)] == [32, 32, 64, 192, 200, 200, 208, 208]
    for n, m in C.ASYNC_SHAPES:  # resident_supported: at most 8 waves of rows up to 208
        assert max(n, m) <= 208 and (n + 63) // 64 + (m + 63) // 64 <= 8
    assert (208 + 63) // 64 * 2 * 64 == 512
    assert len(C.PANEL_SHAPES) == 20
    assert all(t == (max(n, m) + 15) // 16 for t, n, m in C.PANEL_SHAPES)
    assert sorted({t for t, _, _ in C.PANEL_SHAPES}) == list(range(1, 17))
    assert sorted(s[0] for s in PLANT_SHAPES) == [1, 8, 13, 16]
    for shapes, states in ((C.ASYNC_SHAPES, [C.state_of(i, s[0]) for i, s in enumerate(C.ASYNC_SHAPES)]),
                           ([s[1:] for s in C.PANEL_SHAPES], [panel_state(s) for s in C.PANEL_SHAPES])):
        assert any(nu > nx for nx, nu in states) and any(nu == 64 for _, nu in states)
        assert any(nx == 64 for nx, _ in states) and any((nx, nu) == (1, 1) for nx, nu in states)
        assert all(1 <= nu <= min(64, n) for (n, _), (_, nu) in zip(shapes, states))
    assert [panel_state(s)[1] == s[1] for s in C.PANEL_SHAPES if s[1:] in ((40, 64), (40, 250))] == [True, True]  # nu = n
    assert int(C.CLASS_OF.sum()) == 13 and C.CLASS_OF.size == 37


def test_table_placement_cpu(oracle):
    """The table of the module docstring, line by line, from the rule restated in loop_shape_cases.tab_in_lds."""
    assert [C.lp_static_lds(t) for t in (1, 2, 9, 16)] == [4736, 9216, 40576, 71936]  # sizeof, from a host compile
    both = set()
    for shape in C.PANEL_SHAPES:
        t, n, m = shape
        nx, nu = panel_state(shape)
        modes = C.panel_modes(t)
        place = {k: C.tab_in_lds(t, modes[k][2], nx, nu) for k in "abc"}
        top = C.largest_lds_n(t, nx, nu)
        assert all(modes[k][2] % 10 == 0 for k in "abc")
        assert not C.tab_in_lds(t, C.N_PAST, nx, nu)
        if t in (1, 3, 4, 8):
            assert top == 0 and not any(place.values())
        elif t == 2:
            assert top == 100 and place == dict(a=False, b=False, c=True)
            cold = C.oracle_run(oracle, ("panel-shared", n, m), panel_plant(shape), (C.STEPS, C.N_PAST, C.TOL, False))
            assert cold.it.max() >= top  # N = 100 would cap a cold solve: the LDS side is out of mode (b)'s reach
        elif t in (5, 6):
            assert top == modes["b"][2] == C.PANEL_N_LDS[t] and place == dict(a=False, b=True, c=True)
        else:
            assert place == dict(a=True, b=False, c=True) and top == (1140 if t == 7 else 4090)
        if place["a"] != place["b"]:
            both.add(t)
    assert sorted(both) == [5, 6, 7] + list(range(9, 17))


# ------------------------------------------------------------------------------ CPU: the conditions
@pytest.mark.parametrize("shape", C.ASYNC_SHAPES, ids=ASYNC_IDS)
def test_async_conditions_cpu(oracle, shape):
    """The three bindings of an async shape meet the conditions of the module docstring (the seeds of the
    per-pack plants and of the fleets were chosen here)."""
    n, m = shape
    for binding in BINDINGS:
        check_conditions(oracle, ("async-" + binding, n, m), async_binding(binding, shape), C.ASYNC_MODES, m,
                         (binding, n, m) in FLAT_COLD)


@pytest.mark.parametrize("shape", C.PANEL_SHAPES, ids=PANEL_IDS)
def test_panel_conditions_cpu(oracle, shape):
    """The same for the 37 packs of a panel shape: the shared plant, the two classes (their seed was chosen here)
    and, at T = 1, 8, 13, 16, the per-pack plants."""
    t, n, m = shape
    modes = C.panel_modes(t)
    check_conditions(oracle, ("panel-shared", n, m), panel_plant(shape), modes, m)
    check_conditions(oracle, ("panel-classes", n, m), panel_classes(shape).E, modes, m)
    if shape in PLANT_SHAPES:
        check_conditions(oracle, ("panel-plants", n, m), panel_per_pack(shape), modes, m)


def test_classes_differ_cpu(oracle):
    """The two classes of a shape are distinct problems: a pack run on the other class's matrices and maps gives
    other us bits, so a wrong class index cannot pass the fused sweep."""
    shape = (9, 130, 137)
    I = panel_classes(shape)
    cfg = C.cfg_of(C.panel_modes(9)["b"])
    own = C.oracle_run(oracle, ("panel-classes", 130, 137), I.E, cfg)
    for b in (0, 1):  # class 1, class 0
        j = int(np.flatnonzero(I.class_of != I.class_of[b])[0])
        other = TF.oracle_pack(oracle, TF.pack(I.E, b, matrices=j, maps=j), *cfg)
        assert other[4].tobytes() != own.us[:, b].tobytes(), b
    assert len({I.E.PM[b].tobytes() for b in range(37)}) == 2


def test_threaded_oracle_is_the_serial_one_cpu(oracle):
    """loop_shape_cases.oracle_run (a thread pool over test_fleet.oracle_pack) returns what
    test_loop_async.oracle_loop returns."""
    p = async_binding("shared", (20, 30))
    for name in "abc":
        cfg = C.cfg_of(C.ASYNC_MODES[name])
        a = C.oracle_run(oracle, ("async-shared", 20, 30), p, cfg)
        b = T.oracle_loop(oracle, "shapes-20x30", p, p.X0, *cfg)
        for k in ("x", "z", "y", "xs", "us", "it"):
            same_bits(getattr(a, k), getattr(b, k), k)


# ------------------------------------------------------------------------------ CPU: the oracle on the new sizes
def wide_plant(state):
    nx, nu = state
    return T.synthetic(*WIDE, nx, nu)


def oracle_deviation(oracle, state):
    """The largest norm-relative deviation, over the packs and over xs, us, x, z, of the f32 oracle's closed loop
    from loop_ref64 on the same f32-rounded data (mode (c): cold, three steps of 30 iterations)."""
    p = wide_plant(state)
    cfg = C.cfg_of(C.ASYNC_MODES["c"])
    o = C.oracle_run(oracle, ("wide",) + tuple(state), p, cfg)
    pk = R64.make_pack(F32(p.qp.ML), F32(p.qp.G), float(np.float32(p.qp.L)), F32(p.PM), F32(p.Pg), F32(p.M0), F32(p.g0),
                       F32(p.A), F32(p.B))
    steps, N, tol, warm = cfg
    r = R64.fleet_loop([pk] * p.X0.shape[0], p.X0.astype(np.float64), None, steps, N, tol, warm)
    assert (r.it == N).all() and (o.it == N).all()
    rel = lambda a, b: float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b))  # noqa: E731
    packs = range(p.X0.shape[0])
    return max([rel(getattr(o, k)[b], getattr(r, k)[b]) for k in ("x", "z") for b in packs]
               + [rel(getattr(o, k)[:, b], getattr(r, k)[:, b]) for k in ("xs", "us") for b in packs])


ORACLE_DEV_MEASURED = 1.87e-6
ORACLE_DEV_BAR = 4 * ORACLE_DEV_MEASURED


def test_oracle_against_fp64_cpu(oracle):
    """A guard for the oracle itself at the new state sizes: on 70 x 130, mode (c), its f32 xs, us, x and z agree
    with tests/loop_ref64.py (fp64, the same f32-rounded data; the counts are equal by construction) for the five
    STATE entries.  Measured on the CPU, the largest norm-relative deviation per pack and array: 2.9e-7 for
    (2, 3), 4.5e-7 for (5, 2), 1.9e-6 for (1, 1), 1.5e-6 for (64, 1), 6.6e-7 for (3, 64); the largest is 1.87e-6.
    The bar is four times that, 7.48e-6: f32 accumulation over the 90 iterations varies by about that factor
    between seeds.  (A u read one entry late or a dropped constant term moves these loops by 0.1 to 1.)"""
    devs = {s: oracle_deviation(oracle, s) for s in C.STATE}
    print("f32 oracle against loop_ref64, norm-relative:", {s: "%.3g" % d for s, d in devs.items()})
    assert max(devs.values()) <= ORACLE_DEV_BAR, devs


# ------------------------------------------------------------------------------ CPU: signals, f64, fuzz
SIGNAL_SIZES = {"nu-gt-nxa": (2, 7, 3), "row64-u64": (40, 64, 24)}  # (nx, nu, ns)
SIG_N = 1000


def signal_case(name):
    nx, nu, ns = SIGNAL_SIZES[name]
    p = TS.synth(*WIDE, nx, nu, ns)
    X0, S = TS.synth_inputs(p, C.STEPS)
    return p, X0, S


@pytest.mark.parametrize("name", list(SIGNAL_SIZES))
def test_signal_inputs_cpu(oracle, name):
    """nu > nx + ns resp. nx + ns = nu = 64 within the loop kernels' bounds; the oracle's loops are finite and end
    below N, cold and warm, with ragged counts."""
    p, X0, S = signal_case(name)
    assert p.nu > p.nx + p.ns or (p.nx + p.ns == 64 == p.nu)
    assert p.nx + p.ns <= 64 and p.nu <= min(64, p.qp.n)
    for warm in (False, True):
        orc = TS.oracle_loop(oracle, "shapes-" + name, p, X0, S, C.STEPS, SIG_N, C.TOL, warm)
        assert all(np.isfinite(getattr(orc, k)).all() for k in ("x", "z", "y", "xs", "us"))
        assert orc.it.max() < SIG_N and distinct(orc) >= 2


F64_RUNS = [(False, T64.TOL), (True, T64.TOL), (False, 0.0)]
F64_IDS = ["cold-tol", "warm-tol", "cold-fixed"]


@pytest.mark.parametrize("warm,tol", F64_RUNS, ids=F64_IDS)
def test_f64_config_cpu(warm, tol):
    """test_loop_f64's conditions on its reference for configuration B23 (nu = 3 > nx = 2), as
    test_loop_f64.test_counts_are_robust asks them of every run it compares: finite, the counts and codes
    unchanged by a 1e-9 perturbation of every step's state and by numpy dot products, every solve below N."""
    c = T64.config("B23")
    assert (c.nx, c.nu, c.n, c.m) == (2, 3) + WIDE
    r = T64.reference(c, warm, tol)
    p = T64.reference(c, warm, tol, perturb=np.random.default_rng(1))
    d = T64.reference(c, warm, tol, dot=True)
    assert all(np.isfinite(getattr(r, k)).all() for k in ("x", "z", "y", "xs", "us"))
    for other in (p, d):
        np.testing.assert_array_equal(other.it, r.it)
        np.testing.assert_array_equal(other.cd, r.cd)
        assert T64.deviation(other, r) <= 1e-8
    if tol:
        assert r.it.max() < T64.NTOL and (r.cd > 0).all()
    else:
        assert (r.it == T64.NFIX).all() and (r.cd == 0).all()
    # the wrong variant this configuration exists to catch: u taken one entry late
    bad = T64.reference(c, warm, tol, tag="u-shifted", u_offset=1)
    assert T64.deviation(bad, r) > 1e-6


FUZZ_SEED, FUZZ_CASES = 20261018 + 600, 9


def fuzz_case(i):
    return fuzz_util.draw_loop_case(np.random.default_rng(FUZZ_SEED + i), fuzz_util.LOOP_ENGINES)


def fuzz_engine(cfg):
    """The kernel a fuzz case must report (csrc/gpad_state.cpp one_launch_engine; None: a lockstep engine)."""
    qn, qm = cfg["n_u"] * cfg["Nh"], 4 * cfg["n_u"] * cfg["Nh"] + 2 * cfg["Nh"]
    if cfg["engine"] == "loop_panel" and cfg["kernel"] in ("auto", "panel") and (not cfg["tol"] or cfg["N"] % 10 == 0):
        return "loop_panel"
    if (cfg["engine"] == "loop_async" and cfg["kernel"] in ("auto", "resident") and max(qn, qm) <= 208
            and (qn + 63) // 64 + (qm + 63) // 64 <= 8):
        return "loop"
    return None


def test_fuzz_draws_cpu():
    """The engine is drawn after everything else: the recorded lockstep cases of tests/test_fuzz.py are what they
    were (the same fields from the same seeds, engine lockstep), and the cases drawn here hold all three engines
    and both one-launch kernels."""
    import test_fuzz
    for i in range(50):
        old = fuzz_util.draw_loop_case(np.random.default_rng(test_fuzz.SEED + 300 + i))
        new = fuzz_util.draw_loop_case(np.random.default_rng(test_fuzz.SEED + 300 + i), fuzz_util.LOOP_ENGINES)
        assert old.pop("engine") == "lockstep" and new.pop("engine") in fuzz_util.LOOP_ENGINES
        assert json.dumps(old) == json.dumps(new)
    cases = [fuzz_case(i) for i in range(FUZZ_CASES)]
    assert {c["engine"] for c in cases} == set(fuzz_util.LOOP_ENGINES)
    assert {"loop", "loop_panel"} <= {fuzz_engine(c) for c in cases}


# ------------------------------------------------------------------------------ GPU: the asynchronous loops
def check_run(r, ref, orc, kernel):
    assert r.st["kernel"] == kernel, r.st["kernel"]
    assert_same_run(r, ref)
    assert_matches_oracle(r, orc)
    assert_matches_oracle(ref, orc)
    assert r.st["total_iterations"] == int(orc.it.sum())


def check_never_fires(on, r, kernel):
    """The run with the bound that cannot fire: the certificate twin, the same bits, no code 5."""
    assert on.st["kernel"] == kernel, on.st["kernel"]
    assert_same_run(on, r)
    assert 5 not in on.cd and (on.cd > 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("binding", BINDINGS)
@pytest.mark.parametrize("shape", C.ASYNC_SHAPES, ids=ASYNC_IDS)
def test_async_sweep(gpu, oracle, shape, binding):
    """loop_async == the lockstep loop of the same binding == the oracle, in the three modes; then modes (a) and
    (b) on the certificate twin under R_NEVER."""
    n, m = shape
    F = async_binding(binding, shape)
    key = ("async-" + binding, n, m)
    for name in "abc":
        cfg = C.cfg_of(C.ASYNC_MODES[name])
        orc = C.oracle_run(oracle, key, F, cfg)
        if binding == "shared":
            ref = T.lockstep(key, F, F.X0, *cfg)
            r = T.run(F, F.X0, *cfg, async_=True, grid=C.ASYNC_GRID)
            make = lambda: T.make_solver(F, C.ASYNC_PACKS)  # noqa: E731
        else:
            ref = TF.lockstep_fleet(key, F, *cfg)
            r = TF.run(F, *cfg, async_=True, grid=C.ASYNC_GRID)
            make = lambda: TF.make_solver(F)  # noqa: E731
        check_run(r, ref, orc, "loop")
        if name == "c":
            assert (r.it == C.N_FIXED).all() and (r.cd == 0).all()
            continue
        with make() as s:
            s.set_infeasibility_loop_async(True)
            s.set_options(loop_async=1, duo_max_grid=C.ASYNC_GRID)
            s.setup_infeasibility(C.R_NEVER)
            check_never_fires(T.loop(s, F, F.X0, *cfg), r, "loop")


# ------------------------------------------------------------------------------ GPU: the panel loops
@pytest.mark.gpu
@pytest.mark.parametrize("shape", C.PANEL_SHAPES, ids=PANEL_IDS)
def test_panel_sweep(gpu, oracle, shape):
    """loop_panel on the shared plant (and, at T = 1, 8, 13, 16, on per-pack plant maps) == the lockstep loop == the
    oracle in the three modes -- both table placements where the docstring's table has them -- then modes (a) and
    (b) on gpad_loop_panel_farkas_kernel<T> under R_NEVER."""
    t, n, m = shape
    inputs = [("panel-shared", panel_plant(shape))]
    if shape in PLANT_SHAPES:
        inputs.append(("panel-plants", panel_per_pack(shape)))
    for kind, F in inputs:
        key = (kind, n, m)
        make = (lambda: TF.make_solver(F)) if kind == "panel-plants" else (lambda: T.make_solver(F, C.PANEL_PACKS))
        for name, mode in C.panel_modes(t).items():
            cfg = C.cfg_of(mode)
            orc = C.oracle_run(oracle, key, F, cfg)
            ref = TF.lockstep_fleet(key, F, *cfg) if kind == "panel-plants" else T.lockstep(key, F, F.X0, *cfg)
            assert ref.st["kernel"] != TP.NAME
            with make() as s:
                s.set_options(loop_panel=1, panel_max_grid=C.PANEL_GRID)
                r = T.loop(s, F, F.X0, *cfg)
                check_run(r, ref, orc, TP.NAME)
                if name == "c":
                    assert (r.it == C.N_FIXED).all() and (r.cd == 0).all()
                    continue
                s.setup_infeasibility(C.R_NEVER)
                check_never_fires(T.loop(s, F, F.X0, *cfg), r, TP.NAME)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", C.PANEL_SHAPES, ids=PANEL_IDS)
def test_fused_class_sweep(gpu, oracle, shape):
    """The fused class loop on two classes of distinct matrices and maps (24 and 13 packs, interleaved) == the
    class binding's lockstep loop == the oracle, pack by pack on that pack's class; then the certificate twin."""
    t, n, m = shape
    I = panel_classes(shape)
    for name, mode in C.panel_modes(t).items():
        cfg = C.cfg_of(mode)
        orc = C.oracle_run(oracle, ("panel-classes", n, m), I.E, cfg)
        plain = TK.class_plain(I, cfg)
        assert plain.st["kernel"] not in (None, TC.FUSED, TP.NAME, "loop")
        with TC.fused_solver(I, panel_max_grid=C.PANEL_GRID) as s:
            r = T.loop(s, I.C, I.X0, *cfg)
            check_run(r, plain, orc, TC.FUSED)
            if name == "c":
                assert (r.it == C.N_FIXED).all() and (r.cd == 0).all()
                continue
            s.setup_infeasibility(C.R_NEVER)
            check_never_fires(T.loop(s, I.C, I.X0, *cfg), r, TC.FUSED)


# ------------------------------------------------------------------------------ GPU: state and input sizes
@pytest.mark.gpu
@pytest.mark.parametrize("state", C.STATE, ids=["nx%d-nu%d" % s for s in C.STATE])
def test_state_sizes_lockstep(gpu, oracle, state):
    """The five state sizes on 70 x 130 through the lockstep loop (affine2_kernel, plant_step_kernel with
    per = max(nx, nu)) and gpad_run_state, against the oracle."""
    p = wide_plant(state)
    key = ("wide",) + tuple(state)
    for name in "abc":
        cfg = C.cfg_of(C.ASYNC_MODES[name])
        orc = C.oracle_run(oracle, key, p, cfg)
        C.assert_conditions(orc, cfg, WIDE[1])
        r = T.lockstep(key, p, p.X0, *cfg)
        assert_matches_oracle(r, orc)
        assert r.st["total_iterations"] == int(orc.it.sum())
    # gpad_run_state: one solve from z = y = 0 at X0 -- step 0 of the cold loop
    one = C.oracle_run(oracle, key, p, (1, C.N_WARM, C.TOL, False))
    batch = p.X0.shape[0]
    with T.make_solver(p, batch) as s:
        Z, Y = np.zeros((batch, WIDE[0]), np.float32), np.zeros((batch, WIDE[1]), np.float32)
        st = s.run_state(p.X0.copy(), Z, Y, C.N_WARM, C.TOL)
    same_bits(Z, one.z, "z")
    same_bits(Y, one.y, "y")
    assert st["total_iterations"] == int(one.it.sum()) and st["iterations"] == int(one.it.max())


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("name", list(SIGNAL_SIZES))
def test_signal_sizes(gpu, oracle, name, warm):
    """Signals with nu > nx + ns and with nx + ns = nu = 64, compared as tests/test_signals.py compares them: the
    lockstep loop with the augmented handle and the oracle, loop_async and loop_panel with the lockstep loop."""
    p, X0, S = signal_case(name)
    cfg = (C.STEPS, SIG_N, C.TOL, warm)
    key = "shapes-" + name
    ref = TS.lockstep(key, p, X0, S, *cfg)
    assert_same_run(ref, TS.augmented_handle(key, p, X0, S, *cfg))
    TS.assert_matches_oracle(ref, TS.oracle_loop(oracle, key, p, X0, S, *cfg))
    r = TS.run(p, X0, S, *cfg, async_=True, grid=2)
    assert r.st["kernel"] == "loop"
    assert_same_run(r, ref)
    r = TP.signals_run(p, X0, S, *cfg)
    assert r.st["kernel"] == TP.NAME
    assert_same_run(r, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("warm,tol", F64_RUNS, ids=F64_IDS)
def test_f64_nu_above_nx(gpu, warm, tol):
    """(nx, nu) = (2, 3) on the f64 loop against loop_ref64, by test_loop_f64's own bars."""
    T64.check("B23", warm, tol, "stream")


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(FUZZ_CASES))
def test_loop_fuzz_engines(gpu, oracle, i):
    cfg = fuzz_case(i)
    r = fuzz_util.run_loop_case(cfg, oracle)
    assert r["ok"], f"{json.dumps(cfg)}: {r['why']}"
    want = fuzz_engine(cfg)
    assert (r["kernels"][0] == want) if want else (r["kernels"][0] not in (None, "loop", "loop_panel")), (cfg, r["kernels"])
