"""Class fleets with exogenous signals (gpad_setup_class_signals; csrc/gpad_classes.cpp, the S gather of
csrc/gpad_classes.hip and the class-aware panel loop of csrc/gpad_loop_panel.hip with ns > 0).

The contract is bit identity with code that predates the feature: a class-bound handle with class signals
equals (a) the dims.shared = 0 handle of the expanded fleet (problems.expand_classes) bound with a stacked
setup_plant + setup_signals, instance b holding the copies of class class_of[b], and (b) the CPU oracle's
closed loop of every pack on the augmented state (test_signals.oracle_loop, class by class with the class's
matrices and maps).  The fused class loop and the forwarded one-launch loops are also compared with the
class handle with everything off.  x, z, y, xs, us, counts, codes, aggregate stats, tol_floor and flags are
compared; references are computed once per input and mode and shared.

Inputs: class k's plant is battery_plant_signals(n_u, Nh, capacity_ah=caps[k]) with caps and class_of those
of the base input; from rng = default_rng(seed): X0 = a (rng.random((B, n_u)) - 0.5), loads
rng.uniform(-I, I, (steps, B)), references rng.uniform(-0.1, 0.1, (steps, B, n_u)), S = [load, ref], f32.
  SA   test_classes A  (11 packs in classes of 4 / 2 / 5, n = 12, m = 56), seed 211, 6 steps, HARD, N 2000
  SA4  A4 (SA with an empty class)
  SB   B (5 packs in classes of 2 / 3, n = 40, m = 180), seed 212, 4 steps, MILD, N 3000
  SP   P (40 packs in classes of 24 / 16, dims.kernel = PANEL), seed 213, 6 steps, HARD, N 2000
  SQ   test_class_loop Q (33 packs in classes of 17 / 15 / 1), seed 214, 6 steps, HARD, N 2000
HARD: a = 0.9, I = 12; MILD: a = 0.6, I = 7.  Fixed-N mode: N = 100.  test_oracle_guard asserts on the oracle
what these inputs must show (ragged counts, capped next to early solves, every fault visible).

The battery plants bind no M0, so SA also runs with a per-class M0 (m0_input: test_class_loop.class_m0 at scale
0.5) -- through the per-class plant, and through one plant under per-class signals, where M0, g0, B are
replicated beside the packed images.  test_m0_oracle_guard, on the oracle at eps 1e-4, cold / warm: M0 changes the
us bits of 11 of 11 packs, so does M0 rolled by one class; the one-plant variant differs in exactly the 7 packs
outside class 0; 6 to 8 / 6 to 7 distinct counts per step; 3 of the 66 solves capped.
"""
from __future__ import annotations

import ctypes as C
import functools
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import test_signals as TS
from conftest import ROOT
from test_class_loop import FUSED, M0_MODE_IDS, M0_MODES, assert_m0_guard, class_m0, input_q
from test_classes import MODE_IDS, MODES, _L, class_solver, inputs as base_inputs
from test_loop_async import F32, F64, assert_same_run, same_bits
from test_signals import HARD, MILD

SIG_MAPS = ("SM", "Sg", "E")
ALL_MAPS = ("PM", "Pg", "M0", "g0", "A", "B") + SIG_MAPS
#        base input, seed, steps, set, N with a tolerance
SPECS = dict(SA=("A", 211, 6, HARD, 2000), SA4=("A4", 211, 6, HARD, 2000), SB=("B", 212, 4, MILD, 3000),
             SP=("P", 213, 6, HARD, 2000), SQ=("Q", 214, 6, HARD, 2000))


# ------------------------------------------------------------------------------ inputs
def _ns(qp, pl):
    return SimpleNamespace(qp=qp, nx=pl.nx, nu=pl.nu, ns=pl.ns, **{k: getattr(pl, k) for k in ALL_MAPS})


def _signals(seed, B, n_u, steps, a, I, R):
    rng = np.random.default_rng(seed)
    X0 = a * (rng.random((B, n_u)) - 0.5)
    load = rng.uniform(-I, I, (steps, B))
    ref = rng.uniform(-R, R, (steps, B, n_u))
    S = np.concatenate([load[..., None], ref], axis=-1)
    return X0.astype(np.float32), np.ascontiguousarray(S.astype(np.float32))


@functools.lru_cache(maxsize=None)
def sig_input(name):
    """C: the per-class stacks (what the class binding takes); E: the expanded fleet (the references)."""
    from gpad_mpc import _lib, problems
    base, seed, steps, kw, Ntol = SPECS[name]
    J = input_q() if base == "Q" else base_inputs(base)
    meta = J.C.qp.meta
    qp, pl = problems.battery_fleet_signals(meta["n_u"], meta["N"], meta["caps"])
    eq, ep = problems.expand_classes(qp, pl, J.class_of)
    X0, S = _signals(seed, J.class_of.size, meta["n_u"], steps, **kw)
    return SimpleNamespace(name=name, K=J.K, class_of=J.class_of, X0=X0, S=S, C=_ns(qp, pl), E=_ns(eq, ep),
                           steps=steps, Ntol=Ntol, kernel=_lib.KERNEL_PANEL if base == "P" else None)


def with_maps(I, tag, **maps):
    """Input I with other per-class maps (C) and the fleet expanded from them (E); tag: its name in the caches."""
    J = SimpleNamespace(**vars(I))
    J.C = SimpleNamespace(**dict(vars(I.C), **maps))
    J.C.ns = next(m.shape[-1] for m in (J.C.SM, J.C.Sg, J.C.E) if m is not None)
    take = lambda a: None if a is None else np.ascontiguousarray(a[I.class_of])  # noqa: E731
    J.E = SimpleNamespace(**dict(vars(I.E), ns=J.C.ns, **{k: take(v) for k, v in maps.items()}))
    J.name = I.name + "-" + tag
    return J


def reorder(I, order):
    """Input I with its packs in another order (class_of, X0 and S permuted together)."""
    order = np.asarray(order)
    J = SimpleNamespace(**vars(I))
    J.class_of = np.ascontiguousarray(I.class_of[order])
    J.X0 = np.ascontiguousarray(I.X0[order])
    J.S = np.ascontiguousarray(I.S[:, order])
    J.E = None
    return J


def mode(I, warm, tol):
    return I.steps, (I.Ntol if tol else 100), tol, warm


# ------------------------------------------------------------------------------ handles and runs
def _conv(dtype):
    return F64 if dtype == np.float64 else F32


def bind_signals(s, F, c=F32, to=lambda a: a, per_class=True):
    """Class signals from the stacks of F: a copy per class, or class 0's copy for every class."""
    pick = lambda a: None if a is None else to(c(a if per_class else a[0]))  # noqa: E731
    s.setup_class_signals(pick(F.SM), pick(F.Sg), pick(F.E), ns=F.ns)


def sig_solver(I, *, dtype=np.float32, to=lambda a: a, fused=False, per_class=True, **options):
    s = class_solver(I, dtype=dtype, kernel=I.kernel, to=to, **options)
    bind_signals(s, I.C, _conv(dtype), to, per_class)
    if fused:
        s.set_class_loop_fused(True)
    return s


def sig_loop(s, I, cfg, dtype=np.float32):
    steps, N, tol, warm = cfg
    return TS.loop(s, I.C, I.X0, I.S[:steps], steps, N, tol, warm, dtype)


def sig_run(I, cfg, dtype=np.float32, **kw):
    return sig_loop(sig_solver(I, dtype=dtype, **kw), I, cfg, dtype)


def fleet_solver(I, dtype=np.float32):
    """The reference: dims.shared = 0, stacked plant and signal maps, options off."""
    return TS.make_solver(I.E, I.X0.shape[0], dtype=dtype, shared=False)


_cache = {}


def cached(kind, I, cfg, make):
    k = (kind, I.name) + tuple(cfg)
    if k not in _cache:
        _cache[k] = make()
    return _cache[k]


def class_plain(I, cfg):
    """The class handle with class signals and everything else off, once per input and mode."""
    return cached("classes", I, cfg, lambda: sig_run(I, cfg))


def fleet_ref(I, cfg, dtype=np.float32):
    return cached("fleet" + np.dtype(dtype).name, I, cfg, lambda: sig_loop(fleet_solver(I, dtype), I, cfg, dtype))


def class_plant(I, k, maps_from=None):
    """Class k as a one-plant problem of test_signals' shape (the fleet's L); maps_from: the signal maps of
    another class (the guard)."""
    F = I.C
    j = k if maps_from is None else maps_from
    qp = SimpleNamespace(ML=F.qp.ML[k], G=F.qp.G[k], L=F.qp.L, n=F.qp.n, m=F.qp.m)
    one = {m: None if getattr(F, m) is None else getattr(F, m)[j if m in SIG_MAPS else k] for m in ALL_MAPS}
    return SimpleNamespace(qp=qp, nx=F.nx, nu=F.nu, ns=F.ns, **one)


def oracle_ref(oracle, I, cfg, fault=None):
    """The CPU oracle, class by class, placed in the caller's order.  fault: a WRONG implementation for the
    guard -- "maps" (the signal maps of the next non-empty class), "rows" (S left unpermuted: the pack at
    sorted position p reads the caller's row p), "zero" (S dropped)."""
    steps, N, tol, warm = cfg

    def make():
        B = I.X0.shape[0]
        S = I.S[:steps]
        if fault == "rows":
            S = np.empty_like(S)
            S[:, np.argsort(I.class_of, kind="stable")] = I.S[:steps]
        F = I.C
        o = SimpleNamespace(x=np.zeros((B, F.nx), np.float32), z=np.zeros((B, F.qp.n), np.float32),
                            y=np.zeros((B, F.qp.m), np.float32), xs=np.zeros((steps, B, F.nx), np.float32),
                            us=np.zeros((steps, B, F.nu), np.float32), it=np.zeros((steps, B), np.int32))
        present = [k for k in range(I.K) if (I.class_of == k).any()]
        for i, k in enumerate(present):
            idx = np.flatnonzero(I.class_of == k)
            other = present[(i + 1) % len(present)] if fault == "maps" else None
            r = TS.oracle_loop(oracle, (I.name, k, fault), class_plant(I, k, other), I.X0[idx],
                               np.ascontiguousarray(S[:, idx]), steps, N, tol, warm,
                               variant="zero" if fault == "zero" else None)
            for key in ("x", "z", "y"):
                getattr(o, key)[idx] = getattr(r, key)
            for key in ("xs", "us", "it"):
                getattr(o, key)[:, idx] = getattr(r, key)
        return o
    return cached("oracle" + str(fault), I, cfg, make)


def check_against_references(oracle, I, cfg, r):
    """r == the shared = 0 fleet (outputs, counts, codes, stats, tol_floor, flags) == the oracle."""
    steps, N, tol, warm = cfg
    ref = fleet_ref(I, cfg)
    orc = oracle_ref(oracle, I, cfg)
    assert_same_run(r, ref)
    TS.assert_matches_oracle(r, orc)
    assert r.st["total_iterations"] == int(orc.it.sum()) == int(r.it.sum())
    assert r.st["iterations"] == int(r.it.max()) and r.st["converged"] == int((r.cd != 0).sum())
    if not tol:
        assert (r.it == N).all() and (r.cd == 0).all()
    return ref


def check_fused(oracle, I, cfg, r):
    assert r.st["kernel"] == FUSED and r.st["kernel_ms"] > 0.0
    assert_same_run(r, class_plain(I, cfg))
    check_against_references(oracle, I, cfg, r)


# ------------------------------------------------------------------------------ CPU
def test_symbol_and_version():
    """gpad_setup_class_signals is declared, exported, defined behind abi_guard and bound; the minor is 6."""
    from gpad_mpc import _lib
    hdr = open(os.path.join(ROOT, "include", "gpad.h")).read()
    state = open(os.path.join(ROOT, "gpu-dualgradient-mpc_amd", "csrc", "gpad_state.cpp")).read()
    assert re.search(r"\bint gpad_setup_class_signals\(gpad_handle_t h, int ns, int per_class, const void\* SM, "
                     r"const void\* Sg,\s*const void\* E\);", hdr)
    assert re.search(r'gpad_setup_class_signals\([^)]*\)\s*\{\s*return gpad::abi_guard\("gpad_setup_class_signals"',
                     state)
    lib = _lib.load()
    assert "gpad_setup_class_signals" in _lib.EXPORTS and hasattr(lib, "gpad_setup_class_signals")
    assert len(lib.gpad_setup_class_signals.argtypes) == 6
    assert int(re.search(r"#define GPAD_VERSION_MINOR (\d+)", hdr).group(1)) == 6 == _lib.VERSION_MINOR
    assert lib.gpad_setup_class_signals(None, 1, 1, None, None, None) == _lib.ERR_INVALID  # null handle: no GPU
    assert b"gpad_setup_class_signals" in lib.gpad_last_error()


def test_python_surface():
    import gpad_mpc
    fn = gpad_mpc.GpadSolver.setup_class_signals
    par = inspect.signature(fn).parameters
    assert list(par) == ["self", "SM", "Sg", "E", "ns"]
    assert par["ns"].kind is par["ns"].KEYWORD_ONLY and all(par[k].default is None for k in ("SM", "Sg", "E", "ns"))
    s = gpad_mpc.GpadSolver.__new__(gpad_mpc.GpadSolver)  # (argument checks come before the library call)
    s._classes = 3
    with pytest.raises(ValueError):
        fn(s)
    with pytest.raises(ValueError):
        fn(s, np.zeros((3, 12, 4), np.float32), np.zeros((3, 56, 5), np.float32))
    with pytest.raises(ValueError):
        fn(s, np.zeros((3, 12, 4), np.float32), np.zeros((56, 4), np.float32))
    with pytest.raises(ValueError):
        fn(s, np.zeros((2, 12, 4), np.float32))


def test_generator():
    """battery_fleet_signals: class k is battery_plant_signals of caps[k]; minus the signal maps it is
    battery_fleet; L is the maximum."""
    from gpad_mpc import problems
    caps = base_inputs("A").C.qp.meta["caps"]
    qp, pl = problems.battery_fleet_signals(3, 4, caps)
    fq, fp = problems.battery_fleet(3, 4, caps)
    Ls = []
    for k, c in enumerate(caps):
        q1, p1 = problems.battery_plant_signals(3, 4, capacity_ah=c)
        Ls.append(q1.L)
        for name in ("ML", "M", "G", "g", "H", "q"):
            same_bits(getattr(qp, name)[k], getattr(q1, name), name)
        for name in ("PM", "Pg", "g0", "A", "B", "SM", "Sg", "E"):
            same_bits(getattr(pl, name)[k], getattr(p1, name), name)
    for name in ("ML", "M", "G", "g", "H", "q"):
        same_bits(getattr(qp, name), getattr(fq, name), name)
    for name in ("PM", "Pg", "g0", "A", "B"):
        same_bits(getattr(pl, name), getattr(fp, name), name)
    assert pl.M0 is None and fp.M0 is None and qp.L == fq.L == max(Ls)
    assert pl.ns == 4 and pl.SM.shape == (3, 12, 4) and pl.Sg.shape == (3, 56, 4) and pl.E.shape == (3, 3, 4)
    assert len({pl.SM[k].tobytes() for k in range(3)}) == 3  # the classes' signal maps differ
    eq, ep = problems.expand_classes(qp, pl, [2, 0, 1, 2])
    for b, k in enumerate([2, 0, 1, 2]):
        for name in SIG_MAPS:
            same_bits(getattr(ep, name)[b], getattr(pl, name)[k], name)
    with pytest.raises(ValueError):
        problems.battery_fleet_signals(3, 4, caps[:, :2])


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("name", ["SA", "SB", "SP", "SQ"])
def test_oracle_guard(oracle, name, warm):
    """On the oracle alone, at eps 1e-4: the counts are ragged (SA, SP, SQ: at least 4 distinct counts at
    every step with capped and early solves in one run; SB: at least 4 per step, the maximum below N), the
    per-pack totals differ, and each wrong implementation -- another class's SM / Sg / E, S left unpermuted,
    S dropped -- changes xs, us and the counts, the us bits of every pack."""
    I = sig_input(name)
    cfg = mode(I, warm, 1e-4)
    N = cfg[1]
    orc = oracle_ref(oracle, I, cfg)
    for k in ("x", "z", "y", "xs", "us"):
        assert np.isfinite(getattr(orc, k)).all(), k
    distinct = [len(set(row)) for row in orc.it.tolist()]
    assert min(distinct) >= 4, distinct
    assert len(set(orc.it.sum(axis=0).tolist())) > 1
    if name == "SB":
        assert orc.it.max() < N
    else:
        assert (orc.it == N).any() and (orc.it < N).any()
    for fault in ("maps", "rows", "zero"):
        bad = oracle_ref(oracle, I, cfg, fault)
        for k in ("xs", "us", "it"):
            assert getattr(bad, k).tobytes() != getattr(orc, k).tobytes(), (fault, k)
        moved = np.array([bad.us[:, b].tobytes() != orc.us[:, b].tobytes() for b in range(I.X0.shape[0])])
        if fault == "rows":  # (a pack whose sorted position is its own keeps its row)
            moved |= np.argsort(I.class_of, kind="stable") == np.arange(I.class_of.size)
        assert moved.all(), (fault, np.flatnonzero(~moved))


PLANT_MAPS = ("PM", "Pg", "M0", "g0", "A", "B")


def m0_input(roll=0, one_plant=False):
    """SA with test_class_loop.class_m0 as a per-class M0 (rolled by `roll` classes: the guard's wrong class
    index); one_plant: class 0's plant maps, M0[0] among them, for every class under the per-class signals."""
    I = sig_input("SA")
    J = with_maps(I, "M0" + ("-roll%d" % roll if roll else ""), M0=np.roll(class_m0(I.K, I.C.qp.n), roll, axis=0))
    if one_plant:
        J = with_maps(J, "class0-plant", **{k: np.stack([getattr(J.C, k)[0]] * I.K) for k in PLANT_MAPS})
    return J


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_m0_oracle_guard(oracle, warm):
    """On the oracle alone, at eps 1e-4: SA with the per-class M0 meets test_class_loop.assert_m0_guard, and the
    one-plant variant differs from the per-class one in exactly the 7 packs that are not in class 0."""
    I = sig_input("SA")
    cfg = mode(I, warm, 1e-4)
    assert_m0_guard(I, oracle_ref(oracle, I, cfg), oracle_ref(oracle, m0_input(), cfg),
                    oracle_ref(oracle, m0_input(roll=1), cfg), cfg[1],
                    other=oracle_ref(oracle, m0_input(one_plant=True), cfg), differ=I.class_of != 0)
    assert int((I.class_of != 0).sum()) == 7


# ------------------------------------------------------------------------------ GPU: a per-class M0
@pytest.mark.gpu
@pytest.mark.parametrize("warm,tol", M0_MODES, ids=M0_MODE_IDS)
@pytest.mark.parametrize("fused", [False, True], ids=["classes", "fused"])
def test_per_class_m0(gpu, oracle, fused, warm, tol):
    """A per-class plant with M0 under per-class signals: the fleet and the oracle; fused also the class handle
    with everything off."""
    I = m0_input()
    cfg = mode(I, warm, tol)
    r = sig_run(I, cfg, fused=True) if fused else class_plain(I, cfg)
    if fused:
        check_fused(oracle, I, cfg, r)
    else:
        check_against_references(oracle, I, cfg, r)
        assert r.st["kernel"] not in (None, FUSED) and r.st["kernel_ms"] > 0.0


def one_plant_run(I, cfg, fused):
    """m0_input(one_plant=True) as the binding sees it: class 0's maps and M0[0] through the 2-d setup_plant,
    then the per-class signals -- M0, g0 and B are replicated to a copy per class beside the packed images."""
    one = {k: F32(getattr(I.C, k)[0]) for k in PLANT_MAPS}
    s = class_solver(I, kernel=I.kernel)
    s.setup_plant(one["PM"], one["Pg"], M0=one["M0"], g0=one["g0"], A=one["A"], B=one["B"])
    bind_signals(s, I.C)
    if fused:
        s.set_class_loop_fused(True)
    return sig_loop(s, I, cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("warm,tol", M0_MODES, ids=M0_MODE_IDS)
@pytest.mark.parametrize("fused", [False, True], ids=["classes", "fused"])
def test_one_plant_with_m0_under_per_class_signals(gpu, oracle, fused, warm, tol):
    """The replication path: one plant with M0 under per-class signals == the fleet and the oracle with that
    plant replicated; fused also the same binding run class by class.  Not the per-class plant's bits."""
    I = m0_input(one_plant=True)
    cfg = mode(I, warm, tol)
    plain = cached("one-plant", I, cfg, lambda: one_plant_run(I, cfg, False))
    r = one_plant_run(I, cfg, True) if fused else plain
    assert (r.st["kernel"] == FUSED) == fused and r.st["kernel_ms"] > 0.0
    assert_same_run(r, plain)
    check_against_references(oracle, I, cfg, r)
    assert r.us.tobytes() != class_plain(m0_input(), cfg).us.tobytes()


# ------------------------------------------------------------------------------ GPU: class by class
@pytest.mark.gpu
@pytest.mark.parametrize("warm,tol", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["SA", "SB"])
def test_closed_loop(gpu, oracle, name, warm, tol):
    I = sig_input(name)
    cfg = mode(I, warm, tol)
    r = class_plain(I, cfg)
    check_against_references(oracle, I, cfg, r)
    assert r.st["kernel"] not in (None, "loop", "loop_panel", FUSED) and r.st["kernel_ms"] > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["classes", "fused"])
def test_one_copy_of_the_signal_maps(gpu, fused):
    """per_class = 0: class 0's SM, Sg, E for every class over the per-class plants == the fleet with those
    maps replicated; and not the per-class signals."""
    I = sig_input("SA")
    cfg = mode(I, False, 1e-4)
    rep = {k: np.stack([getattr(I.C, k)[0]] * I.K) for k in SIG_MAPS}
    J = with_maps(I, "class0-signals", **rep)
    r = sig_run(I, cfg, per_class=False, fused=fused)
    assert (r.st["kernel"] == FUSED) == fused
    assert_same_run(r, fleet_ref(J, cfg))
    assert r.us.tobytes() != class_plain(I, cfg).us.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["classes", "fused"])
def test_per_class_signals_over_one_plant(gpu, fused):
    """gpad_setup_plant (class 0's maps for every class) under per-class signal maps == the fleet with that
    plant replicated."""
    I = sig_input("SA")
    cfg = mode(I, False, 1e-4)
    one = {k: getattr(I.C, k)[0] for k in ("PM", "Pg", "g0", "A", "B")}
    J = with_maps(I, "class0-plant", **{k: np.stack([v] * I.K) for k, v in one.items()})
    s = class_solver(I, kernel=I.kernel)
    s.setup_plant(F32(one["PM"]), F32(one["Pg"]), g0=F32(one["g0"]), A=F32(one["A"]), B=F32(one["B"]))
    bind_signals(s, I.C)
    if fused:
        s.set_class_loop_fused(True)
    r = sig_loop(s, I, cfg)
    assert (r.st["kernel"] == FUSED) == fused
    assert_same_run(r, fleet_ref(J, cfg))
    assert r.us.tobytes() != class_plain(I, cfg).us.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["classes", "fused"])
@pytest.mark.parametrize("which", SIG_MAPS)
def test_null_map_is_a_zero_map(gpu, which, fused):
    I = sig_input("SA")
    cfg = mode(I, False, 1e-4)
    zero = with_maps(I, "zero-" + which, **{which: np.zeros_like(getattr(I.C, which))})
    null = with_maps(I, "null-" + which, **{which: None})
    a = sig_run(null, cfg, fused=fused)
    assert_same_run(a, sig_run(zero, cfg, fused=fused))
    assert_same_run(a, fleet_ref(zero, cfg))
    assert a.us.tobytes() != class_plain(I, cfg).us.tobytes()


@pytest.mark.gpu
def test_f64(gpu):
    """f64 on SA: the closed loop and gpad_run_state_signals against the f64 fleet."""
    I = sig_input("SA")
    cfg = mode(I, False, 1e-4)
    s = sig_solver(I, dtype=np.float64)
    r = sig_loop(s, I, cfg, np.float64)
    assert r.x.dtype == np.float64
    assert_same_run(r, fleet_ref(I, cfg, np.float64))
    f = fleet_solver(I, np.float64)
    outs = []
    for h in (s, f):
        Z, Y = np.zeros((I.X0.shape[0], I.C.qp.n)), np.zeros((I.X0.shape[0], I.C.qp.m))
        st = h.run_state(F64(I.X0), Z, Y, 400, 1e-4, s=F64(I.S[1]))
        outs.append((Z, Y, st))
    same_bits(outs[0][0], outs[1][0], "run_state z")
    same_bits(outs[0][1], outs[1][1], "run_state y")
    for k in ("iterations", "converged", "total_iterations", "tol_floor", "below_tol_floor", "nonfinite_g"):
        assert outs[0][2][k] == outs[1][2][k], k


@pytest.mark.gpu
@pytest.mark.parametrize("warm,tol", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("option", ["loop_async", "loop_panel"])
@pytest.mark.parametrize("name", ["SA", "SP"])
def test_forwarded_one_launch_loops(gpu, oracle, name, option, warm, tol):
    """The loop options reach every class, which applies them by its own rules with nx + ns columns: the
    bits of the class handle with them off.  (SP forces dims.kernel = PANEL, which the asynchronous loop
    does not serve: its classes stay on the lockstep loop.)"""
    I = sig_input(name)
    cfg = mode(I, warm, tol)
    plain = class_plain(I, cfg)
    r = sig_run(I, cfg, **{option: 1})
    want = "loop_panel" if option == "loop_panel" else ("loop" if name == "SA" else plain.st["kernel"])
    assert r.st["kernel"] == want
    assert_same_run(r, plain)
    TS.assert_matches_oracle(r, oracle_ref(oracle, I, cfg))


# ------------------------------------------------------------------------------ GPU: fused
@pytest.mark.gpu
@pytest.mark.parametrize("warm,tol", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["SA", "SA4", "SB", "SP", "SQ"])
def test_fused_closed_loop(gpu, oracle, name, warm, tol):
    I = sig_input(name)
    cfg = mode(I, warm, tol)
    check_fused(oracle, I, cfg, sig_run(I, cfg, fused=True))


@pytest.mark.gpu
@pytest.mark.parametrize("warm,tol", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("name", ["SA", "SQ"])
def test_fused_grid_caps(gpu, oracle, name, grid, warm, tol):
    """One workgroup walks every class (the class switch reloads [x_0; S[0]] of its new columns); two serve
    three classes."""
    I = sig_input(name)
    cfg = mode(I, warm, tol)
    check_fused(oracle, I, cfg, sig_run(I, cfg, fused=True, panel_max_grid=grid))


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["classes", "fused"])
@pytest.mark.parametrize("order", ["sorted", "reversed"])
def test_order_independence(gpu, order, fused):
    """SQ with its packs sorted, and reversed, S permuted along with them: pack for pack the same bits."""
    I = sig_input("SQ")
    cfg = mode(I, False, 1e-4)
    base = class_plain(I, cfg)
    o = np.argsort(I.class_of, kind="stable")
    if order == "reversed":
        o = o[::-1].copy()
    r = sig_run(reorder(I, o), cfg, fused=fused)
    assert (r.st["kernel"] == FUSED) == fused
    for k in ("x", "z", "y"):
        same_bits(getattr(r, k), getattr(base, k)[o], k)
    for k in ("xs", "us", "it", "cd"):
        same_bits(getattr(r, k), getattr(base, k)[:, o], k)
    for k in ("iterations", "converged", "total_iterations", "tol_floor"):
        assert r.st[k] == base.st[k]


@pytest.mark.gpu
@pytest.mark.parametrize("nxa", [64, 65])
def test_row_limit(gpu, nxa):
    """SA's maps padded with zero columns and S with random values in the padding: at nx + ns = 64 the fused
    loop takes the call, at 65 it runs class by class; both equal the fleet bound with the same padded maps
    (not the unpadded run: fma(0, s, -0) may flip the sign of a zero)."""
    I = sig_input("SA")
    cfg = mode(I, False, 1e-4)
    pad = nxa - I.C.nx - I.C.ns
    wide = {k: np.concatenate([getattr(I.C, k), np.zeros(getattr(I.C, k).shape[:2] + (pad,))], axis=2)
            for k in SIG_MAPS}
    J = with_maps(I, "padded-%d" % nxa, **wide)
    noise = np.random.default_rng(215).uniform(-1, 1, I.S.shape[:2] + (pad,)).astype(np.float32)
    J.S = np.ascontiguousarray(np.concatenate([I.S, noise], axis=2))
    assert J.C.nx + J.C.ns == nxa
    r = sig_run(J, cfg, fused=True)
    assert (r.st["kernel"] == FUSED) == (nxa == 64)
    assert_same_run(r, fleet_ref(J, cfg))


@pytest.mark.gpu
def test_fused_fallback_f64(gpu):
    I = sig_input("SA")
    cfg = (3, 100, 1e-4, False)
    off = sig_run(I, cfg, np.float64)
    on = sig_run(I, cfg, np.float64, fused=True)
    assert on.st["kernel"] not in (None, FUSED) and on.st["kernel"] == off.st["kernel"]
    assert_same_run(on, off)


@pytest.mark.gpu
def test_fused_fallback_limit_off_the_test_period(gpu):
    I = sig_input("SA")
    cfg = (I.steps, I.Ntol + 3, 1e-4, False)
    off = sig_run(I, cfg)
    on = sig_run(I, cfg, fused=True)
    assert on.st["kernel"] not in (None, FUSED) and on.st["kernel"] == off.st["kernel"]
    assert_same_run(on, off)
    assert_same_run(on, fleet_ref(I, cfg))


@pytest.mark.gpu
@pytest.mark.parametrize("tol", [0.0, 1e-4], ids=["fixed", "tol"])
def test_fused_fallback_run_state(gpu, tol):
    """gpad_run_state_signals on a handle with the fused loop on: class by class, the fleet's bits."""
    I = sig_input("SA")
    batch, n, m = I.X0.shape[0], I.C.qp.n, I.C.qp.m
    N = 400 if tol else 60
    outs = []
    for s in (sig_solver(I), sig_solver(I, fused=True), fleet_solver(I)):
        Z, Y = np.zeros((batch, n), np.float32), np.zeros((batch, m), np.float32)
        st = s.run_state(I.X0, Z, Y, N, tol, s=I.S[2])
        outs.append((Z, Y, st))
    assert outs[1][2]["kernel"] not in (None, FUSED) and outs[1][2]["kernel"] == outs[0][2]["kernel"]
    for Z, Y, st in outs[:2]:
        same_bits(Z, outs[2][0], "z")
        same_bits(Y, outs[2][1], "y")
        for k in ("iterations", "converged", "total_iterations", "tol_floor", "below_tol_floor", "nonfinite_g"):
            assert st[k] == outs[2][2][k], k
    # the signals reached the solve: another step's rows give other bits
    Z, Y = np.zeros((batch, n), np.float32), np.zeros((batch, m), np.float32)
    sig_solver(I).run_state(I.X0, Z, Y, N, tol, s=I.S[3])
    assert Z.tobytes() != outs[0][0].tobytes()


# ------------------------------------------------------------------------------ GPU: lifecycle, validation
def _code(fn):
    from gpad_mpc._lib import GpadError
    with pytest.raises(GpadError) as e:
        fn()
    return e.value.code, str(e.value)


@pytest.mark.gpu
def test_status_codes(gpu):
    import gpad_mpc
    from gpad_mpc import _lib
    I = sig_input("SA")
    F, p = I.C, I.C.qp
    batch = I.X0.shape[0]
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    SM, Sg, E = F32(F.SM), F32(F.Sg), F32(F.E)
    Z, Y = np.zeros((batch, p.n), np.float32), np.zeros((batch, p.m), np.float32)
    # not class-bound: a fresh handle, and one with a plain problem and plant
    t = gpad_mpc.GpadSolver(0)
    assert t.lib.gpad_setup_class_signals(t.h, F.ns, 1, vp(SM), vp(Sg), vp(E)) == _lib.ERR_NOT_SETUP
    t.setup(F32(p.ML[0]), F32(p.G[0]), _L(p, np.float32), n=p.n, m=p.m, batch=batch, shared=True)
    t.setup_plant(F32(F.PM[0]), F32(F.Pg[0]), g0=F32(F.g0[0]), A=F32(F.A[0]), B=F32(F.B[0]))
    assert t.lib.gpad_setup_class_signals(t.h, F.ns, 1, vp(SM), vp(Sg), vp(E)) == _lib.ERR_NOT_SETUP
    # class-bound without a plant
    u = gpad_mpc.GpadSolver(0)
    u.setup_classes(F32(p.ML), F32(p.G), _L(p, np.float32), I.class_of, n=p.n, m=p.m)
    lib = u.lib
    assert lib.gpad_setup_class_signals(u.h, F.ns, 1, vp(SM), vp(Sg), vp(E)) == _lib.ERR_NOT_SETUP
    # a plant without A, B: SM, Sg bind, E is refused; a loop has no dynamics
    u.setup_plant(F32(F.PM), F32(F.Pg), g0=F32(F.g0))
    assert lib.gpad_setup_class_signals(u.h, F.ns, 1, vp(SM), vp(Sg), vp(E)) == _lib.ERR_INVALID
    assert lib.gpad_setup_class_signals(u.h, F.ns, 1, vp(SM), vp(Sg), None) == _lib.GPAD_OK
    u.run_state(I.X0, Z, Y, 20, s=I.S[0])
    assert _code(lambda: sig_loop(u, I, (2, 20, 0.0, False)))[0] == _lib.ERR_NOT_SETUP
    # the full plant
    s = class_solver(I)
    assert lib.gpad_setup_class_signals(s.h, -1, 1, vp(SM), vp(Sg), vp(E)) == _lib.ERR_INVALID
    assert lib.gpad_setup_class_signals(s.h, F.ns, 2, vp(SM), vp(Sg), vp(E)) == _lib.ERR_INVALID
    assert lib.gpad_setup_class_signals(s.h, F.ns, -1, vp(SM), vp(Sg), vp(E)) == _lib.ERR_INVALID
    # no class signals bound yet: the plain binding and the _signals runs are unsupported, as before
    code, text = _code(lambda: s.setup_signals(ns=1))
    assert code == _lib.ERR_UNSUPPORTED and "class binding" in text
    code, text = _code(lambda: s.run_state(I.X0, Z, Y, 10, s=I.S[0]))
    assert code == _lib.ERR_UNSUPPORTED and "class binding" in text
    code, text = _code(lambda: sig_loop(s, I, (2, 20, 0.0, False)))
    assert code == _lib.ERR_UNSUPPORTED and "class binding" in text
    assert lib.gpad_setup_class_signals(s.h, F.ns, 1, vp(SM), vp(Sg), vp(E)) == _lib.GPAD_OK
    code, text = _code(lambda: s.setup_signals(ns=1))
    assert code == _lib.ERR_UNSUPPORTED and "class binding" in text
    # bound: the plain runs are invalid, a NULL s / S is invalid
    X = I.X0.copy()
    assert _code(lambda: s.run_state(I.X0, Z, Y, 10))[0] == _lib.ERR_INVALID
    assert _code(lambda: s.closed_loop(X, Z, Y, 2, 10))[0] == _lib.ERR_INVALID
    assert lib.gpad_run_state_signals(s.h, vp(X), None, vp(Z), vp(Y), 10, 0.0, None) == _lib.ERR_INVALID
    assert lib.gpad_closed_loop_signals(s.h, vp(X), vp(Z), vp(Y), None, 2, 10, 0.0, 0, None, None,
                                        None) == _lib.ERR_INVALID
    assert sig_loop(s, I, (2, 20, 0.0, False)).st["iterations"] == 20  # the binding survived all that


@pytest.mark.gpu
def test_lifecycle(gpu):
    """ns = 0 unbinds (the plain loop then equals the class run that never had signals); a new plant and
    gpad_setup_classes unbind; two loops with different S on one handle; fused on, off and on again."""
    from gpad_mpc import _lib
    from test_classes import _bind_plant
    from test_loop_async import loop
    I = sig_input("SA")
    cfg = mode(I, False, 1e-4)
    steps, N, tol, warm = cfg
    base = class_plain(I, cfg)
    s = sig_solver(I)
    assert_same_run(sig_loop(s, I, cfg), base)
    # another S on the same handle, then the first again
    J = SimpleNamespace(**vars(I))
    J.S = np.ascontiguousarray(I.S[::-1])
    J.name = "SA-reversed-steps"
    J.E = I.E
    other = sig_loop(s, J, cfg)
    assert other.us.tobytes() != base.us.tobytes()
    assert_same_run(other, fleet_ref(J, cfg))
    assert_same_run(sig_loop(s, I, cfg), base)
    # fused on, off and on again between runs
    for on in (True, False, True):
        s.set_class_loop_fused(on)
        r = sig_loop(s, I, cfg)
        assert (r.st["kernel"] == FUSED) == on
        assert_same_run(r, base)
    r = sig_loop(s, J, cfg)
    assert r.st["kernel"] == FUSED
    assert_same_run(r, other)
    # ns = 0 unbinds: the plain loop, with the fused loop still on and then off
    s.setup_class_signals(ns=0)
    x0 = I.X0
    nosig = loop(class_solver(I), I.C, x0, steps, N, tol, warm)  # a handle that never had signals
    r = loop(s, I.C, x0, steps, N, tol, warm)
    assert r.st["kernel"] == FUSED
    assert_same_run(r, nosig)
    s.set_class_loop_fused(False)
    assert_same_run(loop(s, I.C, x0, steps, N, tol, warm), nosig)
    assert _code(lambda: sig_loop(s, I, cfg))[0] == _lib.ERR_UNSUPPORTED
    # rebinding works; a new plant unbinds
    bind_signals(s, I.C)
    assert_same_run(sig_loop(s, I, cfg), base)
    _bind_plant(s, I.C, F32)
    assert _code(lambda: sig_loop(s, I, cfg))[0] == _lib.ERR_UNSUPPORTED
    assert_same_run(loop(s, I.C, x0, steps, N, tol, warm), nosig)
    # gpad_setup_classes unbinds (the plant goes with the old binding too)
    bind_signals(s, I.C)
    s.set_class_loop_fused(True)
    p = I.C.qp
    s.setup_classes(F32(p.ML), F32(p.G), _L(p, np.float32), I.class_of, n=p.n, m=p.m)
    assert _code(lambda: bind_signals(s, I.C))[0] == _lib.ERR_NOT_SETUP
    _bind_plant(s, I.C, F32)
    assert _code(lambda: sig_loop(s, I, cfg))[0] == _lib.ERR_UNSUPPORTED
    bind_signals(s, I.C)
    assert_same_run(sig_loop(s, I, cfg), base)
    # signals bound before the fused loop is first switched on
    s.set_class_loop_fused(True)
    r = sig_loop(s, I, cfg)
    assert r.st["kernel"] == FUSED
    assert_same_run(r, base)


# ------------------------------------------------------------------------------ GPU: memory kinds
@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["classes", "fused"])
def test_device_memory(gpu, oracle, fused):
    """Torch device tensors (maps, X, Z, Y, S, xs, us) against host arrays; then the same run without stats
    (asynchronous), after which gpad_sync and gpad_last_stats report the same counts, codes and stats."""
    import torch
    I = sig_input("SQ")
    cfg = mode(I, True, 1e-4)
    steps, N, tol, warm = cfg
    host = class_plain(I, cfg)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    s = sig_solver(I, to=to, fused=fused)
    batch = I.X0.shape[0]
    S = to(I.S)

    def arrays():
        return (to(I.X0), torch.zeros((batch, I.C.qp.n), device=gpu), torch.zeros((batch, I.C.qp.m), device=gpu),
                torch.zeros((steps, batch, I.C.nx), device=gpu), torch.zeros((steps, batch, I.C.nu), device=gpu))
    X, Z, Y, XS, US = arrays()
    IT, CD = np.full(steps * batch, -1, np.int32), np.full(steps * batch, -1, np.int32)
    st = s.closed_loop(X, Z, Y, steps, N, tol, warm=warm, xs=XS, us=US, iters=IT, codes=CD, signals=S)
    dev = SimpleNamespace(x=X.cpu().numpy(), z=Z.cpu().numpy(), y=Y.cpu().numpy(), xs=XS.cpu().numpy(),
                          us=US.cpu().numpy(), it=IT.reshape(steps, batch), cd=CD.reshape(steps, batch), st=st)
    assert (st["kernel"] == FUSED) == fused
    assert_same_run(dev, host)
    TS.assert_matches_oracle(dev, oracle_ref(oracle, I, cfg))
    same_bits(S.cpu().numpy(), I.S, "S is read only")

    X, Z, Y, XS, US = arrays()
    assert s.closed_loop(X, Z, Y, steps, N, tol, warm=warm, xs=XS, us=US, stats=False, signals=S) is None
    s.sync()
    IT2, CD2 = np.full(steps * batch, -1, np.int32), np.full(steps * batch, -1, np.int32)
    st2 = s.last_stats(iters=IT2, codes=CD2)
    same_bits(IT2.reshape(steps, batch), host.it, "iters")
    same_bits(CD2.reshape(steps, batch), host.cd, "codes")
    assert (st2["kernel"] == FUSED) == fused
    for k in ("iterations", "converged", "total_iterations", "tol_floor", "below_tol_floor", "nonfinite_g"):
        assert st2[k] == host.st[k], k
    for k, v in (("x", X), ("z", Z), ("y", Y), ("xs", XS), ("us", US)):
        same_bits(v.cpu().numpy(), getattr(host, k), k)


# ------------------------------------------------------------------------------ GPU: certification floor
@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["classes", "fused"])
def test_certification_floor(gpu, fused):
    """One pack of class 1 gets a large load at one middle step only: tol_floor and the flags cover g(x, s) of
    that step -- they equal the fleet's, and the floor is above that of the undisturbed run."""
    I = sig_input("SA")
    cfg = mode(I, False, 1e-4)
    J = SimpleNamespace(**vars(I))
    J.S = I.S.copy()
    b = int(np.flatnonzero(I.class_of == 1)[1])
    J.S[3, b, 0] = 3.0e4
    J.name = "SA-spike"
    ref = fleet_ref(J, cfg)
    r = sig_run(J, cfg, fused=fused)
    assert (r.st["kernel"] == FUSED) == fused
    assert_same_run(r, ref)
    for k in ("tol_floor", "below_tol_floor", "nonfinite_g"):
        assert r.st[k] == ref.st[k], k
    assert r.st["tol_floor"] > 10.0 * class_plain(I, cfg).st["tol_floor"] > 0.0
