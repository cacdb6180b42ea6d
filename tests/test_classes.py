"""Fleets of a few plant classes: the class binding (gpad_setup_classes, csrc/gpad_classes.cpp and the
row permutations of csrc/gpad_classes.hip).

The contract is bit identity with code that predates the feature: a fleet whose packs come from K
classes, bound with gpad_setup_classes, equals (a) the dims.shared = 0 handle of the same fleet
(problems.expand_classes: every pack its own copy of its class's matrices and maps, stacked plant,
options off), (b) the CPU oracle's closed loop of every pack with its class's matrices and maps, and
for input A (c) one batch-1 handle per pack.  x, z, y, xs, us and the per-step counts and codes are
compared with same_bits in the caller's instance order; the aggregate stats equal the reference's sums
and maxima.  The references of an input and mode are computed once and shared by the cases that vary
only the engine, the option or the memory kind.

Inputs (checked on the oracle: every pack finite at eps 1e-4, the largest count 150 resp. 390, well
under N; counts ragged -- cold, 6-7 distinct counts per step for A and 3 for B -- and at one x0 the
classes give distinct us bits):
  A   n = 12, m = 56: battery_fleet(3, 4, caps[:3]), 11 packs in 3 classes of 4 / 2 / 5, 6 steps
  A4  A with K = 4 and class 3 empty
  B   n = 40, m = 180: battery_fleet(4, 10, caps[:2]), 5 packs in 2 classes of 2 / 3, 4 steps
  P   A's classes 0 and 1 with 40 packs, class_of[b] = (b * 7) % 5 < 2: class 0 has 24 packs (two
      panels, the second ragged), class 1 has 16 (one full panel); dims.kernel = PANEL
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT
from test_fleet import oracle_pack, pack
from test_loop_async import F32, F64, assert_matches_oracle, assert_same_run, loop, same_bits

MAPS = ("PM", "Pg", "M0", "g0", "A", "B")
NOMINAL = 0.027 * 4.1


# ------------------------------------------------------------------------------ inputs
def _ns(qp, pl, X0):
    return SimpleNamespace(qp=qp, PM=pl.PM, Pg=pl.Pg, M0=pl.M0, g0=pl.g0, A=pl.A, B=pl.B, nx=pl.nx, nu=pl.nu, X0=X0)


def _make(name, n_u, Nh, caps, class_of, xseed, steps, Ntol, rag):
    """C: the per-class stacks (what the class binding takes); E: the expanded fleet (what the shared = 0
    reference, the oracle and the batch-1 handles take), both with the per-instance X0."""
    from gpad_mpc import problems
    class_of = np.asarray(class_of, np.int32)
    qp, pl = problems.battery_fleet(n_u, Nh, caps)
    eq, ep = problems.expand_classes(qp, pl, class_of)
    X0 = (np.random.default_rng(xseed).random((class_of.size, n_u)) - 0.5).astype(np.float32)
    return SimpleNamespace(name=name, K=caps.shape[0], class_of=class_of, X0=X0, C=_ns(qp, pl, X0), E=_ns(eq, ep, X0),
                           steps=steps, Ntol=Ntol, rag=rag)


def _caps(rng, packs, n_u):
    return NOMINAL * np.random.default_rng(rng).uniform(0.6, 1.4, (packs, n_u))


@functools.lru_cache(maxsize=None)
def inputs(name):
    a_of = [2, 0, 2, 1, 0, 2, 0, 1, 2, 0, 2]
    if name == "A":
        return _make("A", 3, 4, _caps(107, 7, 3)[:3], a_of, 211, 6, 2000, 6)
    if name == "A4":
        return _make("A4", 3, 4, _caps(107, 7, 3)[:4], a_of, 211, 6, 2000, 6)
    if name == "B":
        return _make("B", 4, 10, _caps(105, 5, 4)[:2], [1, 0, 1, 1, 0], 212, 4, 3000, 3)
    if name == "P":
        return _make("P", 3, 4, _caps(107, 7, 3)[:2], [int((b * 7) % 5 < 2) for b in range(40)], 213, 6, 2000, 6)
    raise KeyError(name)


def reorder(I, order):
    """Input I with its packs in another order (class_of and X0 permuted together)."""
    order = np.asarray(order)
    J = SimpleNamespace(**vars(I))
    J.class_of = np.ascontiguousarray(I.class_of[order])
    J.X0 = np.ascontiguousarray(I.X0[order])
    J.C = SimpleNamespace(**dict(vars(I.C), X0=J.X0))
    J.E = None
    return J


# ------------------------------------------------------------------------------ handles and runs
def _conv(dtype):
    return F64 if dtype == np.float64 else F32


def _L(qp, dtype):
    return float(qp.L) if dtype == np.float64 else float(np.float32(qp.L))


def _bind_plant(s, F, c, to=lambda a: a):
    opt = lambda a: None if a is None else to(c(a))  # noqa: E731
    s.setup_plant(to(c(F.PM)), to(c(F.Pg)), M0=opt(F.M0), g0=opt(F.g0), A=to(c(F.A)), B=to(c(F.B)))


def class_solver(I, *, dtype=np.float32, kernel=None, to=lambda a: a, **options):
    """The class binding of input I: per-class matrices and per-class plant maps.  `to`: host array ->
    what the handle is given (identity: host memory; a torch upload: device memory)."""
    import gpad_mpc
    from gpad_mpc import _lib
    c = _conv(dtype)
    s = gpad_mpc.GpadSolver(0)
    s.setup_classes(to(c(I.C.qp.ML)), to(c(I.C.qp.G)), _L(I.C.qp, dtype), I.class_of, n=I.C.qp.n, m=I.C.qp.m,
                    kernel=_lib.KERNEL_AUTO if kernel is None else kernel)
    _bind_plant(s, I.C, c, to)
    s.set_options(**options)
    return s


def fleet_solver(I, *, dtype=np.float32):
    """The reference: dims.shared = 0, every pack its own matrices and stacked maps, options off -- code
    that the class binding does not touch."""
    import gpad_mpc
    c = _conv(dtype)
    s = gpad_mpc.GpadSolver(0)
    s.setup(c(I.E.qp.ML), c(I.E.qp.G), _L(I.E.qp, dtype), n=I.E.qp.n, m=I.E.qp.m, batch=I.X0.shape[0], shared=False)
    _bind_plant(s, I.E, c)
    return s


def single_solver(p, dtype=np.float32):
    import gpad_mpc
    c = _conv(dtype)
    s = gpad_mpc.GpadSolver(0)
    s.setup(c(p.qp.ML), c(p.qp.G), _L(p.qp, dtype), n=p.qp.n, m=p.qp.m, batch=1, shared=True)
    _bind_plant(s, p, c)
    return s


def mode(I, warm, tol):
    return I.steps, (I.Ntol if tol else 100), tol, warm


_cache = {}


def cached(kind, I, cfg, make):
    k = (kind, I.name) + tuple(cfg)
    if k not in _cache:
        _cache[k] = make()
    return _cache[k]


def class_run(I, cfg, **kw):
    steps, N, tol, warm = cfg
    dtype = kw.get("dtype", np.float32)
    return loop(class_solver(I, **kw), I.C, I.X0, steps, N, tol, warm, dtype)


def class_plain(I, cfg):
    """The class handle with kernel AUTO and both loop options off, once per input and mode."""
    return cached("classes", I, cfg, lambda: class_run(I, cfg))


def fleet_ref(I, cfg, dtype=np.float32):
    steps, N, tol, warm = cfg
    return cached("fleet" + np.dtype(dtype).name, I, cfg,
                  lambda: loop(fleet_solver(I, dtype=dtype), I.E, I.X0, steps, N, tol, warm, dtype))


def _stack(rows):
    return SimpleNamespace(
        x=np.stack([r[0] for r in rows]), z=np.stack([r[1] for r in rows]), y=np.stack([r[2] for r in rows]),
        xs=np.stack([r[3] for r in rows], axis=1), us=np.stack([r[4] for r in rows], axis=1),
        it=np.stack([r[5] for r in rows], axis=1))


def oracle_ref(oracle, I, cfg):
    steps, N, tol, warm = cfg
    return cached("oracle", I, cfg, lambda: _stack(
        [oracle_pack(oracle, pack(I.E, b), steps, N, tol, warm) for b in range(I.X0.shape[0])]))


def singles_ref(I, cfg):
    """One batch-1 handle per pack (gpad_setup shared + gpad_setup_plant), concatenated."""
    steps, N, tol, warm = cfg

    def make():
        rs = []
        for b in range(I.X0.shape[0]):
            p = pack(I.E, b)
            rs.append(loop(single_solver(p), p, p.X0, steps, N, tol, warm))
        cat = lambda k, ax: np.concatenate([getattr(r, k) for r in rs], axis=ax)  # noqa: E731
        return SimpleNamespace(x=cat("x", 0), z=cat("z", 0), y=cat("y", 0), xs=cat("xs", 1), us=cat("us", 1),
                               it=cat("it", 1), cd=cat("cd", 1))
    return cached("singles", I, cfg, make)


def assert_ragged(I, orc, N, warm):
    """The oracle's counts are really ragged and under the cap (a flat input cannot hide a row that
    landed in another pack's place): I.rag distinct counts at every step of a cold run (at some step of
    a warm one, whose later steps start at the solution), unequal totals per pack, every solve under N."""
    distinct = [len(set(row)) for row in orc.it.tolist()]
    assert (max if warm else min)(distinct) >= I.rag, distinct
    assert len(set(orc.it.sum(axis=0).tolist())) > 1
    assert orc.it.max() < N


def assert_outputs_equal(r, ref):
    for k in ("x", "z", "y", "xs", "us", "it", "cd"):
        same_bits(getattr(r, k), getattr(ref, k), k)


# ------------------------------------------------------------------------------ CPU
def test_symbols_and_version():
    """The three entry points are declared, exported and defined; the minor is still 6."""
    from gpad_mpc import _lib
    hdr = open(os.path.join(ROOT, "include", "gpad.h")).read()
    csrc = os.path.join(ROOT, "gpu-dualgradient-mpc_amd", "csrc")
    host = open(os.path.join(csrc, "gpad_host.cpp")).read()
    state = open(os.path.join(csrc, "gpad_state.cpp")).read()  # (the plant and class entry points)
    assert re.search(r"\bint gpad_class_order\(const int\* class_of, int batch, int K, int\* perm, int\* offsets\);", hdr)
    assert re.search(r"\bint gpad_setup_classes\(gpad_handle_t h, const gpad_dims_t\* dims, int K, const int\* class_of,", hdr)
    assert re.search(r"\bint gpad_setup_plant_classes\(gpad_handle_t h, int nx, int nu,", hdr)
    lib = _lib.load()
    for name in ("gpad_class_order", "gpad_setup_classes", "gpad_setup_plant_classes"):
        assert name in _lib.EXPORTS and name in state
        assert hasattr(lib, name)
    assert int(re.search(r"#define GPAD_VERSION_MINOR (\d+)", hdr).group(1)) == 6 == _lib.VERSION_MINOR
    assert re.search(r'gpad_version\(void\) \{ return "gpad-mi355x 0\.6 ', host)


def _class_order(class_of, batch, K, perm=True, offsets=True, ids=True):
    from gpad_mpc import _lib
    lib = _lib.load()
    co = np.ascontiguousarray(class_of, np.int32)
    p = np.full(max(batch, 1), -7, np.int32)
    o = np.full(max(K, 0) + 1, -7, np.int32)
    ip = C.POINTER(C.c_int)
    rc = lib.gpad_class_order(co.ctypes.data_as(ip) if ids else None, batch, K, p.ctypes.data_as(ip) if perm else None,
                              o.ctypes.data_as(ip) if offsets else None)
    return rc, p, o


def test_class_order():
    """perm is numpy's stable argsort, offsets the prefix counts, on 20 seeded class_of with empty
    classes among them; every invalid input is GPAD_ERR_INVALID."""
    from gpad_mpc import _lib
    rng = np.random.default_rng(31)
    empties = 0
    for _ in range(20):
        batch, K = int(rng.integers(1, 201)), int(rng.integers(1, 10))
        co = rng.integers(0, K, batch).astype(np.int32)
        if K > 2:
            co[co == 1] = 0  # an empty class in the middle
        rc, perm, off = _class_order(co, batch, K)
        assert rc == _lib.GPAD_OK
        counts = np.bincount(co, minlength=K)
        empties += int((counts == 0).sum())
        assert np.array_equal(perm, np.argsort(co, kind="stable"))
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(counts)]))
    assert empties > 0
    ok = np.array([0, 1, 0], np.int32)
    assert _class_order(ok, 3, 2)[0] == _lib.GPAD_OK
    assert _class_order(ok, 3, 2, ids=False)[0] == _lib.ERR_INVALID
    assert _class_order(ok, 3, 2, perm=False)[0] == _lib.ERR_INVALID
    assert _class_order(ok, 3, 2, offsets=False)[0] == _lib.ERR_INVALID
    assert _class_order(ok, 0, 2)[0] == _lib.ERR_INVALID
    assert _class_order(ok, 3, 0)[0] == _lib.ERR_INVALID
    assert _class_order(np.array([0, 2, 0], np.int32), 3, 2)[0] == _lib.ERR_INVALID
    assert _class_order(np.array([0, -1, 0], np.int32), 3, 2)[0] == _lib.ERR_INVALID


def test_expand_classes():
    """expand_classes is indexing by hand; L is unchanged; a bad id is refused."""
    from gpad_mpc import problems
    I = inputs("A")
    qp, pl = problems.battery_fleet(3, 4, _caps(107, 7, 3)[:3])
    eq, ep = problems.expand_classes(qp, pl, I.class_of)
    for b, k in enumerate(I.class_of.tolist()):
        for name in ("ML", "M", "G", "g", "H", "q"):
            same_bits(getattr(eq, name)[b], getattr(qp, name)[k], name)
        for name in ("PM", "Pg", "g0", "A", "B"):
            same_bits(getattr(ep, name)[b], getattr(pl, name)[k], name)
    assert ep.M0 is None and eq.L == qp.L and eq.ML.shape == (11, 12, 56) and (ep.nx, ep.nu) == (3, 3)
    with pytest.raises(ValueError):
        problems.expand_classes(qp, pl, [0, 3])


@pytest.mark.parametrize("name", ["A", "B"])
def test_discrimination_guard(oracle, name):
    """On the oracle alone: pack 0 run with the matrices and maps of each other class gives other us and
    x bits -- a wrong class mapping cannot pass the comparisons below."""
    I = inputs(name)
    own_class = int(I.class_of[0])
    own = oracle_pack(oracle, pack(I.E, 0), I.steps, I.Ntol, 1e-4, False)
    others = [k for k in range(I.K) if k != own_class]
    assert others
    for k in others:
        j = int(np.flatnonzero(I.class_of == k)[0])  # a pack of class k lends its matrices and maps
        got = oracle_pack(oracle, pack(I.E, 0, matrices=j, maps=j), I.steps, I.Ntol, 1e-4, False)
        assert got[0].tobytes() != own[0].tobytes(), k  # x
        assert got[4].tobytes() != own[4].tobytes(), k  # us


# ------------------------------------------------------------------------------ GPU
MODES = [(False, 0.0), (False, 1e-4), (True, 0.0), (True, 1e-4)]
MODE_IDS = ["cold-fixed", "cold-tol", "warm-fixed", "warm-tol"]


def check_against_references(oracle, I, cfg, r):
    steps, N, tol, warm = cfg
    ref = fleet_ref(I, cfg)
    orc = oracle_ref(oracle, I, cfg)
    assert_same_run(r, ref)  # outputs, counts, codes, aggregate stats and tol_floor
    assert_matches_oracle(r, orc)
    assert r.st["total_iterations"] == int(orc.it.sum()) == int(r.it.sum())
    assert r.st["iterations"] == int(r.it.max()) and r.st["converged"] == int((r.cd != 0).sum())
    if tol:
        assert_ragged(I, orc, N, warm)
    else:
        assert (r.it == N).all() and (r.cd == 0).all()
    return ref, orc


@pytest.mark.gpu
@pytest.mark.parametrize("warm,tol", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["A", "A4", "B"])
def test_closed_loop(gpu, oracle, name, warm, tol):
    """The class binding == the shared = 0 fleet == the oracle, pack by pack (== batch-1 handles for A)."""
    I = inputs(name)
    cfg = mode(I, warm, tol)
    r = class_plain(I, cfg)
    check_against_references(oracle, I, cfg, r)
    assert r.st["kernel"] not in (None, "loop", "loop_panel") and r.st["kernel_ms"] > 0.0
    if name == "A":
        assert_outputs_equal(r, singles_ref(I, cfg))


@pytest.mark.gpu
@pytest.mark.parametrize("warm,tol", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("kernel", ["panel", "resident"])
def test_closed_loop_forced_engine(gpu, oracle, kernel, warm, tol):
    """A with dims.kernel forced for every class: the same bits, and the stats name that engine."""
    from gpad_mpc import _lib
    I = inputs("A")
    cfg = mode(I, warm, tol)
    r = class_run(I, cfg, kernel=dict(panel=_lib.KERNEL_PANEL, resident=_lib.KERNEL_RESIDENT)[kernel])
    assert r.st["kernel"] == kernel
    check_against_references(oracle, I, cfg, r)


def _qp_data(I):
    """Per-instance M, g of gpad_run from the plant maps at X0 (any data would do: both handles get it)."""
    E = I.E
    M = F32(np.einsum("bij,bj->bi", E.PM, I.X0.astype(np.float64)))
    g = F32(E.g0 + np.einsum("bij,bj->bi", E.Pg, I.X0.astype(np.float64)))
    return M, g


@pytest.mark.gpu
@pytest.mark.parametrize("tol", [0.0, 1e-4], ids=["fixed", "tol"])
@pytest.mark.parametrize("name", ["A", "P"])
def test_run_and_run_state(gpu, name, tol):
    """gpad_run (M, g given) and gpad_run_state against the shared = 0 handle; on P the engine is forced
    to the panels (24 and 16 packs: three panels, one ragged) and the stats say so."""
    from gpad_mpc import _lib
    I = inputs(name)
    batch, n, m = I.X0.shape[0], I.C.qp.n, I.C.qp.m
    N = 300 if tol else 60
    forced = _lib.KERNEL_PANEL if name == "P" else None
    cs, fs = class_solver(I, kernel=forced), fleet_solver(I)
    M, g = _qp_data(I)
    outs = {}
    for tag, s in (("classes", cs), ("fleet", fs)):
        Z, Y = np.zeros((batch, n), np.float32), np.zeros((batch, m), np.float32)
        it, cd = np.full(batch, -1, np.int32), np.full(batch, -1, np.int32)
        st = s.run(Z, Y, M, g, N, tol, iters=it, codes=cd)
        Z2, Y2 = np.zeros((batch, n), np.float32), np.zeros((batch, m), np.float32)
        st2 = s.run_state(I.X0, Z2, Y2, N, tol)
        outs[tag] = (Z, Y, it, cd, st, Z2, Y2, st2)
    a, b = outs["classes"], outs["fleet"]
    for i, what in ((0, "run z"), (1, "run y"), (2, "run iters"), (3, "run codes"), (5, "run_state z"),
                    (6, "run_state y")):
        same_bits(a[i], b[i], what)
    for i in (4, 7):
        for k in ("iterations", "converged", "total_iterations", "below_tol_floor", "nonfinite_g", "tol_floor"):
            assert a[i][k] == b[i][k], k
    assert a[4]["total_iterations"] == int(a[2].sum())
    if tol:  # the reference's counts are ragged and under the cap (on the oracle: 6 and 7 distinct, at most 150)
        assert len(set(b[2].tolist())) >= 6 and b[2].max() < N
    if forced:
        assert a[4]["kernel"] == "panel" and a[7]["kernel"] == "panel"
    # the classes differ: the rows really moved (no two packs of different classes share z)
    assert len({a[0][j].tobytes() for j in range(batch)}) == batch


@pytest.mark.gpu
@pytest.mark.parametrize("warm,tol", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("option,kernel", [("loop_async", "loop"), ("loop_panel", "loop_panel")])
@pytest.mark.parametrize("name", ["A", "B"])
def test_one_launch_loops(gpu, oracle, name, option, kernel, warm, tol):
    """The option reaches every class: each runs its whole loop in one launch, with the bits of the class
    handle with both options off and of the oracle."""
    I = inputs(name)
    cfg = mode(I, warm, tol)
    r = class_run(I, cfg, **{option: 1})
    assert r.st["kernel"] == kernel
    assert_same_run(r, class_plain(I, cfg))
    assert_matches_oracle(r, oracle_ref(oracle, I, cfg))


@pytest.mark.gpu
@pytest.mark.parametrize("option", ["loop_async", "loop_panel"])
def test_one_launch_loop_not_qualified(gpu, option):
    """f64 classes do not qualify for the one-launch loops: the option is accepted and every class runs
    the lockstep loop, with equal bits."""
    I = inputs("A")
    cfg = (3, 100, 1e-4, False)
    off = class_run(I, cfg, dtype=np.float64)
    on = class_run(I, cfg, dtype=np.float64, **{option: 1})
    assert on.st["kernel"] not in (None, "loop", "loop_panel")
    assert_same_run(on, off)


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_memory_kinds(gpu, oracle, warm):
    """Host numpy arrays and torch device tensors take one path after the staging copy: equal outputs."""
    import torch
    I = inputs("A")
    cfg = mode(I, warm, 1e-4)
    steps, N, tol, _ = cfg
    host = class_plain(I, cfg)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    s = class_solver(I, to=to)
    batch = I.X0.shape[0]
    X = to(I.X0)
    Z = torch.zeros((batch, I.C.qp.n), device=gpu)
    Y = torch.zeros((batch, I.C.qp.m), device=gpu)
    XS = torch.zeros((steps, batch, I.C.nx), device=gpu)
    US = torch.zeros((steps, batch, I.C.nu), device=gpu)
    IT, CD = np.full(steps * batch, -1, np.int32), np.full(steps * batch, -1, np.int32)
    st = s.closed_loop(X, Z, Y, steps, N, tol, warm=warm, xs=XS, us=US, iters=IT, codes=CD)
    dev = SimpleNamespace(x=X.cpu().numpy(), z=Z.cpu().numpy(), y=Y.cpu().numpy(), xs=XS.cpu().numpy(),
                          us=US.cpu().numpy(), it=IT.reshape(steps, batch), cd=CD.reshape(steps, batch), st=st)
    assert_same_run(dev, host)
    assert_matches_oracle(dev, oracle_ref(oracle, I, cfg))


@pytest.mark.gpu
def test_f64(gpu):
    """One f64 run of A against its f64 shared = 0 reference."""
    I = inputs("A")
    cfg = mode(I, False, 1e-4)
    r = class_run(I, cfg, dtype=np.float64)
    assert r.x.dtype == np.float64
    assert_same_run(r, fleet_ref(I, cfg, np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["sorted", "reversed"])
def test_order_independence(gpu, order):
    """class_of sorted, and reversed, with X0 permuted along: every pack keeps its bits."""
    I = inputs("A")
    cfg = mode(I, False, 1e-4)
    base = class_plain(I, cfg)
    o = np.argsort(I.class_of, kind="stable")
    if order == "reversed":
        o = o[::-1].copy()
    r = class_run(reorder(I, o), cfg)
    for k in ("x", "z", "y"):
        same_bits(getattr(r, k), getattr(base, k)[o], k)
    for k in ("xs", "us", "it", "cd"):
        same_bits(getattr(r, k), getattr(base, k)[:, o], k)
    for k in ("iterations", "converged", "total_iterations"):
        assert r.st[k] == base.st[k]


def _code(fn):
    from gpad_mpc._lib import GpadError
    with pytest.raises(GpadError) as e:
        fn()
    return e.value.code, str(e.value)


@pytest.mark.gpu
def test_unsupported_and_invalid(gpu):
    from gpad_mpc import _lib
    from gpad_mpc._lib import Dims
    I = inputs("A")
    Cq, n, m, batch = I.C.qp, I.C.qp.n, I.C.qp.m, I.X0.shape[0]
    s = class_solver(I)
    lib = s.lib
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    Z, Y = np.zeros((batch, n), np.float32), np.zeros((batch, m), np.float32)
    E = I.E
    calls = dict(
        hessian=lambda: s.setup_hessian(np.eye(n, dtype=np.float32)),
        signals=lambda: s.setup_signals(ns=1),
        run_scaled=lambda: s.run(Z, Y, Z.copy(), Y.copy(), 10, scaled=True),
        plant_batch=lambda: _lib.check(lib.gpad_setup_plant_batch(
            s.h, 3, 3, vp(F32(E.PM)), None, vp(F32(E.Pg)), vp(F32(E.g0)), vp(F32(E.A)), vp(F32(E.B))),
            "gpad_setup_plant_batch"))
    for name, fn in calls.items():
        code, text = _code(fn)
        assert code == _lib.ERR_UNSUPPORTED and "class binding" in text, (name, text)
    # the phase diagnostics have nothing to say
    assert s.phase_plan()["ends"] == [] and s.phase_counts() == [] and s.last_phases()["ends"] == []
    # the binding survived all that
    assert loop(s, I.C, I.X0, 2, 20, 0.0, False).st["iterations"] == 20

    import gpad_mpc
    t = gpad_mpc.GpadSolver(0)
    maps = [vp(F32(I.C.PM)), None, vp(F32(I.C.Pg)), vp(F32(I.C.g0)), vp(F32(I.C.A)), vp(F32(I.C.B))]
    assert lib.gpad_setup_plant_classes(t.h, 3, 3, *maps) == _lib.ERR_NOT_SETUP
    ML, G, L = F32(Cq.ML), F32(Cq.G), _L(Cq, np.float32)
    co = np.ascontiguousarray(I.class_of)
    ip = C.POINTER(C.c_int)

    def bind(class_of, K, **dims):
        d = dict(n=n, m=m, batch=len(class_of), shared=1, dtype=_lib.DTYPE_F32, memory=_lib.MEM_HOST, check_every=10)
        d.update(dims)
        ids = np.ascontiguousarray(class_of, np.int32)
        return lib.gpad_setup_classes(t.h, C.byref(Dims(**d)), K, ids.ctypes.data_as(ip), vp(ML), vp(G), L)
    assert bind(co, 3, shared=0) == _lib.ERR_INVALID
    assert bind(co[:2], 3) == _lib.ERR_INVALID  # K > batch
    assert bind([0, 3, 1, 2], 3) == _lib.ERR_INVALID
    assert bind([0, -1, 1, 2], 3) == _lib.ERR_INVALID
    assert lib.gpad_setup_plant_classes(t.h, 3, 3, *maps) == _lib.ERR_NOT_SETUP  # (nothing was bound)
    assert bind(co, 3) == _lib.GPAD_OK
    assert lib.gpad_setup_plant_classes(t.h, 3, 3, *maps) == _lib.GPAD_OK
    # a run before any plant is bound on a fresh class binding
    u = gpad_mpc.GpadSolver(0)
    u.setup_classes(ML, G, L, I.class_of, n=n, m=m)
    code, _ = _code(lambda: u.run_state(I.X0, Z, Y, 10))
    assert code == _lib.ERR_NOT_SETUP
    code, _ = _code(lambda: u.last_stats())
    assert code == _lib.ERR_NOT_SETUP
    # a stacked plant must lead with K
    with pytest.raises(ValueError):
        u.setup_plant(F32(E.PM), F32(E.Pg), g0=F32(E.g0), A=F32(E.A), B=F32(E.B))


@pytest.mark.gpu
def test_plain_setup_plant_binds_every_class(gpu):
    """gpad_setup_plant on a class handle == gpad_setup_plant_classes with K identical copies (and not
    the per-class plants)."""
    I = inputs("A")
    cfg = mode(I, False, 1e-4)
    steps, N, tol, warm = cfg
    one = {k: None if getattr(I.C, k) is None else getattr(I.C, k)[0] for k in MAPS}
    s1, s2 = class_solver(I), class_solver(I)
    s1.setup_plant(F32(one["PM"]), F32(one["Pg"]), g0=F32(one["g0"]), A=F32(one["A"]), B=F32(one["B"]))
    rep = lambda a: F32(np.stack([a] * I.K))  # noqa: E731
    s2.setup_plant(rep(one["PM"]), rep(one["Pg"]), g0=rep(one["g0"]), A=rep(one["A"]), B=rep(one["B"]))
    r1 = loop(s1, I.C, I.X0, steps, N, tol, warm)
    r2 = loop(s2, I.C, I.X0, steps, N, tol, warm)
    assert_same_run(r1, r2)
    base = class_plain(I, cfg)
    in0 = np.flatnonzero(I.class_of == 0)
    same_bits(r1.us[:, in0], base.us[:, in0], "class 0")
    assert r1.us.tobytes() != base.us.tobytes()


@pytest.mark.gpu
def test_lifecycle(gpu):
    """A plain gpad_setup ends the binding (the handle then equals a fresh one); rebinding classes with
    another class_of equals a fresh handle."""
    from gpad_mpc import _lib
    I = inputs("A")
    cfg = mode(I, False, 1e-4)
    steps, N, tol, warm = cfg
    s = class_solver(I)
    first = loop(s, I.C, I.X0, steps, N, tol, warm)
    assert_same_run(first, class_plain(I, cfg))
    # another class_of on the same handle
    o = np.argsort(I.class_of, kind="stable")[::-1].copy()
    J = reorder(I, o)
    s.setup_classes(F32(J.C.qp.ML), F32(J.C.qp.G), _L(J.C.qp, np.float32), J.class_of, n=J.C.qp.n, m=J.C.qp.m)
    code, _ = _code(lambda: loop(s, J.C, J.X0, steps, N, tol, warm))  # the plant went with the old binding
    assert code == _lib.ERR_NOT_SETUP
    _bind_plant(s, J.C, F32)
    assert_same_run(loop(s, J.C, J.X0, steps, N, tol, warm), class_run(J, cfg))
    # a plain setup: pack 0 as a shared problem for the whole batch
    p = pack(I.E, 0)
    batch = I.X0.shape[0]

    def plain(h):
        h.setup(F32(p.qp.ML), F32(p.qp.G), _L(p.qp, np.float32), n=p.qp.n, m=p.qp.m, batch=batch, shared=True)
        _bind_plant(h, p, F32)
        return loop(h, p, I.X0, steps, N, tol, warm)
    import gpad_mpc
    assert_same_run(plain(s), plain(gpad_mpc.GpadSolver(0)))
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    maps = [vp(F32(I.C.PM)), None, vp(F32(I.C.Pg)), vp(F32(I.C.g0)), vp(F32(I.C.A)), vp(F32(I.C.B))]
    assert s.lib.gpad_setup_plant_classes(s.h, 3, 3, *maps) == _lib.ERR_NOT_SETUP
    # and classes again after the plain problem
    s.setup_classes(F32(I.C.qp.ML), F32(I.C.qp.G), _L(I.C.qp, np.float32), I.class_of, n=I.C.qp.n, m=I.C.qp.m)
    _bind_plant(s, I.C, F32)
    assert_same_run(loop(s, I.C, I.X0, steps, N, tol, warm), first)


@pytest.mark.gpu
def test_last_stats_after_async_run(gpu):
    """A device-memory run without stats is asynchronous; gpad_last_stats then reports the counts of the
    synchronous run, in the caller's order, and gpad_accumulate_iterations their sum."""
    import torch
    I = inputs("A")
    cfg = mode(I, False, 1e-4)
    steps, N, tol, warm = cfg
    sync = class_plain(I, cfg)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    s = class_solver(I, to=to)
    batch = I.X0.shape[0]
    X = to(I.X0)
    Z = torch.zeros((batch, I.C.qp.n), device=gpu)
    Y = torch.zeros((batch, I.C.qp.m), device=gpu)
    assert s.closed_loop(X, Z, Y, steps, N, tol, warm=warm, stats=False) is None
    acc = torch.zeros(1, dtype=torch.int64, device=gpu)
    s.accumulate_iterations(acc)
    IT = np.full(steps * batch, -1, np.int32)
    st = s.last_stats(iters=IT)
    same_bits(IT.reshape(steps, batch), sync.it, "iters")
    for k in ("iterations", "converged", "total_iterations", "tol_floor"):
        assert st[k] == sync.st[k], k
    s.sync()
    assert int(acc.item()) == sync.st["total_iterations"]
    same_bits(X.cpu().numpy(), sync.x, "x")
    same_bits(Z.cpu().numpy(), sync.z, "z")
