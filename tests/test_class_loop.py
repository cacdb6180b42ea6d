"""The fused class loop (gpad_class_loop_fused): gpad_closed_loop of a class-bound handle as one launch of
the class-aware panel loop (csrc/gpad_loop_panel.hip, gpad_loop_panel_kernel<T, true>; the host side in
csrc/gpad_classes.cpp).

The contract is bit identity with what the class binding computes without it: every case is compared
with the class handle with everything off (test_classes.class_plain), with the dims.shared = 0 fleet and
with the CPU oracle, pack by pack -- outputs, trajectories, per-step counts and codes, the aggregate
stats, tol_floor and the flags -- and reports kernel "loop_classes".  A row that landed in another
pack's place or class cannot pass: the tolerance runs' counts are ragged (assert_ragged on the oracle)
and test_classes.test_discrimination_guard shows that another class's matrices change the bits.

Inputs: A, A4 (an empty class), B (n = 40, m = 180: a 12-tile image) and P (16 + 24 packs: one exactly
full panel, one ragged class that needs queue claims) of test_classes.py, and
  Q   A's three classes with 33 packs in classes of 17 / 15 / 1: a one-column panel remainder, a
      class one short of a panel and a single-pack class
Checked on the oracle at eps 1e-4: P and Q cold have at least 6 distinct counts at every step, at most
150 iterations.
  A-M0  A with a constant term M0 per class (class_m0; the battery plants bind none): the per-class M0 offset
        of the binding and the class index of M0 in the fused loop (test_m0_oracle_guard, test_per_class_m0)
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
from test_classes import (MODE_IDS, MODES, _bind_plant, _caps, _L, _make, check_against_references, class_plain,
                          class_run, class_solver, fleet_ref, inputs, mode, oracle_ref, reorder)
from test_loop_async import F32, assert_matches_oracle, assert_same_run, loop, same_bits

FUSED = "loop_classes"


@functools.lru_cache(maxsize=None)
def input_q():
    sizes = (17, 15, 1)
    class_of = np.concatenate([np.full(c, k, np.int32) for k, c in enumerate(sizes)])
    class_of = class_of[np.random.default_rng(41).permutation(class_of.size)]  # the caller's order is not sorted
    return _make("Q", 3, 4, _caps(107, 7, 3)[:3], class_of, 214, 6, 2000, 6)


def get_input(name):
    return input_q() if name == "Q" else inputs(name)


M0_SCALE = 0.5


def class_m0(K, n, scale=M0_SCALE):
    """A constant term M0 per class -- the battery plants bind none, so the per-class M0 offset, its replication
    under per-class signals and the fused loop's M0 index go unread without it."""
    return (scale * np.random.default_rng(31).standard_normal((K, n))).astype(np.float32)


def with_m0(I, M0, tag):
    """Input I of test_classes with the per-class M0 [K][n] (C) and the fleet expanded from it (E)."""
    J = SimpleNamespace(**vars(I))
    J.C = SimpleNamespace(**dict(vars(I.C), M0=M0))
    J.E = SimpleNamespace(**dict(vars(I.E), M0=np.ascontiguousarray(M0[I.class_of])))
    J.name = I.name + "-" + tag
    return J


A_M0_SCALE = 4.0  # (raised from 0.5 on the oracle: at 0.5, 1 and 2 no solve of A reaches N, test_m0_oracle_guard)


def input_am(roll=0):
    """A with class_m0 at A_M0_SCALE, rolled by `roll` classes (the guard's wrong class index)."""
    I = inputs("A")
    M0 = np.roll(class_m0(I.K, I.C.qp.n, A_M0_SCALE), roll, axis=0)
    return with_m0(I, M0, "M0" + ("-roll%d" % roll if roll else ""))


def fused_solver(I, **kw):
    s = class_solver(I, **kw)
    s.set_class_loop_fused(True)
    return s


def fused_run(I, cfg, **kw):
    steps, N, tol, warm = cfg
    dtype = kw.get("dtype", np.float32)
    return loop(fused_solver(I, **kw), I.C, I.X0, steps, N, tol, warm, dtype)


# ------------------------------------------------------------------------------ CPU
def test_symbols():
    """The two entry points and the reported kernel are declared, exported, defined and bound."""
    from gpad_mpc import _lib
    hdr = open(os.path.join(ROOT, "include", "gpad.h")).read()
    state = open(os.path.join(ROOT, "gpu-dualgradient-mpc_amd", "csrc", "gpad_state.cpp")).read()
    assert re.search(r"\bint gpad_class_loop_fused\(gpad_handle_t h, int on\);", hdr)
    assert re.search(r"\bint gpad_class_loop_deal\(const int\* counts, int K, int grid, int\* start_class\);", hdr)
    assert int(re.search(r"#define GPAD_KERNEL_LOOP_CLASSES (\d+)", hdr).group(1)) == 8 == _lib.KERNEL_LOOP_CLASSES
    assert _lib.KERNEL_NAMES[8] == FUSED
    lib = _lib.load()
    for name in ("gpad_class_loop_fused", "gpad_class_loop_deal"):
        assert name in _lib.EXPORTS and name in state
        assert hasattr(lib, name)
    assert not any("fused" in name for name in _lib.OPTIONS)  # a function, not an option
    import gpad_mpc
    assert callable(gpad_mpc.GpadSolver.set_class_loop_fused)


def _deal(counts, K, grid, start=True, give_counts=True):
    from gpad_mpc import _lib
    lib = _lib.load()
    cn = np.ascontiguousarray(counts, np.int32)
    out = np.full(max(grid, 1), -7, np.int32)
    ip = C.POINTER(C.c_int)
    rc = lib.gpad_class_loop_deal(cn.ctypes.data_as(ip) if give_counts else None, K, grid,
                                  out.ctypes.data_as(ip) if start else None)
    return rc, out


def _check_deal(counts, grid):
    from gpad_mpc import _lib
    counts = np.asarray(counts)
    K = counts.size
    rc, start = _deal(counts, K, grid)
    assert rc == _lib.GPAD_OK, (counts, grid)
    panels = (counts + 15) // 16
    assert ((start >= 0) & (start < K)).all() and (counts[start] > 0).all(), (counts, grid, start)
    dealt = np.bincount(start, minlength=K)
    nonempty = np.flatnonzero(counts > 0)
    if grid >= nonempty.size:
        assert (dealt[nonempty] >= 1).all(), (counts, grid, dealt)
    if (dealt[nonempty] == 0).any():  # someone is short: nobody holds more workgroups than panels
        assert (dealt <= panels).all(), (counts, grid, dealt)
    return dealt


def test_class_loop_deal():
    """Every entry a non-empty class; every non-empty class present when the grid allows; no class above its
    panel count while another has none; shares that follow the panel counts; invalid arguments refused."""
    from gpad_mpc import _lib
    fixed = [([11], 1), ([4, 2, 5], 1), ([4, 2, 5], 2), ([4, 2, 5], 3), ([4, 2, 0, 5], 7), ([16, 24], 3),
             ([17, 15, 1], 2), ([17, 15, 1], 4), ([1600, 16], 2), ([1600, 16], 40), ([0, 0, 3], 5),
             ([2048, 2048, 2048, 2048], 40), ([100, 1, 1, 1, 1, 1, 1, 1, 1], 4)]
    for counts, grid in fixed:
        _check_deal(counts, grid)
    assert _check_deal([1600, 16], 2).tolist() == [1, 1]
    assert _check_deal([1600, 16], 40).tolist() == [39, 1]
    assert _check_deal([2048, 2048, 2048, 2048], 40).tolist() == [10, 10, 10, 10]
    assert _check_deal([100, 1, 1, 1, 1, 1, 1, 1, 1], 4).tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0]  # largest, then lowest
    assert _check_deal([16, 160, 32], 1).tolist() == [0, 1, 0]
    rng = np.random.default_rng(43)
    empties = 0
    for _ in range(300):
        K, grid = int(rng.integers(1, 10)), int(rng.integers(1, 41))
        counts = rng.integers(0, 400, K)
        counts[rng.random(K) < 0.25] = 0
        if not counts.any():
            counts[int(rng.integers(0, K))] = int(rng.integers(1, 400))
        empties += int((counts == 0).sum())
        _check_deal(counts, grid)
    assert empties > 0
    ok = [4, 2, 5]
    assert _deal(ok, 3, 4)[0] == _lib.GPAD_OK
    assert _deal(ok, 3, 4, give_counts=False)[0] == _lib.ERR_INVALID
    assert _deal(ok, 3, 4, start=False)[0] == _lib.ERR_INVALID
    assert _deal(ok, 0, 4)[0] == _lib.ERR_INVALID
    assert _deal(ok, 3, 0)[0] == _lib.ERR_INVALID
    assert _deal([4, -1, 5], 3, 4)[0] == _lib.ERR_INVALID
    assert _deal([0, 0, 0], 3, 4)[0] == _lib.ERR_INVALID


def test_fused_without_a_handle():
    """No GPU, no binding: a null handle is an invalid argument, whatever `on` says."""
    from gpad_mpc import _lib
    lib = _lib.load()
    for on in (0, 1, 2):
        assert lib.gpad_class_loop_fused(None, on) == _lib.ERR_INVALID
    assert b"gpad_class_loop_fused" in lib.gpad_last_error()


def assert_m0_guard(I, base, orc, rolled, N, other=None, differ=None, every_step=True):
    """What an input with a per-class M0 must show on the oracle (shared with test_class_signals): M0 changes
    the us bits of every pack against the input without it (base), so does M0 rolled by one class; `other`
    (the one-plant variant) differs in exactly the packs `differ`; every step has at least 5 distinct counts
    (every_step = False: some step, test_m0_oracle_guard); the run holds capped and early solves; everything is
    finite."""
    packs = range(I.class_of.size)
    changed = lambda a, b: np.array([a.us[:, p].tobytes() != b.us[:, p].tobytes() for p in packs])  # noqa: E731
    for k in ("x", "z", "y", "xs", "us"):
        assert np.isfinite(getattr(orc, k)).all(), k
    assert changed(orc, base).all(), np.flatnonzero(~changed(orc, base))
    assert changed(orc, rolled).all(), np.flatnonzero(~changed(orc, rolled))
    if other is not None:
        assert np.array_equal(changed(orc, other), differ), np.flatnonzero(changed(orc, other))
    distinct = [len(set(row)) for row in orc.it.tolist()]
    assert (min if every_step else max)(distinct) >= 5, distinct
    assert (orc.it == N).any() and (orc.it < N).any()


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_m0_oracle_guard(oracle, warm):
    """On the oracle alone, at eps 1e-4: A with class_m0 at A_M0_SCALE = 4 meets assert_m0_guard.  Measured,
    cold: 11 of 11 packs change with M0 and with M0 rolled by one class, 7 to 8 distinct counts at every step,
    1 of the 66 solves capped at N = 2000 (at scales 0.5, 1 and 2 the largest count is 210, 210 and 320: no
    capped solve, so the scale was doubled until one appeared).  Warm: the same 11 of 11 and 1 capped solve, but
    7 distinct counts at step 0 and 1 to 2 afterwards at every scale up to 16 -- without signals nothing
    disturbs a warm loop, whose later steps start at the solution -- so a warm run must show 5 distinct counts
    at some step, the rule test_classes.assert_ragged already has for warm runs."""
    I = inputs("A")
    cfg = mode(I, warm, 1e-4)
    assert_m0_guard(I, oracle_ref(oracle, I, cfg), oracle_ref(oracle, input_am(), cfg),
                    oracle_ref(oracle, input_am(roll=1), cfg), cfg[1], every_step=not warm)


# ------------------------------------------------------------------------------ GPU
M0_MODES = [(False, 1e-4), (True, 1e-4), (False, 0.0)]
M0_MODE_IDS = ["cold-tol", "warm-tol", "cold-fixed"]


@pytest.mark.gpu
@pytest.mark.parametrize("warm,tol", M0_MODES, ids=M0_MODE_IDS)
@pytest.mark.parametrize("fused", [False, True], ids=["classes", "fused"])
def test_per_class_m0(gpu, oracle, fused, warm, tol):
    """A with a per-class M0 (gpad_setup_plant_classes with all six maps): the shared = 0 fleet and the oracle
    bit for bit -- outputs, counts, codes, stats, tol_floor and flags; fused also the class handle with
    everything off.  (The counts reach N here, test_m0_oracle_guard: no assert_ragged.)"""
    I = input_am()
    cfg = mode(I, warm, tol)
    steps, N, _, _ = cfg
    r = fused_run(I, cfg) if fused else class_plain(I, cfg)
    assert (r.st["kernel"] == FUSED) == fused and r.st["kernel_ms"] > 0.0
    if fused:
        assert_same_run(r, class_plain(I, cfg))
    ref, orc = fleet_ref(I, cfg), oracle_ref(oracle, I, cfg)
    assert_same_run(r, ref)
    assert_matches_oracle(r, orc)
    for k in ("tol_floor", "below_tol_floor", "nonfinite_g"):
        assert r.st[k] == ref.st[k], k
    assert r.st["total_iterations"] == int(orc.it.sum()) == int(r.it.sum())
    assert r.st["iterations"] == int(r.it.max()) and r.st["converged"] == int((r.cd != 0).sum())
    if not tol:
        assert (r.it == N).all() and (r.cd == 0).all()


def check_fused(oracle, I, cfg, r):
    """r is a fused run: the class handle with everything off, the shared = 0 fleet and the oracle, bit for
    bit; the stats of the fleet."""
    steps, N, tol, warm = cfg
    assert r.st["kernel"] == FUSED
    assert_same_run(r, class_plain(I, cfg))
    ref, orc = check_against_references(oracle, I, cfg, r)  # (asserts the ragged counts for a tolerance)
    assert r.st["kernel_ms"] > 0.0
    for k in ("tol_floor", "below_tol_floor", "nonfinite_g"):
        assert r.st[k] == ref.st[k], k
    return orc


@pytest.mark.gpu
@pytest.mark.parametrize("warm,tol", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["A", "A4", "B", "P", "Q"])
def test_fused_closed_loop(gpu, oracle, name, warm, tol):
    I = get_input(name)
    cfg = mode(I, warm, tol)
    check_fused(oracle, I, cfg, fused_run(I, cfg))


@pytest.mark.gpu
@pytest.mark.parametrize("warm,tol", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name,grid", [("A", 1), ("A", 2), ("P", 1), ("Q", 2)])
def test_grid_caps(gpu, oracle, name, grid, warm, tol):
    """One workgroup walks every class through switches; two serve three classes; the default grid (the
    case above): the same bits."""
    I = get_input(name)
    cfg = mode(I, warm, tol)
    check_fused(oracle, I, cfg, fused_run(I, cfg, panel_max_grid=grid))


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
    r = fused_run(reorder(I, o), cfg)
    assert r.st["kernel"] == FUSED
    for k in ("x", "z", "y"):
        same_bits(getattr(r, k), getattr(base, k)[o], k)
    for k in ("xs", "us", "it", "cd"):
        same_bits(getattr(r, k), getattr(base, k)[:, o], k)
    for k in ("iterations", "converged", "total_iterations", "tol_floor"):
        assert r.st[k] == base.st[k]


@pytest.mark.gpu
def test_fallback_f64(gpu):
    I = inputs("A")
    cfg = (3, 100, 1e-4, False)
    off = class_run(I, cfg, dtype=np.float64)
    on = fused_run(I, cfg, dtype=np.float64)
    assert on.st["kernel"] not in (None, FUSED) and on.st["kernel"] == off.st["kernel"]
    assert_same_run(on, off)


@pytest.mark.gpu
def test_fallback_limit_off_the_test_period(gpu):
    """tol > 0 with N no multiple of check_every: the per-class path, its kernel, its bits."""
    I = inputs("A")
    cfg = (I.steps, I.Ntol + 3, 1e-4, False)
    off = class_run(I, cfg)
    on = fused_run(I, cfg)
    assert on.st["kernel"] not in (None, FUSED) and on.st["kernel"] == off.st["kernel"]
    assert_same_run(on, off)


@pytest.mark.gpu
@pytest.mark.parametrize("tol", [0.0, 1e-4], ids=["fixed", "tol"])
def test_fallback_run_state(gpu, tol):
    """gpad_run_state (no loop) on a handle with the fused loop on."""
    I = inputs("A")
    batch, n, m = I.X0.shape[0], I.C.qp.n, I.C.qp.m
    N = 300 if tol else 60
    outs = []
    for s in (class_solver(I), fused_solver(I)):
        Z, Y = np.zeros((batch, n), np.float32), np.zeros((batch, m), np.float32)
        st = s.run_state(I.X0, Z, Y, N, tol)
        outs.append((Z, Y, st))
    (Z0, Y0, st0), (Z1, Y1, st1) = outs
    assert st1["kernel"] not in (None, FUSED) and st1["kernel"] == st0["kernel"]
    same_bits(Z1, Z0, "z")
    same_bits(Y1, Y0, "y")
    for k in ("iterations", "converged", "total_iterations", "tol_floor"):
        assert st1[k] == st0[k], k


@pytest.mark.gpu
def test_lifecycle(gpu, oracle):
    import gpad_mpc
    from gpad_mpc import _lib
    I = inputs("A")
    cfg = mode(I, False, 1e-4)
    steps, N, tol, warm = cfg
    plain = gpad_mpc.GpadSolver(0)
    assert plain.lib.gpad_class_loop_fused(plain.h, 1) == _lib.ERR_NOT_SETUP
    p = I.C.qp
    plain.setup(F32(p.ML[0]), F32(p.G[0]), _L(p, np.float32), n=p.n, m=p.m, batch=4, shared=True)
    assert plain.lib.gpad_class_loop_fused(plain.h, 1) == _lib.ERR_NOT_SETUP
    with pytest.raises(_lib.GpadError):
        plain.set_class_loop_fused(True)
    s = class_solver(I)
    assert s.lib.gpad_class_loop_fused(s.h, 2) == _lib.ERR_INVALID
    assert s.lib.gpad_class_loop_fused(s.h, -1) == _lib.ERR_INVALID
    base = class_plain(I, cfg)
    assert loop(s, I.C, I.X0, steps, N, tol, warm).st["kernel"] != FUSED  # off by default
    s.set_class_loop_fused(True)
    first = loop(s, I.C, I.X0, steps, N, tol, warm)
    second = loop(s, I.C, I.X0, steps, N, tol, warm)
    assert first.st["kernel"] == second.st["kernel"] == FUSED
    assert_same_run(first, base)
    assert_same_run(second, first)
    s.set_class_loop_fused(False)
    third = loop(s, I.C, I.X0, steps, N, tol, warm)
    assert third.st["kernel"] == base.st["kernel"]
    assert_same_run(third, first)
    s.set_class_loop_fused(True)
    assert loop(s, I.C, I.X0, steps, N, tol, warm).st["kernel"] == FUSED
    # the plant rebound while the loop is on: the new maps reach the fused launch
    one = {k: getattr(I.C, k)[0] for k in ("PM", "Pg", "g0", "A", "B")}
    s.setup_plant(F32(one["PM"]), F32(one["Pg"]), g0=F32(one["g0"]), A=F32(one["A"]), B=F32(one["B"]))
    t = class_solver(I)
    t.setup_plant(F32(one["PM"]), F32(one["Pg"]), g0=F32(one["g0"]), A=F32(one["A"]), B=F32(one["B"]))
    same_maps = loop(s, I.C, I.X0, steps, N, tol, warm)
    assert same_maps.st["kernel"] == FUSED
    assert_same_run(same_maps, loop(t, I.C, I.X0, steps, N, tol, warm))
    assert same_maps.us.tobytes() != base.us.tobytes()
    # a rebinding clears it
    s.setup_classes(F32(p.ML), F32(p.G), _L(p, np.float32), I.class_of, n=p.n, m=p.m)
    _bind_plant(s, I.C, F32)
    again = loop(s, I.C, I.X0, steps, N, tol, warm)
    assert again.st["kernel"] == base.st["kernel"]
    assert_same_run(again, base)
    # switched on before the plant is bound
    u = gpad_mpc.GpadSolver(0)
    u.setup_classes(F32(p.ML), F32(p.G), _L(p, np.float32), I.class_of, n=p.n, m=p.m)
    u.set_class_loop_fused(True)
    _bind_plant(u, I.C, F32)
    early = loop(u, I.C, I.X0, steps, N, tol, warm)
    assert early.st["kernel"] == FUSED
    assert_same_run(early, base)


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_memory_kinds(gpu, oracle, warm):
    """Torch device tensors against host arrays; then the same run without stats (asynchronous), after which
    gpad_last_stats reports the same counts and codes and gpad_accumulate_iterations their sum."""
    import torch
    I = input_q()
    cfg = mode(I, warm, 1e-4)
    steps, N, tol, _ = cfg
    host = class_plain(I, cfg)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    s = fused_solver(I, to=to)
    batch = I.X0.shape[0]

    def arrays():
        return (to(I.X0), torch.zeros((batch, I.C.qp.n), device=gpu), torch.zeros((batch, I.C.qp.m), device=gpu),
                torch.zeros((steps, batch, I.C.nx), device=gpu), torch.zeros((steps, batch, I.C.nu), device=gpu))
    X, Z, Y, XS, US = arrays()
    IT, CD = np.full(steps * batch, -1, np.int32), np.full(steps * batch, -1, np.int32)
    st = s.closed_loop(X, Z, Y, steps, N, tol, warm=warm, xs=XS, us=US, iters=IT, codes=CD)
    dev = SimpleNamespace(x=X.cpu().numpy(), z=Z.cpu().numpy(), y=Y.cpu().numpy(), xs=XS.cpu().numpy(),
                          us=US.cpu().numpy(), it=IT.reshape(steps, batch), cd=CD.reshape(steps, batch), st=st)
    assert st["kernel"] == FUSED
    assert_same_run(dev, host)
    assert_matches_oracle(dev, oracle_ref(oracle, I, cfg))

    X, Z, Y, XS, US = arrays()
    assert s.closed_loop(X, Z, Y, steps, N, tol, warm=warm, xs=XS, us=US, stats=False) is None
    acc = torch.zeros(1, dtype=torch.int64, device=gpu)
    s.accumulate_iterations(acc)
    IT2, CD2 = np.full(steps * batch, -1, np.int32), np.full(steps * batch, -1, np.int32)
    st2 = s.last_stats(iters=IT2, codes=CD2)
    same_bits(IT2.reshape(steps, batch), host.it, "iters")
    same_bits(CD2.reshape(steps, batch), host.cd, "codes")
    assert st2["kernel"] == FUSED
    for k in ("iterations", "converged", "total_iterations", "tol_floor"):
        assert st2[k] == host.st[k], k
    s.sync()
    assert int(acc.item()) == host.st["total_iterations"]
    for k, v in (("x", X), ("z", Z), ("y", Y), ("xs", XS), ("us", US)):
        same_bits(v.cpu().numpy(), getattr(host, k), k)
