"""Closed loops for fleets of distinct plants: per-instance plant maps (gpad_setup_plant_batch) on
the lockstep path (csrc/gpad_plant.hip strides) and in the asynchronous loop kernel
(csrc/gpad_loop.h: the two-slot kernel with a per-pack plant, gpad_loop_fleet_kernel for per-pack
matrices).

The contract is bit identity with code that predates the feature: a batch of B distinct plants
equals (a) B separate batch-1 handles, each bound with gpad_setup (shared) + gpad_setup_plant and
run with the option off, and (b) the CPU oracle's closed loop of every pack with that pack's
matrices and maps and the common L.  x, z, y, xs, us, the per-step counts and codes are compared
with same_bits; the aggregate stats equal the sums and maxima of (a).  The references of a
configuration are computed once and shared by the cases that vary only the path or the grid.
"""
from __future__ import annotations

import functools
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import test_loop_async as T
from conftest import ROOT
from test_loop_async import F32, F64, assert_matches_oracle, assert_same_run, same_bits

MAPS = ("PM", "Pg", "M0", "g0", "A", "B")


# ------------------------------------------------------------------------------ problems
# fleet -> (packs, rng of the capacities and X0 seed, steps, N with a tolerance)
FLEETS = {(3, 4): (7, 107, 7, 6, 2000), (4, 10): (5, 105, 5, 4, 3000)}


def _ns(qp, maps, nx, nu, X0):
    return SimpleNamespace(qp=qp, nx=nx, nu=nu, X0=X0, **maps)


@functools.lru_cache(maxsize=None)
def fleet(n_u, Nh):
    """The battery fleet of the issue: unequal cell capacities, so every pack has its own ML, G, PM
    and B; one L (the maximum)."""
    from gpad_mpc import problems
    packs, rng, xseed, _, _ = FLEETS[(n_u, Nh)]
    caps = 0.027 * 4.1 * np.random.default_rng(rng).uniform(0.6, 1.4, (packs, n_u))
    qp, pl = problems.battery_fleet(n_u, Nh, caps)
    X0 = (np.random.default_rng(xseed).random((packs, n_u)) - 0.5).astype(np.float32)
    return _ns(qp, dict(PM=pl.PM, Pg=pl.Pg, M0=None, g0=pl.g0, A=pl.A, B=pl.B), n_u, n_u, X0)


@functools.lru_cache(maxsize=None)
def mismatch(n_u, Nh):
    """One controller (ML, G, PM of pack 0, shared matrices) against the true A, B, Pg, g0 of every
    pack of fleet(n_u, Nh)."""
    f = fleet(n_u, Nh)
    packs = f.X0.shape[0]
    qp = SimpleNamespace(ML=f.qp.ML[0], G=f.qp.G[0], L=f.qp.L, n=f.qp.n, m=f.qp.m)
    return _ns(qp, dict(PM=np.stack([f.PM[0]] * packs), Pg=f.Pg, M0=None, g0=f.g0, A=f.A, B=f.B), n_u, n_u, f.X0)


SYNTH_SEED = 40  # synthetic_fleet: the oracle is finite and under N = 1500 on every pack (asserted)


@functools.lru_cache(maxsize=None)
def synthetic_fleet(n, m, nx, nu, packs=6, seed=SYNTH_SEED):
    """Per-pack synthetic QPs (own ML, G; one L) with per-pack plants drawn as test_loop_async.synthetic
    draws its one: both constant terms bound, nx != nu, a contracting A; one rng per pack."""
    from gpad_mpc import problems
    qp = problems.synthetic_qp(n, m, batch=packs, seed=seed, shared=False)
    d = {k: [] for k in ("PM", "Pg", "A", "B", "X0")}
    for b in range(packs):
        rng = np.random.default_rng([11, b])
        d["PM"].append(0.1 * rng.standard_normal((n, nx)))
        d["Pg"].append(0.05 * rng.standard_normal((m, nx)))
        Q, _ = np.linalg.qr(rng.standard_normal((nx, nx)))
        d["A"].append(0.9 * Q)
        d["B"].append(0.1 * rng.standard_normal((nx, nu)))
        d["X0"].append(rng.uniform(-1, 1, nx))
    d = {k: np.stack(v) for k, v in d.items()}
    X0 = d.pop("X0").astype(np.float32)
    return _ns(qp, dict(M0=qp.M, g0=qp.g, **d), nx, nu, X0)


def is_fleet(F):
    return F.qp.ML.ndim == 3


def pack(F, b, matrices=None, maps=None):
    """Pack b as a one-plant problem (test_loop_async's shape); `matrices` / `maps`: take those of
    another pack instead (the discrimination guard)."""
    mb = b if matrices is None else matrices
    pb = b if maps is None else maps
    ML, G = (F.qp.ML[mb], F.qp.G[mb]) if is_fleet(F) else (F.qp.ML, F.qp.G)
    qp = SimpleNamespace(ML=ML, G=G, L=F.qp.L, n=F.qp.n, m=F.qp.m)
    one = {k: None if getattr(F, k) is None else getattr(F, k)[pb] for k in MAPS}
    return _ns(qp, one, F.nx, F.nu, F.X0[b:b + 1])


def take(F, count):
    """The first `count` packs of F."""
    qp = F.qp
    if is_fleet(F):
        qp = SimpleNamespace(ML=qp.ML[:count], G=qp.G[:count], L=qp.L, n=qp.n, m=qp.m)
    return _ns(qp, {k: None if getattr(F, k) is None else getattr(F, k)[:count] for k in MAPS}, F.nx, F.nu,
               F.X0[:count])


# ------------------------------------------------------------------------------ runs
def make_solver(F, dtype=np.float32):
    """One handle for the whole batch: per-instance matrices when F is a fleet, stacked plant maps."""
    import gpad_mpc
    c = F64 if dtype == np.float64 else F32
    qp = F.qp
    L = float(qp.L) if dtype == np.float64 else float(np.float32(qp.L))
    s = gpad_mpc.GpadSolver(0)
    s.setup(c(qp.ML), c(qp.G), L, n=qp.n, m=qp.m, batch=F.X0.shape[0], shared=not is_fleet(F))
    opt = lambda a: None if a is None else c(a)  # noqa: E731
    s.setup_plant(c(F.PM), c(F.Pg), M0=opt(F.M0), g0=opt(F.g0), A=c(F.A), B=c(F.B))
    return s


def run(F, steps, N, tol, warm, *, async_=False, grid=0, dtype=np.float32):
    s = make_solver(F, dtype)
    if async_:
        s.set_option("loop_async", 1)
    if grid:
        s.set_option("duo_max_grid", grid)
    return T.loop(s, F, F.X0, steps, N, tol, warm, dtype)


_cache = {}


def cached(kind, key, cfg, make):
    k = (kind, key) + tuple(cfg)
    if k not in _cache:
        _cache[k] = make()
    return _cache[k]


def singles(key, F, steps, N, tol, warm, dtype=np.float32):
    """Reference (a): every pack on its own batch-1 handle, gpad_setup (shared) + gpad_setup_plant,
    the option off -- the parent commit's code.  Stats aggregated as one batch would report them."""
    def make():
        rs = []
        for b in range(F.X0.shape[0]):
            p = pack(F, b)
            rs.append(T.loop(T.make_solver(p, 1, dtype=dtype), p, p.X0, steps, N, tol, warm, dtype))
            assert rs[-1].st["kernel"] != "loop"
        cat = lambda k, ax: np.concatenate([getattr(r, k) for r in rs], axis=ax)  # noqa: E731
        st = dict(iterations=max(r.st["iterations"] for r in rs), converged=sum(r.st["converged"] for r in rs),
                  total_iterations=sum(r.st["total_iterations"] for r in rs),
                  below_tol_floor=any(r.st["below_tol_floor"] for r in rs),
                  nonfinite_g=any(r.st["nonfinite_g"] for r in rs),
                  tol_floor=max(r.st["tol_floor"] for r in rs))
        return SimpleNamespace(x=cat("x", 0), z=cat("z", 0), y=cat("y", 0), xs=cat("xs", 1), us=cat("us", 1),
                               it=cat("it", 1), cd=cat("cd", 1), st=st)
    return cached("singles", key, (steps, N, tol, warm, np.dtype(dtype).name), make)


def oracle_pack(oracle, p, steps, N, tol, warm):
    L = np.float32(p.qp.L)
    MGneg, GL, _ = oracle.scale(F32(p.qp.ML), F32(p.qp.G), F32(np.zeros(p.qp.m)), L)
    return oracle.closed_loop_f32(p.X0[0], MGneg, GL, L, p.PM, p.Pg, p.A, p.B, steps, N, tol, M0=p.M0, g0=p.g0,
                                  warm=warm)


def stack_rows(rows):
    return SimpleNamespace(
        x=np.stack([r[0] for r in rows]), z=np.stack([r[1] for r in rows]), y=np.stack([r[2] for r in rows]),
        xs=np.stack([r[3] for r in rows], axis=1), us=np.stack([r[4] for r in rows], axis=1),
        it=np.stack([r[5] for r in rows], axis=1))


def oracle_fleet(oracle, key, F, steps, N, tol, warm):
    """Reference (b): the CPU oracle's closed loop, pack by pack, each with its own matrices and maps."""
    return cached("oracle", key, (steps, N, tol, warm), lambda: stack_rows(
        [oracle_pack(oracle, pack(F, b), steps, N, tol, warm) for b in range(F.X0.shape[0])]))


def lockstep_fleet(key, F, steps, N, tol, warm):
    def make():
        r = run(F, steps, N, tol, warm)
        assert r.st["kernel"] != "loop"
        return r
    return cached("lockstep", key, (steps, N, tol, warm), make)


def assert_ragged(orc, N):
    """The packs are really ragged (a flat input cannot hide a scheduling error): some step with
    >= 3 distinct counts, unequal totals, every solve under the cap."""
    assert max(len(set(row)) for row in orc.it.tolist()) >= 3
    assert len(set(orc.it.sum(axis=0).tolist())) > 1
    assert orc.it.max() < N


def check_lockstep(oracle, key, F, steps, N, tol, warm):
    orc = oracle_fleet(oracle, key, F, steps, N, tol, warm)
    ref = singles(key, F, steps, N, tol, warm)
    r = lockstep_fleet(key, F, steps, N, tol, warm)
    assert_same_run(r, ref)
    assert_matches_oracle(r, orc)
    return r, orc


def check_async(oracle, key, F, steps, N, tol, warm, grid):
    orc = oracle_fleet(oracle, key, F, steps, N, tol, warm)
    ref = lockstep_fleet(key, F, steps, N, tol, warm)
    r = run(F, steps, N, tol, warm, async_=True, grid=grid)
    assert r.st["kernel"] == "loop"
    assert_same_run(r, ref)
    assert_matches_oracle(r, orc)
    assert r.st["total_iterations"] == int(orc.it.sum())
    return r, orc


# ------------------------------------------------------------------------------ CPU
def test_symbol_and_version():
    """gpad_setup_plant_batch is declared and exported; 0.6 in the header, the library and _lib."""
    from gpad_mpc import _lib
    hdr = open(os.path.join(ROOT, "include", "gpad.h")).read()
    assert re.search(r"\bint gpad_setup_plant_batch\(gpad_handle_t h, int nx, int nu,", hdr)
    assert "gpad_setup_plant_batch" in _lib.EXPORTS
    assert int(re.search(r"#define GPAD_VERSION_MINOR (\d+)", hdr).group(1)) == 6 == _lib.VERSION_MINOR
    csrc = os.path.join(ROOT, "gpu-dualgradient-mpc_amd", "csrc")
    host = open(os.path.join(csrc, "gpad_host.cpp")).read()
    assert re.search(r'gpad_version\(void\) \{ return "gpad-mi355x 0\.6 ', host)
    assert "gpad_setup_plant_batch" in open(os.path.join(csrc, "gpad_state.cpp")).read()


def test_equal_capacities_reproduce_battery_plant():
    from gpad_mpc import problems
    qp, pl = problems.battery_plant(3, 4)
    fq, fp = problems.battery_fleet(3, 4, np.full((2, 3), 0.027 * 4.1))
    for b in range(2):
        for k in ("ML", "M", "G", "g", "H", "q"):
            same_bits(getattr(fq, k)[b], getattr(qp, k), k)
        for k in ("PM", "Pg", "g0", "A", "B"):
            same_bits(getattr(fp, k)[b], getattr(pl, k), k)
    assert fp.M0 is None and fq.L == qp.L and (fp.nx, fp.nu, fq.n, fq.m) == (3, 3, 12, 56)


def test_unequal_capacities_differ():
    from gpad_mpc import problems
    caps = problems.battery_fleet_caps(7, 3, 107)
    same_bits(caps, 0.027 * 4.1 * np.random.default_rng(107).uniform(0.6, 1.4, (7, 3)), "caps")
    f = fleet(3, 4)
    same_bits(f.B, np.stack([np.diag(-1.0 / (3600.0 * c)) for c in caps]), "B")
    for b in range(1, 7):
        for k, a in (("ML", f.qp.ML), ("PM", f.PM), ("B", f.B)):
            assert not np.array_equal(F32(a[b]), F32(a[0])), (k, b)
    assert f.qp.L == max(problems.battery_plant(3, 4, capacity_ah=c)[0].L for c in caps)
    with pytest.raises(ValueError):
        problems.battery_fleet(3, 4, caps[:, :2])


def test_discrimination_guard(oracle):
    """On the oracle alone: pack b of the (3, 4) fleet run with pack 0's matrices, or with pack 0's
    plant maps, gives other us and x bits -- so a kernel that ignored the matrix strides or the plant
    strides could not pass the comparisons below."""
    F = fleet(3, 4)
    _, _, _, steps, N = FLEETS[(3, 4)]
    for b in range(1, F.X0.shape[0]):
        own = oracle_pack(oracle, pack(F, b), steps, N, 1e-4, False)
        for other in (pack(F, b, matrices=0), pack(F, b, maps=0)):
            got = oracle_pack(oracle, other, steps, N, 1e-4, False)
            assert got[0].tobytes() != own[0].tobytes(), b  # x
            assert got[4].tobytes() != own[4].tobytes(), b  # us


# ------------------------------------------------------------------------------ GPU
MODES = [(False, 0.0), (False, 1e-4), (True, 0.0), (True, 1e-4)]
MODE_IDS = ["cold-fixed", "cold-tol", "warm-fixed", "warm-tol"]


def cfg(key, tol):
    _, _, _, steps, Ntol = FLEETS[key]
    return steps, (Ntol if tol else 100)


@pytest.mark.gpu
@pytest.mark.parametrize("warm,tol", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("key", sorted(FLEETS), ids=["b3x4", "b4x10"])
def test_fleet_lockstep(gpu, oracle, key, warm, tol):
    """shared = 0 with a stacked plant, option off == B batch-1 handles == oracle (the per-map strides
    of affine2_kernel / plant_step_kernel)."""
    steps, N = cfg(key, tol)
    r, orc = check_lockstep(oracle, key, fleet(*key), steps, N, tol, warm)
    if tol:
        assert_ragged(orc, N)
    else:
        assert (r.it == N).all() and (r.cd == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [0, 2], ids=["grid0", "grid2"])
@pytest.mark.parametrize("warm,tol", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("key", sorted(FLEETS), ids=["b3x4", "b4x10"])
def test_fleet_async(gpu, oracle, key, warm, tol, grid):
    """The fleet kernel == lockstep fleet == oracle.  The default grid gives every pack a workgroup;
    2 workgroups give queue claims with a row reload each and an odd tail (7 and 5 packs)."""
    steps, N = cfg(key, tol)
    _, orc = check_async(oracle, key, fleet(*key), steps, N, tol, warm, grid)
    if tol:
        assert_ragged(orc, N)


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(FLEETS), ids=["b3x4", "b4x10"])
def test_fleet_batch_of_one(gpu, oracle, key):
    steps, N = cfg(key, 1e-4)
    F = take(fleet(*key), 1)
    check_lockstep(oracle, (key, 1), F, steps, N, 1e-4, False)
    check_async(oracle, (key, 1), F, steps, N, 1e-4, False, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_fleet_two_ml_waves(gpu, oracle, warm):
    """n = 70 (two -ML waves), m = 130, six packs with their own matrices and their own PM, Pg, M0, g0,
    A, B (nx = 5 != nu = 2), two workgroups."""
    F = synthetic_fleet(70, 130, 5, 2)
    orc = oracle_fleet(oracle, "s70", F, 5, 1500, 1e-4, warm)
    assert all(np.isfinite(getattr(orc, k)).all() for k in ("x", "z", "y", "xs", "us")) and orc.it.max() < 1500
    check_lockstep(oracle, "s70", F, 5, 1500, 1e-4, warm)
    check_async(oracle, "s70", F, 5, 1500, 1e-4, warm, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("async_", [False, True], ids=["lockstep", "async"])
@pytest.mark.parametrize("warm,tol", MODES, ids=MODE_IDS)
def test_shared_matrices_per_pack_plant(gpu, oracle, warm, tol, async_):
    """Plant/model mismatch: the controller of pack 0 (shared matrices) against every pack's true
    plant, on the lockstep path and in the two-slot kernel over 2 workgroups == B batch-1 handles ==
    oracle."""
    key = (3, 4)
    steps, N = cfg(key, tol)
    F = mismatch(*key)
    assert not is_fleet(F)
    r, orc = check_lockstep(oracle, "mismatch", F, steps, N, tol, warm)
    assert len({orc.us[:, b].tobytes() for b in range(F.X0.shape[0])}) == F.X0.shape[0]
    if async_:
        check_async(oracle, "mismatch", F, steps, N, tol, warm, 2)


@pytest.mark.gpu
def test_run_state_per_pack_maps(gpu):
    """gpad_run_state forms M(x), g(x) from each pack's own maps: == the batch-1 handles."""
    F = synthetic_fleet(70, 130, 5, 2)
    batch = F.X0.shape[0]

    def solve(s, X, b):
        Z = np.zeros((b, F.qp.n), np.float32)
        Y = np.zeros((b, F.qp.m), np.float32)
        st = s.run_state(X, Z, Y, 300, 1e-4)
        return Z, Y, st
    Z, Y, st = solve(make_solver(F), F.X0, batch)
    ones = []
    for b in range(batch):
        p = pack(F, b)
        ones.append(solve(T.make_solver(p, 1), p.X0, 1))
    same_bits(Z, np.concatenate([o[0] for o in ones]), "z")
    same_bits(Y, np.concatenate([o[1] for o in ones]), "y")
    assert st["total_iterations"] == sum(o[2]["total_iterations"] for o in ones)
    assert st["iterations"] == max(o[2]["iterations"] for o in ones)
    assert len({o[0].tobytes() for o in ones}) == batch


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["f64", "n300"])
def test_fleet_fallbacks(gpu, case):
    """Where the loop kernel does not apply the option is accepted and the lockstep loop runs."""
    if case == "n300":
        F, dtype = synthetic_fleet(300, 64, 3, 2, packs=2, seed=1), np.float32
    else:
        F, dtype = fleet(3, 4), np.float64
    ref = singles(case, F, 2, 50, 0.0, False, dtype)
    r = run(F, 2, 50, 0.0, False, async_=True, dtype=dtype)
    assert r.st["kernel"] not in (None, "loop")
    assert_same_run(r, ref)


@pytest.mark.gpu
def test_validation(gpu):
    from gpad_mpc import _lib
    from gpad_mpc._lib import GpadError
    F = fleet(3, 4)
    s = make_solver(F)
    # a plant bound for another batch: NOT_SETUP at run, until a plant is bound again
    sub = take(F, 3)
    s.setup(F32(sub.qp.ML), F32(sub.qp.G), float(np.float32(F.qp.L)), n=F.qp.n, m=F.qp.m, batch=3, shared=False)
    with pytest.raises(GpadError) as e:
        T.loop(s, sub, sub.X0, 2, 20, 0.0, False)
    assert e.value.code == _lib.ERR_NOT_SETUP
    with pytest.raises(GpadError) as e:
        s.run_state(sub.X0, np.zeros((3, F.qp.n), np.float32), np.zeros((3, F.qp.m), np.float32), 20)
    assert e.value.code == _lib.ERR_NOT_SETUP
    s.setup_plant(F32(sub.PM), F32(sub.Pg), g0=F32(sub.g0), A=F32(sub.A), B=F32(sub.B))
    assert T.loop(s, sub, sub.X0, 2, 20, 0.0, False).st["iterations"] == 20
    # A without B; nu > n
    with pytest.raises(GpadError) as e:
        s.setup_plant(F32(sub.PM), F32(sub.Pg), g0=F32(sub.g0), A=F32(sub.A))
    assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(GpadError) as e:
        s.setup_plant(F32(sub.PM), F32(sub.Pg), A=F32(sub.A), B=F32(np.zeros((3, 3, F.qp.n + 1))))
    assert e.value.code == _lib.ERR_INVALID
    # a stacked PM wants every array stacked, for the batch of the setup
    with pytest.raises(ValueError):
        s.setup_plant(F32(sub.PM), F32(sub.Pg), g0=F32(sub.g0[0]), A=F32(sub.A), B=F32(sub.B))
    with pytest.raises(ValueError):
        s.setup_plant(F32(sub.PM), F32(sub.Pg), A=F32(sub.A[0]), B=F32(sub.B))
    with pytest.raises(ValueError):
        s.setup_plant(F32(F.PM), F32(F.Pg), A=F32(F.A), B=F32(F.B))


@pytest.mark.gpu
def test_handle_reuse(gpu):
    """Async fleet, a shared plant bound with gpad_setup_plant on the same handle, the fleet again:
    the first and third runs are identical (queue counter, row registers), and the second ran pack
    0's maps for every pack."""
    F = fleet(3, 4)
    steps, N = cfg((3, 4), 1e-4)
    s = make_solver(F)
    s.set_options(loop_async=1, duo_max_grid=2)
    first = T.loop(s, F, F.X0, steps, N, 1e-4, False)
    s.setup_plant(F32(F.PM[0]), F32(F.Pg[0]), g0=F32(F.g0[0]), A=F32(F.A[0]), B=F32(F.B[0]))
    second = T.loop(s, F, F.X0, steps, N, 1e-4, False)
    s.setup_plant(F32(F.PM), F32(F.Pg), g0=F32(F.g0), A=F32(F.A), B=F32(F.B))
    third = T.loop(s, F, F.X0, steps, N, 1e-4, False)
    assert [r.st["kernel"] for r in (first, second, third)] == ["loop"] * 3
    assert_same_run(third, first)
    same_bits(second.us[:, :1], first.us[:, :1], "pack 0")
    assert second.us[:, 1:].tobytes() != first.us[:, 1:].tobytes()
    assert_same_run(first, lockstep_fleet((3, 4), F, steps, N, 1e-4, False))
