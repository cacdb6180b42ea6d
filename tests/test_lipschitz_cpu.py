"""gpad_lipschitz_host (include/gpad.h): the upper bound of lambda_max(G ML) by repeated squaring, on the CPU.

Reference lam, fp64 numpy: for ML = H^-1 G' the largest eigenvalue (eigvalsh) of the symmetrised G ML; for a
general pair max |eigvals(G ML)|.  The estimate must never lie below lam (GPAD may diverge with L < lam) and,
on the positive semi-definite pairs, never above (1 + rtol) lam.  lam itself carries numpy's rounding, of
order 1e-15 relative; the estimate is rounded up by 1e-9 relative, so `L >= lam` needs no slack.

The end-to-end case pins the inputs of tests/test_lipschitz.py's GPU loops and holds the point of the feature:
on the C1 battery plant the estimate at most halves the total iteration count of the fp64 reference loop
(measured: 2100 / 6660 = 0.32 cold, 640 / 1630 = 0.39 warm).  The cap of 0.5 is a condition: a regression to a
loose bound (||H||_F^2 is 4.03 lam here) must not pass.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import pytest

import loop_ref64 as R

RTOLS = (0.01, 0.5)
BATTERY = [(1, 1), (2, 3), (4, 10), (10, 4)]
SYNTH = [(16, 16), (17, 33), (33, 17), (5, 3), (64, 257), (200, 200)]
PSD = [("battery",) + s for s in BATTERY] + [("synth",) + s for s in SYNTH]
GENERAL = ("random", 12, 20)
IDS = lambda c: "%s-%dx%d" % c  # noqa: E731

# the loop both files run: problems.battery_plant(4, 10) (C1: n = 40, m = 180), 4 packs, 6 steps
LOOP = SimpleNamespace(plant=(4, 10), packs=4, seed=11, span=0.45, steps=6, N=3000, eps=1e-4, cap=0.5)


@functools.lru_cache(maxsize=None)
def pair(case):
    """(ML, G, lam) of a case, fp64."""
    from gpad_mpc import problems
    kind, a, b = case
    if kind == "battery":
        qp = problems.battery_mpc(a, b, seed=0)
    elif kind == "synth":
        qp = problems.synthetic_qp(a, b, batch=1, seed=400)
    else:  # no structure at all: the upper bound still holds, its tightness is not promised
        rng = np.random.default_rng(7)
        ML, G = rng.standard_normal((a, b)), rng.standard_normal((b, a))
        return ML, G, float(np.abs(np.linalg.eigvals(G @ ML)).max())
    ML, G = np.ascontiguousarray(qp.ML, np.float64), np.ascontiguousarray(qp.G, np.float64)
    return ML, G, lam_psd(ML, G)


def lam_psd(ML, G):
    S = G @ ML
    return float(np.linalg.eigvalsh(0.5 * (S + S.T)).max())


def lam_general(ML, G):
    ML, G = np.asarray(ML, np.float64), np.asarray(G, np.float64)
    return float(np.abs(np.linalg.eigvals(ML @ G if ML.shape[0] <= ML.shape[1] else G @ ML)).max())


def bits(x):
    return np.asarray(x, np.float64).tobytes()


@pytest.mark.parametrize("case", PSD + [GENERAL], ids=IDS)
def test_upper_bound(case):
    """L >= lam on every shape, for both squaring counts; on the PSD pairs also L <= (1 + rtol) lam."""
    import gpad_mpc
    ML, G, lam = pair(case)
    assert ML.shape == case[1:] or case[0] == "battery"
    assert lam > 0
    Ls = [gpad_mpc.lipschitz_host(ML, G, rtol=r) for r in RTOLS]
    print(case, "lam %.6g" % lam, ["%.3e" % (L / lam - 1) for L in Ls])
    for r, L in zip(RTOLS, Ls):
        assert L >= lam, (r, L, lam)
        if case != GENERAL:
            assert L <= (1 + r) * lam, (r, L / lam - 1)
    assert Ls[0] <= Ls[1]  # more squarings never loosen the bound
    assert gpad_mpc.lipschitz_host(ML, G) == Ls[0]  # the default rtol is 0.01 ...
    assert gpad_mpc.lipschitz_host(ML, G, rtol=0.0) == Ls[0]  # ... and so is rtol = 0


def test_lam_of_the_table():
    """The shapes behind the figures of README "A tight step bound": lam of C1 is 9.998 against L_ref = 40.28."""
    from gpad_mpc import problems
    ML, G, lam = pair(("battery", 4, 10))
    assert ML.shape == (40, 180)
    assert abs(lam - 9.998) < 1e-3
    assert abs(problems.battery_mpc(4, 10, seed=0).L / lam - 4.03) < 0.01


@pytest.mark.parametrize("case", [("synth", 17, 33), ("synth", 33, 17), ("battery", 4, 10)], ids=IDS)
def test_f32_inputs(case):
    """f32 operands are widened on load: the result is the bound of the rounded matrices, bit for bit the fp64
    call on their widened copies, and an upper bound of their own spectral radius."""
    import gpad_mpc
    ML, G, _ = pair(case)
    ML32, G32 = ML.astype(np.float32), G.astype(np.float32)
    L32 = gpad_mpc.lipschitz_host(ML32, G32)
    assert bits(L32) == bits(gpad_mpc.lipschitz_host(ML32.astype(np.float64), G32.astype(np.float64)))
    lam32 = lam_general(ML32, G32)
    assert lam32 <= L32 <= 1.01 * lam32
    assert bits(L32) != bits(gpad_mpc.lipschitz_host(ML, G))  # (the rounding is visible)


def test_batch_matches_single_calls():
    """shared = 0, three pairs scaled by 1, 10, 0.1 (lam scales with the product): L[b] is the pair's own call."""
    import gpad_mpc
    ML, G, lam = pair(("synth", 17, 33))
    sc = (1.0, 10.0, 0.1)
    MLs = np.stack([ML * s for s in sc])
    Gs = np.stack([G] * 3)
    L = gpad_mpc.lipschitz_host(MLs, Gs, shared=False)
    assert L.shape == (3,) and L.dtype == np.float64
    for b, s in enumerate(sc):
        assert bits(L[b]) == bits(gpad_mpc.lipschitz_host(MLs[b], Gs[b])), b
        assert s * lam * (1 - 1e-12) <= L[b] <= 1.01 * s * lam


def test_zero_matrix():
    import gpad_mpc
    ML, G, _ = pair(("synth", 5, 3))
    assert gpad_mpc.lipschitz_host(np.zeros_like(ML), G) == 0.0
    # a nilpotent product: S != 0, S^2 == 0
    MLn, Gn = np.zeros((2, 3)), np.zeros((3, 2))
    MLn[0, 0], Gn[0, 1] = 1.0, 1.0
    assert np.any(MLn @ Gn) and not np.any((MLn @ Gn) @ (MLn @ Gn))
    assert gpad_mpc.lipschitz_host(MLn, Gn) == 0.0


def test_errors():
    import gpad_mpc
    from gpad_mpc import _lib
    ML, G, _ = pair(("synth", 5, 3))
    bad = ML.copy()
    bad[1, 2] = np.nan
    with pytest.raises(gpad_mpc.GpadError) as e:
        gpad_mpc.lipschitz_host(np.stack([ML, bad]), np.stack([G, G]), shared=False)
    assert e.value.code == _lib.ERR_INVALID and "instance 1" in str(e.value)
    for rtol in (-1.0, 2.0, float("nan")):
        with pytest.raises(gpad_mpc.GpadError) as e:
            gpad_mpc.lipschitz_host(ML, G, rtol=rtol)
        assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(ValueError):
        gpad_mpc.lipschitz_host(ML, G.T.copy())


# ------------------------------------------------------------------------------ end to end on the fp64 reference
@functools.lru_cache(maxsize=None)
def loop_inputs():
    """The pinned loop: (qp, plant, X0)."""
    from gpad_mpc import problems
    qp, pl = problems.battery_plant(*LOOP.plant)
    X0 = np.random.default_rng(LOOP.seed).uniform(-LOOP.span, LOOP.span, (LOOP.packs, LOOP.plant[0]))
    return qp, pl, X0


@functools.lru_cache(maxsize=None)
def reference_loop(L, warm):
    """loop_ref64.fleet_loop of the pinned loop with step bound L, once per session."""
    qp, pl, X0 = loop_inputs()
    pk = R.make_pack(qp.ML, qp.G, L, pl.PM, pl.Pg, pl.M0, pl.g0, pl.A, pl.B)
    return R.fleet_loop([pk] * LOOP.packs, X0, None, LOOP.steps, LOOP.N, LOOP.eps, warm)


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_reference_loop_halves_its_iterations(warm):
    import gpad_mpc
    qp, pl, X0 = loop_inputs()
    L = gpad_mpc.lipschitz_host(qp.ML, qp.G)
    lam = lam_psd(np.asarray(qp.ML, np.float64), np.asarray(qp.G, np.float64))
    assert lam <= L <= 1.01 * lam
    tight, loose = reference_loop(L, warm), reference_loop(float(qp.L), warm)
    ratio = tight.it.sum() / loose.it.sum()
    print("warm" if warm else "cold", "L %.6g against %.6g: %d / %d iterations = %.3f" % (
        L, qp.L, tight.it.sum(), loose.it.sum(), ratio))
    for r in (tight, loose):
        assert set(r.cd.ravel().tolist()) <= {1, 2}
    assert ratio <= LOOP.cap, ratio
