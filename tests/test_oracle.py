"""CPU tests pinning the oracle (oracle/gpad_oracle.c) before anything is compared against it.

Pins, in order of strength:
  1. bit-exact against the reference's OWN seq_functions.cpp (oracle/_ref, compiled from
     /root/reference) -- via the committed golden vectors, and live when _ref is built;
  2. the reference's step-3 known-answer files (build/step3/{1..5}) at their printed precision;
  3. fp64 path against the numpy restatement of acceldualgrad.m (tests/matlab_ref.py).
"""
from __future__ import annotations

import os

import numpy as np
import pytest

from conftest import GOLDEN, GOLDEN_SETS, f32_inputs, load_golden


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("name", GOLDEN_SETS)
@pytest.mark.parametrize("K", [1, 10, 100])
def test_oracle_bitexact_vs_reference_steps(oracle, name, K):
    gd = load_golden(name)
    ML, M, G, g, L = f32_inputs(gd)
    n, m = ML.shape
    z, y, it, conv = oracle.solve_f32(np.zeros(n), np.zeros(m), ML, M, G, g, K, L)
    assert it == K and not conv
    assert np.array_equal(z, gd[f"ref_z_{K}"])
    assert np.array_equal(y, gd[f"ref_y_{K}"])


@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_oracle_warm_start(oracle, name):
    gd = load_golden(name)
    ML, M, G, g, L = f32_inputs(gd)
    z, y, _, _ = oracle.solve_f32(gd["warm_z0"], gd["warm_y0"], ML, M, G, g, 50, L)
    assert np.array_equal(z, gd["ref_warm_z_50"])
    assert np.array_equal(y, gd["ref_warm_y_50"])


@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_oracle_step_kats(oracle, name):
    gd = load_golden(name)
    ML, M, G, g, L = f32_inputs(gd)
    MGneg, GL, pD = oracle.scale(ML, G, g, L)
    w = oracle.step1(gd["kat_y"], gd["kat_ym1"], gd["kat_beta"])
    assert np.array_equal(w, gd["kat_w"])
    zh = oracle.step2(MGneg, w, M)
    assert np.array_equal(zh, gd["kat_zhat"])
    z = oracle.step3(gd["kat_theta"], gd["kat_zm1"], zh)
    assert np.array_equal(z, gd["kat_z"])
    yp = oracle.step4(GL, w, pD, zh)
    assert np.array_equal(yp, gd["kat_yp1"])
    assert (yp >= 0).all()


def read_step3(k):
    d = os.path.join(GOLDEN, "step3", str(k))
    with open(os.path.join(d, "input.txt")) as f:
        tok = f.read().split()
    n_u, N, m, theta = int(tok[0]), int(tok[1]), int(tok[2]), np.float32(tok[3])
    n = n_u * N
    vals = np.array(tok[4:], np.float32)
    zm1, zhat = vals[:n], vals[n:2 * n]
    with open(os.path.join(d, "output.txt")) as f:
        out = np.array(f.read().split(), np.float32)
    return n_u, N, m, theta, zm1, zhat, out


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_oracle_step3_reference_fixtures(oracle, k):
    """step3.cu's known-answer check; the files carry 8 decimals, so compare at 1e-6 relative
    (step3.cu's own 1e-7 absolute bound fails on set 4 from the print rounding alone)."""
    n_u, N, m, theta, zm1, zhat, out = read_step3(k)
    z = oracle.step3(theta, zm1, zhat)
    assert z.shape == out.shape
    assert np.max(np.abs(z - out)) <= 1e-6 * max(1.0, float(np.max(np.abs(out))))


def test_schedule_matches_step3_theta(oracle):
    """The step-3 fixtures were taken at theta = 0.03593498 -- theta_52 of the recursion."""
    th, be = oracle.schedule(100)
    assert abs(th[52] - 0.03593498) < 5e-9
    assert th[0] == 1.0 and be[0] == 0.0 and be[1] == 0.0 and be[2] == 0.0
    thp, bep = oracle.schedule(100, 1)
    np.testing.assert_array_equal(th, thp)
    np.testing.assert_array_equal(be[1:], bep[:-1])  # MATLAB lags beta by one iteration


@pytest.mark.parametrize("name", ["battery_c1", "battery_10x4", "synth_small"])
def test_oracle_f64_vs_matlab_restatement(oracle, name):
    gd = load_golden(name)
    z, y, _, _ = oracle.solve_f64(np.zeros(gd["ML"].shape[0]), np.zeros(gd["ML"].shape[1]),
                                  gd["ML"], gd["M"], gd["G"], gd["g"], 100, float(gd["L"]))
    assert rel(z, gd["matlab_z_100"]) < 1e-12
    assert rel(y, gd["matlab_y_100"]) < 1e-12
    z, y, _, _ = oracle.solve_f64(np.zeros(gd["ML"].shape[0]), np.zeros(gd["ML"].shape[1]),
                                  gd["ML"], gd["M"], gd["G"], gd["g"], 100, float(gd["L"]),
                                  schedule=1)
    assert rel(z, gd["matlab_paper_z_100"]) < 1e-12


@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_fp32_path_within_1e5_of_matlab(name):
    """fp32 reference arithmetic vs the fp64 MATLAB path: ~1e-6 relative after 100 iterations
    (this is a property of fp32, not of any implementation; documented in DESIGN.md)."""
    gd = load_golden(name)
    assert rel(gd["ref_z_100"], gd["matlab_z_100"]) < 1e-5
    assert rel(gd["ref_y_100"], gd["matlab_y_100"]) < 1e-5


@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_oracle_algorithm1_golden(oracle, name):
    gd = load_golden(name)
    ML, M, G, g, L = f32_inputs(gd)
    n, m = ML.shape
    z, y, it, conv = oracle.solve_f32(np.zeros(n), np.zeros(m), ML, M, G, g, 5000, L, 1e-4, 10)
    assert conv and it == int(gd["tol_iters"]) and it % 10 == 0
    assert np.array_equal(z, gd["tol_z"]) and np.array_equal(y, gd["tol_y"])
    # the returned z meets the tolerance it claims, evaluated exactly (fp64) on the caller's
    # f32 data: max(G z* - g) <= 1e-4 (z* = z for test A, zhat for test B)
    viol = float(np.max(G.astype(np.float64) @ z.astype(np.float64) - g.astype(np.float64)))
    assert viol <= 1e-4


def _c4_violations(oracle, n, m, B, tol, N, seed=0):
    """Every instance of a C4-generator batch (bench.make_shard) solved by the oracle to tol;
    returns the exact max(G z* - g) of each converged instance and the iteration counts."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    ML, G, L, M, g = bench.make_shard(n, m, B, 0, seed=seed)
    f = np.float32
    ML32, G32, L32 = ML.astype(f), G.astype(f), f(L)
    MGneg, GL, _ = oracle.scale(ML32, G32, g[0].astype(f), L32)
    g32 = g.astype(f)
    Z, Y, it, _ = oracle.solve_batch_f32(np.zeros((B, n)), np.zeros((B, m)), MGneg, M.astype(f), GL,
                                         oracle.scale_vec(g32, L32), N, L32, tol, threads=8)
    viol = (Z.astype(np.float64) @ G32.astype(np.float64).T - g32.astype(np.float64)).max(axis=1)
    return viol, it


@pytest.mark.parametrize("n,m,B,tol,N", [(200, 200, 512, 1e-4, 5000), (40, 40, 256, 1e-5, 20000),
                                         (40, 180, 256, 1e-5, 20000)])
def test_termination_certified_on_the_constraint(oracle, n, m, B, tol, N):
    """No instance is reported converged above eps: test (A) is nominated by the recursive
    u = G_L z but decided on the direct chain G_L z, both tests keep a rounding margin
    (oracle/gpad_oracle.c orc_check_f32).  Checked exactly (fp64) on the returned z* of every
    converged instance -- C4's generator at eps = 1e-4, and long solves (1e-5) where the
    recursion alone drifts hundreds of f32 units from G_L z."""
    viol, it = _c4_violations(oracle, n, m, B, tol, N)
    conv = it < N
    assert conv.sum() >= 0.9 * B
    assert viol[conv].max() <= tol, (viol[conv].max(), int(np.argmax(np.where(conv, viol, -np.inf))))


def test_oracle_n0_iterations_identity(oracle):
    gd = load_golden("synth_small")
    ML, M, G, g, L = f32_inputs(gd)
    z0 = np.linspace(-1, 1, ML.shape[0]).astype(np.float32)
    y0 = np.linspace(0, 1, ML.shape[1]).astype(np.float32)
    z, y, it, conv = oracle.solve_f32(z0, y0, ML, M, G, g, 0, L)
    assert it == 0 and np.array_equal(z, z0) and np.array_equal(y, y0)


def test_oracle_batch_equals_single(oracle):
    from gpad_mpc import problems
    qp = problems.synthetic_qp(24, 40, batch=6, seed=3)
    ML, G = qp.ML.astype(np.float32), qp.G.astype(np.float32)
    L = np.float32(qp.L)
    MGneg, GL, _ = oracle.scale(ML, G, qp.g[0].astype(np.float32), L)
    PD = oracle.scale_vec(qp.g, L)
    GP = qp.M.astype(np.float32)
    Z0 = np.zeros((6, 24), np.float32)
    Y0 = np.zeros((6, 40), np.float32)
    Z, Y, iters, total = oracle.solve_batch_f32(Z0, Y0, MGneg, GP, GL, PD, 3000, L, 1e-4, threads=4)
    for b in range(6):
        z, y, it, _ = oracle.solve_f32(Z0[b], Y0[b], ML, GP[b], G, qp.g[b].astype(np.float32), 3000,
                                       L, 1e-4)
        assert np.array_equal(Z[b], z) and np.array_equal(Y[b], y) and iters[b] == it
    assert total == int(iters.sum())


def test_reference_build_matches_oracle_c2_live(oracle):
    """Pin at the C2 shape (200 x 200): against the reference build's recorded end states
    (tests/golden/ref_c2.npz, make_golden.py make_c2), and live when the reference was compiled
    here."""
    import pyoracle
    from gpad_mpc import problems
    qp = problems.synthetic_qp(200, 200, seed=0)
    ML, M, G, g = (qp.ML.astype(np.float32), qp.M.astype(np.float32), qp.G.astype(np.float32),
                   qp.g.astype(np.float32))
    L = np.float32(qp.L)
    MGneg, GL, pD = oracle.scale(ML, G, g, L)
    zo, yo, _, _ = oracle.solve_scaled_f32(np.zeros(200), np.zeros(200), MGneg, M, GL, pD, 100, L)
    rec = load_golden("ref_c2")
    assert np.array_equal(rec["z_100"], zo) and np.array_equal(rec["y_100"], yo)
    if pyoracle.RefSeq.available():
        th, be = oracle.schedule_f32(100)
        R = pyoracle.RefSeq()
        zr, yr = R.solve_c(np.zeros(200), np.zeros(200), MGneg, M, GL, pD, th, be, 100)
        assert np.array_equal(zr, zo) and np.array_equal(yr, yo)
