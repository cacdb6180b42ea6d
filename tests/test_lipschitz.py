"""gpad_lipschitz on the device (csrc/gpad_lipschitz.hip) against its host twin, and the loops it is for.

Device against host: both run the same recursion; they differ in the fp64 summation order of the products (the
MFMA's fma chain against mul + add) and of the norms (tile slots against one ascending sum), over at most 257
terms and 10 squarings: of order 1e-13 relative.  The bar is 1e-10, three decades above that.  Bit-level claims
are device against device: a pair alone, in a batch, in another chunk, from host or device memory, twice.
Measured on an MI355X (the case prints it): |L_dev / L_host - 1| is 0 on five of the seven shapes and at most 4.4e-16.

Chunk sizes (csrc/gpad_setup.cpp): a chunk holds at most kLipMaxChunk = 1024 instances and kLipWorkCap = 1 GiB
of workspace.  The instance cap is reached at any K, so the chunking case runs 1027 pairs of K = 3 (5 x 3) --
two chunks, 1024 + 3; the byte cap would need over a thousand pairs of K > 256 and is the same loop.

End to end: the loop pinned in tests/test_lipschitz_cpu.py (C1 battery plant, 4 packs, 6 steps, N = 3000,
eps = 1e-4).  test_f32_oracle_stays_within_the_cap is the CPU check that the f32 reference alone meets the
0.5 cap on these inputs (2100 / 6660 cold, 640 / 1630 warm on the f32 oracle), so the f32 GPU cases may rely
on it.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import pytest

import test_lipschitz_cpu as TC
import test_loop_async as TA
import test_loop_f64 as T64
from test_lipschitz_cpu import LOOP, bits, pair

DEVICE_CASES = [("battery", 1, 1), ("synth", 16, 16), ("synth", 17, 33), ("synth", 33, 17), ("battery", 4, 10),
                ("synth", 64, 257), ("synth", 200, 200)]
COLD_WARM = pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------ the estimator
@pytest.mark.gpu
@pytest.mark.parametrize("case", DEVICE_CASES, ids=TC.IDS)
def test_device_matches_host_twin(gpu, case):
    """(1, 1): k = 0, no squaring launch; 16: one exact MFMA tile; 17, 33: ragged tiles, both products (n < m:
    ML G, m < n: G ML); C1 (40 x 180); 64 x 257: one full workgroup tile and an inner dimension that is no
    multiple of the LDS stage; 200: 4 x 4 workgroup tiles with a ragged edge."""
    import gpad_mpc
    ML, G, lam = pair(case)
    Lh = gpad_mpc.lipschitz_host(ML, G)
    with gpad_mpc.GpadSolver(0) as s:
        Ld = s.lipschitz(ML, G)
        Lt = s.lipschitz(cuda(ML), cuda(G))
    print(case, "L_dev %.15g  L_dev / L_host - 1 = %.3e  L_dev / lam - 1 = %.3e" % (Ld, Ld / Lh - 1, Ld / lam - 1))
    assert isinstance(Ld, float) and isinstance(Lt, float)
    assert bits(Ld) == bits(Lt)
    assert abs(Ld / Lh - 1) <= 1e-10
    assert Ld >= lam and Ld <= 1.01 * lam


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_batch_is_the_single_calls(gpu, dtype):
    """shared = 0, the (17, 33) pair scaled by 1, 10, 0.1: L[b] is the bits of the pair's own call, for host
    and device operands, twice over; f32 operands give the bound of the rounded matrices."""
    import torch

    import gpad_mpc
    ML, G, lam = pair(("synth", 17, 33))
    sc = (1.0, 10.0, 0.1)
    MLs = np.stack([ML * s for s in sc]).astype(dtype)
    Gs = np.stack([G] * 3).astype(dtype)
    with gpad_mpc.GpadSolver(0) as s:
        L = s.lipschitz(MLs, Gs, shared=False)
        Lt = s.lipschitz(cuda(MLs), cuda(Gs), shared=False)
        again = s.lipschitz(MLs, Gs, shared=False)
        single = [s.lipschitz(MLs[b], Gs[b]) for b in range(3)]
        wide = [s.lipschitz(MLs[b].astype(np.float64), Gs[b].astype(np.float64)) for b in range(3)]
    assert isinstance(L, np.ndarray) and L.shape == (3,) and L.dtype == np.float64
    assert isinstance(Lt, torch.Tensor) and Lt.is_cuda and Lt.dtype == torch.float64 and tuple(Lt.shape) == (3,)
    assert bits(L) == bits(Lt.cpu().numpy()) == bits(again) == bits(single) == bits(wide)
    Lh = gpad_mpc.lipschitz_host(MLs, Gs, shared=False)
    for b, sb in enumerate(sc):
        assert abs(L[b] / Lh[b] - 1) <= 1e-10
        lam_b = TC.lam_general(MLs[b], Gs[b])
        assert abs(lam_b / (sb * lam) - 1) < 1e-5
        assert lam_b <= L[b] <= 1.01 * lam_b


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_chunks(gpu, device):
    """1027 pairs of K = 3 against the instance cap of 1024 (module docstring): two chunks, the second staged
    and read from its own offset.  Seven distinct scalings cycle through the batch, so every L[b] is checked
    against its pair's own call."""
    import gpad_mpc
    ML, G, lam = pair(("synth", 5, 3))
    B, sc = 1027, 1.0 + 0.25 * np.arange(7)
    MLs = np.stack([ML * sc[b % 7] for b in range(B)])
    Gs = np.ascontiguousarray(np.broadcast_to(G, (B,) + G.shape))
    with gpad_mpc.GpadSolver(0) as s:
        L = s.lipschitz(cuda(MLs), cuda(Gs), shared=False).cpu().numpy() if device else s.lipschitz(MLs, Gs, shared=False)
        single = np.array([s.lipschitz(ML * sc[i], G) for i in range(7)])
    assert bits(L) == bits(single[np.arange(B) % 7])
    assert (single >= sc * lam * (1 - 1e-12)).all() and (single <= 1.01 * sc * lam).all()


@pytest.mark.gpu
def test_edge_cases_and_errors(gpu):
    import gpad_mpc
    from gpad_mpc import _lib
    ML, G, _ = pair(("synth", 5, 3))
    MLn, Gn = np.zeros((2, 3)), np.zeros((3, 2))  # S != 0, S^2 == 0
    MLn[0, 0], Gn[0, 1] = 1.0, 1.0
    bad = ML.copy()
    bad[1, 2] = np.nan
    with gpad_mpc.GpadSolver(0) as s:
        assert s.lipschitz(np.zeros_like(ML), G) == 0.0
        assert s.lipschitz(MLn, Gn) == 0.0
        with pytest.raises(gpad_mpc.GpadError) as e:
            s.lipschitz(np.stack([ML, bad]), np.stack([G, G]), shared=False)
        assert e.value.code == _lib.ERR_INVALID and "instance 1" in str(e.value)
        for rtol in (-1.0, 2.0, float("nan")):
            with pytest.raises(gpad_mpc.GpadError) as e:
                s.lipschitz(ML, G, rtol=rtol)
            assert e.value.code == _lib.ERR_INVALID
        # the handle still serves after the errors; rtol = 0 is the default 0.01, a larger rtol squares less
        L = s.lipschitz(ML, G)
        assert bits(L) == bits(s.lipschitz(ML, G, rtol=0.0))
        assert L <= s.lipschitz(ML, G, rtol=0.5)


# ------------------------------------------------------------------------------ end to end, f64
def f64_config(L):
    qp, pl, X0 = TC.loop_inputs()
    return T64._cfg("lipschitz", "plant", qp.ML, qp.G, L, T64._maps(pl), X0, LOOP.steps)


def device_L(ML, G):
    import gpad_mpc
    with gpad_mpc.GpadSolver(0) as s:
        return s.lipschitz(ML, G)


@pytest.mark.gpu
@COLD_WARM
def test_loop_f64(gpu, warm):
    """The pinned loop on an f64 handle with L = solver.lipschitz(ML, G): counts and codes equal loop_ref64 run
    with that same L, trajectories within 1e-9 (tests/test_loop_f64.py's bars, all of them), the final z
    feasible to eps in fp64, and at most half the iterations of the same handle set up with qp.L."""
    assert (T64.NTOL, T64.K) == (LOOP.N, 10)
    qp, pl, X0 = TC.loop_inputs()
    L = device_L(np.asarray(qp.ML, np.float64), np.asarray(qp.G, np.float64))
    c = f64_config(L)
    ref = TC.reference_loop(L, warm)
    r = T64.gpu_loop(c, warm, LOOP.eps)
    T64.assert_matches_reference(c, r, ref, warm, LOOP.eps, "stream")
    assert set(r.cd.ravel().tolist()) <= {1, 2}
    g = r.xs[-1] @ c.maps["Pg"].T + c.maps["g0"]
    viol = (r.z @ c.G.T - g).max(axis=1)
    loose = T64.gpu_loop(f64_config(float(qp.L)), warm, LOOP.eps)
    ratio = r.it.sum() / loose.it.sum()
    print("f64 %s: L %.6g against %.6g, %d / %d iterations = %.3f, max(G z - g) %.3e" % (
        "warm" if warm else "cold", L, qp.L, r.it.sum(), loose.it.sum(), ratio, viol.max()))
    assert viol.max() <= LOOP.eps
    assert set(loose.cd.ravel().tolist()) <= {1, 2}
    assert ratio <= LOOP.cap


# ------------------------------------------------------------------------------ end to end, f32
def f32_round_up(L):
    """The smallest f32 >= L: an f32 caller must not round the bound down."""
    Lf = np.float32(L)
    return float(Lf if Lf >= L else np.nextafter(Lf, np.float32(np.inf)))


def f32_inputs():
    qp, pl, X0 = TC.loop_inputs()
    return TA.battery(*LOOP.plant), TA.F32(qp.ML), TA.F32(qp.G), X0.astype(np.float32)


@functools.lru_cache(maxsize=None)
def f32_oracle_loop(L, warm):
    import pyoracle
    o = pyoracle.Oracle()
    p, ML, G, X0 = f32_inputs()
    MGneg, GL, _ = o.scale(ML, G, np.zeros(ML.shape[1], np.float32), np.float32(L))
    rows = [o.closed_loop_f32(X0[b], MGneg, GL, np.float32(L), p.PM, p.Pg, p.A, p.B, LOOP.steps, LOOP.N, LOOP.eps,
                              M0=p.M0, g0=p.g0, warm=warm) for b in range(LOOP.packs)]
    return SimpleNamespace(it=np.stack([r[5] for r in rows], axis=1), xs=np.stack([r[3] for r in rows], axis=1),
                           z=np.stack([r[1] for r in rows]))


@COLD_WARM
def test_f32_oracle_stays_within_the_cap(warm):
    """CPU: the oracle's f32 closed loop with the host twin's L (rounded up to f32) against qp.L."""
    import gpad_mpc
    p, ML, G, X0 = f32_inputs()
    L = f32_round_up(gpad_mpc.lipschitz_host(ML, G))
    tight, loose = f32_oracle_loop(L, warm), f32_oracle_loop(float(np.float32(p.qp.L)), warm)
    print("f32 oracle %s: %d / %d" % ("warm" if warm else "cold", tight.it.sum(), loose.it.sum()))
    assert tight.it.max() < LOOP.N and loose.it.max() < LOOP.N
    assert tight.it.sum() / loose.it.sum() <= LOOP.cap


def f32_run(L, warm, **options):
    import gpad_mpc
    p, ML, G, X0 = f32_inputs()
    s = gpad_mpc.GpadSolver(0)
    s.setup(ML, G, L, n=p.qp.n, m=p.qp.m, batch=LOOP.packs, shared=True)
    s.setup_plant(TA.F32(p.PM), TA.F32(p.Pg), g0=TA.F32(p.g0), A=TA.F32(p.A), B=TA.F32(p.B))
    s.set_options(**options)
    r = TA.loop(s, p, X0, LOOP.steps, LOOP.N, LOOP.eps, warm)
    s.close()
    return r


@pytest.mark.gpu
@COLD_WARM
def test_loop_f32_engines(gpu, oracle, warm):
    """The pinned loop on an f32 handle, L = lipschitz of the f32 matrices it binds: the lockstep loop, loop_async
    and loop_panel agree bit for bit (and with the f32 oracle), every solve converges, the final z of every pack is
    feasible to eps in fp64 on the f32 G and the step's f32 g, and the lockstep run takes at most half the
    iterations of the same handle set up with qp.L."""
    p, ML, G, X0 = f32_inputs()
    L = f32_round_up(device_L(ML, G))
    lock = f32_run(L, warm)
    runs = {"loop": f32_run(L, warm, loop_async=1), "loop_panel": f32_run(L, warm, loop_panel=1)}
    assert lock.st["kernel"] not in runs
    for name, r in runs.items():
        assert r.st["kernel"] == name
        TA.assert_same_run(r, lock)
    orc = f32_oracle_loop(L, warm)
    TA.same_bits(lock.it, orc.it, "oracle counts")
    TA.same_bits(lock.xs, orc.xs, "oracle xs")
    TA.same_bits(lock.z, orc.z, "oracle z")
    assert (lock.cd > 0).all() and lock.it.max() < LOOP.N
    g = np.stack([oracle.affine(p.Pg, p.g0, lock.xs[-1, b]) for b in range(LOOP.packs)]).astype(np.float64)
    viol = (lock.z.astype(np.float64) @ G.astype(np.float64).T - g).max(axis=1)
    loose = f32_run(float(np.float32(p.qp.L)), warm)
    ratio = lock.it.sum() / loose.it.sum()
    print("f32 %s: L %.9g against %.9g, %d / %d iterations = %.3f, max(G z - g) %.3e" % (
        "warm" if warm else "cold", L, p.qp.L, lock.it.sum(), loose.it.sum(), ratio, viol.max()))
    assert viol.max() <= LOOP.eps
    assert (loose.cd > 0).all()
    assert ratio <= LOOP.cap
