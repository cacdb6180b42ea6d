"""A/B of the step bound: the reference's L (||H||_F^2 for the battery plants, ||G H^-1 G'||_F for synthetic_qp)
against GpadSolver.lipschitz (gpad_lipschitz: an upper bound of lambda_max(G ML) within 1 %), one process,
alternated rounds, all in device tensors.

  python tools/lipschitz_ab.py [--rounds 3] [--steps 20] [--batches 256 2048 8192] [--skip-c5]

1. The README's closed loops: C1 plant (battery_plant(4, 10): n = 40, m = 180) and the same under load
   (battery_plant_signals, loads U(-5, 5) A and references U(-0.1, 0.1) as tools/loop_ab.py --signals draws them),
   on the lockstep loop, loop_async and loop_panel, eps cold / eps warm (tol 1e-4, N 3000) and fixed N = 100.
   Per L the three engines are compared bit for bit first (that run is each handle's warm-up); then `rounds` rounds
   alternate all six handles.  One JSON line per (batch, plant, mode): mean iterations per solve and the share of
   solves that converged per L, the median kernel_ms per engine and L, and `ms_tight_over_ref` per engine (below 1:
   the estimate is faster).  Fixed-N rows gain nothing by construction.
2. One batch solve of the C4 shape (bench.make_shard(200, 200, 8192): shared synthetic_qp matrices, eps = 1e-4)
   with its Frobenius L against the estimate.
3. The time of gpad_lipschitz itself (host wall time around the synchronous call, device operands, best and median
   of the rounds after a warm-up): C1, one 200 x 200 pair, and 1024 distinct 800 x 800 pairs (C5; f32 operands,
   5.2 GB of them; --skip-c5 leaves it out).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gpu-dualgradient-mpc_amd")]

MODES = {"eps_cold": dict(N=3000, tol=1e-4, warm=False), "eps_warm": dict(N=3000, tol=1e-4, warm=True),
         "fixed_100": dict(N=100, tol=0.0, warm=False)}
ENGINES = {"lockstep": {}, "async": dict(loop_async=1), "panel": dict(loop_panel=1)}
WANT = {"async": "loop", "panel": "loop_panel"}


def f32_up(L):
    """The smallest f32 >= L (an f32 handle must not round the bound down)."""
    Lf = np.float32(L)
    return float(Lf if Lf >= L else np.nextafter(Lf, np.float32(np.inf)))


def loops(args, dev):
    import torch

    import gpad_mpc
    from gpad_mpc import problems
    steps, rounds = args.steps, max(3, args.rounds)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))).to(dev)  # noqa: E731
    for plant in ("plain", "signals"):
        qp, pl = (problems.battery_plant_signals if plant == "signals" else problems.battery_plant)(4, 10)
        n, m, nx, nu = qp.n, qp.m, pl.nx, pl.nu
        d = {k: t32(getattr(qp if k in ("ML", "G") else pl, k)) for k in ("ML", "G", "PM", "Pg", "g0", "A", "B")}
        if plant == "signals":
            d.update({k: t32(getattr(pl, k)) for k in ("SM", "Sg", "E")})
        with gpad_mpc.GpadSolver(0) as s:
            Ls = {"ref": float(np.float32(qp.L)), "tight": f32_up(s.lipschitz(d["ML"], d["G"]))}
        print(json.dumps({"plant": "battery_plant%s(4, 10)" % ("_signals" if plant == "signals" else ""), "n": n,
                          "m": m, "steps": steps, "rounds": rounds, "L": Ls}), flush=True)
        for B in args.batches:
            X0 = torch.from_numpy((np.random.default_rng(B).random((B, nx)) - 0.5).astype(np.float32)).to(dev)
            sig = None
            if plant == "signals":
                rng = np.random.default_rng([B, 1])
                sig = torch.from_numpy(np.concatenate([rng.uniform(-5, 5, (steps, B, 1)),
                                                       rng.uniform(-0.1, 0.1, (steps, B, nx))],
                                                      axis=-1).astype(np.float32)).to(dev)
            var = {}
            for lname, L in Ls.items():
                for ename, opts in ENGINES.items():
                    s = gpad_mpc.GpadSolver(0)
                    s.setup(d["ML"], d["G"], L, n=n, m=m, batch=B, shared=True)
                    s.setup_plant(d["PM"], d["Pg"], g0=d["g0"], A=d["A"], B=d["B"])
                    if plant == "signals":
                        s.setup_signals(d["SM"], d["Sg"], d["E"])
                    s.set_options(**opts)
                    buf = dict(x=torch.empty(B, nx, device=dev), z=torch.empty(B, n, device=dev),
                               y=torch.empty(B, m, device=dev), xs=torch.empty(steps, B, nx, device=dev),
                               us=torch.empty(steps, B, nu, device=dev))
                    var[lname, ename] = (s, buf)

            def enqueue(key, mode, **kw):
                s, b = var[key]
                b["x"].copy_(X0)
                b["z"].zero_()
                b["y"].zero_()
                torch.cuda.synchronize()
                return s.closed_loop(b["x"], b["z"], b["y"], steps, mode["N"], mode["tol"], warm=mode["warm"],
                                     xs=b["xs"], us=b["us"], signals=sig, **kw)

            for mname, mode in MODES.items():
                its, cds, kern = {}, {}, {}
                for key in var:  # the bit-for-bit check of the engines per L, and each handle's warm-up
                    its[key], cds[key] = np.zeros(steps * B, np.int32), np.zeros(steps * B, np.int32)
                    kern[key] = enqueue(key, mode, iters=its[key], codes=cds[key])["kernel"]
                bad = [(ln, en, k) for (ln, en) in var if en != "lockstep" for k in ("x", "z", "y", "xs", "us")
                       if not torch.equal(var[ln, "lockstep"][1][k].view(torch.int32), var[ln, en][1][k].view(torch.int32))]
                bad += [(ln, en, "iters") for (ln, en) in var
                        if not np.array_equal(its[ln, en], its[ln, "lockstep"]) or not np.array_equal(cds[ln, en], cds[ln, "lockstep"])]
                bad += [(ln, en, "kernel " + str(kern[ln, en])) for (ln, en) in var
                        if (kern[ln, en] == WANT.get(en)) != (en != "lockstep")]
                if bad:
                    print(json.dumps({"batch": B, "plant": plant, "mode": mname, "error": "engines differ", "differ": bad}))
                    continue
                ms = {k: [] for k in var}
                for _ in range(rounds):
                    for key in var:
                        enqueue(key, mode, stats=False)
                        var[key][0].sync()
                        ms[key].append(var[key][0].last_stats()["kernel_ms"])
                med = {k: float(np.median(v)) for k, v in ms.items()}
                print(json.dumps({
                    "batch": B, "plant": plant, "mode": mname,
                    "mean_iters_per_solve": {ln: round(float(its[ln, "lockstep"].mean()), 1) for ln in Ls},
                    "max_iters_per_solve": {ln: int(its[ln, "lockstep"].max()) for ln in Ls},
                    "share_converged": {ln: round(float((cds[ln, "lockstep"] > 0).mean()), 4) for ln in Ls},
                    "iters_tight_over_ref": round(float(its["tight", "lockstep"].sum() / its["ref", "lockstep"].sum()), 3),
                    "kernel_ms": {en: {ln: round(med[ln, en], 4) for ln in Ls} for en in ENGINES},
                    "ms_tight_over_ref": {en: round(med["tight", en] / med["ref", en], 3) for en in ENGINES},
                    "faster": {en: ("tight" if max(ms["tight", en]) < min(ms["ref", en]) else
                                    "ref" if min(ms["tight", en]) > max(ms["ref", en]) else "none") for en in ENGINES}}),
                    flush=True)
            for s, _ in var.values():
                s.close()


def c4_solve(args, dev):
    import torch

    import bench
    import gpad_mpc
    n = m = 200
    B, tol, N = 8192, 1e-4, 5000
    ML, G, L, M, g = bench.make_shard(n, m, B, 0)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))).to(dev)  # noqa: E731
    dML, dG, dM, dg = t32(ML), t32(G), t32(M), t32(g)
    with gpad_mpc.GpadSolver(0) as s:
        Ls = {"ref": float(np.float32(L)), "tight": f32_up(s.lipschitz(dML, dG))}
    hs, z, y = {}, torch.zeros(B, n, device=dev), torch.zeros(B, m, device=dev)
    for ln, Lv in Ls.items():
        hs[ln] = gpad_mpc.GpadSolver(0)
        hs[ln].setup(dML, dG, Lv, n=n, m=m, batch=B, shared=True, check_every=10)
    ms, st = {ln: [] for ln in Ls}, {}
    viol = {}
    for r in range(2 + max(3, args.rounds)):  # the first two solves of a handle build its phase plan
        for ln in Ls:
            st[ln] = hs[ln].run(z.zero_(), y.zero_(), dM, dg, N, tol)
            if r >= 2:
                ms[ln].append(st[ln]["kernel_ms"])
            viol[ln] = float((z.double() @ dG.double().T - dg.double()).max())
    print(json.dumps({
        "case": "C4 shard: 8192 instances sharing ML/G, n = m = 200, eps = 1e-4", "L": Ls,
        "kernel": {ln: st[ln]["kernel"] for ln in Ls},
        "mean_iters_per_solve": {ln: round(st[ln]["total_iterations"] / B, 1) for ln in Ls},
        "converged": {ln: st[ln]["converged"] for ln in Ls},
        "max_violation_fp64": viol,
        "solve_ms": {ln: [round(x, 3) for x in ms[ln]] for ln in Ls},
        "ms_tight_over_ref": round(float(np.median(ms["tight"]) / np.median(ms["ref"])), 3)}), flush=True)
    for h in hs.values():
        h.close()


def estimator_time(args, dev):
    import torch

    import gpad_mpc
    from gpad_mpc import problems
    rounds = max(3, args.rounds)
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)  # noqa: E731
    c1 = problems.battery_mpc(4, 10, seed=0)
    c2 = problems.synthetic_qp(200, 200, batch=1, seed=400)
    cases = [("C1 battery 40 x 180, f64", t64(c1.ML), t64(c1.G), True),
             ("synthetic_qp 200 x 200, f64", t64(c2.ML), t64(c2.G), True)]
    if not args.skip_c5:
        gen = torch.Generator(device=dev).manual_seed(0)
        A = torch.randn(1024, 800, 800, device=dev, generator=gen) / 800 ** 0.5
        cases.append(("C5: 1024 distinct 800 x 800 pairs, f32 (ML = G')", A.transpose(1, 2).contiguous(), A, False))
    with gpad_mpc.GpadSolver(0) as s:
        for name, ML, G, shared in cases:
            s.lipschitz(ML, G, shared=shared)
            ts = []
            for _ in range(rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                L = s.lipschitz(ML, G, shared=shared)
                ts.append((time.perf_counter() - t0) * 1e3)
            K, pairs = min(ML.shape[-2:]), 1 if shared else ML.shape[0]
            k = next(j for j in range(17) if j == 16 or np.log(K) / 2 ** (j + 1) <= np.log1p(0.01))
            flops = pairs * (2.0 * ML.shape[-2] * ML.shape[-1] * K + k * 2.0 * K ** 3)
            print(json.dumps({"case": name, "pairs": pairs, "squarings": k, "launches_per_chunk": k + 1,
                              "wall_ms": [round(t, 3) for t in ts], "best_ms": round(min(ts), 3),
                              "fp64_tflops_at_best": round(flops / (min(ts) / 1e3) / 1e12, 3),
                              "L": round(L, 9) if shared else [round(float(L.min()), 6), round(float(L.max()), 6)]}),
                  flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="*", default=[256, 2048, 8192])
    ap.add_argument("--skip-c5", action="store_true")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    print(json.dumps({"device": torch.cuda.get_device_name(0),
                      "cus": torch.cuda.get_device_properties(0).multi_processor_count}), flush=True)
    estimator_time(args, dev)
    c4_solve(args, dev)
    loops(args, dev)


if __name__ == "__main__":
    main()
