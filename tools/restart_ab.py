"""A/B of the adaptive restart (GPAD_OPT_RESTART): restart off -- the routing every handle had before the option
(pairs, phases, finisher or resident kernel) -- against R = 1, 2, 4, 10 on the restart panels (kernel = PANEL forced
in the batch cases, AUTO in the loops: the T-wave panels' restart variant, no pairs, no finisher), one process,
alternated rounds, median of 3, all in device tensors.  With the tight L of GpadSolver.lipschitz and with
the reference's L.

  python tools/restart_ab.py [--rounds 3] [--steps 20] [--batches 256 2048 8192] [--R 1 2 4 10]

1. Cost per iteration, fixed N = 200 (no restart changes the count): C1 (40 x 180) and synthetic_qp(200, 200),
   at one panel per CU (16 instances per CU) and at 8192 instances: the restart panels per R against the AUTO
   engine with the restart off (the pairs at T > 8: what the restart panels give up per iteration) and against
   the plain stream kernel.
2. End to end, eps = 1e-4: the C4 shard (bench.make_shard(200, 200, 8192)), iterations per solve, ms, converged
   share and the fp64 max(G z* - g).
3. The C1 lockstep closed loop cold and warm per batch, and the loaded plant (battery_plant_signals) at the middle
   batch: iterations per solve, ms, converged share.
One JSON line per row; `ms_over_off` below 1: the restart is faster end to end.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gpu-dualgradient-mpc_amd")]

from lipschitz_ab import f32_up  # noqa: E402


def t32(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))).to(dev)


def median_ms(handles, enqueue, rounds):
    """Alternated rounds over the handles (each already warmed up): median kernel_ms per key."""
    ms = {k: [] for k in handles}
    for _ in range(rounds):
        for k, s in handles.items():
            enqueue(k)
            s.sync()
            ms[k].append(s.last_stats()["kernel_ms"])
    return {k: float(np.median(v)) for k, v in ms.items()}


def batch_case(name, ML, G, L, M, g, N, tol, Rs, rounds, dev, with_stream):
    """One batch solve per variant: off (AUTO), optionally stream (forced, restart off), and R in Rs."""
    import torch

    import gpad_mpc
    from gpad_mpc import _lib
    B, n = M.shape
    m = g.shape[1]
    variants = {"off": (0, _lib.KERNEL_AUTO)}
    if with_stream:
        variants["stream"] = (0, _lib.KERNEL_STREAM)
    variants.update({f"R{R}": (R, _lib.KERNEL_PANEL) for R in Rs})
    hs = {}
    for k, (R, kern) in variants.items():
        hs[k] = gpad_mpc.GpadSolver(0)
        hs[k].setup(ML, G, L, n=n, m=m, batch=B, shared=True, kernel=kern)
        hs[k].set_option("restart", R)
    z, y = torch.zeros(B, n, device=dev), torch.zeros(B, m, device=dev)
    st, viol = {}, {}
    for k in hs:  # two solves: the first two of a handle build its phase plan
        for _ in range(2):
            st[k] = hs[k].run(z.zero_(), y.zero_(), M, g, N, tol)
        viol[k] = float((z.double() @ G.double().T - g.double()).max())
    med = median_ms(hs, lambda k: hs[k].run(z.zero_(), y.zero_(), M, g, N, tol, stats=False), rounds)
    restarts = {k: round(float(hs[k].last_restarts().mean()), 2) for k in hs}
    print(json.dumps({"case": name, "batch": B, "N": N, "tol": tol, "L": L,
                      "kernel": {k: st[k]["kernel"] for k in hs},
                      "mean_iters_per_solve": {k: round(st[k]["total_iterations"] / B, 1) for k in hs},
                      "share_converged": {k: round(st[k]["converged"] / B, 4) for k in hs},
                      "mean_restarts": restarts, "max_violation_fp64": viol,
                      "kernel_ms": {k: round(v, 4) for k, v in med.items()},
                      "ms_over_off": {k: round(med[k] / med["off"], 3) for k in hs},
                      **({"ms_over_stream": {k: round(med[k] / med["stream"], 3) for k in hs}} if with_stream else {})}),
          flush=True)
    for s in hs.values():
        s.close()


def loops(args, dev):
    import torch

    import gpad_mpc
    from gpad_mpc import problems
    steps, rounds = args.steps, max(3, args.rounds)
    for plant in ("plain", "signals"):
        qp, pl = (problems.battery_plant_signals if plant == "signals" else problems.battery_plant)(4, 10)
        n, m, nx, nu = qp.n, qp.m, pl.nx, pl.nu
        d = {k: t32(getattr(qp if k in ("ML", "G") else pl, k), dev) for k in ("ML", "G", "PM", "Pg", "g0", "A", "B")}
        if plant == "signals":
            d.update({k: t32(getattr(pl, k), dev) for k in ("SM", "Sg", "E")})
        with gpad_mpc.GpadSolver(0) as s:
            Ls = {"ref": float(np.float32(qp.L)), "tight": f32_up(s.lipschitz(d["ML"], d["G"]))}
        for B in (args.batches if plant == "plain" else args.batches[len(args.batches) // 2:][:1]):
            X0 = torch.from_numpy((np.random.default_rng(B).random((B, nx)) - 0.5).astype(np.float32)).to(dev)
            sig = None
            if plant == "signals":
                rng = np.random.default_rng([B, 1])
                sig = torch.from_numpy(np.concatenate([rng.uniform(-5, 5, (steps, B, 1)),
                                                       rng.uniform(-0.1, 0.1, (steps, B, nx))],
                                                      axis=-1).astype(np.float32)).to(dev)
            for lname, L in Ls.items():
                hs = {}
                for k, R in [("off", 0)] + [(f"R{R}", R) for R in args.R]:
                    s = hs[k] = gpad_mpc.GpadSolver(0)
                    s.setup(d["ML"], d["G"], L, n=n, m=m, batch=B, shared=True)
                    s.setup_plant(d["PM"], d["Pg"], g0=d["g0"], A=d["A"], B=d["B"])
                    if plant == "signals":
                        s.setup_signals(d["SM"], d["Sg"], d["E"])
                    s.set_option("restart", R)
                x, z, y = torch.empty(B, nx, device=dev), torch.empty(B, n, device=dev), torch.empty(B, m, device=dev)

                def enqueue(k, warm, **kw):
                    x.copy_(X0)
                    z.zero_()
                    y.zero_()
                    torch.cuda.synchronize()
                    return hs[k].closed_loop(x, z, y, steps, 3000, 1e-4, warm=warm, signals=sig, **kw)

                for warm in (False, True):
                    its, cds, kern = {}, {}, {}
                    for k in hs:
                        its[k], cds[k] = np.zeros(steps * B, np.int32), np.zeros(steps * B, np.int32)
                        kern[k] = enqueue(k, warm, iters=its[k], codes=cds[k])["kernel"]
                    med = median_ms(hs, lambda k: enqueue(k, warm, stats=False), rounds)
                    print(json.dumps({"case": f"C1 lockstep loop, {plant}", "batch": B, "steps": steps,
                                      "mode": "eps_warm" if warm else "eps_cold", "L": lname, "kernel": kern,
                                      "mean_iters_per_solve": {k: round(float(its[k].mean()), 1) for k in hs},
                                      "share_converged": {k: round(float(((cds[k] > 0) & (cds[k] < 5)).mean()), 4) for k in hs},
                                      "kernel_ms": {k: round(v, 4) for k, v in med.items()},
                                      "ms_over_off": {k: round(med[k] / med["off"], 3) for k in hs}}), flush=True)
                for s in hs.values():
                    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="*", default=[256, 2048, 8192])
    ap.add_argument("--R", type=int, nargs="*", default=[1, 2, 4, 10])
    ap.add_argument("--skip", nargs="*", default=[], choices=["cost", "c4", "loops"])
    args = ap.parse_args()
    import torch

    import bench
    import gpad_mpc
    from gpad_mpc import problems
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(json.dumps({"device": torch.cuda.get_device_name(0), "cus": cus}), flush=True)
    rounds = max(3, args.rounds)
    c1 = problems.battery_scenarios(4, 10, 8192, seed=0)
    ML4, G4, L4, M4, g4 = bench.make_shard(200, 200, 8192, 0)
    data = {"C1 40 x 180": (t32(c1.ML, dev), t32(c1.G, dev), float(np.float32(c1.L)), t32(c1.M, dev), t32(c1.g, dev)),
            "synthetic_qp 200 x 200": (t32(ML4, dev), t32(G4, dev), float(np.float32(L4)), t32(M4, dev), t32(g4, dev))}
    if "cost" not in args.skip:
        for name, (ML, G, L, M, g) in data.items():
            for B in (16 * cus, 8192):
                batch_case(f"cost per iteration, {name}", ML, G, L, M[:B].contiguous(), g[:B].contiguous(), 200, 0.0,
                           args.R, rounds, dev, True)
    if "c4" not in args.skip:
        ML, G, L, M, g = data["synthetic_qp 200 x 200"]
        with gpad_mpc.GpadSolver(0) as s:
            tight = f32_up(s.lipschitz(ML, G))
        for lname, Lv in (("ref", L), ("tight", tight)):
            batch_case(f"C4 shard end to end, L {lname}", ML, G, Lv, M, g, 5000, 1e-4, args.R, rounds, dev, False)
    if "loops" not in args.skip:
        loops(args, dev)


if __name__ == "__main__":
    main()
