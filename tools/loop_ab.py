"""A/B of the closed loop (gpad_closed_loop): the lockstep loop against the asynchronous kernel
(GPAD_OPT_LOOP_ASYNC, csrc/gpad_loop.hip) on two handles over the same seeded states, all in device
tensors.  C1 plant (battery_plant(4, 10): n = 40, m = 180), 20 MPC steps, batches 1 ... 8192, three
modes: eps cold / eps warm (tol 1e-4, N 3000) and fixed N = 100.

  python tools/loop_ab.py [--rounds 3] [--steps 20] [--batches 1 64 256 512 2048 8192] [--fleet | --signals]
                          [--panel] [--infeas]
  python tools/loop_ab.py --classes K [--signals [--skip-plain]] [--infeas] [--rounds 3] [--steps 20]
                          [--batches 256 2048 8192]

--panel: a third variant, "panel" (GPAD_OPT_LOOP_PANEL, csrc/gpad_loop_panel.hip: the one-launch loop on the
MFMA panels), alternated with lockstep and async in the same process and checked against lockstep like
them; default batches 256 2048 8192.  `panel_over_lockstep` / `panel_over_async` are its rate over the
others', `panel_faster` names panel or lockstep as `faster` does.  With --signals a "sig_panel" variant
joins the two sig_ ones.  With --fleet the case is the plant/model mismatch on shared matrices (the
controller of pack 0 -- its ML, G and PM for everyone -- against every pack's own Pg, g0, A, B): per-pack
matrices have no panels, so the fleet proper is not a --panel case, and async_1wg is left out.

--fleet: a fleet of distinct packs instead (problems.battery_fleet(4, 10, battery_fleet_caps(batch, 4,
seed = batch)): per-pack ML, G and plant maps, setup(shared=False) + a stacked setup_plant), default
batches 1 64 256 2048 8192.  The lockstep loop runs the resident kernel there, the option the fleet
kernel; a third variant, "async_1wg", caps the grid at one workgroup per CU (duo_max_grid = CUs) to
show what the second workgroup per CU buys, and `async_1wg_over_async` is its rate over the default's.

--signals: two more variants in the same process, "sig_lockstep" and "sig_async", on
problems.battery_plant_signals(4, 10) (gpad_setup_signals: s = [i_load, r_1 .. r_4], loads U(-5, 5) A and
references U(-0.1, 0.1) per step and pack, seeded by the batch), each checked against the other; the
plain variants run unchanged beside them, and `sig_over_plain` is the rate with signals over the rate
without, per loop kind (informational: the signals change the QPs, so also the iteration counts).

--classes K: a fleet of K plant classes (problems.battery_fleet(4, 10, battery_fleet_caps(K, 4, seed = K)),
class_of[b] = b % K; default batches 256 2048 8192).  Variant "fleet" is the dims.shared = 0 binding of the
expanded fleet (problems.expand_classes; setup(shared=False) + a stacked setup_plant, lockstep) -- the path
a fleet of classes had to take before the class binding; "classes" is the class binding
(setup_classes, csrc/gpad_classes.cpp) with the options off, "classes_panel" and "classes_async" the
same with loop_panel = 1 and loop_async = 1 (forwarded to every class: K one-launch loops back to back),
"classes_fused" the fused class loop (set_class_loop_fused: every class in one launch, kernel
"loop_classes"); `classes_fused_over_classes_best` is its rate over the best of the other three class
variants.  With K = 1 two more variants: "shared", the plain shared-matrix handle (lockstep) --
`classes_over_shared` is then the price of the row permutations and the child handle -- and
"shared_panel", the same handle with loop_panel = 1: `classes_fused_over_shared_panel` is what the class
bookkeeping of the fused kernel and the row permutations cost against the plain panel loop.  Every variant's outputs are compared with "fleet" bit for bit first; each line has
the rates, `<variant>_over_fleet` and `<variant>_faster` ("none" inside the spread of the rounds).

--classes K --signals: the same variants on problems.battery_fleet_signals (class k =
battery_plant_signals(4, 10, capacity_ah = caps[k]); s = [i_load, r_1 .. r_4] per step and pack, drawn as for
--signals above): "fleet" binds setup_signals with stacked maps, the class variants setup_class_signals
(gpad_setup_class_signals) with one copy per class, "shared" / "shared_panel" class 0's maps.  Every variant
is then also run without signals in the same process (a second set of handles, checked against its own
"fleet" first); `sig_over_plain` is the rate with signals over the rate without, per variant -- what the
S gather and the wider state rows cost (informational: the signals change the QPs, so also the counts; the
fleet's own ratio beside it shows that part).

--infeas (without --classes; with --signals the loads make infeasible steps): the variant "infeas" ("sig_infeas"
with --signals), the lockstep loop with the battery bound bound (setup_infeasibility(problems.battery_zbound())),
and with --panel "infeas_panel" ("sig_infeas_panel"), the panel loop with it; they are compared with each other
bit for bit (outputs, counts, codes) instead of with the unbound loop, and every line gains `share_code5`,
`share_capped`, `infeas_mean_iters_per_solve` and `<bound variant>_over_<variant>`.  One more bound variant,
"infeas_async" ("sig_infeas_async"): the same handle with loop_async = 1 and the certificate in the asynchronous
loop (gpad_infeasibility_loop_async; kernel "loop"), in the same bit-for-bit check; `infeas_async_over_infeas` is
its rate over the bound lockstep loop's.

--classes K [--signals] --infeas: two more variants with the battery bound bound
(setup_infeasibility(problems.battery_zbound()), gpad_setup_infeasibility): "classes_infeas", the class binding
with the options off (lockstep, the certificate panels), and "classes_fused_infeas", the fused class loop.  With a
tolerance their solves end an infeasible step with code 5, so their outputs are not the fleet's: they are left
out of that bit-for-bit check and compared with each other instead (outputs, counts, codes); every line gains
`share_code5` -- per variant the share of (step, pack) codes equal to 5 -- `share_capped` (code 0 at N
iterations), `infeas_mean_iters_per_solve` / `infeas_max_iters_per_solve` and `<bound variant>_over_<variant>`
for every unbound variant.  Three more bound variants set the certificate beside the resident kernel
(gpad_infeasibility_resident): "classes_infeas_res", the bound class binding with the flag on (its lockstep loop
then runs the resident kernel where a class holds at most 4 packs per CU, else the panels as "classes_infeas"),
"fleet_infeas", the dims.shared = 0 fleet with the bound (the stream kernel), and "fleet_infeas_res", that fleet
with the flag on (the resident kernel); all five bound variants are compared bit for bit, and
`infeas_res_over_infeas` is the rate with the flag over the rate without, per binding.  Two more carry the
certificate in the asynchronous loop (gpad_infeasibility_loop_async, loop_async = 1; kernel "loop"):
"fleet_infeas_async", the bound dims.shared = 0 fleet on the fleet kernel's certificate twin, and
"classes_infeas_async", the bound class binding with the option and the flag forwarded (K one-launch loops back to
back); they join the bit-for-bit check of the bound variants, and `infeas_async_over_infeas_res` is their rate
over the flag-on resident variant's, per binding.  --skip-plain (with
--signals) leaves out the second set of handles without signals and `sig_over_plain`.

Per batch and mode the two variants' x, z, y, xs, us and per-step iteration counts are compared first
(that run is also each variant's warm-up); a mismatch aborts the batch.  Then `rounds` rounds
alternate the variants.  One JSON line per case: kernel_ms (events around the whole loop) and host
wall time around a final sync, per round; MPC steps/s of both variants from the median kernel_ms;
their ratio; and `faster`, which names a variant only when its slowest round beats the other's
fastest (a difference inside the spread of the rounds is reported as "none").
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


def classes_ab(args):
    """--classes K: the shared = 0 fleet against the class binding (module docstring)."""
    import torch

    import gpad_mpc
    from gpad_mpc import problems
    K, steps, rounds = args.classes, args.steps, max(3, args.rounds)
    dev = torch.device("cuda:0")
    gen = problems.battery_fleet_signals if args.signals else problems.battery_fleet
    qp, pl = gen(4, 10, problems.battery_fleet_caps(K, 4, K))
    n, m, nx, nu = qp.n, qp.m, pl.nx, pl.nu
    L = float(np.float32(qp.L))
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))).to(dev)  # noqa: E731
    maps = dict(ML=qp.ML, G=qp.G, PM=pl.PM, Pg=pl.Pg, g0=pl.g0, A=pl.A, B=pl.B)
    if args.signals:
        maps.update(SM=pl.SM, Sg=pl.Sg, E=pl.E)
    cls = {k: t32(a) for k, a in maps.items()}
    gname = "battery_fleet_signals" if args.signals else "battery_fleet"
    print(json.dumps({"plant": f"{gname}(4, 10), {K} classes, class_of[b] = b % {K}", "n": n, "m": m,
                      "steps": steps, "rounds": rounds, "device": torch.cuda.get_device_name(0),
                      "cus": torch.cuda.get_device_properties(0).multi_processor_count}))
    names = ("fleet", "classes", "classes_panel", "classes_async", "classes_fused") + (
        ("shared", "shared_panel") if K == 1 else ()) + (
        ("classes_infeas", "classes_fused_infeas", "classes_infeas_res", "fleet_infeas", "fleet_infeas_res",
         "fleet_infeas_async", "classes_infeas_async")
        if args.infeas else ())
    want = {"classes_panel": "loop_panel", "classes_async": "loop", "classes_fused": "loop_classes",
            "shared_panel": "loop_panel", "classes_fused_infeas": "loop_classes", "fleet_infeas_async": "loop",
            "classes_infeas_async": "loop"}
    INF = ("classes_infeas", "classes_fused_infeas", "classes_infeas_res", "fleet_infeas", "fleet_infeas_res",
           "fleet_infeas_async", "classes_infeas_async")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for B in args.batches:
        class_of = np.arange(B, dtype=np.int32) % K
        X0 = torch.from_numpy((np.random.default_rng(B).random((B, nx)) - 0.5).astype(np.float32)).to(dev)
        idx = torch.from_numpy(class_of.astype(np.int64)).to(dev)
        sig = None
        if args.signals:  # (drawn as main()'s --signals draws them)
            rng = np.random.default_rng([B, 1])
            sig = torch.from_numpy(np.concatenate([rng.uniform(-5, 5, (steps, B, 1)),
                                                   rng.uniform(-0.1, 0.1, (steps, B, nx))],
                                                  axis=-1).astype(np.float32)).to(dev)

        def build(with_sig):
            var = {}
            for name in names:
                s = gpad_mpc.GpadSolver(0)
                if name.startswith("fleet"):  # expand_classes on the device: instance b holds the arrays of class b % K
                    f = {k: a[idx].contiguous() for k, a in cls.items()}
                    s.setup(f["ML"], f["G"], L, n=n, m=m, batch=B, shared=False)
                    s.setup_plant(f["PM"], f["Pg"], g0=f["g0"], A=f["A"], B=f["B"])
                    if with_sig:
                        s.setup_signals(f["SM"], f["Sg"], f["E"])
                    del f
                    if name in INF:
                        s.set_infeasibility_resident(name.endswith("_res"))
                        if name.endswith("_async"):
                            s.set_option("loop_async", 1)
                            s.set_infeasibility_loop_async(True)
                        s.setup_infeasibility(problems.battery_zbound())
                elif name in ("shared", "shared_panel"):
                    s.setup(cls["ML"][0], cls["G"][0], L, n=n, m=m, batch=B, shared=True)
                    s.setup_plant(cls["PM"][0], cls["Pg"][0], g0=cls["g0"][0], A=cls["A"][0], B=cls["B"][0])
                    if with_sig:
                        s.setup_signals(cls["SM"][0], cls["Sg"][0], cls["E"][0])
                    s.set_options(loop_panel=int(name == "shared_panel"))
                else:
                    s.setup_classes(cls["ML"], cls["G"], L, class_of, n=n, m=m)
                    s.setup_plant(cls["PM"], cls["Pg"], g0=cls["g0"], A=cls["A"], B=cls["B"])
                    if with_sig:
                        s.setup_class_signals(cls["SM"], cls["Sg"], cls["E"])
                    s.set_options(loop_panel=int(name == "classes_panel"),
                                  loop_async=int(name in ("classes_async", "classes_infeas_async")))
                    s.set_class_loop_fused(name in ("classes_fused", "classes_fused_infeas"))
                    if name in INF:
                        s.set_infeasibility_resident(name.endswith("_res"))
                        s.set_infeasibility_loop_async(name.endswith("_async"))
                        s.setup_infeasibility(problems.battery_zbound())
                buf = dict(x=torch.empty(B, nx, device=dev), z=torch.empty(B, n, device=dev),
                           y=torch.empty(B, m, device=dev), xs=torch.empty(steps, B, nx, device=dev),
                           us=torch.empty(steps, B, nu, device=dev))
                var[name] = (s, buf)
            return var

        var = build(args.signals)
        # the same variants without signals: sig_over_plain
        plain = build(False) if args.signals and not args.skip_plain else None

        def enqueue(vs, name, mode, **kw):
            s, b = vs[name]
            b["x"].copy_(X0)
            b["z"].zero_()
            b["y"].zero_()
            torch.cuda.synchronize()
            return s.closed_loop(b["x"], b["z"], b["y"], steps, mode["N"], mode["tol"], warm=mode["warm"],
                                 xs=b["xs"], us=b["us"], signals=sig if vs is var else None, **kw)

        def measure(vs, mname, mode):
            """The output check (each variant's warm-up), then `rounds` alternated rounds: (its, kern, ms,
            wall, codes), or None after reporting a mismatch."""
            its, kern, cds = {}, {}, {}
            for name in vs:
                its[name], cds[name] = np.zeros(steps * B, np.int32), np.zeros(steps * B, np.int32)
                kern[name] = enqueue(vs, name, mode, iters=its[name], codes=cds[name])["kernel"]
            same = [v for v in vs if v not in INF]  # (the certificate changes results by design)
            bad = [f"{v}.{k}" for k in ("x", "z", "y", "xs", "us") for v in same if v != "fleet"
                   if not torch.equal(vs["fleet"][1][k].view(torch.int32), vs[v][1][k].view(torch.int32))]
            bad += [f"{v}.iters" for v in same if not np.array_equal(its["fleet"], its[v])]
            if "classes_infeas" in vs:  # the bound variants agree with each other, bit for bit
                bad += [f"{v}.{k}" for v in INF[1:] for k in ("x", "z", "y", "xs", "us")
                        if not torch.equal(vs[INF[0]][1][k].view(torch.int32), vs[v][1][k].view(torch.int32))]
                bad += [f"{v}.counts" for v in INF[1:]
                        if not (np.array_equal(its[INF[0]], its[v]) and np.array_equal(cds[INF[0]], cds[v]))]
                if mode["tol"] > 0 and kern["classes_infeas"] not in ("panel", "stream"):
                    bad.append("classes_infeas.kernel")
                # (the reported kernel is the largest class's: the resident kernel up to 4 packs per CU)
                res = "resident" if max(np.bincount(class_of)) <= 4 * cus else "panel"
                if mode["tol"] > 0 and (kern["classes_infeas_res"], kern["fleet_infeas"], kern["fleet_infeas_res"]) != (
                        res, "stream", "resident"):
                    bad.append("infeas_res.kernel")
            if bad or any(kern[v] is None or (kern[v] in ("loop", "loop_panel", "loop_classes")) != (v in want) or
                          (v in want and kern[v] != want[v]) for v in vs):
                print(json.dumps({"batch": B, "mode": mname, "error": "outputs differ" if bad else "wrong kernel",
                                  "differ": bad, "kernels": kern, **({"signals": vs is var} if args.signals else {})}))
                return None
            ms = {k: [] for k in vs}
            wall = {k: [] for k in vs}
            for _ in range(rounds):
                for name in vs:
                    s = vs[name][0]
                    t0 = time.perf_counter()
                    enqueue(vs, name, mode, stats=False)
                    s.sync()
                    wall[name].append((time.perf_counter() - t0) * 1e3)
                    ms[name].append(s.last_stats()["kernel_ms"])
            return its, kern, ms, wall, cds

        for mname, mode in MODES.items():
            res = measure(var, mname, mode)
            if res is None:
                break
            its, kern, ms, wall, cds = res
            med = {k: float(np.median(v)) for k, v in ms.items()}
            rate = {k: B * steps / (med[k] / 1e3) for k in var}
            faster = lambda v, ref: (v if max(ms[v]) < min(ms[ref]) else  # noqa: E731
                                     ref if min(ms[v]) > max(ms[ref]) else "none")
            extra = {}
            if plain is not None:
                pres = measure(plain, mname, mode)
                if pres is None:
                    break
                pmed = {k: float(np.median(v)) for k, v in pres[2].items()}
                extra = {"signals": True, "plain_mean_iters_per_solve": round(float(pres[0]["fleet"].mean()), 1),
                         "plain_median_ms": {k: round(v, 4) for k, v in pmed.items()},
                         "sig_over_plain": {k: round(pmed[k] / med[k], 3) for k in var}}
            print(json.dumps({
                "batch": B, "classes": K, "mode": mname, "kernels": kern,
                "mean_iters_per_solve": round(float(its["fleet"].mean()), 1),
                "max_iters_per_solve": int(its["fleet"].max()),
                "kernel_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                "wall_ms": {k: [round(x, 4) for x in v] for k, v in wall.items()},
                "median_ms": {k: round(v, 4) for k, v in med.items()},
                "mpc_steps_per_s": {k: round(v, 1) for k, v in rate.items()},
                **{f"{v}_over_fleet": round(rate[v] / rate["fleet"], 3) for v in var if v != "fleet"},
                **{f"{v}_faster": faster(v, "fleet") for v in var if v not in ("fleet", "shared", "shared_panel")},
                "classes_fused_over_classes_best": round(
                    rate["classes_fused"] / max(rate[v] for v in ("classes", "classes_panel", "classes_async")), 3),
                **({"classes_fused_over_shared_panel": round(rate["classes_fused"] / rate["shared_panel"], 3),
                    "classes_fused_vs_shared_panel_faster": faster("classes_fused", "shared_panel")}
                   if "shared_panel" in var else {}),
                **({"classes_over_shared": round(rate["classes"] / rate["shared"], 3),
                    "classes_vs_shared_faster": faster("classes", "shared")} if "shared" in var else {}),
                **({"share_code5": {k: round(float((cds[k] == 5).mean()), 4) for k in var},
                    "share_capped": {k: round(float(((cds[k] == 0) & (its[k] == mode["N"])).mean()), 4) for k in var},
                    "infeas_mean_iters_per_solve": round(float(its["classes_infeas"].mean()), 1),
                    "infeas_max_iters_per_solve": int(its["classes_infeas"].max()),
                    **{f"{i}_over_{v}": round(rate[i] / rate[v], 3) for i in INF for v in var if v not in INF},
                    "infeas_res_over_infeas": {"classes": round(rate["classes_infeas_res"] / rate["classes_infeas"], 3),
                                               "fleet": round(rate["fleet_infeas_res"] / rate["fleet_infeas"], 3)},
                    "infeas_async_over_infeas_res": {
                        "classes": round(rate["classes_infeas_async"] / rate["classes_infeas_res"], 3),
                        "fleet": round(rate["fleet_infeas_async"] / rate["fleet_infeas_res"], 3)}}
                   if args.infeas else {}),
                **extra}),
                flush=True)
        for s, _ in list(var.values()) + list((plain or {}).values()):
            s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="*", default=None)
    ap.add_argument("--fleet", action="store_true")
    ap.add_argument("--signals", action="store_true")
    ap.add_argument("--panel", action="store_true")
    ap.add_argument("--classes", type=int, default=0, metavar="K")
    ap.add_argument("--infeas", action="store_true")
    ap.add_argument("--skip-plain", action="store_true")
    args = ap.parse_args()
    if args.classes:
        if args.fleet or args.panel or args.classes < 1:
            ap.error("--classes K >= 1 goes with --signals alone")
        if args.batches is None:
            args.batches = [256, 2048, 8192]
        return classes_ab(args)
    if args.fleet and args.signals:
        ap.error("--fleet and --signals exclude each other")
    if args.batches is None:
        args.batches = ([256, 2048, 8192] if args.panel else [1, 64, 256, 2048, 8192] if args.fleet else
                        [1, 64, 256, 512, 2048, 8192])
    mismatch = args.fleet and args.panel  # shared matrices, per-pack plant maps
    rounds = max(3, args.rounds)
    import torch

    import gpad_mpc
    from gpad_mpc import problems
    dev = torch.device("cuda:0")
    qp, pl = problems.battery_plant(4, 10)
    n, m, nx, nu, steps = qp.n, qp.m, pl.nx, pl.nu, args.steps
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))).to(dev)  # noqa: E731
    dML, dG, dPM, dPg, dg0, dA, dB = (t32(a) for a in (qp.ML, qp.G, pl.PM, pl.Pg, pl.g0, pl.A, pl.B))
    if args.signals:
        qs, ps = problems.battery_plant_signals(4, 10)
        dSM, dSg, dE = (t32(a) for a in (ps.SM, ps.Sg, ps.E))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(json.dumps({"plant": "battery_fleet(4, 10)" if args.fleet else "battery_plant(4, 10)", "n": n, "m": m,
                      "steps": steps, "rounds": rounds, "device": torch.cuda.get_device_name(0), "cus": cus}))
    for B in args.batches:
        X0 = torch.from_numpy((np.random.default_rng(B).random((B, nx)) - 0.5).astype(np.float32)).to(dev)
        if args.fleet:
            qp, pl = problems.battery_fleet(4, 10, problems.battery_fleet_caps(B, 4, B))
            if mismatch:
                qp.ML, qp.G, pl.PM = qp.ML[0], qp.G[0], np.stack([pl.PM[0]] * B)
            dML, dG, dPM, dPg, dg0, dA, dB = (t32(a) for a in (qp.ML, qp.G, pl.PM, pl.Pg, pl.g0, pl.A, pl.B))
        var = {}
        sig = None
        # --infeas: the lockstep loop (and with --panel the panel loop) with the battery bound bound, on the plant
        # with signals when --signals is given (its loads make infeasible steps), else on the plain plant
        pre = "sig_" if args.signals else ""
        infeas_names = ((pre + "infeas",) + ((pre + "infeas_panel",) if args.panel else ()) +
                        (pre + "infeas_async",)) if args.infeas else ()
        if args.signals:
            rng = np.random.default_rng([B, 1])
            sig = torch.from_numpy(np.concatenate([rng.uniform(-5, 5, (steps, B, 1)),
                                                   rng.uniform(-0.1, 0.1, (steps, B, nx))],
                                                  axis=-1).astype(np.float32)).to(dev)
        for name in ("lockstep", "async") + (("async_1wg",) if args.fleet and not mismatch else ()) + (
                ("panel",) if args.panel else ()) + (("sig_lockstep", "sig_async") if args.signals else ()) + (
                ("sig_panel",) if args.signals and args.panel else ()) + infeas_names:
            s = gpad_mpc.GpadSolver(0)
            s.setup(dML, dG, float(np.float32(qp.L)), n=n, m=m, batch=B, shared=mismatch or not args.fleet)
            s.setup_plant(dPM, dPg, g0=dg0, A=dA, B=dB)
            if name.startswith("sig_"):
                s.setup_signals(dSM, dSg, dE)
            s.set_option("loop_async", int("async" in name))
            if args.panel:  # (left alone otherwise: the tool also runs on builds older than the option)
                s.set_option("loop_panel", int(name.endswith("panel")))
            if name in infeas_names:
                if name.endswith("infeas_async"):
                    s.set_infeasibility_loop_async(True)
                s.setup_infeasibility(problems.battery_zbound())
            if name == "async_1wg":
                s.set_option("duo_max_grid", cus)
            buf = dict(x=torch.empty(B, nx, device=dev), z=torch.empty(B, n, device=dev),
                       y=torch.empty(B, m, device=dev), xs=torch.empty(steps, B, nx, device=dev),
                       us=torch.empty(steps, B, nu, device=dev))
            var[name] = (s, buf)

        def enqueue(name, mode, **kw):
            s, b = var[name]
            b["x"].copy_(X0)
            b["z"].zero_()
            b["y"].zero_()
            torch.cuda.synchronize()
            return s.closed_loop(b["x"], b["z"], b["y"], steps, mode["N"], mode["tol"], warm=mode["warm"],
                                 xs=b["xs"], us=b["us"], signals=sig if name.startswith("sig_") else None, **kw)

        for mname, mode in MODES.items():
            its, kern, cds = {}, {}, {}
            for name in var:  # the output check, and each variant's warm-up
                its[name], cds[name] = np.zeros(steps * B, np.int32), np.zeros(steps * B, np.int32)
                kern[name] = enqueue(name, mode, iters=its[name], codes=cds[name])["kernel"]
            # (a bound variant's outputs are not the unbound loop's by design: the bound variants are compared
            # with the first of them)
            base = lambda v: (infeas_names[0] if v in infeas_names else  # noqa: E731
                              "sig_lockstep" if v.startswith("sig_") else "lockstep")
            bad = [k for k in ("x", "z", "y", "xs", "us") for v in var if v != base(v)
                   if not torch.equal(var[base(v)][1][k].view(torch.int32), var[v][1][k].view(torch.int32))]
            if any(not np.array_equal(its[base(v)], its[v]) or not np.array_equal(cds[base(v)], cds[v]) for v in var):
                bad.append("iters")
            want = lambda v: "loop_panel" if v.endswith("panel") else "loop"  # noqa: E731
            if bad or any((kern[v] == want(v)) != (v != base(v)) or kern[v] is None for v in var):
                print(json.dumps({"batch": B, "mode": mname, "error": "outputs differ" if bad else "wrong kernel",
                                  "differ": bad, "kernels": kern}))
                break
            ms = {k: [] for k in var}
            wall = {k: [] for k in var}
            for _ in range(rounds):
                for name in var:
                    s = var[name][0]
                    t0 = time.perf_counter()
                    enqueue(name, mode, stats=False)
                    s.sync()
                    wall[name].append((time.perf_counter() - t0) * 1e3)
                    ms[name].append(s.last_stats()["kernel_ms"])
            med = {k: float(np.median(v)) for k, v in ms.items()}
            rate = {k: B * steps / (med[k] / 1e3) for k in var}
            faster = ("async" if max(ms["async"]) < min(ms["lockstep"]) else
                      "lockstep" if min(ms["async"]) > max(ms["lockstep"]) else "none")
            print(json.dumps({
                "batch": B, "mode": mname, "lockstep_kernel": kern["lockstep"],
                "mean_iters_per_solve": round(float(its["async"].mean()), 1),
                "max_iters_per_solve": int(its["async"].max()),
                "kernel_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                "wall_ms": {k: [round(x, 4) for x in v] for k, v in wall.items()},
                "mpc_steps_per_s": {k: round(v, 1) for k, v in rate.items()},
                "async_over_lockstep": round(rate["async"] / rate["lockstep"], 3), "faster": faster,
                **({"async_1wg_over_async": round(rate["async_1wg"] / rate["async"], 3)} if "async_1wg" in var else {}),
                **({"panel_over_lockstep": round(rate["panel"] / rate["lockstep"], 3),
                    "panel_over_async": round(rate["panel"] / rate["async"], 3),
                    "panel_faster": ("panel" if max(ms["panel"]) < min(ms["lockstep"]) else
                                     "lockstep" if min(ms["panel"]) > max(ms["lockstep"]) else "none")}
                   if args.panel else {}),
                **({"sig_panel_over_sig_lockstep": round(rate["sig_panel"] / rate["sig_lockstep"], 3)}
                   if args.panel and args.signals else {}),
                **({"share_code5": {k: round(float((cds[k] == 5).mean()), 4) for k in var},
                    "share_capped": {k: round(float(((cds[k] == 0) & (its[k] == mode["N"])).mean()), 4) for k in var},
                    "infeas_mean_iters_per_solve": round(float(its[infeas_names[0]].mean()), 1),
                    **{f"{i}_over_{v}": round(rate[i] / rate[v], 3) for i in infeas_names for v in var
                       if v not in infeas_names and v.startswith("sig_") == bool(pre)},
                    "infeas_async_over_infeas": round(rate[pre + "infeas_async"] / rate[pre + "infeas"], 3)}
                   if args.infeas else {}),
                **({"sig_mean_iters_per_solve": round(float(its["sig_async"].mean()), 1),
                    "sig_async_over_sig_lockstep": round(rate["sig_async"] / rate["sig_lockstep"], 3),
                    "sig_over_plain": {"lockstep": round(rate["sig_lockstep"] / rate["lockstep"], 3),
                                       "async": round(rate["sig_async"] / rate["async"], 3)}}
                   if args.signals else {})}),
                flush=True)
        for s, _ in var.values():
            s.close()


if __name__ == "__main__":
    main()
