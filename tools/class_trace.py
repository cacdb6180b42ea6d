"""Kernel timeline of one closed loop of a fleet of K plant classes, per binding: where the time of
tools/loop_ab.py --classes goes.

  rocprofv3 --kernel-trace --output-format csv -d OUT -o run -- \
      python tools/class_trace.py run {fleet|classes|classes_panel|classes_async} [--classes 4] [--batch 8192]
                                      [--mode eps_warm] [--steps 20]
  python tools/class_trace.py summary OUT/.../run_kernel_trace.csv

`run` binds the variant as tools/loop_ab.py --classes does (same seeds), runs the loop once as a warm-up
(the phased panels plan from the previous solve), sleeps a second, and runs it once more.  `summary`
reads the kernel trace, keeps the kernels after the longest pause (the second loop) and prints, per
kernel name, launches and summed duration, then the span from the first start to the last end, the time
some kernel was running, and the gaps between kernels.
"""
from __future__ import annotations

import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gpu-dualgradient-mpc_amd"), os.path.join(ROOT, "tools")]


def run(args):
    import torch

    import gpad_mpc
    from gpad_mpc import problems
    from loop_ab import MODES
    K, B, steps, mode = args.classes, args.batch, args.steps, MODES[args.mode]
    dev = torch.device("cuda:0")
    qp, pl = problems.battery_fleet(4, 10, problems.battery_fleet_caps(K, 4, K))
    n, m, nx, nu = qp.n, qp.m, pl.nx, pl.nu
    L = float(np.float32(qp.L))
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))).to(dev)  # noqa: E731
    cls = {k: t32(a) for k, a in dict(ML=qp.ML, G=qp.G, PM=pl.PM, Pg=pl.Pg, g0=pl.g0, A=pl.A, B=pl.B).items()}
    class_of = np.arange(B, dtype=np.int32) % K
    X0 = torch.from_numpy((np.random.default_rng(B).random((B, nx)) - 0.5).astype(np.float32)).to(dev)
    s = gpad_mpc.GpadSolver(0)
    if args.variant == "fleet":
        idx = torch.from_numpy(class_of.astype(np.int64)).to(dev)
        f = {k: a[idx].contiguous() for k, a in cls.items()}
        s.setup(f["ML"], f["G"], L, n=n, m=m, batch=B, shared=False)
        s.setup_plant(f["PM"], f["Pg"], g0=f["g0"], A=f["A"], B=f["B"])
    else:
        s.setup_classes(cls["ML"], cls["G"], L, class_of, n=n, m=m)
        s.setup_plant(cls["PM"], cls["Pg"], g0=cls["g0"], A=cls["A"], B=cls["B"])
        s.set_options(loop_panel=int(args.variant == "classes_panel"), loop_async=int(args.variant == "classes_async"))
    x, z, y = torch.empty(B, nx, device=dev), torch.empty(B, n, device=dev), torch.empty(B, m, device=dev)
    xs, us = torch.empty(steps, B, nx, device=dev), torch.empty(steps, B, nu, device=dev)
    for i in range(2):
        x.copy_(X0)
        z.zero_()
        y.zero_()
        torch.cuda.synchronize()
        time.sleep(0.3 + 0.7 * i)  # the longest pause of the trace comes right before the second loop
        st = s.closed_loop(x, z, y, steps, mode["N"], mode["tol"], warm=mode["warm"], xs=xs, us=us)
    print(f"{args.variant} K={K} batch={B} {args.mode}: kernel {st['kernel']}, kernel_ms {st['kernel_ms']:.3f}, "
          f"iterations max {st['iterations']} total {st['total_iterations']}")
    s.close()


def summary(args):
    rows = []
    with open(args.csv, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    cut = max(range(1, len(rows)), key=lambda i: rows[i][0] - rows[i - 1][1])
    rows = rows[cut:]
    per = {}
    for a, b, name in rows:
        short = name.split("(")[0].replace("void ", "").replace("gpad::", "")
        c = per.setdefault(short, [0, 0])
        c[0] += 1
        c[1] += b - a
    span = rows[-1][1] - rows[0][0]
    busy, end = 0, rows[0][0]
    for a, b, _ in rows:  # union of the kernels' intervals
        if b > end:
            busy += b - max(a, end)
            end = b
    print(f"{os.path.basename(os.path.dirname(args.csv)) or args.csv}: {len(rows)} launches, span {span / 1e6:.3f} ms, "
          f"some kernel running {busy / 1e6:.3f} ms, gaps {(span - busy) / 1e6:.3f} ms")
    for name, (cnt, ns) in sorted(per.items(), key=lambda kv: -kv[1][1]):
        print(f"  {ns / 1e6:9.3f} ms  {cnt:5d} x  {name[:100]}")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("variant", choices=["fleet", "classes", "classes_panel", "classes_async"])
    r.add_argument("--classes", type=int, default=4)
    r.add_argument("--batch", type=int, default=8192)
    r.add_argument("--mode", default="eps_warm")
    r.add_argument("--steps", type=int, default=20)
    q = sub.add_parser("summary")
    q.add_argument("csv")
    args = ap.parse_args()
    (run if args.cmd == "run" else summary)(args)


if __name__ == "__main__":
    main()
