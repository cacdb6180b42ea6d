"""The phase schedule of a phased panel solve, pinned from two sides.

The parity tests are bit-exact under ANY schedule (a column's arithmetic does not depend on its
phase), so a phase driver that launched other phases, or a planner that planned others, would pass
them and only cost speed.  Here:

* test_phase_planner_matches_pins (CPU): gpad_plan_phases (csrc/gpad_phases.cpp panel_plan) returns,
  for the C4-like spread of test_abi.test_phase_planner_host_only and the 400 random inputs of
  test_abi.test_phase_planner_random_inputs (same seeds, same draws), exactly the plans recorded in
  tests/golden/plan_pins.json -- ends, fins and the modelled cost as a hex float.
* test_launched_phases_follow_the_rule (GPU): what the driver launched (gpad_last_phases) on the
  three driver branches -- T-wave panels, panel pairs, big panels -- equals the documented default
  rule derived here (plan off), and, with the plan on, the plan gpad_plan_phases makes from the
  previous solve's counts.

``python tests/test_phase_schedule.py --write`` records the fixture from the built library.
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

PINS = os.path.join(GOLDEN, "plan_pins.json")


def _planner_inputs():
    """(iters, n, m, N, check_every, num_cus) of the two planner tests of test_abi, draw for draw."""
    rng = np.random.default_rng(0)
    yield np.clip(rng.normal(265, 30, 8192), 170, 380).astype(np.int32), 200, 200, 5000, 10, 256
    rng = np.random.default_rng(3)
    for _ in range(400):
        B = int(rng.choice([1, 2, 15, 16, 17, 255, 1000, 4096, 8193, 70000]))
        N = int(rng.choice([1, 9, 10, 11, 100, 300, 5000, 20000]))
        K = int(rng.choice([1, 2, 5, 10, 16, 100]))
        kind = rng.integers(0, 4)
        if kind == 0:
            it = rng.integers(0, N + 50, B)
        elif kind == 1:
            it = np.clip(rng.normal(rng.uniform(0, N + 1), rng.uniform(1, 200), B), 0, N)
        elif kind == 2:
            it = np.full(B, int(rng.integers(0, N + 1)))
        else:
            it = rng.geometric(rng.uniform(0.001, 0.5), B)
        n, m = int(rng.choice([8, 40, 129, 200, 208, 256])), int(rng.choice([8, 64, 180, 200, 256]))
        yield it.astype(np.int32), n, m, N, K, int(rng.choice([1, 8, 256, 304]))


def _plans():
    from gpad_mpc.solver import GpadSolver
    out = []
    for it, n, m, N, K, cus in _planner_inputs():
        p = GpadSolver.plan_phases(it, n, m, N, K, cus)
        out.append([p["ends"], p["fins"], float(p["cost_us"]).hex()])
    return out


def test_phase_planner_matches_pins():
    with open(PINS) as f:
        pins = json.load(f)
    got = _plans()
    assert len(got) == len(pins) == 401
    assert sum(1 for p in pins if p[0]) > 100  # the fixture pins real plans, not a run of empty ones
    for i, (g, p) in enumerate(zip(got, pins)):
        assert g == p, (i, g, p)


# ---- what the driver launches --------------------------------------------------------------------
def _default_ends(N, length):
    """csrc/gpad_phases.cpp launch_panel_phases with no plan and no explicit phase length: phases of
    `length` iterations (four tests), from the tenth phase on doubling (length << (ph - 9)), the last
    one closing at N."""
    ends, v, ph = [], 0, 0
    while v < N:
        v = min(N, v + (length if ph < 10 else length << (ph - 9)))
        ends.append(v)
        ph += 1
    return ends


def _fin_supported(n, m):
    """The resident finisher's shapes (csrc/gpad_resident.hip resident_supported: rows up to 208, one
    lane per row of z and of y in at most 512 threads)."""
    return max(n, m) <= 208 and 64 * ((n + 63) // 64 + (m + 63) // 64) <= 512


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,B", [(40, 72, 150), (200, 200, 120), (300, 300, 20)])
def test_launched_phases_follow_the_rule(gpu, n, m, B):
    """(a) plan off: the default rule -- multiples of 40 up to the tenth phase, then doubling, closing
    at N (N chosen just past what the slowest instance needs, so the run-out doubles), and with an
    explicit phase_len = 10 uniform phases to N = 400; fins[0] == 0, later fins twice the CU count where
    the resident finisher takes the shape, else 0.  (b) plan on: the second of two identical solves
    follows gpad_plan_phases of the first one's counts (its ends; its fins from the second phase on --
    the first phase has no finisher -- where the finisher takes the shape).  N = 2370 / 400 with these batches are no other
    test's shape, so the process-wide shape prior (keyed by n, m, batch, K, N) decides no first solve
    here; (a) runs with the plan off anyway."""
    import torch

    import gpad_mpc
    from gpad_mpc import _lib, problems
    from gpad_mpc.solver import GpadSolver
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tol, K = 1e-4, 10
    qp = problems.synthetic_qp(n, m, batch=B, seed=21)
    ML, G = qp.ML.astype(np.float32), qp.G.astype(np.float32)
    M, g = qp.M.astype(np.float32), qp.g.astype(np.float32)
    L = float(np.float32(qp.L))
    fin = 2 * cus if _fin_supported(n, m) else 0

    def solve(s, N):
        z, y, it = np.zeros((B, n), np.float32), np.zeros((B, m), np.float32), np.zeros(B, np.int32)
        st = s.run(z, y, M, g, N, tol, iters=it)
        assert st["kernel"] == "panel"
        return it, s.last_phases()

    with gpad_mpc.GpadSolver(0) as s:
        s.setup(ML, G, L, n=n, m=m, batch=B, check_every=K, kernel=_lib.KERNEL_PANEL)
        # (a) the default rule: 40, 80, ..., 400, 480, 640, 960, 1600, 2370
        s.set_options(plan=0, phase_len=0)
        N = 2370
        it0, p = solve(s, N)
        want = _default_ends(N, 4 * K)
        assert want[:11] == [40 * (k + 1) for k in range(10)] + [480] and want[-1] == N and len(want) == 15
        print(f"({n}, {m}) default: {p['ends']} fins {p['fins']} counts {p['counts']}")
        assert not p["prior"]
        assert p["ends"] == want
        assert p["fins"] == [0] + [fin] * (len(want) - 1)
        # ... and an explicit length stays uniform
        s.set_options(phase_len=10)
        _, p = solve(s, 400)
        assert p["ends"] == [10 * (k + 1) for k in range(40)]
        assert p["fins"] == [0] + [fin] * 39
        # (b) planned from the previous solve
        s.set_options(plan=1, phase_len=0)
        it1, _ = solve(s, N)
        np.testing.assert_array_equal(it1, it0)
        it2, p2 = solve(s, N)
        np.testing.assert_array_equal(it2, it0)
        plan = GpadSolver.plan_phases(it1, n, m, N, K, cus)
        print(f"({n}, {m}) planned: {p2['ends']} fins {p2['fins']} plan {plan}")
        if n <= 256 and m <= 256:  # the planner plans the T-wave and pair kernels' shapes only
            assert len(plan["ends"]) >= 1 and plan["ends"][-1] == N
            assert p2["ends"] == plan["ends"]
            assert p2["fins"] == [0] + [f if fin else 0 for f in plan["fins"][1:]]
        else:  # no plan: the default rule again
            assert plan["ends"] == []
            assert p2["ends"] == want and p2["fins"] == [0] + [fin] * (len(want) - 1)
        assert not p2["prior"]


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["--write"]:
        ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        sys.path.insert(0, os.path.join(ROOT, "gpu-dualgradient-mpc_amd"))
        with open(PINS, "w") as f:
            json.dump(_plans(), f, separators=(",", ":"))
            f.write("\n")
        print("wrote", PINS)
