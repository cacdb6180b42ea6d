"""Inputs of tests/test_bigpanel.py: the shape table of the big-panel kernel (csrc/gpad_bigpanel.hip), its
geometry restated from the kernel's documented rules (nothing here is imported from the library), the problems,
and the CPU oracle's solves (the instances of a batch on a thread pool).  TEST INFRASTRUCTURE ONLY.

Geometry, as gpad_bigpanel.hip states it: T1 = ceil(n / 16) and T2 = ceil(m / 16) row tiles; 16 waves, wave w
owning tiles w, w + 16, ... of both GEMMs, NT = 1, 2 or 4 tile slots per wave (ceil(T / 16) rounded up);
GEMM 1 (zhat = -ML w) runs T2 k-blocks whose last has kq1 = ceil((m - 16 (T2 - 1)) / 4) four-steps, GEMM 2
(G/L zhat, also the u seed and the verification of test (A)) runs T1 k-blocks whose last has kq2 likewise from
n; LDS = (T1 + 2 T2) KiB + 16 test slots of 384 B; supported: one of T1, T2 past 16, both at most 64, LDS at
most 160 KiB.

Problems: problems.synthetic_qp(n, m, batch, seed) with its own L.  Fixed-N runs take it as it stands with warm
z0, y0.  Tolerance runs add a per-instance slack to g, g[b] += s_b with s_b drawn from SLACKS: an instance whose
unconstrained optimum becomes feasible passes test (A) at its first test (code 1) while its panel neighbours run
on to test (B) (code 2) or to the cap (code 0).
"""
from __future__ import annotations

import os
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

WAVES, MAX_TILES, LDS_LIMIT = 16, 64, 160 * 1024
SLOT_BYTES = 3 * 64 + 128 + 64  # TestSlot<float>: violz, violh, wmin [16] floats, gap [16] doubles, magh [16] floats
B = 35  # two full panels and a ragged one of 3
SMALL_BATCHES = (1, 16)  # further batch sizes of SMALL
N_FIXED = 23
SLACKS = (0.0, 0.0, 0.3, 1.0, 3.0, 30.0)
SLACK_SEED = 5

# n, m; what the issue's table states of the shape (the CPU tests hold the restated geometry to it); the tolerance
# run: seed of synthetic_qp, tol, check_every, N -- chosen on the CPU oracle, test_bigpanel.test_conditions_cpu
# holds them to the conditions.
Case = namedtuple("Case", "n m T1 T2 nt kq1 kq2 seed tol check_every N what")

TABLE = [
    Case(60, 270, 4, 17, (1, 2), 4, 3, 17, 1e-2, 50, 400, "battery_plant(4, 15)'s shape; T2 = 17: wave 0 pairs"),
    Case(16, 272, 1, 17, (1, 2), 4, 4, 17, 1e-2, 50, 400, "GEMM 2 nkb = 1, full tiles"),
    Case(5, 513, 1, 33, (1, 4), 1, 2, 17, 1e-2, 50, 400, "nkb = 1 with a ragged k-block; T2 = 33"),
    Case(32, 1024, 2, 64, (1, 4), 4, 4, 17, 1e-2, 50, 400, "nkb = 2; T2 = 64 all paired"),
    Case(416, 1024, 26, 64, (2, 4), 4, 4, 17, 1e-2, 50, 200, "LDS exactly 163 840 B"),
    Case(257, 769, 17, 49, (2, 4), 1, 1, 17, 1e-2, 50, 400, "both bucket edges + 1; kq = 1 both"),
    Case(512, 512, 32, 32, (2, 2), 4, 4, 17, 1e-2, 50, 400, "all-paired NT2 = 2; full tiles"),
    Case(272, 256, 17, 16, (2, 1), 4, 4, 17, 1e-3, 50, 400, "all 16 waves hold a GEMM-2 tile"),
    Case(513, 17, 33, 2, (4, 1), 1, 1, 17, 1e-3, 50, 400, "GEMM 1 nkb = 2; 14 waves have no GEMM-2 tile"),
    Case(1024, 16, 64, 1, (4, 1), 4, 4, 17, 1e-3, 50, 400, "GEMM 1 nkb = 1"),
    Case(768, 48, 48, 3, (4, 1), 4, 4, 17, 1e-3, 50, 400, "nkb = 3, odd; T1 = 48, the fourth slot empty"),
    Case(769, 500, 49, 32, (4, 2), 1, 1, 17, 1e-2, 50, 400, "T1 = 49; m = 500: a one-step last block"),
    Case(1024, 720, 64, 45, (4, 4), 4, 4, 17, 1e-2, 50, 200, "LDS exactly 163 840 B on the other side"),
    # beyond the issue's table: its shapes give kq1 in {1, 4} only, these two add kq1 = 2 and 3
    Case(40, 264, 3, 17, (1, 2), 2, 2, 18, 1e-3, 50, 400, "kq1 = 2, kq2 = 2; GEMM 2 nkb = 3"),
    Case(300, 267, 19, 17, (2, 2), 3, 3, 17, 1e-3, 50, 400, "kq1 = 3, kq2 = 3; odd nkb in both GEMMs"),
]
LDS_EDGE = [(416, 1024), (1024, 720)]  # LDS == LDS_LIMIT: a test function of their own
REFUSED = [(417, 1024), (1024, 721), (1024, 1024), (1025, 16), (16, 1025)]
SMALL = (60, 270)  # also at the batch sizes of SMALL_BATCHES, and the shape of the routing and plant tests
ALL_NT = [(1, 2), (1, 4), (2, 1), (2, 2), (2, 4), (4, 1), (4, 2), (4, 4)]  # (1, 1) belongs to the T-wave panels


def case_id(c):
    return "%dx%d" % (c.n, c.m)


def case_of(n, m):
    return next(c for c in TABLE if (c.n, c.m) == (n, m))


# ------------------------------------------------------------------------------ the geometry, restated
def big_tiles(x):
    return (x + 15) // 16


def nt_of(tiles):
    q = (tiles + WAVES - 1) // WAVES
    return 1 if q <= 1 else 2 if q <= 2 else 4


def kq(k):
    """Four-steps of the last k-block of a GEMM over k columns."""
    return (k - 16 * (big_tiles(k) - 1) + 3) // 4


def geometry(n, m):
    """T1, T2, (NT1, NT2), kq1, kq2, nkb1, nkb2."""
    t1, t2 = big_tiles(n), big_tiles(m)
    return dict(T1=t1, T2=t2, nt=(nt_of(t1), nt_of(t2)), kq1=kq(m), kq2=kq(n), nkb1=t2, nkb2=t1)


def lds_bytes(n, m):
    return (big_tiles(n) + 2 * big_tiles(m)) * 1024 + WAVES * SLOT_BYTES


def supported(n, m):
    t1, t2 = big_tiles(n), big_tiles(m)
    return n > 0 and m > 0 and (t1 > 16 or t2 > 16) and t1 <= MAX_TILES and t2 <= MAX_TILES and \
        lds_bytes(n, m) <= LDS_LIMIT


def nkb_class(nkb):
    """The paths of big_gemm / big_gemm2: nkb = 1 (no full block), 2 (one, outside the loop), 3 (one pass of the
    loop, nothing after it), then odd counts (the loop alone) and even counts (the loop and the block after it)."""
    return {1: "1", 2: "2", 3: "3"}.get(nkb, "odd" if nkb % 2 else "even")


def pairing(tiles):
    """(waves that run two tiles interleaved in big_gemm2, waves that run a single big_gemm) over the slot pairs
    (q, q + 1), q even, of a GEMM-2 side with `tiles` row tiles."""
    pairs = singles = 0
    for w in range(WAVES):
        for q in range(0, nt_of(tiles), 2):
            t = w + WAVES * q
            if nt_of(tiles) > 1 and t + WAVES < tiles:
                pairs += 1
            elif t < tiles:
                singles += 1
    return pairs, singles


# ------------------------------------------------------------------------------ problems
F32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))  # noqa: E731
_problem_cache = {}


def problem(n, m, batch, seed):
    """(ML, M, G, g, L) of synthetic_qp in f32, M and g [batch][.]."""
    k = (n, m, batch, seed)
    if k not in _problem_cache:
        from gpad_mpc import problems
        qp = problems.synthetic_qp(n, m, batch=batch, seed=seed)
        M, g = np.atleast_2d(qp.M), np.atleast_2d(qp.g)
        _problem_cache[k] = (F32(qp.ML), F32(M), F32(qp.G), F32(g), np.float32(qp.L))
    return _problem_cache[k]


def slacks(batch):
    return np.random.default_rng(SLACK_SEED).choice(SLACKS, size=batch)


def slack_problem(n, m, batch, seed):
    ML, M, G, g, L = problem(n, m, batch, seed)
    return ML, M, G, F32(g.astype(np.float64) + slacks(batch)[:, None]), L


def starts(n, m, batch, warm):
    """z0 ~ 0.1 N(0, 1), y0 = |0.1 N(0, 1)| (warm: w_0 = y_0, u seeded from G_L z_{-1}), or zeros."""
    if not warm:
        return np.zeros((batch, n), np.float32), np.zeros((batch, m), np.float32)
    rng = np.random.default_rng([n, m, 3])
    return F32(0.1 * rng.normal(size=(batch, n))), F32(np.abs(0.1 * rng.normal(size=(batch, m))))


# ------------------------------------------------------------------------------ the oracle
_pool = None
_oracle_cache = {}


def oracle_batch(oracle, key, prob, z0, y0, N, tol, check_every):
    """oracle.solve_f32(..., code=True) of every instance, once per session and key: (z, y, iters, codes).  The
    library call releases the GIL and keeps no state, so the instances run on a thread pool."""
    global _pool
    k = (key, N, tol, check_every)
    if k not in _oracle_cache:
        if _pool is None:
            _pool = ThreadPoolExecutor(max(1, min(16, os.cpu_count() or 1)))
        ML, M, G, g, L = prob
        rows = list(_pool.map(lambda b: oracle.solve_f32(z0[b], y0[b], ML, M[b], G, g[b], N, L, tol,
                                                         check_every=check_every, code=True), range(M.shape[0])))
        out = (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]),
               np.array([r[2] for r in rows], np.int32), np.array([r[3] for r in rows], np.int32))
        for a in out:
            a.setflags(write=False)
        _oracle_cache[k] = out
    return _oracle_cache[k]


def fixed_oracle(oracle, c, batch=B):
    z0, y0 = starts(c.n, c.m, batch, True)
    prob = problem(c.n, c.m, batch, c.seed)
    return prob, z0, y0, oracle_batch(oracle, ("fixed", c.n, c.m, batch, c.seed), prob, z0, y0, N_FIXED, 0.0, 10)


def tol_oracle(oracle, c, warm, batch=B):
    z0, y0 = starts(c.n, c.m, batch, warm)
    prob = slack_problem(c.n, c.m, batch, c.seed)
    return prob, z0, y0, oracle_batch(oracle, ("tol", c.n, c.m, batch, c.seed, warm), prob, z0, y0, c.N, c.tol,
                                      c.check_every)


def mixed_panels(iters, codes):
    """Panels (instances 16 p .. 16 p + 15 of the unphased run) in which a code-1 and a code-2 finish fall on the
    same iteration."""
    out = []
    for p in range((len(iters) + 15) // 16):
        it, cd = iters[16 * p:16 * p + 16], codes[16 * p:16 * p + 16]
        if set(it[cd == 1].tolist()) & set(it[cd == 2].tolist()):
            out.append(p)
    return out
