"""Reference of the adaptive restart (GPAD_OPT_RESTART, include/gpad.h): test infrastructure.

A restart taken after the iteration of index k (count k + 1) makes iteration k + 1 run with w = y+ and
theta[0], and the schedule count on from position 0.  theta and beta are separate table entries per
iteration, so while the iterates are finite this is the plain solve with a per-instance table

    theta'[k + 1 + i] = theta[i],   beta'[k + 1] = 0 (fma(0, d, y) = y),   beta'[k + 1 + i] = beta[i], i >= 1

and the existing oracle, unchanged, gives z*, y*, counts and codes once the restart iterations are known.
``restart_tables`` only reproduces the decisions: a step loop over Oracle.step1..4 (f32) or plain numpy (f64)
that takes each decision on q = sum (w - y+)(y+ - y) -- the differences rounded once in the dtype, the
products in fp64 (exact for f32), the sum by math.fsum.  A kernel sums the same products in its own order: an
fp64 sum of m <= 256 terms errs by less than m 2^-53 of sum |terms|, so a decision with
|q| <= 2^-30 sum |terms| is called ambiguous (a wide margin) and its instance is left out of a comparison.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

AMBIGUOUS = 2.0 ** -30
MAX_LEFT_OUT = 0.02  # a test fails when more than this share of its instances is ambiguous


def _step_f64(MGneg, gP, GL, pD, z, y, ym1, theta, beta):
    """One iteration of oracle/gpad_oracle.c orc_solve_f64_h on scaled operands (numpy dots: the decisions only)."""
    w = y + beta * (y - ym1)
    zh = MGneg @ w - gP
    z = (1.0 - theta) * z + theta * zh
    s = (w + GL @ zh) + pD
    return w, z, np.where(s > 0.0, s, 0.0)


def restart_tables(oracle, z0, y0, MGneg, gP, GL, pD, N, R, theta, beta):
    """The N-iteration step loop with a decision after every iteration whose count is a multiple of R (R = 0:
    none) and below N.  Returns (theta', beta', restarts, decisions): the spliced tables, the counts (from 1) of
    the iterations after which the instance restarted, and per decision (count, |q| / sum |terms|, sum |terms|).
    The termination test is not run here: the caller cuts the lists at the table solve's final count."""
    f64 = np.asarray(MGneg).dtype == np.float64
    dt = np.float64 if f64 else np.float32
    th = np.array(theta[:N], dt)
    be = np.array(beta[:N], dt)
    z = np.array(z0, dt).reshape(-1)
    y = np.array(y0, dt).reshape(-1)
    ym1 = y.copy()
    restarts, decisions = [], []
    for v in range(N):
        if f64:
            w, z, yp = _step_f64(MGneg, gP, GL, pD, z, y, ym1, th[v], be[v])
        else:
            w = oracle.step1(y, ym1, dt(be[v]))
            zh = oracle.step2(MGneg, w, gP)
            z = oracle.step3(dt(th[v]), z, zh)
            yp = oracle.step4(GL, w, pD, zh)
        c = v + 1
        if R > 0 and c % R == 0 and c < N:
            terms = (w - yp).astype(np.float64) * (yp - y).astype(np.float64)
            q, tot = math.fsum(terms), math.fsum(np.abs(terms))
            decisions.append((c, abs(q) / tot if tot > 0.0 else math.inf, tot))
            if q > 0.0:
                restarts.append(c)
                k = N - c
                th[c:] = np.asarray(theta[:k], dt)
                be[c:] = np.asarray(beta[:k], dt)
                be[c] = 0
        ym1, y = y, yp
    return th, be, restarts, decisions


def expected(oracle, z0, y0, MGneg, gP, GL, pD, N, L, tol, R, theta, beta, check_every=10, f64_problem=None):
    """The restarted solve of one instance: z, y, it, code of the oracle's table solve, the restart count and
    whether a decision before the final count was ambiguous.  f64: f64_problem = (ML, M, G, g), the unscaled
    operands Oracle.solve_f64 takes."""
    th, be, restarts, decisions = restart_tables(oracle, z0, y0, MGneg, gP, GL, pD, N, R, theta, beta)
    if f64_problem is None:
        z, y, it, code = oracle.solve_scaled_f32(z0, y0, MGneg, gP, GL, pD, N, L, tol, check_every, theta=th,
                                                 beta=be, code=True)
    else:
        ML, M, G, g = f64_problem
        z, y, it, code = oracle.solve_f64(z0, y0, ML, M, G, g, N, L, tol, check_every, theta=th, beta=be,
                                          code=True)
    live = [d for d in decisions if d[0] < it]
    return SimpleNamespace(z=z, y=y, it=it, code=code, theta=th, beta=be,
                           restarts=sum(c < it for c in restarts), restart_counts=[c for c in restarts if c < it],
                           ambiguous=any(tot > 0.0 and ratio <= AMBIGUOUS for _, ratio, tot in live),
                           min_ratio=min([r for _, r, tot in live if tot > 0.0], default=math.inf))
