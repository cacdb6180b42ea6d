"""Plain-numpy reference of the infeasibility certificate.  TEST INFRASTRUCTURE ONLY.

The decision rule of include/gpad.h (gpad_setup_infeasibility) restated around a plain-numpy GPAD with
Algorithm 1's tests (A) and (B): no library code; only the theta / beta tables come from the CPU oracle.
``dtype`` float64 is the reference of the f64 engine; float32 emulates the f32 arithmetic (numpy's
matrix products sum in their own order, so f32 iterates are close to the engine's, not equal).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

MU = {np.float32: 2.0 ** -20, np.float64: 2.0 ** -49}  # 16 units of 2^-24 / 2^-53
CODE_INFEASIBLE = 5
_sched = {}


def schedule(N):
    if N not in _sched:
        import pyoracle
        _sched[N] = pyoracle.Oracle().schedule(N)
    return _sched[N]


def farkas_margin(G, g, y, R):
    """-(g'y) - R |G'y|_1 in fp64 on the given arrays; -inf when y has a negative entry."""
    G, g, y = (np.asarray(a).astype(np.float64) for a in (G, g, y))
    return -np.inf if not (y >= 0).all() else float(-(g @ y) - R * np.abs(G.T @ y).sum())


def decide(GL, pD, y, R, mu):
    """(nominated, infeasible) at a certificate event, fp64, ascending sums."""
    GL, pD, y = GL.astype(np.float64), pD.astype(np.float64), y.astype(np.float64)
    q = 0.0
    for i in range(len(y)):
        q += y[i] * pD[i]
    if not q > 0.0:
        return False, False
    t = np.zeros(GL.shape[1])
    for i in range(len(y)):
        t += y[i] * GL[i]
    a = p = s = 0.0
    for tj in t:
        a += abs(tj)
    for i in range(len(y)):
        p += abs(y[i] * pD[i])
        s += y[i] * np.abs(GL[i]).sum()
    return True, bool(q - R * a > mu * (p + R * s))


def solve(ML, M, G, g, L, N, tol, R=0.0, dtype=np.float64, K=10, z0=None, y0=None):
    """-> z, y, it, code (0: ran to N, 1: (A), 2: (B), 5: certificate), nominated (events with q > 0)."""
    T, mu, L = dtype, MU[dtype], float(L)
    th, be = (a.astype(T) for a in schedule(N))
    MG, GL = -np.asarray(ML, T), (np.asarray(G, T).astype(np.float64) / L).astype(T)
    pD, M = (np.asarray(g, T).astype(np.float64) * (-1.0 / L)).astype(T), np.asarray(M, T)
    z = np.zeros(MG.shape[0], T) if z0 is None else np.array(z0, T)
    y = np.zeros(MG.shape[1], T) if y0 is None else np.array(y0, T)
    ym1, u, nominated = y.copy(), GL @ z, 0
    out = lambda zz, it, code: SimpleNamespace(z=zz, y=y, it=it, code=code, nominated=nominated)  # noqa: E731
    for v in range(N):
        w = y + be[v] * (y - ym1)
        zh = MG @ w - M
        z = (T(1) - th[v]) * z + th[v] * zh
        c = GL @ zh
        ym1, y = y, np.maximum((w + pD) + c, T(0))
        u = (T(1) - th[v]) * u + th[v] * c
        it = v + 1
        if not tol > 0.0 or it % K:
            continue
        if float((u + pD).max()) * L <= tol:  # (A) nominated by the recursion, decided on G_L z
            u = GL @ z
            if float((u + pD).max()) * L + mu * float((abs(u) + abs(pD)).max()) * L <= tol:
                return out(z, it, 1)
        t = c + pD
        gap = -float(w.astype(np.float64) @ t.astype(np.float64))
        if float(t.max()) * L + mu * float((abs(c) + abs(pD)).max()) * L <= tol and w.min() >= 0 and gap * L <= tol:
            return out(zh, it, 2)
        if R > 0.0 and it % (4 * K) == 0:
            nom, infeasible = decide(GL, pD, y, R, mu)
            nominated += nom
            if infeasible:
                return out(z, it, CODE_INFEASIBLE)
    return out(z, N, 0)
