"""fp64 reference of the closed loop and its bindings.  TEST INFRASTRUCTURE ONLY.

Plain Python restatement of the documented arithmetic (INTEGRATION.md "Exogenous signals", the header
of csrc/gpad_plant.hip), independent of the library's plant kernels, staging and bindings:

    affine row:  acc = c0[i] (0 when absent); fma(P[i][k], x[k], acc) for k ascending; then the S s terms
    plant row:   acc = 0; the A x terms, the E s terms, the B u terms in one fma chain; u = z*[0:nu]
    loop:        step t forms M, g from (x_t, S[t]), solves (cold: from z = y = 0; warm: from the previous
                 step's z*, y*), records xs[t] = x_t, us[t] = u and advances x with S[t]

A None signal map is a map of zeros.  fma comes from libm through ctypes (Python 3.10 has no math.fma);
the shapes are tiny, so scalar loops do.  The inner solve is the CPU oracle's fp64 Algorithm 1
(pyoracle.solve_f64, or solve_value_f64 with a Hessian), which tests/test_value.py and tests/test_oracle.py
pin to the restatement of acceldualgrad.m.

A `Pack` is one pack's own (ML, G, L, PM, Pg, M0, g0, A, B, SM, Sg, E): per-pack bindings and class
bindings are lists of packs (class class_of[b]'s copy for pack b); for shared = 0, L is the one L given to
gpad_setup.  The keyword-only arguments of closed_loop build the perturbed / dot-product runs of the
robustness check and the deliberately wrong variants of the guards; no library code is involved.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

_libm = ctypes.CDLL("libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_double]
fma = _libm.fma

Pack = namedtuple("Pack", "ML G L PM Pg M0 g0 A B SM Sg E", defaults=(None,) * 8)

_orc = None


def _oracle(oracle=None):
    global _orc
    if oracle is not None:
        return oracle
    if _orc is None:
        import pyoracle
        _orc = pyoracle.Oracle()
    return _orc


def make_pack(ML, G, L, PM, Pg, M0=None, g0=None, A=None, B=None, SM=None, Sg=None, E=None):
    c = lambda a: None if a is None else np.ascontiguousarray(a, np.float64)  # noqa: E731
    return Pack(c(ML), c(G), float(L), c(PM), c(Pg), c(M0), c(g0), c(A), c(B), c(SM), c(Sg), c(E))


def _chain(acc, row, v, dot):
    if dot:  # the robustness check's third run: numpy's own summation order
        return acc + float(np.dot(row, v)) if len(v) else acc
    for k in range(len(v)):
        acc = fma(float(row[k]), float(v[k]), acc)
    return acc


def affine(P, c0, x, S=None, s=None, dot=False):
    """out[i] = c0[i] + P[i] . x + S[i] . s in the documented order (s given, S None: zero terms)."""
    out = np.empty(P.shape[0])
    for i in range(P.shape[0]):
        acc = 0.0 if c0 is None else float(c0[i])
        acc = _chain(acc, P[i], x, dot)
        if s is not None:
            acc = _chain(acc, S[i] if S is not None else np.zeros(len(s)), s, dot)
        out[i] = acc
    return out


def plant_step(A, B, x, u, E=None, s=None, dot=False):
    out = np.empty(A.shape[0])
    for i in range(A.shape[0]):
        acc = _chain(0.0, A[i], x, dot)
        if s is not None:
            acc = _chain(acc, E[i] if E is not None else np.zeros(len(s)), s, dot)
        out[i] = _chain(acc, B[i], u, dot)
    return out


def solve(pk, M, g, z0, y0, N, tol, H=None, check_every=10, oracle=None):
    """One inner solve: (z*, y*, iterations, termination code)."""
    o = _oracle(oracle)
    if H is None:
        return o.solve_f64(z0, y0, pk.ML, M, pk.G, g, N, pk.L, tol, check_every, code=True)
    return o.solve_value_f64(z0, y0, pk.ML, M, pk.G, g, H, N, pk.L, tol, check_every)


def run_state(pk, x, s, z0, y0, N, tol, H=None, *, check_every=10, oracle=None):
    """gpad_run_state / gpad_run_state_signals for one pack: (z*, y*, iterations, code, M, g)."""
    x = np.asarray(x, np.float64)
    s = None if s is None else np.asarray(s, np.float64)
    M = affine(pk.PM, pk.M0, x, pk.SM, s)
    g = affine(pk.Pg, pk.g0, x, pk.Sg, s)
    z, y, it, code = solve(pk, M, g, z0, y0, N, tol, H, check_every, oracle)
    return z, y, it, code, M, g


def closed_loop(pk, x0, S, steps, N, tol, warm, H=None, *, check_every=10, oracle=None, dot=False, perturb=None,
                eps=1e-9, u_offset=0):
    """gpad_closed_loop / gpad_closed_loop_signals for one pack: x, z, y, xs, us, iters, codes.
    S: [steps][ns] or None.  dot / perturb (a numpy Generator: every step's state times
    1 + eps U(-1, 1)) / u_offset (u = z[u_offset : u_offset + nu], a wrong variant) serve the CPU checks."""
    n, m = pk.ML.shape
    nx, nu = pk.A.shape[0], pk.B.shape[1]
    x = np.array(x0, np.float64).reshape(nx)
    z, y = np.zeros(n), np.zeros(m)
    xs, us = np.zeros((steps, nx)), np.zeros((steps, nu))
    iters, codes = np.zeros(steps, np.int32), np.zeros(steps, np.int32)
    for t in range(steps):
        if perturb is not None:
            x = x * (1.0 + eps * perturb.uniform(-1.0, 1.0, nx))
        s = None if S is None else np.asarray(S[t], np.float64)
        M = affine(pk.PM, pk.M0, x, pk.SM, s, dot)
        g = affine(pk.Pg, pk.g0, x, pk.Sg, s, dot)
        if not warm:
            z, y = np.zeros(n), np.zeros(m)
        z, y, iters[t], codes[t] = solve(pk, M, g, z, y, N, tol, H, check_every, oracle)
        xs[t] = x
        us[t] = z[u_offset:u_offset + nu]
        x = plant_step(pk.A, pk.B, x, us[t], pk.E, s, dot)
    return x, z, y, xs, us, iters, codes


def fleet_loop(packs, X0, S, steps, N, tol, warm, H=None, **kw):
    """closed_loop of every pack (packs[b], X0[b], S[:, b]) stacked as the library lays a batch out:
    x, z, y [batch][.], xs, us [steps][batch][.], it, cd [steps][batch]."""
    rows = [closed_loop(pk, X0[b], None if S is None else S[:, b], steps, N, tol, warm, H, **kw)
            for b, pk in enumerate(packs)]
    return SimpleNamespace(x=np.stack([r[0] for r in rows]), z=np.stack([r[1] for r in rows]),
                           y=np.stack([r[2] for r in rows]), xs=np.stack([r[3] for r in rows], axis=1),
                           us=np.stack([r[4] for r in rows], axis=1), it=np.stack([r[5] for r in rows], axis=1),
                           cd=np.stack([r[6] for r in rows], axis=1))
