"""Infeasibility certificates without a GPU: gpad_farkas_margin (host only), the Python surface, and the
reference of the decision rule (tests/infeas_ref64.py) on the inputs of tests/infeas_cases.py.

The reference is asserted on itself: with the fixed seeds it certifies every instance whose plain solve
does not converge in N before N, and never nominates an instance that converges -- so a bad seed fails
here, loudly, rather than hiding a miss in the GPU tests that take these instances as their cases.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import gpad_mpc
import infeas_cases as cases
import infeas_ref64 as ref
from conftest import load_golden
from gpad_mpc import _lib, problems

BATCH, reference = cases.BATCH, cases.reference


def test_surface():
    assert _lib.CODE_INFEASIBLE == 5 == ref.CODE_INFEASIBLE
    assert hasattr(gpad_mpc.GpadSolver, "setup_infeasibility") and callable(gpad_mpc.farkas_margin)
    assert problems.battery_zbound() == 0.3 == cases.R
    assert problems.battery_zbound(umax=0.2, umin=-0.4, xmax=1.0) == 0.4
    lib = _lib.load()  # no handle: the binding needs one, the margin does not
    assert lib.gpad_setup_infeasibility(None, 0.3) == _lib.ERR_INVALID


@pytest.mark.parametrize("shape", list(cases.SHAPES))
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_reference_certifies_every_infeasible_instance_and_no_other(shape, dtype):
    p, b = cases.pack(shape), cases.batch(shape, BATCH, 2)
    plain, cert = reference(shape, dtype, bound=False), reference(shape, dtype)
    stuck = [r.code == 0 for r in plain]
    assert 3 <= sum(stuck) < BATCH and all(b.edge[i] for i in range(BATCH) if stuck[i])
    for i in range(BATCH):
        if stuck[i]:  # infeasible: certified before N, and the certificate holds on the problem's own data
            assert cert[i].code == 5 and cert[i].it < cases.N and cert[i].it % 40 == 0, (i, cert[i].code, cert[i].it)
            assert ref.farkas_margin(p.qp.G, b.g[i], cert[i].y, cases.R) > 0.0
        else:  # feasible: never nominated, and the same solve as without the bound
            assert cert[i].nominated == 0 and (cert[i].code, cert[i].it) == (plain[i].code, plain[i].it)
            assert np.array_equal(cert[i].z, plain[i].z) and np.array_equal(cert[i].y, plain[i].y)


@pytest.mark.parametrize("shape", list(cases.SHAPES))
def test_f32_and_f64_detect_alike(shape):
    a, c = reference(shape, np.float64), reference(shape, np.float32)
    assert [r.code for r in a] == [r.code for r in c]
    assert [r.it for r, s in zip(a, c) if r.code == 5] == [s.it for r, s in zip(a, c) if r.code == 5]


@pytest.mark.parametrize("shape", list(cases.SHAPES))
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_margin_agrees_with_numpy_on_certifying_y(shape, dtype):
    p, b = cases.pack(shape), cases.batch(shape, BATCH, 2)
    G = np.ascontiguousarray(p.qp.G, dtype)
    seen = 0
    for i, r in enumerate(reference(shape, dtype)):
        if r.code != 5:
            continue
        g, y = np.ascontiguousarray(b.g[i], dtype), np.ascontiguousarray(r.y, dtype)
        want = ref.farkas_margin(G, g, y, cases.R)
        got = gpad_mpc.farkas_margin(G, g, y, cases.R)
        assert got > 0.0 and abs(got - want) <= 1e-12 * abs(want), (i, got, want)  # (fp64 sums in another order)
        seen += 1
    assert seen >= 3


@pytest.mark.parametrize("name", ["battery_c1", "synth_small"])
def test_margin_is_not_positive_on_feasible_goldens(name):
    gd = load_golden(name)
    for dtype in (np.float64, np.float32):
        G, g = np.ascontiguousarray(gd["G"], dtype), np.ascontiguousarray(gd["g"], dtype)
        for key in ("ref_y_100", "tol_y", "ref_y_10"):
            y = np.ascontiguousarray(gd[key], dtype)
            assert (y >= 0).all()
            for R in (0.3, 1.0, 1e3):
                got = gpad_mpc.farkas_margin(G, g, y, R)
                assert got <= 0.0 and got == pytest.approx(ref.farkas_margin(G, g, y, R), rel=1e-12, abs=1e-300)


def test_margin_of_a_negative_entry_and_bad_arguments():
    gd = load_golden("synth_small")
    G, g, y = (np.ascontiguousarray(gd[k], np.float64) for k in ("G", "g", "ref_y_100"))
    y = y.copy()
    y[7] = -1e-300
    assert gpad_mpc.farkas_margin(G, g, y, 0.3) == -np.inf
    y[7] = np.nan
    assert gpad_mpc.farkas_margin(G, g, y, 0.3) == -np.inf
    lib, out = _lib.load(), C.c_double(1.0)
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    m, n = G.shape
    ok = (n, m, _lib.DTYPE_F64, vp(G), vp(g), vp(y), 0.3, C.byref(out))
    for pos, bad in ((0, 0), (1, -1), (2, 7), (3, None), (4, None), (5, None), (6, -0.5), (6, float("inf")),
                     (6, float("nan")), (7, None)):
        args = list(ok)
        args[pos] = bad
        assert lib.gpad_farkas_margin(*args) == _lib.ERR_INVALID, pos
    with pytest.raises(ValueError):
        gpad_mpc.farkas_margin(G, g[:-1], y, 0.3)
