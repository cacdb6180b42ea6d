"""gpad_set_option: the bounds of every option, on a plain handle and on a class-bound one (whose
children each get the call forwarded), and the forwarding order -- options set before
gpad_setup_classes reach the children exactly as options set after it.

The bounds are the option table's (csrc/gpad_host.h): value -2 and hi + 1 are GPAD_ERR_INVALID; lo, hi
and GPAD_OPT_DEFAULT succeed.  flat_waves takes exactly 0, 8, 16 and the default.  The fleet is input A
of tests/test_classes.py (11 packs in 3 classes, n = 12, m = 56).
"""
from __future__ import annotations

import numpy as np
import pytest

from test_classes import F32, _L, _bind_plant, inputs
from test_loop_async import assert_same_run, loop

BIG = 1 << 30
BOUNDS = {"plan": (0, 1), "lpt": (0, 1), "flat_a_lds": (0, 1), "debug_drop_handoff": (0, 1), "p64_relay": (0, 1),
          "p64_refill": (0, 1), "loop_async": (0, 1), "loop_panel": (0, 1), "phased": (0, 2), "flat_panels": (0, 4),
          "phase_len": (0, BIG), "finish_thresh": (0, BIG), "panel_max_grid": (0, BIG), "duo_max_grid": (0, BIG),
          "flat_panel_min": (0, BIG), "flat_waves": (0, 16)}


def _plain():
    import gpad_mpc
    I = inputs("A")
    q = I.C.qp
    s = gpad_mpc.GpadSolver(0)
    s.setup(F32(q.ML[0]), F32(q.G[0]), _L(q, np.float32), n=q.n, m=q.m, batch=4, shared=True)
    return s


def _classes(before=None, after=None):
    """The class binding of input A; `before` / `after`: options set before / after gpad_setup_classes."""
    import gpad_mpc
    I = inputs("A")
    q = I.C.qp
    s = gpad_mpc.GpadSolver(0)
    s.set_options(**(before or {}))
    s.setup_classes(F32(q.ML), F32(q.G), _L(q, np.float32), I.class_of, n=q.n, m=q.m)
    _bind_plant(s, I.C, F32)
    s.set_options(**(after or {}))
    return s


_handles = {}


def _handle(kind):
    if kind not in _handles:
        _handles[kind] = _plain() if kind == "plain" else _classes()
    return _handles[kind]


def test_bounds_cover_every_option():
    from gpad_mpc import _lib
    assert set(BOUNDS) == set(_lib.OPTIONS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BOUNDS))
@pytest.mark.parametrize("kind", ["plain", "classes"])
def test_bounds(gpu, kind, name):
    from gpad_mpc import _lib
    s = _handle(kind)
    lo, hi = BOUNDS[name]
    code = _lib.OPTIONS[name]
    set_ = lambda v: s.lib.gpad_set_option(s.h, code, v)  # noqa: E731
    try:
        bad = [-2, hi + 1] + ([4, 12, 17] if name == "flat_waves" else [])
        good = [lo, hi, _lib.OPT_DEFAULT] + ([8] if name == "flat_waves" else [])
        for v in bad:
            assert set_(v) == _lib.ERR_INVALID, (name, v)
        for v in good:
            assert set_(v) == _lib.GPAD_OK, (name, v)
    finally:
        assert set_(_lib.OPT_DEFAULT) == _lib.GPAD_OK  # (no solve runs in between)


@pytest.mark.gpu
@pytest.mark.parametrize("option,grid,kernel", [("loop_panel", "panel_max_grid", "loop_panel"),
                                                ("loop_async", "duo_max_grid", "loop")])
def test_forwarding_order(gpu, option, grid, kernel):
    """The option and its grid cap, set before gpad_setup_classes (forwarded to each new child from the
    parent's tuning) and after it (forwarded call by call): the same engine, and the bits of each other
    and of the options-off run."""
    I = inputs("A")
    steps, N, tol, warm = 3, 2000, 1e-4, False  # N a multiple of check_every = 10: the panel loop qualifies
    opts = {option: 1, grid: 1}
    off = loop(_classes(), I.C, I.X0, steps, N, tol, warm)
    before = loop(_classes(before=opts), I.C, I.X0, steps, N, tol, warm)
    after = loop(_classes(after=opts), I.C, I.X0, steps, N, tol, warm)
    assert off.st["kernel"] not in (None, "loop", "loop_panel")
    assert before.st["kernel"] == kernel and after.st["kernel"] == kernel
    assert_same_run(before, after)
    assert_same_run(before, off)
    assert off.it.max() < N and len(set(off.it[0].tolist())) > 1  # the tolerance stopped ragged solves
