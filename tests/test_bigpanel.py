"""The big-panel kernel (csrc/gpad_bigpanel.hip: shared f32 matrices with n or m in (256, 1024]) at every
instantiation, tile edge and test path.  The contract is tests/test_gpu_parity.py's: every instance equals its
own CPU oracle solve bit for bit -- z, y, the iteration count and the termination code.  Inputs, the geometry
restated from the kernel's rules and the oracle runs: tests/bigpanel_cases.py.

What the table reaches (test_table_geometry_cpu asserts every line)
  the eight instantiations gpad_bigpanel_kernel<NT1, NT2> that launch_bigpanel can reach ((1, 1) is the T-wave
    panels' range);
  the last k-block at kq = 1, 2, 3 and 4 four-steps in both GEMMs -- the issue's thirteen shapes give GEMM 1
    kq1 = 1 and 4 only, so 40 x 264 (kq1 = 2) and 300 x 267 (kq1 = 3) are added;
  the k loops of big_gemm / big_gemm2 at nkb = 1, 2, 3, a longer odd count and an even one, in both GEMMs;
  the bucket edges of the tile counts: T = 16 | 17, 32 | 33, 48 | 49 and 64; T2 = 17 (one wave pairs two tiles, 15
    run one), 45 and 49 (some second pairs), 32 and 64 (all paired), 33 (a single tile in the second pair slot);
  both shapes whose LDS is exactly 163 840 B, and the first refused shape on every side of the range.

Runs, all with kernel PANEL forced (reported "panel"), batch 35 = two full panels and a ragged one of 3; 60 x 270
also at batches 1 and 16:
  fixed N = 23 from warm z0 and y0, on the default grid and on one workgroup that walks the three panels;
  Algorithm 1 on the slack-mixed inputs of bigpanel_cases (codes 0, 1 and 2 in one panel; a code-1 and a code-2
    finish at the same test of one panel, so test (B)'s zhat is stored before the verification GEMM overwrites
    Zh), cold and warm, under three schedules: one launch, a phase boundary at every test on two workgroups
    (park, compact, reload), and the defaults;
  routing: AUTO and a forced PANEL on the refused shapes, AUTO at batch 64 | 65;
  gpad_run_state and a warm closed loop on battery_plant(4, 15) (60 x 270), with loop_panel and loop_async falling
    back to the lockstep loop.

Checked on the CPU oracle (test_conditions_cpu, test_table_conditions_cpu): every case's tolerance input, cold
and warm, ends at least 3 instances with code 1 and at least 3 with code 2, at most a quarter with code 0, and
has a panel with a code-1 and a code-2 finish at the same iteration (every case, not only one per NT2); four
cases (5 x 513, 32 x 1024, 416 x 1024, 40 x 264) have code-0 finishes.  No case departs from the conditions.

Measured on an MI355X: the 75 GPU cases of this file take 8.4 s together, the CPU oracle's solves included (they
run on a pool of 16 threads); the slowest, the plant test, takes 0.84 s and the slowest solve case, Algorithm 1
at 1024 x 720, 0.65 s.  The CPU tests take 16 s, nearly all of it the oracle's 30 tolerance runs of 35 instances.
"""
from __future__ import annotations

import numpy as np
import pytest

import bigpanel_cases as C
import test_loop_async as T
from test_gpu_parity import assert_bitexact, kcode

IDS = [C.case_id(c) for c in C.TABLE]
INNER = [c for c in C.TABLE if (c.n, c.m) not in C.LDS_EDGE]
EDGE = [c for c in C.TABLE if (c.n, c.m) in C.LDS_EDGE]
SMALL = C.case_of(*C.SMALL)
# name -> options of the three schedules of an Algorithm-1 run (check_every: the case's)
SCHEDULES = {
    "one-launch": lambda K: dict(phased=0),
    "every-test": lambda K: dict(phased=1, phase_len=K, panel_max_grid=2),
    "defaults": lambda K: {},
}
PLANT = (4, 15)  # battery_plant(4, 15): n = 60, m = 270
PLANT_PACKS, PLANT_SEED, PLANT_STEPS, PLANT_N, PLANT_TOL = 35, 7, 4, 1000, 1e-4


# ------------------------------------------------------------------------------ CPU: the table
def test_table_geometry_cpu():
    """The restated geometry gives every case the T, (NT1, NT2) and kq the table states, and the table reaches
    what the module docstring lists.  Dropping an instantiation, a kq value, a k-loop path, a bucket edge or a
    limit shape from the table fails here."""
    shapes = [(c.n, c.m) for c in C.TABLE]
    assert len(set(shapes)) == len(shapes) == 15
    assert shapes[:13] == [(60, 270), (16, 272), (5, 513), (32, 1024), (416, 1024), (257, 769), (512, 512), (272, 256),
                           (513, 17), (1024, 16), (768, 48), (769, 500), (1024, 720)]  # the minimum the sweep was set
    geo = {}
    for c in C.TABLE:
        g = geo[c.n, c.m] = C.geometry(c.n, c.m)
        assert (g["T1"], g["T2"], g["nt"], g["kq1"], g["kq2"]) == (c.T1, c.T2, c.nt, c.kq1, c.kq2), C.case_id(c)
        assert C.supported(c.n, c.m) and 1 <= min(c.n, c.m) and max(c.n, c.m) <= 1024, C.case_id(c)
        assert max(c.n, c.m) > 256  # past the T-wave panels
        assert c.N % c.check_every == 0 and c.tol > 0
    # the rules themselves, at their edges
    assert [C.big_tiles(x) for x in (1, 16, 17, 256, 257, 1024, 1025)] == [1, 1, 2, 16, 17, 64, 65]
    assert [C.nt_of(t) for t in (1, 16, 17, 32, 33, 48, 49, 64)] == [1, 1, 2, 2, 4, 4, 4, 4]
    assert [C.kq(k) for k in (1, 4, 5, 8, 9, 12, 13, 16, 17, 500, 1024)] == [1, 1, 2, 2, 3, 3, 4, 4, 1, 1, 4]
    assert [C.nkb_class(k) for k in (1, 2, 3, 4, 5, 63, 64)] == ["1", "2", "3", "even", "odd", "odd", "even"]
    # every instantiation; (1, 1) cannot be reached by a supported shape
    assert sorted({g["nt"] for g in geo.values()}) == C.ALL_NT
    assert not any(C.supported(n, m) for n in (1, 100, 256) for m in (1, 100, 256))
    # kq and the k-loop paths, per GEMM
    for key in ("kq1", "kq2"):
        assert {g[key] for g in geo.values()} == {1, 2, 3, 4}, key
    for key in ("nkb1", "nkb2"):
        assert {C.nkb_class(g[key]) for g in geo.values()} == {"1", "2", "3", "even", "odd"}, key
    # a GEMM of one k-block: that block full (kq = 4) and ragged, on the GEMM 2 side; full on the GEMM 1 side
    assert {(1, 4), (1, 2)} <= {(g["nkb2"], g["kq2"]) for g in geo.values()}
    assert (1, 4) in {(g["nkb1"], g["kq1"]) for g in geo.values()}
    # GEMM 1 with few k-blocks means m <= 48 with n > 256, GEMM 2 the reverse
    assert all((g["nkb1"] <= 3) == (m <= 48) and (g["nkb2"] <= 3) == (n <= 48) for (n, m), g in geo.items())
    # bucket edges of both tile counts, and how GEMM 2's waves pair
    t1s, t2s = {g["T1"] for g in geo.values()}, {g["T2"] for g in geo.values()}
    assert {1, 17, 32, 33, 48, 49, 64} <= t1s
    assert {1, 16, 17, 32, 33, 45, 49, 64} <= t2s  # (45: the fourth slot empty, as 48 on the other side)
    assert [C.pairing(t) for t in (2, 16, 17, 32, 33, 45, 48, 49, 64)] == \
        [(0, 2), (0, 16), (1, 15), (16, 0), (16, 1), (16, 13), (16, 16), (17, 15), (32, 0)]
    # the LDS limit: two shapes on it, the refused shapes past it or past the tile range
    assert [C.lds_bytes(*s) for s in C.LDS_EDGE] == [C.LDS_LIMIT, C.LDS_LIMIT] == [163840, 163840]
    assert all(s in shapes for s in C.LDS_EDGE)
    assert max(C.lds_bytes(*s) for s in shapes if s not in C.LDS_EDGE) < C.LDS_LIMIT
    assert C.REFUSED == [(417, 1024), (1024, 721), (1024, 1024), (1025, 16), (16, 1025)]
    assert not any(C.supported(*s) for s in C.REFUSED)
    assert [C.lds_bytes(*s) - C.LDS_LIMIT for s in C.REFUSED[:3]] == [1024, 2048, 38 * 1024]
    assert C.SLOT_BYTES * C.WAVES == 6 * 1024
    # the batch: two full panels and a ragged one of 3; the slack draw uses every value
    assert C.B == 35 and set(C.slacks(C.B).tolist()) == set(C.SLACKS)
    assert (SMALL.n, SMALL.m) == (60, 270) == (T.battery(*PLANT).qp.n, T.battery(*PLANT).qp.m)


def _finishes(oracle, c, warm):
    _, _, _, (z, y, it, cd) = C.tol_oracle(oracle, c, warm)
    assert np.isfinite(z).all() and np.isfinite(y).all()
    assert set(cd.tolist()) <= {0, 1, 2} and (it[cd == 0] == c.N).all() and (it % c.check_every == 0).all()
    return it, cd


@pytest.mark.parametrize("c", C.TABLE, ids=IDS)
def test_conditions_cpu(oracle, c):
    """The tolerance input of a case, cold and warm, on the oracle alone: the conditions of the module docstring
    (the seed and the tolerance of each case were chosen here)."""
    for warm in (False, True):
        it, cd = _finishes(oracle, c, warm)
        count = [int((cd == k).sum()) for k in (0, 1, 2)]
        assert count[1] >= 3 and count[2] >= 3 and count[0] <= C.B // 4, (C.case_id(c), warm, count)
        assert C.mixed_panels(it, cd), (C.case_id(c), warm)
        assert len(set(it.tolist())) >= 2 or c.T2 <= 2, (C.case_id(c), warm)  # (m <= 17: all stop at the first test)


def test_table_conditions_cpu(oracle):
    """Over the table: a mixed panel at every NT2 (test_conditions_cpu asserts one per case), some code-0
    finishes, and the ragged third panel takes part in the mixed events somewhere."""
    nt2, capped, ragged = set(), 0, False
    for c in C.TABLE:
        for warm in (False, True):
            it, cd = _finishes(oracle, c, warm)
            mixed = C.mixed_panels(it, cd)
            if mixed:
                nt2.add(c.nt[1])
            ragged |= 2 in mixed
            capped += int((cd == 0).sum())
    assert nt2 == {1, 2, 4} and capped >= 1 and ragged


# ------------------------------------------------------------------------------ GPU
def run_gpu(prob, z0, y0, N, tol, check_every=10, kernel="panel", opts=None):
    """One solve of the batch through the C ABI: (z, y, iters, codes, stats)."""
    import gpad_mpc
    ML, M, G, g, L = prob
    (n, m), batch = ML.shape, M.shape[0]
    z, y = z0.copy(), y0.copy()
    iters, codes = np.full(batch, -1, np.int32), np.full(batch, -1, np.int32)
    with gpad_mpc.GpadSolver(0) as s:
        s.setup(ML, G, float(L), n=n, m=m, batch=batch, shared=True, kernel=kcode(kernel), check_every=check_every)
        s.set_options(**(opts or {}))
        st = s.run(z, y, M, g, N, tol, iters=iters, codes=codes)
    return z, y, iters, codes, st


def assert_batch(got, orc, what, rows=None):
    """z, y, iters and codes of every instance (or of `rows`) against the oracle's, bit for bit."""
    z, y, it, cd = got[:4]
    zo, yo, ito, cdo = orc
    sel = slice(None) if rows is None else list(rows)
    assert np.array_equal(it[sel], ito[sel]), (what, "iters", it[sel].tolist(), ito[sel].tolist())
    assert np.array_equal(cd[sel], cdo[sel]), (what, "codes", cd[sel].tolist(), cdo[sel].tolist())
    for b in (range(len(ito)) if rows is None else rows):
        assert_bitexact(z[b], zo[b], f"{what} instance {b} z")
        assert_bitexact(y[b], yo[b], f"{what} instance {b} y")


FIXED = [(c, C.B) for c in C.TABLE] + [(SMALL, b) for b in C.SMALL_BATCHES]
FIXED_IDS = ["%s-B%d" % (C.case_id(c), b) for c, b in FIXED]


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [0, 1], ids=["grid0", "grid1"])
@pytest.mark.parametrize("c,batch", FIXED, ids=FIXED_IDS)
def test_fixed_n(gpu, oracle, c, batch, grid):
    """N = 23 iterations from warm z0 and y0 (w_0 = y_0), no test: both GEMMs and both epilogues at every
    instantiation and k-loop path.  With panel_max_grid = 1 one workgroup walks the panels and reuses its LDS
    tiles."""
    prob, z0, y0, orc = C.fixed_oracle(oracle, c, batch)
    assert (orc[2] == C.N_FIXED).all() and (orc[3] == 0).all()
    got = run_gpu(prob, z0, y0, C.N_FIXED, 0.0, opts=dict(panel_max_grid=grid))
    assert got[4]["kernel"] == "panel"
    assert_batch(got, orc, "%s grid %d" % (C.case_id(c), grid))
    assert got[4]["iterations"] == C.N_FIXED and got[4]["converged"] == 0


def _algorithm1(oracle, c, warm, batch=C.B):
    prob, z0, y0, orc = C.tol_oracle(oracle, c, warm, batch)
    for name, opts in SCHEDULES.items():
        got = run_gpu(prob, z0, y0, c.N, c.tol, c.check_every, opts=opts(c.check_every))
        assert got[4]["kernel"] == "panel", name
        assert_batch(got, orc, "%s %s %s" % (C.case_id(c), "warm" if warm else "cold", name))
        assert got[4]["converged"] == int((orc[3] != 0).sum()), name
        assert got[4]["total_iterations"] == int(orc[2].sum()), name


ALG1 = [(c, C.B) for c in INNER] + [(SMALL, b) for b in C.SMALL_BATCHES]
ALG1_IDS = ["%s-B%d" % (C.case_id(c), b) for c, b in ALG1]


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("c,batch", ALG1, ids=ALG1_IDS)
def test_algorithm1(gpu, oracle, c, batch, warm):
    """Algorithm 1 on the slack-mixed input under the three schedules of SCHEDULES: stage 1 over the 16 wave
    slots, the verification GEMM with code 1 over code 2, test (B)'s zhat stored before z overwrites Zh, codes
    0, 1 and 2 in one panel, the u seed from a warm z0, and -- phased -- park, compaction and reload at every
    test."""
    _algorithm1(oracle, c, warm, batch)


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("c", EDGE, ids=[C.case_id(c) for c in EDGE])
def test_algorithm1_lds_limit(gpu, oracle, c, warm):
    """test_algorithm1 on the two shapes whose LDS is exactly the 160 KiB a workgroup can have."""
    assert C.lds_bytes(c.n, c.m) == C.LDS_LIMIT
    _algorithm1(oracle, c, warm)


@pytest.mark.gpu
@pytest.mark.parametrize("nm", C.REFUSED, ids=["%dx%d" % s for s in C.REFUSED])
def test_refused_shapes(gpu, oracle, nm):
    """The first shapes past the range: AUTO takes the stream kernel (a batch of 70 is past the panels'
    threshold of 64) and is bit-exact; a forced PANEL is refused."""
    import gpad_mpc
    from gpad_mpc import _lib
    n, m = nm
    batch, N = 70, 7
    prob = C.problem(n, m, batch, 17)
    z0, y0 = C.starts(n, m, batch, False)
    rows = (0, 35, 69)
    ML, M, G, g, L = prob
    solves = [oracle.solve_f32(z0[b], y0[b], ML, M[b], G, g[b], N, L, code=True) for b in rows]
    orc = tuple(np.zeros((batch,) + np.shape(solves[0][k]), np.asarray(solves[0][k]).dtype) for k in range(4))
    for b, r in zip(rows, solves):
        for k in range(4):
            orc[k][b] = r[k]
    got = run_gpu(prob, z0, y0, N, 0.0, kernel="auto")
    assert got[4]["kernel"] == "stream"
    assert_batch(got, orc, "%dx%d auto" % nm, rows)
    with gpad_mpc.GpadSolver(0) as s:
        s.setup(ML, G, float(L), n=n, m=m, batch=batch, shared=True, kernel=_lib.KERNEL_PANEL)
        with pytest.raises(_lib.GpadError) as ei:
            s.run(z0.copy(), y0.copy(), M, g, N, 0.0)
    assert ei.value.code == _lib.ERR_UNSUPPORTED


@pytest.mark.gpu
def test_auto_routing_at_the_batch_threshold(gpu, oracle):
    """60 x 270 under AUTO (the resident kernel cannot take m > 208): the panels from batch 65 on."""
    for batch, panel in ((64, False), (65, True)):
        prob, z0, y0, orc = C.fixed_oracle(oracle, SMALL, batch)
        got = run_gpu(prob, z0, y0, C.N_FIXED, 0.0, kernel="auto")
        assert (got[4]["kernel"] == "panel") == panel, (batch, got[4]["kernel"])
        assert got[4]["kernel"] in ("panel", "stream")
        assert_batch(got, orc, "auto batch %d" % batch)
        prob, z0, y0, orc = C.tol_oracle(oracle, SMALL, True, batch)
        got = run_gpu(prob, z0, y0, SMALL.N, SMALL.tol, SMALL.check_every, kernel="auto")
        assert (got[4]["kernel"] == "panel") == panel, (batch, got[4]["kernel"])
        assert_batch(got, orc, "auto tol batch %d" % batch)


@pytest.mark.gpu
def test_plant_on_the_big_panels(gpu, oracle):
    """gpad_run_state and a warm closed loop with a tolerance on battery_plant(4, 15), 35 packs, kernel PANEL:
    every pack equals the oracle's loop; loop_panel and loop_async do not take m > 256 / m > 208 (resp. a forced
    PANEL), so the same call reports the lockstep engine and returns the same bits."""
    from gpad_mpc import _lib
    p = T.battery(*PLANT)
    X0 = T.states(p, PLANT_PACKS, PLANT_SEED)
    # one state solve: the first step of a cold loop
    one = T.oracle_loop(oracle, "big-b4x15", p, X0, 1, PLANT_N, PLANT_TOL, False)
    s = T.make_solver(p, PLANT_PACKS, kernel=_lib.KERNEL_PANEL)
    Z, Y = np.zeros((PLANT_PACKS, p.qp.n), np.float32), np.zeros((PLANT_PACKS, p.qp.m), np.float32)
    st = s.run_state(X0.copy(), Z, Y, PLANT_N, PLANT_TOL)
    s.close()
    assert st["kernel"] == "panel"
    T.same_bits(Z, one.z, "run_state z")
    T.same_bits(Y, one.y, "run_state y")
    assert st["total_iterations"] == int(one.it.sum()) and st["converged"] == PLANT_PACKS
    # the closed loop, lockstep
    cfg = (PLANT_STEPS, PLANT_N, PLANT_TOL, True)
    orc = T.oracle_loop(oracle, "big-b4x15", p, X0, *cfg)
    assert orc.it.max() < PLANT_N and max(len(set(row)) for row in orc.it.tolist()) >= 3
    ref = T.run(p, X0, *cfg, kernel=_lib.KERNEL_PANEL)
    assert ref.st["kernel"] == "panel"
    T.assert_matches_oracle(ref, orc)
    assert ref.st["total_iterations"] == int(orc.it.sum())
    assert (ref.cd != 0).all() and (ref.cd <= 2).all()
    # the one-launch options fall back to it
    for option in ("loop_panel", "loop_async"):
        s = T.make_solver(p, PLANT_PACKS, kernel=_lib.KERNEL_PANEL)
        s.set_option(option, 1)
        r = T.loop(s, p, X0, *cfg)
        s.close()
        assert r.st["kernel"] == "panel", option
        T.assert_same_run(r, ref)
        T.assert_matches_oracle(r, orc)
