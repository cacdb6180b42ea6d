"""bench.py's run modes: a plain run stops at the headline, ``--full`` adds the legs, and
``--dump-outputs DIR`` writes what the last timed step returned."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)


def test_dump_outputs_small_arrays_whole(tmp_path):
    import bench
    z = np.arange(12, dtype=np.float32).reshape(4, 3)
    it = np.array([10, 20, 30, 40], np.int32)
    bench.dump_outputs(str(tmp_path / "d"), {"z": z, "iterations": it})
    assert sorted(os.listdir(tmp_path / "d")) == ["iterations.npy", "z.npy"]
    zr, ir = np.load(tmp_path / "d" / "z.npy"), np.load(tmp_path / "d" / "iterations.npy")
    assert zr.dtype == np.float32 and np.array_equal(zr, z)
    assert ir.dtype == np.float64 and np.array_equal(ir, it)


def test_dump_outputs_samples_past_the_cap(tmp_path, monkeypatch):
    """Past the cap the same seeded rows of every array are written, and the files fit the cap."""
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 40000)
    rng = np.random.default_rng(5)
    z = rng.normal(size=(1000, 7)).astype(np.float32)
    y = rng.normal(size=(1000, 5))
    rows = []
    for d in ("a", "b"):
        p = tmp_path / d
        bench.dump_outputs(str(p), {"z": z, "y": y})
        assert sum(os.path.getsize(p / f) for f in os.listdir(p)) <= 40000
        idx = np.load(p / "sample_rows.npy").astype(np.int64)
        assert 400 < idx.size < 1000 and np.all(np.diff(idx) > 0)
        assert np.array_equal(np.load(p / "z.npy"), z[idx]) and np.array_equal(np.load(p / "y.npy"), y[idx])
        rows.append(idx)
    assert np.array_equal(rows[0], rows[1])


def test_bench_help_names_the_modes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=60, cwd=ROOT)
    assert r.returncode == 0
    assert "--full" in r.stdout and "--dump-outputs DIR" in r.stdout


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(gpu, oracle, tmp_path):
    """A plain run: the headline keys, none of --full's legs, and the dumped z*, y*, counts of the
    last timed step (fresh draw number warmup + steps - 1) bit-exact vs the oracle."""
    import bench
    n, m, B, W, K = 200, 200, 256, 1, 2
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup",
                        str(W), "--batch", str(B), "--dump-outputs", str(out)], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["steps"] == K and d["full"] is False and d["n_gpus"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["unit"] == "GPAD iterations/s" and d["converged"] == B
    assert d["legs"] == {} and d["cpu_baseline"] is None and d["single_instance"] is None
    assert d["value_repeated_inputs"] is None
    z, y, it = (np.load(out / f"{k}.npy") for k in ("z", "y", "iterations"))
    assert z.dtype == np.float32 and z.shape == (B, n) and y.dtype == np.float32 and y.shape == (B, m)
    assert it.dtype == np.float64 and it.shape == (B,)
    ML, G, L, _, _ = bench.make_shard(n, m, 1, 0)
    M, g = bench.make_stream(n, m, B, W + K, 0)[-1]
    ML32, G32, L32 = ML.astype(np.float32), G.astype(np.float32), np.float32(L)
    MGneg, GL, _ = oracle.scale(ML32, G32, g[0].astype(np.float32), L32)
    PD = oracle.scale_vec(g.astype(np.float32), L32)
    Z, Y, iters, _ = oracle.solve_batch_f32(np.zeros((B, n)), np.zeros((B, m)), MGneg, M.astype(np.float32), GL, PD,
                                            5000, L32, 1e-4, threads=min(16, os.cpu_count() or 1))
    np.testing.assert_array_equal(it, iters)
    np.testing.assert_array_equal(z, Z)
    np.testing.assert_array_equal(y, Y)
