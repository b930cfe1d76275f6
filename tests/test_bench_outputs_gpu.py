"""`bench.py --dump-outputs DIR`: what the last timed step returned (a seeded row sample of Q, s, energy) as float64 .npy
files, identical for two runs with the same arguments; a plain run prints the headline only (the extras are --full's)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--rows", "250000"]


def bench(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    res = subprocess.run([sys.executable, BENCH] + ARGS + ["--dump-outputs", str(out_dir)], env=env,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    (line,) = [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]
    return line, {n: np.load(os.path.join(out_dir, n + ".npy")) for n in ("Q_sample", "s", "energy")}


@pytest.mark.gpu
def test_dump_outputs_plain_run(tmp_path):
    line, out = bench(tmp_path / "a")
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["metric"] == "snapshot-DoF/s for POD build" and line["unit"] == "snapshot-DoF/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64"
    assert "cpu_baseline" not in line and "secondary" not in line and line["config"]["single_pod_latency_ms"] is None
    assert sorted(os.listdir(tmp_path / "a")) == ["Q_sample.npy", "energy.npy", "s.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    Q, s, energy = out["Q_sample"], out["s"], out["energy"]
    assert Q.dtype == s.dtype == energy.dtype == np.float64
    assert Q.shape == (65_536, 40) and s.shape == energy.shape == (512,)
    assert np.all(np.isfinite(Q)) and np.abs(Q).max() > 0
    assert s[0] > 0 and s[0] == s.max() and np.all(np.diff(s[:40]) <= 0) and abs(energy[-1] - 1.0) < 1e-12
    # the sampled rows of an orthonormal basis: Q^T Q over all rows is I, so the sample's Gram is close to m/N_h I
    G = Q.T @ Q * (250_000 / Q.shape[0])
    assert np.abs(np.diag(G) - 1.0).max() < 0.1 and np.abs(G - np.diag(np.diag(G))).max() < 0.1
    _, again = bench(tmp_path / "b")   # same arguments, same inputs: the same results up to rounding
    for name, tol in (("Q_sample", 1e-9), ("s", 1e-12), ("energy", 1e-12)):
        np.testing.assert_allclose(again[name], out[name], rtol=0, atol=tol * np.abs(out[name]).max(), err_msg=name)
