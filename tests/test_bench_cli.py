"""bench.py's plain run and its --dump-outputs: a plain run prints only the headline line, and the arrays it dumps are
the timed run's own results (K iterations of the lasso loop from x = z = u = 0), checked against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPED = ("xopt", "zopt", "uopt", "pnorm", "dnorm", "perr", "derr")


def test_bench_arguments():
    import bench

    a = bench.parse([])
    assert not a.full and a.dump_outputs is None and a.steps == 200 and a.warmup == 10
    a = bench.parse(["--steps", "7", "--warmup", "0", "--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d" and a.steps == 7 and a.warmup == 0
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_timed_results(gpu, tmp_path):
    from oracle import solvers_ref

    rows, cols, steps = 4100, 512, 6
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "2", "--rows", str(rows),
           "--cols", str(cols), "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["warmup"] == 2 and out["n_gpus"] == 1
    assert out["unit"] == "iterations/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["value"] > 0 and out["ms_per_step"] == pytest.approx(1e3 / out["value"], rel=1e-9)
    for leg in ("roofline", "cpu_baseline", "parity", "record_history1", "objevals1", "a_streaming", "other_configs"):
        assert leg not in out, leg  # --full only

    assert sorted(os.listdir(tmp_path)) == sorted(f"{k}.npy" for k in DUMPED)
    got = {k: np.load(tmp_path / f"{k}.npy") for k in DUMPED}
    assert all(v.dtype == np.float64 for v in got.values())
    p = __import__("admm_project_amd").synth.lasso_problem(seed=1, rows=rows, cols=cols)
    ref = solvers_ref.lasso(p["D"], p["s"], p["lam"], dict(maxiters=steps, domaxiters=1))
    assert ref["steps"] == steps
    for k in DUMPED:
        b = np.asarray(ref[k], dtype=np.float64).reshape(-1)
        assert got[k].shape == b.shape, (k, got[k].shape, b.shape)
        err = np.max(np.abs(got[k] - b)) / max(1.0, np.max(np.abs(b)))
        assert err < 1e-9, (k, err)
