"""-m gpu: `bench.py --dump-outputs DIR` writes the discharge of the headline call after its LAST timed step (pixel order):
the same file from two runs of the same command, and the C oracle's discharge after exactly --warmup + --steps calls on the
same synthetic inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(out, size, steps, warmup):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", str(size), "--steps",
                        str(steps), "--warmup", str(warmup), "--no-extra", "--no-cpu-baseline", "--dump-outputs", out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert sorted(os.listdir(out)) == ["discharge.npy"]
    return line, np.load(os.path.join(out, "discharge.npy"))


def test_dump_is_the_discharge_after_the_last_timed_step(oracle, tmp_path):
    from lisflood_amd import synthetic as syn
    size, steps, warmup = 160, 5, 2
    line, q = run_bench(str(tmp_path / "a"), size, steps, warmup)
    assert line["steps"] == steps and line["warmup"] == warmup and line["finite"]
    N = size * size
    assert q.dtype == np.float64 and q.shape == (N,)
    _, again = run_bench(str(tmp_path / "b"), size, steps, warmup)
    assert np.array_equal(q, again)
    # bench.py's calls: warm-up and timed steps both take lateral_inflow(N, s % 3) for s = 0, 1, ...
    codes = syn.make_ldd("shallow", size, size, 1)
    mask = np.ones((size, size), bool)
    p = syn.router_params(N)
    kw = oracle.kinematicWave(codes[mask].astype(np.float64), mask, p["alpha"], p["beta"], p["dx"], p["dt"])
    Q = p["Q0"].copy()
    for s in list(range(warmup)) + list(range(steps)):
        before = Q.copy()
        kw.kinematicWaveRouting(Q, syn.lateral_inflow(N, s % 3))
    np.testing.assert_allclose(q, Q, rtol=1e-9, atol=1e-12)
    assert not np.allclose(q, before, rtol=1e-9, atol=1e-12)        # one call fewer is a different discharge
