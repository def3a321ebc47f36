"""`bench.py --dump-outputs DIR`: what the last timed step of the lk workload returned (batch.track: corners, n_iters) as float64 .npy
files, the same from run to run (seeded inputs), so that two builds can be compared output for output."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "MTFHIP_BENCH_STUB")}
    env.update(extra)
    return env


def _bench(args, env):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, cwd=ROOT, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=600)


def test_dump_outputs_writes_float64_and_enforces_the_limit(tmp_path, monkeypatch):
    import bench
    d = tmp_path / "out"
    bench.dump_outputs(str(d), [("n_iters", np.arange(4, dtype=np.int32)), ("corners", np.ones((4, 2, 4)))])
    n, c = np.load(d / "n_iters.npy"), np.load(d / "corners.npy")
    assert n.dtype == np.float64 and c.dtype == np.float64 and c.shape == (4, 2, 4)
    assert np.array_equal(n, np.arange(4))
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 100)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), [("x", np.zeros(13))])


def test_dump_outputs_refused_where_nothing_is_computed_on_the_device(tmp_path):
    p = _bench(["--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "d")], _env(MTFHIP_BENCH_STUB="1"))
    assert p.returncode != 0 and "--dump-outputs" in p.stderr
    p = _bench(["--workload", "grid", "--dump-outputs", str(tmp_path / "d")], _env())
    assert p.returncode != 0 and "--dump-outputs" in p.stderr
    assert not (tmp_path / "d").exists()


@pytest.mark.gpu
def test_bench_dump_outputs_repeatable(tmp_path):
    import bench
    outs = []
    for run, steps in enumerate((3, 3, 5)):
        d = tmp_path / ("run%d" % run)
        p = _bench(["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--repeats", "2", "--no-cpu", "--no-lean", "--configs", "0",
                    "--dump-outputs", str(d)], _env())
        assert p.returncode == 0, p.stderr[-2000:]
        outs.append({name: np.load(d / (name + ".npy")) for name in ("n_iters", "corners")})
    n, c = outs[0]["n_iters"], outs[0]["corners"]
    assert n.dtype == np.float64 and c.dtype == np.float64
    assert n.shape == (64,) and np.all(n == 3)          # --steps iterations of every target
    assert c.shape == (64, 2, 4) and np.all(np.isfinite(c))
    for name in outs[0]:
        assert np.array_equal(outs[0][name], outs[1][name]), name
    # the timed steps' result: not the seeded initial region, and not a warm-up's (--warmup is the same in every run, --steps is not)
    _, _, init = bench.lk_inputs(200, 64)
    assert np.all(np.abs(c - init).max(axis=(1, 2)) > 0)
    assert np.all(outs[2]["n_iters"] == 5)
    assert np.all(np.abs(outs[2]["corners"] - c).max(axis=(1, 2)) > 0)
