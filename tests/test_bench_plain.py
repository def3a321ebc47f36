"""A plain `bench.py --gpus 1 --steps K --warmup W` prints the headline line and nothing it does not need; everything else the lk line
can carry (roofline, lean, single_target, cpu_baseline, parity, configs, pf_strong) is --full's."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "lean", "single_target", "cpu_baseline", "parity", "configs", "pf_strong")


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "MTFHIP_BENCH_STUB")}
    env.update(extra)
    return env


def _bench(args, env):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, cwd=ROOT, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=600)


def test_event_stride_refused_without_full():
    # the events inside the timed regions feed the roofline record alone: a plain run would pay for them and report nothing
    p = _bench(["--steps", "2", "--warmup", "1", "--event-stride", "4"], _env())
    assert p.returncode != 0 and "--event-stride" in p.stderr and "--full" in p.stderr


@pytest.mark.gpu
def test_plain_line_is_the_headline_alone():
    p = _bench(["--gpus", "1", "--steps", "20", "--warmup", "5"], _env())
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["unit"] == "iters/s" and d["higher_is_better"] is True and d["dtype"] == "f64" and d["metric"].startswith("LK iters/sec")
    assert d["steps"] == 20 and d["warmup"] == 5 and d["n_gpus"] == 1 and d["timed_regions"]["count"] == 5
    # value and ms_per_step come from the same (median) timed region: 64 targets x 20 steps in 20 x ms_per_step
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] * 1e-3 - 64) < 1e-6 * 64
    assert not set(FULL_ONLY) & set(d), sorted(set(FULL_ONLY) & set(d))
