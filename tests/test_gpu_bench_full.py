"""bench.py with the real engine at N = 1 (needs an MI355X): a plain run prints the headline line and measures nothing
after its timed region; --full adds the CPU baseline and the single-pair latency mode to the same line."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*extra):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "BENCH_MOCK", "BENCH_REHEARSE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "tiny", "--steps", "2",
                        "--warmup", "1", *extra], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_a_plain_run_prints_the_headline_only_and_full_adds_the_cpu_baseline_and_latency_mode():
    plain = _bench()
    full = _bench("--full")
    for d in (plain, full):
        assert all(k in d for k in HEADLINE), d
        assert d["metric"] == "Mdisparities/s" and d["higher_is_better"] is True and d["dtype"] == "int16"
        assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert "cpu_baseline" not in plain and "latency_mode" not in plain and "speedup_vs_cpu_baseline" not in plain
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["all_threads"]["value"] > 0
    assert full["speedup_vs_cpu_baseline"] > 0 and full["speedup_vs_cpu_all_threads"] > 0
    assert full["latency_mode"]["ms_per_pair"] > 0 and full["latency_mode"]["pairs_in_flight"] == 1
