"""bench.py end to end on a small custom window set (needs an MI355X): a plain run prints the headline line and does
nothing else; --full adds the legs that measure or check anything else, parity against the oracle among them."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config"}
SMALL = ["--gpus", "1", "--bl", "2", "--time", "128", "--chan", "512", "--steps", "1", "--warmup", "1"]


def _run(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["TRI_BENCH_CPU_THREADS"] = "4"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + args, env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_prints_only_the_headline(gpu):
    res = _run([])
    assert set(res) == HEADLINE
    assert res["value"] > 0 and res["steps"] == 1 and res["warmup"] == 1 and res["n_gpus"] == 1


@pytest.mark.gpu
def test_full_run_adds_the_other_legs(gpu):
    res = _run(["--full", "--no-roofline"])
    assert HEADLINE <= set(res)
    assert set(res["other_params"]) == {"defaults", "very_broad", "broad", "narrow"}
    assert res["cpu_baseline"]["cores"] == 4
    assert res["parity_check"]["mismatches"] == 0 and res["parity_ok"] is True
