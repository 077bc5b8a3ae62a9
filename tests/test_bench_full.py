"""`bench.py` plain and with `--full`: a plain run does only what the headline needs (set-up, warm-up, timed steps, the
line); the check of the last timed step, two launches in flight, the secondary configurations and the CPU baseline run
with `--full` only."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_full_is_off_by_default():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.parse_args([]).full is False
    assert bench.parse_args(["--full"]).full is True


def run_bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--scale", "12",
                        "--batches-per-step", "64", *extra], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_leaves_the_rest_to_full():
    plain = run_bench()
    assert plain["config"]["full"] is False and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert "secondary" not in plain and "cpu_baseline" not in plain
    assert "verified_batches" not in plain["config"] and plain["config"]["two_launches_in_flight"] is None
    assert plain["config"]["placements_tried_ms_per_launch"]      # the placement / pipeline pick is set-up: it stays

    full = run_bench("--full", "--no-secondary", "--cpu-seconds", "1")
    assert full["config"]["full"] is True
    assert [v["batch"] for v in full["config"]["verified_batches"]] == [0, 32, 63]
    assert all(v["equals"] == ["fused kernel", "oracle philox-mode"] for v in full["config"]["verified_batches"])
    # two launches in flight need the second placement, which the set-up allocates only while HBM has room for it
    two_placements = len(full["config"]["placements_tried_ms_per_launch"]) > 3
    assert (full["config"]["two_launches_in_flight"] is not None) == two_placements
    assert full["cpu_baseline"]["value"] > 0 and "secondary" not in full
