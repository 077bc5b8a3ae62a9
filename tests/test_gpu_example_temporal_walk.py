"""examples/temporal_walk_loader.py (skip-gram training over TemporalWalkLoader, windows masked by time) runs end to end on
the GPU."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_temporal_walk_loader_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "temporal_walk_loader.py")],
                       cwd=os.path.join(ROOT, "examples"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    losses = [float(x) for x in re.findall(r"loss (\S+)", r.stdout)]
    assert len(losses) == 2 and all(math.isfinite(x) and x > 0 for x in losses), r.stdout
    kept = [float(x) for x in re.findall(r"(\d+)% of the windows", r.stdout)]
    assert len(kept) == 2 and all(0 < k < 100 for k in kept), r.stdout       # the time mask keeps some windows, not all
