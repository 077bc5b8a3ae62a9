"""examples/common_neighbor_heuristics.py (CommonNeighborLoader) runs end to end on the GPU."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_common_neighbor_heuristics_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "common_neighbor_heuristics.py")],
                       cwd=os.path.join(ROOT, "examples"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("common neighbours:"), r.stdout
    aucs = dict(re.findall(r"AUC (\w+) ([\d.]+)", r.stdout))
    assert sorted(aucs) == ["aa", "cn", "jaccard", "ra"] and all(float(a) > 0.5 for a in aucs.values()), r.stdout
