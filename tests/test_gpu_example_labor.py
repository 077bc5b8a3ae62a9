"""examples/labor_loader.py (NeighborLoader with labor=True, with and without layer_dependency) runs end to end on the GPU."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_labor_loader_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "labor_loader.py")],
                       cwd=os.path.join(ROOT, "examples"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 3 and lines[0].startswith("uniform:") and lines[1].startswith("labor:"), r.stdout
    nodes = [float(x) for x in re.findall(r"(\S+) distinct nodes", r.stdout)]
    edges = [float(x) for x in re.findall(r"(\S+) edges per", r.stdout)]
    assert len(nodes) == 3 and nodes[1] < nodes[0] and nodes[2] < nodes[0], r.stdout   # the number the option exists for
    assert min(edges) > 0 and max(edges) < 1.01 * min(edges), r.stdout   # the forest keeps its size: min(degree, k) per slot
