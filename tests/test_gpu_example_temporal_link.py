"""examples/temporal_link_prediction.py (LinkNeighborLoader with time_attr / edge_label_time, unique=True: disjoint
subgraphs per pair, both strategies) runs end to end on the GPU."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_temporal_link_prediction_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "temporal_link_prediction.py")],
                       cwd=os.path.join(ROOT, "examples"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("uniform:") and lines[1].startswith("last:"), r.stdout
    ages = [float(x) for x in re.findall(r"mean age (\S+)", r.stdout)]
    edges = [int(x) for x in re.findall(r"(\d+) edges", r.stdout)]
    pairs = [int(x) for x in re.findall(r"(\d+) pairs", r.stdout)]
    assert len(ages) == 2 and all(e > 0 for e in edges) and pairs == [4000, 4000], r.stdout
    assert ages[1] < ages[0], r.stdout                      # the most recent edges are younger than a uniform draw's
