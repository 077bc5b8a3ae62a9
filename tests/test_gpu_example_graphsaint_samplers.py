"""examples/graphsaint_samplers.py (GraphSAINTNodeLoader and GraphSAINTEdgeLoader with sample_coverage, one epoch each)
runs end to end on the GPU."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_graphsaint_samplers_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "graphsaint_samplers.py")],
                       cwd=os.path.join(ROOT, "examples"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("node sampler: 200 draws") and lines[1].startswith("edge sampler: 120 draws"), \
        r.stdout
