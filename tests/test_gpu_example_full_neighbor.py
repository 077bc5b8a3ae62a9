"""examples/full_neighbor_inference.py (a model trained with NeighborLoader, layer-wise inference over all nodes with
FullNeighborLoader(num_layers=1)) runs end to end on the GPU and passes its own checks."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_full_neighbor_inference_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "full_neighbor_inference.py")],
                       cwd=os.path.join(ROOT, "examples"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("trained:") and lines[1].startswith("inference: 1000 nodes"), r.stdout
    assert lines[0].endswith("fell: True"), r.stdout
    assert lines[1].endswith("block edges per node equal the in-degree: True"), r.stdout
    assert "equals the whole-graph forward: True" in lines[1], r.stdout
