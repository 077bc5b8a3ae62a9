"""examples/cluster_gcn_loader.py (ClusterData over range_partition, ClusterLoader, a GCN trained on unions of clusters) runs
end to end on the GPU."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cluster_gcn_loader_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cluster_gcn_loader.py")],
                       cwd=os.path.join(ROOT, "examples"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("partition: 32 clusters") and lines[1].startswith("trained:"), r.stdout
    assert lines[1].endswith("fell: True"), r.stdout
