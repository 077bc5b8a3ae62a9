"""examples/subgraph_sketch_link_prediction.py (SketchData, SubgraphSketchLoader) runs end to end on the GPU."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_subgraph_sketch_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "subgraph_sketch_link_prediction.py")],
                       cwd=os.path.join(ROOT, "examples"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("subgraph sketches:"), r.stdout
    aucs = dict(re.findall(r"AUC (\w+) ([\d.]+)", r.stdout))
    assert sorted(aucs) == ["cn", "structure"] and float(aucs["structure"]) > 0.5, r.stdout
