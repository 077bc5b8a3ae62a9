"""examples/hetero_link_prediction.py (a dot-product link decoder trained over HeteroLinkNeighborLoader) runs end to end on
the GPU."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hetero_link_prediction_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "hetero_link_prediction.py")],
                       cwd=os.path.join(ROOT, "examples"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    losses = [float(x) for x in re.findall(r"loss (\S+)", r.stdout)]
    assert len(losses) == 2 and all(math.isfinite(x) and x > 0 for x in losses), r.stdout
