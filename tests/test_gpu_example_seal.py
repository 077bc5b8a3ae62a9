"""examples/seal_link_prediction.py (SEALLoader) runs end to end on the GPU."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seal_link_prediction_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "seal_link_prediction.py")],
                       cwd=os.path.join(ROOT, "examples"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("seal:"), r.stdout
    links, masked = int(re.search(r"(\d+) links", r.stdout).group(1)), int(re.search(r"(\d+) target edges masked", r.stdout).group(1))
    hist = [int(w) for w in re.search(r"z histogram \[([\d, ]+)\]", r.stdout).group(1).split(",")]
    nodes = int(re.search(r"(\d+) nodes", r.stdout).group(1))
    # every positive link is an edge both ways; z = 1 is the two roots of every link and nobody else
    assert masked >= links // 2 - 16 and len(hist) == 9 and hist[1] == 2 * links and sum(hist) == nodes, r.stdout
