"""examples/pinsage_loader.py (PinSAGELoader, a weighted mean aggregation over the blocks with edge_weight) runs end to end
on the GPU."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pinsage_loader_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "pinsage_loader.py")],
                       cwd=os.path.join(ROOT, "examples"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("pinsage: 4 mini-batches of 512 seeds"), r.stdout
    nodes = float(re.search(r"(\S+) distinct nodes", r.stdout).group(1))
    edges = float(re.search(r"(\S+) weighted edges", r.stdout).group(1))
    heaviest = int(re.search(r"heaviest edge (\d+) visits", r.stdout).group(1))
    assert 512 < nodes <= 512 * 36 and 0 < edges <= 512 * 5 + 512 * 6 * 5 and 1 <= heaviest <= 20, r.stdout
