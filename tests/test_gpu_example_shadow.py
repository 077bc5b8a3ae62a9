"""examples/shadow_khop_loader.py (ShaDowKHopLoader, untimed and timed) runs end to end on the GPU."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shadow_khop_loader_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "shadow_khop_loader.py")],
                       cwd=os.path.join(ROOT, "examples"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("untimed:") and lines[1].startswith("timed:"), r.stdout
    assert all(line.endswith("share batch: True") for line in lines), r.stdout
    edges = [int(x) for x in re.findall(r"(\d+) induced edges", r.stdout)]
    assert len(edges) == 2 and 0 < edges[1] < edges[0], r.stdout        # times only take edges away
