"""examples/shadow_ppr_loader.py (PPRLoader) runs end to end on the GPU."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shadow_ppr_loader_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "shadow_ppr_loader.py")],
                       cwd=os.path.join(ROOT, "examples"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("ppr:") and lines[0].endswith("share batch: True"), r.stdout
    nodes, edges = int(re.search(r"(\d+) nodes, \d+ induced", r.stdout).group(1)), int(re.search(r"(\d+) induced", r.stdout).group(1))
    assert nodes > 0 and edges > 0, r.stdout
