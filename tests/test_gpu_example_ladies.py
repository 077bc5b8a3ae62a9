"""examples/ladies_loader.py (a two-layer model trained on LADIESLoader's blocks) runs end to end on the GPU and passes its
own checks."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ladies_loader_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ladies_loader.py")],
                       cwd=os.path.join(ROOT, "examples"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("trained:") and lines[1].startswith("blocks:"), r.stdout
    assert lines[0].endswith("fell: True"), r.stdout
    assert "bounded by the budgets: True" in lines[1] and lines[1].endswith("e_id names the edges: True"), r.stdout
