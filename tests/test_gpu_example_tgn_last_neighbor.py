"""examples/tgn_last_neighbor.py (a memory-less attention layer trained on TemporalEventLoader's mini-batches) runs end to end
on the GPU and passes its own checks."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tgn_last_neighbor_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "tgn_last_neighbor.py")],
                       cwd=os.path.join(ROOT, "examples"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("trained:") and lines[1].startswith("lookups:"), r.stdout
    assert lines[0].endswith("fell: True") and lines[1].endswith("later: True"), r.stdout
