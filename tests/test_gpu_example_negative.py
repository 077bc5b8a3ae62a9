"""examples/negative_sampling.py (the reference's example on this backend, transform and loader) runs end to end on the GPU."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_negative_sampling_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "negative_sampling.py")],
                       cwd=os.path.join(ROOT, "examples"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) >= 3
    assert "loader mini-batch 0 == transform at its call id: True" in lines
