"""examples/metapath2vec_loader.py (MetaPath2Vec's skip-gram training over MetaPath2VecLoader) runs end to end on the GPU
and learns: the mean loss of an epoch falls from the first epoch to the last."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_metapath2vec_loader_example_runs_and_its_loss_decreases():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "metapath2vec_loader.py")],
                       cwd=os.path.join(ROOT, "examples"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    losses = [float(x) for x in re.findall(r"loss (\S+)", r.stdout)]
    assert len(losses) == 3 and all(math.isfinite(x) and x > 0 for x in losses), r.stdout
    assert losses[-1] < losses[0], r.stdout
