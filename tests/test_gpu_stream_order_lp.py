"""tg_lp_propose and tg_lp_commit on a non-default stream: the calls of tests/test_gpu_lp.py, word for word against the
restatement, under the one extra stream of the process's stream tests (helpers_stream.side_stream; this file sorts behind the
tests that create it, so the streams a test process creates, and with them their hardware queues, stay what they were)."""
import pytest
import torch

import helpers_stream as hs
from test_gpu_lp import FORMS, graphs  # noqa: F401  (graphs: the fixture)
from test_gpu_lp import test_commit_equals_the_restatement as commit_case, test_propose_equals_the_restatement as propose_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("form", FORMS)
def test_propose_on_the_side_stream(graphs, form):  # noqa: F811
    s = hs.side_stream()
    with torch.cuda.stream(s):
        propose_case(graphs, form, 3000)
    s.synchronize()


@pytest.mark.parametrize("name", ["movers_257", "free_4_wanted_5", "bad_target"])
def test_commit_on_the_side_stream(name):
    s = hs.side_stream()
    with torch.cuda.stream(s):
        commit_case(name)
    s.synchronize()
