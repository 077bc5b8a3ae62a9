"""tg_ppr_topk on a non-default stream: the call of tests/test_gpu_ppr.py, word for word against the restatement, under the
one extra stream of the process's stream tests (helpers_stream.side_stream; this file sorts behind the tests that create it,
so the streams a test process creates, and with them their hardware queues, stay what they were)."""
import pytest
import torch

import helpers_stream as hs
from test_gpu_ppr import POOL, graphs, run  # noqa: F401  (graphs: the fixture)

pytestmark = pytest.mark.gpu


def test_ppr_topk_on_the_side_stream(graphs):  # noqa: F811
    s = hs.side_stream()
    with torch.cuda.stream(s):
        run(graphs["csr"], POOL, k=65)
    s.synchronize()
