"""tg_seal_nodes on a non-default stream: the call of tests/test_gpu_seal.py, word for word against the restatement, in each
form under the one extra stream of the process's stream tests (helpers_stream.side_stream; this file sorts behind the tests
that create it, so the streams a test process creates, and with them their hardware queues, stay what they were)."""
import pytest
import torch

import helpers_stream as hs
from test_gpu_seal import LINKS, graphs, run  # noqa: F401  (graphs: the fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("form", [1, 2])
def test_seal_nodes_on_the_side_stream(graphs, form):  # noqa: F811
    s = hs.side_stream()
    with torch.cuda.stream(s):
        run(graphs["csr"], LINKS, num_hops=3, form=form)
    s.synchronize()
