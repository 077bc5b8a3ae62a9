"""tg_sketch_init, tg_sketch_propagate in each form and tg_sketch_links on a non-default stream: the calls of
tests/test_gpu_sketch.py, word for word against the restatement, under the one extra stream of the process's stream tests
(helpers_stream.side_stream; this file sorts behind the tests that create it, so the streams a test process creates, and with
them their hardware queues, stay what they were)."""
import pytest
import torch

import helpers_stream as hs
from test_gpu_sketch import FORMS, graphs, hop, test_init_and_three_chained_hops_give_equal_bytes_in_every_form as chained  # noqa: F401
from test_gpu_sketch import test_links as links

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("form", FORMS, ids=str)
def test_a_hop_on_the_side_stream(graphs, form):  # noqa: F811
    s = hs.side_stream()
    with torch.cuda.stream(s):
        hop(graphs, "csc", 128, 8, **form)
    s.synchronize()


def test_init_and_links_on_the_side_stream(graphs):  # noqa: F811
    s = hs.side_stream()
    with torch.cuda.stream(s):
        chained(graphs, 128, 8)
        links(graphs, 2, 128, 8)
    s.synchronize()
