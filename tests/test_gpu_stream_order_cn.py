"""tg_cn_links on a non-default stream: the call of tests/test_gpu_cn.py, word for word against the restatement, in each form
under the one extra stream of the process's stream tests (helpers_stream.side_stream; this file sorts behind the tests that
create it, so the streams a test process creates, and with them their hardware queues, stay what they were)."""
import pytest
import torch

import helpers_stream as hs
from test_gpu_cn import FORMS, LINKS, graphs, run  # noqa: F401  (graphs: the fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("form", FORMS, ids=str)
def test_cn_links_on_the_side_stream(graphs, form):  # noqa: F811
    s = hs.side_stream()
    with torch.cuda.stream(s):
        run(graphs, LINKS, **form)
    s.synchronize()
