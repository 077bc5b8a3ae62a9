"""tg_seal_nodes_capped on a non-default stream: the call of tests/test_gpu_seal_capped.py, word for word against the
restatement, in each form under the one extra stream of the process's stream tests (helpers_stream.side_stream; this file sorts
behind the tests that create it)."""
import pytest
import torch

import helpers_stream as hs
from test_gpu_seal_capped import fan, run  # noqa: F401  (fan: the fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("form", [1, 2])
def test_seal_nodes_capped_on_the_side_stream(fan, form):  # noqa: F811
    s = hs.side_stream()
    with torch.cuda.stream(s):
        run(fan, [(fan[3][513], fan[3][2049]), (fan[3][65], fan[4])], [64, 0, 5], key="fan", form=form)
    s.synchronize()
