"""The loaders' epoch plan (tch_geometric.loader._epoch_plan) against a brute-force restatement: which inputs each launch
samples, in how many mini-batches of which width.  No GPU: the plan is plain arithmetic on the host."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan():
    pkg = os.path.join(ROOT, "tch-geometric_amd")
    if not os.path.exists(os.path.join(pkg, "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", pkg, "-s"])
    subprocess.check_call([sys.executable, os.path.join(pkg, "host", "build_host.py")])   # a no-op when up to date
    from tch_geometric.loader import _epoch_plan
    return _epoch_plan


def _mini_batches(n, B, drop_last):
    """The epoch by walking the inputs one by one: [start, end) of every mini-batch."""
    out, cur = [], []
    for i in range(n):
        cur.append(i)
        if len(cur) == B:
            out.append((cur[0], cur[-1] + 1))
            cur = []
    if cur and not drop_last:
        out.append((cur[0], cur[-1] + 1))
    return out


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("prefetch", [1, 3, 16, 1000])
@pytest.mark.parametrize("batch_size", [1, 7, 32, 64, 250])
def test_plan_tiles_the_epoch(plan, batch_size, prefetch, drop_last):
    B = batch_size
    for n in range(201):
        launches = plan(n, B, prefetch, drop_last)
        want = _mini_batches(n, B, drop_last)
        got, at = [], 0
        for i, (start, n_batches, width) in enumerate(launches):
            assert start == at and n_batches >= 1 and width >= 1, (n, launches)        # in order, no gap, no overlap
            assert n_batches <= prefetch
            if width != B:                              # only the last launch may be narrower: one ragged mini-batch
                assert i == len(launches) - 1 and n_batches == 1 and width < B and not drop_last, (n, launches)
            elif i + 1 < len(launches) and launches[i + 1][2] == B:
                assert n_batches == prefetch, (n, launches)                            # full launches are full
            assert start % B == 0                                                       # start // B is its first mini-batch
            got += [(start + j * width, start + (j + 1) * width) for j in range(n_batches)]
            at = start + n_batches * width
        assert at == (n // B * B if drop_last else n), (n, launches)                   # the launches tile the inputs
        assert got == want, (n, launches)
        assert len(got) == (n // B if drop_last else (n + B - 1) // B)                 # len(loader)


def test_len_of_a_loader_is_the_plans_count(plan):
    """_Loader.__len__ on a stand-in with the three fields it reads."""
    import torch
    from tch_geometric.loader import _Loader

    class Stub(_Loader):
        def __init__(self, n, batch_size, drop_last):
            self.input_nodes, self.batch_size, self.drop_last = torch.arange(n), batch_size, drop_last

    for n in (0, 1, 31, 32, 33, 150, 200):
        for B in (1, 32, 64):
            for drop_last in (False, True):
                assert len(Stub(n, B, drop_last)) == sum(g for _, g, _ in plan(n, B, 5, drop_last))
