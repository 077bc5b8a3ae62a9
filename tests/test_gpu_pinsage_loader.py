"""PinSAGELoader on a 300-vertex multigraph with sinks: every block of every mini-batch equals helpers_pinsage.blocks applied
to _cabi.pinsage_hop outputs computed mini-batch by mini-batch (so a mini-batch does not depend on what else is in its
launch), the gathered features follow, prefetch does not change a word, epochs differ, two live iterators do not disturb
each other, and walk_out_edges=True walks the CSR."""
import numpy as np
import pytest
import torch

from helpers_pinsage import blocks, csx
from helpers_saint import random_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, FAN, B, R, T, ALPHA, SEED, CALL0 = 300, [3, 2], 7, 10, 3, 0.5, 77, 1000


@pytest.fixture(scope="module")
def case():
    from tch_geometric.transforms import Graph
    ei = random_graph(N, 2000, 0.1, seed=4)
    rs = np.random.default_rng(8)
    x = rs.standard_normal((N, 16)).astype(np.float32)
    inputs = rs.permutation(N)[:50].astype(np.int64)
    data = Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=N, x=torch.from_numpy(x).to(DEV))
    return dict(data=data, ei=ei, x=x, inputs=inputs)


def build(k, **kw):
    from tch_geometric import PinSAGELoader
    args = dict(input_nodes=torch.from_numpy(k["inputs"]), batch_size=B, n_walks=R, walk_length=T, termination=ALPHA,
                prefetch=4, seed=SEED, call_id0=CALL0, device=DEV)
    args.update(kw)
    return PinSAGELoader(k["data"], FAN, **args)


def restated_batch(graph, seeds, run_index):
    """mini-batch `run_index` (epoch * len(loader) + j) from single-mini-batch hops"""
    from tch_geometric import _cabi

    def hop(l, F):
        out = _cabi.pinsage_hop(graph, torch.from_numpy(F).to(DEV), FAN[l], R, T, ALPHA, SEED,
                                CALL0 + run_index * len(FAN) + l)
        cnt, off, nbr, par, vis = (t.cpu().numpy() for t in out)
        total = int(off[-1])
        return cnt, nbr[:total], par[:total], vis[:total]

    return blocks(seeds, hop, len(FAN))


def as_host(mb):
    return dict(n_id=mb.n_id.cpu().numpy(), x=mb.x.cpu().numpy(), input_nodes=mb.input_nodes.cpu().numpy(),
                batch_size=mb.batch_size,
                blocks=[dict(n_id=b.n_id.cpu().numpy(), n_dst=b.n_dst, edge_index=b.edge_index.cpu().numpy(),
                             edge_weight=b.edge_weight.cpu().numpy()) for b in mb.blocks])


def same(a, b):
    return (np.array_equal(a["n_id"], b["n_id"]) and np.array_equal(a["x"], b["x"]) and a["batch_size"] == b["batch_size"]
            and len(a["blocks"]) == len(b["blocks"])
            and all(x["n_dst"] == y["n_dst"] and all(np.array_equal(x[f], y[f]) for f in ("n_id", "edge_index", "edge_weight"))
                    for x, y in zip(a["blocks"], b["blocks"])))


def check_epoch(k, loader, graph, epoch):
    got = [as_host(mb) for mb in loader]
    assert len(got) == len(loader) == 8
    for j, mb in enumerate(got):
        seeds = k["inputs"][j * B:(j + 1) * B]
        want, F = restated_batch(graph, seeds, epoch * len(loader) + j)
        assert mb["batch_size"] == len(seeds) and np.array_equal(mb["input_nodes"], seeds)
        assert np.array_equal(mb["n_id"], F) and np.array_equal(mb["x"], k["x"][F])
        assert len(mb["blocks"]) == len(FAN)
        for blk, ref in zip(mb["blocks"], want):
            assert blk["n_dst"] == ref["n_dst"] and blk["edge_weight"].dtype == np.int64
            for f in ("n_id", "edge_index", "edge_weight"):
                assert np.array_equal(blk[f], ref[f]), (j, f)
        # outermost first; the first n_dst entries of a block's n_id are the previous frontier, in order
        inner, outer = mb["blocks"][1], mb["blocks"][0]
        assert np.array_equal(inner["n_id"][:inner["n_dst"]], seeds) and inner["n_dst"] == len(seeds)
        assert np.array_equal(outer["n_id"][:outer["n_dst"]], inner["n_id"]) and outer["n_dst"] == len(inner["n_id"])
        assert len(set(mb["n_id"].tolist())) == len(mb["n_id"])
        assert (inner["edge_weight"] >= 1).all() and inner["edge_index"][1].max() < inner["n_dst"]
    assert got[-1]["batch_size"] == 50 - 7 * B
    return got


def test_blocks_equal_the_restatement_over_two_epochs(case):
    loader = build(case)
    first = check_epoch(case, loader, loader._walk_graph, 0)
    second = check_epoch(case, loader, loader._walk_graph, 1)
    assert not all(same(a, b) for a, b in zip(first, second))
    sizes = [len(sb) for sb in build(case).super_batches()]
    assert sizes == [4, 3, 1]


def test_prefetch_does_not_change_a_word(case):
    a = [as_host(mb) for mb in build(case, prefetch=1)]
    b = [as_host(mb) for mb in build(case, prefetch=4)]
    assert len(a) == len(b) == 8 and all(same(x, y) for x, y in zip(a, b))


def test_two_live_iterators_do_not_disturb_each_other(case):
    ref = build(case)
    e0, e1 = [as_host(mb) for mb in ref], [as_host(mb) for mb in ref]
    loader = build(case)
    pairs = [(as_host(x), as_host(y)) for x, y in zip(loader, loader)]     # the second iterator is the next epoch
    assert len(pairs) == 8
    assert all(same(x, a) and same(y, b) for (x, y), a, b in zip(pairs, e0, e1))


def test_walk_out_edges_walks_the_csr(case):
    from tch_geometric import _cabi
    loader = build(case, walk_out_edges=True)
    ptrs, idx = csx(case["ei"], N, False)
    keep = (torch.from_numpy(ptrs).to(DEV), torch.from_numpy(idx).to(DEV))
    graph = _cabi.graph_view(*keep)
    out = check_epoch(case, loader, graph, 0)
    inward = [as_host(mb) for mb in build(case)]
    assert not all(same(a, b) for a, b in zip(out, inward))
