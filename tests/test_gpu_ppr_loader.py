"""PPRLoader: every mini-batch has the nodes, groups and weights of the restatement (helpers_ppr) per seed and the edges of
the per-subgraph induced rule (helpers_shadow) on those lists; over two epochs, prefetch 1 against 4, two iterators at once;
a too-small node_cap raises."""
import numpy as np
import pytest
import torch

import helpers_ppr as hp
from helpers_induced import csc_of
from helpers_shadow import grouped_induced_rule
from test_gpu_ppr import N, csr, edges

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, B = 12, 16


@pytest.fixture(scope="module")
def graph():
    from tch_geometric.transforms import Graph
    ei = edges()
    rs = np.random.default_rng(3)
    x = rs.standard_normal((N, 3)).astype(np.float32)
    w = rs.standard_normal((ei.shape[1], 2)).astype(np.float32)
    data = Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=N, x=torch.from_numpy(x).to(DEV), w=torch.from_numpy(w).to(DEV))
    nodes = rs.integers(0, N, 100).astype(np.int64)          # 100 inputs: 6 mini-batches of 16 and a ragged one of 4
    return dict(data=data, ei=ei, x=x, w=w, nodes=nodes, out=csr(ei, N), csc=csc_of(ei, N), memo={})


def loader(g, **kw):
    from tch_geometric.loader import PPRLoader
    kw = dict(dict(k=K, alpha=0.15, eps=5e-4, input_nodes=torch.from_numpy(g["nodes"]), batch_size=B, prefetch=4, device=DEV), **kw)
    return PPRLoader(g["data"], **kw)


def same(g, ld, mb, seeds):
    """mini-batch mb against the restatement over `seeds`"""
    n_id, batch, ppr = [], [], []
    for slot, s in enumerate(seeds.tolist()):
        if s not in g["memo"]:
            st = hp.push(*g["out"], s, ld.sizes.alpha_q, ld.sizes.eps_q, ld.sizes.max_rounds, ld.node_cap)
            g["memo"][s] = hp.top(st, s, K)
        nodes, score = g["memo"][s]
        n_id += nodes
        batch += [slot] * len(nodes)
        ppr += score
    n_id, batch = np.array(n_id, dtype=np.int64), np.array(batch, dtype=np.int64)
    assert np.array_equal(mb.n_id.cpu().numpy(), n_id) and np.array_equal(mb.batch.cpu().numpy(), batch)
    assert np.array_equal(mb.ppr.cpu().numpy(), np.array(ppr, dtype=np.float32) * np.float32(2.0 ** -31))
    assert mb.batch_size == len(seeds) and mb.num_nodes == n_id.size
    root = mb.root_n_id.cpu().numpy()
    assert np.array_equal(n_id[root], seeds) and np.array_equal(batch[root], np.arange(len(seeds)))
    ptrs, indices, perm = g["csc"]
    rows, cols, e = grouped_induced_rule(n_id, batch, ptrs, indices, n_groups=B)
    assert np.array_equal(mb.edge_index.cpu().numpy(), np.stack([rows, cols])) and mb.num_edges == rows.size
    e_id = mb.e_id.cpu().numpy()
    assert np.array_equal(g["ei"][0][e_id], n_id[rows]) and np.array_equal(g["ei"][1][e_id], n_id[cols])
    assert np.array_equal(mb.x.cpu().numpy(), g["x"][n_id]) and np.array_equal(mb.w.cpu().numpy(), g["w"][e_id])
    return rows.size


@pytest.mark.parametrize("prefetch", [1, 4])
def test_two_epochs_full_and_ragged_mini_batches(graph, prefetch):
    ld = loader(graph, prefetch=prefetch)
    assert len(ld) == 7 and ld.node_cap == N
    for epoch in range(2):
        seen = edges_ = 0
        for j, mb in enumerate(ld):
            edges_ += same(graph, ld, mb, graph["nodes"][j * B:(j + 1) * B])
            assert mb.call_id == epoch * 7 + j
            seen += 1
        assert seen == 7 and edges_ > 0
    assert ld.slab_allocations == 1                          # the second epoch reused the slab set


def test_two_iterators_shuffle_drop_last_and_forced_chunk_growth(graph):
    ld = loader(graph, shuffle=True, drop_last=True, seed=5, chunk_cap=1)
    assert len(ld) == 6
    orders = []
    for epoch in range(2):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(5 * 1000003 + epoch)
        orders.append(graph["nodes"][torch.randperm(100, device=DEV, generator=gen).cpu().numpy()])
    n = 0
    for j, (a, b) in enumerate(zip(ld, ld)):                 # the second iterator is the next epoch
        same(graph, ld, a, orders[0][j * B:(j + 1) * B])
        same(graph, ld, b, orders[1][j * B:(j + 1) * B])
        n += 1
    assert n == 6 and ld.slab_allocations == 2 and ld.chunk_cap > 1


def test_a_too_small_node_cap_raises_and_refusals_need_no_launch(graph):
    with pytest.raises(RuntimeError, match="node_cap = 20"):
        list(loader(graph, node_cap=20))
    for kw in (dict(k=0), dict(k=21, node_cap=20), dict(batch_size=0), dict(prefetch=0), dict(chunk_cap=0), dict(alpha=-1.0, node_cap=0)):
        with pytest.raises(ValueError):
            loader(graph, **kw)
