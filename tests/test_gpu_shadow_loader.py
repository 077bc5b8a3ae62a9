"""ShaDowKHopLoader: for the same (seed, call ids) every mini-batch has the nodes of NeighborLoader(unique=True,
disjoint=True) -- n_id, batch, node_time -- and the edges of the per-subgraph induced rule
(helpers_shadow.grouped_induced_rule) applied to them, with e_id, edge attributes, layer_edges and root_n_id to match; with
and without times; over full and ragged launches, a second epoch and two iterators at once; and through the capacity
growth path, forced and natural."""
import numpy as np
import pytest
import torch

from helpers_disjoint import temporal_graph
from helpers_induced import edges_before
from helpers_shadow import CHUNK, chunks_of, grouped_induced_rule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, SEED, CALL0, WINDOW = 2000, 13, 700, (0, 400)


@pytest.fixture(scope="module")
def graph():
    from tch_geometric.transforms import Graph
    ei, time, x = temporal_graph(N)
    rs = np.random.default_rng(32)
    w = rs.standard_normal((ei.shape[1], 2)).astype(np.float32)
    data = Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=N, x=torch.from_numpy(x).to(DEV),
                 time=torch.from_numpy(time).to(DEV), w=torch.from_numpy(w).to(DEV))
    nodes = rs.integers(0, 60, 100).astype(np.int64)         # 100 inputs among 60 nodes: the same node under several seeds
    input_time = rs.integers(300, 1300, 100).astype(np.int64)
    return dict(data=data, ei=ei, time=time, x=x, w=w, nodes=nodes, input_time=input_time)


def same(k, loader, s, d, timed):
    """mini-batch s of a ShaDowKHopLoader against mini-batch d of the disjoint loader with the same draws"""
    hp, hi, perm = (t.cpu().numpy() for t in (loader.col_ptrs, loader.row_indices, loader.perm))
    n_id, batch = s.n_id.cpu().numpy(), s.batch.cpu().numpy()
    B = d.batch_size
    assert torch.equal(s.n_id, d.n_id) and torch.equal(s.batch, d.batch) and s.num_nodes == d.num_nodes
    assert s.batch_size == B and s.layer_nodes == d.layer_nodes and s.call_id == d.call_id and s.layer_offsets is None
    assert np.array_equal(s.x.cpu().numpy(), k["x"][n_id])
    ts = group_time = window = None
    if timed:
        assert torch.equal(s.node_time, d.node_time) and torch.equal(s.input_time, d.input_time)
        ts, group_time, window = loader.edge_time.cpu().numpy(), s.input_time.cpu().numpy(), WINDOW
        assert group_time.size == B
    else:
        with pytest.raises(AttributeError):
            s.node_time
    rows, cols, e = grouped_induced_rule(n_id, batch, hp, hi, ts, group_time, window, n_groups=B)
    ei = s.edge_index.cpu().numpy()
    assert np.array_equal(ei, np.stack([rows, cols])) and s.num_edges == rows.size
    e_id = s.e_id.cpu().numpy()
    assert np.array_equal(e_id, perm[e])
    assert np.array_equal(k["ei"][0][e_id], n_id[rows]) and np.array_equal(k["ei"][1][e_id], n_id[cols])
    assert np.array_equal(s.w.cpu().numpy(), k["w"][e_id])                   # edge attributes are gathered by e_id
    assert s.layer_edges == edges_before(cols, s.layer_nodes, n_id.size)
    assert np.array_equal(batch[ei[0]], batch[ei[1]])                        # both ends of every edge share batch
    root = s.root_n_id.cpu().numpy()
    assert root.shape == (B,) and np.array_equal(batch[root], np.arange(B))  # every seed's own entry
    assert np.array_equal(n_id[root], d.n_id.cpu().numpy()[:B])
    if timed:
        age = group_time[batch[cols]] - k["time"][e_id]
        assert np.all((age >= WINDOW[0]) & (age <= WINDOW[1]))
    forest = set(zip(*d.edge_index.cpu().numpy().tolist(), d.e_id.cpu().numpy().tolist())) if d.num_edges else set()
    assert forest <= set(zip(rows.tolist(), cols.tolist(), e_id.tolist()))   # the sampled tree is inside the induced edges
    return s.num_edges - len(forest)


def loaders(k, depth, fan, timed, strategy="uniform", **more):
    from tch_geometric.loader import NeighborLoader, ShaDowKHopLoader
    kw = dict(input_nodes=torch.from_numpy(k["nodes"]), batch_size=16, prefetch=3, seed=SEED, call_id0=CALL0, device=DEV)
    if timed:
        kw.update(time_attr="time", input_time=torch.from_numpy(k["input_time"]), temporal_strategy=strategy,
                  time_window=WINDOW, shuffle=True)
    return (ShaDowKHopLoader(k["data"], depth, fan, **kw, **more),
            NeighborLoader(k["data"], [fan] * depth, unique=True, disjoint=True, **kw))


@pytest.mark.parametrize("depth, fan", [(2, 3), (1, 4)])
def test_untimed_two_epochs_full_and_ragged_launches(graph, depth, fan):
    shadow, disjoint = loaders(graph, depth, fan, False)
    assert len(shadow) == 7 and shadow.disjoint and shadow.induced and shadow.unique and shadow.fanout == [fan] * depth
    for epoch in range(2):
        seen = extra = 0
        for s, d in zip(shadow, disjoint):                                   # launches of 3, 3 and a ragged 4 wide
            extra += same(graph, shadow, s, d, False)
            assert s.call_id == CALL0 + epoch * 7 + seen
            seen += 1
        assert seen == 7 and extra > 0                                       # more than the tree
    assert len(shadow._pool) == 1 and "ind" in shadow._pool[0][0]            # the second epoch reused slabs and workspace


def test_two_iterators_alive_at_once(graph):
    shadow, disjoint = loaders(graph, 2, 3, False)
    n = 0
    for (s0, s1), (d0, d1) in zip(zip(shadow, shadow), zip(disjoint, disjoint)):
        assert s1.call_id == s0.call_id + 7
        same(graph, shadow, s0, d0, False)
        same(graph, shadow, s1, d1, False)
        n += 1
    assert n == 7


@pytest.mark.parametrize("strategy", ["uniform", "last"])
def test_temporal(graph, strategy):
    shadow, disjoint = loaders(graph, 2, 3, True, strategy)
    edges = n = 0
    for s, d in zip(shadow, disjoint):
        same(graph, shadow, s, d, True)
        edges += s.num_edges
        n += 1
    assert n == 7 and edges > 0


def test_forced_growth_gives_the_same_mini_batches(graph):
    for timed in (False, True):
        (tight, _), (roomy, disjoint) = loaders(graph, 2, 3, timed, chunk_cap=1), loaders(graph, 2, 3, timed)
        assert tight.chunk_cap == 1 and roomy.chunk_cap == 0
        for t, r, d in zip(tight, roomy, disjoint):
            same(graph, tight, t, d, timed)
            assert torch.equal(t.edge_index, r.edge_index) and torch.equal(t.e_id, r.e_id) and t.layer_edges == r.layer_edges
        assert tight.chunk_cap > 1 and roomy.chunk_cap == 0                  # the larger capacity is kept


def test_natural_growth_on_a_hub_under_every_seed():
    """a hub column of 1 100 entries and 64 seeds whose only in-neighbour is the hub: fan-out [2] gives pitch 192, the
    default capacity is 192 + ceil(1 164 / 512) = 195 chunks, the mini-batch needs 64 x 3 (the hub under every seed) + 64"""
    from tch_geometric.loader import ShaDowKHopLoader
    from tch_geometric.transforms import Graph
    rs = np.random.default_rng(7)
    n, hub, seeds = 400, 0, np.arange(1, 65)
    into_hub = np.concatenate([seeds, rs.integers(65, n, 1100 - 64)])          # every seed is a source of the hub as well
    ei = np.concatenate([np.stack([into_hub, np.full(1100, hub)]), np.stack([np.full(64, hub), seeds])], axis=1).astype(np.int64)
    data = Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=n)
    loader = ShaDowKHopLoader(data, 1, 2, input_nodes=torch.from_numpy(seeds), batch_size=64, prefetch=2, seed=3, device=DEV)
    hp, hi = loader.col_ptrs.cpu().numpy(), loader.row_indices.cpu().numpy()
    for epoch in range(2):
        (mb,) = list(loader)
        n_id, batch = mb.n_id.cpu().numpy(), mb.batch.cpu().numpy()
        assert mb.num_nodes == 128 and np.array_equal(n_id[:64], seeds) and (n_id[64:] == hub).all()
        assert chunks_of(n_id, hp) == 256 > 192 + -(-ei.shape[1] // CHUNK) == 195
        rows, cols, _ = grouped_induced_rule(n_id, batch, hp, hi, n_groups=64)
        assert np.array_equal(mb.edge_index.cpu().numpy(), np.stack([rows, cols]))
        assert mb.num_edges == 128 and np.array_equal(batch[rows], batch[cols])  # hub -> seed and seed -> hub, per subgraph
        assert loader.chunk_cap >= 256                                        # grown once, kept for the second epoch
