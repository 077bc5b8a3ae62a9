"""NeighborLoader(unique=True, disjoint=True) with and without seed times: for the
same (seed, call_id0) the unique=False loader hands out the forest, and the disjoint loader must hand out the NumPy
restatement of the grouped dedup (helpers_disjoint.disjoint_rule, one subgraph per seed) applied to that forest -- n_id,
edge_index, batch, node_time, layer_nodes -- plus the properties a consumer relies on, and the refusals that remain."""
import numpy as np
import pytest
import torch

from helpers_disjoint import disjoint_rule, temporal_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, SEED, CALL0, HI = 2000, 13, 700, 400


@pytest.fixture(scope="module")
def graph():
    from tch_geometric.transforms import Graph
    ei, time, x = temporal_graph(N)
    data = Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=N, x=torch.from_numpy(x).to(DEV),
                 time=torch.from_numpy(time).to(DEV))
    rs = np.random.default_rng(32)
    nodes = rs.integers(0, 60, 100).astype(np.int64)         # 100 inputs among 60 nodes: the same node under several seeds
    input_time = rs.integers(300, 1300, 100).astype(np.int64)
    return dict(data=data, ei=ei, time=time, x=x, nodes=nodes, input_time=input_time)


def pairs_of(forest, disjoint):
    """zip of the two loaders' mini-batches with what every case checks: the restatement and the properties."""
    n = 0
    for f, u in zip(forest, disjoint):
        s, e = f.n_id.cpu().numpy(), f.edge_index.cpu().numpy()
        B = f.batch_size
        starts = [lo[0] for lo in f.layer_offsets]
        nodes, group, inverse, rows_u, cols_u, layers = disjoint_rule(s, e[0], e[1], B, None, starts)
        n_id, batch, ei = u.n_id.cpu().numpy(), u.batch.cpu().numpy(), u.edge_index.cpu().numpy()
        assert np.array_equal(n_id, nodes) and np.array_equal(batch, group) and u.num_nodes == nodes.size
        assert np.array_equal(ei, np.stack([rows_u, cols_u])) and u.num_edges == f.num_edges
        assert u.layer_nodes == layers and u.layer_offsets == f.layer_offsets and u.call_id == f.call_id
        assert u.batch_size == B and (not layers or layers[0] == B)       # one subgraph per seed: every seed is distinct
        assert np.array_equal(n_id[:B], s[:B]) and np.array_equal(batch[:B], np.arange(B))
        assert len(set(zip(batch.tolist(), n_id.tolist()))) == n_id.size  # pairs (batch, n_id) are distinct
        assert np.array_equal(batch[ei[0]], batch[ei[1]])                 # both ends of every edge share batch
        assert torch.equal(u.e_id, f.e_id) and f.batch is None
        n += 1
        yield f, u, n_id, batch, ei
    assert n == len(forest) == len(disjoint)


@pytest.mark.parametrize("fanout", [[3, 2], [4]])
def test_untimed_disjoint_against_the_forest_loader(graph, fanout):
    from tch_geometric.loader import NeighborLoader
    k = graph
    kw = dict(input_nodes=torch.from_numpy(k["nodes"]), batch_size=16, prefetch=3, seed=SEED, call_id0=CALL0, device=DEV)
    forest = NeighborLoader(k["data"], fanout, **kw)
    disjoint = NeighborLoader(k["data"], fanout, unique=True, disjoint=True, **kw)
    plain = NeighborLoader(k["data"], fanout, unique=True, **kw)
    assert len(disjoint) == 7 and disjoint.disjoint and not plain.disjoint and not forest.disjoint
    more = 0
    for (f, u, n_id, batch, ei), p in zip(pairs_of(forest, disjoint), plain):
        assert np.array_equal(u.x.cpu().numpy(), k["x"][n_id])
        assert p.batch is None and p.num_nodes <= u.num_nodes <= f.num_nodes
        more += p.num_nodes < u.num_nodes
        with pytest.raises(AttributeError):
            u.node_time
    assert more > 0                                                       # nodes the plain dedup merged across seeds stay apart


@pytest.mark.parametrize("strategy", ["last", "uniform"])
@pytest.mark.parametrize("fanout", [[3, 2], [4]])
def test_temporal_disjoint_against_the_temporal_forest(graph, strategy, fanout):
    from tch_geometric.loader import NeighborLoader
    k = graph
    kw = dict(input_nodes=torch.from_numpy(k["nodes"]), batch_size=32, prefetch=3, seed=SEED, call_id0=CALL0, device=DEV,
              time_attr="time", input_time=torch.from_numpy(k["input_time"]), temporal_strategy=strategy, time_window=(0, HI),
              shuffle=True)
    forest, disjoint = NeighborLoader(k["data"], fanout, **kw), NeighborLoader(k["data"], fanout, unique=True, disjoint=True, **kw)
    assert disjoint.disjoint and len(disjoint) == 4                       # 3 x 32 in one launch, a ragged 4
    edges = 0
    for f, u, n_id, batch, ei in pairs_of(forest, disjoint):
        t0 = u.input_time.cpu().numpy()
        assert torch.equal(u.input_time, f.input_time) and t0.size == u.batch_size
        assert np.array_equal(u.node_time.cpu().numpy(), t0[batch])       # time is a function of the subgraph
        age = t0[batch[ei[1]]] - k["time"][u.e_id.cpu().numpy()]
        assert np.all((age >= 0) & (age <= HI))
        assert np.array_equal(k["ei"][0][u.e_id.cpu().numpy()], n_id[ei[0]])
        assert np.array_equal(k["ei"][1][u.e_id.cpu().numpy()], n_id[ei[1]])
        assert np.array_equal(u.x.cpu().numpy(), k["x"][n_id])
        edges += u.num_edges
    assert edges > 0


def test_refusals_and_the_graphs_own_batch_attribute(graph):
    from tch_geometric.loader import NeighborLoader
    from tch_geometric.transforms import Graph
    k = graph
    nodes, t = torch.from_numpy(k["nodes"]), torch.from_numpy(k["input_time"])
    with pytest.raises(ValueError, match="unique=True"):
        NeighborLoader(k["data"], [3], input_nodes=nodes, disjoint=True, device=DEV)
    with pytest.raises(ValueError, match="out of scope"):
        NeighborLoader(k["data"], [3], input_nodes=nodes, unique=True, induced=True, disjoint=True, device=DEV)
    with pytest.raises(ValueError, match="out of scope"):
        NeighborLoader(k["data"], [3], input_nodes=nodes, unique=True, induced=True, disjoint=True, time_attr="time",
                       input_time=t, device=DEV)
    with pytest.raises(ValueError, match="needs disjoint=True"):          # plain dedup under seed times stays refused
        NeighborLoader(k["data"], [3], input_nodes=nodes, unique=True, time_attr="time", input_time=t, device=DEV)
    own = Graph(edge_index=k["data"].edge_index, num_nodes=N, batch=torch.arange(N, device=DEV) % 7)
    with pytest.raises(ValueError, match="batch"):
        NeighborLoader(own, [3], input_nodes=nodes, unique=True, disjoint=True, device=DEV)
    for b in NeighborLoader(own, [3], input_nodes=nodes[:20], unique=True, batch_size=10, device=DEV):
        assert torch.equal(b.batch, b.n_id % 7)                           # not disjoint: the name stays the graph's attribute
