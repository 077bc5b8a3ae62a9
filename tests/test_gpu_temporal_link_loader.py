"""LinkNeighborLoader with time_attr / edge_label_time: both endpoints of a pair sample under the pair's time, a negative
under its positive's; unique=False hands out the temporal forest, unique=True the disjoint contract -- the NumPy
restatement of the grouped dedup (helpers_disjoint) applied to that forest with the link layouts' group maps -- with
edge_label_index (or the triplet indices) taken from the inverse.  Binary and triplet, K = 0 and K = 2, "last" and
"uniform", shuffled, prefetch 3 with a ragged last launch."""
import numpy as np
import pytest
import torch

from helpers_disjoint import BINARY, TRIPLET, disjoint_rule, link_groups, temporal_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, SEED, CALL0, HI, N_LABEL, BATCH = 2000, 14, 900, 500, 76, 8


@pytest.fixture(scope="module")
def graph():
    from tch_geometric.transforms import Graph
    ei, time, x = temporal_graph(N)
    data = Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=N, x=torch.from_numpy(x).to(DEV),
                 time=torch.from_numpy(time).to(DEV))
    rs = np.random.default_rng(33)
    pick = rs.choice(ei.shape[1], N_LABEL, replace=False)
    eli = ei[:, pick].copy()
    eli[1, :6] = eli[0, :6]                                   # a few self pairs: src_j == dst_j inside one subgraph
    elt = 600 + np.arange(N_LABEL, dtype=np.int64) * 5        # distinct, so a time names its label edge
    return dict(data=data, ei=ei, time=time, x=x, eli=eli, elt=elt)


def loaders(k, mode, K, strategy, fanout, **kw):
    from tch_geometric.loader import LinkNeighborLoader
    common = dict(edge_label_index=torch.from_numpy(k["eli"]), neg_sampling_ratio=K, neg_sampling=mode, batch_size=BATCH,
                  prefetch=3, seed=SEED, call_id0=CALL0, device=DEV, time_attr="time",
                  edge_label_time=torch.from_numpy(k["elt"]), temporal_strategy=strategy, time_window=(0, HI), **kw)
    return LinkNeighborLoader(k["data"], fanout, **common), LinkNeighborLoader(k["data"], fanout, unique=True, **common)


@pytest.mark.parametrize("strategy,fanout", [("last", [3, 2]), ("uniform", [4])])
@pytest.mark.parametrize("K", [0, 2])
@pytest.mark.parametrize("mode", ["binary", "triplet"])
def test_forest_and_disjoint_against_the_restatement(graph, mode, K, strategy, fanout):
    k = graph
    forest, disjoint = loaders(k, mode, K, strategy, fanout, shuffle=True)
    assert disjoint.disjoint and not forest.disjoint and len(forest) == len(disjoint) == 10   # 3 + 3 + 3 and a ragged 4
    seen, n, edges = [], 0, 0
    for f, u in zip(forest, disjoint):
        E = f.batch_size
        P = E + E * K
        seed_group, of_positive, n_groups = link_groups(E, K, BINARY if mode == "binary" else TRIPLET)
        S = seed_group.size
        ids = f.input_id.cpu().numpy()
        seen += ids.tolist()
        assert E == (BATCH if n < 9 else 4) and u.batch_size == E and torch.equal(u.input_id, f.input_id)
        # ---- the forest: times travel with their label edges, every seed samples under its positive's time
        s, e = f.n_id.cpu().numpy(), f.edge_index.cpu().numpy()
        t_pos = k["elt"][ids]                                             # shuffle=True keeps times with their edges
        want_elt = t_pos[of_positive[:P]] if mode == "binary" else t_pos
        assert np.array_equal(f.edge_label_time.cpu().numpy(), want_elt)
        assert np.array_equal(f.input_time.cpu().numpy(), t_pos[of_positive]) and f.input_time.numel() == S
        root = np.arange(s.size)
        for i, c in enumerate(e[1]):
            root[S + i] = root[c]
        node_time = f.node_time.cpu().numpy()
        assert np.array_equal(node_time, t_pos[of_positive][root]) and f.batch is None
        e_time = k["time"][f.e_id.cpu().numpy()]
        age = node_time[e[1]] - e_time                                    # 0 <= T_group - t <= hi
        assert np.all((age >= 0) & (age <= HI))
        if mode == "binary":
            eli = f.edge_label_index.cpu().numpy()
            assert np.array_equal(s[eli][:, :E], k["eli"][:, ids]) and eli.shape == (2, P)
        else:
            assert np.array_equal(s[f.src_index.cpu().numpy()], k["eli"][0, ids])
            assert np.array_equal(s[f.dst_pos_index.cpu().numpy()], k["eli"][1, ids])
        # ---- the disjoint mini-batch: the restatement applied to that forest
        starts = [lo[0] for lo in f.layer_offsets]
        nodes, group, inverse, rows_u, cols_u, layers = disjoint_rule(s, e[0], e[1], S, seed_group, starts)
        n_id, batch, ei = u.n_id.cpu().numpy(), u.batch.cpu().numpy(), u.edge_index.cpu().numpy()
        assert np.array_equal(n_id, nodes) and np.array_equal(batch, group)
        assert np.array_equal(ei, np.stack([rows_u, cols_u])) and u.layer_nodes == layers
        assert u.layer_offsets == f.layer_offsets and u.call_id == f.call_id and torch.equal(u.e_id, f.e_id)
        assert torch.equal(u.edge_label_time, f.edge_label_time) and torch.equal(u.input_time, f.input_time)
        assert np.array_equal(u.node_time.cpu().numpy(), want_elt[batch]) and want_elt.size == n_groups
        assert len(set(zip(batch.tolist(), n_id.tolist()))) == n_id.size  # pairs (batch, n_id) are distinct
        assert np.array_equal(batch[ei[0]], batch[ei[1]])                 # both ends of every edge share batch
        assert np.array_equal(u.x.cpu().numpy(), k["x"][n_id])
        if mode == "binary":
            got = u.edge_label_index.cpu().numpy()
            assert np.array_equal(got, inverse[:S].reshape(2, P))
            assert np.array_equal(n_id[got], s[:S].reshape(2, P))          # the global endpoints, negatives included
            assert np.array_equal(batch[got[0]], np.arange(P)) and np.array_equal(batch[got[1]], np.arange(P))
            assert torch.equal(u.edge_label, f.edge_label)
            same = k["eli"][0, ids] == k["eli"][1, ids]
            assert np.array_equal(got[0, :E][same], got[1, :E][same])     # src_j == dst_j: one entry of the pair's subgraph
        else:
            src, pos, neg = (x.cpu().numpy() for x in (u.src_index, u.dst_pos_index, u.dst_neg_index))
            assert np.array_equal(src, inverse[:E]) and np.array_equal(pos, inverse[E:2 * E])
            assert np.array_equal(neg, inverse[2 * E:S].reshape(E, K)) and neg.shape == (E, K)
            assert np.array_equal(n_id[src], k["eli"][0, ids]) and np.array_equal(n_id[pos], k["eli"][1, ids])
            assert np.array_equal(n_id[neg], s[2 * E:S].reshape(E, K))
            assert np.array_equal(batch[src], np.arange(E)) and np.array_equal(batch[pos], np.arange(E))
            assert np.array_equal(batch[neg], np.repeat(np.arange(E), K).reshape(E, K))
        n += 1
        edges += u.num_edges
    assert n == 10 and edges > 0 and sorted(seen) == list(range(N_LABEL)) and seen != list(range(N_LABEL))


def test_untimed_disjoint_link_loader(graph):
    """disjoint=True without times: the same group maps, no time fields."""
    from tch_geometric.loader import LinkNeighborLoader
    k = graph
    kw = dict(edge_label_index=torch.from_numpy(k["eli"]), neg_sampling_ratio=1, batch_size=16, prefetch=2, seed=SEED,
              call_id0=CALL0, device=DEV)
    forest = LinkNeighborLoader(k["data"], [3, 2], **kw)
    disjoint = LinkNeighborLoader(k["data"], [3, 2], unique=True, disjoint=True, **kw)
    for f, u in zip(forest, disjoint):
        E = f.batch_size
        seed_group, _, _ = link_groups(E, 1, BINARY)
        s, e = f.n_id.cpu().numpy(), f.edge_index.cpu().numpy()
        nodes, group, inverse, rows_u, cols_u, layers = disjoint_rule(s, e[0], e[1], 4 * E, seed_group,
                                                                      [lo[0] for lo in f.layer_offsets])
        assert np.array_equal(u.n_id.cpu().numpy(), nodes) and np.array_equal(u.batch.cpu().numpy(), group)
        assert np.array_equal(u.edge_index.cpu().numpy(), np.stack([rows_u, cols_u])) and u.layer_nodes == layers
        assert np.array_equal(u.edge_label_index.cpu().numpy(), inverse[:4 * E].reshape(2, 2 * E))
        assert u.edge_label_time is None and f.edge_label_time is None


def test_refusals_come_before_device_work(graph):
    from tch_geometric.loader import LinkNeighborLoader
    k = graph
    eli, elt = torch.from_numpy(k["eli"]), torch.from_numpy(k["elt"])
    with pytest.raises(ValueError, match="come together"):
        LinkNeighborLoader(k["data"], [3], edge_label_index=eli, edge_label_time=elt, device=DEV)
    with pytest.raises(ValueError, match="come together"):
        LinkNeighborLoader(k["data"], [3], edge_label_index=eli, time_attr="time", device=DEV)
    with pytest.raises(ValueError, match="edge_label_time"):
        LinkNeighborLoader(k["data"], [3], edge_label_index=eli, time_attr="time", edge_label_time=elt.to(torch.int32), device=DEV)
    with pytest.raises(ValueError, match="edge_label_time"):
        LinkNeighborLoader(k["data"], [3], edge_label_index=eli, time_attr="time", edge_label_time=elt[:-1], device=DEV)
    with pytest.raises(ValueError, match="unique=True"):
        LinkNeighborLoader(k["data"], [3], edge_label_index=eli, disjoint=True, device=DEV)
    with pytest.raises(ValueError, match="temporal_strategy"):
        LinkNeighborLoader(k["data"], [3], edge_label_index=eli, temporal_strategy="last", device=DEV)
