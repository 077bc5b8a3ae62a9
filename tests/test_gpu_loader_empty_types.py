"""A node type or a relation that collects nothing over a WHOLE launch: HeteroNeighborLoader and HGTLoader hand out
empty tensors there (as the per-call operators do) and everything else still equals the oracle.  The fake hetero fixture
reaches every one of its types, so it gets one more node type that no sampled edge leads to and one more relation
without edges (from that type into the seeds' type)."""
import numpy as np
import pytest
import torch

import orc
from helpers import load_fake_hetero, rel_key

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LONELY = "zz_unreached"                                 # sorts behind the fixture's types: the seeds' type stays first


def _data():
    from tch_geometric.transforms import HeteroGraph
    counts, edges = load_fake_hetero()
    nt0 = sorted(counts)[0]
    assert LONELY not in counts and LONELY > max(counts)
    counts[LONELY] = 7
    empty = (LONELY, "none", nt0)
    edges[empty] = np.zeros((2, 0), dtype=np.int64)
    node_types, edge_types = sorted(counts), sorted(edges)
    rs = np.random.default_rng(4)
    data, feats, eattr = HeteroGraph(), {}, {}
    for nt in node_types:
        feats[nt] = rs.standard_normal((counts[nt], 6)).astype(np.float32)
        data[nt].x, data[nt].num_nodes = torch.from_numpy(feats[nt]).to(DEV), counts[nt]
    for et in edge_types:
        data[et].edge_index = torch.from_numpy(edges[et]).to(DEV)
        eattr[et] = rs.standard_normal((edges[et].shape[1], 3)).astype(np.float32)
        data[et].edge_attr = torch.from_numpy(eattr[et]).to(DEV)
    P, I, PERM = {}, {}, {}
    for et in edge_types:
        P[rel_key(et)], I[rel_key(et)], PERM[rel_key(et)] = orc.to_csc(edges[et], (counts[et[0]], counts[et[2]]))
    nodes = torch.from_numpy(rs.integers(0, counts[nt0], 150))
    return data, node_types, edge_types, nt0, empty, nodes, feats, eattr, P, I, PERM


def _check_batch(b, node_types, edge_types, empty, o_nodes, o_rows, o_cols, o_eidx, feats, eattr, PERM, where):
    for nt in node_types:
        s = b[nt].n_id.cpu().numpy()
        assert np.array_equal(s, o_nodes[nt]), (where, nt)
        assert b[nt].num_nodes == len(s) and np.array_equal(b[nt].x.cpu().numpy(), feats[nt][s]), (where, nt)
    for et in edge_types:
        k = rel_key(et)
        assert np.array_equal(b[et].edge_index.cpu().numpy(), np.stack([o_rows[k], o_cols[k]])), (where, k)
        assert np.array_equal(b[et].e_id.cpu().numpy(), PERM[k][o_eidx[k]]), (where, k)
        assert np.array_equal(b[et].edge_attr.cpu().numpy(), eattr[et][PERM[k][o_eidx[k]]]), (where, k)
    # what collected nothing: empty tensors of the usual shape, dtype and device
    n_id = b[LONELY].n_id
    assert n_id.shape == (0,) and n_id.dtype == torch.int64 and n_id.is_cuda and b[LONELY].num_nodes == 0
    assert b[LONELY].x.shape == (0, 6) and b[LONELY].x.dtype == torch.float32
    st = b[empty]
    assert st.edge_index.shape == (2, 0) and st.edge_index.dtype == torch.int64 and st.edge_index.is_cuda
    assert st.e_id.shape == (0,) and st.e_id.dtype == torch.int64 and st.e_id.is_cuda
    assert st.edge_attr.shape == (0, 3) and st.edge_attr.dtype == torch.float32


def test_hetero_neighbor_loader_with_an_unreached_type_and_an_empty_relation():
    from tch_geometric.loader import HeteroNeighborLoader
    data, node_types, edge_types, nt0, empty, nodes, feats, eattr, P, I, PERM = _data()
    loader = HeteroNeighborLoader(data, [4, 3], nt0, input_nodes=nodes, batch_size=32, prefetch=3, seed=5, call_id0=40)
    assert len(loader) == 5
    nn = {rel_key(et): [4, 3] for et in edge_types}
    n_seen = 0
    for j, b in enumerate(loader):
        seeds = nodes[j * 32:(j + 1) * 32].numpy()
        o = orc.ns_hetero(node_types, edge_types, P, I, {nt0: seeds}, nn, 2, orc.rng_philox(5, 40 + j))
        _check_batch(b, node_types, edge_types, empty, o[0], o[1], o[2], o[3], feats, eattr, PERM, j)
        for et in edge_types:
            assert b[et].layer_offsets == o[4][rel_key(et)], (j, et)
        assert b[nt0].batch_size == len(seeds) and b.call_id == 40 + j
        n_seen += 1
    assert n_seen == 5


def test_hgt_loader_with_an_unreached_type_and_an_empty_relation():
    from tch_geometric.loader import HGTLoader
    data, node_types, edge_types, nt0, empty, nodes, feats, eattr, P, I, PERM = _data()
    loader = HGTLoader(data, [12, 8], nt0, input_nodes=nodes, batch_size=32, prefetch=3, seed=5, call_id0=40)
    assert len(loader) == 5 and loader.prefetch == 3
    ns = {t: [12, 8] for t in node_types}
    n_seen = 0
    for j, b in enumerate(loader):
        seeds = nodes[j * 32:(j + 1) * 32].numpy()
        o = orc.hgt(node_types, edge_types, P, I, None, {nt0: seeds}, None, ns, 2, orc.rng_philox(5, 40 + j))
        _check_batch(b, node_types, edge_types, empty, o[0], o[2], o[3], o[4], feats, eattr, PERM, j)
        for nt in node_types:
            assert np.array_equal(b.samples_timestamps[nt].cpu().numpy(), o[1][nt]), (j, nt)
        assert b.samples_timestamps[LONELY].shape == (0,) and b.samples_timestamps[LONELY].dtype == torch.int64
        assert b[nt0].batch_size == len(seeds) and b.call_id == 40 + j
        n_seen += 1
    assert n_seen == 5
