"""SEALLoader: every mini-batch has the nodes, link slots and labels of the restatement (helpers_seal) per link on the CSC and
the edges of the per-subgraph induced rule (helpers_shadow) on those lists; target_edge against its definition; over two
epochs, prefetch 1 against 4, shuffled with drop_last through the chunk-cap growth path; a too-small node_cap raises."""
import numpy as np
import pytest
import torch

import helpers_seal as hs
from helpers_induced import csc_of
from helpers_shadow import grouped_induced_rule
from test_gpu_seal import HUB, N, edges

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, L, HOPS, CAP, ZMAX = 16, 100, 2, 300, 9


@pytest.fixture(scope="module")
def graph():
    from tch_geometric.transforms import Graph
    ei = np.ascontiguousarray(edges()[::-1])                 # reversed: the hub's 1 101 entries are one COLUMN of the CSC
    rs = np.random.default_rng(3)
    x = rs.standard_normal((N, 3)).astype(np.float32)
    w = rs.standard_normal((ei.shape[1], 2)).astype(np.float32)
    data = Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=N, x=torch.from_numpy(x).to(DEV), w=torch.from_numpy(w).to(DEV))
    links = rs.integers(0, N, (2, L)).astype(np.int64)       # 100 links: 6 mini-batches of 16 and a ragged one of 4
    links[:, :3] = [[1, HUB, 3], [0, 5, HUB]]                # an edge of the graph with parallel entries; two links on the hub
    links[1] = np.where(links[0] == links[1], (links[1] + 1) % N, links[1])
    label = (np.arange(L) % 2).astype(np.float32)
    return dict(data=data, ei=ei, x=x, w=w, links=links, label=label, csc=csc_of(ei, N), memo={})


def loader(g, **kw):
    from tch_geometric.loader import SEALLoader
    kw = dict(dict(edge_label_index=torch.from_numpy(g["links"]), edge_label=torch.from_numpy(g["label"]), num_hops=HOPS,
                   node_cap=CAP, z_max=ZMAX, batch_size=B, prefetch=4, device=DEV), **kw)
    return SEALLoader(g["data"], **kw)


def same(g, mb, picked, labelled=True):
    """mini-batch mb against the restatement over the links at the positions `picked` -> its target edges"""
    ptrs, indices, perm = g["csc"]
    links = g["links"][:, picked]
    n_id, batch, z = [], [], []
    for slot, (u, v) in enumerate(links.T.tolist()):
        if (u, v) not in g["memo"]:
            g["memo"][u, v] = hs.seal(ptrs, indices, u, v, HOPS, CAP, ZMAX)
        st = g["memo"][u, v]
        n_id += st["nodes"]
        batch += [slot] * len(st["nodes"])
        z += st["z"]
    n_id, batch = np.array(n_id, dtype=np.int64), np.array(batch, dtype=np.int64)
    assert np.array_equal(mb.n_id.cpu().numpy(), n_id) and np.array_equal(mb.batch.cpu().numpy(), batch)
    assert np.array_equal(mb.z.cpu().numpy(), np.array(z, dtype=np.int64))
    assert mb.batch_size == len(picked) and mb.num_nodes == n_id.size
    assert np.array_equal(mb.edge_label_index.cpu().numpy(), links)
    assert np.array_equal(mb.edge_label.cpu().numpy(), g["label"][picked]) if labelled else mb.edge_label is None
    root = mb.root_n_id.cpu().numpy()
    assert root.shape == (len(picked), 2) and np.array_equal(n_id[root].T, links)
    rows, cols, e = grouped_induced_rule(n_id, batch, ptrs, indices, n_groups=B)
    assert np.array_equal(mb.edge_index.cpu().numpy(), np.stack([rows, cols])) and mb.num_edges == rows.size
    e_id = mb.e_id.cpu().numpy()
    assert np.array_equal(g["ei"][0][e_id], n_id[rows]) and np.array_equal(g["ei"][1][e_id], n_id[cols])
    assert np.array_equal(mb.x.cpu().numpy(), g["x"][n_id]) and np.array_equal(mb.w.cpu().numpy(), g["w"][e_id])
    u, v = links[:, batch[cols]]                             # the definition: the two ends are the link's two roots and differ
    target = ((n_id[rows] == u) & (n_id[cols] == v)) | ((n_id[rows] == v) & (n_id[cols] == u))
    assert np.array_equal(mb.target_edge.cpu().numpy(), target)
    return int(target.sum())


@pytest.mark.parametrize("prefetch", [1, 4])
def test_two_epochs_full_and_ragged_mini_batches(graph, prefetch):
    ld = loader(graph, prefetch=prefetch)
    assert len(ld) == 7
    for epoch in range(2):
        seen = targets = 0
        for j, mb in enumerate(ld):
            targets += same(graph, mb, np.arange(j * B, min((j + 1) * B, L)))
            assert mb.call_id == epoch * 7 + j
            seen += 1
        assert seen == 7 and targets >= 5                    # the 3 + 2 parallel entries of the link (1, 0) at least
    assert ld.slab_allocations == 1                          # the second epoch reused the slab set


def test_shuffle_drop_last_and_the_chunk_growth_path_under_the_hub(graph):
    ld = loader(graph, shuffle=True, drop_last=True, seed=5, chunk_cap=1, edge_label=None)
    assert len(ld) == 6
    for epoch in range(2):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(5 * 1000003 + epoch)
        order = torch.randperm(L, device=DEV, generator=gen).cpu().numpy()
        n = 0
        for j, mb in enumerate(ld):
            same(graph, mb, order[j * B:(j + 1) * B], labelled=False)
            n += 1
        assert n == 6 and ld.chunk_cap >= 3                  # the hub's column alone is three chunks
    assert ld.slab_allocations == 1


def test_a_too_small_node_cap_raises_naming_it(graph):
    with pytest.raises(RuntimeError, match="node_cap = 20"):
        list(loader(graph, node_cap=20))
