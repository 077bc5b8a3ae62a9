"""ClusterData / ClusterLoader on a random multigraph under a random and a range partition: the setup equals the restated
renumbering, every mini-batch equals the restatement (helpers_cluster: epoch order, expand, induced_rule) in original ids,
data.edge_index[:, e_id] == n_id[edge_index], attributes follow; every cluster once per epoch with and without drop_last,
shuffling differs between epochs and repeats from (seed, epoch), prefetch 1 and 4 agree, two live iterators own a slab set
each and a second epoch allocates nothing."""
import numpy as np
import pytest
import torch

from helpers_cluster import cluster_rule, epoch_lists, renumber

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, E, P, Q, SEED = 600, 7000, 23, 4, 5


@pytest.fixture(scope="module", params=["random", "range"])
def case(request):
    from tch_geometric.loader import ClusterData, random_partition, range_partition
    from tch_geometric.transforms import Graph
    rs = np.random.default_rng(3)
    ei = rs.integers(0, N, (2, E)).astype(np.int64)
    ei[:, :40] = ei[:, 40:80]                                            # parallel edges
    ei[1, 80:120] = ei[0, 80:120]                                        # self loops
    x = rs.standard_normal((N, 3)).astype(np.float32)
    w = rs.standard_normal((E, 2)).astype(np.float32)
    data = Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=N, x=torch.from_numpy(x).to(DEV),
                 edge_attr=torch.from_numpy(w).to(DEV))
    part = random_partition(N, P, 9) if request.param == "random" else range_partition(N, P)
    if request.param == "random":
        part[part == 7] = 8                                              # an empty cluster
    cd = ClusterData(data, part, P, device=DEV)
    host = renumber(part.numpy(), P, ei)
    return dict(cd=cd, data=data, ei=ei, x=x, w=w, part=part.numpy(), host=host)


def build(k, **kw):
    from tch_geometric.loader import ClusterLoader
    args = dict(batch_size=Q, prefetch=4, seed=SEED)
    args.update(kw)
    return ClusterLoader(k["cd"], **args)


def test_setup_equals_the_restated_renumbering(case):
    cd = case["cd"]
    for got, want in zip((cd.node_perm, cd.node_inv, cd.partptr, cd.col_ptrs, cd.row_indices, cd.perm), case["host"]):
        assert np.array_equal(got.cpu().numpy(), want)
    assert len(cd) == P and cd.graph.n_major == N and cd.graph.n_edges == E and cd.graph.indices32 and cd.graph.ptrs32


def check_batch(k, mb, clusters):
    """one mini-batch against the restatement -> n_id"""
    node_perm, _, partptr, ptrs, indices, perm = k["host"]
    nodes, rows, cols, e, status = cluster_rule(partptr, clusters, ptrs, indices, node_ids=node_perm)
    assert status == 0
    n_id = mb.n_id.cpu().numpy()
    assert np.array_equal(n_id, nodes) and mb.num_nodes == nodes.size and len(set(n_id.tolist())) == n_id.size
    assert sorted(n_id.tolist()) == np.nonzero(np.isin(k["part"], clusters))[0].tolist()       # the union of the clusters
    assert np.array_equal(mb.edge_index.cpu().numpy(), np.stack([rows, cols])) and mb.num_edges == rows.size
    e_id = mb.e_id.cpu().numpy()
    assert np.array_equal(e_id, perm[e])
    assert np.array_equal(k["ei"][:, e_id], n_id[np.stack([rows, cols])])                       # row = source, col = target
    inside = np.isin(k["ei"][0], n_id) & np.isin(k["ei"][1], n_id)
    assert sorted(e_id.tolist()) == np.nonzero(inside)[0].tolist()                              # every edge between them
    assert np.array_equal(mb.x.cpu().numpy(), k["x"][n_id])
    assert np.array_equal(mb.edge_attr.cpu().numpy(), k["w"][e_id])
    assert mb.batch_size == Q and mb.layer_offsets is None and mb.layer_nodes is None
    return n_id


@pytest.mark.parametrize("drop_last", [False, True])
def test_epochs_cover_every_cluster_once(case, drop_last):
    k = case
    loader = build(k, drop_last=drop_last)
    assert len(loader) == (P // Q if drop_last else -(-P // Q))
    epochs = []
    for epoch in range(2):
        lists = epoch_lists(P, Q, SEED, epoch, drop_last=drop_last)
        sizes, seen = [], []
        for sb in loader.super_batches():
            sizes.append(len(sb))
            assert sb.num_nodes == sb.n_id.numel() and sb.num_edges == sb.edge_index.shape[1]
            for mb in sb:
                seen.append(check_batch(k, mb, lists[len(seen)]))
        assert sizes == ([4, 1] if drop_last else [4, 2]) and len(seen) == len(lists)
        named = np.concatenate(lists)
        assert len(set(named.tolist())) == named.size == (P // Q * Q if drop_last else P)       # every cluster at most once
        got = np.concatenate(seen)
        assert np.array_equal(np.sort(got), np.nonzero(np.isin(k["part"], named))[0])
        epochs.append(lists)
        if epoch == 0:
            assert loader.slab_allocations == 1
            slab_ptr = loader._pool[0]["lists"].data_ptr()
    assert any(a.tolist() != b.tolist() for a, b in zip(*epochs))       # the epochs differ under shuffle
    assert loader.slab_allocations == 1 and loader._pool[0]["lists"].data_ptr() == slab_ptr     # a second epoch allocates nothing


def test_shuffle_is_reproducible_and_can_be_switched_off(case):
    k = case
    a, b = build(k), build(k)
    for epoch in range(2):
        x, y = [mb.n_id for mb in a], [mb.n_id for mb in b]
        assert len(x) == len(y) == 6 and all(torch.equal(p, q) for p, q in zip(x, y))
    other = [mb.n_id for mb in build(k, seed=SEED + 1)]
    first = [mb.n_id for mb in build(k)]
    assert any(not torch.equal(p, q) for p, q in zip(first, other))
    plain = build(k, shuffle=False)
    for epoch in range(2):                                               # arange: every epoch the same lists
        for j, mb in enumerate(plain):
            check_batch(k, mb, list(range(j * Q, min(P, (j + 1) * Q))))


def test_prefetch_1_and_4_agree(case):
    k = case
    one, four = build(k, prefetch=1), build(k, prefetch=4)
    assert [len(sb) for sb in build(k, prefetch=1).super_batches()] == [1] * 6
    n = 0
    for p, q in zip(one, four):
        assert torch.equal(p.n_id, q.n_id) and torch.equal(p.edge_index, q.edge_index) and torch.equal(p.e_id, q.e_id)
        assert torch.equal(p.x, q.x) and torch.equal(p.edge_attr, q.edge_attr)
        n += 1
    assert n == 6


def test_two_live_iterators_own_a_slab_set_each(case):
    k = case
    loader = build(k)
    it1, it2 = iter(loader), iter(loader)                                # epochs 0 and 1
    a, b = next(it1), next(it2)
    assert loader.slab_allocations == 2
    check_batch(k, a, epoch_lists(P, Q, SEED, 0)[0])
    check_batch(k, b, epoch_lists(P, Q, SEED, 1)[0])
    rest1, rest2 = list(it1), list(it2)
    assert len(rest1) == len(rest2) == 5 and len(loader._pool) == 2
    check_batch(k, rest1[-1], epoch_lists(P, Q, SEED, 0)[-1])
    check_batch(k, rest2[-1], epoch_lists(P, Q, SEED, 1)[-1])
    list(loader)
    assert loader.slab_allocations == 2


def test_one_big_batch_is_the_whole_graph(case):
    k = case
    (mb,) = list(build(k, batch_size=P, shuffle=False))
    assert mb.num_nodes == N and mb.num_edges == E
    assert np.array_equal(mb.n_id.cpu().numpy(), k["host"][0])
