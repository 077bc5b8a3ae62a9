"""FullNeighborLoader on a random multigraph: every mini-batch's blocks equal the chained restatement (helpers_full.blocks)
for one and two layers, data.edge_index[:, e_id] == n_id[edge_index], every seed has its whole in-degree, attributes follow;
every input node once per epoch with and without drop_last, shuffling repeats from (seed, epoch), prefetch 1 and 4 agree,
two live iterators, the growth path is taken once, and on a graph of in-degree <= 32 every mini-batch holds what
NeighborLoader(num_neighbors=[32], unique=True) holds."""
import numpy as np
import pytest
import torch

from helpers_full import blocks, chunks_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, E, B = 500, 6000, 64


@pytest.fixture(scope="module")
def case():
    from tch_geometric.transforms import Graph
    rs = np.random.default_rng(3)
    ei = rs.integers(0, N, (2, E)).astype(np.int64)
    ei[:, :40] = ei[:, 40:80]                                            # parallel edges
    ei[1, 80:120] = ei[0, 80:120]                                        # self loops
    ei[1, ei[1] >= N - 20] = 7                                           # twenty nodes without in-edges
    x = rs.standard_normal((N, 3)).astype(np.float32)
    data = Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=N, x=torch.from_numpy(x).to(DEV))
    inputs = rs.permutation(N)[:300].astype(np.int64)                    # 4 full mini-batches and one of 44
    return dict(data=data, ei=ei, x=x, inputs=inputs, deg=np.bincount(ei[1], minlength=N), ref={})


def build(k, **kw):
    from tch_geometric.loader import FullNeighborLoader
    args = dict(num_layers=2, input_nodes=torch.from_numpy(k["inputs"]), batch_size=B, prefetch=4, device=DEV)
    args.update(kw)
    return FullNeighborLoader(k["data"], **args)


def host_csc(k, loader):
    """the loader's CSC on the host, checked against the edge list: perm[e] is the edge of offset e"""
    ptrs, idx, perm = (t.cpu().numpy() for t in (loader.col_ptrs, loader.row_indices, loader.perm))
    assert np.array_equal(k["ei"][0][perm], idx) and np.array_equal(k["ei"][1][perm], np.repeat(np.arange(N), np.diff(ptrs)))
    assert sorted(perm.tolist()) == list(range(E))
    return ptrs, idx, perm


def check_batch(k, csc, mb, seeds, L):
    """one mini-batch against the restatement (computed once per seed list and depth)"""
    ptrs, idx, perm = csc
    key = (tuple(seeds.tolist()), L)
    if key not in k["ref"]:
        k["ref"][key] = blocks(ptrs, idx, seeds, L)
    want = k["ref"][key]
    assert len(mb.blocks) == L and mb.batch_size == seeds.size and np.array_equal(mb.input_nodes.cpu().numpy(), seeds)
    for block, (n_id, n_dst, rows, cols, e) in zip(reversed(mb.blocks), want):          # blocks come outermost first
        got = block.n_id.cpu().numpy()
        assert np.array_equal(got, n_id) and block.n_dst == n_dst and block.num_src_nodes == n_id.size
        assert len(set(got.tolist())) == got.size
        assert np.array_equal(block.edge_index.cpu().numpy(), np.stack([rows, cols])) and block.num_edges == rows.size
        e_id = block.e_id.cpu().numpy()
        assert np.array_equal(e_id, perm[e])
        assert np.array_equal(k["ei"][:, e_id], got[np.stack([rows, cols])])            # row = source, col = destination
        assert np.array_equal(np.bincount(cols, minlength=n_dst), k["deg"][got[:n_dst]])    # the whole in-degree
    inner, outer = mb.blocks[-1], mb.blocks[0]
    assert np.array_equal(inner.n_id.cpu().numpy()[:seeds.size], seeds)
    assert torch.equal(mb.n_id, outer.n_id) and mb.num_nodes == outer.n_id.numel()
    assert np.array_equal(mb.x.cpu().numpy(), k["x"][mb.n_id.cpu().numpy()])


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("drop_last", [False, True])
def test_blocks_equal_the_restatement_and_cover_the_inputs(case, L, drop_last):
    k = case
    loader = build(k, num_layers=L, drop_last=drop_last)
    csc = host_csc(k, loader)
    assert len(loader) == (4 if drop_last else 5)
    for epoch in range(2):                                               # no shuffle: every epoch the same lists
        sizes, seen = [], []
        for sb in loader.super_batches():
            sizes.append(len(sb))
            assert len(sb.layers) == L and sb.n_id.numel() == sb.node_ptr[-1]
            for mb in sb:
                j = len(seen)
                check_batch(k, csc, mb, k["inputs"][j * B:(j + 1) * B], L)
                seen.append(mb.input_nodes.cpu().numpy())
        assert sizes == ([4] if drop_last else [4, 1])
        assert np.array_equal(np.concatenate(seen), k["inputs"][:256 if drop_last else 300])   # every input node once
    assert loader.growths <= L                                           # at most one growth per layer, then kept


def test_all_nodes_by_default(case):
    loader = build(case, num_layers=1, input_nodes=None, batch_size=200)
    csc = host_csc(case, loader)
    got = list(loader)
    assert [mb.batch_size for mb in got] == [200, 200, 100]
    check_batch(case, csc, got[2], np.arange(400, 500), 1)               # the nodes without in-edges are among them
    assert sum(mb.blocks[0].num_edges for mb in got) == E


def test_shuffle_is_a_function_of_seed_and_epoch(case):
    k = case
    a, b = build(k, shuffle=True, seed=5), build(k, shuffle=True, seed=5)
    epochs = []
    for epoch in range(2):
        x, y = [mb.input_nodes for mb in a], [mb.input_nodes for mb in b]
        assert len(x) == len(y) == 5 and all(torch.equal(p, q) for p, q in zip(x, y))
        assert sorted(torch.cat(x).tolist()) == sorted(k["inputs"].tolist())
        epochs.append(torch.cat(x))
    assert not torch.equal(epochs[0], epochs[1])
    other = torch.cat([mb.input_nodes for mb in build(k, shuffle=True, seed=6)])
    assert not torch.equal(other, epochs[0])
    csc = host_csc(k, a)
    mb = next(iter(a))                                                   # a shuffled mini-batch is still the restatement
    check_batch(k, csc, mb, mb.input_nodes.cpu().numpy(), 2)


def test_prefetch_1_and_4_agree(case):
    k = case
    assert [len(sb) for sb in build(k, prefetch=1).super_batches()] == [1] * 5
    n = 0
    for p, q in zip(build(k, prefetch=1), build(k, prefetch=4)):
        assert torch.equal(p.n_id, q.n_id) and torch.equal(p.x, q.x)
        for s, t in zip(p.blocks, q.blocks):
            assert torch.equal(s.n_id, t.n_id) and torch.equal(s.edge_index, t.edge_index) and torch.equal(s.e_id, t.e_id)
            assert s.n_dst == t.n_dst
        n += 1
    assert n == 5


def test_two_live_iterators(case):
    k = case
    loader = build(k, shuffle=True, seed=2)
    csc = host_csc(k, loader)
    it1, it2 = iter(loader), iter(loader)                                # epochs 0 and 1
    a, b = next(it1), next(it2)
    rest1, rest2 = list(it1), list(it2)
    assert len(rest1) == len(rest2) == 4
    for mb in [a, b, rest1[-1], rest2[-1]]:                              # what one iterator holds survives the other's launches
        check_batch(k, csc, mb, mb.input_nodes.cpu().numpy(), 2)
    assert not torch.equal(a.input_nodes, b.input_nodes)


def test_growth_path_is_taken_once():
    from tch_geometric.loader import FullNeighborLoader
    from tch_geometric.transforms import Graph
    rs = np.random.default_rng(8)
    n, hub = 3000, 5
    src = np.concatenate([rs.integers(0, n, 2500), rs.integers(0, n, 9000)])
    dst = np.concatenate([np.full(2500, hub), rs.integers(0, n, 9000)])
    order = rs.permutation(src.size)
    ei = np.stack([src[order], dst[order]]).astype(np.int64)
    data = Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=n)
    seeds = np.concatenate([[hub], np.arange(100, 163)]).astype(np.int64)                  # 64 seeds under a hub
    loader = FullNeighborLoader(data, 1, input_nodes=torch.from_numpy(seeds), batch_size=64, device=DEV)
    ptrs, idx = loader.col_ptrs.cpu().numpy(), loader.row_indices.cpu().numpy()
    (n_id, n_dst, rows, cols, e), = blocks(ptrs, idx, seeds, 1)
    loader._node_cap, loader._chunk_cap = [64], [1]                                        # below the need on both counts
    assert 64 + rows.size > 2500 and chunks_of(ptrs, seeds) > 5
    for epoch in range(2):
        (mb,) = list(loader)
        assert loader.growths == 1                                                        # grown once, kept afterwards
        need, chunks = 64 + rows.size, chunks_of(ptrs, seeds)                             # the exact counts plus a quarter
        assert loader._node_cap == [need + need // 4] and loader._chunk_cap == [chunks + chunks // 4]
        assert np.array_equal(mb.n_id.cpu().numpy(), n_id)
        assert np.array_equal(mb.blocks[0].edge_index.cpu().numpy(), np.stack([rows, cols]))
        assert np.array_equal(ei[:, mb.blocks[0].e_id.cpu().numpy()], n_id[np.stack([rows, cols])])


def test_equals_neighbor_loader_where_the_fan_out_covers_every_column():
    from tch_geometric.loader import FullNeighborLoader, NeighborLoader
    from tch_geometric.transforms import Graph
    rs = np.random.default_rng(4)
    n = 400
    deg = rs.integers(0, 33, n)                                          # in-degrees 0 .. 32
    dst = np.repeat(np.arange(n), deg)
    src = rs.integers(0, n, dst.size)
    order = rs.permutation(dst.size)
    ei = np.stack([src[order], dst[order]]).astype(np.int64)
    assert np.bincount(ei[1], minlength=n).max() == 32
    data = Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=n)
    inputs = torch.from_numpy(rs.permutation(n)[:150].astype(np.int64))
    full = FullNeighborLoader(data, 1, input_nodes=inputs, batch_size=64, prefetch=2, device=DEV)
    sampled = NeighborLoader(data, [32], input_nodes=inputs, batch_size=64, prefetch=2, unique=True, device=DEV)
    count = 0
    for f, s in zip(full, sampled):                                      # without replacement and k >= degree: every neighbour
        block = f.blocks[0]
        f_id, s_id = block.n_id.cpu().numpy(), s.n_id.cpu().numpy()
        assert set(f_id.tolist()) == set(s_id.tolist()) and f_id.size == s_id.size
        fr, fc = block.edge_index.cpu().numpy()
        sr, sc = s.edge_index.cpu().numpy()
        mine = set(zip(f_id[fr].tolist(), f_id[fc].tolist(), block.e_id.cpu().tolist()))
        theirs = set(zip(s_id[sr].tolist(), s_id[sc].tolist(), s.e_id.cpu().tolist()))
        assert mine == theirs and len(mine) == fr.size == sr.size
        count += 1
    assert count == 3
