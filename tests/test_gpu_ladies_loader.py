"""LADIESLoader on a random multigraph: every mini-batch's blocks equal the chained restatement (helpers_ladies.blocks) for
one and two layers under call id j * L + l, edge_weight as bits, data.edge_index[:, e_id] == n_id[edge_index], attributes
follow; prefetch 1 and 4 agree, two epochs draw afresh, two live iterators, weight_attr with and without row_normalize (the
sums against float64 NumPy), and the growth path is taken once under a hub."""
import numpy as np
import pytest
import torch

from helpers_ladies import blocks, chunks_of, columns

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, E, B = 500, 6000, 64
SAMPLES = [48, 32]


@pytest.fixture(scope="module")
def case():
    from tch_geometric.transforms import Graph
    rs = np.random.default_rng(3)
    ei = rs.integers(0, N, (2, E)).astype(np.int64)
    ei[:, :40] = ei[:, 40:80]                                            # parallel edges
    ei[1, 80:120] = ei[0, 80:120]                                        # self loops
    ei[1, ei[1] >= N - 20] = 7                                           # twenty nodes without in-edges
    x = rs.standard_normal((N, 3)).astype(np.float32)
    w = (rs.random(E) * 1.2).astype(np.float32)                          # some above 1
    w[::11] = 0.0
    data = Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=N, x=torch.from_numpy(x).to(DEV),
                 lap=torch.from_numpy(w).to(DEV))
    inputs = rs.permutation(N)[:300].astype(np.int64)                    # 4 full mini-batches and one of 44
    return dict(data=data, ei=ei, x=x, w=w, inputs=inputs, ref={})


def build(k, **kw):
    from tch_geometric.loader import LADIESLoader
    args = dict(num_samples=SAMPLES, input_nodes=torch.from_numpy(k["inputs"]), batch_size=B, prefetch=4, shuffle=False,
                seed=21, device=DEV)
    args.update(kw)
    return LADIESLoader(k["data"], **args)


def host_csc(k, loader):
    """the loader's CSC on the host, checked against the edge list: perm[e] is the edge of offset e"""
    ptrs, idx, perm = (t.cpu().numpy() for t in (loader.col_ptrs, loader.row_indices, loader.perm))
    assert np.array_equal(k["ei"][0][perm], idx) and np.array_equal(k["ei"][1][perm], np.repeat(np.arange(N), np.diff(ptrs)))
    weights = None if loader.weights is None else loader.weights.cpu().numpy()
    return ptrs, idx, perm, weights


def check_batch(k, csc, loader, mb, seeds, j):
    """mini-batch j of the run against the restatement (computed once per seed list, budgets, weights and call id)"""
    ptrs, idx, perm, weights = csc
    L = loader.n_layers
    key = (tuple(seeds.tolist()), tuple(loader.num_samples), loader.seed, j, loader.weight_attr, loader.row_normalize)
    if key not in k["ref"]:
        k["ref"][key] = blocks(ptrs, idx, weights, seeds, loader.num_samples, loader.seed, j * L)
    want = k["ref"][key]
    assert len(mb.blocks) == L and mb.batch_size == seeds.size and np.array_equal(mb.input_nodes.cpu().numpy(), seeds)
    assert mb.call_id == j * L
    for block, s, (n_id, n_dst, rows, cols, e, ew) in zip(reversed(mb.blocks), loader.num_samples, want):   # outermost first
        got = block.n_id.cpu().numpy()
        assert np.array_equal(got, n_id) and block.n_dst == n_dst and block.num_src_nodes == n_id.size
        assert len(set(got.tolist())) == got.size and got.size <= n_dst + s                  # bounded by the budget
        assert np.array_equal(block.edge_index.cpu().numpy(), np.stack([rows, cols])) and block.num_edges == rows.size
        assert np.array_equal(block.edge_weight.cpu().numpy().view(np.uint32), ew.view(np.uint32))
        e_id = block.e_id.cpu().numpy()
        assert np.array_equal(e_id, perm[e])
        assert np.array_equal(k["ei"][:, e_id], got[np.stack([rows, cols])])                 # row = source, col = destination
    inner, outer = mb.blocks[-1], mb.blocks[0]
    assert np.array_equal(inner.n_id.cpu().numpy()[:seeds.size], seeds)
    assert torch.equal(mb.n_id, outer.n_id) and mb.num_nodes == outer.n_id.numel()
    assert np.array_equal(mb.x.cpu().numpy(), k["x"][mb.n_id.cpu().numpy()])
    return want


@pytest.mark.parametrize("samples", [[48], SAMPLES], ids=["one-layer", "two-layers"])
def test_blocks_equal_the_restatement_over_two_epochs(case, samples):
    k = case
    loader = build(k, num_samples=samples)
    csc = host_csc(k, loader)
    assert len(loader) == 5
    firsts = []
    for epoch in range(2):                                               # no shuffle: the same lists, fresh call ids
        sizes, j = [], 0
        for sb in loader.super_batches():
            sizes.append(len(sb))
            assert len(sb.layers) == len(samples) and sb.n_id.numel() == sb.node_ptr[-1]
            for mb in sb:
                want = check_batch(k, csc, loader, mb, k["inputs"][j * B:(j + 1) * B], epoch * 5 + j)
                if j == 0:
                    firsts.append(want[0][0])
                j += 1
        assert sizes == [4, 1] and j == 5
    assert not np.array_equal(firsts[0], firsts[1])                      # the second epoch draws afresh
    assert loader.growths <= len(samples)


def test_prefetch_1_and_4_agree(case):
    k = case
    assert [len(sb) for sb in build(k, prefetch=1).super_batches()] == [1] * 5
    n = 0
    for p, q in zip(build(k, prefetch=1), build(k, prefetch=4)):
        assert torch.equal(p.n_id, q.n_id) and torch.equal(p.x, q.x) and p.call_id == q.call_id
        for s, t in zip(p.blocks, q.blocks):
            assert torch.equal(s.n_id, t.n_id) and torch.equal(s.edge_index, t.edge_index) and torch.equal(s.e_id, t.e_id)
            assert torch.equal(s.edge_weight.view(torch.int32), t.edge_weight.view(torch.int32)) and s.n_dst == t.n_dst
        n += 1
    assert n == 5


def test_two_live_iterators_and_shuffle(case):
    k = case
    loader = build(k, shuffle=True, seed=2)
    csc = host_csc(k, loader)
    it1, it2 = iter(loader), iter(loader)                                # epochs 0 and 1
    a, b = next(it1), next(it2)
    rest1, rest2 = list(it1), list(it2)
    assert len(rest1) == len(rest2) == 4
    for mb, j in ((a, 0), (b, 5), (rest1[-1], 4), (rest2[-1], 9)):       # what one iterator holds survives the other's launches
        check_batch(k, csc, loader, mb, mb.input_nodes.cpu().numpy(), j)
    assert not torch.equal(a.input_nodes, b.input_nodes)
    assert sorted(torch.cat([a.input_nodes] + [m.input_nodes for m in rest1]).tolist()) == sorted(k["inputs"].tolist())


@pytest.mark.parametrize("row_normalize", [False, True])
def test_weight_attr(case, row_normalize):
    k = case
    loader = build(k, weight_attr="lap", row_normalize=row_normalize)
    csc = host_csc(k, loader)
    ptrs, idx, perm, weights = csc
    w_csc = k["w"][perm].astype(np.float64)
    if row_normalize:
        col = np.repeat(np.arange(N), np.diff(ptrs))
        sums = np.zeros(N)
        np.add.at(sums, col, w_csc)                                      # float64: non-negative sums of at most 2^31 terms
        got = loader.col_sum.cpu().numpy()
        assert np.allclose(got, sums, rtol=1e-9, atol=0)
        # the weights the kernel reads: float32 of the float64 quotient by the loader's own sums, 0 where the sum is 0
        with np.errstate(invalid="ignore", divide="ignore"):
            exp = np.where(got[col] > 0, w_csc / got[col], 0.0).astype(np.float32)
        assert np.array_equal(weights.view(np.uint32), exp.view(np.uint32))
        assert np.allclose(np.bincount(col, weights=weights.astype(np.float64), minlength=N)[sums > 0], 1.0, rtol=1e-5)
    else:
        assert loader.col_sum is None and np.array_equal(weights, k["w"][perm])
    for j, mb in enumerate(loader):
        check_batch(k, csc, loader, mb, k["inputs"][j * B:(j + 1) * B], j)
    assert j == 4


def test_growth_path_is_taken_once():
    from tch_geometric.loader import LADIESLoader
    from tch_geometric.transforms import Graph
    rs = np.random.default_rng(8)
    n, hub = 3000, 5
    src = np.concatenate([rs.integers(0, n, 2500), rs.integers(0, n, 9000)])
    dst = np.concatenate([np.full(2500, hub), rs.integers(0, n, 9000)])
    order = rs.permutation(src.size)
    ei = np.stack([src[order], dst[order]]).astype(np.int64)
    data = Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=n)
    seeds = np.concatenate([[hub], np.arange(100, 163)]).astype(np.int64)                  # 64 seeds under a hub
    loader = LADIESLoader(data, [256], input_nodes=torch.from_numpy(seeds), batch_size=64, shuffle=False, seed=4, device=DEV)
    ptrs, idx = loader.col_ptrs.cpu().numpy(), loader.row_indices.cpu().numpy()
    m, chunks = int(columns(ptrs, seeds)[1].sum()), chunks_of(ptrs, seeds)
    loader._node_cap, loader._chunk_cap = [64], [1]                                        # below the need on both counts
    assert 64 + m > 2500 and chunks > 5
    for epoch in range(2):
        (mb,) = list(loader)
        assert loader.growths == 1                                                        # grown once, kept afterwards
        need = 64 + m                                                                     # the exact counts plus a quarter
        assert loader._node_cap == [need + need // 4] and loader._chunk_cap == [chunks + chunks // 4]
        (n_id, n_dst, rows, cols, e, ew), = blocks(ptrs, idx, None, seeds, [256], 4, epoch)
        assert np.array_equal(mb.n_id.cpu().numpy(), n_id)
        assert np.array_equal(mb.blocks[0].edge_index.cpu().numpy(), np.stack([rows, cols]))
        assert np.array_equal(mb.blocks[0].edge_weight.cpu().numpy().view(np.uint32), ew.view(np.uint32))
        assert np.array_equal(ei[:, mb.blocks[0].e_id.cpu().numpy()], n_id[np.stack([rows, cols])])
