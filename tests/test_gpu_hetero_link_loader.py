"""HeteroLinkNeighborLoader on the GPU: every mini-batch is tg_ns_hetero_batched (and tg_ns_typed_unique) run alone on the
two seed rows the CPU model of tests/helpers_link_typed.py makes at that call id, and its link fields, numbered against the
per-type n_id, name the model's global pairs.  The fake hetero fixture with an x per type; the labelled relation is
(v0, e0, v2) -- two node types, 897 and 982 nodes -- or (v0, e0, v0)."""
import numpy as np
import pytest
import torch

import helpers_link_typed as ht
import orc
from helpers import load_fake_hetero, rel_key

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEED, CALL0, TRIES, PREFETCH, N = 21, 500, 4, 3, 203
RELS = {"two-types": ("v0", "e0", "v2"), "one-type": ("v0", "e0", "v0")}


@pytest.fixture(scope="module")
def fake():
    """-> (HeteroGraph with x per type, {name: (edge type, edge_label_index [2, N] of its edges)})"""
    from tch_geometric.transforms import HeteroGraph
    counts, edges = load_fake_hetero()
    data = HeteroGraph()
    for nt, n in counts.items():
        data[nt].num_nodes = n
        data[nt].x = torch.arange(n, dtype=torch.float32, device=DEV).view(-1, 1).repeat(1, 3)
    for et, ei in edges.items():
        data[et].edge_index = torch.from_numpy(ei).to(DEV)
    labelled = {}
    for k, (name, et) in enumerate(RELS.items()):
        pick = np.random.default_rng(4 + k).permutation(edges[et].shape[1])[:N]
        labelled[name] = (et, torch.from_numpy(edges[et][:, pick]))
    return data, labelled


def make(fake, name, fanout, batch, **kw):
    from tch_geometric.loader import HeteroLinkNeighborLoader
    data, labelled = fake
    kw.setdefault("neg_sampling_ratio", 2)
    kw.setdefault("try_count", TRIES)
    return HeteroLinkNeighborLoader(data, fanout, labelled[name], batch_size=batch, prefetch=PREFETCH, seed=SEED,
                                    call_id0=CALL0, device=DEV, **kw)


_host = {}


def host_csc(loader):
    """every relation's CSC as the loader ingested it, on the host"""
    if not _host:
        _host["P"] = {k: v.cpu().numpy() for k, v in loader.col_ptrs.items()}
        _host["I"] = {k: v.cpu().numpy() for k, v in loader.row_indices.items()}
    return _host["P"], _host["I"]


def model_rows(loader, positions, call_id):
    P, I = host_csc(loader)
    k = rel_key(loader.edge_type)
    eli = loader.edge_label_index.cpu().numpy()
    return ht.seed_rows(P[k], I[k], eli[0][positions][None], eli[1][positions][None], loader.K, loader.mode,
                        loader.try_count, loader.seed, call_id, loader.n_src, loader.n_dst, loader.same_type)


def inputs_of(loader, srow, drow):
    """the model's rows as per-type inputs: one joined row when both endpoints are one type"""
    A, B = loader.edge_type[0], loader.edge_type[2]
    return {A: np.concatenate([srow, drow])} if A == B else {A: srow, B: drow}


def reference(loader, srow, drow, call_id):
    """({type: n_id}, {relation: edge_index}, {type: unique seeds or None}) of the sampler (and the dedup under unique) run
    alone on the model's rows as inputs of the two types at this call id"""
    from tch_geometric import _cabi
    ins = inputs_of(loader, srow, drow)
    inputs = [torch.from_numpy(ins[t][None]).to(DEV) if t in ins else None for t in loader.node_types]
    hb = _cabi.NsHeteroBatched(len(loader.node_types), loader._rels, inputs, len(loader.fanout), 1, DEV, sampler=loader.sampler)
    hb.run(loader.seed, call_id)
    res, seed_counts = hb, None
    if loader.unique:
        res = _cabi.ns_typed_unique(hb, 1, loader._id_bounds, in_place=True)
        seed_counts = res.seed_counts.cpu().numpy()[0]
    torch.cuda.synchronize()
    c = res.counts.cpu().numpy()[0]
    T = len(loader.node_types)
    n_id = {t: res.samples[i][0, :c[i]].cpu().numpy() for i, t in enumerate(loader.node_types)}
    ei = {et: np.stack([res.rows[r][0, :c[T + r]].cpu().numpy(), res.cols[r][0, :c[T + r]].cpu().numpy()])
          for r, et in enumerate(loader.edge_types)}
    return n_id, ei, None if seed_counts is None else {t: int(seed_counts[i]) for i, t in enumerate(loader.node_types)}


def check_mini_batch(loader, g, positions, call_id):
    """-> the model's (src row, dst row); asserts everything a mini-batch promises"""
    et = loader.edge_type
    A, B = et[0], et[2]
    E, K, mode = positions.size, loader.K, loader.mode
    srows, drows, unv = model_rows(loader, positions, call_id)
    Ws, Wd = ht.widths(E, K, mode)
    assert g.call_id == call_id
    assert np.array_equal(g[et].input_id.cpu().numpy(), positions)
    assert int(g.neg_unverified) == unv[0] and g.neg_unverified.is_cuda and g.neg_unverified.dim() == 0
    n_id, edge_index, seed_counts = reference(loader, srows[0], drows[0], call_id)
    got = {t: g[t].n_id.cpu().numpy() for t in loader.node_types}
    for t in loader.node_types:
        assert np.array_equal(got[t], n_id[t]), t
        assert g[t].num_nodes == n_id[t].size
        assert np.array_equal(g[t].x.cpu().numpy()[:, 0], got[t].astype(np.float32)) and g[t].x.shape == (got[t].size, 3)
        if loader.unique:
            assert np.unique(got[t]).size == got[t].size
    for r in loader.edge_types:
        assert np.array_equal(g[r].edge_index.cpu().numpy(), edge_index[r]), r
    ins = inputs_of(loader, srows[0], drows[0])
    for t, row in ins.items():                                   # the seeds of a type lead its n_id
        if loader.unique:
            first = row[np.sort(np.unique(row, return_index=True)[1])]
            assert g[t].batch_size == seed_counts[t] == first.size and np.array_equal(got[t][:first.size], first)
        else:
            assert g[t].batch_size == row.size and np.array_equal(got[t][:row.size], row)
    pairs = ht.pairs(srows, drows, E, K, mode)[0]
    P = pairs.shape[1]
    if mode == ht.BINARY:
        local = g[et].edge_label_index.cpu().numpy()
        assert local.shape == (2, P) and g[et].edge_label_index.dtype == torch.int64
        assert np.array_equal(got[A][local[0]], pairs[0]) and np.array_equal(got[B][local[1]], pairs[1])
        assert g[et].edge_label.dtype == torch.float32
        assert np.array_equal(g[et].edge_label.cpu().numpy(), np.r_[np.ones(E), np.zeros(P - E)].astype(np.float32))
    else:
        assert not hasattr(g[et], "edge_label_index") and g[B].dst_neg_index.shape == (E, K)
        assert np.array_equal(got[A][g[A].src_index.cpu().numpy()], pairs[0, :E])
        assert np.array_equal(got[B][g[B].dst_pos_index.cpu().numpy()], pairs[1, :E])
        assert np.array_equal(got[B][g[B].dst_neg_index.cpu().numpy()], pairs[1, E:].reshape(E, K))
    return srows[0], drows[0]


@pytest.mark.parametrize("mode", ["binary", "triplet"])
@pytest.mark.parametrize("unique", [False, True], ids=["forest", "unique"])
@pytest.mark.parametrize("batch", [5, 64])
@pytest.mark.parametrize("fanout", [[3, 2], []], ids=["3-2", "seeds-only"])
@pytest.mark.parametrize("name", list(RELS))
def test_mini_batches_equal_the_composition(fake, name, fanout, batch, unique, mode):
    assert N % batch != 0
    loader = make(fake, name, fanout, batch, unique=unique, neg_sampling=mode)
    assert len(loader) == -(-N // batch) and loader.same_type == (name == "one-type")
    duplicates = 0
    mbs = list(loader)
    assert len(mbs) == len(loader)
    for j, g in enumerate(mbs):
        positions = np.arange(j * batch, min((j + 1) * batch, N))
        for row in check_mini_batch(loader, g, positions, CALL0 + j):
            duplicates += np.unique(row).size < row.size
        if not fanout:                                            # the seeds alone: no relation holds an edge
            assert all(g[r].edge_index.shape == (2, 0) for r in loader.edge_types)
    assert mbs[-1][loader.edge_type].input_id.numel() == N % batch   # the ragged last mini-batch: other widths
    if batch == 64:                                               # 64 edges' ends and 128 draws among fewer than 1 000 nodes:
        assert duplicates > 0                                     # seed rows with repeated endpoints were covered


def test_against_the_oracle(fake):
    """the sampler-independent check: the CPU oracle in Philox mode on the model's rows as inputs of two types"""
    loader = make(fake, "two-types", [3, 2], 64)
    P, I = host_csc(loader)
    nn = {rel_key(r): [3, 2] for r in loader.edge_types}
    A, B = loader.edge_type[0], loader.edge_type[2]
    for j, g in enumerate(loader):
        positions = np.arange(j * 64, min((j + 1) * 64, N))
        srows, drows, _ = model_rows(loader, positions, CALL0 + j)
        s, r, c, e, lo = orc.ns_hetero(loader.node_types, loader.edge_types, P, I, {A: srows[0], B: drows[0]}, nn, 2,
                                       orc.rng_philox(SEED, CALL0 + j))
        for t in loader.node_types:
            assert np.array_equal(g[t].n_id.cpu().numpy(), s[t]), (j, t)
        for et in loader.edge_types:
            k = rel_key(et)
            assert np.array_equal(g[et].edge_index.cpu().numpy(), np.stack([r[k], c[k]])), (j, et)
            assert g[et].layer_offsets == lo[k], (j, et)


@pytest.mark.parametrize("name", list(RELS))
def test_drop_last_and_edge_set(fake, name):
    loader = make(fake, name, [3, 2], 64, drop_last=True, edge_set=True, unique=True)
    assert loader._edge_set is not None and len(loader) == N // 64
    mbs = list(loader)
    assert len(mbs) == N // 64
    for j, g in enumerate(mbs):
        check_mini_batch(loader, g, np.arange(j * 64, (j + 1) * 64), CALL0 + j)


def test_shuffle_hands_out_the_permutation_and_reproduces(fake):
    a, b = (make(fake, "two-types", [3, 2], 64, shuffle=True) for _ in range(2))
    et = a.edge_type
    perms = []
    for epoch in range(2):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(SEED * 1000003 + epoch)
        perm = torch.randperm(N, device=DEV, generator=gen).cpu().numpy()
        perms.append(perm)
        seen = []
        for j, (ga, gb) in enumerate(zip(a, b)):
            check_mini_batch(a, ga, perm[j * 64:(j + 1) * 64], CALL0 + epoch * len(a) + j)
            seen.append(ga[et].input_id.cpu().numpy())
            assert torch.equal(ga[et].input_id, gb[et].input_id) and torch.equal(ga[et].edge_label_index, gb[et].edge_label_index)
            for t in a.node_types:
                assert torch.equal(ga[t].n_id, gb[t].n_id)
        assert np.array_equal(np.concatenate(seen), perm)
    assert not np.array_equal(perms[0], perms[1]) and sorted(perms[0]) == list(range(N))


@pytest.mark.parametrize("mode", ["binary", "triplet"])
def test_labels_pass_through_without_negatives(fake, mode):
    labels = torch.arange(N, dtype=torch.float32) * 0.5
    loader = make(fake, "two-types", [3, 2], 64, neg_sampling_ratio=0, edge_label=labels, shuffle=True, neg_sampling=mode)
    et, eli = loader.edge_type, loader.edge_label_index
    for g in loader:
        ids = g[et].input_id
        assert torch.equal(g[et].edge_label.cpu(), labels[ids.cpu()]) and int(g.neg_unverified) == 0
        if mode == "binary":
            local = g[et].edge_label_index
            assert torch.equal(g["v0"].n_id[local[0]], eli[0, ids]) and torch.equal(g["v2"].n_id[local[1]], eli[1, ids])
        else:
            assert torch.equal(g["v0"].n_id[g["v0"].src_index], eli[0, ids]) and g["v2"].dst_neg_index.shape == (ids.numel(), 0)


def test_the_relation_itself_is_the_default_and_epochs_draw_afresh(fake):
    from tch_geometric.loader import HeteroLinkNeighborLoader
    data, _ = fake
    et = RELS["two-types"]
    kw = dict(batch_size=64, prefetch=2, seed=SEED, call_id0=CALL0, device=DEV, drop_last=True)
    bare, none = HeteroLinkNeighborLoader(data, [2], et, **kw), HeteroLinkNeighborLoader(data, [2], (et, None), **kw)
    assert torch.equal(bare.edge_label_index, data[et].edge_index) and torch.equal(none.edge_label_index, data[et].edge_index)
    n = len(bare)
    first = [g for g, _ in zip(bare, range(2))]
    second = [g for g, _ in zip(bare, range(2))]
    assert [g.call_id for g in first] == [CALL0, CALL0 + 1] and [g.call_id for g in second] == [CALL0 + n, CALL0 + n + 1]
    for g1, g2 in zip(first, second):
        assert torch.equal(g1[et].input_id, g2[et].input_id)          # the same positives ...
        p1 = g1["v2"].n_id[g1[et].edge_label_index[1]]
        p2 = g2["v2"].n_id[g2[et].edge_label_index[1]]
        assert torch.equal(p1[:64], p2[:64]) and not torch.equal(p1[64:], p2[64:])   # ... with fresh negatives


def test_refusals(fake):
    from tch_geometric.loader import HeteroLinkNeighborLoader
    from tch_geometric.transforms import Graph
    data, labelled = fake
    et, eli = labelled["two-types"]
    with pytest.raises(ValueError, match="LinkNeighborLoader"):
        HeteroLinkNeighborLoader(Graph(edge_index=eli.to(DEV), num_nodes=1000), [3], (et, eli), device=DEV)
    with pytest.raises(ValueError):
        HeteroLinkNeighborLoader(data, [3], (("v0", "e9", "v2"), eli), device=DEV)
    with pytest.raises(ValueError):
        HeteroLinkNeighborLoader(data, [3], (et, eli.t().contiguous()), device=DEV)
    with pytest.raises(ValueError):
        HeteroLinkNeighborLoader(data, [3], (et, eli), edge_label=torch.ones(N), neg_sampling_ratio=1, device=DEV)
    with pytest.raises(ValueError):
        HeteroLinkNeighborLoader(data, [3], (et, eli), edge_label=torch.ones(N - 1), neg_sampling_ratio=0, device=DEV)
    with pytest.raises(ValueError):
        HeteroLinkNeighborLoader(data, [3], (et, eli), neg_sampling="structured", device=DEV)
    with pytest.raises(ValueError):
        HeteroLinkNeighborLoader(data, [3], (et, eli), neg_sampling_ratio=-1, device=DEV)
    with pytest.raises(ValueError):
        HeteroLinkNeighborLoader(data, [3], (et, eli), try_count=0, device=DEV)
    for row, bad in ((0, 897), (1, 982), (0, -1), (1, -1)):      # v0 has 897 nodes, v2 has 982: 900 is a v2 but no v0
        wrong = eli.clone()
        wrong[row, 7] = bad
        with pytest.raises(IndexError):                           # at construction: nothing was launched with it
            HeteroLinkNeighborLoader(data, [3], (et, wrong), device=DEV)
    ok = eli.clone()
    ok[1, 7] = 981
    HeteroLinkNeighborLoader(data, [3], (et, ok), device=DEV)


def test_package_exports_the_loader():
    import tch_geometric
    from tch_geometric.loader import HeteroLinkNeighborLoader, HeteroNeighborLoader
    assert tch_geometric.HeteroLinkNeighborLoader is HeteroLinkNeighborLoader
    assert issubclass(HeteroLinkNeighborLoader, HeteroNeighborLoader)
    assert HeteroLinkNeighborLoader.WITH_INVERSE and not HeteroNeighborLoader.WITH_INVERSE
