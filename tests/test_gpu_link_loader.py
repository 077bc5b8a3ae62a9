"""LinkNeighborLoader on the GPU: every mini-batch is the sampler (and the dedup) run on the seed row the CPU model of
tests/helpers_link.py makes at that call id, and its link fields, numbered against n_id, name the model's global pairs."""
import numpy as np
import pytest
import torch

import helpers_link as hl
import orc
from helpers import load_karate

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEED, CALL0, TRIES, PREFETCH = 21, 500, 4, 3


@pytest.fixture(scope="module")
def datasets():
    """name -> (Graph, edge_label_index or None, N): karate's own 156 edges; 203 of RMAT-10's 16 K edges"""
    from tch_geometric.transforms import Graph
    ei, n = load_karate()
    x = np.arange(n * 3, dtype=np.float32).reshape(n, 3)
    karate = Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=n, x=torch.from_numpy(x).to(DEV))
    n2 = 1 << 10
    row, col = orc.rmat_edges(10, n2 * 16, 99)
    rmat = Graph(edge_index=torch.from_numpy(np.stack([row, col])).to(DEV), num_nodes=n2)
    pick = np.random.default_rng(4).permutation(row.size)[:203]
    return {"karate": (karate, None, ei.shape[1]), "rmat": (rmat, torch.from_numpy(np.stack([row, col])[:, pick]), 203)}


def make(datasets, name, fanout, batch, **kw):
    from tch_geometric.loader import LinkNeighborLoader
    data, eli, _ = datasets[name]
    kw.setdefault("neg_sampling_ratio", 2)
    return LinkNeighborLoader(data, fanout, edge_label_index=eli, try_count=TRIES, batch_size=batch, prefetch=PREFETCH,
                              seed=SEED, call_id0=CALL0, device=DEV, **kw)


_csc = {}


def host_csc(loader, name):
    if name not in _csc:
        _csc[name] = (loader.col_ptrs.cpu().numpy(), loader.row_indices.cpu().numpy())
    return _csc[name]


def reference(loader, row, call_id):
    """(n_id, edge_index) of the sampler (and the dedup under unique) run alone on one seed row at this call id"""
    from tch_geometric import _cabi
    seeds = torch.from_numpy(row[None]).to(DEV)
    out = _cabi.NsBatchedOut(1, row.size, loader.fanout, DEV)
    _cabi.ns_homo_batched(loader._graph, seeds, loader.fanout, loader.seed, call_id, out, sampler=loader.sampler)
    res = _cabi.ns_homo_unique(out, 1, loader.n_nodes) if loader.unique else out
    torch.cuda.synchronize()
    s, r, c, _, _ = res.batch(0)
    return s.cpu().numpy(), np.stack([r.cpu().numpy(), c.cpu().numpy()])


def check_mini_batch(loader, name, mb, positions, call_id):
    """-> the model's seed row; asserts everything a mini-batch promises"""
    ptrs, idx = host_csc(loader, name)
    eli = loader.edge_label_index.cpu().numpy()
    src, dst = eli[0][positions][None], eli[1][positions][None]
    E, K, mode = positions.size, loader.K, loader.mode
    rows, unv = hl.seed_rows(ptrs, idx, src, dst, K, mode, loader.try_count, loader.seed, call_id, loader.n_nodes)
    assert mb.call_id == call_id and mb.batch_size == E
    assert np.array_equal(mb.input_id.cpu().numpy(), positions)
    assert int(mb.neg_unverified) == unv[0] and mb.neg_unverified.is_cuda and mb.neg_unverified.dim() == 0
    n_id, edge_index = reference(loader, rows[0], call_id)
    got = mb.n_id.cpu().numpy()
    assert np.array_equal(got, n_id) and np.array_equal(mb.edge_index.cpu().numpy(), edge_index)
    assert mb.num_nodes == n_id.size and mb.num_edges == edge_index.shape[1]
    pairs = hl.pairs(rows, E, K, mode)[0]
    P = pairs.shape[1]
    if mode == hl.BINARY:
        local = mb.edge_label_index.cpu().numpy()
        assert local.shape == (2, P) and np.array_equal(got[local], pairs)
        assert mb.edge_label.dtype == torch.float32
        assert np.array_equal(mb.edge_label.cpu().numpy(), np.r_[np.ones(E), np.zeros(P - E)].astype(np.float32))
        assert mb.src_index is None and mb.dst_neg_index is None
    else:
        assert mb.edge_label_index is None and mb.dst_neg_index.shape == (E, K)
        assert np.array_equal(got[mb.src_index.cpu().numpy()], pairs[0, :E])
        assert np.array_equal(got[mb.dst_pos_index.cpu().numpy()], pairs[1, :E])
        assert np.array_equal(got[mb.dst_neg_index.cpu().numpy()], pairs[1, E:].reshape(E, K))
    if "x" in mb._sb.node_attrs:
        assert np.array_equal(mb.x.cpu().numpy(), loader.data.x.cpu().numpy()[got])
    if loader.unique:
        assert np.unique(got).size == got.size
    return rows[0]


@pytest.mark.parametrize("mode", ["binary", "triplet"])
@pytest.mark.parametrize("unique", [False, True], ids=["forest", "unique"])
@pytest.mark.parametrize("batch", [5, 64])
@pytest.mark.parametrize("fanout", [[3, 2], []], ids=["3-2", "seeds-only"])
@pytest.mark.parametrize("name", ["karate", "rmat"])
def test_mini_batches_equal_the_composition(datasets, name, fanout, batch, unique, mode):
    N = datasets[name][2]
    assert N % batch != 0
    loader = make(datasets, name, fanout, batch, unique=unique, neg_sampling=mode)
    assert len(loader) == -(-N // batch)
    duplicates = 0
    mbs = list(loader)
    assert len(mbs) == len(loader)
    for j, mb in enumerate(mbs):
        positions = np.arange(j * batch, min((j + 1) * batch, N))
        row = check_mini_batch(loader, name, mb, positions, CALL0 + j)
        duplicates += np.unique(row).size < row.size
    assert mbs[-1].batch_size == N % batch                         # the ragged last mini-batch: another E, another S
    if name == "karate" or batch == 64:                             # 34 nodes, or 256 and more seeds among 1 024 nodes:
        assert duplicates > 0                                       # seed rows with repeated endpoints were covered


def test_drop_last_and_edge_set(datasets):
    N = datasets["karate"][2]
    loader = make(datasets, "karate", [3, 2], 64, drop_last=True, edge_set=True, unique=True)
    assert loader._edge_set is not None and len(loader) == N // 64
    mbs = list(loader)
    assert len(mbs) == N // 64 and all(mb.batch_size == 64 for mb in mbs)
    for j, mb in enumerate(mbs):
        check_mini_batch(loader, "karate", mb, np.arange(j * 64, (j + 1) * 64), CALL0 + j)


def test_shuffle_hands_out_the_permutation_and_reproduces(datasets):
    N = datasets["rmat"][2]
    a, b = (make(datasets, "rmat", [3, 2], 64, shuffle=True) for _ in range(2))
    perms = []
    for epoch in range(2):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(SEED * 1000003 + epoch)
        perm = torch.randperm(N, device=DEV, generator=gen).cpu().numpy()
        perms.append(perm)
        for j, (ma, mb) in enumerate(zip(a, b)):
            positions = perm[j * 64:(j + 1) * 64]
            check_mini_batch(a, "rmat", ma, positions, CALL0 + epoch * len(a) + j)
            for f in ("n_id", "edge_index", "edge_label_index", "input_id"):
                assert torch.equal(getattr(ma, f), getattr(mb, f))
    assert not np.array_equal(perms[0], perms[1]) and sorted(perms[0]) == list(range(N))


def test_two_epochs_use_disjoint_call_ids(datasets):
    loader = make(datasets, "karate", [3, 2], 64)
    first, second = list(loader), list(loader)
    ids = [mb.call_id for mb in first], [mb.call_id for mb in second]
    assert ids[0] == list(range(CALL0, CALL0 + 3)) and ids[1] == list(range(CALL0 + 3, CALL0 + 6))
    for mb1, mb2 in zip(first, second):
        assert torch.equal(mb1.input_id, mb2.input_id)               # the same positives ...
        g1, g2 = mb1.n_id[mb1.edge_label_index], mb2.n_id[mb2.edge_label_index]
        E = mb1.batch_size
        assert torch.equal(g1[:, :E], g2[:, :E]) and not torch.equal(g1[:, E:], g2[:, E:])   # ... with fresh negatives


@pytest.mark.parametrize("unique", [False, True], ids=["forest", "unique"])
def test_two_iterators_alive_at_once_keep_their_slabs_apart(datasets, unique):
    kw = dict(unique=unique, neg_sampling="triplet")
    alone = make(datasets, "rmat", [3, 2], 5, **kw)
    epochs = [list(alone), list(alone)]
    both = make(datasets, "rmat", [3, 2], 5, **kw)
    n = 0
    for m0, m1 in zip(both, both):                                   # the second iterator is the next epoch
        for got, want in ((m0, epochs[0][n]), (m1, epochs[1][n])):
            for f in ("n_id", "edge_index", "src_index", "dst_pos_index", "dst_neg_index", "input_id", "neg_unverified"):
                assert torch.equal(getattr(got, f), getattr(want, f)), f
        n += 1
    assert n == len(alone)


@pytest.mark.parametrize("mode", ["binary", "triplet"])
@pytest.mark.parametrize("unique", [False, True], ids=["forest", "unique"])
def test_super_batch_fields_are_the_mini_batches_stacked(datasets, unique, mode):
    loader = make(datasets, "karate", [3, 2], 5, unique=unique, neg_sampling=mode)
    fields = ("edge_label_index", "edge_label", "src_index", "dst_pos_index", "dst_neg_index", "input_id", "neg_unverified")
    seen = 0
    for sb in loader.super_batches():
        assert sb.batch_size == sb.input_id.shape[1] and sb.neg_sampling == mode
        for f in fields:
            flat = getattr(sb, f)
            if flat is None:
                assert all(getattr(mb, f) is None for mb in sb)
                continue
            assert flat.shape[0] == len(sb)
            for j, mb in enumerate(sb):
                assert torch.equal(getattr(mb, f), flat[j]), f
        for j, mb in enumerate(sb):                                  # the views cut from the flat node arrays
            a = sb.node_ptr[j]
            assert torch.equal(mb.n_id, sb.n_id[a:sb.node_ptr[j + 1]])
        seen += len(sb)
    assert seen == len(loader)


@pytest.mark.parametrize("mode", ["binary", "triplet"])
def test_labels_pass_through_without_negatives(datasets, mode):
    N = datasets["rmat"][2]
    labels = torch.arange(N, dtype=torch.float32) * 0.5
    loader = make(datasets, "rmat", [3, 2], 64, neg_sampling_ratio=0, edge_label=labels, shuffle=True, neg_sampling=mode)
    eli = loader.edge_label_index
    for mb in loader:
        assert torch.equal(mb.edge_label.cpu(), labels[mb.input_id.cpu()])
        assert int(mb.neg_unverified) == 0
        if mode == "binary":
            assert torch.equal(mb.n_id[mb.edge_label_index], eli[:, mb.input_id])
        else:
            assert torch.equal(mb.n_id[mb.src_index], eli[0, mb.input_id]) and mb.dst_neg_index.shape == (mb.batch_size, 0)
    plain = make(datasets, "rmat", [], 64, neg_sampling_ratio=0)
    for mb in plain:
        assert torch.equal(mb.edge_label, torch.ones(mb.batch_size, device=DEV))


def test_refusals(datasets):
    from tch_geometric.loader import LinkNeighborLoader
    data, eli, N = datasets["rmat"]
    with pytest.raises(ValueError):
        LinkNeighborLoader(data, [3], edge_label_index=eli, edge_label=torch.ones(N), neg_sampling_ratio=1, device=DEV)
    with pytest.raises(ValueError):
        LinkNeighborLoader(data, [3], edge_label_index=eli, neg_sampling="structured", device=DEV)
    with pytest.raises(ValueError):
        LinkNeighborLoader(data, [3], edge_label_index=eli, neg_sampling_ratio=-1, device=DEV)
    for bad in (1 << 10, -1):
        wrong = eli.clone()
        wrong[1, 7] = bad
        with pytest.raises(IndexError):                              # at construction: nothing was launched with it
            LinkNeighborLoader(data, [3], edge_label_index=wrong, device=DEV)


def test_package_exports_the_loader():
    import tch_geometric
    from tch_geometric.loader import LinkNeighborLoader, NeighborLoader
    assert tch_geometric.LinkNeighborLoader is LinkNeighborLoader and issubclass(LinkNeighborLoader, NeighborLoader)
