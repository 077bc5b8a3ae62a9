"""LastNeighborLoader and TemporalEventLoader against the NumPy restatement (helpers_lastn): every (n_id, edge_index, e_id)
over a stream of insert / lookup rounds, including a batch with more than `size` events on one node, where PyG's published
algorithm (torch_geometric/nn/models/tgn.py, restated in NumPy below) keeps other entries; the event loader's mini-batches
over two epochs, under two prefetch depths, and its rule for two live iterators: the loader holds one state, so a newer
iterator REFUSES the older one (RuntimeError at the older one's next launch)."""
import numpy as np
import pytest
import torch

import helpers_lastn as hl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class PyGRule:
    """PyG's LastNeighborLoader.insert in NumPy: a batch's entries of a node are numbered `arange % size` over the node-sorted
    batch, so more than `size` of them collide (the last write wins), then the top `size` e_ids of old ++ new are kept"""

    def __init__(self, n, size):
        self.size, self.cur = size, 0
        self.nbr, self.e_id = np.zeros((n, size), np.int64), np.full((n, size), -1, np.int64)

    def insert(self, src, dst):
        size = self.size
        nbrs, nodes = np.concatenate([src, dst]), np.concatenate([dst, src])
        e_id = np.tile(np.arange(self.cur, self.cur + src.size), 2)
        self.cur += src.size
        perm = np.argsort(nodes, kind="stable")
        nodes, nbrs, e_id = nodes[perm], nbrs[perm], e_id[perm]
        n_id, assoc = np.unique(nodes, return_inverse=True)
        dense = np.arange(nodes.size) % size + assoc.reshape(-1) * size
        d_e, d_n = np.full(n_id.size * size, -1, np.int64), np.zeros(n_id.size * size, np.int64)
        d_e[dense], d_n[dense] = e_id, nbrs
        all_e = np.concatenate([self.e_id[n_id], d_e.reshape(-1, size)], axis=1)
        all_n = np.concatenate([self.nbr[n_id], d_n.reshape(-1, size)], axis=1)
        top = np.argsort(-all_e, axis=1, kind="stable")[:, :size]
        self.e_id[n_id], self.nbr[n_id] = np.take_along_axis(all_e, top, 1), np.take_along_axis(all_n, top, 1)

    def kept(self, v):
        return sorted(int(e) for e in self.e_id[v] if e >= 0)


def same(got, want):
    return all(np.array_equal(g.cpu().numpy(), np.asarray(w)) for g, w in zip(got, want)) and len(got) == len(want)


def test_fifty_rounds_against_the_restatement_and_pyg_differs_on_a_burst():
    import tch_geometric
    n, size = 120, 4
    loader = tch_geometric.LastNeighborLoader(n, size, device=DEV)
    ref, pyg, rs, base = hl.State(n, size), PyGRule(n, size), np.random.default_rng(3), 0
    for rnd in range(50):
        q = rs.integers(0, n, int(rs.integers(1, 40)))                # repeats happen
        got = loader(torch.from_numpy(q))
        assert same(got, hl.loader_view(*ref.sample(q, [size])[:4])), rnd
        assert got[0][:1].item() == q[0] and got[1].shape[0] == 2
        m = int(rs.integers(1, 60))
        src, dst = rs.integers(0, n, m), rs.integers(0, n, m)
        burst = rnd == 20
        if burst:
            # 12 events on node 17 in one insert, as source and as destination in turn: PyG sorts the batch by node with
            # the destination roles first, so its numbering `arange % size` keeps events 4, 6, 8, 10 of the 12
            other, odd = rs.integers(18, n, 3 * size), np.arange(3 * size) % 2 == 1
            src, dst = np.where(odd, other, 17), np.where(odd, 17, other)
        loader.insert(torch.from_numpy(src).to(DEV), torch.from_numpy(dst))
        ref.insert(src, dst, e_base=base)
        pyg.insert(src, dst)
        base += src.size
        assert loader.cur_e_id == base
        ours17 = sorted(e for _, e in ref.newest(17, size))
        if burst:
            assert ours17 == list(range(base - size, base))          # exactly the newest `size`
            assert pyg.kept(17) != ours17                            # PyG's numbering collides there
    assert same(loader(torch.arange(n)), hl.loader_view(*ref.sample(np.arange(n), [size])[:4]))
    loader.reset_state()
    n_id, ei, e_id = loader(torch.arange(5))
    assert n_id.tolist() == [0, 1, 2, 3, 4] and ei.shape == (2, 0) and e_id.numel() == 0 and loader.cur_e_id == 0


def test_pyg_agrees_where_no_node_exceeds_size_in_one_insert():
    n, size = 60, 5
    ref, pyg, rs, base = hl.State(n, size), PyGRule(n, size), np.random.default_rng(4), 0
    for _ in range(30):
        src = rs.permutation(n)[:10]
        dst = (src + 1 + rs.integers(0, 3, 10)) % n                  # a node appears at most size = 5 times in the batch
        counts = np.bincount(np.concatenate([src, dst]), minlength=n)
        assert counts.max() <= size
        ref.insert(src, dst, e_base=base)
        pyg.insert(src, dst)
        base += 10
        for v in range(n):
            assert pyg.kept(v) == sorted(e for _, e in ref.newest(v, size))


def test_two_hops_state_dict_and_refusals():
    import tch_geometric
    n, size = 80, 3
    loader = tch_geometric.LastNeighborLoader(n, size, device=DEV, num_hops=2)
    ref, rs = hl.State(n, size), np.random.default_rng(5)
    src, dst = rs.integers(0, n, 300), rs.integers(0, n, 300)
    loader.insert(torch.from_numpy(src), torch.from_numpy(dst))
    ref.insert(src, dst)
    q = rs.integers(0, n, 25)
    want2 = hl.loader_view(*ref.sample(q, [size, size])[:4])
    assert same(loader(torch.from_numpy(q)), want2)
    assert same(loader(torch.from_numpy(q), num_hops=1), hl.loader_view(*ref.sample(q, [size])[:4]))
    saved = loader.state_dict()
    loader.insert(torch.from_numpy(dst), torch.from_numpy(src))
    assert not same(loader(torch.from_numpy(q)), want2) and loader.cur_e_id == 600
    loader.load_state_dict(saved)
    assert same(loader(torch.from_numpy(q)), want2) and loader.cur_e_id == 300
    with pytest.raises(ValueError, match="nodes"):
        tch_geometric.LastNeighborLoader(n + 1, size, device=DEV).load_state_dict(saved)
    with pytest.raises(RuntimeError, match="outside"):
        loader(torch.tensor([0, n]))
    assert same(loader(torch.from_numpy(q)), want2)                   # the status word was cleared


def event_list(n=90, E=1000, seed=6):
    rs = np.random.default_rng(seed)
    src, dst = rs.integers(0, n, E), rs.integers(0, n, E)
    dst[100:140] = 7                                                 # a burst inside one mini-batch
    t = np.sort(rs.integers(0, 500, E))
    return n, torch.from_numpy(src), torch.from_numpy(dst), torch.from_numpy(t)


def check_epoch(loader, n, size, fanout, src, dst, t, batch_size):
    """every mini-batch of one epoch against the restatement, with neg_dst taken from the batch as given -> the batches"""
    ref, a, batches = hl.State(n, size), 0, list(loader)
    assert len(batches) == len(loader) == -(-src.numel() // batch_size)
    for j, b in enumerate(batches):
        w = min(batch_size, src.numel() - a)
        assert torch.equal(b.src.cpu(), src[a:a + w]) and torch.equal(b.dst.cpu(), dst[a:a + w]) and torch.equal(b.t.cpu(), t[a:a + w])
        assert b.input_id.tolist() == list(range(a, a + w)) and b.neg_dst.numel() == w * loader.ratio
        assert 0 <= int(b.neg_dst.min()) and int(b.neg_dst.max()) < n
        seeds = np.concatenate([b.src.cpu().numpy(), b.dst.cpu().numpy(), b.neg_dst.cpu().numpy()])
        n_id, ei, e_id = hl.loader_view(*ref.sample(seeds, fanout)[:4])
        assert same((b.n_id, b.edge_index, b.e_id), (n_id, ei, e_id)), j
        assert torch.equal(b.n_id[b.src_index], b.src) and torch.equal(b.n_id[b.dst_index], b.dst)
        assert torch.equal(b.n_id[b.neg_index], b.neg_dst)
        assert b.e_id.numel() == 0 or int(b.e_id.max()) < a              # no event of this mini-batch or a later one
        assert j == 0 or b.e_id.numel() > 0
        ref.insert(src[a:a + w].numpy(), dst[a:a + w].numpy(), e_base=a)
        a += w
    return batches


@pytest.mark.parametrize("prefetch", [1, 8])
@pytest.mark.parametrize("num_neighbors", [None, [3, 2]])
def test_event_loader_two_epochs(prefetch, num_neighbors):
    import tch_geometric
    n, src, dst, t = event_list()
    loader = tch_geometric.TemporalEventLoader(src, dst, t, n, 5, 64, num_neighbors=num_neighbors, prefetch=prefetch, seed=9, device=DEV)
    fanout = [5] if num_neighbors is None else num_neighbors
    first = check_epoch(loader, n, 5, fanout, src, dst, t, 64)
    second = check_epoch(loader, n, 5, fanout, src, dst, t, 64)      # the state was reset: the restatement starts empty again
    assert not all(torch.equal(a.neg_dst, b.neg_dst) for a, b in zip(first, second))      # keyed by the epoch
    again = tch_geometric.TemporalEventLoader(src, dst, t, n, 5, 64, num_neighbors=num_neighbors, prefetch=prefetch, seed=9, device=DEV)
    assert all(torch.equal(a.neg_dst, b.neg_dst) and torch.equal(a.n_id, b.n_id) for a, b in zip(first, again))


def test_prefetch_depth_does_not_change_the_batches():
    """the negatives are keyed by the launch, so the depths are compared without them (every field), and with them through
    the restatement (test_event_loader_two_epochs runs both depths)"""
    import tch_geometric
    n, src, dst, t = event_list()
    one, eight = (list(tch_geometric.TemporalEventLoader(src, dst, t, n, 5, 64, neg_sampling_ratio=0, prefetch=p, device=DEV))
                  for p in (1, 8))
    assert len(one) == len(eight) == 16
    for a, b in zip(one, eight):
        for f in a.__slots__:
            assert torch.equal(getattr(a, f), getattr(b, f)), f
        assert a.neg_dst.numel() == 0 and a.neg_index.numel() == 0


def test_a_newer_iterator_refuses_the_older_one():
    import tch_geometric
    n, src, dst, t = event_list()
    loader = tch_geometric.TemporalEventLoader(src, dst, t, n, 5, 64, prefetch=2, neg_range=(10, 20), device=DEV)
    old = iter(loader)
    next(old)
    new = iter(loader)
    first = next(new)
    next(old)                                                        # still of the launch the older one had made
    with pytest.raises(RuntimeError, match="newer iterator"):
        next(old)
    rest = [first] + list(new)
    assert len(rest) == 16 and first.e_id.numel() == 0 and rest[1].e_id.numel() > 0
    assert all(10 <= int(b.neg_dst.min()) and int(b.neg_dst.max()) < 20 for b in rest)
