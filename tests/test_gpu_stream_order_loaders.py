"""The loaders as consumers that run BEHIND the host (tests/helpers_stream.py): a whole epoch with the current stream set
to a side stream and a blocker enqueued on it before every next(it); every mini-batch's tensors are cloned on that stream
and compared, at the end, with the same epoch of a fresh loader iterated on the default stream.  This is where a missing
side.wait_stream(cur) or `free` event lets launch i + 2 overwrite a slab whose compaction copy has not run yet.  Every
loader runs prefetch = 2, at least 5 launches and a ragged last mini-batch."""
import numpy as np
import pytest
import torch

import helpers_stream as hs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, E = 500, 6000
OPTIONAL = ("input_time", "node_time", "batch", "root_n_id", "edge_label_index", "edge_label", "edge_label_time", "input_id",
            "src_index", "dst_pos_index", "dst_neg_index")


def _graph():
    from tch_geometric.transforms import Graph
    rs = np.random.default_rng(11)
    ei = np.stack([rs.integers(0, N, E), rs.integers(0, N, E)]).astype(np.int64)
    return Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=N,
                 x=torch.from_numpy(rs.standard_normal((N, 12)).astype(np.float32)).to(DEV),
                 edge_attr=torch.from_numpy(rs.standard_normal((E, 2)).astype(np.float32)).to(DEV),
                 time=torch.from_numpy(rs.integers(0, 100, E)).to(DEV))


def _tensors(b):
    """every tensor a mini-batch hands out, cloned on the current stream, plus its host-side facts"""
    out = {k: v.clone() for k, v in b.tensor_items()}
    for k in OPTIONAL:
        try:
            v = getattr(b, k)
        except AttributeError:
            continue
        if isinstance(v, torch.Tensor):
            out[k] = v.clone()
    out["call_id"], out["batch_size"] = b.call_id, int(b.batch_size)
    return out


def _epoch(loader, stream=None):
    """one epoch -> the clones of every mini-batch; with `stream`: on it, a blocker ahead of every next()"""
    got = []
    if stream is None:
        for b in loader:
            got.append(_tensors(b))
        return got
    with torch.cuda.stream(stream):
        it = iter(loader)
        while True:
            hs.block(stream)
            try:
                b = next(it)
            except StopIteration:
                return got
            got.append(_tensors(b))


def _same_epoch(make):
    want = _epoch(make())
    torch.cuda.synchronize()
    lagging = make()
    torch.cuda.synchronize()
    s = hs.side_stream()
    got = _epoch(lagging, s)
    s.synchronize()
    torch.cuda.synchronize()
    assert len(got) == len(want) >= 10
    assert any(bool(t.ne(0).any()) for b in want for t in b.values() if isinstance(t, torch.Tensor))
    for j, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == sorted(w), j
        for k in w:
            if isinstance(w[k], torch.Tensor):
                assert g[k].shape == w[k].shape and torch.equal(g[k], w[k]), (j, k)
            else:
                assert g[k] == w[k], (j, k)
    return want


NEIGHBOR = {
    "plain": dict(),
    "unique+induced": dict(unique=True, induced=True),
    "temporal+disjoint": dict(unique=True, disjoint=True, time_attr="time"),
}


@pytest.mark.parametrize("config", sorted(NEIGHBOR))
def test_neighbor_loader_behind_the_host(config):
    from tch_geometric.loader import NeighborLoader
    g = _graph()
    kw = dict(NEIGHBOR[config])
    if "time_attr" in kw:
        kw["input_time"] = torch.from_numpy(np.random.default_rng(12).integers(50, 100, N)).to(DEV)
    # 500 seeds, 48 per mini-batch: 10 full ones in 5 launches of 2, then the ragged eleventh
    want = _same_epoch(lambda: NeighborLoader(g, [5, 4], batch_size=48, prefetch=2, seed=9, call_id0=100, **kw))
    assert len(want) == 11 and want[-1]["batch_size"] <= 500 - 480


def test_link_neighbor_loader_behind_the_host():
    from tch_geometric.loader import LinkNeighborLoader
    g = _graph()
    eli = g.edge_index[:, :1000].contiguous()
    want = _same_epoch(lambda: LinkNeighborLoader(g, [4, 3], edge_label_index=eli, neg_sampling_ratio=2, batch_size=96,
                                                  prefetch=2, seed=9, call_id0=100))
    assert len(want) == 11                                          # 10 full mini-batches in 5 launches, 40 edges left over


def test_shadow_loader_behind_the_host():
    from tch_geometric.loader import ShaDowKHopLoader
    g = _graph()
    want = _same_epoch(lambda: ShaDowKHopLoader(g, 2, 4, batch_size=48, prefetch=2, seed=9, call_id0=100))
    assert len(want) == 11


def test_pipelined_partitioned_sampler_behind_the_host():
    """partitioned.PipelinedPartitionedSampler, world 1: a stream per lane, forked from the caller's stream and joined
    back.  The seeds arrive on the caller's stream behind the blocker (copied over decoys), the lanes' outputs are cloned in
    `consume`, on the lane's stream."""
    from tch_geometric import _cabi, partitioned
    dev = torch.device(DEV)
    n, nb, B, fan, jobs = 1 << 12, 3, 50, [4, 3], 5
    row, col = _cabi.rmat_edges(12, n * 16, 0xAA, dev)
    ptrs, idx, _ = _cabi.coo_to_csx(row, col, n, n, True)
    shard = partitioned.CscShard.from_full(ptrs, idx, 0, 1)
    real = [_cabi.seed_batches(9, 40 + nb * i, nb, B, n, dev) for i in range(jobs)]
    decoy = [_cabi.seed_batches(10, 40 + nb * i, nb, B, n, dev) for i in range(jobs)]

    def run(seeds):
        ps = partitioned.PipelinedPartitionedSampler(shard, nb, B, fan, lanes=2)
        snaps = {}

        def consume(i, out):
            snaps[i] = [t.clone() for t in (out.samples, out.rows, out.cols, out.edge_index, out.layer_offsets, out.counts)]
        ps.sample_many(jobs, lambda i: seeds[i], 17, lambda i: (300 + nb * i, None), consume)
        return ps, snaps

    _, want = run(real)
    _, other = run(decoy)
    torch.cuda.synchronize()
    assert any(not torch.equal(a, b) for i in want for a, b in zip(want[i], other[i]))
    assert all(bool(want[i][5].ne(0).any()) for i in want)
    seeds = [d.clone() for d in decoy]
    torch.cuda.synchronize()
    s = hs.side_stream()
    hs.block(s)
    with torch.cuda.stream(s):
        for buf, r in zip(seeds, real):
            buf.copy_(r)
        ps, got = run(seeds)
    s.synchronize()
    torch.cuda.synchronize()
    assert sorted(got) == sorted(want) == list(range(jobs))
    for i in want:
        for k, (a, b) in enumerate(zip(got[i], want[i])):
            # words past a batch's counts are never written: compare what the counts cover
            if k < 4:
                lim = want[i][5][:, 0 if k == 0 else 1]
                mask = torch.arange(a.shape[1], device=dev)[None, :] < lim[:, None]
                assert torch.equal(a[mask], b[mask]), (i, k)
            else:
                assert torch.equal(a, b), (i, k)
