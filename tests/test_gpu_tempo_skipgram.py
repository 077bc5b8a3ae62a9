"""GPU parity of tg_tempo_skipgram (HIP, C ABI) and TemporalWalkLoader: the positive windows and their timestamps are the
windows of the oracle's temporal walks (and of tg_tempo_random_walk's) at each mini-batch's call id, the negative windows
are tg_rw_skipgram's, bit for bit."""
import numpy as np
import pytest
import torch

import orc
from helpers import load_karate
from helpers_skipgram import negatives, windows

pytestmark = pytest.mark.gpu
SEED, FIRST = 0x5C1B6A, 41
SHAPES = [(5, 3, 5), (50, 3, 3), (64, 1, 2), (1, 1, 1)]          # (B, R, G): 15 walkers per batch put batch boundaries
LENGTHS = (2, 11, 17, 33)                                        # inside a workgroup's 4 walkers; 64 puts them on its edge
M_WINDOW = {"karate": (4, (0, 2)), "rmat": (50, (0, 15))}        # timestamps in [-1, M), the walk's window


@pytest.fixture(scope="module")
def cabi():
    from tch_geometric import _cabi
    return _cabi


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _to(dev, *arrs):
    return [torch.from_numpy(np.array(a, order="C")).to(dev) for a in arrs]    # a copy: the shared inputs are read-only


class _G:
    def __init__(self, name, ptrs, idx, n, dev, cabi):
        self.name, self.ptrs, self.idx, self.n = name, ptrs, idx, n
        self.M, self.window = M_WINDOW[name]
        rng = np.random.default_rng(7)
        self.node_ts = rng.integers(-1, self.M, n).astype(np.int64)
        self.edge_ts = rng.integers(-1, self.M, idx.size).astype(np.int64)
        self.p_d, self.i_d, self.nts_d, self.ets_d = _to(dev, ptrs, idx, self.node_ts, self.edge_ts)
        self.view = cabi.graph_view(self.p_d, self.i_d)
        self.deg = np.diff(ptrs)


@pytest.fixture(scope="module")
def graphs(cabi, dev):
    ei, n = load_karate()
    kp, ki, _ = orc.to_csr(ei, n)
    n2 = 1 << 10                                                 # directed RMAT: vertices without out-edges, rows of 999
    row, col = orc.rmat_edges(10, n2 * 16, 99)
    rp, ri, _ = orc.to_csr(np.stack([row, col]), n2)
    return {"karate": _G("karate", kp, ki, n, dev, cabi), "rmat": _G("rmat", rp, ri, n2, dev, cabi)}


_inputs = {}


def _seeds(g, G, B):
    """[G, B] seeds and start times; on the RMAT graph the first seed is a sink.  seeds_ts[0, -1] admits nothing (that walker
    only restarts), seeds_ts[0, 1 % B] = -1 admits everything."""
    key = (g.name, G, B)
    if key not in _inputs:
        s = orc.seed_batches(0x57A27 + B, 0, G, B, g.n).astype(np.int64)
        if g.name == "rmat":
            s[0, 0] = int(np.flatnonzero(g.deg == 0)[0])
        rng = np.random.default_rng(7)                           # the graph's generator, past node_ts and edge_ts
        rng.integers(-1, g.M, g.n), rng.integers(-1, g.M, g.idx.size)
        ts = rng.integers(-1, g.M, (G, B)).astype(np.int64)
        ts[0, -1] = g.M + 5
        ts[0, 1 % B] = -1
        s.setflags(write=False)
        ts.setflags(write=False)
        _inputs[key] = (s, ts)
    return _inputs[key]


_walks = {}


def _oracle_walks(g, seeds, seeds_ts, R, L):
    """[G] of (walks [W, L], timestamps [W, L]) by the oracle (computed once per case, shared, never written to)"""
    key = (g.name, seeds.shape, R, L)
    if key not in _walks:
        out = []
        for b in range(seeds.shape[0]):
            w, t = orc.tempo_random_walk(g.ptrs, g.idx, g.node_ts, g.edge_ts, np.tile(seeds[b], R), np.tile(seeds_ts[b], R), L,
                                         g.window, orc.rng_philox(SEED, FIRST + b))
            w.setflags(write=False)
            t.setflags(write=False)
            out.append((w, t))
        _walks[key] = out
    return _walks[key]


def _run(cabi, g, seeds_d, ts_d, L, C, R, K, first=FIRST, **kw):
    cfg = cabi.tempo_skipgram_config(L, C, g.window, R, K, g.n)
    pos, pts, neg = cabi.tempo_skipgram(g.view, g.nts_d, g.ets_d, seeds_d, ts_d, cfg, SEED, first, **kw)
    return pos.cpu().numpy(), None if pts is None else pts.cpu().numpy(), neg.cpu().numpy()


def _check_preconditions(g, ref, seeds, seeds_ts, B, R, L):
    """what the inputs were chosen for, asserted on the oracle's walks before anything is compared"""
    rows = np.concatenate([w for w, _ in ref])
    assert (rows >= 0).all()                                     # a temporal walk restarts, it never ends
    if g.name != "rmat" or B < 5 or L < 11:
        return
    assert g.deg.max() == 999
    on_long_rows = int((g.deg[rows[:, :-1]] > 128).sum())        # steps taken from rows longer than 128: both stream_row_ts
    assert on_long_rows >= 50, on_long_rows                      # paths run and the chunk draws pass chunk 0, dozens of times
    seen = np.array([np.isin(r, r[:1]).all() for r in rows])     # a walker that never left its start only restarted ...
    assert seen.any() and not seen.all()                         # ... and others moved
    assert g.deg[seeds[0, 0]] == 0 and (ref[0][0][0::B][:, :] == seeds[0, 0]).all()
    if R > 1:                                                    # R copies of one seed walk differently
        W = R * B
        first = ref[0][0].reshape(R, B, L)
        assert any((first[0, i] != first[1, i]).any() for i in range(B)), W


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%dR%dG%d" % s)
@pytest.mark.parametrize("graph", ["karate", "rmat"])
def test_windows_equal_the_oracle_and_tempo_random_walk(cabi, dev, graphs, graph, shape):
    g, (B, R, G) = graphs[graph], shape
    seeds, seeds_ts = _seeds(g, G, B)
    seeds_d, ts_d = _to(dev, seeds, seeds_ts)
    W = R * B
    case = 0
    for L in LENGTHS:
        ref = _oracle_walks(g, seeds, seeds_ts, R, L)
        _check_preconditions(g, ref, seeds, seeds_ts, B, R, L)
        dev_walks = [cabi.tempo_random_walk(g.view, g.nts_d, g.ets_d, seeds_d[b].repeat(R), ts_d[b].repeat(R), L, g.window, SEED,
                                            FIRST + b) for b in range(G)]
        dev_walks = [(w.cpu().numpy(), t.cpu().numpy()) for w, t in dev_walks]
        for b in range(G):
            assert np.array_equal(dev_walks[b][0], ref[b][0]) and np.array_equal(dev_walks[b][1], ref[b][1])
        for C in sorted({1, 2, L - 1, L}):
            K = (0, 1, 3)[case % 3]                              # every K meets every shape
            case += 1
            nw, U = L - C + 1, R * K * B
            pos, pts, neg = _run(cabi, g, seeds_d, ts_d, L, C, R, K)
            assert pos.shape == pts.shape == (G, nw * W, C) and neg.shape == (G, nw * U, C)
            for b in range(G):
                assert np.array_equal(pos[b], windows(ref[b][0], C)), (L, C, K, b)
                assert np.array_equal(pts[b], windows(ref[b][1], C)), (L, C, K, b)
                assert np.array_equal(pos[b], windows(dev_walks[b][0], C)) and np.array_equal(pts[b], windows(dev_walks[b][1], C))
            _, rw_neg = cabi.rw_skipgram(g.view, seeds_d, L - 1, C, R, K, 1.0, 1.0, SEED, FIRST, g.n)
            assert np.array_equal(neg, rw_neg.cpu().numpy())     # tg_rw_skipgram's negatives with T = L - 1, bit for bit
            if K and B <= 5 and L <= 11:                         # the negatives' rule, where the Python restatement is quick
                for b in range(G):
                    assert np.array_equal(neg[b], windows(negatives(SEED, FIRST + b, seeds[b], R, K, L, g.n), C))


@pytest.mark.parametrize("with_ts,K", [(True, 3), (False, 3), (True, 0)], ids=["all", "no-ts", "no-neg"])
def test_every_word_is_written_and_nothing_else(cabi, dev, graphs, with_ts, K):
    g, (B, R, G), L, C, PAD, MARK = graphs["rmat"], (5, 3, 5), 11, 4, 1000, -7777
    seeds, seeds_ts = _seeds(g, G, B)
    seeds_d, ts_d = _to(dev, seeds, seeds_ts)
    cfg = cabi.tempo_skipgram_config(L, C, g.window, R, K, g.n)
    pos_rows, neg_rows = cabi.tempo_skipgram_capacity(cfg, B)
    assert (neg_rows == 0) == (K == 0)
    sizes = [G * pos_rows * C, G * pos_rows * C, G * neg_rows * C]
    bufs = [torch.full((n + 2 * PAD,), MARK, dtype=torch.int64, device=dev) for n in sizes]
    pos_v, pts_v, neg_v = [b[PAD:PAD + n] for b, n in zip(bufs, sizes)]
    out = (pos_v.view(G, pos_rows, C), pts_v.view(G, pos_rows, C) if with_ts else None, neg_v.view(G, neg_rows, C))
    pos, pts, neg = cabi.tempo_skipgram(g.view, g.nts_d, g.ets_d, seeds_d, ts_d, cfg, SEED, FIRST, with_ts=with_ts, out=out)
    assert pos.data_ptr() == pos_v.data_ptr() and (pts is None) == (not with_ts)
    for which, (b, n) in enumerate(zip(bufs, sizes)):
        h = b.cpu().numpy()
        assert (h[:PAD] == MARK).all() and (h[PAD + n:] == MARK).all()        # the words before and after are untouched
        if which == 1 and not with_ts:
            assert (h == MARK).all()                                          # pos_ts was not wanted: not written
        else:
            assert (h[PAD:PAD + n] != MARK).all()                             # every word inside was written
    ref = _oracle_walks(g, seeds, seeds_ts, R, L)
    for b in range(G):
        assert np.array_equal(pos[b].cpu().numpy(), windows(ref[b][0], C))
        if with_ts:
            assert np.array_equal(pts[b].cpu().numpy(), windows(ref[b][1], C))


def test_long_rows(cabi, dev, graphs):
    """an L at which a workgroup holds fewer walkers than its maximum, and the largest L the call accepts"""
    g, (B, R, G) = graphs["karate"], (3, 1, 2)
    seeds, seeds_ts = _seeds(g, G, B)
    seeds_d, ts_d = _to(dev, seeds, seeds_ts)
    tile = lambda L: cabi.tempo_skipgram_lds_bytes(cabi.tempo_skipgram_config(L, 1, g.window, R, 1, g.n))[0]
    full = tile(2)
    shrunk = next(L for L in range(2, 1 << 16) if tile(L) < full)
    lo, hi = shrunk, 1 << 16                                     # tile(lo) accepted; find the last accepted L by bisection
    with pytest.raises(cabi.TchGeoError):
        tile(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        try:
            tile(mid)
            lo = mid
        except cabi.TchGeoError:
            hi = mid
    longest = lo
    assert 1 < tile(shrunk) < full and tile(longest) == 1 and longest > shrunk
    for L, C in ((shrunk, 7), (longest, longest - 2)):
        ref = _oracle_walks(g, seeds, seeds_ts, R, L)
        assert all((w >= 0).all() for w, _ in ref)
        pos, pts, neg = _run(cabi, g, seeds_d, ts_d, L, C, R, 1)
        for b in range(G):
            assert np.array_equal(pos[b], windows(ref[b][0], C)) and np.array_equal(pts[b], windows(ref[b][1], C))
        assert neg.shape == (G, (L - C + 1) * R * B, C) and ((neg >= 0) & (neg < g.n)).all()
    with pytest.raises(cabi.TchGeoError, match="walk_length %d" % (longest + 1)):
        _run(cabi, g, seeds_d, ts_d, longest + 1, 3, R, 1)


def test_call_ids_continue_across_launches(cabi, dev, graphs):
    g, (B, R, G), L, C, K = graphs["rmat"], (5, 3, 5), 17, 4, 2
    seeds, seeds_ts = _seeds(g, G, B)
    seeds_d, ts_d = _to(dev, seeds, seeds_ts)
    whole = _run(cabi, g, seeds_d, ts_d, L, C, R, K)
    head = _run(cabi, g, seeds_d[:2].contiguous(), ts_d[:2].contiguous(), L, C, R, K, first=FIRST)
    tail = _run(cabi, g, seeds_d[2:].contiguous(), ts_d[2:].contiguous(), L, C, R, K, first=FIRST + 2)
    for w, h, t in zip(whole, head, tail):
        assert np.array_equal(w, np.concatenate([h, t]))
    assert not np.array_equal(whole[0][0], whole[0][1])          # and the mini-batches are not copies of one another


def test_loader_equals_the_one_call_operator(cabi, dev, graphs):
    from tch_geometric import TemporalWalkLoader
    from tch_geometric import tch_geometric as host
    from tch_geometric.transforms import Graph
    ei, n = load_karate()
    E = ei.shape[1]
    rng = np.random.default_rng(11)
    edge_ts = torch.from_numpy(rng.integers(-1, 4, E).astype(np.int64))
    node_ts = torch.from_numpy(rng.integers(-1, 4, n).astype(np.int64))
    nodes = torch.from_numpy(rng.permutation(n)[:23].astype(np.int64))           # a subset, out of order
    input_ts = torch.from_numpy(rng.integers(-1, 4, 23).astype(np.int64))
    data = Graph(edge_index=torch.from_numpy(ei).to(dev), num_nodes=n, timestamps=edge_ts.to(dev))
    L, C, R, K, window = 9, 4, 2, 2, (0, 2)
    mk = lambda **kw: TemporalWalkLoader(data, L, C, window, walks_per_node=R, num_negative_samples=K, node_timestamps=node_ts,
                                         input_nodes=nodes, input_timestamps=input_ts, batch_size=5, prefetch=3, seed=SEED,
                                         call_id0=FIRST, **kw)
    loader = mk()
    # the operator on the same graph: CSR and the timestamps carried into its edge order
    ptrs, idx, perm = host.to_csr(data.edge_index, n)
    view, ets_csr, nts_d = cabi.graph_view(ptrs, idx), edge_ts.to(dev)[perm], node_ts.to(dev)
    cfg = cabi.tempo_skipgram_config(L, C, window, R, K, n)
    widths, epochs = [5, 5, 5, 5, 3], []
    assert len(loader) == 5
    for epoch in range(2):                                       # a second epoch continues the call ids
        minis = list(loader)
        assert [m.batch_size for m in minis] == widths
        assert [m.call_id for m in minis] == [FIRST + epoch * 5 + j for j in range(5)]
        for j, m in enumerate(minis):
            s = nodes[5 * j:5 * j + widths[j]].to(dev).reshape(1, -1).contiguous()
            t = input_ts[5 * j:5 * j + widths[j]].to(dev).reshape(1, -1).contiguous()     # sliced exactly as the nodes are
            pos, pts, neg = cabi.tempo_skipgram(view, nts_d, ets_csr, s, t, cfg, SEED, m.call_id)
            assert torch.equal(m.pos_rw, pos[0]) and torch.equal(m.pos_ts, pts[0]) and torch.equal(m.neg_rw, neg[0])
            assert m.pos_rw.shape == ((L - C + 1) * R * widths[j], C) == m.pos_ts.shape
            assert m.neg_rw.shape == ((L - C + 1) * R * K * widths[j], C)
        epochs.append(minis)
    assert not torch.equal(epochs[0][0].pos_rw, epochs[1][0].pos_rw)             # epoch 1 draws afresh
    sbs = list(mk().super_batches())
    assert [len(sb) for sb in sbs] == [3, 1, 1] and [sb.call_id0 for sb in sbs] == [FIRST, FIRST + 3, FIRST + 4]
    flat = [sb[b] for sb in sbs for b in range(len(sb))]
    for a, m in zip(flat, epochs[0]):
        assert torch.equal(a.pos_rw, m.pos_rw) and torch.equal(a.pos_ts, m.pos_ts) and torch.equal(a.neg_rw, m.neg_rw)
    bare = list(mk(with_timestamps=False))
    assert all(m.pos_ts is None for m in bare) and next(iter(mk(with_timestamps=False).super_batches())).pos_ts is None
    for a, m in zip(bare, epochs[0]):
        assert torch.equal(a.pos_rw, m.pos_rw) and torch.equal(a.neg_rw, m.neg_rw)
    # the oracle on the first mini-batch: the loader's CSR order and timestamps are the ones the walk law is stated on
    w, t = orc.tempo_random_walk(ptrs.cpu().numpy(), idx.cpu().numpy(), node_ts.numpy(), ets_csr.cpu().numpy(),
                                 np.tile(nodes[:5].numpy(), R), np.tile(input_ts[:5].numpy(), R), L, window,
                                 orc.rng_philox(SEED, FIRST))
    assert np.array_equal(epochs[0][0].pos_rw.cpu().numpy(), windows(w, C))
    assert np.array_equal(epochs[0][0].pos_ts.cpu().numpy(), windows(t, C))
