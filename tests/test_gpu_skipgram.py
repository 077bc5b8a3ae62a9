"""GPU parity of tg_rw_skipgram (HIP, C ABI) and Node2VecLoader: the positive windows are the windows of the oracle's walks
(and of tg_random_walk's) at each mini-batch's call id, the negative windows are the addressed draws of helpers_skipgram,
in all three forms (1 = rows in LDS as uint32, 2 = as int64, 3 = flat through a workspace), bit for bit."""
import numpy as np
import pytest
import torch

import orc
from helpers import load_karate
from helpers_skipgram import negatives, windows

pytestmark = pytest.mark.gpu
SEED, FIRST = 0x5C1B6A, 41
FORMS = (1, 2, 3)
SHAPES = [(5, 3, 5), (50, 3, 3), (64, 1, 2), (1, 1, 1)]          # (B, R, G): 15 walkers per batch puts batch boundaries
LENGTHS = (2, 11, 17, 33)                                        # inside a wave; 64 puts them on a wave edge


@pytest.fixture(scope="module")
def cabi():
    from tch_geometric import _cabi
    return _cabi


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _to(dev, *arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


class _G:
    def __init__(self, name, ptrs, idx, n, dev, cabi):
        self.name, self.ptrs, self.idx, self.n = name, ptrs, idx, n
        self.p_d, self.i_d = _to(dev, ptrs, idx)
        self.view = cabi.graph_view(self.p_d, self.i_d)
        self.edge_set = cabi.edge_set(self.view, dev)
        self.deg = np.diff(ptrs)


@pytest.fixture(scope="module")
def graphs(cabi, dev):
    ei, n = load_karate()                                        # undirected: no dead ends
    kp, ki, _ = orc.to_csr(ei, n)
    n2 = 1 << 10                                                 # directed RMAT: many vertices without out-edges
    row, col = orc.rmat_edges(10, n2 * 16, 99)
    rp, ri, _ = orc.to_csr(np.stack([row, col]), n2)
    return {"karate": _G("karate", kp, ki, n, dev, cabi), "rmat": _G("rmat", rp, ri, n2, dev, cabi)}


def _seeds(g, G, B):
    """[G, B] seeds; on the RMAT graph the first one is a sink"""
    s = orc.seed_batches(0x57A27 + B, 0, G, B, g.n).astype(np.int64)
    if g.name == "rmat":
        s[0, 0] = int(np.flatnonzero(g.deg == 0)[0])
    return s


def _run(cabi, g, seeds_d, T, C, R, K, p, q, form, edge_set=None, n_nodes=None):
    pos, neg = cabi.rw_skipgram(g.view, seeds_d, T, C, R, K, p, q, SEED, FIRST, g.n if n_nodes is None else n_nodes,
                                edge_set=edge_set, form=form)
    return pos.cpu().numpy(), neg.cpu().numpy()


_walks = {}


def _oracle_walks(g, seeds, R, T, p, q):
    """[G][W, L] oracle walks of the mini-batches (computed once per case, shared, never written to)"""
    key = (g.name, seeds.tobytes(), seeds.shape, R, T, p, q)
    if key not in _walks:
        _walks[key] = [orc.random_walk(g.ptrs, g.idx, np.tile(seeds[b], R), T, p, q, orc.rng_philox(SEED, FIRST + b))
                       for b in range(seeds.shape[0])]
        for w in _walks[key]:
            w.setflags(write=False)
    return _walks[key]


@pytest.mark.parametrize("pq_es", [(1.0, 1.0, False), (1.0, 1.5, False), (1.0, 1.5, True)],
                         ids=["p1q1", "p1q1.5", "p1q1.5-edge-set"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%dR%dG%d" % s)
@pytest.mark.parametrize("graph", ["karate", "rmat"])
def test_windows_equal_the_oracle_and_random_walk(cabi, dev, graphs, graph, shape, pq_es):
    g, (B, R, G), (p, q, use_es) = graphs[graph], shape, pq_es
    seeds = _seeds(g, G, B)
    (seeds_d,) = _to(dev, seeds)
    W = R * B
    case = 0
    for L in LENGTHS:
        T = L - 1
        ref = _oracle_walks(g, seeds, R, T, p, q)
        dev_walks = [cabi.random_walk(g.view, seeds_d[b].repeat(R), T, p, q, SEED, FIRST + b).cpu().numpy() for b in range(G)]
        for b in range(G):
            assert np.array_equal(dev_walks[b], ref[b])
        for C in sorted({1, 2, L - 1, L}):
            K = (0, 1, 3)[case % 3]                              # every K meets every shape and form
            case += 1
            nw, U = L - C + 1, R * K * B
            outs = [_run(cabi, g, seeds_d, T, C, R, K, p, q, form, g.edge_set if use_es else None) for form in FORMS]
            for pos, neg in outs:
                assert pos.shape == (G, nw * W, C) and neg.shape == (G, nw * U, C)
                for b in range(G):
                    assert np.array_equal(pos[b], windows(ref[b], C)), (L, C, K, b)
                    assert np.array_equal(pos[b], windows(dev_walks[b], C))
                assert ((neg >= 0) & (neg < g.n)).all()
                if K:
                    assert np.array_equal(neg[:, :U, 0], np.tile(seeds, (1, R * K)))    # column 0 of window 0: the seed
            for pos, neg in outs[1:]:
                assert np.array_equal(pos, outs[0][0]) and np.array_equal(neg, outs[0][1])
            if K and B <= 5 and L <= 11:                         # the negatives' rule, where the Python restatement is quick
                for b in range(G):
                    assert np.array_equal(outs[0][1][b], windows(negatives(SEED, FIRST + b, seeds[b], R, K, L, g.n), C))


@pytest.mark.parametrize("pq", [(1.0, 1.0), (1.0, 1.5)])
def test_dead_ends_keep_their_padding(cabi, dev, graphs, pq):
    g, (B, R, G), L, C = graphs["rmat"], (50, 3, 3), 17, 4
    seeds = _seeds(g, G, B)
    ref = _oracle_walks(g, seeds, R, L - 1, *pq)
    rows = np.concatenate(ref)
    died_mid_walk = (rows[:, 1] >= 0) & (rows[:, -1] == -1)
    assert g.deg[seeds[0, 0]] == 0 and died_mid_walk.any() and (rows[:, -1] >= 0).any()   # the seeds were chosen for this
    (seeds_d,) = _to(dev, seeds)
    W, nw = R * B, L - C + 1
    for form in FORMS:
        pos, _ = _run(cabi, g, seeds_d, L - 1, C, R, 1, *pq, form)
        for b in range(G):
            assert np.array_equal(pos[b], windows(ref[b], C))
        sink = pos[0].reshape(nw, W, C)[:, 0::B, :]              # the R walkers of the sink seed: the seed, then -1
        assert (sink[0, :, 0] == seeds[0, 0]).all() and (sink[0, :, 1:] == -1).all() and (sink[1:] == -1).all()
        full = (pos >= 0).all(-1)                                # the documented mask
        assert full.any() and not full.all()


def test_negatives_are_the_addressed_draws(cabi, dev, graphs):
    g, (B, R, K, L), G = graphs["karate"], (7, 2, 2, 6), 2
    seeds = _seeds(g, G, B)
    (seeds_d,) = _to(dev, seeds)
    U = R * K * B
    for n_nodes in (g.n, 1, (1 << 40) + 12345):
        rows = [negatives(SEED, FIRST + b, seeds[b], R, K, L, n_nodes) for b in range(G)]
        for C in (1, 3, 6):
            for form in (FORMS if n_nodes < 2 ** 32 - 1 else (2, 3)):        # ids past 2^32 - 2 do not fit uint32 staging
                _, neg = _run(cabi, g, seeds_d, L - 1, C, R, K, 1.0, 1.0, form, n_nodes=n_nodes)
                for b in range(G):
                    assert np.array_equal(neg[b], windows(rows[b], C)), (n_nodes, C, form, b)
                assert (neg[:, :U, 0] == np.tile(seeds, (1, R * K))).all()
                draws = neg.reshape(G, L - C + 1, U, C)[:, 0, :, 1:] if C > 1 else neg.reshape(G, L - C + 1, U)[:, 1:]
                assert ((draws >= 0) & (draws < n_nodes)).all()
                if n_nodes == 1:
                    assert (draws == 0).all()
    assert len({int(x) for r in rows for x in r[:, 1:].ravel()}) > U          # and they are not all one value


@pytest.mark.parametrize("form", FORMS)
def test_nothing_is_written_outside_the_slabs(cabi, dev, graphs, form):
    g, (B, R, G), L, C, K, PAD, MARK = graphs["rmat"], (5, 3, 5), 11, 4, 3, 1000, -7777
    seeds = _seeds(g, G, B)
    (seeds_d,) = _to(dev, seeds)
    cfg = cabi.rw_skipgram_config(L - 1, C, R, K, g.n)
    pos_rows, neg_rows = cabi.rw_skipgram_capacity(cfg, B)
    ws_words = cabi.rw_skipgram_workspace_bytes(cfg, G, B, g.n, form) // 8
    assert (ws_words > 0) == (form == 3)
    sizes = [G * pos_rows * C, G * neg_rows * C, ws_words]
    bufs = [torch.full((n + 2 * PAD,), MARK, dtype=torch.int64, device=dev) for n in sizes]
    pos_v, neg_v, ws_v = [b[PAD:PAD + n] for b, n in zip(bufs, sizes)]
    out = (pos_v.view(G, pos_rows, C), neg_v.view(G, neg_rows, C))
    pos, neg = cabi.rw_skipgram(g.view, seeds_d, L - 1, C, R, K, 1.0, 1.5, SEED, FIRST, g.n, form=form,
                                ws=ws_v if form == 3 else None, out=out)
    assert pos.data_ptr() == pos_v.data_ptr() and neg.data_ptr() == neg_v.data_ptr()
    for b, n in zip(bufs, sizes):
        h = b.cpu().numpy()
        assert (h[:PAD] == MARK).all() and (h[PAD + n:] == MARK).all()        # the words before and after are untouched
        assert (h[PAD:PAD + n] != MARK).all()                                 # and every word inside was written
    ref = _oracle_walks(g, seeds, R, L - 1, 1.0, 1.5)
    for b in range(G):
        assert np.array_equal(pos[b].cpu().numpy(), windows(ref[b], C))


@pytest.mark.parametrize("drop_last", [False, True])
def test_loader_equals_the_one_call_operator(cabi, dev, graphs, drop_last):
    from tch_geometric import Node2VecLoader
    from tch_geometric.transforms import Graph
    g = graphs["karate"]
    ei, n = load_karate()
    data = Graph(edge_index=torch.from_numpy(ei).to(dev), num_nodes=n)
    nodes = torch.from_numpy(np.random.default_rng(5).permutation(n)[:23].astype(np.int64))
    T, C, R, K, p, q = 8, 4, 2, 2, 1.0, 1.5
    loader = Node2VecLoader(data, T, C, walks_per_node=R, num_negative_samples=K, p=p, q=q, input_nodes=nodes, batch_size=5,
                            prefetch=3, drop_last=drop_last, seed=SEED, call_id0=FIRST)
    n_batches = 4 if drop_last else 5
    assert len(loader) == n_batches
    widths = [5, 5, 5, 5] + ([] if drop_last else [3])
    for epoch in range(2):                                       # a second epoch continues the call ids
        minis = list(loader)
        assert [m.batch_size for m in minis] == widths
        assert [m.call_id for m in minis] == [FIRST + epoch * n_batches + j for j in range(n_batches)]
        for j, m in enumerate(minis):
            s = nodes[5 * j:5 * j + widths[j]].to(dev).reshape(1, -1).contiguous()
            pos, neg = cabi.rw_skipgram(g.view, s, T, C, R, K, p, q, SEED, m.call_id, n, edge_set=g.edge_set)
            assert torch.equal(m.pos_rw, pos[0]) and torch.equal(m.neg_rw, neg[0])
            assert m.pos_rw.shape == ((T + 2 - C) * R * widths[j], C) and m.neg_rw.shape == ((T + 2 - C) * R * K * widths[j], C)
    assert loader._edge_set is not None                          # p != q: has_edge is answered from the edge set
    again = Node2VecLoader(data, T, C, walks_per_node=R, num_negative_samples=K, p=p, q=q, input_nodes=nodes, batch_size=5,
                           prefetch=3, drop_last=drop_last, seed=SEED, call_id0=FIRST)
    sbs = list(again.super_batches())
    assert [len(sb) for sb in sbs] == [3, 1] + ([] if drop_last else [1])
    assert [sb.call_id0 for sb in sbs] == [FIRST, FIRST + 3] + ([] if drop_last else [FIRST + 4])
    first_epoch = list(Node2VecLoader(data, T, C, walks_per_node=R, num_negative_samples=K, p=p, q=q, input_nodes=nodes,
                                      batch_size=5, prefetch=3, drop_last=drop_last, seed=SEED, call_id0=FIRST))
    flat = [(sb.pos_rw[b], sb.neg_rw[b]) for sb in sbs for b in range(len(sb))]
    assert len(flat) == len(first_epoch)
    for (pos, neg), m in zip(flat, first_epoch):
        assert torch.equal(pos, m.pos_rw) and torch.equal(neg, m.neg_rw)
    plain = Node2VecLoader(data, T, C, p=1.0, q=1.0, batch_size=5)
    assert next(iter(plain)).batch_size == 5 and plain._edge_set is None     # p = q = 1 never asks has_edge
