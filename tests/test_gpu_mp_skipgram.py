"""GPU parity of tg_mp_skipgram (HIP, C ABI) and MetaPath2VecLoader: the positive windows are the windows of the walks that
helpers_metapath restates (test_mp_skipgram_cpu.py ties that restatement to the oracle's random_walk), the negatives are
its addressed draws per column type, in all three forms (1 = rows in LDS as uint32 local ids, 2 = as int64, 3 = flat
through a workspace), bit for bit; with a one-relation metapath both slabs are tg_rw_skipgram's."""
import numpy as np
import pytest
import torch

import orc
from helpers import load_fake_hetero, load_karate
from helpers_metapath import column_types, finish, negatives, walks, windows

pytestmark = pytest.mark.gpu
SEED, FIRST = 0x3E7A9A7, 57
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


class _Typed:
    """a typed graph: node types in order, their counts, per relation the COO edges, the host CSR and its device view"""

    def __init__(self, name, counts, edges, dev, cabi):
        self.name, self.types, self.counts = name, list(counts), [counts[t] for t in counts]
        self.tix = {t: i for i, t in enumerate(self.types)}
        self.start = np.concatenate([[0], np.cumsum(self.counts)[:-1]]).astype(np.int64)
        self.dummy = int(sum(self.counts))
        self.edges, self.csr, self.view, self._keep = edges, {}, {}, []
        for et, ei in edges.items():
            ptrs, idx, _ = orc.to_csr(ei, (counts[et[0]], counts[et[2]]))
            self.csr[et] = (ptrs, idx)
            p_d, i_d = _to(dev, ptrs, idx)
            self.view[et] = cabi.graph_view(p_d, i_d)

    def path(self, names):
        ets = [next(et for et in self.edges if et[1] == n) if isinstance(n, str) else n for n in names]
        return ets, [self.tix[et[0]] for et in ets], [self.tix[et[2]] for et in ets]

    def config(self, cabi, names, T, C, R, K, starts="global", pad=None):
        ets, src, dst = self.path(names)
        starts = self.start if isinstance(starts, str) else starts
        pad = (self.dummy if starts is not None else -1) if pad is None else pad
        return cabi.mp_skipgram_config([self.view[et] for et in ets], src, dst, self.counts, T, C, R, K, type_start=starts,
                                       pad_value=pad)


def _hand_graph():
    """A (37), B (11), C (5); every relation has rows without out-edges"""
    g = np.random.default_rng(20240607)
    counts = {"A": 37, "B": 11, "C": 5}
    sinks = {"ab": (3, 20, 36), "ba": (5,), "bc": (0, 7), "cb": (2,), "aa": (1, 3, 30)}
    edges = {}
    for s, r, d in (("A", "ab", "B"), ("B", "ba", "A"), ("B", "bc", "C"), ("C", "cb", "B"), ("A", "aa", "A")):
        rows = [i for i in range(counts[s]) if i not in sinks[r] for _ in range(int(g.integers(1, 5)))]
        edges[(s, r, d)] = np.stack([np.asarray(rows, dtype=np.int64), g.integers(0, counts[d], len(rows))])
    return counts, edges, sinks


@pytest.fixture(scope="module")
def graphs(cabi, dev):
    counts, edges, _ = _hand_graph()
    fcounts, fedges = load_fake_hetero()
    return {"hand": _Typed("hand", counts, edges, dev, cabi), "fake": _Typed("fake", fcounts, fedges, dev, cabi)}


CASES = {                                                        # name -> (graph, metapath, the longest row it may walk)
    "ab-ba": ("hand", ["ab", "ba"], None),
    "ab-bc-cb-ba": ("hand", ["ab", "bc", "cb", "ba"], None),     # B is visited twice, through different relations
    "aa": ("hand", ["aa"], None),
    "open-ab-bc": ("hand", ["ab", "bc"], 3),                     # an open path: T <= 2
    "fake-v0-v2-v0": ("fake", [("v0", "e0", "v2"), ("v2", "e0", "v0")], None),
    "fake-v0-v1-v2-v0": ("fake", [("v0", "e0", "v1"), ("v1", "e0", "v2"), ("v2", "e0", "v0")], None),
}


def _seeds(g, first_type, G, B, sink=None):
    """[G, B] local ids of the metapath's first type; the first one is a row without out-edges where the graph has one"""
    s = orc.seed_batches(0x57A27 + B, 0, G, B, g.counts[first_type]).astype(np.int64)
    if sink is not None:
        s[0, 0] = sink
    return s


def _run(cabi, cfg, seeds_d, form, **kw):
    pos, neg = cabi.mp_skipgram(cfg, seeds_d, SEED, FIRST, form=form, **kw)
    return pos.cpu().numpy(), neg.cpu().numpy()


_ref = {}


def _ref_walks(g, names, seeds, R, T):
    """[G][W, L] local-id walks of the mini-batches (computed once per case, shared, never written to)"""
    key = (g.name, tuple(names), seeds.tobytes(), seeds.shape, R, T)
    if key not in _ref:
        ets, src, dst = g.path(names)
        _ref[key] = [walks(SEED, FIRST + b, [g.csr[et] for et in ets], src, dst, seeds[b], R, T) for b in range(seeds.shape[0])]
        for w in _ref[key]:
            w.setflags(write=False)
    return _ref[key]


def _first_sink(g, names):
    ets, _, _ = g.path(names)
    dead = np.flatnonzero(np.diff(g.csr[ets[0]][0]) == 0)
    return int(dead[0]) if dead.size else None


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%dR%dG%d" % s)
@pytest.mark.parametrize("case", list(CASES))
def test_windows_equal_the_restated_law(cabi, dev, graphs, case, shape):
    gname, names, max_L = CASES[case]
    g, (B, R, G) = graphs[gname], shape
    ets, src, dst = g.path(names)
    seeds = _seeds(g, src[0], G, B, _first_sink(g, names))
    (seeds_d,) = _to(dev, seeds)
    W = R * B
    n_case = 0
    for L in [x for x in LENGTHS if max_L is None or x <= max_L] + ([max_L] if max_L else []):
        T = L - 1
        ref = _ref_walks(g, names, seeds, R, T)
        types = column_types(src, dst, L)
        words = [finish(r, types, g.start, g.dummy) for r in ref]
        if gname == "hand" and B == 50 and L == (max_L or 17):   # the inputs were made for this: walks that end at step 0,
            rows = np.concatenate(ref)                           # mid-walk and never
            assert (rows[:, 1] == -1).any() and ((rows[:, 1] >= 0) & (rows[:, -1] == -1)).any() and (rows[:, -1] >= 0).any()
        lo = np.asarray([g.start[t] for t in types])
        hi = lo + np.asarray([g.counts[t] for t in types])
        for C in sorted({1, 2, L - 1, L}):
            K = (0, 1, 3)[n_case % 3]                            # every K meets every shape and form
            n_case += 1
            nw, U = L - C + 1, R * K * B
            cfg = g.config(cabi, names, T, C, R, K)
            outs = [_run(cabi, cfg, seeds_d, form) for form in FORMS]
            for pos, neg in outs:
                assert pos.shape == (G, nw * W, C) and neg.shape == (G, nw * U, C)
            for pos, neg in outs[1:]:
                assert np.array_equal(pos, outs[0][0]) and np.array_equal(neg, outs[0][1])
            pos, neg = outs[0]
            for b in range(G):
                assert np.array_equal(pos[b], windows(words[b], C)), (L, C, K, b)
            if K and B <= 5 and L <= 11:                         # the negatives' rule, where the Python restatement is quick
                for b in range(G):
                    x = negatives(SEED, FIRST + b, src, dst, seeds[b], R, K, L, g.counts)
                    assert np.array_equal(neg[b], windows(finish(x, types, g.start, g.dummy), C)), (L, C, K, b)
            elif K:                                              # elsewhere: every word lies in its column type's range
                v = neg.reshape(G, nw, U, C)
                for j in range(nw):
                    assert ((v[:, j] >= lo[j:j + C]) & (v[:, j] < hi[j:j + C])).all(), (L, C, K, j)
                assert np.array_equal(v[:, 0, :, 0], np.tile(seeds, (1, R * K)) + g.start[src[0]])


@pytest.mark.parametrize("graph", ["karate", "rmat"])
def test_one_relation_one_type_is_rw_skipgram(cabi, dev, graph):
    """the anchor: M = 1, one node type, no starts, pad -1 -> tg_rw_skipgram(p = q = 1) bit for bit, in every form"""
    if graph == "karate":
        ei, n = load_karate()
    else:
        n = 1 << 10                                              # directed RMAT: many vertices without out-edges
        ei = np.stack(orc.rmat_edges(10, n * 16, 99))
    ptrs, idx, _ = orc.to_csr(ei, n)
    p_d, i_d = _to(dev, ptrs, idx)
    view = cabi.graph_view(p_d, i_d)
    n_case = 0
    for B, R, G in ((5, 3, 5), (50, 3, 3)):
        seeds = orc.seed_batches(0x57A27 + B, 0, G, B, n).astype(np.int64)
        if graph == "rmat":
            seeds[0, 0] = int(np.flatnonzero(np.diff(ptrs) == 0)[0])
        (seeds_d,) = _to(dev, seeds)
        for L in (2, 11, 33):
            for C in sorted({1, 2, L}):
                K = (0, 1, 3)[n_case % 3]
                n_case += 1
                cfg = cabi.mp_skipgram_config([view], [0], [0], [n], L - 1, C, R, K, type_start=None, pad_value=-1)
                for form in FORMS:
                    rp, rn = cabi.rw_skipgram(view, seeds_d, L - 1, C, R, K, 1.0, 1.0, SEED, FIRST, n, form=form)
                    mp, mn = cabi.mp_skipgram(cfg, seeds_d, SEED, FIRST, form=form)
                    assert torch.equal(mp, rp) and torch.equal(mn, rn), (B, L, C, K, form)
                if graph == "rmat":
                    assert (rp[0, 0::B][:R, 1:] == -1).all() and (rp >= 0).all(-1).any()   # the sink's rows; whole windows


@pytest.mark.parametrize("form", FORMS)
def test_offsets_are_added_at_emit_in_64_bits(cabi, dev, graphs, form):
    g, names, (B, R, G), L, K = graphs["hand"], ["ab", "bc", "cb", "ba"], (50, 3, 3), 17, 2
    ets, src, dst = g.path(names)
    seeds = _seeds(g, src[0], G, B, _first_sink(g, names))
    (seeds_d,) = _to(dev, seeds)
    types = column_types(src, dst, L)
    for C in (1, 4, L):
        nw = L - C + 1
        lpos, lneg = _run(cabi, g.config(cabi, names, L - 1, C, R, K, starts=None), seeds_d, form)
        assert (lpos == -1).any() and (lneg >= 0).all()
        # PyG's table, and starts past 2^32 over counts of 37, 11 and 5: the uint32 form stages local ids
        for starts, pad in ((g.start, g.dummy), (np.asarray([1 << 33, (1 << 34) + 5, 7]), 1 << 40)):
            pos, neg = _run(cabi, g.config(cabi, names, L - 1, C, R, K, starts=starts, pad=pad), seeds_d, form)
            off = np.asarray([starts[t] for t in types], dtype=np.int64)
            for out, local in ((pos, lpos), (neg, lneg)):
                v, lv = out.reshape(G, nw, -1, C), local.reshape(G, nw, -1, C)
                for j in range(nw):
                    assert np.array_equal(v[:, j], np.where(lv[:, j] >= 0, lv[:, j] + off[j:j + C], pad)), (C, j)


@pytest.mark.parametrize("form", FORMS)
def test_nothing_is_written_outside_the_slabs(cabi, dev, graphs, form):
    g, names, (B, R, G), L, C, PAD, MARK = graphs["hand"], ["ab", "bc", "cb", "ba"], (5, 3, 5), 11, 4, 1000, -7777
    ets, src, dst = g.path(names)
    seeds = _seeds(g, src[0], G, B, _first_sink(g, names))
    (seeds_d,) = _to(dev, seeds)
    ref = _ref_walks(g, names, seeds, R, L - 1)
    types = column_types(src, dst, L)
    for K in (3, 0):
        cfg = g.config(cabi, names, L - 1, C, R, K)
        pos_rows, neg_rows = cabi.mp_skipgram_capacity(cfg, B)
        ws_words = cabi.mp_skipgram_workspace_bytes(cfg, G, B, form) // 8
        assert (ws_words > 0) == (form == 3) and (neg_rows > 0) == (K > 0)
        sizes = [G * pos_rows * C, G * neg_rows * C, ws_words]
        bufs = [torch.full((n + 2 * PAD,), MARK, dtype=torch.int64, device=dev) for n in sizes]
        pos_v, neg_v, ws_v = [b[PAD:PAD + n] for b, n in zip(bufs, sizes)]
        out = (pos_v.view(G, pos_rows, C), neg_v.view(G, neg_rows, C) if K else None)      # K = 0: no neg_rw at all
        pos, neg = cabi.mp_skipgram(cfg, seeds_d, SEED, FIRST, form=form, ws=ws_v if form == 3 else None, out=out)
        assert pos.data_ptr() == pos_v.data_ptr() and (not K or neg.data_ptr() == neg_v.data_ptr())
        assert tuple(neg.shape) == (G, neg_rows, C)
        for b, n in zip(bufs, sizes):
            h = b.cpu().numpy()
            assert (h[:PAD] == MARK).all() and (h[PAD + n:] == MARK).all()    # the words before and after are untouched
            assert (h[PAD:PAD + n] != MARK).all()                             # and every word inside was written
        for b in range(G):
            assert np.array_equal(pos[b].cpu().numpy(), windows(finish(ref[b], types, g.start, g.dummy), C))


@pytest.mark.parametrize("global_ids", [True, False])
@pytest.mark.parametrize("drop_last", [False, True])
def test_loader_equals_the_one_call_operator(cabi, dev, graphs, drop_last, global_ids):
    from tch_geometric import MetaPath2VecLoader
    from tch_geometric.transforms import HeteroGraph
    g, names = graphs["hand"], ["ab", "bc", "cb", "ba"]
    ets, src, dst = g.path(names)
    data = HeteroGraph()
    for t, n in zip(g.types, g.counts):
        data[t].num_nodes = n
    for et, ei in g.edges.items():
        data[et].edge_index = torch.from_numpy(ei).to(dev)
    nodes = torch.from_numpy(np.random.default_rng(5).permutation(37)[:23].astype(np.int64))
    T, C, R, K = 8, 4, 2, 2
    mk = lambda: MetaPath2VecLoader(data, ets, T, C, walks_per_node=R, num_negative_samples=K, input_nodes=nodes, batch_size=5,
                                    prefetch=3, drop_last=drop_last, seed=SEED, call_id0=FIRST, global_ids=global_ids)
    loader = mk()
    assert (loader.dummy_idx, loader.num_embeddings) == (53, 54) and loader.start == {"A": 0, "B": 37, "C": 48}
    cfg = g.config(cabi, names, T, C, R, K, starts="global" if global_ids else None)
    n_batches = 4 if drop_last else 5
    assert len(loader) == n_batches
    widths = [5, 5, 5, 5] + ([] if drop_last else [3])
    epochs = []
    for epoch in range(2):                                       # a second epoch continues the call ids
        minis = list(loader)
        assert [m.batch_size for m in minis] == widths
        assert [m.call_id for m in minis] == [FIRST + epoch * n_batches + j for j in range(n_batches)]
        for j, m in enumerate(minis):                            # the ragged last mini-batch included
            s = nodes[5 * j:5 * j + widths[j]].to(dev).reshape(1, -1).contiguous()
            pos, neg = cabi.mp_skipgram(cfg, s, SEED, m.call_id)
            assert torch.equal(m.pos_rw, pos[0]) and torch.equal(m.neg_rw, neg[0])
            assert m.pos_rw.shape == ((T + 2 - C) * R * widths[j], C) and m.neg_rw.shape == ((T + 2 - C) * R * K * widths[j], C)
        epochs.append(minis)
        pad = loader.dummy_idx if global_ids else -1
        assert any((m.pos_rw == pad).any() for m in minis) and all((m.neg_rw != pad).all() for m in minis)
    assert not torch.equal(epochs[0][0].pos_rw, epochs[1][0].pos_rw)          # fresh draws in the second epoch ...
    again = mk()
    sbs = list(again.super_batches())
    assert [len(sb) for sb in sbs] == [3, 1] + ([] if drop_last else [1])
    assert [sb.call_id0 for sb in sbs] == [FIRST, FIRST + 3] + ([] if drop_last else [FIRST + 4])
    flat = [(sb.pos_rw[b], sb.neg_rw[b]) for sb in sbs for b in range(len(sb))]
    assert len(flat) == len(epochs[0])
    for (pos, neg), m in zip(flat, epochs[0]):                   # the super-batch views are the per-batch objects
        assert torch.equal(pos, m.pos_rw) and torch.equal(neg, m.neg_rw)
    for m2, m in zip(list(again), epochs[1]):                    # ... which a loader with the same seed reproduces
        assert torch.equal(m2.pos_rw, m.pos_rw) and torch.equal(m2.neg_rw, m.neg_rw)
    assert len(again._graph) == 4                                # one CSR per distinct relation
