"""GPU parity of tg_link_seeds (HIP, C ABI) with the CPU model of tests/helpers_link.py: the seed rows and the unverified
counts, bit for bit, on the plain int64 view, on the view with u32 shadows and with the edge set."""
import numpy as np
import pytest
import torch

import helpers_link as hl
import orc
from helpers import load_karate

pytestmark = pytest.mark.gpu
SEED, FIRST = 0x11A4B5, 77
SHAPES = [(1, 1, 1), (5, 3, 5), (50, 2, 3), (64, 1, 2), (130, 1, 2), (7, 0, 3)]   # (E, K, G): 15 and 100 negatives per
TRIES = (1, 2, 8)                                   # mini-batch put its boundaries inside a wave, 64 on a wave edge
POISON, GUARD = -0x7A7A7A7A7A7A7A7A, 64


@pytest.fixture(scope="module")
def cabi():
    from tch_geometric import _cabi
    return _cabi


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


class _G:
    def __init__(self, name, ptrs, idx, dev, cabi):
        self.name, self.ptrs, self.idx, self.n = name, np.asarray(ptrs), np.asarray(idx), len(ptrs) - 1
        self.p_d = torch.from_numpy(np.ascontiguousarray(self.ptrs)).to(dev)
        self.i_d = torch.from_numpy(np.ascontiguousarray(self.idx)).to(dev)
        self.plain = cabi.graph_view(self.p_d, self.i_d)
        self.u32 = cabi.graph_view(self.p_d, self.i_d, indices32=self.i_d.to(torch.int32), ptrs32=self.p_d.to(torch.int32))
        self.edge_set = cabi.edge_set(self.plain, dev)
        self.deg = np.diff(self.ptrs)

    def views(self):
        return (("int64", self.plain, None), ("u32", self.u32, None), ("edge set", self.u32, self.edge_set))


def tiny_graph():
    """8 nodes: column 0 is empty, column 1 has one entry, the others two to seven, with ids below and above their ends"""
    cols = {1: [3], 2: [3, 5], 3: [1, 2, 4, 6], 4: [0, 7], 5: [2, 3, 4], 6: [0, 1, 2, 3, 4, 5, 7], 7: [1, 3, 5]}
    return hl.csc_of([(s, d) for d, ss in cols.items() for s in ss], 8)


@pytest.fixture(scope="module")
def graphs(cabi, dev):
    ei, n = load_karate()
    kp, ki, _ = orc.to_csc(ei, n)
    n2 = 1 << 10
    row, col = orc.rmat_edges(10, n2 * 16, 99)                   # hub columns (long searches) and many empty columns
    rp, ri, _ = orc.to_csc(np.stack([row, col]), n2)
    mk = lambda name, p, i: _G(name, p, i, dev, cabi)
    return {"karate": mk("karate", kp, ki), "rmat": mk("rmat", rp, ri), "complete": mk("complete", *hl.complete_graph(6)),
            "punctured": mk("punctured", *hl.complete_graph(6, without_in_edges_of=0)), "tiny": mk("tiny", *tiny_graph())}


def _positives(g, G, E):
    """[G, E] edges of the graph (CSC positions drawn with a fixed generator) as (src, dst)"""
    r = np.random.default_rng(1000 * G + E)
    pos = r.integers(0, len(g.idx), (G, E))
    return g.idx[pos].astype(np.int64), (np.searchsorted(g.ptrs, pos, side="right") - 1).astype(np.int64)


def _launch(cabi, dev, g, view, edge_set, src, dst, K, mode, tries, call_id=FIRST):
    """-> (rows, unverified) of one launch into poisoned slabs with GUARD words behind them, which must stay as they were"""
    G, E = src.shape
    S, _ = hl.capacity(E, K, mode)
    buf = torch.full((G * S + GUARD,), POISON, dtype=torch.int64, device=dev)
    ubuf = torch.full((G + GUARD,), POISON, dtype=torch.int64, device=dev)
    s_d, d_d = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
    rows, unv = cabi.link_seeds(view, s_d, d_d, K, mode, tries, SEED, call_id, g.n, edge_set=edge_set,
                                out=buf[:G * S].view(G, S), unverified=ubuf[:G])
    torch.cuda.synchronize()
    assert rows.data_ptr() == buf.data_ptr() and unv.data_ptr() == ubuf.data_ptr()
    assert (buf[G * S:] == POISON).all() and (ubuf[G:] == POISON).all(), "wrote behind the slab"
    assert not (buf[:G * S] == POISON).any() and not (ubuf[:G] == POISON).any(), "left words of the slab unwritten"
    return rows.cpu().numpy(), unv.cpu().numpy()


@pytest.mark.parametrize("mode", [hl.BINARY, hl.TRIPLET], ids=["binary", "triplet"])
@pytest.mark.parametrize("tries", TRIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "E%d-K%d-G%d" % s)
@pytest.mark.parametrize("name", ["karate", "complete", "punctured", "rmat"])
def test_rows_equal_the_cpu_model_on_every_view(cabi, dev, graphs, name, shape, tries, mode):
    g = graphs[name]
    E, K, G = shape
    src, dst = _positives(g, G, E)
    ref_rows, ref_unv = hl.seed_rows(g.ptrs, g.idx, src, dst, K, mode, tries, SEED, FIRST, g.n)
    if name == "complete" and tries > 1:
        assert ref_unv.tolist() == [K * E] * G                   # every try fails: exact, non-zero counts
    if tries == 1:
        assert not ref_unv.any()
    for label, view, es in g.views():
        rows, unv = _launch(cabi, dev, g, view, es, src, dst, K, mode, tries)
        assert np.array_equal(rows, ref_rows), label
        assert np.array_equal(unv, ref_unv), label


@pytest.mark.parametrize("mode", [hl.BINARY, hl.TRIPLET], ids=["binary", "triplet"])
def test_punctured_graph_counts_are_non_zero_and_partial(cabi, dev, graphs, mode):
    g = graphs["punctured"]
    src, dst = _positives(g, 3, 50)
    rows, unv = _launch(cabi, dev, g, g.u32, None, src, dst, 2, mode, 2)
    assert ((unv > 0) & (unv < 100)).all()                       # some negatives found node 0 in two tries, some did not
    assert np.array_equal(unv, hl.seed_rows(g.ptrs, g.idx, src, dst, 2, mode, 2, SEED, FIRST, g.n)[1])


@pytest.mark.parametrize("mode", [hl.BINARY, hl.TRIPLET], ids=["binary", "triplet"])
def test_column_ends_and_short_columns(cabi, dev, graphs, mode):
    """the look-ups of this case hit a column's first and last entry and columns of length 0 and 1 (shown by the model's
    trace), and the rows still equal the model's on every view"""
    g = graphs["tiny"]
    src, dst = _positives(g, 3, 50)
    trace = []
    ref_rows, ref_unv = hl.seed_rows(g.ptrs, g.idx, src, dst, 2, mode, 8, SEED, FIRST, g.n, trace=trace)
    first = lambda d: g.idx[g.ptrs[d]]
    last = lambda d: g.idx[g.ptrs[d + 1] - 1]
    assert any(g.deg[d] == 0 for s, d in trace) and any(g.deg[d] == 1 for s, d in trace)
    assert any(g.deg[d] == 1 and s == first(d) for s, d in trace)
    assert any(g.deg[d] >= 2 and s == first(d) for s, d in trace)
    assert any(g.deg[d] >= 2 and s == last(d) for s, d in trace)
    assert any(g.deg[d] >= 2 and s < first(d) for s, d in trace) and any(g.deg[d] >= 2 and s > last(d) for s, d in trace)
    for label, view, es in g.views():
        rows, unv = _launch(cabi, dev, g, view, es, src, dst, 2, mode, 8)
        assert np.array_equal(rows, ref_rows) and np.array_equal(unv, ref_unv), label


@pytest.mark.parametrize("mode", [hl.BINARY, hl.TRIPLET], ids=["binary", "triplet"])
@pytest.mark.parametrize("name", ["karate", "rmat"])
def test_call_g_of_a_launch_is_a_launch_of_its_own(cabi, dev, graphs, name, mode):
    g = graphs[name]
    src, dst = _positives(g, 5, 5)
    rows, unv = _launch(cabi, dev, g, g.u32, g.edge_set, src, dst, 3, mode, 8)
    for b in range(5):
        r1, u1 = _launch(cabi, dev, g, g.u32, g.edge_set, src[b:b + 1], dst[b:b + 1], 3, mode, 8, call_id=FIRST + b)
        assert np.array_equal(r1[0], rows[b]) and u1[0] == unv[b]


def test_unverified_may_be_null_and_empty_launches_write_nothing(cabi, dev, graphs):
    import ctypes as C
    g = graphs["karate"]
    src, dst = _positives(g, 2, 5)
    ref, _ = hl.seed_rows(g.ptrs, g.idx, src, dst, 1, hl.BINARY, 8, SEED, FIRST, g.n)
    s_d, d_d = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
    out = torch.full((2, 20), POISON, dtype=torch.int64, device=dev)
    rng = cabi.TgRng(SEED, FIRST)
    call = lambda G, E: cabi.lib.tg_link_seeds(
        C.byref(g.plain), None, C.c_int64(0), cabi.ptr(s_d), cabi.ptr(d_d), C.c_int64(G), C.c_int64(E), C.c_int64(1),
        C.c_int32(0), C.c_int32(8), C.byref(rng), C.c_int64(g.n), cabi.ptr(out), None, cabi.stream_ptr(dev))
    assert call(0, 5) == 0 and call(2, 0) == 0
    torch.cuda.synchronize()
    assert (out == POISON).all()
    assert call(2, 5) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)
