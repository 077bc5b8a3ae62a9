"""GPU parity of tg_link_seeds_typed (HIP, C ABI) with the CPU model of tests/helpers_link_typed.py: both rows and the
unverified counts, bit for bit, on the plain int64 view, on the view with u32 shadows and with the edge set; launched into
poisoned buffers whose guard and gap words must keep their poison."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers_link as hl
import helpers_link_typed as ht
import orc
from helpers import load_fake_hetero, load_karate

pytestmark = pytest.mark.gpu
SEED, FIRST = 0x11A4B5, 77
SHAPES = [(1, 1, 1), (5, 3, 5), (50, 2, 3), (64, 1, 2), (130, 1, 2), (7, 0, 3)]   # (E, K, G): 15 and 100 negatives per
TRIES = (1, 2, 8)                                   # mini-batch put its boundaries inside a wave, 64 on a wave edge
MODES = pytest.mark.parametrize("mode", [ht.BINARY, ht.TRIPLET], ids=["binary", "triplet"])
POISON, GUARD = -0x7A7A7A7A7A7A7A7A, 64


@pytest.fixture(scope="module")
def cabi():
    from tch_geometric import _cabi
    return _cabi


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


class _Rel:
    def __init__(self, name, ptrs, idx, n_src, dev, cabi):
        self.name, self.ptrs, self.idx = name, np.asarray(ptrs, dtype=np.int64), np.asarray(idx, dtype=np.int64)
        self.n_src, self.n_dst = n_src, len(ptrs) - 1
        assert self.idx.size == 0 or self.idx.max() < n_src
        self.p_d = torch.from_numpy(np.ascontiguousarray(self.ptrs)).to(dev)
        self.i_d = torch.from_numpy(np.ascontiguousarray(self.idx)).to(dev)
        self.plain = cabi.graph_view(self.p_d, self.i_d)
        self.u32 = cabi.graph_view(self.p_d, self.i_d, indices32=self.i_d.to(torch.int32), ptrs32=self.p_d.to(torch.int32))
        self.edge_set = cabi.edge_set(self.plain, dev)

    def views(self):
        return (("int64", self.plain, None), ("u32", self.u32, None), ("edge set", self.u32, self.edge_set))


@pytest.fixture(scope="module")
def rels(cabi, dev):
    counts, edges = load_fake_hetero()
    fp, fi, _ = orc.to_csc(edges[("v0", "e0", "v2")], (counts["v0"], counts["v2"]))
    row, col = orc.rmat_edges(10, (1 << 10) * 16, 99)
    ei, n = load_karate()
    kp, ki, _ = orc.to_csc(ei, n)
    rp, ri, _ = orc.to_csc(np.stack([row, col]), 1 << 10)
    mk = lambda name, pi, n_src: _Rel(name, pi[0], pi[1], n_src, dev, cabi)
    return {"fake": mk("fake", (fp, fi), counts["v0"]),
            "wide": mk("wide", ht.fold(row, col, 37, 1024), 37), "tall": mk("tall", ht.fold(row, col, 1024, 37), 1024),
            "complete": mk("complete", ht.complete_bipartite(3, 5), 3),
            "punctured": mk("punctured", ht.complete_bipartite(3, 5, without_in_edges_of=0), 3),
            "tiny": mk("tiny", ht.tiny_relation(), ht.TINY_N_SRC), "empty": mk("empty", ht.empty_relation(2), 2),
            "karate": mk("karate", (kp, ki), n), "rmat": mk("rmat", (rp, ri), 1 << 10)}


def _launch(cabi, dev, r, view, edge_set, src, dst, K, mode, tries, same_type=False, call_id=FIRST, gaps=(0, 0), joined=False):
    """-> (src rows, dst rows, unverified) of one launch into poisoned slabs with GUARD words behind them; the guards and the
    words between a row's width and its pitch must stay as they were, every word inside the widths must be written.
    joined: ONE slab of pitch Ws + Wd holds both rows (tg_link_seeds' layout)."""
    G, E = src.shape
    Ws, Wd = ht.widths(E, K, mode)
    sp, dp = (Ws + Wd, Ws + Wd) if joined else (Ws + gaps[0], Wd + gaps[1])
    sbuf = torch.full((G * sp + GUARD,), POISON, dtype=torch.int64, device=dev)
    dbuf = sbuf if joined else torch.full((G * dp + GUARD,), POISON, dtype=torch.int64, device=dev)
    ubuf = torch.full((G + GUARD,), POISON, dtype=torch.int64, device=dev)
    s_view = sbuf[:G * sp].view(G, sp)[:, :Ws]
    d_view = sbuf[:G * sp].view(G, sp)[:, Ws:] if joined else dbuf[:G * dp].view(G, dp)[:, :Wd]
    s_d, d_d = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
    so, do, unv = cabi.link_seeds_typed(view, s_d, d_d, K, mode, tries, SEED, call_id, r.n_src, r.n_dst, same_type,
                                        edge_set=edge_set, src_out=s_view, dst_out=d_view, unverified=ubuf[:G])
    torch.cuda.synchronize()
    assert so.data_ptr() == s_view.data_ptr() and do.data_ptr() == d_view.data_ptr() and unv.data_ptr() == ubuf.data_ptr()
    assert (ubuf[G:] == POISON).all() and not (ubuf[:G] == POISON).any()
    for buf, pitch, width in ((sbuf, sp, sp if joined else Ws), (dbuf, dp, dp if joined else Wd)):
        slab = buf[:G * pitch].view(G, pitch)
        assert (buf[G * pitch:] == POISON).all(), "wrote behind the slab"
        assert (slab[:, width:] == POISON).all(), "wrote between a row's width and its pitch"
        assert not (slab[:, :width] == POISON).any(), "left words of a row unwritten"
    return so.cpu().numpy(), do.cpu().numpy(), unv.cpu().numpy()


def _model(r, src, dst, K, mode, tries, same_type=False, call_id=FIRST, **kw):
    return ht.seed_rows(r.ptrs, r.idx, src, dst, K, mode, tries, SEED, call_id, r.n_src, r.n_dst, same_type, **kw)


def _same(got, want, label=""):
    for g, w, what in zip(got, want, ("src rows", "dst rows", "unverified")):
        assert np.array_equal(g, w), (label, what)


@MODES
@pytest.mark.parametrize("tries", TRIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "E%d-K%d-G%d" % s)
@pytest.mark.parametrize("name", ["fake", "wide", "tall", "complete", "punctured", "tiny"])
def test_rows_equal_the_cpu_model_on_every_view(cabi, dev, rels, name, shape, tries, mode):
    r = rels[name]
    E, K, G = shape
    src, dst = ht.positives(r.ptrs, r.idx, G, E)
    ref = _model(r, src, dst, K, mode, tries)
    if name == "complete" and tries > 1:
        assert ref[2].tolist() == [K * E] * G                    # every try fails: exact, non-zero counts
    if tries == 1:
        assert not ref[2].any()
    for label, view, es in r.views():
        _same(_launch(cabi, dev, r, view, es, src, dst, K, mode, tries), ref, label)


@MODES
def test_punctured_graph_counts_are_non_zero_and_partial(cabi, dev, rels, mode):
    r = rels["punctured"]
    src, dst = ht.positives(r.ptrs, r.idx, 3, 50)
    got = _launch(cabi, dev, r, r.u32, None, src, dst, 2, mode, 2)
    assert ((got[2] > 0) & (got[2] < 100)).all()                 # tests/test_link_seeds_typed_cpu.py shows the model's are
    _same(got, _model(r, src, dst, 2, mode, 2))


@MODES
def test_column_ends_and_short_columns(cabi, dev, rels, mode):
    """the case whose look-ups tests/test_link_seeds_typed_cpu.py shows to reach columns of length 0 and 1 and both ends"""
    r = rels["tiny"]
    src, dst = ht.positives(r.ptrs, r.idx, 3, 50)
    ref = _model(r, src, dst, 2, mode, 8)
    for label, view, es in r.views():
        _same(_launch(cabi, dev, r, view, es, src, dst, 2, mode, 8), ref, label)


def test_equal_ids_of_two_types_stay_eligible(cabi, dev, rels):
    r = rels["empty"]
    src, dst = ht.positives(r.ptrs, r.idx, 2, 50)
    first = []
    ref0 = _model(r, src, dst, 2, ht.BINARY, 8, first=first)
    assert any(s == d for s, d in first)
    for label, view, es in r.views():
        s0, d0, u0 = got0 = _launch(cabi, dev, r, view, es, src, dst, 2, ht.BINARY, 8)
        _same(got0, ref0, label)
        assert [tuple(x) for x in np.stack([s0[:, 50:].ravel(), d0[:, 50:].ravel()], 1)] == first   # attempt 0's, all of them
        assert not u0.any()
        s1, d1, u1 = got1 = _launch(cabi, dev, r, view, es, src, dst, 2, ht.BINARY, 8, same_type=True)
        _same(got1, _model(r, src, dst, 2, ht.BINARY, 8, same_type=True), label)
        differ = ((s0 != s1) | (d0 != d1))[:, 50:]
        assert np.array_equal(differ, np.array([s == d for s, d in first]).reshape(2, 100))         # exactly where s == d


@MODES
@pytest.mark.parametrize("tries", [1, 8])
@pytest.mark.parametrize("name", ["karate", "rmat"])
def test_same_type_joined_layout_is_tg_link_seeds(cabi, dev, rels, name, tries, mode):
    r = rels[name]
    for E, K, G in ((5, 3, 5), (130, 1, 2)):
        src, dst = ht.positives(r.ptrs, r.idx, G, E)
        ref_rows, ref_unv = hl.seed_rows(r.ptrs, r.idx, src, dst, K, mode, tries, SEED, FIRST, r.n_dst)
        s_d, d_d = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
        for label, view, es in r.views():
            rows, unv = cabi.link_seeds(view, s_d, d_d, K, mode, tries, SEED, FIRST, r.n_dst, edge_set=es)
            so, do, unv_t = _launch(cabi, dev, r, view, es, src, dst, K, mode, tries, same_type=True, joined=True)
            got = ht.joined(so, do)
            assert np.array_equal(got, rows.cpu().numpy()) and np.array_equal(unv_t, unv.cpu().numpy()), label
            assert np.array_equal(got, ref_rows) and np.array_equal(unv_t, ref_unv), label


@MODES
def test_pitches_wider_than_the_rows(cabi, dev, rels, mode):
    r = rels["fake"]
    src, dst = ht.positives(r.ptrs, r.idx, 5, 5)
    _same(_launch(cabi, dev, r, r.u32, None, src, dst, 3, mode, 8, gaps=(3, 5)), _model(r, src, dst, 3, mode, 8))


@MODES
@pytest.mark.parametrize("name", ["fake", "wide"])
def test_call_g_of_a_launch_is_a_launch_of_its_own(cabi, dev, rels, name, mode):
    r = rels[name]
    src, dst = ht.positives(r.ptrs, r.idx, 5, 5)
    so, do, unv = _launch(cabi, dev, r, r.u32, r.edge_set, src, dst, 3, mode, 8)
    for b in range(5):
        s1, d1, u1 = _launch(cabi, dev, r, r.u32, r.edge_set, src[b:b + 1], dst[b:b + 1], 3, mode, 8, call_id=FIRST + b)
        assert np.array_equal(s1[0], so[b]) and np.array_equal(d1[0], do[b]) and u1[0] == unv[b]


def test_unverified_may_be_null_and_empty_launches_write_nothing(cabi, dev, rels):
    r = rels["fake"]
    src, dst = ht.positives(r.ptrs, r.idx, 2, 5)
    ref = _model(r, src, dst, 1, ht.BINARY, 8)
    s_d, d_d = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
    so = torch.full((2, 10), POISON, dtype=torch.int64, device=dev)
    do = torch.full((2, 10), POISON, dtype=torch.int64, device=dev)
    rel, rng = cabi.link_rel(r.plain, r.n_src, r.n_dst, False), cabi.TgRng(SEED, FIRST)
    call = lambda G, E: cabi.lib.tg_link_seeds_typed(
        C.byref(rel), cabi.ptr(s_d), cabi.ptr(d_d), C.c_int64(G), C.c_int64(E), C.c_int64(1), C.c_int32(0), C.c_int32(8),
        C.byref(rng), cabi.ptr(so), C.c_int64(10), cabi.ptr(do), C.c_int64(10), None, cabi.stream_ptr(dev))
    assert call(0, 5) == 0 and call(2, 0) == 0
    torch.cuda.synchronize()
    assert (so == POISON).all() and (do == POISON).all()
    assert call(2, 5) == 0
    torch.cuda.synchronize()
    assert np.array_equal(so.cpu().numpy(), ref[0]) and np.array_equal(do.cpu().numpy(), ref[1])
