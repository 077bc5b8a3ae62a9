"""tg_link_seeds_typed's host side (no GPU): the CPU model of the typed seed rule (helpers_link_typed) against the
homogeneous model and on the fixtures the GPU test uses, and the argument errors the library refuses before any launch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers_link as hl
import helpers_link_typed as ht
import orc
from helpers import load_karate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000                      # a non-null address nothing dereferences: every call below is refused or launches nothing
SEED, FIRST = 0x11A4B5, 77         # what tests/test_gpu_link_seeds_typed.py launches with
MODES = [ht.BINARY, ht.TRIPLET]


# ---- the model --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tries", [1, 2, 8])
def test_same_type_on_a_square_graph_is_the_homogeneous_model(mode, tries):
    ei, n = load_karate()
    ptrs, idx, _ = orc.to_csc(ei, n)
    for E, K, G in ((5, 3, 5), (50, 2, 3), (7, 0, 3)):
        src, dst = ht.positives(ptrs, idx, G, E)
        rows, unv = hl.seed_rows(ptrs, idx, src, dst, K, mode, tries, SEED, FIRST, n)
        srows, drows, unv_t = ht.seed_rows(ptrs, idx, src, dst, K, mode, tries, SEED, FIRST, n, n, True)
        assert np.array_equal(ht.joined(srows, drows), rows) and np.array_equal(unv_t, unv)
        assert np.array_equal(ht.pairs(srows, drows, E, K, mode), hl.pairs(rows, E, K, mode))


@pytest.mark.parametrize("mode", MODES)
def test_complete_bipartite_graph_exhausts_every_negative(mode):
    ptrs, idx = ht.complete_bipartite(3, 5)
    for E, K, G in ((5, 3, 5), (50, 2, 3), (130, 1, 2)):
        src, dst = ht.positives(ptrs, idx, G, E)
        for tries in (2, 8):
            assert ht.seed_rows(ptrs, idx, src, dst, K, mode, tries, SEED, FIRST, 3, 5, False)[2].tolist() == [K * E] * G


@pytest.mark.parametrize("mode", MODES)
def test_punctured_graph_counts_are_partial_in_every_mini_batch(mode):
    ptrs, idx = ht.complete_bipartite(3, 5, without_in_edges_of=0)
    src, dst = ht.positives(ptrs, idx, 3, 50)
    unv = ht.seed_rows(ptrs, idx, src, dst, 2, mode, 2, SEED, FIRST, 3, 5, False)[2]
    assert ((unv > 0) & (unv < 100)).all()


def test_empty_square_relation_draws_equal_ids():
    ptrs, idx = ht.empty_relation(2)
    src, dst = ht.positives(ptrs, idx, 2, 50)
    first = []
    s0, d0, unv0 = ht.seed_rows(ptrs, idx, src, dst, 2, ht.BINARY, 8, SEED, FIRST, 2, 2, False, first=first)
    assert any(s == d for s, d in first) and any(s != d for s, d in first)
    assert not unv0.any()
    assert [tuple(x) for x in np.stack([s0[:, 50:].ravel(), d0[:, 50:].ravel()], 1)] == first    # attempt 0 is kept
    s1, d1, _ = ht.seed_rows(ptrs, idx, src, dst, 2, ht.BINARY, 8, SEED, FIRST, 2, 2, True)
    differ = (s0 != s1) | (d0 != d1)
    equal0 = np.array([s == d for s, d in first]).reshape(2, 100)
    assert not differ[:, :50].any() and np.array_equal(differ[:, 50:], equal0)                   # exactly there
    assert (s1[:, 50:] != d1[:, 50:]).mean() > 0.9                                               # and hardly any are left


@pytest.mark.parametrize("mode", MODES)
def test_tiny_relation_trace_reaches_the_column_ends(mode):
    ptrs, idx = ht.tiny_relation()
    deg = np.diff(ptrs)
    assert sorted(set(deg.tolist())) == [0, 1, 2, 3, 7]
    src, dst = ht.positives(ptrs, idx, 3, 50)
    trace = []
    ht.seed_rows(ptrs, idx, src, dst, 2, mode, 8, SEED, FIRST, ht.TINY_N_SRC, ht.TINY_N_DST, False, trace=trace)
    first = lambda d: idx[ptrs[d]]
    last = lambda d: idx[ptrs[d + 1] - 1]
    assert any(deg[d] == 0 for s, d in trace) and any(deg[d] == 1 for s, d in trace)
    assert any(deg[d] == 1 and s == first(d) for s, d in trace)
    assert any(deg[d] >= 2 and s == first(d) for s, d in trace) and any(deg[d] >= 2 and s == last(d) for s, d in trace)
    assert any(deg[d] >= 2 and s < first(d) for s, d in trace) and any(deg[d] >= 2 and s > last(d) for s, d in trace)
    assert any(s == d for s, d in trace)                         # equal ids of two types are looked up like any other pair


def test_ranges_are_not_swapped_in_the_model():
    ptrs, idx = ht.empty_relation(1024)
    src, dst = ht.positives(ptrs, idx, 1, 64)
    s, d, _ = ht.seed_rows(ptrs, idx, src, dst, 1, ht.BINARY, 1, SEED, FIRST, 37, 1024, False)
    assert s.max() < 37 <= d[:, 64:].max() < 1024


# ---- the library's refusals ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cabi():
    pkg = os.path.join(ROOT, "tch-geometric_amd")
    if not os.path.exists(os.path.join(pkg, "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", pkg, "-s"])
    subprocess.check_call([sys.executable, os.path.join(pkg, "host", "build_host.py")])   # a no-op when up to date
    from tch_geometric import _cabi
    return _cabi


def fake_graph(cabi, n_major=10, n_edges=20):
    g = cabi.TgGraph()
    g.ptrs, g.indices, g.n_major, g.n_edges = FAKE, FAKE, n_major, n_edges
    return g


def call(cabi, rel=True, graph=None, edge_set=None, edge_set_bytes=0, n_src=7, n_dst=10, same_type=0, src=FAKE, dst=FAKE, G=2,
         E=3, K=1, mode=0, try_count=4, rng=True, src_seeds=FAKE, src_pitch=None, dst_seeds=FAKE + (1 << 20), dst_pitch=None,
         unverified=FAKE):
    lib = cabi.lib
    g = fake_graph(cabi) if graph is None else graph
    r = cabi.TgRng(1, 2)
    P = max(E, 0) * (1 + max(K, 0))
    Ws = P if mode == 0 else max(E, 0)
    lr = cabi.TgLinkRel(C.pointer(g) if g is not False else None, edge_set, edge_set_bytes, n_src, n_dst, same_type)
    rc = lib.tg_link_seeds_typed(C.byref(lr) if rel else None, C.c_void_p(src), C.c_void_p(dst), C.c_int64(G), C.c_int64(E),
                                 C.c_int64(K), C.c_int32(mode), C.c_int32(try_count), C.byref(r) if rng else None,
                                 C.c_void_p(src_seeds), C.c_int64(Ws if src_pitch is None else src_pitch),
                                 C.c_void_p(dst_seeds), C.c_int64(P if dst_pitch is None else dst_pitch),
                                 C.c_void_p(unverified), None)
    return rc, lib.tg_last_error().decode()


@pytest.mark.parametrize("kw, text", [
    (dict(rel=False), "null rel"),
    (dict(graph=False), "null graph"),
    (dict(rng=False), "null rng"),
    (dict(src=None), "null buffers"),
    (dict(dst=None), "null buffers"),
    (dict(src_seeds=None), "null buffers"),
    (dict(dst_seeds=None), "null buffers"),
    (dict(n_src=0), "n_src"),
    (dict(n_dst=0), "n_dst"),
    (dict(n_dst=11), "n_dst = 11 is not the graph's 10 columns"),
    (dict(n_src=10, n_dst=7), "n_dst = 7 is not the graph's 10 columns"),       # the two ranges swapped
    (dict(same_type=1), "same_type"),
    (dict(src_pitch=5), "src_pitch"),                                           # binary: Ws = P = 6
    (dict(mode=1, src_pitch=2), "src_pitch"),                                   # triplet: Ws = E = 3
    (dict(dst_pitch=5), "dst_pitch"),
    (dict(mode=1, dst_pitch=5), "dst_pitch"),
    (dict(try_count=0), "try_count"),
    (dict(try_count=-3), "try_count"),
    (dict(mode=2), "mode"),
    (dict(mode=-1), "mode"),
    (dict(G=-1), "n_batches"),
    (dict(E=-1), "n_edges"),
    (dict(K=-1), "n_neg"),
    (dict(E=1 << 39, K=1 << 39), "too many"),
    (dict(G=1 << 39, E=1 << 30, K=0), "too many"),
    (dict(edge_set=FAKE, edge_set_bytes=8), "was not built for this graph"),
    (dict(dst_seeds=FAKE + 8 * 3), "overlap"),                                   # inside the first source row
    (dict(dst_seeds=FAKE + 8 * 6, src_pitch=12, dst_pitch=13), "overlap"),       # interleaved, but at two pitches
])
def test_bad_arguments_are_refused_before_any_launch(cabi, kw, text):
    rc, err = call(cabi, **kw)
    assert rc == 1 and "tg_link_seeds_typed" in err and text in err, (rc, err)


def test_graph_without_arrays_and_wide_edge_sets_are_refused(cabi):
    g = fake_graph(cabi)
    g.ptrs = None
    rc, err = call(cabi, graph=g)
    assert rc == 1 and "null graph" in err
    big = 2 ** 32 - 1                                           # the set's 32-bit halves keep 2^32 - 1 for "empty"
    es = dict(edge_set=FAKE, edge_set_bytes=8 * 64)
    rc, err = call(cabi, graph=fake_graph(cabi, big, 20), n_dst=big, **es)
    assert rc == 1 and "2^32 - 1" in err
    rc, err = call(cabi, n_src=big, **es)
    assert rc == 1 and "2^32 - 1" in err
    rc, err = call(cabi, graph=fake_graph(cabi, big - 1, 20), n_src=big - 1, n_dst=big - 1, G=0, **es)
    assert rc == 0, err


def test_empty_launches_return_ok(cabi):
    assert call(cabi, G=0)[0] == 0
    assert call(cabi, E=0)[0] == 0
    assert call(cabi, G=0, src=None, dst=None, src_seeds=None, dst_seeds=None, unverified=None)[0] == 0
    assert call(cabi, n_src=10, same_type=1, E=0)[0] == 0


def test_wrapper_checks_shapes_on_the_host(cabi):
    import torch
    g = fake_graph(cabi)
    src = torch.zeros((2, 3), dtype=torch.int64)
    args = (1, 0, 4, 0, 0, 7, 10, False)
    with pytest.raises(ValueError):
        cabi.link_seeds_typed(g, src, src[:, :2], *args)
    with pytest.raises(ValueError):
        cabi.link_seeds_typed(g, src.to(torch.int32), src.to(torch.int32), *args)
    with pytest.raises(ValueError):
        cabi.link_seeds_typed(g, src, src, *args, src_out=torch.zeros((2, 5), dtype=torch.int64))
    with pytest.raises(ValueError):
        cabi.link_seeds_typed(g, src, src, *args, dst_out=torch.zeros((6, 2), dtype=torch.int64).t())
    with pytest.raises(ValueError):
        cabi.link_seeds_typed(g, src, src, *args, unverified=torch.zeros(3, dtype=torch.int64))
