"""tg_link_seeds' host side (no GPU): the shapes, the argument errors that are refused before any launch, and the CPU
model of the seed rule (helpers_link) on graphs whose answers are known."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers_link as hl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000                      # a non-null address nothing dereferences: every call below is refused or launches nothing


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


def call(cabi, graph=None, edge_set=None, edge_set_bytes=0, src=FAKE, dst=FAKE, G=2, E=3, K=1, mode=0, try_count=4, rng=True,
         n_nodes=10, seeds=FAKE, unverified=FAKE):
    lib = cabi.lib
    g = fake_graph(cabi) if graph is None else graph
    r = cabi.TgRng(1, 2)
    rc = lib.tg_link_seeds(C.byref(g) if g is not False else None, C.c_void_p(edge_set), C.c_int64(edge_set_bytes),
                           C.c_void_p(src), C.c_void_p(dst), C.c_int64(G), C.c_int64(E), C.c_int64(K), C.c_int32(mode),
                           C.c_int32(try_count), C.byref(r) if rng else None, C.c_int64(n_nodes), C.c_void_p(seeds),
                           C.c_void_p(unverified), None)
    return rc, lib.tg_last_error().decode()


def test_capacity(cabi):
    for E, K in ((1, 1), (5, 3), (50, 2), (64, 1), (130, 1), (7, 0), (0, 4), (1024, 1)):
        P = E + K * E
        assert cabi.link_seeds_capacity(E, K, cabi.LINK_BINARY) == (2 * P, P) == hl.capacity(E, K, hl.BINARY)
        assert cabi.link_seeds_capacity(E, K, cabi.LINK_TRIPLET) == (E * (2 + K), P) == hl.capacity(E, K, hl.TRIPLET)
    S, P = C.c_int64(), C.c_int64()
    lib = cabi.lib
    assert lib.tg_link_seeds_capacity(C.c_int64(4), C.c_int64(1), C.c_int32(2), C.byref(S), C.byref(P)) == 1
    assert b"mode" in lib.tg_last_error()
    assert lib.tg_link_seeds_capacity(C.c_int64(-1), C.c_int64(1), C.c_int32(0), C.byref(S), C.byref(P)) == 1
    assert b"n_edges" in lib.tg_last_error()
    assert lib.tg_link_seeds_capacity(C.c_int64(4), C.c_int64(-1), C.c_int32(0), C.byref(S), C.byref(P)) == 1
    assert b"n_neg" in lib.tg_last_error()
    assert lib.tg_link_seeds_capacity(C.c_int64(4), C.c_int64(1), C.c_int32(0), None, C.byref(P)) == 1
    assert b"null output" in lib.tg_last_error()


@pytest.mark.parametrize("kw, text", [
    (dict(graph=False), "null graph"),
    (dict(src=None), "null buffers"),
    (dict(dst=None), "null buffers"),
    (dict(seeds=None), "null buffers"),
    (dict(rng=False), "null rng"),
    (dict(G=-1), "n_batches"),
    (dict(E=-1), "n_edges"),
    (dict(K=-1), "n_neg"),
    (dict(try_count=0), "try_count"),
    (dict(try_count=-3), "try_count"),
    (dict(mode=2), "mode"),
    (dict(mode=-1), "mode"),
    (dict(n_nodes=0), "n_nodes"),
    (dict(n_nodes=11), "n_nodes = 11 is not the graph's 10 columns"),
    (dict(edge_set=FAKE, edge_set_bytes=8), "was not built for this graph"),
])
def test_bad_arguments_are_refused_before_any_launch(cabi, kw, text):
    rc, err = call(cabi, **kw)
    assert rc == 1 and text in err, (rc, err)


def test_graph_without_arrays_and_wide_edge_set_are_refused(cabi):
    g = fake_graph(cabi)
    g.ptrs = None
    rc, err = call(cabi, graph=g)
    assert rc == 1 and "null graph" in err
    big = 2 ** 32 - 1                                           # the set's 32-bit halves keep 2^32 - 1 for "empty"
    rc, err = call(cabi, graph=fake_graph(cabi, big, 20), n_nodes=big, edge_set=FAKE, edge_set_bytes=8 * 64)
    assert rc == 1 and "2^32 - 1" in err
    rc, err = call(cabi, graph=fake_graph(cabi, big - 1, 20), n_nodes=big - 1, edge_set=FAKE, edge_set_bytes=8 * 64, G=0)
    assert rc == 0, err


def test_empty_launches_return_ok(cabi):
    assert call(cabi, G=0)[0] == 0
    assert call(cabi, E=0)[0] == 0
    assert call(cabi, G=0, src=None, dst=None, seeds=None, unverified=None)[0] == 0


def test_wrapper_checks_shapes_on_the_host(cabi):
    import torch
    g = fake_graph(cabi)
    src = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(ValueError):
        cabi.link_seeds(g, src, src[:, :2], 1, 0, 4, 0, 0, 10)
    with pytest.raises(ValueError):
        cabi.link_seeds(g, src.to(torch.int32), src.to(torch.int32), 1, 0, 4, 0, 0, 10)
    with pytest.raises(ValueError):
        cabi.link_seeds(g, src, src, 1, 0, 4, 0, 0, 10, out=torch.zeros((2, 11), dtype=torch.int64))
    with pytest.raises(ValueError):
        cabi.link_seeds(g, src, src, 1, 0, 4, 0, 0, 10, unverified=torch.zeros(3, dtype=torch.int64))


# ---- the CPU model ---------------------------------------------------------------------------------------------------------
def ring(n=12):
    return hl.csc_of([(i, (i + 1) % n) for i in range(n)] + [(i, (i + 3) % n) for i in range(n)], n)


@pytest.mark.parametrize("mode", [hl.BINARY, hl.TRIPLET])
def test_one_try_keeps_the_raw_draws(mode):
    ptrs, idx = ring()
    src, dst = np.array([[0, 1, 2], [3, 4, 5]]), np.array([[1, 2, 3], [4, 5, 6]])
    K, E = 2, 3
    rows, unv = hl.seed_rows(ptrs, idx, src, dst, K, mode, 1, 7, 100, 12)
    assert not unv.any()
    S, P = hl.capacity(E, K, mode)
    assert rows.shape == (2, S)
    for g in range(2):
        for u in range(K * E):
            c0, c1 = hl.candidates(7, 100 + g, u, 0, 12)
            if mode == hl.BINARY:
                assert (rows[g, E + u], rows[g, P + E + u]) == (c0, c1)
            else:
                assert rows[g, 2 * E + u] == c0
    pr = hl.pairs(rows, E, K, mode)
    assert np.array_equal(pr[:, 0, :E], src) and np.array_equal(pr[:, 1, :E], dst)
    if mode == hl.TRIPLET:
        assert np.array_equal(pr[:, 0, E:], np.repeat(src, K, axis=1))


@pytest.mark.parametrize("mode", [hl.BINARY, hl.TRIPLET])
@pytest.mark.parametrize("tries", [2, 8])
def test_kept_negatives_are_non_edges_or_counted(mode, tries):
    ptrs, idx = ring()
    edges = {(int(s), d) for d in range(12) for s in idx[ptrs[d]:ptrs[d + 1]]}
    g = np.random.default_rng(5)
    src, dst = g.integers(0, 12, (3, 10)), g.integers(0, 12, (3, 10))
    K, E = 3, 10
    rows, unv = hl.seed_rows(ptrs, idx, src, dst, K, mode, tries, 11, 0, 12)
    pr = hl.pairs(rows, E, K, mode)
    for b in range(3):
        bad = sum(1 for s, d in zip(pr[b, 0, E:], pr[b, 1, E:]) if s == d or (int(s), int(d)) in edges)
        assert bad <= unv[b]                # an exhausted slot keeps its last candidate, which may happen to be a non-edge
    # the same count, derived attempt by attempt
    for b in range(3):
        n = 0
        for u in range(K * E):
            ok = False
            for a in range(tries):
                c0, c1 = hl.candidates(11, b, u, a, 12)
                s, d = (c0, c1) if mode == hl.BINARY else (int(src[b, u // K]), c0)
                if s != d and (s, d) not in edges:
                    ok = True
                    break
            n += not ok
        assert n == unv[b]


@pytest.mark.parametrize("mode", [hl.BINARY, hl.TRIPLET])
def test_complete_graph_exhausts_every_negative(mode):
    ptrs, idx = hl.complete_graph(6)
    src, dst = np.array([[0, 1, 2, 3], [4, 5, 0, 1]]), np.array([[1, 2, 3, 4], [5, 0, 1, 2]])
    rows, unv = hl.seed_rows(ptrs, idx, src, dst, 3, mode, 4, 1, 0, 6)
    assert unv.tolist() == [12, 12]
    for b in range(2):                                          # the last attempt's candidate is what stays
        for u in range(12):
            c0, c1 = hl.candidates(1, b, u, 3, 6)
            assert rows[b, (4 + u, 2 * 4 + u)[mode]] == c0
            if mode == hl.BINARY:
                assert rows[b, 16 + 4 + u] == c1


@pytest.mark.parametrize("mode", [hl.BINARY, hl.TRIPLET])
def test_verified_negatives_of_the_punctured_graph_point_at_node_0(mode):
    ptrs, idx = hl.complete_graph(6, without_in_edges_of=0)
    assert ptrs[1] == 0 and len(idx) == 25
    src, dst = np.array([[1, 2, 3, 4, 5, 1, 2, 3]]), np.array([[2, 3, 4, 5, 1, 3, 4, 5]])
    K, E, tries = 4, 8, 6
    rows, unv = hl.seed_rows(ptrs, idx, src, dst, K, mode, tries, 3, 9, 6)
    pr = hl.pairs(rows, E, K, mode)[0]
    verified = 0
    for u in range(K * E):
        accepted = False
        for a in range(tries):
            c0, c1 = hl.candidates(3, 9, u, a, 6)
            s, d = (c0, c1) if mode == hl.BINARY else (int(src[0, u // K]), c0)
            if s != d and d == 0:
                accepted = True
                break
        if accepted:
            verified += 1
            assert pr[1, E + u] == 0 and pr[0, E + u] != 0
    assert verified == K * E - unv[0] and 0 < verified
