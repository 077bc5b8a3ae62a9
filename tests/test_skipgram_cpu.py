"""tg_rw_skipgram's host side (no GPU): the window rule, capacities, form selection, workspace sizes, argument errors that
are refused before any launch, and Node2VecLoader's epoch plan and call ids."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers_skipgram import windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 40 * 1024            # tchgeo.h: the LDS forms are taken while 64 * (L | 1) * word + 512 <= 40 KiB


@pytest.fixture(scope="module")
def cabi():
    pkg = os.path.join(ROOT, "tch-geometric_amd")
    if not os.path.exists(os.path.join(pkg, "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", pkg, "-s"])
    subprocess.check_call([sys.executable, os.path.join(pkg, "host", "build_host.py")])   # a no-op when up to date
    from tch_geometric import _cabi
    return _cabi


def test_windows_against_a_triple_loop():
    g = np.random.default_rng(3)
    for n, L in ((1, 1), (1, 4), (5, 2), (7, 11), (3, 17)):
        rows = g.integers(-1, 50, (n, L))
        for Cs in sorted(c for c in {1, 2, L - 1, L} if 1 <= c <= L):
            nw = L - Cs + 1
            ref = np.empty((nw * n, Cs), dtype=rows.dtype)
            for j in range(nw):
                for w in range(n):
                    for c in range(Cs):
                        ref[j * n + w, c] = rows[w, j + c]
            assert np.array_equal(windows(rows, Cs), ref)


def test_capacity(cabi):
    for T, Cs, R, K, B in ((20, 10, 10, 1, 128), (1, 1, 1, 0, 1), (1, 2, 3, 2, 5), (32, 32, 2, 3, 7), (16, 1, 1, 1, 64)):
        cfg = cabi.rw_skipgram_config(T, Cs, R, K, 100)
        nw = T + 1 - Cs + 1
        assert cabi.rw_skipgram_capacity(cfg, B) == (nw * R * B, nw * R * K * B)
    assert cabi.rw_skipgram_capacity(cabi.rw_skipgram_config(4, 2, 3, 2, 9), 0) == (0, 0)


def test_form_selection_at_the_lds_limit(cabi):
    lds = lambda L, word: 64 * (L | 1) * word + 512
    for L in (2, 11, 33, 79, 80, 81, 129, 157, 158, 159, 300):
        cfg = cabi.rw_skipgram_config(L - 1, 1, 1, 1, 10)
        small, big = cabi.rw_skipgram_form(cfg, 1000), cabi.rw_skipgram_form(cfg, 1 << 33)
        assert small == (1 if lds(L, 4) <= LDS_LIMIT else 2 if lds(L, 8) <= LDS_LIMIT else 3, lds(L, 4))
        assert big == (2 if lds(L, 8) <= LDS_LIMIT else 3, lds(L, 8))
        assert cabi.rw_skipgram_form(cfg, 1000, 1)[0] == 3                    # nothing fits one byte
        assert cabi.rw_skipgram_form(cfg, 1000, lds(L, 4))[0] == 1            # exactly at a caller's limit ...
        assert cabi.rw_skipgram_form(cfg, 1000, lds(L, 4) - 1)[0] == 3        # ... and one byte below it
        assert cabi.rw_skipgram_form(cfg, (1 << 32) - 2, lds(L, 4))[0] == 1   # the largest id bound 32-bit staging takes
        assert cabi.rw_skipgram_form(cfg, (1 << 32) - 1, lds(L, 8))[0] == 2   # 0xffffffff stands for -1
    # the documented limits: L <= 157 as uint32, L <= 79 as int64, L = 129 inside the 32-bit form
    assert lds(157, 4) <= LDS_LIMIT < lds(158, 4) and lds(79, 8) <= LDS_LIMIT < lds(80, 8)
    assert cabi.rw_skipgram_form(cabi.rw_skipgram_config(128, 5, 1, 1, 10), 1000)[0] == 1


def test_workspace_bytes(cabi):
    cfg = cabi.rw_skipgram_config(20, 10, 10, 1, 1000)
    for form in (0, 1, 2):
        assert cabi.rw_skipgram_workspace_bytes(cfg, 4, 128, 1000, form) == 0
    assert cabi.rw_skipgram_workspace_bytes(cfg, 4, 128, 1000, 3) == 4 * 1280 * 21 * 8
    long_rows = cabi.rw_skipgram_config(299, 10, 2, 1, 1000)                  # L = 300: auto is the flat form
    assert cabi.rw_skipgram_workspace_bytes(long_rows, 3, 5, 1000, 0) == 3 * 10 * 300 * 8
    assert cabi.rw_skipgram_workspace_bytes(long_rows, 0, 5, 1000, 3) == 0
    with pytest.raises(cabi.TchGeoError):
        cabi.rw_skipgram_workspace_bytes(cfg, 4, 128, 1000, 4)


def _call(cabi, cfg, G=1, B=1, graph=None, seeds=None, out=None, rng=True, form=0, ws=None, ws_bytes=0):
    r = cabi.TgRng(1, 2)
    return cabi.lib.tg_rw_skipgram(graph, None, C.c_int64(0), seeds, C.c_int64(G), C.c_int64(B), C.byref(cfg) if cfg else None,
                                   C.byref(r) if rng else None, out, ws, C.c_int64(ws_bytes), C.c_int32(form), None)


def test_argument_errors_are_refused_before_any_launch(cabi):
    """every one returns TG_ERR_INVALID = 1 (a launch on this GPU-less machine would fail with TG_ERR_HIP = 2)"""
    err = lambda: cabi.lib.tg_last_error().decode()
    ok = dict(walk_length=4, context_size=3, walks_per_node=2, num_negative_samples=1, n_nodes=10)
    for bad, word in ((dict(context_size=0), "context_size"), (dict(context_size=6), "context_size"),
                      (dict(walks_per_node=0), "walks_per_node"), (dict(num_negative_samples=-1), "num_negative_samples"),
                      (dict(walk_length=0), "walk_length"), (dict(n_nodes=0), "n_nodes"), (dict(p=0.0), "p and q"),
                      (dict(q=-1.0), "p and q")):
        cfg = cabi.rw_skipgram_config(**dict(ok, **bad))
        assert _call(cabi, cfg) == 1 and word in err(), (bad, err())
        pos, neg = C.c_int64(0), C.c_int64(0)
        assert cabi.lib.tg_rw_skipgram_capacity(C.byref(cfg), C.c_int64(4), C.byref(pos), C.byref(neg)) == 1
    assert _call(cabi, cabi.rw_skipgram_config(**dict(ok, n_nodes=0, num_negative_samples=0)), G=0) == 0   # K = 0 needs no range
    cfg = cabi.rw_skipgram_config(**ok)
    assert _call(cabi, None) == 1 and "null config" in err()
    assert _call(cabi, cfg, rng=False) == 1 and "null rng" in err()
    assert _call(cabi, cfg, form=4) == 1 and "form" in err()
    assert _call(cabi, cfg, G=-1) == 1 and _call(cabi, cfg, B=-1) == 1
    assert _call(cabi, cfg) == 1 and "null graph" in err()
    # a graph without buffers behind it: the null seeds / outputs are refused before it is looked at
    ptrs = (C.c_int64 * 3)(0, 0, 0)
    g = cabi.TgGraph()
    g.ptrs, g.n_major, g.n_edges = C.addressof(ptrs), 2, 0
    assert _call(cabi, cfg, graph=C.byref(g)) == 1 and "null buffers" in err()
    seeds = (C.c_int64 * 1)(0)
    assert _call(cabi, cfg, graph=C.byref(g), seeds=seeds) == 1 and "null buffers" in err()
    o = cabi.TgRwSkipgramOut(C.addressof(ptrs), None)                         # K = 1 and no neg_rw
    assert _call(cabi, cfg, graph=C.byref(g), seeds=seeds, out=C.byref(o)) == 1 and "null buffers" in err()
    o = cabi.TgRwSkipgramOut(C.addressof(ptrs), C.addressof(ptrs))
    assert _call(cabi, cfg, graph=C.byref(g), seeds=seeds, out=C.byref(o), form=3) == 1 and "workspace" in err()
    assert _call(cabi, cfg, graph=C.byref(g), seeds=seeds, out=C.byref(o), form=3, ws=seeds, ws_bytes=8) == 1
    long_rows = cabi.rw_skipgram_config(**dict(ok, walk_length=200))
    assert _call(cabi, long_rows, graph=C.byref(g), seeds=seeds, out=C.byref(o), form=1) == 1 and "form 1" in err()
    assert _call(cabi, long_rows, graph=C.byref(g), seeds=seeds, out=C.byref(o), form=2) == 1 and "form 2" in err()
    g.n_major = 1 << 33                                                       # ids that do not fit 32-bit staging
    assert _call(cabi, cfg, graph=C.byref(g), seeds=seeds, out=C.byref(o), form=1) == 1 and "form 1" in err()


def test_empty_launches_return_ok(cabi):
    cfg = cabi.rw_skipgram_config(4, 3, 2, 1, 10)
    assert _call(cabi, cfg, G=0, B=5) == 0
    assert _call(cabi, cfg, G=3, B=0) == 0


@pytest.mark.parametrize("drop_last", [False, True])
def test_loader_len_plan_and_call_ids(cabi, drop_last):
    import torch
    from tch_geometric import Node2VecLoader
    from tch_geometric.transforms import Graph
    data = Graph(edge_index=torch.zeros((2, 0), dtype=torch.int64), num_nodes=40)
    loader = Node2VecLoader(data, 6, 3, walks_per_node=2, num_negative_samples=1, input_nodes=torch.arange(23), batch_size=5,
                            prefetch=3, drop_last=drop_last, seed=9, call_id0=100)
    assert len(loader) == (4 if drop_last else 5)
    full = [(0, 3, 5, 100), (15, 1, 5, 103)]
    assert loader.plan(0) == (full if drop_last else full + [(20, 1, 3, 104)])
    n = len(loader)
    assert [x[3] for x in loader.plan(2)] == [100 + 2 * n, 100 + 2 * n + 3] + ([] if drop_last else [100 + 2 * n + 4])
    # every mini-batch of an epoch has its own call id, in order
    ids = [cid + g for _, G, _, cid in loader.plan(1) for g in range(G)]
    assert ids == list(range(100 + n, 100 + 2 * n))
    # prefetch is clamped by the launch's memory: one mini-batch here is (pos + neg rows) * C * 8 bytes
    per = sum(cabi.rw_skipgram_capacity(loader.cfg, 5)) * 3 * 8
    assert Node2VecLoader(data, 6, 3, 2, 1, batch_size=5, prefetch=64, max_workspace_bytes=2 * per).prefetch == 2
    assert Node2VecLoader(data, 6, 3, 2, 1, batch_size=5, prefetch=64, max_workspace_bytes=1).prefetch == 1
    with pytest.raises(cabi.TchGeoError):
        Node2VecLoader(data, 6, 8)                                            # context_size > walk_length + 1
    with pytest.raises(IndexError):
        Node2VecLoader(data, 6, 3, input_nodes=torch.tensor([40]))
