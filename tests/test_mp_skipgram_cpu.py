"""tg_mp_skipgram's host side (no GPU): the restated walk law against the oracle's random_walk, capacities, form selection
at the documented LDS formula, workspace sizes, every refusal that happens before a launch, and MetaPath2VecLoader's
epoch plan, call ids and PyG fields."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import orc
from helpers import load_karate
from helpers_metapath import walks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 40 * 1024            # tchgeo.h: the LDS forms are taken while TG_MP_SKIPGRAM_LDS_BYTES(L, word) <= 40 KiB
lds = lambda L, word: 64 * (L | 1) * word + 512 + 8 * L   # TG_MP_SKIPGRAM_LDS_BYTES: rows, walker offsets, column starts


@pytest.fixture(scope="module")
def cabi():
    pkg = os.path.join(ROOT, "tch-geometric_amd")
    if not os.path.exists(os.path.join(pkg, "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", pkg, "-s"])
    subprocess.check_call([sys.executable, os.path.join(pkg, "host", "build_host.py")])   # a no-op when up to date
    from tch_geometric import _cabi
    return _cabi


def _cfg(cabi, T=4, Cs=3, R=2, K=1, src=(0, 1), dst=(1, 0), counts=(7, 5), rows=None, starts=None, pad=-1):
    """a config whose graph descriptors carry sizes only (no buffers behind them)"""
    rows = [counts[s] if 0 <= s < len(counts) else 1 for s in src] if rows is None else rows
    return cabi.mp_skipgram_config([cabi.graph_sizing(n, 0) for n in rows], src, dst, counts, T, Cs, R, K, type_start=starts,
                                   pad_value=pad)


@pytest.mark.parametrize("graph", ["karate", "rmat"])
def test_one_step_metapath_is_the_oracles_random_walk(graph):
    """M = 1: the restated law is TAG_RW's with p = q = 1, on a graph without and one with sinks"""
    if graph == "karate":
        ei, n = load_karate()
    else:
        n = 1 << 10
        ei = np.stack(orc.rmat_edges(10, n * 16, 99))
    ptrs, idx, _ = orc.to_csr(ei, n)
    seeds = orc.seed_batches(0x57A27, 0, 1, 9, n).astype(np.int64)[0]
    if graph == "rmat":
        seeds[0] = int(np.flatnonzero(np.diff(ptrs) == 0)[0])
    R, T, seed, call_id = 3, 12, 0x5C1B6A, 44
    mine = walks(seed, call_id, [(ptrs, idx)], [0], [0], seeds, R, T)
    ref = orc.random_walk(ptrs, idx, np.tile(seeds, R), T, 1.0, 1.0, orc.rng_philox(seed, call_id))
    assert np.array_equal(mine, ref)
    if graph == "rmat":
        assert (ref[:, -1] == -1).any() and (ref[:, -1] >= 0).any() and (ref[0, 1:] == -1).all()


def test_capacity_equals_rw_skipgrams(cabi):
    for T, Cs, R, K, B in ((20, 10, 10, 1, 128), (1, 1, 1, 0, 1), (1, 2, 3, 2, 5), (32, 32, 2, 3, 7), (16, 1, 1, 1, 64)):
        ref = cabi.rw_skipgram_capacity(cabi.rw_skipgram_config(T, Cs, R, K, 100), B)
        assert cabi.mp_skipgram_capacity(_cfg(cabi, T, Cs, R, K), B) == ref
        nw = T + 1 - Cs + 1
        assert ref == (nw * R * B, nw * R * K * B)
    assert cabi.mp_skipgram_capacity(_cfg(cabi), 0) == (0, 0)


def test_form_selection_at_the_lds_formula(cabi):
    assert cabi.mp_skipgram_lds_bytes(21, 4) == lds(21, 4)
    for L in (2, 11, 33, 77, 78, 79, 129, 153, 154, 155, 300):
        small = _cfg(cabi, T=L - 1, Cs=1, R=1)
        big = _cfg(cabi, T=L - 1, Cs=1, R=1, counts=(7, 1 << 33), rows=(7, 1 << 33))
        assert cabi.mp_skipgram_form(small) == (1 if lds(L, 4) <= LDS_LIMIT else 2 if lds(L, 8) <= LDS_LIMIT else 3, lds(L, 4))
        assert cabi.mp_skipgram_form(big) == (2 if lds(L, 8) <= LDS_LIMIT else 3, lds(L, 8))
        assert cabi.mp_skipgram_form(small, 1)[0] == 3                      # nothing fits one byte
        assert cabi.mp_skipgram_form(small, lds(L, 4))[0] == 1              # exactly at a caller's limit ...
        assert cabi.mp_skipgram_form(small, lds(L, 4) - 1)[0] == 3          # ... and one byte below it
        assert cabi.mp_skipgram_form(big, lds(L, 8))[0] == 2
        assert cabi.mp_skipgram_form(big, lds(L, 8) - 1)[0] == 3
        # local ids are staged: what counts is the largest type, 0xffffffff stands for an ended walk
        edge = (1 << 32) - 2
        fits = _cfg(cabi, T=L - 1, Cs=1, R=1, counts=(7, edge), rows=(7, edge))
        over = _cfg(cabi, T=L - 1, Cs=1, R=1, counts=(7, edge + 1), rows=(7, edge + 1))
        assert cabi.mp_skipgram_form(fits, lds(L, 4)) == (1, lds(L, 4))
        assert cabi.mp_skipgram_form(over, lds(L, 8)) == (2, lds(L, 8))
        # a large type_start does not change the form
        far = _cfg(cabi, T=L - 1, Cs=1, R=1, starts=(1 << 40, 1 << 41))
        assert cabi.mp_skipgram_form(far, lds(L, 4)) == (1, lds(L, 4))
    # the documented limits: L <= 153 as uint32, L <= 77 as int64
    assert lds(153, 4) <= LDS_LIMIT < lds(154, 4) and lds(77, 8) <= LDS_LIMIT < lds(78, 8)


def test_workspace_bytes(cabi):
    cfg = _cfg(cabi, 20, 10, 10, 1)
    for form in (0, 1, 2):
        assert cabi.mp_skipgram_workspace_bytes(cfg, 4, 128, form) == 0
    assert cabi.mp_skipgram_workspace_bytes(cfg, 4, 128, 3) == 4 * 1280 * 21 * 8
    long_rows = _cfg(cabi, 299, 10, 2, 1)                                     # L = 300: auto is the flat form
    assert cabi.mp_skipgram_workspace_bytes(long_rows, 3, 5, 0) == 3 * 10 * 300 * 8
    assert cabi.mp_skipgram_workspace_bytes(long_rows, 0, 5, 3) == 0
    with pytest.raises(cabi.TchGeoError):
        cabi.mp_skipgram_workspace_bytes(cfg, 4, 128, 4)


def _call(cabi, cfg, G=1, B=1, seeds=None, out=None, rng=True, form=0, ws=None, ws_bytes=0):
    r = cabi.TgRng(1, 2)
    return cabi.lib.tg_mp_skipgram(C.byref(cfg) if cfg is not None else None, seeds, C.c_int64(G), C.c_int64(B),
                                   C.byref(r) if rng else None, out, ws, C.c_int64(ws_bytes), C.c_int32(form), None)


def test_argument_errors_are_refused_before_any_launch(cabi):
    """every one returns TG_ERR_INVALID = 1 (a launch on this GPU-less machine would fail with TG_ERR_HIP = 2)"""
    err = lambda: cabi.lib.tg_last_error().decode()
    pos, neg, nbytes, form = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0)

    def refused(cfg, word):
        assert _call(cabi, cfg) == 1 and word in err(), (word, err())
        assert cabi.lib.tg_mp_skipgram_capacity(C.byref(cfg), C.c_int64(4), C.byref(pos), C.byref(neg)) == 1 and word in err()
        assert cabi.lib.tg_mp_skipgram_form(C.byref(cfg), C.c_int64(0), C.byref(form), C.byref(nbytes)) == 1
        assert cabi.lib.tg_mp_skipgram_workspace_bytes(C.byref(cfg), C.c_int64(1), C.c_int64(1), C.c_int32(0),
                                                       C.byref(nbytes)) == 1

    for bad, word in ((dict(Cs=0), "context_size"), (dict(Cs=6), "context_size"), (dict(R=0), "walks_per_node"),
                      (dict(K=-1), "num_negative_samples"), (dict(T=0), "walk_length")):
        refused(_cfg(cabi, **bad), word)
    refused(_cfg(cabi, src=(), dst=()), "n_steps")                            # M = 0
    refused(_cfg(cabi, src=(0,) * 17, dst=(0,) * 17), "n_steps")              # M = 17
    refused(_cfg(cabi, src=(0, 2), dst=(2, 0)), "step 0")                     # a type index outside [0, n_types)
    refused(_cfg(cabi, src=(0, 1), dst=(1, -1)), "step 1")
    refused(_cfg(cabi, src=(0, 0), dst=(1, 0)), "step 0: broken chain")       # step 0 ends at 1, step 1 starts at 0
    refused(_cfg(cabi, T=3, src=(0, 1), dst=(1, 1)), "step 1: open path")     # 3 steps over an open path of 2
    refused(_cfg(cabi, rows=(7, 6)), "step 1")                                # the CSR of step 1 has 6 rows, its type 5 nodes
    assert "n_major" in err()
    refused(_cfg(cabi, counts=(7, 0), rows=(7, 0)), "type_count[1]")
    refused(_cfg(cabi, counts=(7, 5, 0)), "type_count[2]")                    # also a type the path never visits
    assert _call(cabi, _cfg(cabi, T=2, src=(0, 1), dst=(1, 1)), G=0) == 0     # an open path of 2 walked for 2 steps is fine
    cfg = _cfg(cabi)
    assert _call(cabi, None) == 1 and "null config" in err()
    for field in ("graphs", "step_src", "step_dst", "type_count"):
        broken = _cfg(cabi)
        setattr(broken, field, None)
        assert _call(cabi, broken) == 1 and "null graphs" in err()
    assert _call(cabi, cfg, rng=False) == 1 and "null rng" in err()
    assert _call(cabi, cfg, form=4) == 1 and "form" in err()
    assert _call(cabi, cfg, G=-1) == 1 and _call(cabi, cfg, B=-1) == 1
    assert _call(cabi, cfg, G=1 << 39, B=1 << 39) == 1 and "too large" in err()   # products that leave int64
    assert _call(cabi, cfg) == 1 and "step 0: null graph" in err()
    # descriptors with offsets but no other buffers: the null seeds / outputs are refused before they are looked at
    ptrs = (C.c_int64 * 8)(*([0] * 8))
    views = []
    for n in (7, 5):
        g = cabi.TgGraph()
        g.ptrs, g.n_major, g.n_edges = C.addressof(ptrs), n, 0
        views.append(g)
    mk = lambda **kw: cabi.mp_skipgram_config(views, (0, 1), (1, 0), kw.pop("counts", (7, 5)), kw.pop("T", 4), 3, 2, 1, **kw)
    cfg = mk()
    assert _call(cabi, cfg) == 1 and "null buffers" in err()
    seeds = (C.c_int64 * 1)(0)
    assert _call(cabi, cfg, seeds=seeds) == 1 and "null buffers" in err()
    o = cabi.TgRwSkipgramOut(C.addressof(ptrs), None)                         # K = 1 and no neg_rw
    assert _call(cabi, cfg, seeds=seeds, out=C.byref(o)) == 1 and "null buffers" in err()
    o = cabi.TgRwSkipgramOut(C.addressof(ptrs), C.addressof(ptrs))
    assert _call(cabi, cfg, seeds=seeds, out=C.byref(o), form=3) == 1 and "workspace" in err()
    assert _call(cabi, cfg, seeds=seeds, out=C.byref(o), form=3, ws=seeds, ws_bytes=8) == 1 and "workspace" in err()
    long_rows = mk(T=200)
    assert _call(cabi, long_rows, seeds=seeds, out=C.byref(o), form=1) == 1 and "form 1" in err()
    assert _call(cabi, long_rows, seeds=seeds, out=C.byref(o), form=2) == 1 and "form 2" in err()
    views[1].n_major = 1 << 33                                                # local ids that do not fit 32-bit staging
    assert _call(cabi, mk(counts=(7, 1 << 33)), seeds=seeds, out=C.byref(o), form=1) == 1 and "form 1" in err()


def test_empty_launches_return_ok(cabi):
    cfg = _cfg(cabi)
    assert _call(cabi, cfg, G=0, B=5) == 0
    assert _call(cabi, cfg, G=3, B=0) == 0


def _typed_data():
    import torch
    from tch_geometric.transforms import HeteroGraph
    data = HeteroGraph()
    for t, n in (("a", 40), ("b", 11), ("c", 5)):
        data[t].num_nodes = n
    for et in (("a", "ab", "b"), ("b", "ba", "a"), ("b", "bc", "c"), ("c", "cb", "b"), ("a", "aa", "a")):
        data[et].edge_index = torch.zeros((2, 0), dtype=torch.int64)
    return data


@pytest.mark.parametrize("drop_last", [False, True])
def test_loader_len_plan_and_call_ids(cabi, drop_last):
    import torch
    from tch_geometric import MetaPath2VecLoader
    data = _typed_data()
    path = [("a", "ab", "b"), ("b", "ba", "a")]
    loader = MetaPath2VecLoader(data, path, 6, 3, walks_per_node=2, num_negative_samples=1, input_nodes=torch.arange(23),
                                batch_size=5, prefetch=3, drop_last=drop_last, seed=9, call_id0=100, device="cpu")
    assert len(loader) == (4 if drop_last else 5)
    full = [(0, 3, 5, 100), (15, 1, 5, 103)]
    assert loader.plan(0) == (full if drop_last else full + [(20, 1, 3, 104)])
    n = len(loader)
    assert [x[3] for x in loader.plan(2)] == [100 + 2 * n, 100 + 2 * n + 3] + ([] if drop_last else [100 + 2 * n + 4])
    ids = [cid + g for _, G, _, cid in loader.plan(1) for g in range(G)]     # every mini-batch has its own call id, in order
    assert ids == list(range(100 + n, 100 + 2 * n))
    # prefetch is clamped by the launch's memory: one mini-batch here is (pos + neg rows) * C * 8 bytes
    per = sum(cabi.mp_skipgram_capacity(loader.cfg, 5)) * 3 * 8
    assert per == sum(cabi.rw_skipgram_capacity(cabi.rw_skipgram_config(6, 3, 2, 1, 1), 5)) * 3 * 8
    assert MetaPath2VecLoader(data, path, 6, 3, 2, 1, batch_size=5, prefetch=64, max_workspace_bytes=2 * per).prefetch == 2
    assert MetaPath2VecLoader(data, path, 6, 3, 2, 1, batch_size=5, prefetch=64, max_workspace_bytes=1).prefetch == 1
    assert MetaPath2VecLoader(data, path, 6, 3).input_nodes.numel() == 40    # default: every node of metapath[0][0]


def test_loader_speaks_pygs_conventions(cabi):
    import torch
    from tch_geometric import MetaPath2VecLoader
    data = _typed_data()
    ab, ba, bc, cb, aa = [et for et in data.edge_types]
    loader = MetaPath2VecLoader(data, [ab, bc, cb, ba], 8, 3)
    assert loader.start == {"a": 0, "b": 40, "c": 51} and loader.end == {"a": 40, "b": 51, "c": 56}
    assert loader.dummy_idx == 56 and loader.num_embeddings == 57
    assert loader.cfg.pad_value == 56 and [loader.cfg.type_start[t] for t in range(3)] == [0, 40, 51]
    local = MetaPath2VecLoader(data, [ab, bc, cb, ba], 8, 3, global_ids=False)
    assert local.cfg.pad_value == -1 and not local.cfg.type_start and local.dummy_idx == 56
    with pytest.raises(ValueError, match="step 0: broken chain"):
        MetaPath2VecLoader(data, [ab, ab], 2, 2)
    with pytest.raises(ValueError, match="step 1: open path"):
        MetaPath2VecLoader(data, [ab, bc], 3, 2)
    assert len(MetaPath2VecLoader(data, [ab, bc], 2, 2, batch_size=8)) == 5   # the open path walked once is fine
    with pytest.raises(ValueError, match="step 1"):
        MetaPath2VecLoader(data, [ab, ("b", "nope", "a")], 2, 2)
    with pytest.raises(cabi.TchGeoError):
        MetaPath2VecLoader(data, [ab, ba], 6, 8)                              # context_size > walk_length + 1
    with pytest.raises(IndexError):
        MetaPath2VecLoader(data, [ab, ba], 6, 3, input_nodes=torch.tensor([40]))
    with pytest.raises(IndexError):
        MetaPath2VecLoader(data, [bc, cb], 6, 3, input_nodes=torch.tensor([11]))   # the range is the FIRST type's
