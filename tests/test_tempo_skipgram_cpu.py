"""tg_tempo_skipgram's host side (no GPU): capacities, the workgroup tile and its LDS bytes at the header's formula, every
refusal that happens before a launch, empty launches, the exports, and TemporalWalkLoader's epoch plan, call ids and
constructor errors."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 3                               # tchgeo.h TG_ERR_INVALID, TG_ERR_UNSUPPORTED
lds = lambda L, walkers: walkers * (((2 * L) | 1) + 1) * 8   # TG_TEMPO_SKIPGRAM_LDS_BYTES: per walker an offset and a [node | ts] row
TILE_LDS, ONE_LDS, MAX_TILE = 16 * 1024, 64 * 1024, 4     # tchgeo.h: the tile halves past 16 KiB, one walker may take 64 KiB


@pytest.fixture(scope="module")
def cabi():
    pkg = os.path.join(ROOT, "tch-geometric_amd")
    if not os.path.exists(os.path.join(pkg, "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", pkg, "-s"])
    subprocess.check_call([sys.executable, os.path.join(pkg, "host", "build_host.py")])   # a no-op when up to date
    from tch_geometric import _cabi
    return _cabi


def _cfg(cabi, L=5, Cs=3, R=2, K=1, n_nodes=10, window=(0, 4)):
    return cabi.tempo_skipgram_config(L, Cs, window, R, K, n_nodes)


def test_capacity(cabi):
    for L, Cs, R, K, B in ((20, 10, 10, 1, 128), (1, 1, 1, 0, 1), (2, 2, 3, 2, 5), (33, 33, 2, 3, 7), (17, 1, 1, 1, 64)):
        nw = L - Cs + 1
        assert cabi.tempo_skipgram_capacity(_cfg(cabi, L, Cs, R, K), B) == (nw * R * B, nw * R * K * B)
        if L > 1:                                         # the same rows as tg_rw_skipgram with T = L - 1 steps
            assert cabi.tempo_skipgram_capacity(_cfg(cabi, L, Cs, R, K), B) == \
                cabi.rw_skipgram_capacity(cabi.rw_skipgram_config(L - 1, Cs, R, K, 10), B)
    assert cabi.tempo_skipgram_capacity(_cfg(cabi), 0) == (0, 0)


def _expected_tile(L):
    tile = MAX_TILE
    while tile > 1 and lds(L, tile) > TILE_LDS:
        tile //= 2
    return tile


def test_lds_bytes_and_the_workgroup_tile(cabi):
    assert (lds(20, 4), lds(255, 4), lds(256, 2), lds(4095, 1)) == (1344, 16384, 8224, 65536)   # the formula, pinned
    assert cabi.tempo_skipgram_lds_bytes(_cfg(cabi, 20, 10)) == (4, 1344)
    assert cabi.tempo_skipgram_lds_bytes(_cfg(cabi, 1, 1)) == (4, 4 * 4 * 8)
    # the documented steps: 4 walkers to L = 255, 2 to 511, one to 4095
    for L, tile in ((63, 4), (255, 4), (256, 2), (511, 2), (512, 1), (1000, 1), (4095, 1)):
        assert cabi.tempo_skipgram_lds_bytes(_cfg(cabi, L, 1)) == (tile, lds(L, tile)), L
    prev_tile, prev_row, seen = MAX_TILE, 0, set()
    for L in range(1, 4096):
        tile, nbytes = cabi.tempo_skipgram_lds_bytes(_cfg(cabi, L, 1))
        assert tile == _expected_tile(L) and nbytes == lds(L, tile)
        assert tile <= prev_tile and nbytes // tile > prev_row       # monotone in L: fewer walkers, longer rows
        assert nbytes <= (TILE_LDS if tile > 1 else ONE_LDS)
        prev_tile, prev_row = tile, nbytes // tile
        seen.add(tile)
    assert seen == {4, 2, 1} and prev_tile == 1               # down to one walker before the first refusal ...
    walkers, nbytes = C.c_int32(-1), C.c_int64(-1)
    first_refused = _cfg(cabi, 4096, 1)
    assert lds(4096, 1) > ONE_LDS
    assert cabi.lib.tg_tempo_skipgram_lds_bytes(C.byref(first_refused), C.byref(walkers), C.byref(nbytes)) == UNSUPPORTED
    assert "walk_length 4096" in cabi.lib.tg_last_error().decode()
    assert _call(cabi, first_refused) == UNSUPPORTED                  # ... and the launch says the same, before any buffer
    assert cabi.tempo_skipgram_capacity(first_refused, 3) == (4096 * 2 * 3, 4096 * 2 * 3)   # sizes alone are still answered


def _call(cabi, cfg, G=1, B=1, graph=None, node_ts=None, edge_ts=None, seeds=None, seeds_ts=None, out=None, rng=True):
    r = cabi.TgRng(1, 2)
    return cabi.lib.tg_tempo_skipgram(C.byref(graph) if graph is not None else None, node_ts, edge_ts, seeds, seeds_ts,
                                      C.c_int64(G), C.c_int64(B), C.byref(cfg) if cfg is not None else None,
                                      C.byref(r) if rng else None, out, None)


def test_argument_errors_are_refused_before_any_launch(cabi):
    """every one returns TG_ERR_INVALID = 1 with null device pointers (a launch on this GPU-less machine would fail with
    TG_ERR_HIP = 2, and one with null buffers would fault)"""
    err = lambda: cabi.lib.tg_last_error().decode()
    pos, neg, walkers, nbytes = C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_int64(0)

    def refused(cfg, word):
        assert _call(cabi, cfg) == INVALID and word in err(), (word, err())
        assert cabi.lib.tg_tempo_skipgram_capacity(C.byref(cfg), C.c_int64(4), C.byref(pos), C.byref(neg)) == INVALID
        assert word in err()
        assert cabi.lib.tg_tempo_skipgram_lds_bytes(C.byref(cfg), C.byref(walkers), C.byref(nbytes)) == INVALID

    for bad, word in ((dict(Cs=0), "context_size"), (dict(Cs=6), "context_size"), (dict(R=0), "walks_per_node"),
                      (dict(K=-1), "num_negative_samples"), (dict(L=0, Cs=1), "walk_length"), (dict(L=-3, Cs=1), "walk_length"),
                      (dict(n_nodes=0), "n_nodes"), (dict(n_nodes=-1, K=2), "n_nodes")):
        refused(_cfg(cabi, **bad), word)
    assert _call(cabi, _cfg(cabi, n_nodes=0, K=0), G=0) == 0                  # without negatives n_nodes is not looked at
    assert _call(cabi, _cfg(cabi, L=5, Cs=5), G=0) == 0                       # C = L: the raw walks
    cfg = _cfg(cabi)
    assert _call(cabi, None) == INVALID and "null config" in err()
    assert _call(cabi, cfg, rng=False) == INVALID and "null rng" in err()
    assert _call(cabi, cfg, G=-1) == INVALID and _call(cabi, cfg, B=-1) == INVALID
    assert _call(cabi, cfg, G=1 << 39, B=1 << 39) == INVALID and "too large" in err()   # products that leave int64
    assert _call(cabi, _cfg(cabi, R=1 << 39, K=1 << 39), B=1 << 39) == INVALID and "too large" in err()
    assert cabi.lib.tg_tempo_skipgram_capacity(C.byref(cfg), C.c_int64(4), None, C.byref(neg)) == INVALID
    assert cabi.lib.tg_tempo_skipgram_lds_bytes(C.byref(cfg), None, C.byref(nbytes)) == INVALID
    assert _call(cabi, cfg) == INVALID and "null graph" in err()
    # a descriptor with offsets and nothing else: each null buffer is refused before it is looked at
    words = (C.c_int64 * 12)(*([0] * 12))
    at = C.addressof(words)
    g = cabi.TgGraph()
    g.ptrs, g.n_major, g.n_edges = at, 10, 0
    o = cabi.TgTempoSkipgramOut(at, at, at)
    full = dict(graph=g, node_ts=words, seeds=words, seeds_ts=words, out=C.byref(o))
    for missing in ("node_ts", "seeds", "seeds_ts", "out"):
        args = dict(full)
        args[missing] = None
        assert _call(cabi, cfg, **args) == INVALID and "null buffers" in err(), missing
    assert _call(cabi, cfg, **dict(full, out=C.byref(cabi.TgTempoSkipgramOut(None, at, at)))) == INVALID and "null buffers" in err()
    assert _call(cabi, cfg, **dict(full, out=C.byref(cabi.TgTempoSkipgramOut(at, at, None)))) == INVALID   # K = 1, no neg_rw
    g.n_edges = 3                                                             # edges, and neither indices nor edge_ts
    assert _call(cabi, cfg, **full) == INVALID and "null graph" in err()
    g.indices = at
    assert _call(cabi, cfg, **full) == INVALID and "null buffers" in err()


def test_empty_launches_return_ok(cabi):
    cfg = _cfg(cabi)
    assert _call(cabi, cfg, G=0, B=5) == 0
    assert _call(cabi, cfg, G=3, B=0) == 0
    assert _call(cabi, cfg, G=0, B=0) == 0


def test_exports(cabi):
    names = ["tg_tempo_skipgram_capacity", "tg_tempo_skipgram_lds_bytes", "tg_tempo_skipgram"]
    header = open(os.path.join(ROOT, "include", "tchgeo.h")).read()
    declared = set(re.findall(r"TG_API\s+[\w\s\*]+?\b(tg_\w+)\s*\(", header))
    for n in names:
        assert n in cabi.EXPORTS and n in declared and hasattr(cabi.lib, n), n
    assert "TG_TEMPO_SKIPGRAM_LDS_BYTES" in header


def _data(n=34, e=60, timestamps=True):
    import torch
    from tch_geometric.transforms import Graph
    gen = torch.Generator().manual_seed(3)
    data = Graph(edge_index=torch.randint(0, n, (2, e), generator=gen), num_nodes=n)
    if timestamps:
        data.timestamps = torch.randint(0, 9, (e,), generator=gen)
    return data


@pytest.mark.parametrize("drop_last", [False, True])
def test_loader_len_plan_and_call_ids(cabi, drop_last):
    import torch
    from tch_geometric import TemporalWalkLoader
    data = _data()
    loader = TemporalWalkLoader(data, 6, 3, (0, 4), walks_per_node=2, num_negative_samples=1, input_nodes=torch.arange(23),
                                batch_size=5, prefetch=3, drop_last=drop_last, seed=9, call_id0=100, device="cpu")
    assert len(loader) == (4 if drop_last else 5)
    full = [(0, 3, 5, 100), (15, 1, 5, 103)]
    assert loader.plan(0) == (full if drop_last else full + [(20, 1, 3, 104)])
    n = len(loader)
    assert [x[3] for x in loader.plan(2)] == [100 + 2 * n, 100 + 2 * n + 3] + ([] if drop_last else [100 + 2 * n + 4])
    ids = [cid + g for _, G, _, cid in loader.plan(1) for g in range(G)]     # every mini-batch has its own call id, in order
    assert ids == list(range(100 + n, 100 + 2 * n))
    assert loader.cfg.walk_length == 6 and (loader.cfg.win0, loader.cfg.win1) == (0, 4)   # columns, not steps
    assert loader.input_ts.numel() == 23 and bool((loader.input_ts == -1).all())
    # prefetch is clamped by the launch's memory: one mini-batch is (2 x pos + neg rows) * C * 8 bytes, pos once without pos_ts
    pos_rows, neg_rows = cabi.tempo_skipgram_capacity(loader.cfg, 5)
    per = (2 * pos_rows + neg_rows) * 3 * 8
    mk = lambda **kw: TemporalWalkLoader(data, 6, 3, (0, 4), 2, 1, batch_size=5, prefetch=64, **kw)
    assert mk(max_workspace_bytes=2 * per).prefetch == 2 and mk(max_workspace_bytes=1).prefetch == 1
    assert mk(max_workspace_bytes=2 * per, with_timestamps=False).prefetch == 2 * per // ((pos_rows + neg_rows) * 3 * 8)
    assert mk().input_nodes.numel() == 34 and mk().prefetch == 64            # default: every node


def test_loader_constructor_errors(cabi):
    import torch
    from tch_geometric import TemporalWalkLoader
    data, bare = _data(), _data(timestamps=False)
    ts = torch.arange(60)
    with pytest.raises(ValueError, match="timestamps"):
        TemporalWalkLoader(bare, 6, 3, (0, 4))                               # no data.timestamps and no edge_timestamps
    assert len(TemporalWalkLoader(bare, 6, 3, (0, 4), edge_timestamps=ts, batch_size=8)) == 5
    with pytest.raises(ValueError, match="edge_timestamps"):
        TemporalWalkLoader(data, 6, 3, (0, 4), edge_timestamps=ts[:59])
    with pytest.raises(ValueError, match="node_timestamps"):
        TemporalWalkLoader(data, 6, 3, (0, 4), node_timestamps=torch.zeros(33, dtype=torch.int64))
    with pytest.raises(ValueError, match="input_timestamps"):
        TemporalWalkLoader(data, 6, 3, (0, 4), input_nodes=torch.arange(7), input_timestamps=torch.zeros(6, dtype=torch.int64))
    for window in ((4, 4), (5, 0)):
        with pytest.raises(ValueError, match="window"):
            TemporalWalkLoader(data, 6, 3, window)
    for bad, word in ((dict(walk_length=6, context_size=7), "context_size"), (dict(walk_length=6, context_size=0), "context_size"),
                      (dict(walk_length=0, context_size=1), "walk_length"), (dict(walks_per_node=0), "walks_per_node"),
                      (dict(num_negative_samples=-1), "num_negative_samples"), (dict(walk_length=4096), "walk_length 4096")):
        args = dict(walk_length=6, context_size=3, window=(0, 4))
        args.update(bad)
        with pytest.raises(ValueError, match=word):
            TemporalWalkLoader(data, **args)
    with pytest.raises(ValueError, match="batch_size"):
        TemporalWalkLoader(data, 6, 3, (0, 4), batch_size=0)
    with pytest.raises(IndexError):
        TemporalWalkLoader(data, 6, 3, (0, 4), input_nodes=torch.tensor([34]))
