"""TG_SAMPLER_LABOR without a device: the NumPy Philox against the oracle's, the restatement (helpers_labor.py) against brute
force, the law of one vertex by enumeration, a negative control of the device law test's statistic, the header as C, the
refusals of the C ABI (fake pointers: nothing is launched) and of the loaders."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import exact_laws
import orc
from helpers_labor import (SAMPLER_LABOR, SAMPLER_LABOR_SHARED, TAG_LABOR, labor_hop, labor_key, labor_ns_homo,
                           labor_test_graph, long_degrees, named_draw)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tchgeo.h")
MODES = [(-1, False), (0, False), (1, False), (1, True), (2, False), (2, True)]


def test_numpy_philox_equals_the_oracles_named_draw():
    rs = np.random.default_rng(0x14B)
    N = 1000
    seed = rs.integers(0, 2 ** 64, N, dtype=np.uint64)
    call = rs.integers(0, 2 ** 64, N, dtype=np.uint64)
    tag = rs.integers(0, 2 ** 32, N, dtype=np.uint64)
    ids = rs.integers(0, 2 ** 64, N, dtype=np.uint64)
    ids[::3] = rs.integers(0, 2 ** 20, len(ids[::3]), dtype=np.uint64)     # small ids as well as ids past 2^32
    d0 = rs.integers(0, 2 ** 32, N, dtype=np.uint64)
    d1 = rs.integers(0, 2 ** 32, N, dtype=np.uint64)
    assert (ids >= 2 ** 32).sum() > 300
    got = np.stack(named_draw(seed, call, tag, ids, d0, d1), axis=1)
    for i in range(N):
        want = orc.philox_named_draw(int(seed[i]), int(call[i]), int(tag[i]), int(ids[i]), int(d0[i]), int(d1[i]))
        assert got[i].tolist() == want, i
    # the key: the low 64 bits shifted right by one -- non-negative, and a function of (seed, call id, t, layer) only
    w = orc.philox_named_draw(7, 9, TAG_LABOR, 123456789012, 3, 0)
    assert int(labor_key(7, 9, np.array([123456789012]), 3)[0]) == (w[0] | (w[1] << 32)) >> 1
    assert (labor_key(7, 9, np.arange(1000), 0) >= 0).all()


def _brute_column(idx, ts, e0, e1, state, k, mode, forward, window, seed, call, layer):
    """keys in a dict, one oracle draw per distinct neighbour; a Python sort of (key, edge pointer) tuples"""
    keys = {}
    left = []
    for e in range(e0, e1):
        if mode != -1:
            t = int(ts[e])
            x = t if mode == 0 else (t - state if forward else state - t)
            if not (window[0] <= x <= window[1]):
                continue
        t = int(idx[e])
        if t not in keys:
            w = orc.philox_named_draw(seed, call, TAG_LABOR, t, layer, 0)
            keys[t] = (w[0] | (w[1] << 32)) >> 1
        left.append((keys[t], e))
    return [e for _, e in sorted(left)[:k]]


@pytest.mark.parametrize("mode,forward", MODES)
def test_helper_equals_brute_force_on_tiny_columns(mode, forward):
    rs = np.random.default_rng(31 + mode + 10 * forward)
    deg = rs.integers(0, 12, 30)
    ptrs = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    idx = rs.integers(0, 8, ptrs[-1])                     # few distinct neighbours: parallel edges, equal keys
    ts = rs.integers(0, 4, ptrs[-1])
    vertices = rs.integers(-1, 30, 40)
    states = rs.integers(-2, 6, 40)
    calls = rs.integers(0, 3, 40)
    window = (0, 2) if mode != 0 else (1, 3)
    for k, layer in ((1, 0), (3, 1), (64, 2)):
        cnt, off, nbr, ep, par, sto = labor_hop(ptrs, idx, ts, vertices, states, k, 77, calls, layer, mode, forward, window)
        assert off[0] == 0 and np.array_equal(np.diff(off), cnt) and len(ep) == off[-1]
        for i, w in enumerate(vertices):
            want = [] if w < 0 else _brute_column(idx, ts, ptrs[w], ptrs[w + 1], int(states[i]), k, mode, forward, window, 77,
                                                  int(calls[i]), layer)
            a, b = off[i], off[i + 1]
            assert ep[a:b].tolist() == want, (i, k)
            assert np.array_equal(nbr[a:b], idx[ep[a:b]]) and np.all(par[a:b] == i)
            assert np.array_equal(sto[a:b], ts[ep[a:b]] if mode == 2 else np.full(b - a, states[i]))


def test_seeds_with_shared_neighbours_pick_them_in_the_same_order():
    g = labor_test_graph(64, scale=8)                     # a small threshold: the graph only has to have its shape here
    a, b = g["shared"]
    common = set(g["common"].tolist())
    for sampler_layer in (0, 1):
        cnt, off, nbr, ep, par, _ = labor_hop(g["ptrs"], g["idx"], None, [a, b], None, 64, 5, 9, sampler_layer)
        na, nb = nbr[off[0]:off[1]], nbr[off[1]:off[2]]
        first = lambda x: [t for i, t in enumerate(x.tolist()) if t in common and t not in x[:i].tolist()]
        fa, fb = first(na), first(nb)
        n = min(len(fa), len(fb))
        assert n > 20 and fa[:n] == fb[:n]                # the same vertices, in the same order
        assert len(set(na.tolist()) & set(nb.tolist())) > 20
    # another call id: other variates
    other = labor_hop(g["ptrs"], g["idx"], None, [a], None, 64, 5, 10, 0)[2]
    assert other.tolist() != nbr[off[0]:off[1]].tolist()
    # the column made of one neighbour: equal keys throughout, pure pointer order
    e0 = int(g["ptrs"][g["same"]])
    assert labor_hop(g["ptrs"], g["idx"], None, [g["same"]], None, 64, 5, 9, 0)[3].tolist() == list(range(e0, e0 + 64))


def test_graph_has_the_columns_the_device_tests_need():
    g = labor_test_graph(8192)
    deg = np.diff(g["ptrs"])
    assert tuple(deg[g["long"]]) == long_degrees(8192) == (8191, 8192, 8193, 16447, 131089)
    assert deg[g["same"]] == 70 and len(set(g["idx"][g["ptrs"][g["same"]]:g["ptrs"][g["same"] + 1]].tolist())) == 1
    assert g["idx"].max() < g["base"] and len(g["ptrs"]) == g["n"] + 1


def test_law_of_one_vertex_by_enumeration():
    """d = 6 distinct neighbours, k = 3: the selection depends on the keys only through their order.  Over all 720 orders
    every ordered triple comes up 720 / 120 = 6 times -- a uniform k-subset in uniform order, TG_SAMPLER_UNIFORM's law."""
    d, k = 6, 3
    ptrs = np.array([0, d], dtype=np.int64)
    idx = np.arange(100, 100 + d, dtype=np.int64)
    import helpers_labor
    seen = {}
    real = helpers_labor.labor_key
    try:
        for perm in itertools.permutations(range(d)):
            helpers_labor.labor_key = lambda seed, c, t, layer, tag=TAG_LABOR, bits=63, perm=perm: np.asarray(perm, dtype=np.int64)[np.asarray(t) - 100]
            out = tuple(helpers_labor.labor_hop(ptrs, idx, None, [0], None, k, 0, 0, 0)[2].tolist())
            seen[out] = seen.get(out, 0) + 1
    finally:
        helpers_labor.labor_key = real
    assert len(seen) == 6 * 5 * 4 and set(seen.values()) == {6}


def _pair_counts(first, second, d):
    counts = np.zeros((d, d), dtype=np.int64)
    np.add.at(counts, (first, second), 1)
    return counts


def pair_law(d):
    p = np.full((d, d), 1.0 / (d * (d - 1)))
    np.fill_diagonal(p, 0.0)
    return p.reshape(-1)


def test_the_law_statistic_accepts_real_keys_and_rejects_keys_cut_to_six_bits():
    """the device law test's statistic on the restatement: 2^16 call ids, one column of 20 distinct neighbours, the ordered
    pair (first, second).  With 63-bit keys it passes; with keys cut to 6 bits ties are frequent and go to the smaller edge
    pointer, which favours ascending pairs: the same test must reject."""
    d, N = 20, 1 << 16
    t = np.arange(d, dtype=np.int64)
    calls = np.arange(N, dtype=np.uint64)
    for bits, passes in ((63, True), (6, False)):
        keys = labor_key(3, calls[:, None], t[None, :], 0, bits=bits)           # [N, d]
        order = np.argsort(keys * d + t[None, :] if bits == 6 else keys, axis=1, kind="stable")
        counts = _pair_counts(order[:, 0], order[:, 1], d).reshape(-1)
        if passes:
            exact_laws.chi2_gof(counts, pair_law(d), "restated labor pairs")
        else:
            with pytest.raises(AssertionError):
                exact_laws.chi2_gof(counts, pair_law(d), "6-bit keys")


def test_shared_and_plain_agree_at_hop_0_and_differ_later():
    g = labor_test_graph(64, scale=8)
    seeds = np.arange(40, dtype=np.int64)
    a = labor_ns_homo(g["ptrs"], g["idx"], None, seeds, [3, 3], 1, 2, SAMPLER_LABOR)
    b = labor_ns_homo(g["ptrs"], g["idx"], None, seeds, [3, 3], 1, 2, SAMPLER_LABOR_SHARED)
    n0 = a[4][1][1]                                       # edges of hop 0
    assert a[4][:2] == b[4][:2]
    assert np.array_equal(a[3][:n0], b[3][:n0]) and not np.array_equal(a[3][n0:], b[3][n0:])


# ---------------------------------------------------------------- header and constants
def test_header_compiles_as_c_with_the_new_ids(tmp_path):
    src = tmp_path / "labor.c"
    src.write_text('#include "tchgeo.h"\n'
                   'typedef char a4[TG_SAMPLER_LABOR == 4 ? 1 : -1];\n'
                   'typedef char a5[TG_SAMPLER_LABOR_SHARED == 5 ? 1 : -1];\n'
                   'typedef char a14[TG_TAG_LABOR == 14u ? 1 : -1];\n'
                   'int main(void) { tg_hop_in in; in.sampler = TG_SAMPLER_LABOR; return in.sampler == 4 ? TG_OK : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-fsyntax-only", str(src)])


def test_cabi_mirrors_the_header():
    from tch_geometric import _cabi
    text = open(HEADER).read()
    assert (_cabi.SAMPLER_LABOR, _cabi.SAMPLER_LABOR_SHARED) == (4, 5) and callable(_cabi.ns_hop_labor)
    m = re.search(r"#define TG_LABOR_LONG_COLUMN (\d+)", text)
    assert m and int(m.group(1)) == _cabi.LABOR_LONG_COLUMN
    prev = _cabi.ns_hop_labor_long_column(123)
    assert prev == _cabi.LABOR_LONG_COLUMN and _cabi.ns_hop_labor_long_column(0) == 123
    assert _cabi.ns_hop_labor_long_column(0) == _cabi.LABOR_LONG_COLUMN
    for name in ("tg_ns_hop_labor", "tg_ns_hop_labor_workspace_bytes"):
        assert name in _cabi.EXPORTS and hasattr(_cabi.lib, name)
    nbytes = C.c_int64(0)
    assert _cabi.lib.tg_ns_hop_labor_workspace_bytes(C.c_int64(1000), C.byref(nbytes)) == 0 and nbytes.value >= 1001 * 8
    assert _cabi.lib.tg_ns_hop_labor_workspace_bytes(C.c_int64(-1), C.byref(nbytes)) == 1


def test_labor_edge_sampler():
    from tch_geometric import LaborEdgeSampler
    from tch_geometric.utils import LaborEdgeSampler as same
    s = LaborEdgeSampler()
    assert LaborEdgeSampler is same and s.layer_dependency is False and LaborEdgeSampler(True).layer_dependency is True
    assert s.validate() is None
    for other in ("with_replacement", "weights", "temporal_strategy"):     # the host module tries those first
        assert not hasattr(s, other)
    with pytest.raises(ValueError, match="LaborEdgeSampler: homogeneous sampling only"):
        s.validate(hetero=True)
    import tch_geometric as tg
    with pytest.raises(ValueError, match="LaborEdgeSampler: homogeneous sampling only"):
        tg.neighbor_sampling_heterogenous(["a"], [("a", "r", "a")], {}, {}, {}, {}, 1, s, None)


# ---------------------------------------------------------------- refusals of the C ABI: fake pointers, nothing is launched
FAKE = 1 << 20


def _hop_args(cabi, sampler=4, m=1, fanout=4, n_edges=100, max_degree=0, timestamps=True):
    g = cabi.TgGraph()
    g.ptrs = g.indices = FAKE
    g.timestamps = FAKE if timestamps else None
    g.n_major, g.n_edges, g.max_degree = 8, n_edges, max_degree
    hin, hout, flt = cabi.TgHopIn(), cabi.TgHopOut(), cabi.TgHopFilter()
    hin.vertices, hin.m, hin.fanout, hin.sampler = FAKE, m, fanout, sampler
    hout.cnt = hout.offsets = hout.neighbors = hout.edge_ptrs = hout.parents = FAKE
    flt.filter_mode = -1
    return g, hin, hout, flt


def _hop(cabi, g, hin, hout, flt, layer=0, states_out=None, ws=FAKE << 8, ws_bytes=1 << 30, rng=True):
    r = cabi.TgRng(1, 2)
    rc = cabi.lib.tg_ns_hop_labor(C.byref(g), C.byref(hin), C.byref(flt) if flt is not None else None,
                                  C.byref(r) if rng else None, C.c_int32(layer), C.byref(hout), states_out,
                                  C.c_void_p(ws) if ws else None, C.c_int64(ws_bytes), None)
    return rc, cabi.lib.tg_last_error().decode()


def test_flat_hop_refusals():
    from tch_geometric import _cabi as cabi
    for sampler in (0, 1, 2, 3, 6):
        rc, err = _hop(cabi, *_hop_args(cabi, sampler=sampler))
        assert rc == 1 and "TG_SAMPLER_LABOR" in err
    for k in (0, 65, -1):
        rc, err = _hop(cabi, *_hop_args(cabi, fanout=k))
        assert rc == 1 and "1..64" in err
    for n_edges, max_degree in ((2 ** 32 - 1, 0), (2 ** 33, 0), (2 ** 33, 2 ** 32 - 1), (2 ** 33, 2 ** 33)):
        rc, err = _hop(cabi, *_hop_args(cabi, n_edges=n_edges, max_degree=max_degree))
        assert rc == 1 and "2^32 - 1" in err
    rc, err = _hop(cabi, *_hop_args(cabi, m=-1))
    assert rc == 1 and "negative" in err
    rc, err = _hop(cabi, *_hop_args(cabi), layer=-1)
    assert rc == 1 and "layer" in err
    rc, err = _hop(cabi, *_hop_args(cabi), rng=False)
    assert rc == 1 and "null" in err
    for mode in (-2, 3):
        g, hin, hout, flt = _hop_args(cabi)
        flt.filter_mode = mode
        rc, err = _hop(cabi, g, hin, hout, flt)
        assert rc == 1 and "bad filter" in err
    g, hin, hout, flt = _hop_args(cabi, timestamps=False)      # a filter needs the timestamps ...
    flt.filter_mode, flt.states = 1, FAKE
    rc, err = _hop(cabi, g, hin, hout, flt, states_out=C.c_void_p(FAKE))
    assert rc == 1 and "timestamps" in err
    g, hin, hout, flt = _hop_args(cabi)                        # ... its states and states_out
    flt.filter_mode = 1
    rc, err = _hop(cabi, g, hin, hout, flt, states_out=C.c_void_p(FAKE))
    assert rc == 1 and "states" in err
    flt.states = FAKE
    rc, err = _hop(cabi, g, hin, hout, flt, states_out=None)
    assert rc == 1 and "states" in err
    rc, err = _hop(cabi, *_hop_args(cabi), ws=None)            # the workspace: missing, short, misaligned
    assert rc == 1 and "workspace" in err
    rc, err = _hop(cabi, *_hop_args(cabi, m=1000), ws_bytes=1000 * 8)
    assert rc == 1 and "too small" in err
    rc, err = _hop(cabi, *_hop_args(cabi), ws=(FAKE << 8) + 4)
    assert rc == 1 and "aligned" in err


def _batched(cabi, sampler=4, fanout=(4,), n_edges=100, ws=FAKE << 8, ws_bytes=1 << 40, mode=-1, timestamps=True,
             seed_ids=False, use_ws=True, states=True):
    g = cabi.TgGraph()
    g.ptrs = g.indices = FAKE
    g.timestamps = FAKE if timestamps else None
    g.n_major, g.n_edges = 8, n_edges
    cfg, rng, out = cabi.TgNsConfig(), cabi.TgRng(1, 2), cabi.TgNsOut()
    cfg.sampler, cfg.filter_mode = sampler, mode
    if seed_ids:
        cfg.seed_ids = cfg.seed_call_ids = FAKE
    if mode != -1 and states:
        cfg.seeds_state = FAKE
        out.states = FAKE
    out.samples = out.rows = out.cols = out.edge_index = out.layer_offsets = out.counts = FAKE
    out.cap_nodes, out.cap_edges = 1 << 30, 1 << 30
    fan = (C.c_int64 * len(fanout))(*fanout)
    args = (C.byref(g), C.c_void_p(FAKE), C.c_int64(1), C.c_int64(4), fan, C.c_int32(len(fanout)), C.byref(cfg),
            C.byref(rng), C.byref(out))
    if use_ws:
        rc = cabi.lib.tg_ns_homo_batched_ws(*args, C.c_void_p(ws) if ws else None, C.c_int64(ws_bytes if ws else 0),
                                            C.c_int32(0), None)
    else:
        rc = cabi.lib.tg_ns_homo_batched(*args, None)
    return rc, cabi.lib.tg_last_error().decode()


@pytest.mark.parametrize("sampler", [4, 5])
def test_batched_refusals(sampler):
    from tch_geometric import _cabi as cabi
    rc, err = _batched(cabi, sampler, fanout=(4, 65))
    assert rc == 1 and "1..64" in err and "TG_SAMPLER_LABOR" in err
    rc, err = _batched(cabi, sampler, n_edges=2 ** 32 - 1)
    assert rc == 1 and "2^32 - 1" in err
    rc, err = _batched(cabi, sampler, seed_ids=True)
    assert rc == 1 and "seed_ids" in err
    rc, err = _batched(cabi, sampler, use_ws=False)
    assert rc == 1 and "workspace" in err
    rc, err = _batched(cabi, sampler, ws_bytes=64)
    assert rc == 1 and "too small" in err
    rc, err = _batched(cabi, sampler, ws=(FAKE << 8) + 8)
    assert rc == 1 and "aligned" in err
    rc, err = _batched(cabi, sampler, mode=1, timestamps=False)
    assert rc == 1 and "timestamps" in err
    rc, err = _batched(cabi, sampler, mode=1, states=False)
    assert rc == 1 and "seeds_state" in err
    rc, err = _batched(cabi, 6)
    assert rc == 1 and "bad sampler" in err
    # the workspace query: sized for the new ids, refusing a fan-out of 65
    g = cabi.TgGraph()
    g.n_major, g.n_edges = 8, 100
    cfg, need = cabi.TgNsConfig(), C.c_int64(0)
    cfg.sampler, cfg.filter_mode = sampler, -1
    q = lambda fan: cabi.lib.tg_ns_homo_batched_workspace_bytes(C.byref(g), C.c_int64(3), C.c_int64(8), (C.c_int64 * 2)(*fan),
                                                                C.c_int32(2), C.byref(cfg), C.byref(need))
    assert q((3, 2)) == 0 and need.value > 0
    labor_bytes = need.value
    cfg.sampler = cabi.SAMPLER_RECENT
    assert q((3, 2)) == 0 and labor_bytes > need.value      # RECENT's layout plus the long-column list
    cfg.sampler = sampler
    assert q((3, 65)) == 1
    # the form queries answer "neither window-ordered form"
    out = cabi.TgNsOut()
    out.cap_nodes, out.cap_edges = 1 << 20, 1 << 20
    form = C.c_int32(-1)
    assert cabi.lib.tg_ns_homo_batched_form(C.byref(g), C.c_int64(4096), C.c_int64(8), (C.c_int64 * 2)(3, 2), C.c_int32(2),
                                            C.byref(cfg), C.byref(out), C.c_int64(1 << 40), C.c_int32(0), C.byref(form),
                                            None) == 0
    assert form.value == 2                                   # TG_NS_FORM_FUSED: what the scanning samplers report


def test_other_entry_points_keep_refusing_the_ids():
    from tch_geometric import _cabi as cabi
    g, hin, hout, flt = _hop_args(cabi)
    rng = cabi.TgRng(1, 2)
    for sampler in (4, 5):
        hin.sampler = sampler
        assert cabi.lib.tg_ns_hop(C.byref(g), C.byref(hin), C.byref(rng), C.byref(hout), C.c_void_p(FAKE << 8),
                                  C.c_int64(1 << 30), None) == 1
        assert cabi.lib.tg_ns_hop_recent(C.byref(g), C.byref(hin), None, C.byref(hout), None, None) == 1
        st = C.c_void_p(FAKE)
        flt.filter_mode, flt.states = 1, FAKE
        assert cabi.lib.tg_ns_hop_scan(C.byref(g), C.byref(hin), C.byref(flt), C.byref(rng), C.byref(hout), st, st,
                                       C.c_void_p(FAKE << 8), C.c_int64(1 << 30), C.c_int64(1024), None) == 1


# ---------------------------------------------------------------- loaders
def _graph():
    from tch_geometric.transforms import Graph
    ei = torch.tensor([[0, 1, 2, 3, 4, 0], [1, 2, 3, 4, 0, 2]])
    return Graph(edge_index=ei, num_nodes=5, time=torch.arange(6))


T5 = torch.zeros(5, dtype=torch.int64)


@pytest.mark.parametrize("kw,match", [
    (dict(labor=True, replace=True), "replace"),
    (dict(labor=True, time_attr="time", input_time=T5, temporal_strategy="last"), "last"),
    (dict(labor=True, unique=True, disjoint=True), "disjoint"),
    (dict(labor=True, num_neighbors=[2, 65]), "64"),
    (dict(layer_dependency=True), "labor=True"),
])
def test_loader_refusals_need_no_device(kw, match):
    from tch_geometric.loader import LinkNeighborLoader, NeighborLoader
    kw = dict(kw)
    fan = kw.pop("num_neighbors", [2, 2])
    with pytest.raises(ValueError, match=match):
        NeighborLoader(_graph(), fan, device="cuda:0", **kw)
    if "input_time" in kw:
        kw["edge_label_time"] = torch.zeros(6, dtype=torch.int64)
        del kw["input_time"]
    with pytest.raises(ValueError, match=match):
        LinkNeighborLoader(_graph(), fan, device="cuda:0", **kw)


def test_shadow_loader_does_not_get_the_option():
    from tch_geometric.loader import ShaDowKHopLoader
    with pytest.raises(TypeError):
        ShaDowKHopLoader(_graph(), 2, 2, labor=True, device="cuda:0")
