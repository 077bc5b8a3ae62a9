"""TG_SAMPLER_RECENT without a device: the NumPy restatement (helpers_recent.py) against brute force and against the
oracle's filter semantics, RecentEdgeSampler's validation, the temporal NeighborLoader's refusals, and the header as C."""
import os
import subprocess

import numpy as np
import pytest
import torch

import orc
from helpers import load_karate
from helpers_recent import recent_hop, recent_ns_homo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(-1, False), (-1, True), (0, False), (1, False), (1, True), (2, False), (2, True)]


def _brute_column(ts, e0, e1, state, k, mode, forward, window):
    """pick the best remaining edge k times: no sort, no vector arithmetic"""
    left = []
    for e in range(e0, e1):
        t = int(ts[e])
        x = t if mode == 0 else (t - state if forward else state - t)
        if mode == -1 or window[0] <= x <= window[1]:
            left.append(e)
    out = []
    while left and len(out) < k:
        best = left[0]
        for e in left[1:]:
            better = ts[e] < ts[best] if forward else ts[e] > ts[best]
            if better or (ts[e] == ts[best] and e < best):
                best = e
        out.append(best)
        left.remove(best)
    return out


@pytest.mark.parametrize("mode,forward", MODES)
def test_helper_equals_brute_force_on_tiny_columns(mode, forward):
    rs = np.random.default_rng(3 + mode + 10 * forward)
    deg = rs.integers(0, 9, 40)
    ptrs = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    idx = rs.integers(0, 40, ptrs[-1])
    for ts in (rs.integers(0, 4, ptrs[-1]), rs.permutation(int(ptrs[-1])) - 50):
        vertices = rs.integers(-1, 40, 60)
        states = rs.integers(-2, 6, 60)
        window = (0, 2) if mode != 0 else (1, 3)
        for k in (1, 3, 8, 64):
            cnt, off, nbr, ep, par, sto = recent_hop(ptrs, idx, ts, vertices, states, k, mode, forward, window)
            assert off[0] == 0 and np.array_equal(np.diff(off), cnt) and len(ep) == off[-1]
            for i, w in enumerate(vertices):
                want = [] if w < 0 else _brute_column(ts, ptrs[w], ptrs[w + 1], int(states[i]), k, mode, forward, window)
                a, b = off[i], off[i + 1]
                assert ep[a:b].tolist() == want, (i, k)
                assert np.array_equal(nbr[a:b], idx[ep[a:b]]) and np.all(par[a:b] == i)
                assert np.array_equal(sto[a:b], ts[ep[a:b]] if mode == 2 else np.full(b - a, states[i]))


@pytest.mark.parametrize("mode,forward", MODES[2:])
@pytest.mark.parametrize("fanout", [[17], [17, 17]])
def test_admitted_set_equals_the_oracles_where_everything_is_taken(mode, forward, fanout):
    """degree <= k: the uniform sampler and the most-recent-k sampler both take every admitted edge, so the oracle's edges
    under the same filter are the helper's -- in another order within a column, hence compared as sorted lists"""
    ei, n = load_karate()
    ptrs, idx, _ = orc.to_csc(ei, n)
    assert int(np.diff(ptrs).max()) <= 17
    rs = np.random.default_rng(7)
    ts = rs.permutation(len(idx)).astype(np.int64)                # distinct
    seeds = np.array([0, 33, 5, 16, 2], dtype=np.int64)
    st = rs.integers(40, 120, len(seeds))
    window = (30, 110) if mode == 0 else (0, 60)
    o = orc.ns_homo(ptrs, idx, seeds, fanout, orc.rng_philox(1, 2), filter_mode=mode, forward=forward, window=window,
                    timestamps=ts, inputs_state=st)
    h = recent_ns_homo(ptrs, idx, ts, seeds, fanout, st, mode, forward, window)
    assert h[4] == o[4] and h[5] == (len(o[0]), len(o[3]))
    assert len(o[3]) > 0 and sorted(h[3].tolist()) == sorted(o[3].tolist())
    assert sorted(h[0].tolist()) == sorted(o[0].tolist())


def test_ns_homo_helper_bookkeeping():
    ptrs = np.array([0, 3, 4, 4, 6], dtype=np.int64)
    idx = np.array([1, 2, 3, 0, 0, 1], dtype=np.int64)
    ts = np.array([5, 9, 9, 1, 2, 7], dtype=np.int64)
    s, r, c, e, lo, counts, st = recent_ns_homo(ptrs, idx, ts, [0, 3, 2], [2, 1])
    # hop 0: v0 -> e1, e2 (equal times: the smaller pointer first), v3 -> e5, e4, v2 has no column; hop 1, k = 1, over
    # the frontier [2, 3, 1, 0] at slots 3..6: v3 -> e5, v1 -> e3, v0 -> e1
    assert e.tolist() == [1, 2, 5, 4, 5, 3, 1]
    assert s.tolist() == [0, 3, 2, 2, 3, 1, 0, 1, 0, 2]
    assert r.tolist() == list(range(3, 10)) and c.tolist() == [0, 0, 1, 1, 4, 5, 6]
    assert lo == [(3, 0, 3), (7, 4, 7)] and counts == (10, 7) and st.tolist() == [0] * 10


def test_recent_edge_sampler_validates_int64():
    from tch_geometric import RecentEdgeSampler
    from tch_geometric.utils import RecentEdgeSampler as same
    assert RecentEdgeSampler is same and RecentEdgeSampler.temporal_strategy == "last"
    s = RecentEdgeSampler(torch.arange(4))
    assert s.validate() is None and s.temporal_strategy == "last"
    assert not hasattr(s, "with_replacement") and not hasattr(s, "weights")   # the host module tries those first
    with pytest.raises(TypeError):
        RecentEdgeSampler(torch.arange(4, dtype=torch.int32)).validate()
    with pytest.raises(TypeError):
        RecentEdgeSampler({"a__b__c": torch.zeros(3)}).validate(hetero=True)
    assert RecentEdgeSampler({"a__b__c": torch.arange(3)}).validate(hetero=True) is None


def test_cabi_names_the_sampler():
    from tch_geometric import _cabi
    assert _cabi.SAMPLER_RECENT == 3 and callable(_cabi.ns_hop_recent)
    text = open(os.path.join(ROOT, "include", "tchgeo.h")).read()
    assert "#define TG_SAMPLER_RECENT 3" in text


def _graph(with_time=True):
    from tch_geometric.transforms import Graph
    ei = torch.tensor([[0, 1, 2, 3, 4, 0], [1, 2, 3, 4, 0, 2]])
    kw = {"time": torch.arange(6)} if with_time else {}
    return Graph(edge_index=ei, num_nodes=5, **kw)


@pytest.mark.parametrize("kw", [
    dict(time_attr="time"),                                                        # no input_time
    dict(input_time=torch.zeros(5, dtype=torch.int64)),                            # no time_attr
    dict(temporal_strategy="last"),                                                # "last" without times
    dict(temporal_strategy="recent", time_attr="time", input_time=torch.zeros(5, dtype=torch.int64)),
    dict(time_attr="time", input_time=torch.zeros(4, dtype=torch.int64)),          # one per input node
    dict(time_attr="time", input_time=torch.zeros(5, dtype=torch.int64), input_nodes=torch.arange(3)),
    dict(time_attr="time", input_time=torch.zeros(5, dtype=torch.int32)),          # int64 only
    dict(time_attr="stamp", input_time=torch.zeros(5, dtype=torch.int64)),         # no such attribute
    dict(time_attr="time", input_time=torch.zeros(5, dtype=torch.int64), unique=True),
    dict(time_attr="time", input_time=torch.zeros(5, dtype=torch.int64), temporal_strategy="last", num_neighbors=[65]),
    dict(time_window=(0, 5)),
])
def test_temporal_loader_refusals_need_no_device(kw):
    from tch_geometric.loader import NeighborLoader
    kw = dict(kw)
    fan = kw.pop("num_neighbors", [2, 2])
    with pytest.raises(ValueError):
        NeighborLoader(_graph(), fan, device="cuda:0", **kw)


def test_edge_times_must_match_the_edges():
    from tch_geometric.loader import NeighborLoader
    from tch_geometric.transforms import Graph
    g = Graph(edge_index=torch.tensor([[0, 1, 2], [1, 2, 0]]), num_nodes=3, time=torch.arange(3), x=torch.zeros(3, 2))
    g.time = torch.arange(2)
    with pytest.raises(ValueError):
        NeighborLoader(g, [2], time_attr="time", input_time=torch.zeros(3, dtype=torch.int64), device="cuda:0")


def test_temporal_loader_refuses_a_graph_with_fields_of_its_own_names():
    from tch_geometric.loader import NeighborLoader
    from tch_geometric.transforms import Graph
    ei = torch.tensor([[0, 1, 2, 3, 4, 0], [1, 2, 3, 4, 0, 2]])
    for name in ("node_time", "input_time"):
        g = Graph(edge_index=ei, num_nodes=5, time=torch.arange(6), **{name: torch.arange(5)})
        with pytest.raises(ValueError, match=name):
            NeighborLoader(g, [2], time_attr="time", input_time=torch.zeros(5, dtype=torch.int64), device="cuda:0")


def test_columns_past_the_32_bit_position_are_refused_before_any_launch():
    """a column of 2^32 - 1 edges or more cannot be ranked (32-bit positions): a graph that large must state a max_degree
    below the limit -- checked on the host, so fake addresses are never read"""
    import ctypes as C
    from tch_geometric import _cabi
    fake = 1 << 20
    g = _cabi.TgGraph()
    g.ptrs = g.indices = g.timestamps = fake
    g.n_major = 8
    hin, hout = _cabi.TgHopIn(), _cabi.TgHopOut()
    hin.vertices, hin.m, hin.fanout, hin.sampler = fake, 1, 4, _cabi.SAMPLER_RECENT
    hout.cnt = hout.offsets = hout.neighbors = hout.edge_ptrs = hout.parents = fake
    for n_edges, max_degree in ((2 ** 32 - 1, 0), (2 ** 33, 0), (2 ** 33, 2 ** 32 - 1), (2 ** 33, 2 ** 33)):
        g.n_edges, g.max_degree = n_edges, max_degree
        assert _cabi.lib.tg_ns_hop_recent(C.byref(g), C.byref(hin), None, C.byref(hout), None, None) == 1
        assert b"2^32 - 1" in _cabi.lib.tg_last_error()
        cfg, rng, out = _cabi.TgNsConfig(), _cabi.TgRng(1, 2), _cabi.TgNsOut()
        cfg.sampler, cfg.filter_mode = _cabi.SAMPLER_RECENT, -1
        out.samples = out.rows = out.cols = out.edge_index = out.layer_offsets = out.counts = fake
        out.cap_nodes, out.cap_edges = 1 << 20, 1 << 20
        fan = (C.c_int64 * 1)(4)
        assert _cabi.lib.tg_ns_homo_batched_ws(C.byref(g), C.c_void_p(fake), C.c_int64(1), C.c_int64(4), fan, C.c_int32(1),
                                               C.byref(cfg), C.byref(rng), C.byref(out), C.c_void_p(fake << 8),
                                               C.c_int64(1 << 40), C.c_int32(0), None) == 1
        assert b"2^32 - 1" in _cabi.lib.tg_last_error()


def test_link_loader_refuses_time_attr():
    from tch_geometric.loader import LinkNeighborLoader
    with pytest.raises(ValueError, match="time_attr"):
        LinkNeighborLoader(_graph(), [2], time_attr="time", device="cuda:0")


def test_header_still_compiles_as_c(tmp_path):
    src = tmp_path / "recent.c"
    src.write_text('#include "tchgeo.h"\n'
                   'int main(void) { tg_hop_in in; in.sampler = TG_SAMPLER_RECENT; return in.sampler == 3 ? TG_OK : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-fsyntax-only", str(src)])
