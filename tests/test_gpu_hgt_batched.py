"""GPU parity of batched hgt_sampling (tg_hgt_sample_batched): call b of a launch equals the oracle with call id
call_id0 + b and the single call (tg_hgt_sample through hgt_sampling) with that call id, word for word -- samples,
sample timestamps, rows, cols, edge_index, counts and the panic flag.  Then the same at cfg4's scale and HGTLoader."""
import numpy as np
import pytest
import torch

import orc
from helpers import load_fake_hetero, rel_key

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -0x5A5A5A5A5A5A5A5B


@pytest.fixture(scope="module")
def tg():
    import tch_geometric
    return tch_geometric


@pytest.fixture(scope="module")
def cabi():
    from tch_geometric import _cabi
    return _cabi


@pytest.fixture(scope="module")
def graph():
    counts, edges = load_fake_hetero()
    node_types, edge_types = sorted(counts), sorted(edges)
    P, I = {}, {}
    for et in edge_types:
        P[rel_key(et)], I[rel_key(et)], _ = orc.to_csc(edges[et], (counts[et[0]], counts[et[2]]))
    return node_types, edge_types, P, I


def _dev(a):
    return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(DEV)


def _batched(cabi, graph, calls, calls_ts, ns, hops, rts=None, timerange=None, pad=0):
    """calls: per call a dict type -> seeds (the same types and lengths in every call); calls_ts likewise or None."""
    node_types, edge_types, P, I = graph
    tix = {t: i for i, t in enumerate(node_types)}
    rels = [(tix[et[0]], tix[et[2]], _dev(P[rel_key(et)]), _dev(I[rel_key(et)]),
             _dev(rts[rel_key(et)]) if rts is not None and rel_key(et) in rts else None) for et in edge_types]
    slab = lambda per_call, t: _dev(np.stack([np.asarray(c[t], dtype=np.int64) for c in per_call])) if t in per_call[0] else None
    inputs = [slab(calls, t) for t in node_types]
    input_ts = [slab(calls_ts, t) for t in node_types] if calls_ts is not None else None
    hb = cabi.HgtBatched(len(node_types), rels, inputs, [ns.get(t) for t in node_types], hops, len(calls), DEV,
                         input_ts=input_ts, timerange=timerange, pad=pad)
    if pad:
        for slabs in (hb.samples, hb.sample_ts, hb.rows, hb.cols, hb.edge_index):
            for x in slabs:
                x.fill_(SENTINEL)
    return hb


def _check(tg, cabi, graph, calls, calls_ts, ns, hops, seed, rts=None, timerange=None, pad=0, call_id0=0, panics=()):
    """One batched launch against the oracle and against the single calls, call by call."""
    node_types, edge_types, P, I = graph
    T, R = len(node_types), len(edge_types)
    hb = _batched(cabi, graph, calls, calls_ts, ns, hops, rts, timerange, pad)
    hb.run(seed, call_id0)
    counts = hb.counts.cpu().numpy()
    tg.seed(seed)
    for _ in range(call_id0):                                   # the single calls' ids start at call_id0
        tg.hgt_sampling(node_types, edge_types, {k: _dev(v) for k, v in P.items()}, {k: _dev(v) for k, v in I.items()},
                        None, {node_types[0]: _dev([0])}, None, {t: [0] * hops for t in node_types}, hops)
    Pd, Id = {k: _dev(v) for k, v in P.items()}, {k: _dev(v) for k, v in I.items()}
    rtsd = {k: _dev(v) for k, v in rts.items()} if rts is not None else None
    for b, c in enumerate(calls):
        cts = calls_ts[b] if calls_ts is not None else None
        got = hb.call(b, counts)
        assert got[5] == (1 if b in panics else 0), b
        if b in panics:
            with pytest.raises(RuntimeError, match="panic"):
                orc.hgt(node_types, edge_types, P, I, rts, c, cts, ns, hops, orc.rng_philox(seed, call_id0 + b),
                        timerange=timerange)
            with pytest.raises(RuntimeError, match="reference panics"):
                tg.hgt_sampling(node_types, edge_types, Pd, Id, rtsd, {k: _dev(v) for k, v in c.items()},
                                {k: _dev(v) for k, v in cts.items()} if cts is not None else None, ns, hops, timerange)
            continue
        o = orc.hgt(node_types, edge_types, P, I, rts, c, cts, ns, hops, orc.rng_philox(seed, call_id0 + b),
                    timerange=timerange)
        s = tg.hgt_sampling(node_types, edge_types, Pd, Id, rtsd, {k: _dev(v) for k, v in c.items()},
                            {k: _dev(v) for k, v in cts.items()} if cts is not None else None, ns, hops, timerange)
        for t, nt in enumerate(node_types):
            for k in (0, 1):                                    # samples, sample timestamps
                g = got[k][t].cpu().numpy()
                assert np.array_equal(g, o[k][nt]), (b, nt, k)
                assert np.array_equal(g, s[k][nt].cpu().numpy()), (b, nt, k)
        for r, et in enumerate(edge_types):
            key = rel_key(et)
            for k in (2, 3, 4):                                 # rows, cols, edge_index
                g = got[k][r].cpu().numpy()
                assert np.array_equal(g, o[k][key]), (b, key, k)
                assert np.array_equal(g, s[k][key].cpu().numpy()), (b, key, k)
    if pad:                                                     # nothing written past a call's counts
        for t in range(T):
            for x in (hb.samples[t], hb.sample_ts[t]):
                tail = torch.arange(x.shape[1], device=DEV)[None, :] >= hb.counts[:, t:t + 1]
                assert bool((x[tail] == SENTINEL).all()), t
        for r in range(R):
            for x in (hb.rows[r], hb.cols[r], hb.edge_index[r]):
                tail = torch.arange(x.shape[1], device=DEV)[None, :] >= hb.counts[:, T + r:T + r + 1]
                assert bool((x[tail] == SENTINEL).all()), r
    return hb, counts


@pytest.mark.parametrize("n_calls", [1, 3, 64, 257])
def test_batched_equals_oracle_and_single_calls(tg, cabi, graph, n_calls):
    node_types = graph[0]
    rs = np.random.default_rng(n_calls)
    calls = [{t: rs.integers(0, 800, 4) for t in node_types} for _ in range(n_calls)]
    _check(tg, cabi, graph, calls, None, {t: [20, 15] for t in node_types}, 2, 11 + n_calls, call_id0=5 if n_calls == 3 else 0)


def test_batched_distinct_seed_sets_with_repeats(tg, cabi, graph):
    rs = np.random.default_rng(3)
    calls = [{"v0": rs.integers(0, 40, 40), "v2": rs.integers(0, 5, 3)} for _ in range(24)]   # repeated seeds in a call
    _check(tg, cabi, graph, calls, None, {t: [64, 48, 32] for t in graph[0]}, 3, 2)


def test_batched_input_and_row_timestamps_with_timerange(tg, cabi, graph):
    node_types, edge_types, P, I = graph
    g = np.random.default_rng(5)
    rts = {k: g.integers(-1, 30, len(I[k])) for k in I}
    calls = [{"v0": g.integers(0, 800, 4), "v2": g.integers(0, 800, 2)} for _ in range(20)]
    calls_ts = [{"v0": g.integers(-1, 25, 4), "v2": g.integers(-1, 25, 2)} for _ in range(20)]
    _check(tg, cabi, graph, calls, calls_ts, {t: [10, 6] for t in node_types}, 2, 9, rts=rts, timerange=(5, 20))
    some = {k: v for k, v in list(rts.items())[:3]}                            # row timestamps on some relations only
    calls = [{"v1": g.integers(0, 800, 2)} for _ in range(9)]                  # v0 and v2 have no inputs
    calls_ts = [{"v1": g.integers(0, 25, 2)} for _ in range(9)]
    _check(tg, cabi, graph, calls, calls_ts, {t: [30, 30] for t in node_types}, 2, 10, rts=some)


def test_batched_poisoned_wide_slabs(tg, cabi, graph):
    """Pitches beyond the capacities, slabs filled with a sentinel: every word past a call's counts stays the sentinel."""
    rs = np.random.default_rng(8)
    calls = [{"v1": rs.integers(0, 800, 3)} for _ in range(17)]
    _check(tg, cabi, graph, calls, None, {t: [1000, 1000] for t in graph[0]}, 2, 4, pad=37)   # whole budgets taken
    calls = [{"v0": rs.integers(0, 800, 5), "v2": rs.integers(0, 800, 5)} for _ in range(17)]
    _check(tg, cabi, graph, calls, None, {t: [7, 3] for t in graph[0]}, 2, 6, pad=5)


def test_batched_panic_isolated_to_its_call(tg, cabi):
    """Type X has no num_samples entry.  It owns a budget (the reference panics, hgt_sampling.rs:202) only in the calls
    whose Z seed has a Y neighbour: those calls set their own flag; the others finish and match the oracle.  W has no
    relations and no num_samples entry either (never a budget, never a panic)."""
    node_types = ["W", "X", "Y", "Z"]
    edge_types = [("X", "r", "Y"), ("Y", "s", "Z")]
    e_xy = np.array([[0, 1, 2, 3], [0, 1, 2, 3]])            # x_i -> y_i
    e_yz = np.array([[0, 1, 2], [0, 0, 2]])                  # y0, y1 -> z0; y2 -> z2; z1, z3 have no Y neighbour
    P, I = {}, {}
    P["X__r__Y"], I["X__r__Y"], _ = orc.to_csc(e_xy, (4, 4))
    P["Y__s__Z"], I["Y__s__Z"], _ = orc.to_csc(e_yz, (4, 4))
    g = (node_types, edge_types, P, I)
    calls = [{"Z": [z]} for z in (0, 1, 2, 3, 1, 3, 0)]
    _check(tg, cabi, g, calls, None, {"Y": [1, 1], "Z": [1, 1]}, 2, 3, panics=(0, 2, 6))


def test_batched_scan_limit_refused(cabi, graph):
    """A type past the one-workgroup scan limit (16 384 nodes) is refused with an error naming the limit, before any
    launch; tg_hgt_sample takes the same shape through its library scans (test_gpu_hgt.py)."""
    calls = [{"v0": np.zeros(16385, dtype=np.int64)} for _ in range(2)]
    with pytest.raises(cabi.TchGeoError, match="one-workgroup scan limit"):
        _batched(cabi, graph, calls, None, {t: [1] for t in graph[0]}, 1)


# ---------------------------------------------------------------- cfg4 scale
NODE_TYPES4 = ["A", "B", "C"]
SCALES4 = {"A": 23, "B": 22, "C": 22}
EDGE_TYPES4 = [("A", "e0", "A"), ("A", "e1", "B"), ("B", "e2", "A"), ("B", "e3", "C"), ("C", "e4", "A")]


def test_cfg4_256_calls(tg, cabi):
    """cfg4 (built as bench.py builds it): 256 calls of 1 024 seeds, [512, 512] per type, in one launch chain, against
    the 256 single calls on the device and against the oracle on two calls."""
    P, I = {}, {}
    for r, (s, _, d) in enumerate(EDGE_TYPES4):
        rw, cl = cabi.rmat_edges_rect(SCALES4[s], SCALES4[d], 20_000_000, 0xC0F4 + r, DEV)
        P[rel_key(EDGE_TYPES4[r])], I[rel_key(EDGE_TYPES4[r])], _ = cabi.coo_to_csx(rw, cl, 1 << SCALES4[s], 1 << SCALES4[d], True)
    del rw, cl
    N, seed = 256, 77
    seeds = cabi.seed_batches(0xBA7C4, 9000, N, 1024, 1 << SCALES4["A"], DEV)
    rels = [(0, 0, P["A__e0__A"], I["A__e0__A"], None), (0, 1, P["A__e1__B"], I["A__e1__B"], None),
            (1, 0, P["B__e2__A"], I["B__e2__A"], None), (1, 2, P["B__e3__C"], I["B__e3__C"], None),
            (2, 0, P["C__e4__A"], I["C__e4__A"], None)]
    ns = {t: [512, 512] for t in NODE_TYPES4}
    hb = cabi.HgtBatched(3, rels, [seeds, None, None], [ns[t] for t in NODE_TYPES4], 2, N, DEV)
    hb.run(seed, 0)
    counts = hb.counts.cpu().numpy()
    assert counts[:, 8].sum() == 0 and counts[:, 3:8].sum() > N * 10_000          # no panics; edges
    tg.seed(seed)
    for b in range(N):
        s = tg.hgt_sampling(NODE_TYPES4, EDGE_TYPES4, P, I, None, {"A": seeds[b]}, None, ns, 2)
        got = hb.call(b, counts)
        for t, nt in enumerate(NODE_TYPES4):
            assert torch.equal(got[0][t], s[0][nt]) and torch.equal(got[1][t], s[1][nt]), (b, nt)
        for r, et in enumerate(EDGE_TYPES4):
            k = rel_key(et)
            assert torch.equal(got[2][r], s[2][k]) and torch.equal(got[3][r], s[3][k]) and torch.equal(got[4][r], s[4][k]), (b, k)
    hP = {k: v.cpu().numpy() for k, v in P.items()}
    hI = {k: v.cpu().numpy() for k, v in I.items()}
    for b in (0, 201):
        o = orc.hgt(NODE_TYPES4, EDGE_TYPES4, hP, hI, None, {"A": seeds[b].cpu().numpy()}, None, ns, 2, orc.rng_philox(seed, b))
        got = hb.call(b, counts)
        for t, nt in enumerate(NODE_TYPES4):
            assert np.array_equal(got[0][t].cpu().numpy(), o[0][nt]), (b, nt)
        for r, et in enumerate(EDGE_TYPES4):
            assert np.array_equal(got[3][r].cpu().numpy(), o[3][rel_key(et)]), (b, et)
            assert np.array_equal(got[4][r].cpu().numpy(), o[4][rel_key(et)]), (b, et)


# ---------------------------------------------------------------- HGTLoader
def _hetero_data():
    from tch_geometric.transforms import HeteroGraph
    counts, edges = load_fake_hetero()
    node_types, edge_types = sorted(counts), sorted(edges)
    rs = np.random.default_rng(4)
    data, feats, ets = HeteroGraph(), {}, {}
    for nt in node_types:
        feats[nt] = rs.standard_normal((counts[nt], 6)).astype(np.float32)
        data[nt].x, data[nt].num_nodes = torch.from_numpy(feats[nt]).to(DEV), counts[nt]
    for et in edge_types:
        data[et].edge_index = torch.from_numpy(edges[et]).to(DEV)
        ets[et] = rs.integers(0, 100, edges[et].shape[1])
        data[et].timestamps = torch.from_numpy(ets[et]).to(DEV)
    P, I, PERM = {}, {}, {}
    for et in edge_types:
        P[rel_key(et)], I[rel_key(et)], PERM[rel_key(et)] = orc.to_csc(edges[et], (counts[et[0]], counts[et[2]]))
    return data, node_types, edge_types, counts, feats, ets, P, I, PERM


@pytest.mark.parametrize("temporal", [False, True])
def test_hgt_loader_two_epochs_ragged_attributes(temporal):
    """Every mini-batch of two epochs (150 seeds, batches of 32: four full and a ragged one, three per launch) equals
    the oracle with (seed, call_id0 + j); node and edge attributes ride along; temporal mode passes row timestamps,
    per-seed input timestamps and the time range."""
    from tch_geometric.loader import HGTLoader
    data, node_types, edge_types, counts, feats, ets, P, I, PERM = _hetero_data()
    rs = np.random.default_rng(6)
    nt0 = node_types[0]
    nodes = torch.from_numpy(rs.integers(0, counts[nt0], 150))
    in_ts = torch.from_numpy(rs.integers(0, 100, 150)) if temporal else None
    tr = (10, 80) if temporal else None
    loader = HGTLoader(data, [12, 8], nt0, input_nodes=nodes, batch_size=32, prefetch=3, temporal=temporal,
                       input_timestamps=in_ts, timerange=tr, seed=5, call_id0=40)
    assert len(loader) == 5 and loader.prefetch == 3
    rts = {rel_key(et): ets[et][PERM[rel_key(et)]] for et in edge_types} if temporal else None
    ns = {t: [12, 8] for t in node_types}
    for epoch in range(2):
        n_seen = 0
        for j, b in enumerate(loader):
            sl = slice(j * 32, (j + 1) * 32)
            seeds = nodes[sl].numpy()
            cid = 40 + epoch * 5 + j
            o = orc.hgt(node_types, edge_types, P, I, rts, {nt0: seeds}, {nt0: in_ts[sl].numpy()} if temporal else None,
                        ns, 2, orc.rng_philox(5, cid), timerange=tr)
            for nt in node_types:
                s = b[nt].n_id.cpu().numpy()
                assert np.array_equal(s, o[0][nt]), (epoch, j, nt)
                assert np.array_equal(b.samples_timestamps[nt].cpu().numpy(), o[1][nt]), (epoch, j, nt)
                assert np.array_equal(b[nt].x.cpu().numpy(), feats[nt][s])
                assert b[nt].num_nodes == len(s)
            for et in edge_types:
                k = rel_key(et)
                assert np.array_equal(b[et].edge_index.cpu().numpy(), np.stack([o[2][k], o[3][k]])), (epoch, j, k)
                assert np.array_equal(b[et].e_id.cpu().numpy(), PERM[k][o[4][k]])
                assert np.array_equal(b[et].timestamps.cpu().numpy(), ets[et][PERM[k][o[4][k]]])
            assert b[nt0].batch_size == len(seeds) and b.call_id == cid
            n_seen += 1
        assert n_seen == 5


def test_hgt_loader_workspace_clamp():
    """prefetch is clamped so that a launch's workspace stays within max_workspace_bytes (at least one call)."""
    from tch_geometric import _cabi
    from tch_geometric.loader import HGTLoader
    data, node_types = _hetero_data()[:2]
    loader = HGTLoader(data, [12, 8], node_types[0], batch_size=32, prefetch=1000)
    per_call = _cabi.hgt_batched_workspace_bytes(loader._problem(32), 1)
    assert loader.prefetch == min(1000, (4 << 30) // per_call)
    small = HGTLoader(data, [12, 8], node_types[0], batch_size=32, prefetch=1000, max_workspace_bytes=3 * per_call + 1)
    assert small.prefetch == 3
    assert HGTLoader(data, [12, 8], node_types[0], batch_size=32, max_workspace_bytes=1).prefetch == 1
