"""GPU parity of batched budget_sampling (tg_budget_sample_batched): call b of a launch equals the oracle with call id
call_id0 + b and the single call (tg_budget_sample through budget_sampling) with that call id, word for word -- samples,
sample timestamps, rows, cols, edge_index and counts.  Then the same at cfg4's scale, and BudgetLoader."""
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


def _batched(cabi, graph, calls, calls_ts, nn, hops, rts=None, window=None, forward=False, relative=False, pad=0):
    """calls: per call a dict type -> seeds (the same types and lengths in every call); calls_ts likewise or None."""
    node_types, edge_types, P, I = graph
    tix = {t: i for i, t in enumerate(node_types)}
    rels = [(tix[et[0]], tix[et[2]], _dev(P[rel_key(et)]), _dev(I[rel_key(et)]),
             _dev(rts[rel_key(et)]) if rts is not None and rel_key(et) in rts else None) for et in edge_types]
    slab = lambda per_call, t: _dev(np.stack([np.asarray(c[t], dtype=np.int64) for c in per_call])) if t in per_call[0] else None
    inputs = [slab(calls, t) for t in node_types]
    input_ts = [slab(calls_ts, t) for t in node_types] if calls_ts is not None else None
    bb = cabi.BudgetBatched(len(node_types), rels, inputs, [nn[t] for t in node_types], hops, len(calls), DEV,
                            input_ts=input_ts, window=window, forward=forward, relative=relative, pad=pad)
    if pad:
        for slabs in (bb.samples, bb.sample_ts, bb.rows, bb.cols, bb.edge_index):
            for x in slabs:
                x.fill_(SENTINEL)
    return bb


def _check(tg, cabi, graph, calls, calls_ts, nn, hops, seed, rts=None, window=None, forward=False, relative=False, pad=0,
           call_id0=0):
    """One batched launch against the oracle and against the single calls, call by call."""
    node_types, edge_types, P, I = graph
    T, R = len(node_types), len(edge_types)
    bb = _batched(cabi, graph, calls, calls_ts, nn, hops, rts, window, forward, relative, pad)
    bb.run(seed, call_id0)
    counts = bb.counts.cpu().numpy()
    Pd, Id = {k: _dev(v) for k, v in P.items()}, {k: _dev(v) for k, v in I.items()}
    rtsd = {k: _dev(v) for k, v in rts.items()} if rts is not None else None
    n_edges = 0
    for b, c in enumerate(calls):
        cts = calls_ts[b] if calls_ts is not None else None
        got = bb.call(b, counts)
        o = orc.budget(node_types, edge_types, P, I, rts, c, cts, nn, hops, orc.rng_philox(seed, call_id0 + b), window=window,
                       forward=forward, relative=relative)
        tg.set_rng_state(seed, call_id0 + b)
        s = tg.budget_sampling(node_types, edge_types, Pd, Id, rtsd, {k: _dev(v) for k, v in c.items()},
                               {k: _dev(v) for k, v in cts.items()} if cts is not None else None, nn, hops, window, forward,
                               relative)
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
            n_edges += len(o[2][key])
    if pad:                                                     # nothing written past a call's counts, nor into the next row
        for t in range(T):
            for x in (bb.samples[t], bb.sample_ts[t]):
                tail = torch.arange(x.shape[1], device=DEV)[None, :] >= bb.counts[:, t:t + 1]
                assert bool((x[tail] == SENTINEL).all()), t
        for r in range(R):
            for x in (bb.rows[r], bb.cols[r], bb.edge_index[r]):
                tail = torch.arange(x.shape[1], device=DEV)[None, :] >= bb.counts[:, T + r:T + r + 1]
                assert bool((x[tail] == SENTINEL).all()), r
    return bb, n_edges


@pytest.mark.parametrize("n_calls", [1, 3, 64, 257])
def test_batched_equals_oracle_and_single_calls(tg, cabi, graph, n_calls):
    """Inputs in two of the types, none in the others."""
    node_types = graph[0]
    rs = np.random.default_rng(n_calls)
    calls = [{"v0": rs.integers(0, 800, 4), "v2": rs.integers(0, 800, 3)} for _ in range(n_calls)]
    _, n_edges = _check(tg, cabi, graph, calls, None, {t: [5, 3] for t in node_types}, 2, 11 + n_calls,
                        call_id0=5 if n_calls == 3 else 0)
    assert n_edges > 10 * n_calls


@pytest.mark.parametrize("relative", [False, True])
@pytest.mark.parametrize("forward", [False, True])
def test_batched_timestamps_and_window(tg, cabi, graph, forward, relative):
    """Input and row timestamps (-1 = missing), some relations without row timestamps, the window filter."""
    node_types, edge_types, P, I = graph
    g = np.random.default_rng(7 + 2 * forward + relative)
    rts = {k: g.integers(-1, 12, len(I[k])) for k in list(I)[:4]}
    calls = [{"v0": g.integers(0, 800, 5), "v1": g.integers(0, 800, 2)} for _ in range(21)]
    calls_ts = [{"v0": g.integers(-1, 8, 5), "v1": g.integers(0, 8, 2)} for _ in range(21)]
    _check(tg, cabi, graph, calls, calls_ts, {t: [4, 2, 2] for t in node_types}, 3, 5, rts=rts, window=(0, 4),
           forward=forward, relative=relative, call_id0=100)
    # timestamps without a filter, and a window without input timestamps
    _check(tg, cabi, graph, calls, calls_ts, {t: [6, 3] for t in node_types}, 2, 6, rts=rts)
    _check(tg, cabi, graph, calls, None, {t: [6, 3] for t in node_types}, 2, 7, rts=rts, window=(-3, 3), forward=forward,
           relative=relative)


def test_batched_repeats_zero_quotas_no_hops(tg, cabi, graph):
    node_types = graph[0]
    rs = np.random.default_rng(3)
    calls = [{"v0": rs.integers(0, 40, 40), "v2": rs.integers(0, 5, 3)} for _ in range(24)]   # repeated seeds in a call
    nn = {t: [[60, 0, 5], [0, 7, 0], [3, 3, 0]][i % 3] for i, t in enumerate(node_types)}      # zero quotas, one above 50
    _check(tg, cabi, graph, calls, None, nn, 3, 2)
    _check(tg, cabi, graph, calls, None, {t: [] for t in node_types}, 0, 3)                   # no hops: the inputs only


def test_batched_poisoned_wide_slabs(tg, cabi, graph):
    """Pitches beyond the capacities, slabs filled with a sentinel: every word past a call's counts stays the sentinel."""
    rs = np.random.default_rng(8)
    calls = [{"v1": rs.integers(0, 800, 3)} for _ in range(17)]
    _check(tg, cabi, graph, calls, None, {t: [64, 64] for t in graph[0]}, 2, 4, pad=37)       # every candidate taken
    calls = [{"v0": rs.integers(0, 800, 5), "v2": rs.integers(0, 800, 5)} for _ in range(17)]
    _check(tg, cabi, graph, calls, None, {t: [7, 3] for t in graph[0]}, 2, 6, pad=5)


# ---------------------------------------------------------------- cfg4 scale
NODE_TYPES4 = ["A", "B", "C"]
SCALES4 = {"A": 23, "B": 22, "C": 22}
EDGE_TYPES4 = [("A", "e0", "A"), ("A", "e1", "B"), ("B", "e2", "A"), ("B", "e3", "C"), ("C", "e4", "A")]


def test_cfg4_256_calls(tg, cabi):
    """cfg4 (built as tools/bench_misc.py builds it): 256 calls of 1 024 seeds, [15, 10] per type, in one launch chain,
    against the 256 single calls on the device and against the oracle on two calls."""
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
    nn = {t: [15, 10] for t in NODE_TYPES4}
    bb = cabi.BudgetBatched(3, rels, [seeds, None, None], [nn[t] for t in NODE_TYPES4], 2, N, DEV)
    bb.run(seed, 0)
    counts = bb.counts.cpu().numpy()
    assert counts[:, :3].sum() > N * 10_000 and counts[:, 3:].sum() > N * 10_000                # nodes; edges
    tg.seed(seed)
    for b in range(N):
        s = tg.budget_sampling(NODE_TYPES4, EDGE_TYPES4, P, I, None, {"A": seeds[b]}, None, nn, 2, None, False, False)
        got = bb.call(b, counts)
        for t, nt in enumerate(NODE_TYPES4):
            assert torch.equal(got[0][t], s[0][nt]) and torch.equal(got[1][t], s[1][nt]), (b, nt)
        for r, et in enumerate(EDGE_TYPES4):
            k = rel_key(et)
            assert torch.equal(got[2][r], s[2][k]) and torch.equal(got[3][r], s[3][k]) and torch.equal(got[4][r], s[4][k]), (b, k)
    hP = {k: v.cpu().numpy() for k, v in P.items()}
    hI = {k: v.cpu().numpy() for k, v in I.items()}
    for b in (0, 201):
        o = orc.budget(NODE_TYPES4, EDGE_TYPES4, hP, hI, None, {"A": seeds[b].cpu().numpy()}, None, nn, 2, orc.rng_philox(seed, b))
        got = bb.call(b, counts)
        for t, nt in enumerate(NODE_TYPES4):
            assert np.array_equal(got[0][t].cpu().numpy(), o[0][nt]), (b, nt)
        for r, et in enumerate(EDGE_TYPES4):
            for k in (2, 3, 4):
                assert np.array_equal(got[k][r].cpu().numpy(), o[k][rel_key(et)]), (b, et, k)


# ---------------------------------------------------------------- BudgetLoader
def _hetero_data():
    from tch_geometric.transforms import HeteroGraph
    counts, edges = load_fake_hetero()
    node_types, edge_types = sorted(counts), sorted(edges)
    rs = np.random.default_rng(4)
    data, feats, ets, eattr = HeteroGraph(), {}, {}, {}
    for nt in node_types:
        feats[nt] = rs.standard_normal((counts[nt], 6)).astype(np.float32)
        data[nt].x, data[nt].num_nodes = torch.from_numpy(feats[nt]).to(DEV), counts[nt]
    for et in edge_types:
        data[et].edge_index = torch.from_numpy(edges[et]).to(DEV)
        ets[et] = rs.integers(0, 100, edges[et].shape[1])
        eattr[et] = rs.standard_normal((edges[et].shape[1], 3)).astype(np.float32)
        data[et].timestamps = torch.from_numpy(ets[et]).to(DEV)
        data[et].edge_attr = torch.from_numpy(eattr[et]).to(DEV)
    P, I, PERM = {}, {}, {}
    for et in edge_types:
        P[rel_key(et)], I[rel_key(et)], PERM[rel_key(et)] = orc.to_csc(edges[et], (counts[et[0]], counts[et[2]]))
    return data, node_types, edge_types, counts, edges, feats, ets, eattr, P, I, PERM


@pytest.mark.parametrize("temporal", [False, True])
def test_budget_loader_two_epochs_ragged_attributes(temporal):
    """Every mini-batch of two epochs (150 seeds, batches of 32: four full and a ragged one, three per launch) equals
    the oracle with (seed, call_id0 + j); e_id maps every sampled edge back to its COO edge (edge_index[:, e_id] ==
    (n_id_src[row], n_id_dst[col])); node and edge attributes ride along; temporal mode passes row timestamps, per-seed
    input timestamps and the window filter."""
    from tch_geometric.loader import BudgetLoader
    data, node_types, edge_types, counts, edges, feats, ets, eattr, P, I, PERM = _hetero_data()
    rs = np.random.default_rng(6)
    nt0 = node_types[0]
    nodes = torch.from_numpy(rs.integers(0, counts[nt0], 150))
    in_ts = torch.from_numpy(rs.integers(0, 100, 150)) if temporal else None
    window = (0, 40) if temporal else None
    loader = BudgetLoader(data, [12, 8], nt0, input_nodes=nodes, batch_size=32, prefetch=3, temporal=temporal,
                          input_timestamps=in_ts, window=window, forward=False, relative=temporal, seed=5, call_id0=40)
    assert len(loader) == 5 and loader.prefetch == 3
    rts = {rel_key(et): ets[et][PERM[rel_key(et)]] for et in edge_types} if temporal else None
    nn = {t: [12, 8] for t in node_types}
    n_edges = 0
    for epoch in range(2):
        n_seen = 0
        for j, b in enumerate(loader):
            sl = slice(j * 32, (j + 1) * 32)
            seeds = nodes[sl].numpy()
            cid = 40 + epoch * 5 + j
            o = orc.budget(node_types, edge_types, P, I, rts, {nt0: seeds}, {nt0: in_ts[sl].numpy()} if temporal else None,
                           nn, 2, orc.rng_philox(5, cid), window=window, forward=False, relative=temporal)
            n_id = {}
            for nt in node_types:
                n_id[nt] = b[nt].n_id.cpu().numpy()
                assert np.array_equal(n_id[nt], o[0][nt]), (epoch, j, nt)
                assert np.array_equal(b.samples_timestamps[nt].cpu().numpy(), o[1][nt]), (epoch, j, nt)
                assert np.array_equal(b[nt].x.cpu().numpy(), feats[nt][n_id[nt]])
                assert b[nt].num_nodes == len(n_id[nt])
            for et in edge_types:
                k = rel_key(et)
                ei = b[et].edge_index.cpu().numpy()
                e_id = b[et].e_id.cpu().numpy()
                assert np.array_equal(ei, np.stack([o[2][k], o[3][k]])), (epoch, j, k)
                want = PERM[k][P[k][o[0][et[2]][o[3][k]]] + o[4][k]]          # the index inside the column -> COO edge
                assert np.array_equal(e_id, want), (epoch, j, k)
                assert np.array_equal(edges[et][:, e_id], np.stack([n_id[et[0]][ei[0]], n_id[et[2]][ei[1]]]))
                assert np.array_equal(b[et].timestamps.cpu().numpy(), ets[et][e_id])
                assert np.array_equal(b[et].edge_attr.cpu().numpy(), eattr[et][e_id])
                n_edges += len(e_id)
            assert b[nt0].batch_size == len(seeds) and b.call_id == cid
            n_seen += 1
        assert n_seen == 5
    assert n_edges > 500


def test_budget_loader_prefetch_clamp_counts_slabs():
    """prefetch is clamped so that a launch's workspace AND output slabs stay within max_workspace_bytes (at least one
    call); the slabs, sized for the worst case, are most of it."""
    from tch_geometric import _cabi
    from tch_geometric.loader import BudgetLoader
    data, node_types = _hetero_data()[:2]
    loader = BudgetLoader(data, [12, 8], node_types[0], batch_size=32, prefetch=1000)
    p = loader._problem(32)
    per_call = _cabi.budget_batched_bytes(p, 1)
    ws = _cabi.budget_batched_workspace_bytes(p, 1)
    pn, pe = _cabi.budget_batched_pitches(p)
    assert per_call == ws + 8 * (2 * sum(pn) + 3 * sum(pe) + len(pn) + len(pe)) and per_call > 2 * ws
    assert loader.prefetch == min(1000, (4 << 30) // per_call)
    small = BudgetLoader(data, [12, 8], node_types[0], batch_size=32, prefetch=1000, max_workspace_bytes=3 * per_call + 1)
    assert small.prefetch == 3
    ws_only = BudgetLoader(data, [12, 8], node_types[0], batch_size=32, prefetch=1000, max_workspace_bytes=3 * ws + 1)
    assert ws_only.prefetch == 1                                 # three workspaces fit, not three calls' slabs
    assert BudgetLoader(data, [12, 8], node_types[0], batch_size=32, max_workspace_bytes=1).prefetch == 1
