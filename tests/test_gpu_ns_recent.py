"""TG_SAMPLER_RECENT on the device: the flat hop (tg_ns_hop_recent), the batched launch (tg_ns_homo_batched_ws through the
generalised flat driver), the status codes and the operator surface, every output compared for exact equality with the
NumPy restatement in helpers_recent.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers_recent import (HUB_DEGREE, recent_hop, recent_ns_homo, recent_test_graph, recent_test_times)

pytestmark = pytest.mark.gpu
POISON = -777
TIMES = ["ties", "asc", "desc", "wide"]
# (filter_mode, forward): none in both directions, STATIC, RELATIVE and DYNAMIC each forward and backward
FILTERS = [(-1, False), (-1, True), (0, False), (1, True), (1, False), (2, True), (2, False)]


@pytest.fixture(scope="module")
def cabi():
    from tch_geometric import _cabi
    return _cabi


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def graph():
    return recent_test_graph()


@pytest.fixture(scope="module")
def times(graph):
    ptrs, _, _, _, hub = graph
    return {k: recent_test_times(ptrs, hub, k) for k in TIMES}


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


def _view(cabi, dev, graph, ts, narrow=True):
    ptrs, idx = graph[0], graph[1]
    P, I = _t(dev, ptrs), _t(dev, idx)
    kw = dict(indices32=I.to(torch.int32), ptrs32=P.to(torch.int32)) if narrow else {}
    return cabi.graph_view(P, I, timestamps=_t(dev, ts) if ts is not None else None, **kw)


def _windows(ts, mode):
    """Windows narrow enough to reject every edge of some vertices, wide enough to fill others' fan-outs."""
    lo, hi = int(ts.min()), int(ts.max())
    span = hi - lo
    return (lo + span // 4, lo + span // 2) if mode == 0 else (0, max(span // 4, 1))


def _states(ts, shape, seed):
    lo, hi = int(ts.min()), int(ts.max())
    span = hi - lo
    return np.random.default_rng(seed).integers(lo - span // 4, hi + span // 4 + 1, shape).astype(np.int64)


def _frontier(graph, m, seed):
    """m frontier vertices: every 13th an empty slot, the crafted columns and the hub among the others"""
    _, _, n, crafted, hub = graph
    v = np.random.default_rng(seed).integers(0, n, m).astype(np.int64)
    v[::13] = -1
    free = [i for i in range(m) if i % 13]
    special = np.concatenate([[hub], crafted])[:len(free)]
    v[free[:len(special)]] = special
    return v


def _frontier_states(ts, vertices, hub, seed):
    """random states around the timestamps' range; the hub's is their median, so that its window admits many edges"""
    st = _states(ts, len(vertices), seed)
    st[vertices == hub] = int(np.median(ts))
    return st


def _check_hop(cabi, dev, graph, ts, g, vertices, states, k, mode, forward, window):
    filtered = mode != -1
    want = recent_hop(graph[0], graph[1], ts, vertices, states if filtered else None, k, mode, forward, window)
    got = cabi.ns_hop_recent(g, _t(dev, vertices), k, states=_t(dev, states) if filtered else None, filter_mode=mode,
                             window=window, forward=forward)
    torch.cuda.synchronize()
    cnt, off, nbr, ep, par, sto = want
    tot = int(off[-1])
    assert torch.equal(got[0].cpu(), torch.from_numpy(cnt)), "cnt"
    assert torch.equal(got[1].cpu(), torch.from_numpy(off)), "offsets"
    for name, a, b in (("neighbors", got[2], nbr), ("edge_ptrs", got[3], ep), ("parents", got[4], par)):
        assert torch.equal(a[:tot].cpu(), torch.from_numpy(b)), name
    if filtered:
        assert torch.equal(got[5][:tot].cpu(), torch.from_numpy(sto)), "states_out"
    else:
        assert got[5] is None
    return cnt


@pytest.mark.parametrize("kind", TIMES)
@pytest.mark.parametrize("mode,forward", FILTERS)
def test_flat_hop_equals_the_restatement(cabi, dev, graph, times, kind, mode, forward):
    ts = times[kind]
    g = _view(cabi, dev, graph, ts)
    window = _windows(ts, mode)
    vertices = _frontier(graph, 600, 1)                    # 600: a last partial workgroup of the wavefront-per-vertex kernel
    assert (vertices[::13] == -1).all()
    states = _frontier_states(ts, vertices, graph[4], 2)
    for k in (1, 7, 33, 64):
        cnt = _check_hop(cabi, dev, graph, ts, g, vertices, states, k, mode, forward, window)
        live = vertices >= 0
        assert (cnt[live] == k).any()
        if mode != -1:
            deg = np.diff(graph[0])[np.maximum(vertices, 0)]
            assert ((cnt == 0) & live & (deg > 0)).any()  # the window rejected a whole column
    hub = np.array([graph[4]], dtype=np.int64)            # a frontier of one: the hub alone
    _check_hop(cabi, dev, graph, ts, g, hub, _frontier_states(ts, hub, graph[4], 3), 33, mode, forward, window)
    _check_hop(cabi, dev, graph, ts, g, np.array([-1], dtype=np.int64), states[:1], 7, mode, forward, window)


def test_flat_hop_without_the_u32_shadows_and_with_null_filter(cabi, dev, graph, times):
    """the int64 `ptrs` / `indices` path, and filter = NULL (none, most recent first)"""
    ts = times["wide"]
    g = _view(cabi, dev, graph, ts, narrow=False)
    vertices = _frontier(graph, 100, 4)
    _check_hop(cabi, dev, graph, ts, g, vertices, None, 7, -1, False, (0, 0))
    want = recent_hop(graph[0], graph[1], ts, vertices, None, 5)
    m, o = len(vertices), dict(dtype=torch.int64, device=dev)
    cnt, off = torch.empty(m, **o), torch.empty(m + 1, **o)
    nbr, ep, par = (torch.full((m * 5,), POISON, **o) for _ in range(3))
    hin, hout = cabi.TgHopIn(), cabi.TgHopOut()
    V = _t(dev, vertices)
    hin.vertices, hin.m, hin.fanout, hin.sampler = V.data_ptr(), m, 5, cabi.SAMPLER_RECENT
    hout.cnt, hout.offsets = cnt.data_ptr(), off.data_ptr()
    hout.neighbors, hout.edge_ptrs, hout.parents = nbr.data_ptr(), ep.data_ptr(), par.data_ptr()
    cabi.check(cabi.lib.tg_ns_hop_recent(C.byref(g), C.byref(hin), None, C.byref(hout), None, cabi.stream_ptr(dev)))
    torch.cuda.synchronize()
    tot = int(want[1][-1])
    assert torch.equal(off.cpu(), torch.from_numpy(want[1])) and torch.equal(ep[:tot].cpu(), torch.from_numpy(want[3]))
    assert torch.equal(nbr[:tot].cpu(), torch.from_numpy(want[2])) and torch.equal(par[:tot].cpu(), torch.from_numpy(want[4]))
    assert bool((ep[tot:] == POISON).all()) and bool((par[tot:] == POISON).all())


def _hub_scan_is_exercised(graph, ts):
    """the restatement's own view of the hub under both timestamp orders: the winners sit at the column's two ends"""
    ptrs, idx, _, _, hub = graph
    return recent_hop(ptrs, idx, ts, [hub], None, 64)[3] - ptrs[hub]


def test_hub_orders_put_the_winners_at_opposite_ends(graph, times):
    assert _hub_scan_is_exercised(graph, times["asc"]).tolist() == list(range(HUB_DEGREE - 1, HUB_DEGREE - 65, -1))
    assert _hub_scan_is_exercised(graph, times["desc"]).tolist() == list(range(64))


# ---------------------------------------------------------------- batched
BATCHED = [(1, 50, [64]), (3, 50, [5, 3]), (3, 7, [2, 2, 2]), (300, 4, [3, 2])]   # 300: past the other samplers' 256-batch switch


def _seeds(graph, n_batches, n_seeds, seed):
    _, _, n, crafted, hub = graph
    s = np.random.default_rng(seed).integers(0, n, (n_batches, n_seeds)).astype(np.int64)
    s[0, 0] = s[0, 1] = hub                               # a duplicate seed inside a batch
    s[0, 2:2 + min(n_seeds - 2, len(crafted))] = crafted[:max(0, min(n_seeds - 2, len(crafted)))]
    if n_batches > 1:
        s[1] = s[0]                                       # a duplicate batch
    return s


def _launch(cabi, dev, g, seeds, fanout, states, mode, forward, window, rng=(1, 2), poison=True):
    B, S = seeds.shape
    out = cabi.NsBatchedOut(B, S, fanout, dev, with_states=True)
    if poison:
        for t in (out.samples, out.rows, out.cols, out.edge_index, out.states):
            t.fill_(POISON)
    ws = cabi.ns_homo_batched_workspace(g, B, S, fanout, dev, sampler=cabi.SAMPLER_RECENT, filter_mode=mode)
    assert ws is not None
    cabi.ns_homo_batched(g, _t(dev, seeds), fanout, rng[0], rng[1], out, sampler=cabi.SAMPLER_RECENT, filter_mode=mode,
                         forward=forward, window=window, seeds_state=_t(dev, states) if mode != -1 else None, ws=ws)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n_batches,n_seeds,fanout", BATCHED)
@pytest.mark.parametrize("kind,mode,forward", [("ties", -1, False), ("wide", 1, False), ("asc", 2, True), ("desc", 0, True)])
def test_batched_equals_the_restatement(cabi, dev, graph, times, n_batches, n_seeds, fanout, kind, mode, forward):
    ts = times[kind]
    g = _view(cabi, dev, graph, ts)
    window = _windows(ts, mode)
    seeds = _seeds(graph, n_batches, n_seeds, 11)
    states = _states(ts, seeds.shape, 12)
    states[0, 1] = states[0, 0]
    if n_batches > 1:
        states[1] = states[0]
    out = _launch(cabi, dev, g, seeds, fanout, states, mode, forward, window)
    S, R, Cc, E, ST = (t.cpu().numpy() for t in (out.samples, out.rows, out.cols, out.edge_index, out.states))
    LO, CN = out.layer_offsets.cpu().numpy(), out.counts.cpu().numpy()
    H = len(fanout)
    for b in range(n_batches):
        s, r, c, e, lo, counts, st = recent_ns_homo(graph[0], graph[1], ts, seeds[b], fanout,
                                                    states[b] if mode != -1 else None, mode, forward, window)
        ns, ne = counts
        assert tuple(CN[b]) == (ns, ne), b
        assert [tuple(x) for x in LO[b, :H]] == lo, b
        for name, slab, want, n in (("samples", S, s, ns), ("rows", R, r, ne), ("cols", Cc, c, ne), ("edge_index", E, e, ne)):
            assert np.array_equal(slab[b, :n], want), (b, name)
            assert (slab[b, n:] == POISON).all(), (b, name, "written past its recorded length")
        if mode != -1:
            assert np.array_equal(ST[b, :ns], st), (b, "states")
            assert (ST[b, ns:] == POISON).all(), b
        else:
            assert (ST[b] == POISON).all(), b            # no filter: no states are kept
    # duplicate seeds (same vertex, same state) give identical subtrees: hop 0's samples of slots 0 and 1
    k0 = fanout[0]
    c0 = Cc[0, :CN[0, 1]]
    first = S[0, n_seeds:][:len(c0)]
    assert np.array_equal(first[c0 == 0], first[c0 == 1]) and (c0 == 0).sum() <= k0
    if n_batches > 1:                                     # ... and identical batches, whatever their call ids
        for slab in (S, R, Cc, E):
            assert np.array_equal(slab[0], slab[1])
    # no draw is made: another tg_rng changes nothing
    again = _launch(cabi, dev, g, seeds, fanout, states, mode, forward, window, rng=(0xDEAD, 99))
    for a, b_ in ((out.samples, again.samples), (out.rows, again.rows), (out.cols, again.cols),
                  (out.edge_index, again.edge_index), (out.states, again.states), (out.counts, again.counts),
                  (out.layer_offsets, again.layer_offsets)):
        assert torch.equal(a, b_)


# ---------------------------------------------------------------- status codes
def _raw_launch(cabi, dev, g, seeds, fanout, out, ws, ws_bytes, use_ws=True, mode=-1):
    cfg = cabi.TgNsConfig()
    cfg.sampler, cfg.filter_mode = cabi.SAMPLER_RECENT, mode
    rng = cabi.TgRng(1, 2)
    fan = (C.c_int64 * len(fanout))(*fanout)
    so = out.struct()
    args = (C.byref(g), cabi.ptr(seeds), C.c_int64(seeds.shape[0]), C.c_int64(seeds.shape[1]), fan, C.c_int32(len(fanout)),
            C.byref(cfg), C.byref(rng), C.byref(so))
    if use_ws:
        return cabi.lib.tg_ns_homo_batched_ws(*args, cabi.ptr(ws), C.c_int64(ws_bytes), C.c_int32(0), cabi.stream_ptr(dev))
    return cabi.lib.tg_ns_homo_batched(*args, cabi.stream_ptr(dev))


def test_refusals_are_invalid_and_launch_nothing(cabi, dev, graph, times):
    ts = times["ties"]
    g, g_bare = _view(cabi, dev, graph, ts), _view(cabi, dev, graph, None)
    seeds = _t(dev, _seeds(graph, 2, 8, 5))
    out = cabi.NsBatchedOut(2, 8, [65], dev, with_states=True)
    slabs = (out.samples, out.rows, out.cols, out.edge_index, out.counts)
    for t in slabs:
        t.fill_(POISON)
    need = C.c_int64(0)
    cfg = cabi.TgNsConfig()
    cfg.sampler, cfg.filter_mode = cabi.SAMPLER_RECENT, -1
    fan2 = (C.c_int64 * 2)(3, 2)
    assert cabi.lib.tg_ns_homo_batched_workspace_bytes(C.byref(g), C.c_int64(2), C.c_int64(8), fan2, C.c_int32(2),
                                                       C.byref(cfg), C.byref(need)) == 0
    assert need.value > 0
    ws = torch.empty(need.value // 8 + 64, dtype=torch.int64, device=dev)
    big = ws.numel() * 8
    err = lambda: cabi.lib.tg_last_error().decode()
    assert _raw_launch(cabi, dev, g_bare, seeds, [3, 2], out, ws, big) == 1 and "timestamps" in err()
    assert _raw_launch(cabi, dev, g, seeds, [65], out, ws, big) == 1 and "1..64" in err()
    assert _raw_launch(cabi, dev, g, seeds, [3, 2], out, None, 0, use_ws=False) == 1 and "workspace" in err()
    assert _raw_launch(cabi, dev, g, seeds, [3, 2], out, ws, need.value - 1) == 1 and "too small" in err()
    assert _raw_launch(cabi, dev, g, seeds, [3, 2], out, ws[1:], big - 8) == 1 and "aligned" in err()
    ids = torch.zeros_like(seeds)
    cfg.seed_ids, cfg.seed_call_ids = ids.data_ptr(), ids.data_ptr()
    so, rng, fan1 = out.struct(), cabi.TgRng(1, 2), (C.c_int64 * 1)(3)
    assert cabi.lib.tg_ns_homo_batched_ws(C.byref(g), cabi.ptr(seeds), C.c_int64(2), C.c_int64(8), fan1, C.c_int32(1),
                                          C.byref(cfg), C.byref(rng), C.byref(so), cabi.ptr(ws), C.c_int64(big), C.c_int32(0),
                                          cabi.stream_ptr(dev)) == 1 and "seed_ids" in err()
    assert cabi.lib.tg_ns_homo_batched_workspace_bytes(C.byref(g), C.c_int64(2), C.c_int64(8), (C.c_int64 * 1)(65),
                                                       C.c_int32(1), C.byref(cfg), C.byref(need)) == 1
    with pytest.raises(cabi.TchGeoError, match="tchgeo error 1"):          # the plain flat hop keeps rejecting the id
        cabi.ns_hop(g, seeds[0], 3, 1, sampler=cabi.SAMPLER_RECENT)
    with pytest.raises(cabi.TchGeoError, match="tchgeo error 1"):
        cabi.ns_hop_scan(g, seeds[0], seeds[0], 3, 1, 1, (0, 5), sampler=cabi.SAMPLER_RECENT)
    with pytest.raises(cabi.TchGeoError, match="tchgeo error 1"):
        cabi.ns_hop_recent(g, seeds[0], 65)
    with pytest.raises(cabi.TchGeoError, match="tchgeo error 1"):
        cabi.ns_hop_recent(g_bare, seeds[0], 3)
    torch.cuda.synchronize()
    for t in slabs:
        assert bool((t == POISON).all())                  # nothing was launched


# ---------------------------------------------------------------- operator surface
@pytest.mark.parametrize("where", ["cpu", "cuda"])
@pytest.mark.parametrize("filtered", [False, True])
def test_operator_surface_equals_the_restatement(graph, times, where, filtered):
    import tch_geometric as tg
    ptrs, idx, n, crafted, hub = graph
    ts = times["wide"]
    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a))) if where == "cpu" else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
    P, I, T = put(ptrs), put(idx), put(ts)
    seeds = np.concatenate([[hub, hub], crafted, np.arange(20)]).astype(np.int64)
    st = _states(ts, len(seeds), 8)
    window = _windows(ts, 1)
    flt = (tg.TemporalEdgeFilter(window, T, False, tg.TEMPORAL_SAMPLE_RELATIVE), put(st)) if filtered else None
    s, r, c, e, lo = tg.neighbor_sampling_homogenous(P, I, put(seeds), [7, 3], tg.RecentEdgeSampler(T), flt)
    want = recent_ns_homo(ptrs, idx, ts, seeds, [7, 3], st if filtered else None, 1 if filtered else -1, False, window)
    assert s.device.type == where and lo == want[4]
    for got, w in zip((s, r, c, e), want[:4]):
        assert torch.equal(got.cpu(), torch.from_numpy(w))


def test_operator_surface_refusals(graph, times):
    import tch_geometric as tg
    ptrs, idx = graph[0], graph[1]
    P, I = torch.from_numpy(ptrs).cuda(), torch.from_numpy(idx).cuda()
    T = torch.from_numpy(times["ties"]).cuda()
    seeds = torch.tensor([1, 2, 3]).cuda()
    smp = tg.RecentEdgeSampler(T)
    other = (tg.TemporalEdgeFilter((0, 3), T.clone(), False, tg.TEMPORAL_SAMPLE_RELATIVE), torch.zeros(3, dtype=torch.int64).cuda())
    with pytest.raises(ValueError, match="timestamps"):
        tg.neighbor_sampling_homogenous(P, I, seeds, [3], smp, other)
    with pytest.raises(ValueError, match="64"):
        tg.neighbor_sampling_homogenous(P, I, seeds, [65], smp, None)
    with pytest.raises(ValueError, match="RecentEdgeSampler: homogeneous sampling only"):
        tg.neighbor_sampling_heterogenous(["a"], [("a", "r", "a")], {}, {}, {}, {}, 1, smp, None)


@pytest.mark.parametrize("filtered", [False, True])
def test_operator_surface_with_more_inputs_than_one_launch_takes(graph, times, filtered):
    """above 2048 inputs the call runs hop by hop (tg_ns_hop_recent per hop) instead of as one batch: the same result"""
    import tch_geometric as tg
    ptrs, idx, n, crafted, hub = graph
    ts = times["ties"]
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    P, I, T = put(ptrs), put(idx), put(ts)
    seeds = np.concatenate([[hub, hub], crafted, np.random.default_rng(31).integers(0, n, 3000)]).astype(np.int64)
    st = _states(ts, len(seeds), 9)
    window = _windows(ts, 2)
    flt = (tg.TemporalEdgeFilter(window, T, True, tg.TEMPORAL_SAMPLE_DYNAMIC), put(st)) if filtered else None
    s, r, c, e, lo = tg.neighbor_sampling_homogenous(P, I, put(seeds), [3, 2], tg.RecentEdgeSampler(T), flt)
    want = recent_ns_homo(ptrs, idx, ts, seeds, [3, 2], st if filtered else None, 2 if filtered else -1, filtered, window)
    assert lo == want[4]
    for got, w in zip((s, r, c, e), want[:4]):
        assert torch.equal(got.cpu(), torch.from_numpy(w))
