"""TG_SAMPLER_LABOR / TG_SAMPLER_LABOR_SHARED on the device: the flat hop (tg_ns_hop_labor, short and long columns), the
batched launch (tg_ns_homo_batched_ws through the flat driver), the operator surface and the law of one vertex.  Every output
is compared for exact equality with the NumPy restatement in helpers_labor.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import exact_laws
from helpers_labor import SAMPLER_LABOR, SAMPLER_LABOR_SHARED, labor_hop, labor_ns_homo, labor_test_graph
from helpers_recent import recent_test_times
from test_gpu_ns_recent import BATCHED

pytestmark = pytest.mark.gpu
POISON = -777
SEED = 0x1AB02


@pytest.fixture(scope="module")
def cabi():
    from tch_geometric import _cabi
    return _cabi


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def graph(cabi):
    return labor_test_graph(cabi.LABOR_LONG_COLUMN)


@pytest.fixture(scope="module")
def times(graph):
    return {k: recent_test_times(graph["ptrs"], graph["hub"], k) for k in ("ties", "wide")}


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


def _view(cabi, dev, graph, ts=None, narrow=True):
    P, I = _t(dev, graph["ptrs"]), _t(dev, graph["idx"])
    kw = dict(indices32=I.to(torch.int32), ptrs32=P.to(torch.int32)) if narrow else {}
    return cabi.graph_view(P, I, timestamps=_t(dev, ts) if ts is not None else None, **kw)


def _windows(ts, mode):
    lo, hi = int(ts.min()), int(ts.max())
    span = hi - lo
    return (lo + span // 4, lo + span // 2) if mode == 0 else (0, max(span // 4, 1))


def _states(ts, shape, seed):
    lo, hi = int(ts.min()), int(ts.max())
    span = hi - lo
    return np.random.default_rng(seed).integers(lo - span // 4, hi + span // 4 + 1, shape).astype(np.int64)


def _special(graph):
    return np.concatenate([graph["long"], [graph["same"]], graph["shared"], [graph["hub"]], graph["crafted"]]).astype(np.int64)


def _frontier(graph, m, seed, repeats=2):
    """m frontier vertices: every 13th an empty slot; the long columns, the one-neighbour column, the two that share
    neighbours, the hub and the crafted columns among the others, `repeats` times over"""
    v = np.random.default_rng(seed).integers(0, graph["base"], m).astype(np.int64)
    v[::13] = -1
    free = [i for i in range(m) if i % 13]
    special = np.tile(_special(graph), repeats)[:len(free)]
    v[free[:len(special)]] = special
    return v


def _check_hop(cabi, dev, graph, g, vertices, k, call, layer=0, call_ids=None, ts=None, states=None, mode=-1, forward=False,
               window=(0, 0), sampler=SAMPLER_LABOR):
    filtered = mode != -1
    want = labor_hop(graph["ptrs"], graph["idx"], ts, vertices, states if filtered else None, k, SEED,
                     call_ids if call_ids is not None else call, layer, mode, forward, window)
    got = cabi.ns_hop_labor(g, _t(dev, vertices), k, SEED, call, layer=layer,
                            call_ids=_t(dev, call_ids) if call_ids is not None else None,
                            states=_t(dev, states) if filtered else None, filter_mode=mode, window=window, forward=forward,
                            sampler=sampler)
    torch.cuda.synchronize()
    cnt, off, nbr, ep, par, sto = want
    tot = int(off[-1])
    assert torch.equal(got[0].cpu(), torch.from_numpy(cnt)), "cnt"
    assert torch.equal(got[1].cpu(), torch.from_numpy(off)), "offsets"
    for name, a, b in (("edge_ptrs", got[3], ep), ("neighbors", got[2], nbr), ("parents", got[4], par)):
        assert torch.equal(a[:tot].cpu(), torch.from_numpy(b)), name
    if filtered:
        assert torch.equal(got[5][:tot].cpu(), torch.from_numpy(sto)), "states_out"
    else:
        assert got[5] is None
    return got, cnt


@pytest.mark.parametrize("k", [1, 7, 33, 64])
def test_flat_hop_equals_the_restatement(cabi, dev, graph, k):
    g = _view(cabi, dev, graph)
    vertices = _frontier(graph, 300, 1)                   # the long columns twice each; a last partial workgroup
    assert (vertices[::13] == -1).all() and (np.bincount(vertices[vertices >= 0])[graph["long"]] == 2).all()
    _, cnt = _check_hop(cabi, dev, graph, g, vertices, k, 5, layer=1)
    deg = np.diff(graph["ptrs"])[np.maximum(vertices, 0)]
    assert np.array_equal(cnt, np.where(vertices >= 0, np.minimum(deg, k), 0))
    one = np.array([graph["long"][-1]], dtype=np.int64)   # a frontier of one long column, and of one empty slot
    _check_hop(cabi, dev, graph, g, one, k, 6)
    _check_hop(cabi, dev, graph, g, np.array([-1], dtype=np.int64), k, 6)


def test_per_vertex_call_ids_against_a_scalar_and_other_addresses(cabi, dev, graph):
    g = _view(cabi, dev, graph)
    vertices = _frontier(graph, 200, 2)                   # the long columns twice, under different call ids
    calls = np.random.default_rng(3).integers(0, 4, len(vertices)).astype(np.int64) + (1 << 40)
    got, _ = _check_hop(cabi, dev, graph, g, vertices, 7, 0, layer=2, call_ids=calls)
    ep = {}
    for c in range(4):                                    # vertex by vertex the scalar launch of its call id
        only, _ = _check_hop(cabi, dev, graph, g, vertices, 7, (1 << 40) + c, layer=2)
        ep[c] = only
    off = got[1].cpu().numpy()
    for i in range(len(vertices)):
        o = ep[int(calls[i] - (1 << 40))]
        oo = o[1].cpu().numpy()
        assert torch.equal(got[3][off[i]:off[i + 1]], o[3][oo[i]:oo[i + 1]]), i
    # seed, call id and layer are all in the address; the sampler id is not (the layer is passed as given)
    tot = int(ep[0][1][-1])                               # without a filter the counts are the same under every address
    base = ep[0][3][:tot]
    for kw in (dict(seed=SEED + 1), dict(call_id=(1 << 40) + 1), dict(layer=3)):
        a = dict(seed=SEED, call_id=1 << 40, layer=2)
        a.update(kw)
        other = cabi.ns_hop_labor(g, _t(dev, vertices), 7, a["seed"], a["call_id"], layer=a["layer"])
        assert int(other[1][-1]) == tot and not torch.equal(other[3][:tot], base), kw
    same = cabi.ns_hop_labor(g, _t(dev, vertices), 7, SEED, 1 << 40, layer=2, sampler=SAMPLER_LABOR_SHARED)
    assert torch.equal(same[3][:tot], base)


def test_u32_shadows_or_not_and_null_filter_give_equal_words(cabi, dev, graph, times):
    vertices = _frontier(graph, 120, 4)
    wide, narrow = _view(cabi, dev, graph, narrow=False), _view(cabi, dev, graph)
    # both are held to the restatement's words, hence to each other's
    _check_hop(cabi, dev, graph, wide, vertices, 33, 9)
    _check_hop(cabi, dev, graph, narrow, vertices, 33, 9)
    ts = times["wide"]
    st = _states(ts, len(vertices), 6)
    window = _windows(ts, 1)
    _check_hop(cabi, dev, graph, _view(cabi, dev, graph, ts, narrow=False), vertices, 7, 9, ts=ts, states=st, mode=1,
               window=window)
    _check_hop(cabi, dev, graph, _view(cabi, dev, graph, ts), vertices, 7, 9, ts=ts, states=st, mode=1, window=window)
    # filter = NULL, raw call with poisoned outputs: nothing is written past the total
    want = labor_hop(graph["ptrs"], graph["idx"], None, vertices, None, 5, SEED, 11, 0)
    m, o = len(vertices), dict(dtype=torch.int64, device=dev)
    cnt, off = torch.empty(m, **o), torch.empty(m + 1, **o)
    nbr, ep, par = (torch.full((m * 5,), POISON, **o) for _ in range(3))
    hin, hout = cabi.TgHopIn(), cabi.TgHopOut()
    V = _t(dev, vertices)
    hin.vertices, hin.m, hin.fanout, hin.sampler = V.data_ptr(), m, 5, cabi.SAMPLER_LABOR
    hout.cnt, hout.offsets = cnt.data_ptr(), off.data_ptr()
    hout.neighbors, hout.edge_ptrs, hout.parents = nbr.data_ptr(), ep.data_ptr(), par.data_ptr()
    ws = torch.empty(m + 64, **o)
    rng = cabi.TgRng(SEED, 11)
    cabi.check(cabi.lib.tg_ns_hop_labor(C.byref(narrow), C.byref(hin), None, C.byref(rng), C.c_int32(0), C.byref(hout), None,
                                        cabi.ptr(ws), C.c_int64(ws.numel() * 8), cabi.stream_ptr(dev)))
    torch.cuda.synchronize()
    tot = int(want[1][-1])
    assert torch.equal(off.cpu(), torch.from_numpy(want[1])) and torch.equal(ep[:tot].cpu(), torch.from_numpy(want[3]))
    assert torch.equal(nbr[:tot].cpu(), torch.from_numpy(want[2])) and torch.equal(par[:tot].cpu(), torch.from_numpy(want[4]))
    assert bool((ep[tot:] == POISON).all()) and bool((par[tot:] == POISON).all())


@pytest.mark.parametrize("kind", ["ties", "wide"])
@pytest.mark.parametrize("mode,forward", [(0, False), (1, True), (1, False), (2, True), (2, False)])
def test_flat_hop_under_every_filter(cabi, dev, graph, times, kind, mode, forward):
    ts = times[kind]
    g = _view(cabi, dev, graph, ts)
    window = _windows(ts, mode)
    vertices = _frontier(graph, 150, 7)
    states = _states(ts, len(vertices), 8)
    states[np.isin(vertices, graph["long"])] = int(np.median(ts))   # the long columns' windows admit many edges
    for k in (7, 64):
        _, cnt = _check_hop(cabi, dev, graph, g, vertices, k, 3, layer=1, ts=ts, states=states, mode=mode, forward=forward,
                            window=window)
        live = vertices >= 0
        deg = np.diff(graph["ptrs"])[np.maximum(vertices, 0)]
        assert (cnt[live] == k).any() and ((cnt < np.minimum(deg, k)) & live).any()   # the filter bites somewhere


def test_results_do_not_depend_on_the_long_column_threshold(cabi, dev, graph, times):
    ts = times["ties"]
    g = _view(cabi, dev, graph, ts)
    vertices = _frontier(graph, 150, 9)
    states = _states(ts, len(vertices), 10)
    window = _windows(ts, 1)
    try:
        for threshold in (1, 64, 100, 2048, 1 << 30):     # 1: every non-empty column past one edge takes the long kernel
            assert cabi.ns_hop_labor_long_column(threshold) > 0
            _check_hop(cabi, dev, graph, g, vertices, 33, 4, layer=1)
            _check_hop(cabi, dev, graph, g, vertices, 7, 4, ts=ts, states=states, mode=1, window=window)
    finally:
        cabi.ns_hop_labor_long_column(0)


def test_empty_launches_are_ok(cabi, dev, graph):
    g = _view(cabi, dev, graph)
    got = cabi.ns_hop_labor(g, torch.empty(0, dtype=torch.int64, device=dev), 5, 1, 2)
    torch.cuda.synchronize()
    assert got[1].tolist() == [0]
    out = cabi.NsBatchedOut(1, 4, [3], dev)
    out.counts.fill_(POISON)
    ws = torch.empty(1 << 16, dtype=torch.int64, device=dev)
    seeds = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    cfg, rng, so = cabi.TgNsConfig(), cabi.TgRng(1, 2), out.struct()
    cfg.sampler, cfg.filter_mode = cabi.SAMPLER_LABOR, -1
    assert cabi.lib.tg_ns_homo_batched_ws(C.byref(g), cabi.ptr(seeds), C.c_int64(0), C.c_int64(4), (C.c_int64 * 1)(3),
                                          C.c_int32(1), C.byref(cfg), C.byref(rng), C.byref(so), cabi.ptr(ws),
                                          C.c_int64(ws.numel() * 8), C.c_int32(0), cabi.stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    assert bool((out.counts == POISON).all())             # n_batches = 0: TG_OK and nothing launched


# ---------------------------------------------------------------- batched
def _seeds(graph, n_batches, n_seeds, seed):
    s = np.random.default_rng(seed).integers(0, graph["base"], (n_batches, n_seeds)).astype(np.int64)
    special = _special(graph)
    s[0, 0] = s[0, 1] = graph["hub"]                      # a duplicate seed inside a batch
    n = max(0, min(n_seeds - 2, len(special)))
    s[0, 2:2 + n] = special[:n]
    if n_batches > 1:
        s[1] = s[0]                                       # a duplicate batch: another call id, other variates
    return s


def _launch(cabi, dev, g, seeds, fanout, sampler, states, mode, window, rng=(SEED, 7)):
    B, S = seeds.shape
    out = cabi.NsBatchedOut(B, S, fanout, dev, with_states=True)
    for t in (out.samples, out.rows, out.cols, out.edge_index, out.states):
        t.fill_(POISON)
    ws = cabi.ns_homo_batched_workspace(g, B, S, fanout, dev, sampler=sampler, filter_mode=mode)
    assert ws is not None
    cabi.ns_homo_batched(g, _t(dev, seeds), fanout, rng[0], rng[1], out, sampler=sampler, filter_mode=mode, forward=False,
                         window=window, seeds_state=_t(dev, states) if mode != -1 else None, ws=ws)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n_batches,n_seeds,fanout", BATCHED)
@pytest.mark.parametrize("sampler", [SAMPLER_LABOR, SAMPLER_LABOR_SHARED])
@pytest.mark.parametrize("mode", [-1, 1])
def test_batched_equals_the_restatement(cabi, dev, graph, times, n_batches, n_seeds, fanout, sampler, mode):
    ts = times["wide"]
    g = _view(cabi, dev, graph, ts if mode != -1 else None)
    window = _windows(ts, mode)
    seeds = _seeds(graph, n_batches, n_seeds, 11)
    states = _states(ts, seeds.shape, 12)
    out = _launch(cabi, dev, g, seeds, fanout, sampler, states, mode, window)
    S, R, Cc, E, ST = (t.cpu().numpy() for t in (out.samples, out.rows, out.cols, out.edge_index, out.states))
    LO, CN = out.layer_offsets.cpu().numpy(), out.counts.cpu().numpy()
    H = len(fanout)
    for b in range(n_batches):
        s, r, c, e, lo, counts, st = labor_ns_homo(graph["ptrs"], graph["idx"], ts, seeds[b], fanout, SEED, 7 + b, sampler,
                                                   states[b] if mode != -1 else None, mode, False, window)
        ns, ne = counts
        assert tuple(CN[b]) == (ns, ne), b
        assert [tuple(x) for x in LO[b, :H]] == lo, b
        for name, slab, want, n in (("edge_index", E, e, ne), ("samples", S, s, ns), ("rows", R, r, ne), ("cols", Cc, c, ne)):
            assert np.array_equal(slab[b, :n], want), (b, name)
            assert (slab[b, n:] == POISON).all(), (b, name, "written past its recorded length")
        if mode != -1:
            assert np.array_equal(ST[b, :ns], st), (b, "states")
            assert (ST[b, ns:] == POISON).all(), b
        else:
            assert (ST[b] == POISON).all(), b
    # duplicate seeds of a batch share the variates: identical subtrees at hop 0
    c0 = Cc[0, :CN[0, 1]]
    first = S[0, n_seeds:][:len(c0)]
    if mode == -1:
        assert np.array_equal(first[c0 == 0], first[c0 == 1])
    if n_batches > 1 and mode == -1:                      # the duplicate batch draws under the next call id
        assert not np.array_equal(E[0], E[1])


def test_shared_and_plain_agree_at_hop_0_and_differ_from_hop_1_on(cabi, dev, graph):
    g = _view(cabi, dev, graph)
    seeds = _seeds(graph, 3, 40, 13)
    a = _launch(cabi, dev, g, seeds, [4, 3, 2], SAMPLER_LABOR, None, -1, (0, 0))
    b = _launch(cabi, dev, g, seeds, [4, 3, 2], SAMPLER_LABOR_SHARED, None, -1, (0, 0))
    for bt in range(3):
        lo = a.layer_offsets[bt].cpu().numpy()
        n0 = int(lo[1][1])                                # edges of hop 0
        assert torch.equal(a.layer_offsets[bt][:2], b.layer_offsets[bt][:2])
        assert torch.equal(a.edge_index[bt, :n0], b.edge_index[bt, :n0])
        n1 = int(lo[2][1])
        assert not torch.equal(a.edge_index[bt, n0:n1], b.edge_index[bt, n0:n1])


# ---------------------------------------------------------------- the law
def _law_graph(d=20):
    """vertex 0: a column of d distinct neighbours (10 .. 10 + d); vertex 1: one edge to vertex 0; the rest: none"""
    n = 10 + d
    deg = np.zeros(n, dtype=np.int64)
    deg[0], deg[1] = d, 1
    ptrs = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    idx = np.concatenate([np.arange(10, 10 + d), [0]]).astype(np.int64)
    return dict(ptrs=ptrs, idx=idx)


@pytest.mark.parametrize("seed,chain", [(1, False), (0xFEED5EED, False), (1, True)])
def test_the_ordered_pair_of_one_vertex_is_uniform(cabi, dev, seed, chain):
    """2^16 batches of one seed in one launch, k = 5, 20 distinct neighbours: (first, second) in rank order is uniform over
    the 380 ordered pairs.  chain: the column is reached at hop 1 of a two-hop launch (layer 1 of the address)."""
    d, N = 20, 1 << 16
    lg = _law_graph(d)
    g = _view(cabi, dev, lg)
    fanout = [5, 5] if chain else [5]
    seeds = np.full((N, 1), 1 if chain else 0, dtype=np.int64)
    out = cabi.NsBatchedOut(N, 1, fanout, dev)
    ws = cabi.ns_homo_batched_workspace(g, N, 1, fanout, dev, sampler=cabi.SAMPLER_LABOR)
    cabi.ns_homo_batched(g, _t(dev, seeds), fanout, seed, 100, out, sampler=cabi.SAMPLER_LABOR, ws=ws)
    torch.cuda.synchronize()
    S = out.samples.cpu().numpy()
    at = 2 if chain else 1                                # samples: the seed, (vertex 0,) then the five in rank order
    assert (out.counts[:, 0].cpu().numpy() == at + 5).all()
    if chain:
        assert (S[:, 1] == 0).all()
    first, second = S[:, at] - 10, S[:, at + 1] - 10
    counts = np.zeros((d, d), dtype=np.int64)
    np.add.at(counts, (first, second), 1)
    law = np.full((d, d), 1.0 / (d * (d - 1)))
    np.fill_diagonal(law, 0.0)
    exact_laws.chi2_gof(counts.reshape(-1), law.reshape(-1), "labor ordered pairs")
    for b in (0, 1, N - 1):                               # and the address: batch b draws under call id 100 + b
        want = labor_ns_homo(lg["ptrs"], lg["idx"], None, seeds[b], fanout, seed, 100 + b)[0]
        assert np.array_equal(S[b, :len(want)], want)


# ---------------------------------------------------------------- operator surface
@pytest.mark.parametrize("where,dependency,many", [("cpu", False, False), ("cuda", True, False), ("cuda", False, True),
                                                   ("cpu", True, True)])
def test_operator_surface_equals_the_restatement(graph, times, where, dependency, many):
    """up to 2048 inputs one launch of the batched driver, above hop by hop (tg_ns_hop_labor per hop): the same law"""
    import tch_geometric as tg
    ptrs, idx = graph["ptrs"], graph["idx"]
    ts = times["wide"]
    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a))) if where == "cpu" else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
    P, I, T = put(ptrs), put(idx), put(ts)
    extra = np.random.default_rng(31).integers(0, graph["base"], 2100 if many else 20)
    seeds = np.concatenate([_special(graph), extra]).astype(np.int64)
    st = _states(ts, len(seeds), 8)
    window = _windows(ts, 1)
    sampler = SAMPLER_LABOR_SHARED if dependency else SAMPLER_LABOR
    fan = [3, 2] if many else [7, 3]
    for filtered in (False, True):
        flt = (tg.TemporalEdgeFilter(window, T, False, tg.TEMPORAL_SAMPLE_RELATIVE), put(st)) if filtered else None
        tg.seed(4242)
        seed, call = tg.rng_state()
        s, r, c, e, lo = tg.neighbor_sampling_homogenous(P, I, put(seeds), fan, tg.LaborEdgeSampler(dependency), flt)
        assert tg.rng_state() == (seed, call + 1)
        want = labor_ns_homo(ptrs, idx, ts, seeds, fan, seed, call, sampler, st if filtered else None,
                             1 if filtered else -1, False, window)
        assert s.device.type == where and lo == want[4]
        for got, w in zip((e, s, r, c), (want[3], want[0], want[1], want[2])):
            assert torch.equal(got.cpu(), torch.from_numpy(w))


def test_operator_surface_refusals(graph):
    import tch_geometric as tg
    P, I = torch.from_numpy(graph["ptrs"]).cuda(), torch.from_numpy(graph["idx"]).cuda()
    seeds = torch.tensor([1, 2, 3]).cuda()
    with pytest.raises(ValueError, match="64"):
        tg.neighbor_sampling_homogenous(P, I, seeds, [65], tg.LaborEdgeSampler(), None)
    with pytest.raises(ValueError, match="LaborEdgeSampler: homogeneous sampling only"):
        tg.neighbor_sampling_heterogenous(["a"], [("a", "r", "a")], {}, {}, {}, {}, 1, tg.LaborEdgeSampler(), None)
