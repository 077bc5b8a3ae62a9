"""hgt_sampling and budget_sampling on the device against the EXACT output laws of the reference's loops
(tests/exact_laws.py: hgt_budget_weights, hgt_layer_law, the edge-phase and budget laws, all derived from
hgt_sampling.rs and budget_sampling.rs), past 64 candidates: the sizes at which hgt.hip's blocked f64 running sum crosses a
64-entry chunk, a wavefront's four chunks, a workgroup's sweep and a tile of chunk totals, at which its slot table leaves
the LDS, at which a live entry's rank differs from its entry index, and at which budget.hip's ticket chain runs over lists of
up to 800 candidates.  Word-for-word parity with the oracle cannot see an error the kernels and the oracle's philox-mode
share; these one-sample tests can.

One outcome is one call (HGT sample_from), one hub (HGT edge phase) or one frontier node (budget); call id = outcome index,
fixed seeds, counts reduced on the device: a failure reproduces exactly.  Every launched outcome is counted and a call
whose panic word is set fails the test.  The outcome counts come from exact_laws (hgt_outcomes, EDGE_OUTCOMES,
BUDGET_CASES); tests/test_exact_laws_cpu.py asserts their power against the named wrong laws."""
import numpy as np
import pytest
import torch

import exact_laws as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LAUNCH_BYTES = 6 << 30                                          # slabs and workspace of one batched launch, at most


@pytest.fixture(scope="module")
def cabi():
    from tch_geometric import _cabi
    return _cabi


@pytest.fixture(scope="module")
def tg():
    import tch_geometric
    return tch_geometric


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pow2_floor(x):
    return 1 << (int(x).bit_length() - 1)


def _rels(g, row_ts=None):
    """(src type index, dst type index, ptrs, indices, row timestamps) per relation, on the device"""
    tix = {t: i for i, t in enumerate(g["node_types"])}
    out = []
    for s, r, d in g["edge_types"]:
        key = "%s__%s__%s" % (s, r, d)
        out.append((tix[s], tix[d], _t(g["ptrs"][key]), _t(g["indices"][key]), _t(row_ts[key]) if row_ts else None))
    return out


def _dev_dicts(g):
    return {k: _t(v) for k, v in g["ptrs"].items()}, {k: _t(v) for k, v in g["indices"].items()}


# ---------------------------------------------------------------- HGT sample_from
def _hgt_batched_ranks(cabi, g, quotas, pre, N, seed):
    """N calls of tg_hgt_sample_batched (several launches with advancing call ids when one launch's slabs and workspace
    would pass LAUNCH_BYTES) -> [N, k] ranks of the last layer's samples of type b, slot order.  pre: the samples of the
    layers before it (their ids must be g["keys0"] in order, call after call)."""
    rels, hops, k = _rels(g), len(quotas), quotas[-1]
    m = len(g["inputs"]["a"])
    ns = [[0] * hops, list(quotas)]                             # type a has no budget: its quota is never read
    per_call = cabi.HgtBatched.bytes_of(cabi.hgt_problem(2, rels, [m, -1], ns, hops), 1)
    calls = min(N, 32768, _pow2_floor(max(LAUNCH_BYTES // per_call, 1)))
    hb = cabi.HgtBatched(2, rels, [_t(g["inputs"]["a"]).expand(calls, m).contiguous(), None], ns, hops, calls, DEV)
    rank_of = _t(g["rank_of"])
    keys0 = _t(g["keys0"]) if pre else None
    E = torch.empty((N, k), dtype=torch.int64, device=DEV)
    for c0 in range(0, N, calls):
        hb.run(seed, c0)
        assert int(hb.counts[:, -1].sum()) == 0, "a call set its panic word"
        assert bool((hb.counts[:, 0] == m).all()) and bool((hb.counts[:, 1] == pre + k).all())
        if pre:
            assert bool((hb.samples[1][:, :pre] == keys0).all()), "layer 0 takes the whole budget: slot s holds entry s"
        E[c0:c0 + calls] = rank_of[hb.samples[1][:, pre:pre + k]]
    return E


@pytest.mark.parametrize("k,n", L.HGT_CASES + L.HGT_LARGE)
def test_hgt_sample_from_law(cabi, k, n):
    """(k, n): each the smallest size that crosses one boundary of hgt_reservoir_body -- the first chunk (2, 65), an exact
    chunk with k no power of two (3, 64), a wavefront's four chunks plus one with k below, at and above 64 (63..65, 257),
    one sweep of the workgroup plus one (191, 4097), a large k still in the LDS slot table (1000, 4097), the second tile of
    chunk totals (16, 65537) and the global slot table (8193, 12288: five marginals and one pair only)."""
    g = L.hgt_wide_graph(n, 100 + n)
    N = L.hgt_outcomes(k, n)
    E = _hgt_batched_ranks(cabi, g, [k], 0, N, 0xA10 + k)
    pairs = ((0, 8192),) if k == 8193 else None
    assert L.check_reservoir(E, L.hgt_layer_law(g["w"], k), "hgt sample_from k=%d n=%d" % (k, n), zero_pos=None,
                             slots=L.hgt_slots(k), positions=L.hgt_positions(k, n), pairs=pairs) > 0


def test_hgt_dead_prefix_law(cabi):
    """layer 0 takes all n0 = 100 entries (quota 128, no draw), layer 1 samples k1 = 7 of the n1 = 300 fresh entries behind
    them: a live entry's rank differs from its entry index across a chunk boundary (hgt_live_list_body)"""
    n0, n1, k = L.HGT_DEAD
    g = L.hgt_dead_prefix_graph(n0, n1, 5)
    E = _hgt_batched_ranks(cabi, g, [128, k], n0, L.hgt_outcomes(k, n1), 0xA20)
    assert L.check_reservoir(E, L.hgt_layer_law(g["w"], k), "hgt dead prefix", zero_pos=None, slots=L.hgt_slots(k),
                             positions=L.hgt_positions(k, n1)) > 0


def test_hgt_sample_from_law_single_calls(tg):
    """(2, 65) through tg.hgt_sampling, HGT_SURFACE_CALLS = 4096 single calls (the unbatched launch).  Power at 4096
    outcomes: >= 0.999 against weights score instead of score^2 and against the previous candidate's running sum
    (test_power_hgt_surface_loop)."""
    k, n = 2, 65
    g = L.hgt_wide_graph(n, 100 + n)
    P, I = _dev_dicts(g)
    inputs = {"a": _t(g["inputs"]["a"])}
    tg.seed(0xA30)
    got = []
    for _ in range(L.HGT_SURFACE_CALLS):                        # every call draws with the next call id
        got.append(tg.hgt_sampling(g["node_types"], g["edge_types"], P, I, None, inputs, None, {"a": [k], "b": [k]}, 1)[0]["b"])
    E = _t(g["rank_of"])[torch.stack(got).to(DEV)]
    assert E.shape == (L.HGT_SURFACE_CALLS, k)
    assert L.check_reservoir(E, L.hgt_layer_law(g["w"], k), "hgt sample_from single calls", zero_pos=None,
                             slots=L.hgt_slots(k), positions=L.hgt_positions(k, n)) > 0


# ---------------------------------------------------------------- HGT edge phase
@pytest.mark.parametrize("deg", [d for d in L.EDGE_DEGS if d + 64 <= 16384])
def test_hgt_edge_phase_law(cabi, deg):
    """a ticket reservoir takes 50 of a column of deg > 50 entries (hgt_sampling.rs:258-259): num_hops = 0, the pool and H
    hubs as inputs, H outcomes per call, the launches' outcomes counted launch by launch.  EDGE_OUTCOMES[deg] outcomes reach
    power 0.999 against the law without the quirk (test_power_budget_and_edge_phase_without_the_quirk)."""
    N = L.EDGE_OUTCOMES[deg]
    H = min(N, _pow2_floor(16384 - deg))                        # the batched form takes 16 384 nodes of a type
    nt, et, P, I, inputs, hub_ptrs = L.hgt_edge_graph(deg, H)
    g = dict(node_types=nt, edge_types=et, ptrs=P, indices=I)
    rels, m = _rels(g), deg + H
    per_call = cabi.HgtBatched.bytes_of(cabi.hgt_problem(1, rels, [m], [[]], 0), 1)
    calls = min(N // H, _pow2_floor(max(LAUNCH_BYTES // per_call, 1)))
    hb = cabi.HgtBatched(1, rels, [_t(inputs).expand(calls, m).contiguous()], [[]], 0, calls, DEV)
    base = _t(hub_ptrs)[None, :, None]
    cols = (deg + torch.arange(H, device=DEV)).repeat_interleave(50)
    tally = L.ReservoirTally(N, 50, L.uniform_law(deg, 50), "hgt edges deg=%d" % deg)
    for c0 in range(0, N // H, calls):
        hb.run(0xB10 + deg, c0)
        assert int(hb.counts[:, -1].sum()) == 0, "a call set its panic word"
        assert bool((hb.counts[:, 0] == m).all()) and bool((hb.counts[:, 1] == 50 * H).all())
        assert bool((hb.cols[0][:, :50 * H] == cols).all())     # 50 edges per hub, hub after hub
        E = hb.edge_index[0][:, :50 * H].reshape(calls, H, 50) - base
        assert bool((hb.rows[0][:, :50 * H].reshape(calls, H, 50) == E).all())   # the pool node's local id = its position
        tally.add(E.reshape(calls * H, 50))
    assert tally.finish() > 0


def test_hgt_edge_phase_law_long_column(tg):
    """deg = 70 000: the pool is past the batched form's 16 384 nodes, so single calls of tg.hgt_sampling with 4096 hubs.
    The graph is hgt_edge_graph's, laid out on the device (its 2.3 GB of row indices need not cross the host)."""
    deg, H = 70000, 4096
    N = L.EDGE_OUTCOMES[deg]
    ptrs = torch.zeros(deg + H + 1, dtype=torch.int64, device=DEV)
    ptrs[deg + 1:] = deg * torch.arange(1, H + 1, device=DEV)
    idx = torch.arange(deg, device=DEV).repeat(H)
    inputs = {"a": torch.arange(deg + H, device=DEV)}
    base = ptrs[deg:deg + H, None]
    cols = (deg + torch.arange(H, device=DEV)).repeat_interleave(50)
    tally = L.ReservoirTally(N, 50, L.uniform_law(deg, 50), "hgt edges deg=70000")
    tg.seed(0xB20)
    for _ in range(N // H):
        o = tg.hgt_sampling(["a"], [("a", "r", "a")], {"a__r__a": ptrs}, {"a__r__a": idx}, None, inputs, None, {"a": []}, 0)
        assert o[0]["a"].numel() == deg + H
        assert torch.equal(o[3]["a__r__a"].to(DEV), cols)       # 50 edges per hub, hub after hub
        E = o[4]["a__r__a"].to(DEV).reshape(H, 50) - base
        assert torch.equal(o[2]["a__r__a"].to(DEV).reshape(H, 50), E)            # the pool node's local id = its position
        tally.add(E)
    assert tally.finish() > 0


# ---------------------------------------------------------------- budget
def _budget_chunks(route, tg, cabi, g, k, N, seed, window=None):
    """N outcomes (frontier nodes, all the hub) of one budget layer, in launches of at most 4 GiB of output slabs (every
    relation's three edge slabs hold the worst case) with advancing call ids -> yields [chunk, k]: the node id held by
    slot s of node j, which is its rank in the hub's candidate list"""
    R = len(g["edge_types"])
    chunk = min(N, _pow2_floor((1 << 29) // ((3 * R + 2) * k)))
    its = torch.full((chunk,), g["hub_ts"], dtype=torch.int64, device=DEV) if window is not None else None
    hub = torch.zeros(chunk, dtype=torch.int64, device=DEV)
    rels = _rels(g, g["row_ts"])
    if route == "surface":
        P, I = _dev_dicts(g)
        TS = {key: _t(v) for key, v in g["row_ts"].items()} if g["row_ts"] else None
        tg.seed(seed)                                           # every call draws with the next call id
    elif route == "batched":                                    # 4 calls per launch, their outcomes pooled
        nc, per = 4, chunk // 4
        hb = cabi.BudgetBatched(2, rels, [hub.reshape(nc, per), None], [[k], [k]], 1, nc, DEV,
                                input_ts=[its.reshape(nc, per), None] if its is not None else None, window=window)
    for c in range(N // chunk):
        if route == "surface":
            o = tg.budget_sampling(g["node_types"], g["edge_types"], P, I, TS, {"a": hub},
                                   {"a": its} if its is not None else None, {"a": [k], "b": [k]}, 1, window, False, False)
            S = o[0]["b"].to(DEV)
            assert S.numel() == chunk * k and o[0]["a"].numel() == chunk
            yield S.reshape(chunk, k)
        elif route == "batched":
            hb.run(seed, nc * c)
            assert bool((hb.counts[:, 0] == per).all()) and bool((hb.counts[:, 1] == per * k).all())
            yield hb.samples[1][:, :per * k].reshape(chunk, k)
        else:
            sel_v, _, sel_rel, _ = cabi.budget_layer(rels, list(range(R)), 0, k, hub,
                                                     its if its is not None else torch.full_like(hub, -1), seed, c, window=window)
            assert int((sel_rel < 0).sum()) == 0, "an empty slot although the list is longer than k"
            yield sel_v


def _budget_check(route, tg, cabi, g, n, k, N, seed, what, window=None):
    law = L.uniform_law(n, k)
    tally = L.ReservoirTally(N, k, law, what)
    for E in _budget_chunks(route, tg, cabi, g, k, N, seed, window):
        tally.add(E.contiguous())
    # k = 1, n = 2: the quirk makes candidate 1 always replace candidate 0 -- one outcome of probability 1, asserted exactly
    # by the structural zeros, and no chi-square to run
    assert tally.finish() > 0 or law.marginal(0).max() == 1.0


@pytest.mark.parametrize("route", ["surface", "batched", "layer"])
@pytest.mark.parametrize("n,k,N", L.BUDGET_CASES)
def test_budget_sample_law(tg, cabi, route, n, k, N):
    """Budget::sample over a list of n candidates from 2, 3 or 16 relations (budget_sampling.rs:128-152), through
    tg.budget_sampling and tg_budget_sample_batched (the fused budf_select_kernel) and tg_budget_layer
    (budget_layer_kernel); N reaches power 0.999 against the law without the quirk for every (n, k)
    (test_power_budget_and_edge_phase_without_the_quirk)"""
    g = L.budget_hub_graph(L.BUDGET_LISTS[n])
    _budget_check(route, tg, cabi, g, n, k, N, 0xC10 + n + k, "budget %s k=%d n=%d" % (route, k, n))


@pytest.mark.parametrize("route", ["surface", "batched", "layer"])
def test_budget_sample_law_filtered(tg, cabi, route):
    """row timestamps and a window that admits a known subset: the law is uniform_law on the admitted subsequence"""
    f = L.BUDGET_FILTERED
    g = L.budget_hub_graph(f["lengths"], f["window"], 3)
    _budget_check(route, tg, cabi, g, g["n"], f["k"], L.BUDGET_FILTERED_OUTCOMES, 0xC20, "budget %s filtered" % route,
                  window=f["window"])
