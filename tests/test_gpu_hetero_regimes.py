"""neighbor_sampling_heterogenous under a temporal filter / with the weighted sampler on every route its driver takes
(host/python_module.cpp, the all_at_once branch): packed and padded frontier, long frontier and long group list inside
hs_run, the retry with eight times the column groups (also the one that drops the layout), mixed fan-outs in one round,
several rounds of one hop on different layouts, and the host-driven loop.  The route depends on worst-case sizes, so the
graphs are tiny and only the bounds are large.  Every case asserts three things: its regime (helpers_hetero.
worst_case_bounds), equality with the oracle word for word, and the oracle-free validator (check_hetero_result)."""
import numpy as np
import pytest
import torch

import orc
from helpers_hetero import (FILTER_DYNAMIC, FILTER_RELATIVE, FILTER_STATIC, PACKED_GROUPS_MAX, PACKED_M_MAX, admissible,
                            check_hetero_result, frontier_groups, rel_key, worst_case_bounds)

pytestmark = pytest.mark.gpu

WINDOW = (0, 5)
# name: (weighted, filter mode or None, forward).  Static ignores the direction (neighbor_sampling.rs:58).
VARIANTS = {
    "temporal-static": (False, FILTER_STATIC, True),
    "temporal-relative-backward": (False, FILTER_RELATIVE, False),
    "temporal-dynamic-forward": (False, FILTER_DYNAMIC, True),
    "weighted": (True, None, False),
    "weighted+temporal": (True, FILTER_DYNAMIC, False),
    "weighted+temporal-static": (True, FILTER_STATIC, False),
}
ALL = list(VARIANTS)[:5]
NODE_TYPES = ["a", "b", "c"]
# a self relation, two relations between the same pair, one into "c" (which has no inputs in most cases: no frontier in
# hop 0), one without edges
EDGE_TYPES = [("a", "self", "a"), ("b", "x", "a"), ("b", "y", "a"), ("a", "z", "b"), ("c", "w", "b"), ("a", "v", "c"),
              ("c", "none", "b")]
COUNTS = {"a": 300, "b": 200, "c": 100}


@pytest.fixture(scope="module")
def tg():
    import tch_geometric
    return tch_geometric


class Graph:
    def __init__(self, node_types, edge_types, counts, P, I, TS, W):
        self.node_types, self.edge_types, self.counts = node_types, edge_types, counts
        self.P, self.I, self.TS, self.W = P, I, TS, W
        self.rels = [rel_key(et) for et in edge_types]
        self.n_edges = {k: len(I[k]) for k in self.rels}
        self._cuda = {}

    def cuda(self, name):
        if name not in self._cuda:
            self._cuda[name] = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in getattr(self, name).items()}
        return self._cuda[name]


def csc_from_degrees(rs, n_src, degrees):
    P = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int64)
    return P, rs.integers(0, n_src, int(P[-1])).astype(np.int64)


def make_graph(seed, mean_degree, node_types=NODE_TYPES, edge_types=EDGE_TYPES, counts=COUNTS, degrees=None):
    """degrees: {relation: per-column degrees} overrides the Poisson columns of a relation"""
    rs = np.random.default_rng(seed)
    P, I, TS, W = {}, {}, {}, {}
    for et in edge_types:
        k = rel_key(et)
        if degrees is not None and k in degrees:
            deg = np.asarray(degrees[k], dtype=np.int64)
        elif et[1] == "none":
            deg = np.zeros(counts[et[2]], dtype=np.int64)
        else:
            deg = rs.poisson(mean_degree, counts[et[2]])
        P[k], I[k] = csc_from_degrees(rs, counts[et[0]], deg)
        TS[k] = rs.integers(0, 12, len(I[k]))
        W[k] = rs.uniform(0.1, 4.0, len(I[k]))
    return Graph(node_types, edge_types, counts, P, I, TS, W)


def _cuda(d):
    return {k: torch.from_numpy(np.ascontiguousarray(np.asarray(v))).cuda() for k, v in d.items()}


def bounds(g, inputs, nn, hops, variant, group_mult=1):
    return worst_case_bounds(g.node_types, g.edge_types, nn, hops, {t: len(v) for t, v in inputs.items()}, g.n_edges,
                             VARIANTS[variant][1] is not None, group_mult)


def hop_groups(g, inputs):
    """column groups the frontier of a ONE-hop call really needs: sum of ceil(deg / 512) over every relation's frontier"""
    return sum(frontier_groups(g.P[rel_key(et)], inputs[et[2]]) for et in g.edge_types if et[2] in inputs)


def run(tg, g, inputs, states, nn, hops, variant, seed, validate=True):
    """one call through the operator surface: equal to the oracle word for word, accepted by the validator"""
    weighted, mode, fwd = VARIANTS[variant]
    sampler, flt, kw, fdesc = None, None, {}, None
    if weighted:
        sampler, kw = tg.WeightedEdgeSampler(g.cuda("W")), dict(sampler=orc.SAMPLER_WEIGHTED, weights=g.W)
    if mode is not None:
        flt = (tg.TemporalEdgeFilter(WINDOW, g.cuda("TS"), fwd, mode), _cuda(states))
        kw.update(filter_mode=mode, forward=fwd, window=WINDOW, timestamps=g.TS, inputs_state=states)
        fdesc = dict(mode=mode, forward=fwd, window=WINDOW, timestamps=g.TS, inputs_state=states)
    tg.seed(seed)
    got = tg.neighbor_sampling_heterogenous(g.node_types, g.edge_types, g.cuda("P"), g.cuda("I"), _cuda(inputs), nn, hops,
                                            sampler, flt)
    o = orc.ns_hetero(g.node_types, g.edge_types, g.P, g.I, inputs, nn, hops, orc.rng_philox(seed, 0), **kw)
    res = tuple({k: v.cpu().numpy() for k, v in d.items()} for d in got[:4]) + ({k: [tuple(x) for x in got[4][k]] for k in g.rels},)
    for t in g.node_types:
        assert np.array_equal(res[0][t], o[0][t]), ("samples", t)
    for j, name in ((1, "rows"), (2, "cols"), (3, "edge_index")):
        for k in g.rels:
            assert np.array_equal(res[j][k], o[j][k]), (name, k)
    for k in g.rels:
        assert res[4][k] == o[4][k], ("layer_offsets", k)
    if validate:
        check_hetero_result(g.node_types, g.edge_types, g.P, g.I, inputs, nn, hops, res, weights=g.W if weighted else None,
                            flt=fdesc)
    return res


def make_inputs(rs, g, n):
    inputs = {t: rs.integers(0, g.counts[t], c) for t, c in n.items() if c}
    return inputs, {t: rs.integers(0, 12, len(v)) for t, v in inputs.items()}


@pytest.fixture(scope="module")
def sparse():
    return make_graph(101, 1.5)


@pytest.fixture(scope="module")
def denser():
    return make_graph(106, 2.5)


# ---------------------------------------------------------------- padded frontier, long m, short group list
@pytest.mark.parametrize("variant", ALL)
def test_padded_frontier_long_m_short_group_list(tg, denser, variant):
    g = denser
    inputs, states = make_inputs(np.random.default_rng(1), g, {"a": 701, "b": 697})
    nn = {k: [6 + i % 3, 2, 7] for i, k in enumerate(g.rels)}
    b = bounds(g, inputs, nn, 3, variant)
    assert b["route"] == "device"
    assert b["cap_f"][0][g.rels.index("a__v__c")] == 0 and g.n_edges["c__none__b"] == 0
    padded = [(h, r) for h in range(3) for r in b["rounds"][h] if not r["packed"]]
    assert padded and all(gb <= PACKED_GROUPS_MAX for gb in b["group_bound"])     # long m alone drops the layout
    assert any(r["m_round"] % 256 and r["m_round"] % 1024 for _, r in padded)
    assert all(r["packed"] for r in b["rounds"][0])                                 # and hop 0 of the same call is packed
    res = run(tg, g, inputs, states, nn, 3, variant, 21)
    assert 10 ** 4 <= sum(len(v) for v in res[1].values()) <= 10 ** 6


# ---------------------------------------------------------------- long group list
@pytest.mark.parametrize("variant", ALL)
def test_long_group_list(tg, sparse, variant):
    g = sparse
    inputs, states = make_inputs(np.random.default_rng(2), g, {"a": 2001, "b": 1999})
    nn = {k: [8, 8, 7] for k in g.rels}
    b = bounds(g, inputs, nn, 3, variant)
    assert b["route"] == "device"
    assert max(b["hop_m"]) > 1 << 19 and max(b["group_bound"]) > PACKED_GROUPS_MAX
    assert b["group_bound"][0] <= PACKED_GROUPS_MAX < b["group_bound"][2]
    res = run(tg, g, inputs, states, nn, 3, variant, 22)
    assert 10 ** 4 <= sum(len(v) for v in res[1].values()) <= 10 ** 6


# ---------------------------------------------------------------- exactly at the thresholds
def solve_inputs(g, target_m):
    """inputs per type with sum over relations of the frontier = target_m in a one-hop call (inputs on "a" and "c")"""
    into = {t: sum(1 for et in g.edge_types if et[2] == t) for t in g.node_types}
    for nc in range(into["a"]):
        rest = target_m - nc * into["c"]
        if rest >= 0 and rest % into["a"] == 0:
            return {"a": rest // into["a"], "c": nc}
    raise AssertionError("no solution")


@pytest.mark.parametrize("variant", ["temporal-relative-backward", "temporal-dynamic-forward", "weighted", "weighted+temporal"])
@pytest.mark.parametrize("m_round", [PACKED_M_MAX, PACKED_M_MAX + 1])
def test_frontier_bound_at_the_layout_threshold(tg, sparse, variant, m_round):
    g = sparse
    inputs, states = make_inputs(np.random.default_rng(3), g, solve_inputs(g, m_round))
    nn = {k: [2] for k in g.rels}
    b = bounds(g, inputs, nn, 1, variant)
    assert b["route"] == "device" and len(b["rounds"][0]) == 1
    assert b["rounds"][0][0]["m_round"] == m_round and b["group_bound"][0] <= PACKED_GROUPS_MAX
    assert b["rounds"][0][0]["packed"] == (m_round <= PACKED_M_MAX)
    run(tg, g, inputs, states, nn, 1, variant, 23)


@pytest.mark.parametrize("variant", ["temporal-static", "temporal-relative-backward", "temporal-dynamic-forward", "weighted",
                                     "weighted+temporal"])
@pytest.mark.parametrize("side", ["at-or-below", "above"])
def test_group_bound_at_the_scan_threshold(tg, sparse, variant, side):
    g = sparse
    fixed = sum(g.n_edges[rel_key(et)] // 512 for et in g.edge_types if et[2] == "a") + 2
    into_a = sum(1 for et in g.edge_types if et[2] == "a")
    n = (PACKED_GROUPS_MAX - fixed) // (2 * into_a)          # the largest n with fixed + 2 * into_a * n <= 2^20
    n += side == "above"
    inputs, states = make_inputs(np.random.default_rng(4), g, {"a": n})
    nn = {k: [1] for k in g.rels}
    b = bounds(g, inputs, nn, 1, variant)
    assert b["route"] == "device" and b["group_bound"][0] == fixed + 2 * into_a * n
    assert (b["group_bound"][0] <= PACKED_GROUPS_MAX) == (side != "above")
    assert b["group_bound"][0] + 2 * into_a > PACKED_GROUPS_MAX >= b["group_bound"][0] - 2 * into_a
    assert not b["rounds"][0][0]["packed"]                   # m is long on both sides: only the group scan changes
    run(tg, g, inputs, states, nn, 1, variant, 24)


# ---------------------------------------------------------------- retry with eight times the column groups
HUB = 7                                                       # the vertex of "a" whose column in b -x-> a is the hub


def hub_graph(hub_degree, seed=102):
    rs = np.random.default_rng(seed)
    deg = rs.poisson(1.5, COUNTS["a"])
    deg[HUB] = hub_degree
    return make_graph(seed, 1.5, degrees={"b__x__a": deg})


def hub_inputs(g, repeats, seed=5):
    rs = np.random.default_rng(seed)
    tail = np.array([3, 11, 200, 42, 7], dtype=np.int64)
    a = np.concatenate([np.full(repeats, HUB, dtype=np.int64), tail])
    return {"a": a}, {"a": np.concatenate([rs.integers(0, 12, max(repeats, 600))[:repeats], np.arange(5)])}


@pytest.fixture(scope="module")
def hub4096():
    return hub_graph(4096)


@pytest.mark.parametrize("variant", ALL)
def test_retry_with_eight_times_the_groups(tg, hub4096, variant):
    g = hub4096
    nn = {k: [3] for k in g.rels}
    inputs, states = hub_inputs(g, 600)
    b1, b8 = bounds(g, inputs, nn, 1, variant), bounds(g, inputs, nn, 1, variant, 8)
    need = hop_groups(g, inputs)
    assert b1["route"] == "device" and b1["group_bound"][0] < need < b8["group_bound"][0]     # one retry, then it fits
    assert b1["rounds"][0][0]["packed"] and b8["rounds"][0][0]["packed"]
    big = run(tg, g, inputs, states, nn, 1, variant, 25)
    few, few_states = hub_inputs(g, 9)
    assert hop_groups(g, few) < bounds(g, few, nn, 1, variant)["group_bound"][0]                # no retry
    small = run(tg, g, few, few_states, nn, 1, variant, 25)
    # one hop: a draw is addressed by (seed, call, relation tag, slot of the frontier vertex in its type's list)
    # (tchgeo.h, "Draw address"), so the first nine slots -- same vertex, same state -- sample the same edges
    for k in g.rels:
        assert np.array_equal(big[3][k][big[2][k] < 9], small[3][k][small[2][k] < 9]), k
        assert np.array_equal(big[2][k][big[2][k] < 9], small[2][k][small[2][k] < 9]), k


@pytest.mark.parametrize("variant", ["temporal-dynamic-forward", "weighted"])
def test_homogeneous_one_call_path_retries(tg, hub4096, variant):
    """run_ns_filtered_device: the same retry for neighbor_sampling_homogenous (bound: max(1024, E / 512 + 2 m + 2))"""
    g = hub4096
    weighted, mode, fwd = VARIANTS[variant]
    rs = np.random.default_rng(6)
    n = g.counts["a"]
    deg = rs.poisson(1.5, n)
    deg[HUB] = 4096
    P, I = csc_from_degrees(rs, n, deg)
    ts, w = rs.integers(0, 12, len(I)), rs.uniform(0.1, 4.0, len(I))
    inputs, states = hub_inputs(g, 600)
    inputs, states = inputs["a"], states["a"]
    first = max(1024, len(I) // 512 + 2 * len(inputs) + 2)
    assert first < frontier_groups(P, inputs) < 8 * first <= PACKED_GROUPS_MAX
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tg.seed(26)
    if weighted:
        got = tg.neighbor_sampling_homogenous(c(P), c(I), c(inputs), [3], tg.WeightedEdgeSampler(c(w)))
        o = orc.ns_homo(P, I, inputs, [3], orc.rng_philox(26, 0), sampler=orc.SAMPLER_WEIGHTED, weights=w)
    else:
        got = tg.neighbor_sampling_homogenous(c(P), c(I), c(inputs), [3], None,
                                              (tg.TemporalEdgeFilter(WINDOW, c(ts), fwd, mode), c(states)))
        o = orc.ns_homo(P, I, inputs, [3], orc.rng_philox(26, 0), filter_mode=mode, forward=fwd, window=WINDOW,
                        timestamps=ts, inputs_state=states)
    for a, b_ in zip(got[:4], o[:4]):
        assert np.array_equal(a.cpu().numpy(), b_)
    assert [tuple(x) for x in got[4]] == o[4]
    res = tuple({"n__e__n": x.cpu().numpy()} if j else {"n": x.cpu().numpy()} for j, x in enumerate(got[:4])) + \
        ({"n__e__n": [tuple(x) for x in got[4]]},)
    check_hetero_result(["n"], [("n", "e", "n")], {"n__e__n": P}, {"n__e__n": I}, {"n": inputs}, {"n__e__n": [3]}, 1, res,
                        weights={"n__e__n": w} if weighted else None,
                        flt=None if weighted else dict(mode=mode, forward=fwd, window=WINDOW, timestamps={"n__e__n": ts},
                                                       inputs_state={"n": states}))


@pytest.mark.parametrize("variant", ["temporal-static", "weighted"])
def test_retry_that_drops_the_layout(tg, variant):
    """every input is the hub and only b -x-> a points into "a": the first attempt is packed and overflows, eight times
    its group bound is above 2^20, so the second attempt runs on the padded frontier"""
    et = [("b", "x", "a"), ("a", "z", "b"), ("c", "w", "b")]
    deg = np.random.default_rng(7).poisson(1.5, COUNTS["a"])
    deg[HUB] = 2048                                           # four groups a column: the oracle's scan stays short
    g = make_graph(103, 1.5, edge_types=et, degrees={"b__x__a": deg})
    # one hop, one relation into "a": the first bound is fixed + 2 n.  The smallest n whose eightfold bound passes 2^20
    fixed = g.n_edges["b__x__a"] // 512 + 2
    n = (PACKED_GROUPS_MAX // 8 - fixed) // 2 + 1
    assert 8 * (fixed + 2 * n) > PACKED_GROUPS_MAX >= 8 * (fixed + 2 * (n - 1)) and n <= PACKED_M_MAX
    rs = np.random.default_rng(8)
    inputs, states = {"a": np.full(n, HUB, dtype=np.int64)}, {"a": rs.integers(0, 12, n)}
    nn = {k: [2] for k in g.rels}
    b1, b8 = bounds(g, inputs, nn, 1, variant), bounds(g, inputs, nn, 1, variant, 8)
    need = hop_groups(g, inputs)
    assert b1["route"] == "device"
    assert b1["group_bound"][0] <= PACKED_GROUPS_MAX and b1["rounds"][0][0]["packed"]
    assert b1["group_bound"][0] < need < b8["group_bound"][0]
    assert b8["group_bound"][0] > PACKED_GROUPS_MAX and not b8["rounds"][0][0]["packed"]
    run(tg, g, inputs, states, nn, 1, variant, 27)


# ---------------------------------------------------------------- mixed fan-outs in one round
MIXED_FANOUT = {"a__self__a": 1, "b__x__a": 65, "b__y__a": 200, "a__z__b": 1024, "c__w__b": 7, "a__v__c": 3, "c__none__b": 2}


def mixed_graph(variant):
    weighted, mode, fwd = VARIANTS[variant]
    rs = np.random.default_rng(104)
    degrees = {}
    for et in EDGE_TYPES[:5]:
        k = rel_key(et)
        f = MIXED_FANOUT[k]
        deg = rs.poisson(2.0, COUNTS[et[2]])
        deg[:6] = [max(f - 1, 0), f, f + 1, 3 * f, 0, 2 * f + 1]     # column lengths on both sides of the fan-out
        if k == "b__x__a":
            deg[6] = 1500                                              # three 512-edge groups
        degrees[k] = deg
    g = make_graph(104, 2.0, degrees=degrees)
    g.W["b__y__a"] = 10.0 ** rs.uniform(-6, 6, len(g.I["b__y__a"]))    # magnitudes 10^12 apart
    if mode not in (None, FILTER_STATIC):      # a state-dependent filter moves a column's first admissible edge, so the
        return g                               # running sum could start at zero (a panic by rule): no zeros there
    for k in g.rels:                                                    # exact zeros, but never on the first edge a
        z = rs.random(len(g.I[k])) < 0.2                                # column offers: the running sum stays > 0
        first = np.zeros(len(z), dtype=bool)
        if mode is not None:
            ok = admissible(g.TS[k], 0, mode, fwd, WINDOW)
            for c in range(len(g.P[k]) - 1):
                col = np.arange(g.P[k][c], g.P[k][c + 1])
                col = col[ok[col]]
                first[col[:1]] = True
        else:
            first[g.P[k][:-1][np.diff(g.P[k]) > 0]] = True
        g.W[k][z & ~first] = 0.0
    return g


@pytest.mark.parametrize("variant", ["temporal-static", "temporal-relative-backward", "temporal-dynamic-forward", "weighted",
                                     "weighted+temporal-static", "weighted+temporal"])
def test_mixed_fanouts_in_one_round(tg, variant):
    """(weights with exact zeros need a first admissible edge that no state moves: the static filter carries them;
    weighted under the dynamic filter runs the same fan-outs without zeros)"""
    g = mixed_graph(variant)
    inputs = {"a": np.concatenate([np.arange(12), [6, 6, 3]]).astype(np.int64), "b": np.arange(10, dtype=np.int64)}
    rs = np.random.default_rng(9)
    states = {t: rs.integers(0, 12, len(v)) for t, v in inputs.items()}
    nn = {k: [MIXED_FANOUT[k], 1 + i % 3] for i, k in enumerate(g.rels)}
    b = bounds(g, inputs, nn, 2, variant)
    assert b["route"] == "device" and len(b["rounds"][0]) == 1 and b["rounds"][0][0]["segments"] == 6
    res = run(tg, g, inputs, states, nn, 2, variant, 28)
    lo = res[4]
    assert lo["a__z__b"][1][1] > 1024 and lo["b__y__a"][1][1] > 200             # the wide fan-outs were really filled
    assert sum(len(res[1][k]) - lo[k][1][1] for k in g.rels) > 1000              # and served as the next frontier


# ---------------------------------------------------------------- several rounds of one hop on different layouts
def many_relations_graph():
    """the 23-relation graph of test_gpu_random_sweep_hetero.test_hetero_many_relations_take_several_rounds"""
    rs = np.random.default_rng(9100)
    node_types, counts = ["a", "b", "c"], {"a": 150, "b": 90, "c": 40}
    edge_types, P, I, TS, W = [], {}, {}, {}, {}
    for r in range(23):
        s, d = node_types[int(rs.integers(0, 3))], node_types[int(rs.integers(0, 3))]
        if r in (4, 17):
            d = "c"
        et = (s, "r%d" % r, d)
        e = 0 if r == 9 else int(rs.integers(50, 900))
        ei = np.stack([rs.integers(0, counts[s], e), rs.integers(0, counts[d], e)]).astype(np.int64).reshape(2, e)
        edge_types.append(et)
        P[rel_key(et)], I[rel_key(et)], _ = orc.to_csc(ei, (counts[s], counts[d]))
    rs = np.random.default_rng(9101)
    for k in P:
        TS[k], W[k] = rs.integers(0, 12, len(I[k])), rs.uniform(0.1, 4.0, len(I[k]))
    return Graph(node_types, edge_types, counts, P, I, TS, W)


@pytest.mark.parametrize("variant", ["temporal-dynamic-forward", "weighted", "weighted+temporal"])
def test_many_relations_rounds_on_different_layouts(tg, variant):
    g = many_relations_graph()
    nn = {k: [1 + i % 2, 1 + (i + 1) % 2] for i, k in enumerate(g.rels)}
    found = None
    for n in range(500, 40000, 250):                          # the smallest call with a padded and a packed round in one hop
        sizes = {"a": n, "b": n // 2 + 1}
        b = worst_case_bounds(g.node_types, g.edge_types, nn, 2, sizes, g.n_edges, VARIANTS[variant][1] is not None)
        if any(len({r["packed"] for r in rr}) == 2 for rr in b["rounds"]):
            found = (sizes, b)
            break
    assert found, "no call size puts two layouts into one hop"
    sizes, b = found
    assert b["route"] == "device" and all(len(rr) >= 2 for rr in b["rounds"])    # > 16 entries, > 8 segments
    inputs, states = make_inputs(np.random.default_rng(10), g, sizes)
    res = run(tg, g, inputs, states, nn, 2, variant, 29)
    assert 10 ** 4 <= sum(len(v) for v in res[1].values()) <= 10 ** 6


# ---------------------------------------------------------------- host-driven route
@pytest.fixture(scope="module")
def thin():
    rs = np.random.default_rng(105)
    degrees = {}
    for et in EDGE_TYPES[:6]:
        deg = np.minimum(rs.poisson(1.2, COUNTS[et[2]]), 30)
        deg[5] = 30
        degrees[rel_key(et)] = deg
    return make_graph(105, 1.2, degrees=degrees)


@pytest.mark.parametrize("variant", ["temporal-static", "temporal-relative-backward", "weighted", "weighted+temporal"])
@pytest.mark.parametrize("fanout,route", [(1024, "host"), (30, "device")])
def test_host_driven_route_and_its_device_twin(tg, thin, variant, fanout, route):
    g = thin
    inputs = {"a": np.array([5, 1, 17, 5], dtype=np.int64), "b": np.array([5, 2, 9], dtype=np.int64)}
    states = {"a": np.array([0, 3, 6, 9]), "b": np.array([2, 5, 11])}
    nn = {k: [fanout] * 3 for k in g.rels}
    b = bounds(g, inputs, nn, 3, variant)
    assert b["route"] == route and b["affordable"]
    assert (b["bytes"] > 8e9) == (route == "host")
    assert max(int(np.diff(g.P[k]).max()) for k in g.rels) == 30               # fan-out 30 already takes whole columns
    res = run(tg, g, inputs, states, nn, 3, variant, 30)
    assert 100 < sum(len(v) for v in res[1].values()) <= 10 ** 6


# ---------------------------------------------------------------- the zero-sum panic survives the routes
def _zero_column(g, rel, vertex):
    W = {k: v.copy() for k, v in g.W.items()}
    W[rel][g.P[rel][vertex]:g.P[rel][vertex + 1]] = 0.0
    out = Graph(g.node_types, g.edge_types, g.counts, g.P, g.I, g.TS, W)
    return out


@pytest.mark.parametrize("route", ["padded", "retry", "host"])
def test_zero_weight_column_panics_on_every_route(tg, sparse, hub4096, thin, route):
    """sampling.rs:49: a float range that is empty panics in the reference; the operator raises PanicException, whatever
    the route the call took"""
    if route == "padded":
        g = sparse
        v = int(np.argmax(np.diff(g.P["a__self__a"])))
        assert g.P["a__self__a"][v + 1] - g.P["a__self__a"][v] > 2
        g = _zero_column(g, "a__self__a", v)
        inputs = {"a": np.concatenate([np.random.default_rng(11).integers(0, g.counts["a"], 50000), [v]])}
        nn = {k: [2] for k in g.rels}
        b = bounds(g, inputs, nn, 1, "weighted")
        assert b["route"] == "device" and not b["rounds"][0][0]["packed"]
        hops = 1
    elif route == "retry":
        g = _zero_column(hub4096, "b__x__a", HUB)
        inputs, _ = hub_inputs(g, 600)
        nn = {k: [3] for k in g.rels}
        b1, b8 = bounds(g, inputs, nn, 1, "weighted"), bounds(g, inputs, nn, 1, "weighted", 8)
        assert b1["group_bound"][0] < hop_groups(g, inputs) < b8["group_bound"][0]
        hops = 1
    else:
        g = _zero_column(thin, "b__x__a", 5)                  # the column of 30 edges
        inputs = {"a": np.array([1, 5], dtype=np.int64)}
        nn = {k: [1024 if k != "b__x__a" else 7] * 3 for k in g.rels}
        assert bounds(g, inputs, nn, 3, "weighted")["route"] == "host"
        hops = 3
    with pytest.raises(tg.PanicException):
        tg.neighbor_sampling_heterogenous(g.node_types, g.edge_types, g.cuda("P"), g.cuda("I"), _cuda(inputs), nn, hops,
                                          tg.WeightedEdgeSampler(g.cuda("W")), None)
