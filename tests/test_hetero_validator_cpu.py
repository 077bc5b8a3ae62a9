"""The oracle-free validator of tests/helpers_hetero.py accepts what the oracle samples and rejects every single
corruption of it, naming the relation; worst_case_bounds reproduces hand-computed shapes.  No GPU."""
import copy

import numpy as np
import pytest

import orc
from helpers_hetero import (FILTER_DYNAMIC, FILTER_RELATIVE, FILTER_STATIC, admissible, check_hetero_result, rel_key,
                            worst_case_bounds)

NODE_TYPES = ["a", "b", "c"]
EDGE_TYPES = [("a", "self", "a"), ("b", "x", "a"), ("b", "y", "a"), ("a", "z", "b"), ("c", "w", "b")]
COUNTS = {"a": 60, "b": 45, "c": 30}
HOPS = 2
WINDOW = (0, 5)


def _graph():
    rs = np.random.default_rng(424242)
    P, I, W, TS = {}, {}, {}, {}
    for et in EDGE_TYPES:
        k = rel_key(et)
        e = 700
        ei = np.stack([rs.integers(0, COUNTS[et[0]], e), rs.integers(0, COUNTS[et[2]], e)]).astype(np.int64)
        P[k], I[k], _ = orc.to_csc(ei, (COUNTS[et[0]], COUNTS[et[2]]))
        W[k] = rs.uniform(0.5, 2.0, e)
        TS[k] = rs.integers(0, 12, e)
        z = np.flatnonzero(rs.random(e) < 0.15)               # exact zeros, never on a column's first edge
        z = z[~np.isin(z, P[k])]
        W[k][z] = 0.0
    inputs = {"a": rs.integers(0, COUNTS["a"], 9), "b": rs.integers(0, COUNTS["b"], 6)}
    ST = {t: rs.integers(0, 12, len(v)) for t, v in inputs.items()}
    nn = {rel_key(et): [3, 2] for et in EDGE_TYPES}
    return P, I, W, TS, inputs, ST, nn


VARIANTS = {
    # name: (sampler, weighted, filter mode or None, forward)
    "filtered": (orc.SAMPLER_UNIFORM, False, FILTER_DYNAMIC, True),
    "weighted": (orc.SAMPLER_WEIGHTED, True, None, False),
    "weighted+filtered": (orc.SAMPLER_WEIGHTED, True, FILTER_STATIC, False),
    "replace": (orc.SAMPLER_UNIFORM_REPL, False, FILTER_RELATIVE, False),
}


def _run(variant):
    P, I, W, TS, inputs, ST, nn = _graph()
    sampler, weighted, mode, fwd = VARIANTS[variant]
    kw, flt = dict(sampler=sampler), None
    if weighted:
        if mode is not None:                                  # the first admissible edge of a column keeps a weight
            for k in W:
                for c in range(len(P[k]) - 1):
                    col = np.arange(P[k][c], P[k][c + 1])
                    ok = col[admissible(TS[k][col], 0, mode, fwd, WINDOW)]
                    if len(ok) and W[k][ok[0]] == 0:
                        W[k][ok[0]] = 1.0
        kw["weights"] = W
    if mode is not None:
        kw.update(filter_mode=mode, forward=fwd, window=WINDOW, timestamps=TS, inputs_state=ST)
        flt = dict(mode=mode, forward=fwd, window=WINDOW, timestamps=TS, inputs_state=ST)
    res = orc.ns_hetero(NODE_TYPES, EDGE_TYPES, P, I, inputs, nn, HOPS, orc.rng_philox(11, 0), **kw)
    args = (NODE_TYPES, EDGE_TYPES, P, I, inputs, nn, HOPS)
    ck = dict(replace=sampler == orc.SAMPLER_UNIFORM_REPL, weights=W if weighted else None, flt=flt)
    return args, ck, res, (P, I, W, TS)


def _rejects(args, ck, res, key, **more):
    with pytest.raises(AssertionError, match=key):
        check_hetero_result(*args, res, **ck, **more)


def _hop_slice(res, key, h):
    lo = res[4][key]
    return lo[h][1], (lo[h + 1][1] if h + 1 < HOPS else len(res[1][key]))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_validator_accepts_the_oracle_and_rejects_each_corruption(variant):
    args, ck, res, (P, I, W, TS) = _run(variant)
    states = check_hetero_result(*args, res, **ck)
    assert sum(len(res[1][k]) for k in res[1]) > 100
    flt = ck["flt"]
    key = rel_key(EDGE_TYPES[1])                              # b -x-> a, shares the pair (b, a) with "y"
    src, dst = "b", "a"
    e0, e1 = _hop_slice(res, key, 0)
    assert e1 - e0 > 4

    def mutated():
        return copy.deepcopy(res)

    # 1. one edge_index moved to the neighbouring column
    m = mutated()
    e = next(e for e in range(e0, e1) if P[key][m[0][dst][m[2][key][e]] + 1] < len(I[key]))
    v = m[0][dst][m[2][key][e]]
    m[3][key][e] = P[key][v + 1]                             # first edge pointer past the column
    _rejects(args, ck, m, key)
    # 2. one cols entry shifted by one
    m = mutated()
    m[2][key][e0 + 1] += 1 if m[2][key][e0 + 1] == m[2][key][e0] else -1
    _rejects(args, ck, m, key)
    # 3. one sampled edge swapped for an inadmissible edge of the same column (filter), or for a zero-weight edge that
    #    comes after the reservoir's fill (weights alone)
    done = False
    for e in range(e0, e1):
        m = mutated()
        c = m[2][key][e]
        v = m[0][dst][c]
        col = np.arange(P[key][v], P[key][v + 1])
        if flt is not None:
            bad = col[~admissible(TS[key][col], states[dst][c], flt["mode"], flt["forward"], WINDOW)]
        else:
            bad = col[3:][W[key][col[3:]] == 0]
            bad = bad[~np.isin(bad, m[3][key][e0:e1][m[2][key][e0:e1] == c])]
        if len(bad):
            m[3][key][e] = bad[0]
            m[0][src][m[1][key][e]] = I[key][bad[0]]
            _rejects(args, ck, m, key)
            done = True
            break
    assert done, "the fixture has no inadmissible edge to swap in"
    # 4. one duplicate edge pointer, in the last hop so that no later frontier depends on the sample (legal with
    #    replacement, so not a corruption there)
    cl = res[2][key]
    l0, l1 = _hop_slice(res, key, HOPS - 1)
    e = next(e for e in range(l0, l1 - 1) if cl[e] == cl[e + 1])
    m = mutated()
    m[3][key][e + 1] = m[3][key][e]
    m[0][src][m[1][key][e + 1]] = m[0][src][m[1][key][e]]
    if ck["replace"]:
        check_hetero_result(*args, m, **ck)
    else:
        _rejects(args, ck, m, key)
    # 5. one column short by one sample: the last edge of the relation that appended last to its src list
    last = next(rel_key(et) for et in reversed(EDGE_TYPES)
                if len(res[1][rel_key(et)]) and res[1][rel_key(et)][-1] == len(res[0][et[0]]) - 1)
    m = mutated()
    for j in (1, 2, 3):
        m[j][last] = m[j][last][:-1]
    m[0][last.split("__")[0]] = m[0][last.split("__")[0]][:-1]
    _rejects(args, ck, m, last)
    # 6. layer_offsets of one hop off by one
    m = mutated()
    a, b, c = m[4][key][1]
    m[4][key][1] = (a, b + 1, c)
    _rejects(args, ck, m, key)
    # 7. one carried state changed
    if flt is not None:
        check_hetero_result(*args, res, **ck, states=states)
        st = {t: s.copy() for t, s in states.items()}
        st[src][res[1][key][e0]] += 1
        _rejects(args, ck, res, key, states=st)


def test_validator_rejects_a_sample_list_with_an_extra_sample():
    args, ck, res, _ = _run("filtered")
    m = copy.deepcopy(res)
    m[0]["c"] = np.append(m[0]["c"], 0)
    with pytest.raises(AssertionError, match="type c"):
        check_hetero_result(*args, m, **ck)


def test_worst_case_bounds_two_relations_by_hand():
    """a(10 inputs) <-x- b <-y- a, fan-outs x = [3, 2], y = [4, 5]:
    hop 0: cap_f = (10, 0): hop_m 10, one segment; fresh b = 30
    hop 1: cap_f = (0, 30): hop_m 30; fresh a = 150
    lists: a 10 + 150, b 30; edges x 30, y 150; max_f 30, max_out 150
    words = (160 + 30) * 2 + 3 * 180 + (5 * 30 + 4 * 150) * 2 = 380 + 540 + 1500 = 2420"""
    et = [("b", "x", "a"), ("a", "y", "b")]
    b = worst_case_bounds(["a", "b"], et, {"b__x__a": [3, 2], "a__y__b": [4, 5]}, 2, {"a": 10},
                          {"b__x__a": 5120, "a__y__b": 1023}, True)
    assert b["hop_m"] == [10, 30]
    assert b["group_bound"] == [1024, 1024]                   # 10 + 22 and 1 + 62: the floor of 1024 holds
    assert [[(r["m_round"], r["entries"], r["segments"], r["packed"]) for r in h] for h in b["rounds"]] == \
        [[(10, 2, 1, True)], [(30, 2, 1, True)]]
    assert b["words"] == 2420 and b["route"] == "device"
    assert worst_case_bounds(["a", "b"], et, {"b__x__a": [3, 2], "a__y__b": [4, 5]}, 2, {"a": 10},
                             {"b__x__a": 5120, "a__y__b": 1023}, False)["words"] == 2420 - 190


def test_worst_case_bounds_thresholds_by_hand():
    """one self relation, one hop, 2^17 + 1 inputs, fan-out 2, 4096 edges: m_round = 131073 > 2^17 -> padded;
    group bound = 8 + 262146 + 2 = 262156 <= 2^20; eightfold 2097248 > 2^20.  Three hops of fan-out 1024 from 8 inputs:
    edges 8 * (1024 + 1024^2 + 1024^3) * 3 words alone are above 8e9 bytes -> host-driven."""
    et = [("a", "s", "a")]
    n = (1 << 17) + 1
    b = worst_case_bounds(["a"], et, {"a__s__a": [2]}, 1, {"a": n}, {"a__s__a": 4096}, True)
    assert b["hop_m"] == [n] and b["group_bound"] == [262156]
    assert b["rounds"] == [[dict(m_round=n, entries=1, segments=1, packed=False)]]
    assert worst_case_bounds(["a"], et, {"a__s__a": [2]}, 1, {"a": n - 1}, {"a__s__a": 4096}, True)["rounds"][0][0]["packed"]
    b8 = worst_case_bounds(["a"], et, {"a__s__a": [2]}, 1, {"a": n - 1}, {"a__s__a": 4096}, True, group_mult=8)
    assert b8["group_bound"] == [8 * 262154] and not b8["rounds"][0][0]["packed"]
    big = worst_case_bounds(["a"], et, {"a__s__a": [1024] * 3}, 3, {"a": 8}, {"a__s__a": 100}, False)
    assert big["bytes"] > 8e9 and big["route"] == "host" and big["affordable"]
    assert big["hop_m"] == [8, 8 * 1024, 8 * 1024 * 1024]


def test_worst_case_bounds_rounds_of_16_entries_and_8_segments_by_hand():
    """20 relations in one hop: 0..9 into "a" (5 inputs), 10..19 into "b" (no inputs, so no segment).
    Round 1 closes when the 9th segment arrives: relations 0..7 (8 entries, 8 segments, m = 40); round 2 takes
    relations 8..19: 12 entries, 2 segments, m = 10.  With the first 17 into "b" instead: 16 entries without a segment,
    then 4 entries of which three have one (m = 15)."""
    nt = ["a", "b"]
    et = [("b", "r%d" % i, "a" if i < 10 else "b") for i in range(20)]
    nn = {rel_key(e): [2] for e in et}
    ne = {rel_key(e): 512 * (i + 1) for i, e in enumerate(et)}
    b = worst_case_bounds(nt, et, nn, 1, {"a": 5}, ne, True)
    assert b["hop_m"] == [50]
    assert b["group_bound"] == [max(1024, sum(range(1, 11)) + 100 + 2)]
    assert [(r["m_round"], r["entries"], r["segments"]) for r in b["rounds"][0]] == [(40, 8, 8), (10, 12, 2)]
    et2 = [("b", "r%d" % i, "b" if i < 17 else "a") for i in range(20)]
    b = worst_case_bounds(nt, et2, {rel_key(e): [2] for e in et2}, 1, {"a": 5}, {rel_key(e): 0 for e in et2}, True)
    assert [(r["m_round"], r["entries"], r["segments"]) for r in b["rounds"][0]] == [(0, 16, 0), (15, 4, 3)]
