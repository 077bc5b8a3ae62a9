"""The closed-form laws of exact_laws.py against exhaustive enumeration of the reference's loops (rational arithmetic), the
oracle's philox-mode (the counter-addressed restatements the kernels share) against those laws on long columns, and the
power of the test against named wrong laws at the sample sizes tests/test_gpu_exact_laws.py and
tests/test_gpu_exact_laws_typed.py use.  The typed samplers (hgt_sampling, budget_sampling) have their enumeration, oracle and
power tests here as well, and so have the batch kernels of tests/test_gpu_exact_laws_batches.py (link seed rows, skip-gram
negatives, consecutive walk steps): enumeration of the sequential loops, the NumPy models of tests/helpers_*.py against the
laws, and the power at that file's sample sizes."""
from collections import Counter
from fractions import Fraction
from itertools import product

import numpy as np
import pytest
import torch

import exact_laws as L
import orc
from exact_laws import N_NEG, N_WALK, n_outcomes
from test_reservoir_equivalence import law_reference_loop, law_tickets


# ---------------------------------------------------------------- closed forms == enumeration
def _slot_marginals(law_counter, n, k):
    M = np.zeros((k, n))
    for dst, p in law_counter.items():
        for s, v in enumerate(dst):
            M[s, v] += float(p)
    return M


def _pair(law_counter, n, s, t):
    J = np.zeros((n, n))
    for dst, p in law_counter.items():
        J[dst[s], dst[t]] += float(p)
    return J


def _binned_pair(J, law, edges):
    """fold an exact [n, n] joint law of two slots into ReservoirLaw.pair_table's categories"""
    cat = np.searchsorted(edges, np.arange(law.n), side="right")
    m = len(edges) - 1
    T = np.zeros((m + 1, m + 1))
    np.add.at(T, (cat[:, None].repeat(law.n, 1), cat[None, :].repeat(law.n, 0)), J)
    return T


def law_weighted_loop(w, k):
    """sampling.rs:28-55 enumerated: candidate i >= k is taken with probability w_i / W_i, then writes slot
    U[0, k)."""
    w = [Fraction(x) for x in w]
    n = len(w)
    law = Counter({tuple(range(k)): Fraction(1)})
    W = sum(w[:k])
    for i in range(k, n):
        W += w[i]
        t = w[i] / W
        nxt = Counter()
        for dst, p in law.items():
            nxt[dst] += p * (1 - t)
            for j in range(k):
                d = list(dst)
                d[j] = i
                nxt[tuple(d)] += p * t / k
        law = nxt
    return law


def law_chunked_one_slot(raw_pos):
    """orc_reservoir_one_chunked enumerated over its chunk draws: a chunk with m eligible candidates after M takes the
    slot with probability m / (M + m) and holds each of its m with probability 1 / m."""
    n = len(raw_pos)
    P = [Fraction(0)] * n
    P[0] = Fraction(1)
    seen, i = 0, 1
    while i < n:
        j = i
        while j < n and raw_pos[j] >> 6 == raw_pos[i] >> 6:
            j += 1
        m = j - i
        t = Fraction(1) if seen == 0 else Fraction(m, seen + m)
        P = [x * (1 - t) for x in P[:i]] + [t / m] * m + P[j:]
        seen += m
        i = j
    return P


@pytest.mark.parametrize("n,k", [(2, 1), (5, 1), (4, 2), (6, 2), (7, 3), (8, 3), (7, 5)])
def test_uniform_closed_form_equals_enumeration(n, k):
    ref = law_reference_loop(n, k)
    assert law_tickets(n, k) == ref
    law = L.uniform_law(n, k)
    M = _slot_marginals(ref, n, k)
    for s in range(k):
        assert np.allclose(law.marginal(s), M[s], atol=1e-14, rtol=0)
    if k >= 2:
        edges = np.arange(k, n + 1)                                        # one bin per later position: exact pairs
        for s, t in ((0, 1), (1, 0), (0, k - 1)):
            assert np.allclose(law.pair_table(edges), _binned_pair(_pair(ref, n, s, t), law, edges), atol=1e-14, rtol=0)
        coarse = np.array([k, (k + n + 1) // 2, n]) if n - k > 1 else np.array([k, n])
        assert np.allclose(law.pair_table(coarse), _binned_pair(_pair(ref, n, 0, 1), law, coarse), atol=1e-14, rtol=0)


@pytest.mark.parametrize("w,k", [([1, 2, 3, 4, 5, 6], 2), ([3, 0, 1, 0, 7, 2, 5], 2), ([1, 5, 0, 2, 9], 1),
                                 ([0, 2, 1e-3, 0, 6, 1, 4], 3), ([1, 1, 1, 1, 1, 1, 1], 3)])
def test_weighted_closed_form_equals_enumeration(w, k):
    ref = law_weighted_loop(w, k)
    n = len(w)
    law = L.weighted_law(w, k)
    M = _slot_marginals(ref, n, k)
    for s in range(k):
        assert np.allclose(law.marginal(s), M[s], atol=1e-13, rtol=0)
    zero = [p for p in range(k, n) if w[p] == 0]
    assert all(M[:, p].sum() == 0 for p in zero) and all(law.marginal(0)[p] == 0 for p in zero)
    if k >= 2:
        edges = np.arange(k, n + 1)
        for s, t in ((0, 1), (k - 1, 0)):
            assert np.allclose(law.pair_table(edges), _binned_pair(_pair(ref, n, s, t), law, edges), atol=1e-13, rtol=0)


@pytest.mark.parametrize("raw", [[0], [3, 9], list(range(10)), [5, 70, 71, 200, 300], [0, 63, 64, 65, 127, 128, 1000],
                                 [70, 71, 72, 500, 4999]])
def test_one_slot_laws_equal_enumeration(raw):
    n = len(raw)
    exact = law_chunked_one_slot(raw)
    assert sum(exact) == 1
    assert np.allclose(L.one_slot_walk_law(n), [float(x) for x in exact], atol=1e-15, rtol=0)
    assert np.allclose(L.one_slot_chunked_law(raw), L.one_slot_walk_law(n), atol=1e-15, rtol=0)
    if n <= 8:                                                           # the literal loop with k = 1
        lit = law_reference_loop(n, 1) if n > 1 else Counter({(0,): Fraction(1)})
        assert [float(lit.get((c,), 0)) for c in range(n)] == pytest.approx(L.one_slot_walk_law(n), abs=1e-15)


def test_negative_item_law_equals_enumeration():
    size, tries = 6, 3
    adm = np.array([0, 1, 1, 0, 1, 0], dtype=bool)
    P = [Fraction(0)] * (size + 1)
    for ws in product(range(size), repeat=tries):                        # every draw sequence, equally likely
        hit = next((w for w in ws if adm[w]), None)
        P[size if hit is None else hit] += Fraction(1, size ** tries)
    assert np.allclose(L.negative_item_law(size, adm, tries), [float(x) for x in P], atol=1e-15, rtol=0)


def test_node2vec_law_is_the_rejection_loop_fixed_point():
    """the loop's law: P(v) = sum_r (1 - A)^r acc_v / deg = acc_v / (deg A), A the mean acceptance (exact)"""
    ptrs = np.array([0, 1, 5, 6, 8, 9])
    col = np.array([1, 0, 2, 2, 3, 4, 0, 1, 1])                          # vertex 1's row: 0, 2, 2, 3 (a multiplicity)
    law = L.node2vec_step_law(ptrs, col, 1, 0, 0.5, 4.0)
    p0, p1, p2 = L.node2vec_probs(0.5, 4.0)
    acc = np.array([p0, p2, p2, p1])                                     # 0 = prev; 3 -> 0 is an edge; 2 -> 0 is not
    assert np.allclose(law, acc / acc.sum())


# ---------------------------------------------------------------- the oracle's philox-mode on long columns
def _hub(n):
    return np.array([0, n], dtype=np.int64), np.zeros(n, dtype=np.int64)


N_CPU = 1 << 16


@pytest.mark.parametrize("n,k", [(18, 17), (64, 17), (1000, 33), (70000, 65), (1000, 129)])
def test_oracle_uniform_reservoir_follows_the_exact_law(n, k):
    N = N_CPU if k < 100 else N_CPU // 4
    ptrs, idx = _hub(n)
    o = orc.ns_homo(ptrs, idx, np.zeros(N, dtype=np.int64), [k], orc.rng_philox(0xE1, 3))
    E = torch.from_numpy(o[3].reshape(N, k))
    assert L.check_reservoir(E, L.uniform_law(n, k), "oracle uniform k=%d n=%d" % (k, n)) > 0


def test_oracle_replacement_follows_the_exact_law():
    n, k = 1000, 33
    ptrs, idx = _hub(n)
    o = orc.ns_homo(ptrs, idx, np.zeros(N_CPU, dtype=np.int64), [k], orc.rng_philox(0xE2, 3), sampler=1)
    L.check_reservoir(torch.from_numpy(o[3].reshape(N_CPU, k)), L.ReplacementLaw(n, k), "oracle replacement", replace=True)


def weights_wide(n, seed):
    """weights 1e-6 .. 1e6 (log-uniform) with zeros interleaved; the first candidate positive (the reference panics on
    an empty running sum)"""
    rs = np.random.default_rng(seed)
    w = 10.0 ** rs.uniform(-6, 6, n)
    w[rs.random(n) < 0.25] = 0.0
    w[0] = 1.0
    return w


@pytest.mark.parametrize("n,k", [(65, 5), (5000, 5), (5000, 64), (513, 1)])
def test_oracle_weighted_reservoir_follows_the_exact_law(n, k):
    ptrs, idx = _hub(n)
    w = weights_wide(n, n + k)
    o = orc.ns_homo(ptrs, idx, np.zeros(N_CPU, dtype=np.int64), [k], orc.rng_philox(0xE3, 3), sampler=2, weights=w)
    E = torch.from_numpy(o[3].reshape(N_CPU, k))
    L.check_reservoir(E, L.weighted_law(w, k), "oracle weighted k=%d n=%d" % (k, n), zero_pos=torch.from_numpy(w == 0))


def test_oracle_filtered_weighted_reservoir_follows_the_law_on_the_admitted_subsequence():
    n, k = 5000, 5
    rs = np.random.default_rng(9)
    ts = rs.integers(0, 90, n)
    w = weights_wide(n, 77)
    adm = (ts >= 10) & (ts <= 40)                                        # FILTER_STATIC: the window is inclusive
    ptrs, idx = _hub(n)
    o = orc.ns_homo(ptrs, idx, np.zeros(N_CPU, dtype=np.int64), [k], orc.rng_philox(0xE4, 3), sampler=2, weights=w,
                    filter_mode=0, window=(10, 40), timestamps=ts, inputs_state=np.zeros(N_CPU, dtype=np.int64))
    rank = np.full(n, -1)
    rank[adm] = np.arange(adm.sum())
    E = torch.from_numpy(rank[o[3].reshape(N_CPU, k)])
    wa = w[adm]
    L.check_reservoir(E, L.weighted_law(wa, k), "oracle filtered weighted", zero_pos=torch.from_numpy(wa == 0))


def walk_row(length, pattern):
    """admissible raw positions of a tempo-walk row: 'scatter' (about a third), 'edges' (first admissible candidate in
    chunk 1, empty chunks between, one in the last chunk and around every chunk boundary)"""
    if pattern == "all":
        return np.arange(length)
    if pattern == "scatter":
        return np.flatnonzero(np.random.default_rng(length).random(length) < 0.35)
    pos = {64, length - 1}
    for c in range(1, (length - 1) // 64 + 1):
        if c % 3 != 2:                                                   # every third chunk stays empty
            pos |= {64 * c - 1, 64 * c, 64 * c + 1} if c > 1 else {64, 65}
    return np.array(sorted(p for p in pos if 64 <= p < length))


def tempo_graph(length, adm):
    """vertex 0's CSR row: `length` out-edges to vertices 1..length, edge time 10 where admissible, 100 elsewhere"""
    ptrs = np.zeros(length + 2, dtype=np.int64)
    ptrs[1:] = length
    idx = np.arange(1, length + 1, dtype=np.int64)
    ets = np.full(length, 100, dtype=np.int64)
    ets[adm] = 10
    return ptrs, idx, np.full(length + 1, -1, dtype=np.int64), ets


@pytest.mark.parametrize("length,pattern", [(2, "all"), (65, "edges"), (129, "edges"), (5000, "edges"), (5000, "scatter")])
def test_oracle_chunked_walk_step_follows_the_exact_law(length, pattern):
    adm = walk_row(length, pattern)
    ptrs, idx, nts, ets = tempo_graph(length, adm)
    st = np.zeros(N_CPU, dtype=np.int64)
    w, _ = orc.tempo_random_walk(ptrs, idx, nts, ets, st, np.full(N_CPU, 5, dtype=np.int64), 2, (0, 20),
                                 orc.rng_philox(0xE5, 1))
    rank = np.full(length + 1, -1)
    rank[adm + 1] = np.arange(adm.size)
    L.chi2_gof(np.bincount(rank[w[:, 1]], minlength=adm.size), L.one_slot_walk_law(adm.size), "oracle tempo walk")


def node2vec_graph(row):
    """start S = 0 -> hub H = 1 only; H's row of `row` entries: S once, vertices 2..9 (which have S in their rows:
    distance 1) twice each, the rest distance-2 vertices; so step 2 (prev = S, cur = H) sees all three cases"""
    near = list(range(2, 10))
    far = list(range(10, 10 + row - 1 - 2 * len(near)))
    n = far[-1] + 1
    rows = {0: [1], 1: sorted([0] + near * 2 + far)}
    for v in near:
        rows[v] = [0, 1]
    for v in far:
        rows[v] = [1]
    ptrs = np.zeros(n + 1, dtype=np.int64)
    ptrs[1:] = np.cumsum([len(rows[v]) for v in range(n)])
    col = np.concatenate([rows[v] for v in range(n)]).astype(np.int64)
    return ptrs, col, n


def test_oracle_node2vec_step_follows_the_exact_law():
    ptrs, col, n = node2vec_graph(100)
    w = orc.random_walk(ptrs, col, np.zeros(N_CPU, dtype=np.int64), 2, 0.5, 4.0, orc.rng_philox(0xE6, 1))
    assert np.all(w[:, 1] == 1)
    law = L.node2vec_step_law(ptrs, col, 1, 0, 0.5, 4.0)
    P = np.bincount(col[ptrs[1]:ptrs[2]], weights=law, minlength=n)
    L.chi2_gof(np.bincount(w[:, 2], minlength=n), P / P.sum(), "oracle node2vec step 2")


@pytest.mark.parametrize("bias", ["uniform", "linear", "exponential"])
def test_oracle_biased_step_follows_the_exact_law(bias):
    row = 65
    times = 5 + np.random.default_rng(2).permutation(row)                # distinct times >= the start time 5
    times[[0, np.argmin(times)]] = times[[np.argmin(times), 0]]          # candidate 0 weighs > 0 (else the reference panics)
    ptrs = np.zeros(row + 2, dtype=np.int64)
    ptrs[1:] = row
    idx = np.arange(1, row + 1, dtype=np.int64)
    w, _ = orc.biased_tempo_random_walk(ptrs, idx, np.full(row + 1, -1), times, np.zeros(N_CPU, dtype=np.int64),
                                        np.full(N_CPU, 5, dtype=np.int64), 2, bias, True, 1, orc.rng_philox(0xE7, 1))
    L.chi2_gof(np.bincount(w[:, 1] - 1, minlength=row), L.biased_step_law(times, 5, bias), "oracle biased " + bias)


def test_oracle_negative_item_follows_the_exact_law():
    size, tries = 1000, 3
    rs = np.random.default_rng(5)
    row = np.sort(rs.choice(size, size // 2, replace=False))
    ptrs = np.zeros(size + 1, dtype=np.int64)
    ptrs[1:] = row.size                                                  # vertex 0 holds the row
    B, k = N_CPU // 8, 8
    s, r, c, _ = orc.neg_homo(ptrs, row, (size, size), np.zeros(B, dtype=np.int64), k, tries, orc.rng_philox(0xE8, 1))
    got = np.bincount(s[c], minlength=size + 1)
    got[size] = B * k - c.size
    adm = np.ones(size, dtype=bool)
    adm[row] = False
    adm[0] = False
    L.chi2_gof(got, L.negative_item_law(size, adm, tries), "oracle negatives")


# ---------------------------------------------------------------- the typed samplers: hgt_sampling, budget_sampling
def test_hgt_budget_weights_and_layer_law_equal_enumeration():
    """a0's column b3 b1 b4, a1's b1 b5, a2's b2 b4 b6 b0: seven entries in first-contribution order, b1 and b4 with
    two contributions (scores by hand, hgt_sampling.rs:73,96); sample_from's loop enumerated over its accept and slot
    choices (weights score^2 as exact rationals of the f64 values)"""
    ptrs, idx = np.array([0, 3, 5, 9]), np.array([3, 1, 4, 1, 5, 2, 4, 6, 0])
    keys, w, _ = L.hgt_budget_weights([(ptrs, idx, [0, 1, 2])])
    assert keys.tolist() == [3, 1, 4, 5, 2, 6, 0]
    hand = [Fraction(1, 3), Fraction(1, 3) + Fraction(1, 2), Fraction(1, 3) + Fraction(1, 4), Fraction(1, 2),
            Fraction(1, 4), Fraction(1, 4), Fraction(1, 4)]
    assert np.allclose(w, [float(x * x) for x in hand], rtol=1e-15, atol=0)
    keys_s, w_s, _ = L.hgt_budget_weights([(ptrs, idx, [0, 1, 2])], sampled=[1, 6])     # :80 sampled ones are skipped
    assert keys_s.tolist() == [3, 4, 5, 2, 0] and np.allclose(w_s, w[[0, 2, 3, 4, 6]], rtol=0, atol=0)
    for k in (1, 2, 3):
        ref = law_weighted_loop(w, k)
        law = L.hgt_layer_law(w, k)
        M = _slot_marginals(ref, 7, k)
        for s in range(k):
            assert np.allclose(law.marginal(s), M[s], atol=1e-13, rtol=0)
        if k >= 2:
            edges = np.arange(k, 8)
            assert np.allclose(law.pair_table(edges), _binned_pair(_pair(ref, 7, 0, k - 1), law, edges), atol=1e-13, rtol=0)
    assert L.hgt_layer_law(w, 7) is None and L.hgt_layer_law(w, 9) is None            # n <= k: every entry, in order


def test_hgt_dead_prefix_law_equals_enumeration():
    """the dead-prefix builder at toy size: layer 0 takes its 3 entries, layer 1's 6 live entries get their weights from
    the b -> b columns of those 3 alone (recomputed here from the columns), and the law over them is the loop's"""
    g = L.hgt_dead_prefix_graph(3, 6, 1, fan=2)
    pb, ib = g["ptrs"]["b__s__b"], g["indices"]["b__s__b"]
    assert len(g["keys0"]) == 3 and len(g["keys"]) == 6 and not set(g["keys0"]) & set(g["keys"])
    score, order = {}, []
    for v in g["keys0"]:
        col = ib[pb[v]:pb[v + 1]]
        for u in col[:50]:
            if u in g["keys0"]:
                continue
            if u not in score:
                order.append(u)
            score[u] = score.get(u, Fraction(0)) + Fraction(1, min(len(col), 50))
    assert order == g["keys"].tolist()
    assert np.allclose(g["w"], [float(score[u] ** 2) for u in order], rtol=1e-14, atol=0)
    assert len(set(g["w"])) > 1
    for k in (1, 2):
        ref = law_weighted_loop(g["w"], k)
        law = L.hgt_layer_law(g["w"], k)
        M = _slot_marginals(ref, 6, k)
        for s in range(k):
            assert np.allclose(law.marginal(s), M[s], atol=1e-13, rtol=0)


def test_typed_builders_have_the_promised_shape():
    g = L.hgt_wide_graph(257, 357)
    P = g["ptrs"]["b__r__a"]
    lens = np.diff(P)
    assert lens.min() == 1 and lens.max() == 50 and g["w"].min() < 1e-3 and g["w"].max() > 4.0
    idx = g["indices"]["b__r__a"]
    assert np.bincount(idx).max() >= 3                                  # entries with several contributions
    assert all(len(set(idx[P[c]:P[c + 1]])) == lens[c] for c in range(lens.size))       # distinct inside a column
    assert np.array_equal(g["rank_of"][g["keys"]], np.arange(257)) and not np.array_equal(g["keys"], np.arange(257))
    for n, lengths in L.BUDGET_LISTS.items():
        assert L.budget_hub_graph(lengths)["n"] == n == sum(min(x, 50) for x in lengths)
    f = L.budget_hub_graph(L.BUDGET_FILTERED["lengths"], L.BUDGET_FILTERED["window"], 3)
    assert L.BUDGET_FILTERED["k"] < 40 < f["n"] < 110                   # a known, proper subset is admitted


def _hgt_oracle_ranks(g, quotas, N, seed):
    """N oracle calls (philox-mode, call id = outcome) -> [N, last quota] ranks of the last layer's samples"""
    hops, k = len(quotas), quotas[-1]
    ns = {"a": list(quotas), "b": list(quotas)}
    E = np.empty((N, k), dtype=np.int64)
    first = None
    for c in range(N):
        s = orc.hgt(g["node_types"], g["edge_types"], g["ptrs"], g["indices"], None, g["inputs"], None, ns, hops,
                    orc.rng_philox(seed, c))[0]["b"]
        if first is None:
            first = s[:len(s) - k].copy()
        assert len(s) == len(first) + k and np.array_equal(s[:len(first)], first)
        E[c] = g["rank_of"][s[len(first):]]
    return E, first


@pytest.mark.parametrize("k,n", [(2, 65), (5, 257)])
def test_oracle_hgt_sample_from_follows_the_exact_law(k, n):
    g = L.hgt_wide_graph(n, 100 + n)
    E, _ = _hgt_oracle_ranks(g, [k], N_CPU, 0xE9)
    L.check_reservoir(torch.from_numpy(E), L.hgt_layer_law(g["w"], k), "oracle hgt k=%d n=%d" % (k, n), zero_pos=None,
                      positions=[h for h in L.hgt_heavy_ranks(n) if h >= k] + [n - 1])


def test_oracle_hgt_dead_prefix_follows_the_exact_law():
    g = L.hgt_dead_prefix_graph(100, 300, 5)
    E, first = _hgt_oracle_ranks(g, [128, 7], N_CPU // 4, 0xEA)
    assert np.array_equal(first, g["keys0"])                            # layer 0: slot s holds entry s, no draw
    L.check_reservoir(torch.from_numpy(E), L.hgt_layer_law(g["w"], 7), "oracle hgt dead prefix", zero_pos=None)


@pytest.mark.parametrize("deg", [51, 65])
def test_oracle_hgt_edge_phase_follows_the_exact_law(deg):
    nt, et, P, I, inputs, hub_ptrs = L.hgt_edge_graph(deg, N_CPU)
    o = orc.hgt(nt, et, P, I, None, {"a": inputs}, None, {"a": []}, 0, orc.rng_philox(0xEB, 2))
    rows, cols, eidx = o[2]["a__r__a"], o[3]["a__r__a"], o[4]["a__r__a"]
    assert np.array_equal(cols, np.repeat(deg + np.arange(N_CPU), 50))  # 50 edges per hub, every source a sampled node
    E = eidx.reshape(N_CPU, 50) - hub_ptrs[:, None]
    assert np.array_equal(rows.reshape(N_CPU, 50), E)                   # the pool node's local id is its column position
    L.check_reservoir(torch.from_numpy(E), L.uniform_law(deg, 50), "oracle hgt edges deg=%d" % deg)


def _budget_oracle_ranks(g, k, N, seed, window=None):
    its = {"a": np.full(N, g["hub_ts"], dtype=np.int64)} if window is not None else None
    o = orc.budget(g["node_types"], g["edge_types"], g["ptrs"], g["indices"], g["row_ts"], {"a": np.zeros(N, dtype=np.int64)},
                   its, {"a": [k], "b": [k]}, 1, orc.rng_philox(seed, 4), window=window, forward=False, relative=False)
    assert len(o[0]["b"]) == N * k
    return o[0]["b"].reshape(N, k)


@pytest.mark.parametrize("n,k", [(65, 5), (65, 64), (150, 5), (150, 50)])
def test_oracle_budget_sample_follows_the_exact_law(n, k):
    g = L.budget_hub_graph(L.BUDGET_LISTS[n])
    E = _budget_oracle_ranks(g, k, N_CPU, 0xEC)
    L.check_reservoir(torch.from_numpy(E), L.uniform_law(n, k), "oracle budget k=%d n=%d" % (k, n))


def test_oracle_filtered_budget_follows_the_law_on_the_admitted_subsequence():
    f = L.BUDGET_FILTERED
    g = L.budget_hub_graph(f["lengths"], f["window"], 3)
    E = _budget_oracle_ranks(g, f["k"], N_CPU, 0xED, window=f["window"])
    L.check_reservoir(torch.from_numpy(E), L.uniform_law(g["n"], f["k"]), "oracle budget filtered")


# ---------------------------------------------------------------- power against named wrong laws, negative controls
def _reject(counts, probs):
    with pytest.raises(AssertionError):
        L.chi2_gof(counts, probs, "wrong law")


def test_power_uniform_without_the_quirk():
    """j from 0..=i instead of 0..i: at the GPU file's k = 16, n = 64 the own-position marginal moves 15/63 -> 16/64"""
    n, k = 64, 16
    N = n_outcomes(k)
    right, wrong = L.uniform_law(n, k).marginal(0), L.uniform_law(n, k, quirk=False).marginal(0)
    assert L.power(wrong, right, N) >= 0.999
    _reject(np.random.default_rng(1).multinomial(N, wrong), right)
    L.chi2_gof(np.random.default_rng(1).multinomial(N, right), right, "right law")
    n, k = 2, 1                                                          # k = 1, n = 2: the quirk always takes candidate 1
    assert L.power(L.uniform_law(n, k, quirk=False).marginal(0), L.uniform_law(n, k).marginal(0), n_outcomes(1)) >= 0.999


def test_power_weighted_with_the_previous_running_sum():
    n, k = 5000, 5
    w = weights_wide(n, n + k)
    N = n_outcomes(k)
    right, wrong = L.weighted_law(w, k).marginal(0), L.weighted_law(w, k, shift=True).marginal(0)
    assert L.power(wrong, right, N) >= 0.999
    _reject(np.random.default_rng(2).multinomial(N, wrong), right)
    L.chi2_gof(np.random.default_rng(2).multinomial(N, right), right, "right law")


def test_power_chunked_walk_step_off_by_one():
    adm = walk_row(5000, "edges")
    right, wrong = L.one_slot_walk_law(adm.size), L.one_slot_chunked_law(adm, off_by_one=True)
    assert L.power(wrong, right, N_WALK) >= 0.999
    _reject(np.random.default_rng(3).multinomial(N_WALK, wrong), right)
    L.chi2_gof(np.random.default_rng(3).multinomial(N_WALK, right), right, "right law")


def test_power_node2vec_p_q_swapped():
    ptrs, col, n = node2vec_graph(100)
    right, wrong = L.node2vec_step_law(ptrs, col, 1, 0, 0.5, 4.0), L.node2vec_step_law(ptrs, col, 1, 0, 4.0, 0.5)
    assert L.power(wrong, right, N_WALK) >= 0.999
    _reject(np.random.default_rng(4).multinomial(N_WALK, wrong), right)


def test_power_negative_tries_off_by_one():
    size = 1000
    adm = np.ones(size, dtype=bool)
    adm[: size // 2] = False
    right, wrong = L.negative_item_law(size, adm, 3), L.negative_item_law(size, adm, 2)
    assert L.power(wrong, right, N_NEG) >= 0.999
    _reject(np.random.default_rng(5).multinomial(N_NEG, wrong), right)


def test_power_of_a_biased_slot_at_k_129():
    """slot 128 of 129 holding the 64 positions of one chunk 20 % too often"""
    n, k = 1000, 129
    right = L.uniform_law(n, k).marginal(128)
    wrong = right.copy()
    wrong[192:256] *= 1.2
    wrong[k:] *= (1 - wrong[128]) / wrong[k:].sum()
    assert L.power(wrong, right, n_outcomes(k)) >= 0.999


# ---------------------------------------------------------------- the typed samplers' sample sizes
def _hgt_wrongs(w, k, n):
    """named wrong laws (a) weights score instead of score^2 and, for n <= 4097, (b) the previous candidate's running sum"""
    wrongs = [L.weighted_law(np.sqrt(w), k)]
    if n <= 4097:
        wrongs.append(L.weighted_law(w, k, shift=True))
    return wrongs


@pytest.mark.parametrize("k,n", L.HGT_CASES + L.HGT_LARGE)
def test_power_hgt_score_not_squared_and_previous_running_sum(k, n):
    g = L.hgt_wide_graph(n, 100 + n)
    right = L.hgt_layer_law(g["w"], k)
    N = L.hgt_outcomes(k, n)
    slots, positions = L.hgt_slots(k), L.hgt_positions(k, n)
    for wrong in _hgt_wrongs(g["w"], k, n):
        assert L.reservoir_power(wrong, right, N, slots, positions) >= 0.999


def test_power_hgt_surface_loop():
    """the (2, 65) case through single calls of the operator surface: HGT_SURFACE_CALLS outcomes reach the bound too"""
    g = L.hgt_wide_graph(65, 165)
    right = L.hgt_layer_law(g["w"], 2)
    for wrong in _hgt_wrongs(g["w"], 2, 65):
        assert L.reservoir_power(wrong, right, L.HGT_SURFACE_CALLS, L.hgt_slots(2), L.hgt_positions(2, 65)) >= 0.999


def test_power_hgt_dead_entries_kept_alive():
    """(c): the law over all n0 + n1 entries, the dead ones with their old weights -- it samples dead entries, which the
    right law (ranks among the live ones) holds at probability zero"""
    n0, n1, k = L.HGT_DEAD
    g = L.hgt_dead_prefix_graph(n0, n1, 5)
    right, wrong = L.hgt_layer_law(g["w"], k), L.weighted_law(np.concatenate([g["w_dead"], g["w"]]), k)
    N = L.hgt_outcomes(k, n1)
    for s in (0, k - 1):
        live = np.concatenate([np.zeros(n0), right.marginal(s)])
        assert L.power(wrong.marginal(s), live, N) >= 0.999
    for w2 in _hgt_wrongs(g["w"], k, n1):                               # (a) and (b) hold for this case as well
        assert L.reservoir_power(w2, right, N, L.hgt_slots(k), L.hgt_positions(k, n1)) >= 0.999


def test_power_budget_and_edge_phase_without_the_quirk():
    """(d) uniform_law(n, k, quirk=False).  The quirk moves a slot's own-position marginal from (k-1)/(n-1) to k/n and
    every later position from 1/(n-1) to 1/n: the noncentrality per outcome is about (n-k)^2 / (n^2 (n-1) (k-1)) + 1/n^2
    and fades with growing k and n, so the outcome counts grow to 2^25 (budget n = 800 at k = 63, 64; the edge phase, whose k
    is 50, at deg 1000).  Every budget case of BUDGET_LISTS x BUDGET_K and the edge phase up to deg 1000 reach the bound.
    At deg 70 000 no count does (1/69 999 against 1/70 000: more than 10^9 outcomes); that case runs EDGE_OUTCOMES[70000]
    outcomes against the law all the same, and what it can see is an error in the width of a position -- the wrong law below
    cuts positions to 16 bits."""
    assert {(n, k) for n, k, _ in L.BUDGET_CASES} == {(n, k) for n in L.BUDGET_LISTS for k in L.BUDGET_K if k < n}
    for n, k, N in L.BUDGET_CASES:
        assert L.reservoir_power(L.uniform_law(n, k, quirk=False), L.uniform_law(n, k), N) >= 0.999, (n, k, N)
    f = L.BUDGET_FILTERED
    n = L.budget_hub_graph(f["lengths"], f["window"], 3)["n"]
    assert L.reservoir_power(L.uniform_law(n, f["k"], quirk=False), L.uniform_law(n, f["k"]), L.BUDGET_FILTERED_OUTCOMES) >= 0.999
    for deg in (51, 64, 65, 1000):
        assert L.reservoir_power(L.uniform_law(deg, 50, quirk=False), L.uniform_law(deg, 50), L.EDGE_OUTCOMES[deg]) >= 0.999, deg
    right = L.uniform_law(70000, 50).marginal(49)
    wrong = right.copy()
    wrong[1 << 16:] = 0.0                                               # a position cut to 16 bits: nothing past 65 535
    wrong[50:] *= (1 - wrong[49]) / wrong[50:].sum()
    assert L.power(wrong, right, L.EDGE_OUTCOMES[70000]) >= 0.999


# ---------------------------------------------------------------- link seed rows, skip-gram negatives, consecutive steps
# closed forms == enumeration of the sequential loops
def _edge_sets(ptrs, indices):
    return {(int(s), d) for d in range(len(ptrs) - 1) for s in indices[ptrs[d]:ptrs[d + 1]]}


def _enumerate_kept_attempt(cells, accepted, tries):
    """negative_sampling.rs:33-43 with tg_link_seeds' fixed-shape rule, every sequence of `tries` candidates equally
    likely: the first accepted one is kept, else the last; tries = 1 keeps attempt 0 unchecked.
    -> ({cell: probability}, P(unverified)) in rationals"""
    P, unv = {c: Fraction(0) for c in cells}, Fraction(0)
    w = Fraction(1, len(cells) ** tries)
    for seq in product(cells, repeat=tries):
        kept = seq[0] if tries == 1 else next((c for c in seq if accepted(c)), None)
        if kept is None:
            kept, unv = seq[-1], unv + w
        P[kept] += w
    return P, unv


TOY_RELATIONS = {                                                        # name -> (n_src, n_dst, edges s -> d, same_type)
    "square": (4, 4, [(0, 1), (1, 0), (2, 1), (3, 3), (0, 2), (3, 0)], True),        # one self-loop, 0 <-> 1 both ways
    "rect": (3, 4, [(0, 0), (1, 0), (2, 3), (0, 2), (1, 1)], False),                 # equal ids (0, 0), (1, 1) are edges
    "full-row": (4, 4, [(2, 0), (2, 1), (2, 3), (0, 1)], True),                      # source 2 has no admissible d
}


@pytest.mark.parametrize("tries", [1, 2, 3])
@pytest.mark.parametrize("name", list(TOY_RELATIONS))
def test_link_laws_equal_enumeration(name, tries):
    import helpers_link as hl
    n_src, n_dst, edges, same = TOY_RELATIONS[name]
    ptrs, idx = hl.csc_of(edges, n_dst)
    E = _edge_sets(ptrs, idx)
    assert E == set(edges)
    accepted = lambda c: c not in E and not (same and c[0] == c[1])      # !has_edge(v, w) && v != w
    adm = L.link_admissible(ptrs, idx, n_src, same)
    cells = [(s, d) for s in range(n_src) for d in range(n_dst)]
    assert [bool(adm[c]) for c in cells] == [accepted(c) for c in cells]
    P, unv = _enumerate_kept_attempt(cells, accepted, tries)
    assert sum(P.values()) == 1
    assert np.allclose(L.link_binary_law(n_src, n_dst, adm, tries), [float(P[c]) for c in cells], atol=1e-15, rtol=0)
    assert np.allclose(L.link_unverified_law(adm, tries), [float(1 - unv), float(unv)], atol=1e-15, rtol=0)
    for s in range(n_src):                                               # triplet: the anchor's row alone
        row = [(s, d) for d in range(n_dst)]
        P, unv = _enumerate_kept_attempt(row, accepted, tries)
        assert np.allclose(L.link_triplet_law(n_dst, adm[s], tries), [float(P[c]) for c in row], atol=1e-15, rtol=0)
        assert np.allclose(L.link_unverified_law(adm[s], tries), [float(1 - unv), float(unv)], atol=1e-15, rtol=0)
    if tries > 1 and adm.any():                                          # the named wrong law keeps accepted attempts only
        keep = {c: p for c, p in _enumerate_kept_attempt(cells, accepted, tries)[0].items() if accepted(c)}
        tot = sum(keep.values())
        assert np.allclose(L.link_binary_law(n_src, n_dst, adm, tries, drop_last=True),
                           [float(keep.get(c, 0) / tot) for c in cells], atol=1e-15, rtol=0)


def _enumerate_chain(step, start, m):
    """the walk loop of random_walk.rs:43-71, every choice of every step enumerated: step(prev, cur) -> [(next,
    probability)], empty at a dead end (`break`: the later columns keep their padding).  -> {path: probability}, None = ended"""
    out = Counter()

    def go(prev, cur, path, pr):
        if len(path) == m:
            out[path] += pr
            return
        nxt = step(prev, cur) if cur is not None else []
        if not nxt:
            out[path + (None,) * (m - len(path))] += pr
            return
        for v, t in nxt:
            go(cur, v, path + (v,), pr * t)
    go(-1, start, (), Fraction(1))
    return out


def _chain_equals(P, exact):
    sizes = [s - 1 for s in P.shape]
    Q = np.zeros(P.shape)
    for path, pr in exact.items():
        Q[tuple(s if v is None else v for v, s in zip(path, sizes))] += float(pr)
    assert sum(exact.values()) == 1
    assert np.allclose(P, Q, atol=1e-14, rtol=0) and np.array_equal(P == 0, Q == 0)


TOY_ROWS = {0: [1, 2, 3], 1: [0, 2], 2: [3, 3, 0], 3: []}               # a multiplicity (2 -> 3 twice) and a dead end


def _toy_csr(rows, n):
    ptrs = np.concatenate([[0], np.cumsum([len(rows[v]) for v in range(n)])]).astype(np.int64)
    return ptrs, np.array([u for v in range(n) for u in rows[v]], dtype=np.int64)


@pytest.mark.parametrize("m", [2, 3])
def test_chain_law_of_uniform_steps_equals_enumeration(m):
    ptrs, col = _toy_csr(TOY_ROWS, 4)
    uniform = lambda prev, cur: [(v, Fraction(1, len(TOY_ROWS[cur]))) for v in TOY_ROWS[cur]]   # neighbors[gen_range(0..len)]
    for start in (0, 1):
        P = L.chain_law([L.csr_step(ptrs, col, 4)] * m, start)
        assert P.shape == (5,) * m
        _chain_equals(P, _enumerate_chain(uniform, start, m))
    assert L.chain_law([L.csr_step(ptrs, col, 4)] * m, 3, sizes=(4,) * m)[(4,) * m] == 1.0          # a start without out-edges


def test_chain_law_of_node2vec_steps_equals_enumeration():
    """acceptance weights as exact rationals of the f32 values; the rejection loop's law is weight / sum (shown above);
    step 1 has prev = -1, which is no vertex: every proposal has prob2"""
    rows = {0: [1, 2], 1: [0, 2, 3], 2: [0, 1], 3: [1, 0]}                # 3 -> 0 is one-way: has_edge(3, 0), not (0, 3)
    ptrs, col = _toy_csr(rows, 4)
    p, q = 0.5, 4.0
    p0, p1, p2 = (Fraction(x) for x in L.node2vec_probs(p, q))

    def step(prev, cur):
        acc = [p0 if v == prev else p1 if prev in rows.get(v, []) else p2 for v in rows[cur]]
        return [(v, a / sum(acc)) for v, a in zip(rows[cur], acc)]
    exact = _enumerate_chain(step, 0, 3)
    _chain_equals(L.chain_law([L.node2vec_step(ptrs, col, 4, p, q)] * 3, 0), exact)
    assert exact[(1, 3, 0)] != exact[(1, 3, 1)]                          # from 0 over 1 to 3: back to 1 (prob0) or on to 0 (prob1)
    swapped = L.chain_law([L.node2vec_step(ptrs, col, 4, p, q, swap_lookup=True)] * 3, 0)
    assert not np.allclose(swapped, L.chain_law([L.node2vec_step(ptrs, col, 4, p, q)] * 3, 0))
    first = L.chain_law([L.node2vec_step(ptrs, col, 4, p, q)], 0)
    assert np.allclose(first, [0, 0.5, 0.5, 0, 0])                       # step 1 is uniform


def test_chain_law_of_temporal_steps_equals_enumeration():
    """the one-slot reservoir (the literal loop with k = 1, enumerated) at every step of the complete graph on 4 vertices,
    every edge admissible; as ranks the joint law is one_slot_walk_law(3) x itself"""
    ptrs, col = L.complete_csr(4)
    rows = {v: col[ptrs[v]:ptrs[v + 1]].tolist() for v in range(4)}
    lit = law_reference_loop(3, 1)
    step = lambda prev, cur: [(rows[cur][c], lit[(c,)]) for c in range(3) if lit.get((c,), 0)]
    P = L.chain_law([L.csr_step(ptrs, col, 4, L.one_slot_walk_law)] * 2, 0)
    _chain_equals(P, _enumerate_chain(step, 0, 2))
    R = np.zeros((3, 3))
    for x1 in range(4):
        for x2 in range(4):
            if P[x1, x2]:
                R[rows[0].index(x1), rows[x1].index(x2)] += P[x1, x2]
    assert np.allclose(R, np.outer(L.one_slot_walk_law(3), L.one_slot_walk_law(3)), atol=1e-15, rtol=0)


def test_metapath_chain_with_a_sink_equals_enumeration():
    (pa, ca), (pb, cb) = L.metapath_graph()
    rows = [{a: ca[pa[a]:pa[a + 1]].tolist() for a in range(5)}, {b: cb[pb[b]:pb[b + 1]].tolist() for b in range(7)}]
    assert rows[1][L.MP_SINK] == [] and all(rows[0][a] for a in range(5)) and sum(1 for b in range(7) if not rows[1][b]) == 1
    exact = Counter()
    for x1 in rows[0][0]:                                                # csrs[l mod 2]: A -> B, B -> A, A -> B
        t1 = Fraction(1, len(rows[0][0]))
        if not rows[1][x1]:
            exact[(x1, None, None)] += t1
            continue
        for x2 in rows[1][x1]:
            t2 = t1 / len(rows[1][x1])
            for x3 in rows[0][x2]:
                exact[(x1, x2, x3)] += t2 / len(rows[0][x2])
    laws = [L.csr_step(pa, ca, 7), L.csr_step(pb, cb, 5), L.csr_step(pa, ca, 7)]
    P = L.chain_law(laws, 0, sizes=(7, 5, 7))
    _chain_equals(P, exact)
    assert P[L.MP_SINK, 5, 7] == pytest.approx(1 / 5) and P[L.MP_SINK, :5, :].sum() == 0   # ended: padding in every later column


def test_pair_laws_equal_enumeration():
    for n_a, n_b in ((3, 2), (5, 7), (7, 7)):
        D = 4 * n_a * n_b                                                # a draw of log2(D) bits, every value once
        got = np.zeros((n_a, n_b))
        for a in range(D):
            got[a * n_a // D, a * n_b // D] += 1.0 / D
        assert np.allclose(L.shared_draw_pair_law(n_a, n_b), got.ravel(), atol=1e-15, rtol=0)
        assert np.allclose(L.product_uniform_law(n_a, n_b), np.outer(np.full(n_a, 1 / n_a), np.full(n_b, 1 / n_b)).ravel())
    ptrs, col = _toy_csr(TOY_ROWS, 4)                                    # one draw for every step: rows of 3, 2, 3, 0 entries
    P = L.shared_draw_chain_law([(ptrs, col)], 0, 2, (4, 4))
    exact = Counter()
    for j in range(6):
        x1 = TOY_ROWS[0][j * 3 // 6]
        exact[(x1, TOY_ROWS[x1][j * len(TOY_ROWS[x1]) // 6] if TOY_ROWS[x1] else None)] += Fraction(1, 6)
    _chain_equals(P, exact)


# ---------------------------------------------------------------- the NumPy models of the batch kernels against the laws
def _neg_pairs(rows, E, K, mode):
    import helpers_link as hl
    pr = hl.pairs(rows, E, K, mode)
    return pr[:, 0, E:], pr[:, 1, E:]                                    # [G, K E] negative sources and destinations


@pytest.mark.parametrize("tries", [1, 2])
def test_link_model_binary_follows_the_exact_law(tries):
    import helpers_link as hl
    n = 13
    ptrs, idx, _ = L.link_graph(n, n, 0.5, 31)
    adm = L.link_admissible(ptrs, idx, n, True)
    G, E, K = 4, 25, 60
    src, dst = np.zeros((G, E), dtype=np.int64), np.ones((G, E), dtype=np.int64)
    rows, unv = hl.seed_rows(ptrs, idx, src, dst, K, hl.BINARY, tries, 0xF1, 5, n)
    s, d = _neg_pairs(rows, E, K, hl.BINARY)
    assert L.chi2_gof(np.bincount((s * n + d).ravel(), minlength=n * n), L.link_binary_law(n, n, adm, tries),
                      "link model binary")[1] > 0
    bad = int((~adm[s, d]).sum())
    assert int(unv.sum()) == (bad if tries > 1 else 0)
    L.chi2_gof([G * E * K - int(unv.sum()), int(unv.sum())], L.link_unverified_law(adm, tries), "link model unverified")


def test_link_model_triplet_follows_the_exact_law():
    import helpers_link as hl
    n, tries = 13, 3
    ptrs, idx, M = L.link_graph(n, n, 0.5, 32)
    adm = L.link_admissible(ptrs, idx, n, True)
    G, E, K = 4, 10, 50
    anchors = [1, 4, 7, 10]
    src = np.repeat(np.array(anchors, dtype=np.int64)[:, None], E, axis=1)
    rows, unv = hl.seed_rows(ptrs, idx, src, np.zeros_like(src), K, hl.TRIPLET, tries, 0xF2, 5, n)
    s, d = _neg_pairs(rows, E, K, hl.TRIPLET)
    for g, a in enumerate(anchors):
        assert np.all(s[g] == a)
        L.chi2_gof(np.bincount(d[g], minlength=n), L.link_triplet_law(n, adm[a], tries), "link model triplet anchor %d" % a)
        assert int(unv[g]) == int((~adm[a, d[g]]).sum())
        L.chi2_gof([E * K - int(unv[g]), int(unv[g])], L.link_unverified_law(adm[a], tries), "link model unverified")


@pytest.mark.parametrize("same_type", [0, 1])
def test_typed_link_model_follows_the_exact_law(same_type):
    import helpers_link as hl
    import helpers_link_typed as hlt
    (n_src, n_dst), tries = ((7, 7) if same_type else (5, 7)), 2
    ptrs, idx, M = L.link_graph(n_src, n_dst, 0.5, 33 + same_type)
    adm = L.link_admissible(ptrs, idx, n_src, same_type)
    assert same_type or (adm[3, 3] and not adm[0, 0] and M[0, 0])                    # equal ids of two types: eligible unless an edge
    G, E, K = 2, 25, 60
    src, dst = np.zeros((G, E), dtype=np.int64), np.ones((G, E), dtype=np.int64)
    srows, drows, unv = hlt.seed_rows(ptrs, idx, src, dst, K, hlt.BINARY, tries, 0xF3, 5, n_src, n_dst, same_type)
    s, d = srows[:, E:], drows[:, E:]
    assert s.max() < n_src and d.max() < n_dst and s.min() >= 0 and d.min() >= 0
    got = np.bincount((s * n_dst + d).ravel(), minlength=n_src * n_dst)
    L.chi2_gof(got, L.link_binary_law(n_src, n_dst, adm, tries), "typed link model same_type=%d" % same_type)
    if not same_type:
        assert got[3 * n_dst + 3] > 0
    assert int(unv.sum()) == int((~adm[s, d]).sum())
    if same_type:                                                        # the homogeneous model, word for word
        rows, unv1 = hl.seed_rows(ptrs, idx, src, dst, K, hl.BINARY, tries, 0xF3, 5, n_src)
        assert np.array_equal(hlt.joined(srows, drows), rows) and np.array_equal(unv, unv1)


def test_skipgram_negative_model_follows_the_exact_law():
    import helpers_skipgram as hs
    n, Lc, B, R, K = 7, 3, 50, 4, 10
    seeds = np.arange(B, dtype=np.int64) % n
    x = [hs.negatives(0xF4, 9 + g, seeds, R, K, Lc, n) for g in range(2)]
    for g in range(2):
        assert np.array_equal(x[g][:, 0], np.tile(seeds, R * K))
        for m in (1, 2):
            L.chi2_gof(np.bincount(x[g][:, m], minlength=n), np.full(n, 1 / n), "negative model word %d" % m)
        L.chi2_gof(np.bincount(x[g][:, 1] * n + x[g][:, 2], minlength=n * n), L.product_uniform_law(n, n), "words 1, 2")
    both = np.concatenate([x[0][:, m] * n + x[1][:, m] for m in (1, 2)])
    L.chi2_gof(np.bincount(both, minlength=n * n), L.product_uniform_law(n, n), "negative model, call ids c and c + 1")


def test_metapath_model_follows_the_exact_laws():
    import helpers_metapath as hm
    csrs = L.metapath_graph()
    (pa, ca), (pb, cb) = csrs
    nA, nB = L.MP_COUNTS
    W = 3000
    w = hm.walks(0xF5, 3, csrs, [0, 1], [1, 0], np.zeros(W // 4, dtype=np.int64), 4, 3)
    assert w.shape == (W, 4) and np.all(w[:, 0] == 0)
    sizes = (nB, nA, nB)
    cat = np.zeros(W, dtype=np.int64)
    for c, s in enumerate(sizes):
        x = np.where(w[:, c + 1] < 0, s, w[:, c + 1])
        assert np.all((x >= 0) & (x <= s))
        cat = cat * (s + 1) + x
    P = L.chain_law([L.csr_step(pa, ca, nB), L.csr_step(pb, cb, nA), L.csr_step(pa, ca, nB)], 0, sizes=sizes)
    assert L.chi2_gof(np.bincount(cat, minlength=P.size), P.ravel(), "metapath model walks")[1] > 0
    U = 2000
    x = hm.negatives(0xF5, 3, [0, 1], [1, 0], np.zeros(U // 4, dtype=np.int64), 2, 2, 3, [nA, nB])
    assert x.shape == (U, 3) and x[:, 1].max() < nB and x[:, 2].max() < nA
    L.chi2_gof(np.bincount(x[:, 1] * nA + x[:, 2], minlength=nA * nB), L.product_uniform_law(nB, nA), "metapath model negatives")


# ---------------------------------------------------------------- power at the sample sizes of test_gpu_exact_laws_batches.py
def _show(wrong, right, N, seed):
    """the file's demonstration: a multinomial draw from the wrong law is rejected, one from the right law is not"""
    _reject(np.random.default_rng(seed).multinomial(N, wrong), right)
    L.chi2_gof(np.random.default_rng(seed).multinomial(N, right), right, "right law")


def link_wrong_laws(M, ptrs, idx, n_src, n_dst, same_type, tries, row=None):
    """name -> wrong law of one negative of the relation M (row: the triplet anchor), for every named error that exists at
    this configuration"""
    adm = L.link_admissible(ptrs, idx, n_src, same_type)
    law = (lambda a, t, **kw: L.link_binary_law(n_src, n_dst, a, t, **kw)) if row is None else \
        (lambda a, t, **kw: L.link_triplet_law(n_dst, a[row], t, **kw))
    wrong = {"one attempt too many": law(adm, tries + 1)}
    if tries > 1:
        wrong["one attempt too few"] = law(adm, tries - 1)
        if (adm if row is None else adm[row]).any():
            wrong["the last attempt dropped"] = law(adm, tries, drop_last=True)
        flipped = ~M if same_type else ~M & ~np.eye(n_src, n_dst, dtype=bool)
        wrong["s == d %s" % ("not rejected within one type" if same_type else "rejected across two types")] = law(flipped, tries)
        if n_src == n_dst:
            back = ~M.T
            if same_type:
                back = back & ~np.eye(n_src, dtype=bool)
            wrong["look-up direction swapped"] = law(back, tries)
    return wrong


def _link_power_cases():
    n = L.LINK_N
    for density in L.LINK_DENSITIES:
        for tries in L.LINK_TRIES:
            yield "homo", n, n, 1, density, tries
            yield "typed", L.LINK_TYPED[0], L.LINK_TYPED[1], 0, density, tries


@pytest.mark.parametrize("kind,n_src,n_dst,same,density,tries", list(_link_power_cases()))
def test_power_link_seed_laws(kind, n_src, n_dst, same, density, tries):
    ptrs, idx, M = L.link_graph(n_src, n_dst, density, L.link_seed(kind, density))
    adm = L.link_admissible(ptrs, idx, n_src, same)
    right = L.link_binary_law(n_src, n_dst, adm, tries)
    for name, wrong in link_wrong_laws(M, ptrs, idx, n_src, n_dst, same, tries).items():
        assert L.link_power(wrong, right, adm, N_NEG) >= 0.999, (name, L.link_power(wrong, right, adm, N_NEG))
    if tries == 2:
        for name, wrong in link_wrong_laws(M, ptrs, idx, n_src, n_dst, same, tries).items():
            _show(wrong, right, N_NEG, 11)
    N_a = L.LINK_TRIPLET_LAUNCHES * N_NEG // L.LINK_ANCHORS              # triplet: every anchor's row law at its own N
    for a in L.link_anchors(M):
        right = L.link_triplet_law(n_dst, adm[a], tries)
        for name, wrong in link_wrong_laws(M, ptrs, idx, n_src, n_dst, same, tries, row=a).items():
            if np.allclose(wrong, right, atol=1e-15, rtol=0):
                continue                                                 # the error does not touch this anchor's row
            assert L.link_power(wrong, right, adm[a], N_a) >= 0.999, (name, a, L.link_power(wrong, right, adm[a], N_a))
    if tries > 1:                                                        # the unverified total against an attempt more or fewer
        for t in (tries - 1, tries + 1):
            if t > 1:
                assert L.power(L.link_unverified_law(adm, t), L.link_unverified_law(adm, tries), N_NEG) >= 0.999


def _walk_chain(name):
    """-> (right law, {name: wrong law}) of the walk configurations of the GPU file"""
    m = L.WALK_STEPS
    if name == "complete":
        ptrs, col = L.complete_csr(7)
        right = L.chain_law([L.csr_step(ptrs, col, 7)] * m, 0)
        return right, {"steps share one draw": L.shared_draw_chain_law([(ptrs, col)], 0, m, (7,) * m)}
    if name == "wedge":
        ptrs, col, n = L.wedge_graph()
        mk = lambda p, q, **kw: L.chain_law([L.node2vec_step(ptrs, col, n, p, q, **kw)] * m, 0, sizes=(n,) * m)
        return mk(0.5, 4.0), {"p and q swapped": mk(4.0, 0.5), "prev ignored": mk(1.0, 1.0),
                              "look-up direction swapped": mk(0.5, 4.0, swap_lookup=True)}
    if name == "metapath":
        (pa, ca), (pb, cb) = L.metapath_graph()
        nA, nB = L.MP_COUNTS
        right = L.chain_law([L.csr_step(pa, ca, nB), L.csr_step(pb, cb, nA), L.csr_step(pa, ca, nB)], 0, sizes=(nB, nA, nB))
        return right, {"steps share one draw": L.shared_draw_chain_law([(pa, ca), (pb, cb)], 0, m, (nB, nA, nB))}
    ptrs, col = L.complete_csr(7)                                        # temporal: two steps, the rank of step 2 = step 1's
    step = L.csr_step(ptrs, col, 7, L.one_slot_walk_law)
    right = L.chain_law([step] * 2, 0)
    wrong = np.zeros_like(right)
    for r, pr in enumerate(L.one_slot_walk_law(6)):
        x1 = col[ptrs[0] + r]
        wrong[x1, col[ptrs[x1] + r]] += pr
    return right, {"steps share one draw": wrong}


@pytest.mark.parametrize("name", ["complete", "wedge", "metapath", "temporal"])
def test_power_consecutive_steps(name):
    right, wrongs = _walk_chain(name)
    assert abs(right.sum() - 1) < 1e-12
    for what, wrong in wrongs.items():
        assert abs(wrong.sum() - 1) < 1e-12
        assert L.power(wrong.ravel(), right.ravel(), N_WALK) >= 0.999, what
        _show(wrong.ravel(), right.ravel(), N_WALK, 12)


def test_power_negative_words_sharing_one_draw():
    """two words from one draw (columns m and m + 1, mini-batches g and g + 1, launches, or the walk's and the negatives'
    stream) at the smallest N any of those pair tests counts"""
    B, R, K, G, T = L.NEG_SHAPE
    U = R * K * B
    assert G * U * T == N_NEG
    N = U * T                                                            # one pair of mini-batches, every (u, m)
    n = L.NEG_NODES
    for a, b in ((n, n), L.NEG_MP_COUNTS, L.NEG_MP_COUNTS[::-1]):
        right, wrong = L.product_uniform_law(a, b), L.shared_draw_pair_law(a, b)
        assert L.power(wrong, right, N) >= 0.999 and L.power(wrong, right, U) >= 0.999
        _show(wrong, right, U, 13)
    for a, b in ((6, n), (3, n), (5, n), (5, 7)):                        # walker w's x_1 (a rank of its start's row) and word 1 of
        assert L.power(L.shared_draw_pair_law(a, b), L.product_uniform_law(a, b), N_WALK) >= 0.999   # its negative row
    short = np.concatenate([np.full(17, 1 / 17), np.zeros(n - 17)])      # a word bounded by the other type's count
    assert L.power(short, np.full(n, 1 / n), G * U) >= 0.999
