"""Exact output laws of the reference's samplers, in closed form (f64), and a one-sample goodness-of-fit test.

Every law here is derived from the reference's sequential algorithm, quirks included (src/utils/sampling.rs,
src/algo/random_walk.rs, src/algo/negative_sampling.rs), never from the counter-addressed restatements the kernels and
the oracle share: a test against these laws sees an error the two would have in common.

Reservoir laws (uniform without replacement, weighted).  Both loops fill slots 0..k-1 with candidates 0..k-1, then
let each later candidate i overwrite ONE slot, chosen uniformly, with some probability; the chance that candidate i
writes a given slot is

    uniform   a_i = 1 / i                  (j drawn from 0..i, sampling.rs:19 -- the quirk: not 0..=i)
    weighted  a_i = w_i / (k * W_i)        (W_i = w_0 + ... + w_i, sampling.rs:47-51)

and a slot's final content is the last candidate that wrote it.  So, with C1 / S1 the prefix / suffix sums of
log(1 - a_i) and S2 the suffix sums of log(1 - 2 a_i) over i >= k:

    P(slot s = s)               = exp(S1[k])
    P(slot s = p), p >= k       = a_p exp(S1[p+1])
    P(slot s = p, slot t = q)   = a_p a_q exp(C1[q] - C1[p+1] + S2[q+1])       k <= p < q (either slot order)
    P(slot s = s, slot t = q)   = a_q exp(C1[q] + S2[q+1])
    P(slot s = s, slot t = t)   = exp(S2[k])

and every other position (p < k, p != s; a zero-weight candidate p >= k) has probability exactly 0.  For the uniform
loop these give the textbook values: (k-1)/(n-1) for the own position, 1/(n-1) for each later one, 1/((n-1)(n-2)) for
two later positions.

Batch kernels (link seed rows, skip-gram negatives, consecutive walk steps): their laws are stated where they are defined
below -- the rejection loop of negative_sampling.rs with the last attempt kept (link_binary_law, link_triplet_law,
link_unverified_law), PyG's randint per column (product_uniform_law) and the product of random_walk.rs' per-step laws with
an absorbing `ended` category (chain_law).

The test: chi-square goodness of fit of observed counts against such a law, categories pooled in order into bins of
expected count >= 20, every structural zero asserted exactly (count == 0), rejection at p < 1e-6."""
import numpy as np
from scipy import stats

ALPHA = 1e-6
MIN_EXPECTED = 20.0


# ---------------------------------------------------------------- the statistic
def pool(probs, N, min_expected=MIN_EXPECTED):
    """Bin id of every category of positive probability (pooled in order so that each bin expects >= min_expected of N
    outcomes; a short remainder joins the last bin), -1 for the structural zeros.  -> (bin id per category, n_bins)"""
    probs = np.asarray(probs, dtype=np.float64)
    pos = np.flatnonzero(probs > 0)
    ids = np.full(probs.size, -1, dtype=np.int64)
    run = np.cumsum(probs[pos] * N)
    ends = []                                   # greedy: a bin closes at the first category that brings it to the bound
    i, base = 0, 0.0
    while i < run.size:
        j = int(np.searchsorted(run, base + min_expected * (1 - 1e-12), side="left"))
        if j >= run.size:
            break
        ends.append(j + 1)
        base, i = run[j], j + 1
    if not ends:
        ends = [run.size]
    ends[-1] = run.size                         # a short remainder joins the last bin
    b = np.zeros(run.size, dtype=np.int64)
    b[np.asarray(ends[:-1], dtype=np.int64)] = 1
    ids[pos] = np.cumsum(b)
    return ids, len(ends)


def _binned(counts, probs, N, min_expected=MIN_EXPECTED):
    ids, nb = pool(probs, N, min_expected)
    keep = ids >= 0
    o = np.bincount(ids[keep], weights=np.asarray(counts, dtype=np.float64)[keep], minlength=nb)
    p = np.bincount(ids[keep], weights=np.asarray(probs, dtype=np.float64)[keep], minlength=nb)
    return o, p


def chi2_gof(counts, probs, what, alpha=ALPHA, min_expected=MIN_EXPECTED):
    """Asserts that `counts` (per category) follow `probs` (per category, summing to 1): structural zeros exactly, the
    rest by a pooled chi-square at level alpha.  -> (statistic, dof, p); dof 0 when pooling leaves one bin (no test)."""
    counts = np.asarray(counts, dtype=np.int64)
    probs = np.asarray(probs, dtype=np.float64)
    assert counts.shape == probs.shape, (what, counts.shape, probs.shape)
    assert abs(probs.sum() - 1.0) < 1e-9, "%s: law sums to %.15f" % (what, probs.sum())
    zero = probs <= 0
    bad = np.flatnonzero(zero & (counts != 0))
    assert bad.size == 0, "%s: %d outcomes in structural zeros, first categories %s" % (
        what, int(counts[bad].sum()), bad[:8].tolist())
    N = int(counts.sum())
    o, p = _binned(counts, probs, N, min_expected)
    dof = o.size - 1
    if dof == 0:
        return 0.0, 0, 1.0
    e = p * N
    stat = float(((o - e) ** 2 / e).sum())
    pv = float(stats.chi2.sf(stat, dof))
    assert pv >= alpha, "%s: chi2 %.1f on %d dof, p = %.2e (N = %d) -- counts do not follow the exact law" % (
        what, stat, dof, pv, N)
    return stat, dof, pv


def power(alt_probs, probs, N, alpha=ALPHA, min_expected=MIN_EXPECTED):
    """Probability that chi2_gof(counts ~ Multinomial(N, alt_probs), probs) fails: the pooled chi-square's power
    (noncentral chi-square, scipy.stats.ncx2) combined with the chance of at least one outcome in a structural zero."""
    alt = np.asarray(alt_probs, dtype=np.float64)
    probs = np.asarray(probs, dtype=np.float64)
    o, p = _binned(alt * N, probs, N, min_expected)
    q = o / N
    dof = p.size - 1
    miss = 1.0
    if dof > 0:
        lam = N * float(((q - p) ** 2 / p).sum())
        crit = stats.chi2.isf(alpha, dof)
        miss = float(stats.ncx2.cdf(crit, dof, lam)) if lam > 0 else 1.0 - alpha
    zmass = float(alt[probs <= 0].sum())
    miss *= (1.0 - min(zmass, 1.0)) ** N
    return 1.0 - miss


# ---------------------------------------------------------------- reservoir laws
class ReservoirLaw:
    """Output law of a k-slot reservoir loop over n candidates in which candidate i >= k writes each slot with
    probability a[i] (module docstring).  Positions are candidate ranks 0..n-1."""

    def __init__(self, a, n, k):
        assert n > k >= 1
        self.n, self.k = n, k
        a = np.asarray(a, dtype=np.float64)
        assert a.size == n and np.all(a[k:] >= 0) and np.all(a[k:] * k <= 1 + 1e-12)
        self.a = np.where(np.arange(n) >= k, a, 0.0)
        with np.errstate(divide="ignore"):                                   # a_i = 1: log 0 = -inf is meant
            lg1 = np.log1p(-np.minimum(self.a, 1.0))
            lg2 = np.log1p(-np.minimum(2 * self.a, 1.0)) if k >= 2 else None
        self.S1 = np.concatenate([np.cumsum(lg1[::-1])[::-1], [0.0]])           # S1[j] = sum_{i >= j}
        self.C1 = np.concatenate([[0.0], np.cumsum(lg1)])                       # C1[j] = sum_{i < j}
        if k >= 2:
            self.S2 = np.concatenate([np.cumsum(lg2[::-1])[::-1], [0.0]])

    def marginal(self, s):
        """P(slot s holds position p), p = 0..n-1"""
        n, k = self.n, self.k
        P = np.zeros(n)
        P[k:] = self.a[k:] * np.exp(self.S1[k + 1:n + 1])
        P[s] = np.exp(self.S1[k])
        return P

    def tail_bins(self, n_bins):
        """edges k = e_0 < ... <= n of contiguous position bins of about equal marginal probability"""
        P = self.marginal(0)[self.k:]
        c = np.cumsum(P) / P.sum()
        cuts = np.searchsorted(c, np.arange(1, n_bins) / n_bins, side="right") + self.k
        return np.unique(np.concatenate([[self.k], cuts, [self.n]]))

    def pair_table(self, edges):
        """joint law of (category of slot s, category of slot t), s != t: category 0 = own position, c = 1.. = tail bin
        [edges[c-1], edges[c]).  Symmetric; the same for every pair of distinct slots."""
        assert self.k >= 2
        n, k, a, C1, S2 = self.n, self.k, self.a, self.C1, self.S2
        q = np.arange(k, n)
        f = a[k:] * np.exp(-C1[k + 1:n + 1])                                   # f(p) = a_p exp(-C1[p+1])
        g = a[k:] * np.exp(C1[k:n] + S2[k + 1:n + 1])                          # g(q) = a_q exp(C1[q] + S2[q+1])
        h = g                                                                  # own & q: a_q exp(C1[q] + S2[q+1])
        assert np.all(np.isfinite(f)) and np.all(np.isfinite(g))
        m = len(edges) - 1
        T = np.zeros((m + 1, m + 1))
        T[0, 0] = np.exp(S2[k])
        bid = np.searchsorted(edges, q, side="right") - 1
        Fb = np.bincount(bid, weights=f, minlength=m)
        Gb = np.bincount(bid, weights=g, minlength=m)
        Hb = np.bincount(bid, weights=h, minlength=m)
        T[0, 1:] = T[1:, 0] = Hb
        # within a bin: sum over p < q of f(p) g(q), both slot orders
        cf = np.cumsum(f) - f                                                  # sum of f over positions before q ...
        start = np.concatenate([[0.0], np.cumsum(Fb)])[bid]                    # ... minus those of earlier bins
        Wb = np.bincount(bid, weights=g * (cf - start), minlength=m)
        for A in range(m):
            T[1 + A, 1 + A] = 2 * Wb[A]
            T[1 + A, 2 + A:] = Fb[A] * Gb[A + 1:]
            T[2 + A:, 1 + A] = Fb[A] * Gb[A + 1:]
        return T


def uniform_a(n, k, quirk=True):
    """uniform reservoir: candidate i draws j from 0..i (the reference: 0..i exclusive, quirk=True) or 0..=i"""
    i = np.arange(n, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(i >= k, 1.0 / (i if quirk else i + 1), 0.0)


def weighted_a(w, k, shift=False):
    """weighted reservoir: candidate i is taken with probability w_i / W_i, then writes one of k slots uniformly.
    shift=True is the named wrong law W_{i-1} in place of W_i (capped at probability 1)."""
    w = np.asarray(w, dtype=np.float64)
    W = np.cumsum(w)
    if shift:
        W = np.concatenate([[w[0]], W[:-1]])
    with np.errstate(divide="ignore", invalid="ignore"):
        take = np.where(W > 0, np.minimum(w / W, 1.0), 0.0)
    return np.where(np.arange(w.size) >= k, take / k, 0.0)


def uniform_law(n, k, quirk=True):
    return ReservoirLaw(uniform_a(n, k, quirk), n, k)


def weighted_law(w, k, shift=False):
    w = np.asarray(w, dtype=np.float64)
    assert w[:k].sum() > 0, "the reference panics on an empty float range (sampling.rs:49)"
    return ReservoirLaw(weighted_a(w, k, shift), w.size, k)


def replacement_marginal(n):
    return np.full(n, 1.0 / n)


# ---------------------------------------------------------------- walks
def one_slot_walk_law(n):
    """tempo_random_walk's step over n admissible candidates (reservoir_sampling with k = 1, random_walk.rs:140-141):
    candidate 0 only when n == 1 (the quirk: candidate 1 always replaces it), else uniform over 1..n-1."""
    P = np.zeros(n)
    if n == 1:
        P[0] = 1.0
    else:
        P[1:] = 1.0 / (n - 1)
    return P


def one_slot_chunked_law(raw_pos, off_by_one=False):
    """The law of the chunked one-slot restatement (one draw per chunk of 64 raw positions): a chunk with m eligible
    candidates after M take the slot with probability m / (M + m).  off_by_one=True: the named wrong law m / (M + m + 1).
    Exact for the correct form (= one_slot_walk_law); the wrong one is computed chunk by chunk."""
    raw_pos = np.asarray(raw_pos)
    n = raw_pos.size
    P = np.zeros(n)
    if n == 0:
        return P
    P[0] = 1.0
    seen, i = 0, 1
    while i < n:
        ch = raw_pos[i] >> 6
        j = i
        while j < n and (raw_pos[j] >> 6) == ch:
            j += 1
        m = j - i
        t = 1.0 if seen == 0 else m / (seen + m + (1 if off_by_one else 0))
        P[:i] *= 1.0 - t
        P[i:j] = t / m
        seen += m
        i = j
    return P


def node2vec_probs(p, q):
    """(prob0, prob1, prob2) as random_walk.rs:28-37 computes them, in f32"""
    f = np.float32
    inv_p, one, inv_q = f(1.0) / f(p), f(1.0), f(1.0) / f(q)
    mx = max(inv_p, one, inv_q)
    return float(inv_p / mx), float(one / mx), float(inv_q / mx)


def node2vec_step_law(row_ptrs, col, cur, prev, p, q, look=None):
    """P(next = position j of cur's row) of the rejection loop random_walk.rs:52-66: a uniform position, accepted with
    prob0 if it is prev, prob1 if it has an edge to prev, prob2 otherwise; prev = -1 before the first step.  look: (ptrs,
    col) of the graph whose rows answer has_edge, the walked graph unless a named wrong law says otherwise."""
    nb = col[row_ptrs[cur]:row_ptrs[cur + 1]]
    p0, p1, p2 = node2vec_probs(p, q)
    acc = np.empty(nb.size)
    look_ptrs, look_col = (row_ptrs, col) if look is None else look
    for j, v in enumerate(nb):
        if v == prev:
            acc[j] = p0
        elif prev >= 0 and prev in look_col[look_ptrs[v]:look_ptrs[v + 1]]:
            acc[j] = p1
        else:
            acc[j] = p2
    return acc / acc.sum()


def bias_weights(times, t, bias, forward=True):
    """BiasType::apply (random_walk.rs:160-181): uniform ones; linear = argsort(times, descending) as weights (the
    reference's quirk: indices of the sorted order, not ranks), normalised; exponential = softmax(t - times) forward,
    softmax(times - t) backward.  Distinct times only (argsort ties are not pinned)."""
    times = np.asarray(times, dtype=np.int64)
    if bias == "uniform":
        return np.ones(times.size)
    if bias == "linear":
        assert np.unique(times).size == times.size
        w = np.argsort(-times, kind="stable").astype(np.float64)
        return w / w.sum()
    d = (t - times) if forward else (times - t)
    d = d.astype(np.float64)
    e = np.exp(d - d.max())
    return e / e.sum()


def biased_step_law(times, t, bias, forward=True):
    """one-slot weighted reservoir (k = 1) over the bias weights: P(candidate i) = w_i / sum(w) (telescoping)"""
    w = bias_weights(times, t, bias, forward)
    return w / w.sum()


# ---------------------------------------------------------------- negative sampling
def negative_item_law(size, admissible, tries):
    """one item of negative_sample_neighbors_homogenous (negative_sampling.rs:31-45): up to `tries` draws of w from
    0..size, the first admissible one wins.  -> probabilities over [w = 0..size-1, no negative]"""
    adm = np.asarray(admissible, dtype=bool)
    a = int(adm.sum())
    b = (size - a) / size
    miss = b ** tries
    P = np.zeros(size + 1)
    P[:size][adm] = (1.0 - miss) / a if a else 0.0
    P[size] = miss
    return P


class ReplacementLaw:
    """with replacement (sampling.rs:57-69): every slot uniform over n, slots independent; same interface as
    ReservoirLaw with no own-position category (tail0 = 0)"""

    def __init__(self, n, k):
        self.n, self.k, self.tail0 = n, k, 0

    def marginal(self, s):
        return np.full(self.n, 1.0 / self.n)

    def tail_bins(self, n_bins):
        return np.unique(np.linspace(0, self.n, n_bins + 1).round().astype(np.int64))

    def pair_table(self, edges):
        P = np.concatenate([[0.0], np.diff(edges) / self.n])
        return np.outer(P, P)


ReservoirLaw.tail0 = property(lambda self: self.k)
BOUNDARY_SLOTS = (15, 16, 31, 32, 63, 64, 127, 128)


def default_slots(k):
    return sorted({0, 1, k // 2, k - 1, *BOUNDARY_SLOTS} & set(range(k)))


class ReservoirTally:
    """check_reservoir over outcomes that arrive in chunks: add() asserts a chunk's structure and adds its counts (on
    the chunk's device), finish() runs the chi-square tests over all N outcomes.  Arguments as check_reservoir's."""

    def __init__(self, N, k, law, what, replace=False, zero_pos=None, slots=None, positions=None, pairs=None, pair_bins=24):
        n = law.n
        self.N, self.k, self.law, self.what, self.replace, self.zero_pos, self.seen = N, k, law, what, replace, zero_pos, 0
        self.slots = list(default_slots(k) if slots is None else slots)
        self.positions = [] if replace else list(sorted({k, (k + n) // 2, n - 1}) if positions is None else positions)
        self.pairs = []
        if k >= 2:
            nb = int(min(pair_bins, max(1, np.sqrt(N / MIN_EXPECTED) - 1), n - law.tail0))
            self.edges = law.tail_bins(nb)
            self.m = len(self.edges) - 1
            self.pairs = [(a, b) for a, b in (((0, 1), (0, k - 1), (k // 2, k - 1)) if pairs is None else pairs) if a != b]
        self.cnt = {}

    def _acc(self, key, t):
        self.cnt[key] = t if key not in self.cnt else self.cnt[key] + t

    def add(self, E):
        import torch
        what, k, n, replace = self.what, self.k, self.law.n, self.replace
        assert E.shape[1] == k
        assert int(((E < 0) | (E >= n)).sum()) == 0, "%s: ranks outside [0, n)" % what
        if not replace:
            ar = torch.arange(k, device=E.device)
            assert int(((E < k) & (E != ar)).sum()) == 0, "%s: a slot holds an earlier candidate other than its own" % what
            if k > 1:
                srt = E.sort(1).values
                assert int((srt[:, 1:] == srt[:, :-1]).sum()) == 0, "%s: a candidate twice in one outcome" % what
        if self.zero_pos is not None:
            hit = self.zero_pos[E] & (E >= (0 if replace else k))
            assert int(hit.sum()) == 0, "%s: a zero-probability candidate was sampled" % what
        for s in dict.fromkeys(self.slots):                  # a slot, rank or pair listed twice is counted once
            self._acc(("slot", s), torch.bincount(E[:, s], minlength=n))
        for q in dict.fromkeys(self.positions):
            self._acc(("pos", q), (E == q).sum(0))
        if self.pairs:
            et = torch.as_tensor(self.edges, device=E.device)
            m = self.m
            for a, b in dict.fromkeys(self.pairs):
                ca = torch.bucketize(E[:, a].contiguous(), et, right=True)
                cb = torch.bucketize(E[:, b].contiguous(), et, right=True)
                self._acc(("pair", a, b), torch.bincount(ca * (m + 1) + cb, minlength=(m + 1) ** 2))
        self.seen += E.shape[0]
        return self

    def finish(self):
        what, k, law, N = self.what, self.k, self.law, self.N
        assert self.seen == N, "%s: %d of %d outcomes counted" % (what, self.seen, N)
        tests = 0
        for s in self.slots:
            tests += chi2_gof(self.cnt[("slot", s)].cpu().numpy(), law.marginal(s), "%s slot %d" % (what, s))[1] > 0
        for q in self.positions:
            held = self.cnt[("pos", q)].cpu().numpy()
            pq = law.marginal(0)[q]
            probs = np.concatenate([np.full(k, pq), [max(0.0, 1.0 - k * pq)]])
            probs /= probs.sum()
            tests += chi2_gof(np.concatenate([held, [N - held.sum()]]), probs, "%s which slot holds rank %d" % (what, q))[1] > 0
        if self.pairs:
            T = law.pair_table(self.edges)
            for a, b in self.pairs:
                joint = self.cnt[("pair", a, b)].cpu().numpy()
                tests += chi2_gof(joint, (T / T.sum()).ravel(), "%s slots (%d, %d)" % (what, a, b))[1] > 0
        return tests


def check_reservoir(E, law, what, replace=False, zero_pos=None, slots=None, positions=None, pairs=None, pair_bins=24):
    """One-sample tests of N sampled outcomes E ([N, k] int64 torch tensor of candidate ranks, any device; counted where
    it lives) against `law` (ReservoirLaw, or ReplacementLaw with replace=True):
      - every slot: ranks in [0, n); without replacement no rank < k but the slot's own and no rank twice in a row;
        zero_pos (bool tensor over ranks, e.g. zero weights) never sampled;
      - each slot of `slots`: its marginal over the n ranks;
      - each rank of `positions` (>= k, without replacement): which slot holds it, or none -- exclusive events;
      - each pair of `pairs`: the joint law of the two slots' (own / tail bin) categories.
    -> number of chi-square tests run (dof > 0)."""
    N, k = E.shape
    return ReservoirTally(N, k, law, what, replace, zero_pos, slots, positions, pairs, pair_bins).add(E).finish()


# ---------------------------------------------------------------- the typed samplers: hgt_sampling, budget_sampling
# Derived from src/algo/hgt_sampling.rs and src/algo/budget_sampling.rs alone.  Canonical order (the reference's HashMap
# order is not reproducible): relations in `edge_types` order, samples in list order, neighbours in column order.
TYPED_MAX_NB = 50                                                       # MAX_NEIGHBORS (hgt_sampling.rs:10, budget_sampling.rs:10)


def hgt_budget_weights(contribs, sampled=(), budget=None):
    """`BudgetDict::update_budget` (hgt_sampling.rs:27-102) for ONE source node type, restated literally: `contribs` is
    the list of (col_ptrs, row_indices, samples) of the relations out of that type, in canonical order; every sample w
    contributes the first min(deg, 50) entries of its column (:72: the reservoir over 0..min(len, 50) into 50 slots takes
    them all, in order, without a draw), each adding inv_deg = 1 / min(deg, 50) with a sequential f64 `+=` (:96) unless
    the neighbour is in `sampled` (:80).  `budget` (an insertion-ordered dict key -> score) is continued when given.
    -> (keys in insertion order [n] int64, score ** 2 [n] f64 -- the weights of sample_from, :110 -- and the dict)"""
    sampled = set(int(v) for v in sampled)
    budget = {} if budget is None else budget
    for ptrs, indices, samples in contribs:
        for w in samples:
            lo, hi = int(ptrs[w]), int(ptrs[w + 1])
            if hi == lo:
                continue                                                # :60
            cnt = min(hi - lo, TYPED_MAX_NB)
            inv_deg = 1.0 / float(cnt)
            for i in range(cnt):
                v = int(indices[lo + i])
                if v in sampled:
                    continue
                budget[v] = budget.get(v, 0.0) + inv_deg                # python floats are f64: the same rounding chain
    keys = np.fromiter(budget.keys(), dtype=np.int64, count=len(budget))
    score = np.fromiter(budget.values(), dtype=np.float64, count=len(budget))
    return keys, score * score, budget


def hgt_layer_law(w, k):
    """One layer of `BudgetDict::sample_from` (hgt_sampling.rs:104-135) over a budget of n live entries with weights w
    (insertion order): it IS reservoir_sampling_weighted (sampling.rs:28-55) with k slots, so the law is
    weighted_law(w, k) -- no new maths.  Ranks are positions among the LIVE entries (a removed entry is gone from the
    HashMap, :220).  n <= k takes every entry in order with no draw: there is no law then (-> None) and slot s holds
    entry s."""
    w = np.asarray(w, dtype=np.float64)
    if w.size <= k:
        return None
    return weighted_law(w, k)


def _csc(columns, n_cols):
    """CSC of {column: list of row ids} -> (ptrs [n_cols + 1], indices)"""
    ptrs = np.zeros(n_cols + 1, dtype=np.int64)
    for c, rows in columns.items():
        ptrs[c + 1] = len(rows)
    ptrs = np.cumsum(ptrs)
    idx = np.concatenate([np.asarray(columns[c], dtype=np.int64) for c in sorted(columns)] or [np.zeros(0, dtype=np.int64)])
    return ptrs, idx


def hgt_heavy_ranks(n):
    """ranks of hgt_wide_graph's heavy entries: one early, then at 30 %, 55 % and 80 % of the budget"""
    return sorted({r for r in (1, (3 * n) // 10, (11 * n) // 20, (4 * n) // 5) if 1 <= r < n})


def hgt_wide_graph(n, seed):
    """An HGT budget of exactly n entries with wide, known weights.  Types a (inputs) and b, one relation b -> a.  The
    inputs' columns have 1..50 entries: some fresh b nodes and some shared with earlier columns (early ranks more often),
    so scores run from 1/50 up and many entries have two or more contributions; the entries of hgt_heavy_ranks(n) are
    also the only neighbour of a few further inputs each (score += 1 per input: several units, the square is of the order
    of all the weight before them -- where a mis-carried running sum shows).  b's node ids are a permutation: an id is not
    its rank.  -> dict(node_types, edge_types, ptrs, indices, inputs {"a": ids}, keys [n], w [n], rank_of [n_b])"""
    rs = np.random.default_rng(seed)
    n_b = n + 7
    ids = rs.permutation(n_b)[:n]                                       # node id of rank r
    heavy = hgt_heavy_ranks(n)
    columns, made, pending = [], 0, []
    while made < n:
        length = int(rs.integers(1, TYPED_MAX_NB + 1))
        fresh = min(n - made, length if made == 0 else int(rs.integers((length + 1) // 2, length + 1)))
        old = min(length - fresh, made)
        col = list(range(made, made + fresh))                          # fresh entries in rank order: label = rank
        if old:
            pick = np.unique((rs.random(3 * old) ** 2 * made).astype(np.int64))[:old]
            for v in pick.tolist():                                     # shared ones anywhere between them
                col.insert(int(rs.integers(0, len(col) + 1)), v)
        columns.append(col)
        for h in heavy:
            if made <= h < made + fresh:
                pending.append(h)
        made += fresh
        for h in pending:                                               # after its first appearance: columns of one entry
            columns += [[h]] * max(2, int(np.ceil(np.sqrt(0.05 * h))))
        pending = []
    m = len(columns)
    ptrs, idx = _csc({c: ids[np.asarray(col)] for c, col in enumerate(columns)}, m)
    inputs = np.arange(m, dtype=np.int64)
    keys, w, _ = hgt_budget_weights([(ptrs, idx, inputs)])
    assert keys.size == n and np.unique(keys).size == n
    rank_of = np.full(n_b, -1, dtype=np.int64)
    rank_of[keys] = np.arange(n)
    return dict(node_types=["a", "b"], edge_types=[("b", "r", "a")], ptrs={"b__r__a": ptrs}, indices={"b__r__a": idx},
                inputs={"a": inputs}, keys=keys, w=w, rank_of=rank_of, n_b=n_b)


def hgt_dead_prefix_graph(n0, n1, seed, fan=TYPED_MAX_NB):
    """The dead-prefix case: relations b -> a and b -> b.  Layer 0 (quota >= n0) takes the whole budget of n0 entries --
    no draw: slot s holds entry s, all n0 die -- and layer 1 samples from the n1 FRESH entries the b -> b columns of those
    n0 samples contribute (columns also list layer-0 nodes: already sampled, skipped, :80), which sit behind n0 dead ones.
    Its law is weighted_law over the n1 live entries.  -> dict as hgt_wide_graph, with keys0 (layer 0, in order), keys / w /
    rank_of of layer 1's live entries, and w_dead (the n0 dead entries' old weights: named wrong law (c))."""
    rs = np.random.default_rng(seed)
    n_b = n0 + n1 + 5
    ids = rs.permutation(n_b)
    first, second = ids[:n0], ids[n0:n0 + n1]
    m = -(-n0 // fan)
    cols_a = {c: first[c * fan:(c + 1) * fan] for c in range(m)}
    pa, ia = _csc(cols_a, m)
    heavy = hgt_heavy_ranks(n1)[1:] if n0 >= 20 else []                  # each: three columns of that one entry, score += 3
    M = n0 - 3 * len(heavy)                                             # the other columns share the n1 fresh entries evenly
    assert n1 <= 40 * M
    cols_b, made, normal, pending = {}, 0, 0, []
    for v in first:
        if pending:
            cols_b[int(v)] = [second[pending.pop()]]
            continue
        fresh = n1 // M + (1 if normal < n1 % M else 0)
        normal += 1
        col = list(second[made:made + fresh]) + list(rs.choice(first, min(n0, int(rs.integers(0, 5))), replace=False))
        if made:
            col += list(rs.choice(second[:made], min(made, int(rs.integers(0, 4))), replace=False))
        cols_b[int(v)] = [col[i] for i in rs.permutation(len(col))]
        pending = [h for h in heavy if made <= h < made + fresh for _ in range(3)]
        made += fresh
    assert made == n1 and not pending
    pb, ib = _csc(cols_b, n_b)
    inputs = np.arange(m, dtype=np.int64)
    keys0, w0, bud = hgt_budget_weights([(pa, ia, inputs)])
    assert np.array_equal(keys0, first)
    for v in keys0:                                                     # :220 the samples leave the budget
        del bud[int(v)]
    keys, w, _ = hgt_budget_weights([(pb, ib, keys0)], sampled=keys0, budget=bud)
    assert keys.size == n1 and np.unique(keys).size == n1
    rank_of = np.full(n_b, -1, dtype=np.int64)
    rank_of[keys] = np.arange(n1)
    return dict(node_types=["a", "b"], edge_types=[("b", "r", "a"), ("b", "s", "b")],
                ptrs={"b__r__a": pa, "b__s__b": pb}, indices={"b__r__a": ia, "b__s__b": ib}, inputs={"a": inputs},
                keys0=keys0, keys=keys, w=w, w_dead=w0, rank_of=rank_of, n_b=n_b)


def hgt_edge_graph(deg, n_hubs):
    """The HGT edge phase (hgt_sampling.rs:254-267): one type, one relation a -> a.  Inputs = a pool of `deg` nodes
    (0..deg-1, empty columns) followed by n_hubs hubs, each hub's column the whole pool in order; num_hops = 0.  Every
    source is a sampled node, so hub i pushes exactly min(deg, 50) edges, in slot order, and edge_index - ptrs[hub] is
    the slot's column position: its law is uniform_law(deg, 50) (deg > 50), quirk included.
    -> (node_types, edge_types, ptrs, indices, inputs, hub_ptrs [n_hubs])"""
    n = deg + n_hubs
    ptrs = np.zeros(n + 1, dtype=np.int64)
    ptrs[deg + 1:] = deg * np.arange(1, n_hubs + 1)
    idx = np.tile(np.arange(deg, dtype=np.int64), n_hubs)
    return ["a"], [("a", "r", "a")], {"a__r__a": ptrs}, {"a__r__a": idx}, np.arange(n, dtype=np.int64), ptrs[deg:n].copy()


def budget_hub_graph(lengths, window=None, seed=0):
    """budget_sampling's `Budget::sample` (budget_sampling.rs:128-152) over one hub's candidate list.  Types a (the hub,
    node 0) and b; len(lengths) relations b -> a, relation r's column of the hub `lengths[r]` long (0: the relation is
    skipped, :90).  The list is the concatenation, relations in order, of every column's first 50 entries (:100) that pass
    the filter; its law is uniform_law(n, k), quirk included, n the list's length.  The admitted entry of list rank q has
    node id q; every other column entry (past the prefix, or filtered out) has an id >= n.  window = (lo, hi): row
    timestamps 0..89 at random and the hub at time 100 with forward = False, so an entry is admitted iff lo <= 100 - t <
    hi (:20-29).  -> dict(node_types, edge_types, ptrs, indices, row_ts or None, n, hub_ts)"""
    rs = np.random.default_rng(seed)
    R = len(lengths)
    rels = [("b", "r%02d" % r, "a") for r in range(R)]
    ts = [rs.integers(0, 90, L_) for L_ in lengths] if window is not None else None
    adm = []
    for r, L_ in enumerate(lengths):
        a = np.zeros(L_, dtype=bool)
        a[:TYPED_MAX_NB] = True
        if window is not None:
            a &= (100 - ts[r] >= window[0]) & (100 - ts[r] < window[1])
        adm.append(a)
    n = int(sum(a.sum() for a in adm))
    ptrs, indices, row_ts, q, spare = {}, {}, {}, 0, n
    for r, L_ in enumerate(lengths):
        key = "b__r%02d__a" % r
        ids = np.empty(L_, dtype=np.int64)
        na = int(adm[r].sum())
        ids[adm[r]] = np.arange(q, q + na)
        ids[~adm[r]] = np.arange(spare, spare + L_ - na)
        q, spare = q + na, spare + L_ - na
        ptrs[key], indices[key] = np.array([0, L_], dtype=np.int64), ids
        if ts is not None:
            row_ts[key] = ts[r].astype(np.int64)
    return dict(node_types=["a", "b"], edge_types=rels, ptrs=ptrs, indices=indices, row_ts=row_ts if ts is not None else None,
                n=n, hub_ts=100)


BUDGET_LISTS = {                                                        # list length n -> column lengths of the relations
    2: [1, 1], 6: [3, 0, 3], 51: [57, 1], 64: [50, 14], 65: [70, 0, 15], 100: [50, 64], 150: [50, 51, 100],
    800: [50 + (7 * r) % 30 for r in range(16)],
}
BUDGET_K = (1, 5, 50, 63, 64)
BUDGET_FILTERED = dict(lengths=[60, 55, 70], window=(20, 70), k=5)     # three relations, about half of 150 admitted
EDGE_DEGS = (51, 64, 65, 1000, 70000)


def reservoir_power(wrong, right, N, slots=None, positions=()):
    """The chance that check_reservoir rejects N outcomes drawn from the law `wrong` when it tests against `right`: at
    least that of its most powerful single test -- a slot's marginal (slots: default_slots) or which slot holds one rank
    of `positions`."""
    k = right.k
    best = 0.0
    for s in (default_slots(k) if slots is None else slots):
        best = max(best, power(wrong.marginal(s), right.marginal(s), N))
        if best >= 1.0 - 1e-12:
            return best
    for q in positions:
        pr, pw = right.marginal(0)[q], wrong.marginal(0)[q]
        a = np.concatenate([np.full(k, pr), [max(0.0, 1.0 - k * pr)]])
        b = np.concatenate([np.full(k, pw), [max(0.0, 1.0 - k * pw)]])
        best = max(best, power(b / b.sum(), a / a.sum(), N))
    return best


# sample sizes of tests/test_gpu_exact_laws_typed.py; tests/test_exact_laws_cpu.py asserts their power
HGT_CASES = [(1, 2), (2, 65), (3, 64), (63, 257), (64, 257), (65, 257), (191, 4097), (1000, 4097)]
HGT_LARGE = [(16, 65537), (8193, 12288)]                                # second tile of chunk totals; global slot table
HGT_DEAD = (100, 300, 7)                                                # n0, n1, k1
HGT_SURFACE_CALLS = 4096                                                # single calls of the (2, 65) case
BUDGET_FILTERED_OUTCOMES = 1 << 17
# (n, k, N): BUDGET_LISTS x BUDGET_K with k < n, N the smallest power of two at which reservoir_power against the law
# without the quirk reaches 0.999 (the quirk moves a slot's own-position marginal from (k-1)/(n-1) to k/n: the larger k and
# n, the more outcomes it takes); the GPU tests run them in launches of bounded size
BUDGET_CASES = [(2, 1, 1 << 12), (6, 1, 1 << 12), (6, 5, 1 << 14),
                (51, 1, 1 << 12), (51, 5, 1 << 15), (51, 50, 1 << 23),
                (64, 1, 1 << 12), (64, 5, 1 << 16), (64, 50, 1 << 21), (64, 63, 1 << 24),
                (65, 1, 1 << 12), (65, 5, 1 << 16), (65, 50, 1 << 21), (65, 63, 1 << 24), (65, 64, 1 << 25),
                (100, 1, 1 << 12), (100, 5, 1 << 17), (100, 50, 1 << 21), (100, 63, 1 << 21), (100, 64, 1 << 21),
                (150, 1, 1 << 12), (150, 5, 1 << 17), (150, 50, 1 << 21), (150, 63, 1 << 22), (150, 64, 1 << 22),
                (800, 1, 1 << 13), (800, 5, 1 << 21), (800, 50, 1 << 24), (800, 63, 1 << 25), (800, 64, 1 << 25)]
# hubs of the edge phase: deg 51..1000 reach 0.999 against the law without the quirk; at deg 70 000 that law is out of
# reach (1/69 999 against 1/70 000), see test_power_budget_and_edge_phase_without_the_quirk
EDGE_OUTCOMES = {51: 1 << 23, 64: 1 << 21, 65: 1 << 21, 1000: 1 << 25, 70000: 1 << 15}


def hgt_outcomes(k, n):
    """calls of an HGT sample_from case: 2^16 for the small budgets, 2^14 from n = 4097 on, 2^12 for the two large ones
    (each at least what reservoir_power needs against the named wrong laws)"""
    return 1 << (16 if n <= 300 else 14 if n <= 4097 else 12)


def hgt_slots(k):
    """default slots (slot k - 1 among them); the global-slot-table case looks at five marginals only"""
    return [0, 1, 4096, 8191, 8192] if k == 8193 else default_slots(k)


def hgt_positions(k, n):
    """the heavy entries behind the first k, and the last entry"""
    return sorted({h for h in hgt_heavy_ranks(n) if h >= k} | {n - 1})


# ---------------------------------------------------------------- link seed rows: checked negatives in rows of fixed shape
# The rejection loop of negative_sampling.rs:33-43 (draw, reject on has_edge(v, w) or v == w, at most try_count times) with
# the one rule tg_link_seeds adds because a row's shape is fixed (tchgeo.h, "The first accepted attempt..."): when no attempt
# was accepted the LAST one is kept, and counted as unverified.  try_count = 1 makes no look-up: attempt 0 is kept.
def link_admissible(ptrs, indices, n_src, same_type):
    """bool [n_src, n_dst] of a relation's CSC (column d lists the sources s of its edges s -> d): True where a candidate
    (s, d) is accepted -- not edge(s -> d) and, when both endpoints are one node type, s != d"""
    ptrs, indices = np.asarray(ptrs, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    n_dst = ptrs.size - 1
    adm = np.ones((n_src, n_dst), dtype=bool)
    adm[indices, np.repeat(np.arange(n_dst), np.diff(ptrs))] = False
    if same_type:
        assert n_src == n_dst
        adm[np.arange(n_src), np.arange(n_src)] = False
    return adm


def _kept_attempt_law(adm, tries, drop_last=False):
    """Candidates uniform over adm's cells, up to `tries` attempts, the first admissible one kept, else the last attempt:
    with q = 1 - |A| / n an admissible cell has (1 - q^tries) / |A| (the geometric sum of q^a / n), an inadmissible one
    q^(tries-1) / n (tries - 1 rejections, then this very cell).  tries = 1: uniform.  drop_last=True is the named wrong law
    that emits accepted attempts only (the reference's rule, which a row of fixed shape cannot follow): uniform over A."""
    adm = np.asarray(adm, dtype=bool).ravel()
    assert tries >= 1 and adm.size > 0
    n, a = adm.size, int(adm.sum())
    q = 1.0 - a / n
    if drop_last:
        assert a > 0
        return adm / float(a)
    P = np.full(n, q ** (tries - 1) / n)
    if a:
        P[adm] = (1.0 - q ** tries) / a
    return P


def link_binary_law(n_src, n_dst, admissible, tries, drop_last=False):
    """TG_LINK_BINARY: one negative's (s, d), both ends drawn; category s * n_dst + d.  admissible: link_admissible's matrix"""
    adm = np.asarray(admissible, dtype=bool)
    assert adm.shape == (n_src, n_dst)
    return _kept_attempt_law(adm, tries, drop_last)


def link_triplet_law(n_dst, admissible_row, tries, drop_last=False):
    """TG_LINK_TRIPLET: one negative's d given its anchor s; admissible_row = link_admissible(...)[s]"""
    adm = np.asarray(admissible_row, dtype=bool)
    assert adm.shape == (n_dst,)
    return _kept_attempt_law(adm, tries, drop_last)


def link_unverified_law(admissible, tries):
    """[verified, unverified] of one negative: every attempt rejected has q^tries, so a launch's count is Binomial(N,
    q^tries); tries = 1 makes no look-up and counts nothing (a structural zero)."""
    adm = np.asarray(admissible, dtype=bool)
    u = 0.0 if tries == 1 else (1.0 - adm.sum() / adm.size) ** tries
    return np.array([1.0 - u, u])


# ---------------------------------------------------------------- skip-gram negatives (PyG's randint per column)
def product_uniform_law(n_a, n_b):
    """two independent words, uniform on [0, n_a) and [0, n_b); category a * n_b + b"""
    return np.full(n_a * n_b, 1.0 / (n_a * n_b))


def shared_draw_pair_law(n_a, n_b):
    """the named wrong law of two words made from ONE draw u in [0, 1): (floor(u n_a), floor(u n_b)); a cell's
    probability is the length of the intersection of its two intervals"""
    a, b = np.arange(n_a)[:, None], np.arange(n_b)[None, :]
    overlap = np.minimum((a + 1) * n_b, (b + 1) * n_a) - np.maximum(a * n_b, b * n_a)      # in units of 1 / (n_a n_b)
    return (np.maximum(overlap, 0) / float(n_a * n_b)).ravel()


# ---------------------------------------------------------------- consecutive walk steps
def chain_law(step_laws, start, sizes=None):
    """Joint law of (x_1, ..., x_m) of a walk from `start`: the product of the per-step conditional laws.  step_laws[l]
    (prev, cur) -> the law of x_{l+1} over the step's target ids given the walker stands at cur and came from prev (-1
    before the first step), all zero (or empty) at a dead end: the walk has ended, random_walk.rs:45-47, and `ended` absorbs
    every later column.  -> f64 array of shape (n_1 + 1, ..., n_m + 1), index n_l = ended; sizes: the n_l (else the sizes
    of the laws returned, 0 for a step no walk reaches)."""
    m = len(step_laws)
    paths, seen = {}, [0] * m

    def go(l, prev, cur, path, pr):
        if l == m:
            paths[path] = paths.get(path, 0.0) + pr
            return
        law = np.zeros(0) if cur < 0 else np.asarray(step_laws[l](prev, cur), dtype=np.float64)
        seen[l] = max(seen[l], law.size)
        nz = np.flatnonzero(law)
        if nz.size == 0:
            go(l + 1, cur, -1, path + (-1,), pr)
            return
        assert abs(law.sum() - 1.0) < 1e-12
        for v in nz.tolist():
            go(l + 1, cur, v, path + (v,), pr * float(law[v]))

    go(0, -1, int(start), (), 1.0)
    sizes = seen if sizes is None else list(sizes)
    assert all(s >= t for s, t in zip(sizes, seen))
    P = np.zeros([s + 1 for s in sizes])
    for path, pr in paths.items():
        P[tuple(s if v < 0 else v for v, s in zip(path, sizes))] += pr
    return P


def csr_step(ptrs, col, n_dst, rank_law=None):
    """step law over a CSR row: rank_law(deg) over the row's positions (default uniform: random_walk.rs:53 with p = q = 1,
    where every proposal is accepted, and the metapath step), folded onto the target ids"""
    ptrs, col = np.asarray(ptrs, dtype=np.int64), np.asarray(col, dtype=np.int64)

    def law(prev, cur):
        lo, hi = int(ptrs[cur]), int(ptrs[cur + 1])
        if hi == lo:
            return np.zeros(n_dst)
        w = np.full(hi - lo, 1.0 / (hi - lo)) if rank_law is None else rank_law(hi - lo)
        return np.bincount(col[lo:hi], weights=w, minlength=n_dst)
    return law


def node2vec_step(ptrs, col, n, p, q, swap_lookup=False):
    """node2vec_step_law folded onto vertex ids.  Step 1 has prev = -1: `next == prev` is false and has_edge(next, -1) is
    false, so every proposal is accepted with prob2 and the step is uniform (random_walk.rs:39, 56-63).  swap_lookup=True
    is the named wrong law that asks has_edge(prev, next) in place of has_edge(next, prev)."""
    ptrs, col = np.asarray(ptrs, dtype=np.int64), np.asarray(col, dtype=np.int64)
    look = None
    if swap_lookup:                                                      # has_edge answered by the transposed graph
        order = np.argsort(col, kind="stable")
        look = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n))]), np.repeat(np.arange(n), np.diff(ptrs))[order]

    def law(prev, cur):
        lo, hi = int(ptrs[cur]), int(ptrs[cur + 1])
        if hi == lo:
            return np.zeros(n)
        return np.bincount(col[lo:hi], weights=node2vec_step_law(ptrs, col, cur, prev, p, q, look), minlength=n)
    return law


def shared_draw_chain_law(csrs, start, m, sizes):
    """the named wrong law of m uniform steps that all use ONE draw u in [0, 1): x_{l+1} = row[floor(u deg)] at every step
    (step l over csrs[l mod M] = (ptrs, col)).  Exact: u runs over the cells of width 1 / lcm(degrees)."""
    degs = [int(d) for ptrs, _ in csrs for d in np.diff(ptrs) if d > 0]
    D = int(np.lcm.reduce(degs))
    P = np.zeros([s + 1 for s in sizes])
    for j in range(D):
        cur, path = int(start), []
        for l in range(m):
            ptrs, col = csrs[l % len(csrs)]
            if cur >= 0 and ptrs[cur + 1] > ptrs[cur]:
                deg = int(ptrs[cur + 1] - ptrs[cur])
                cur = int(col[ptrs[cur] + (j * deg) // D])
                path.append(cur)
            else:
                cur = -1
                path.append(sizes[l])
        P[tuple(path)] += 1.0 / D
    return P


def complete_csr(n):
    """the complete directed graph on n vertices without loops -> (ptrs, col), rows ascending"""
    col = np.array([v for u in range(n) for v in range(n) if v != u], dtype=np.int64)
    return np.arange(n + 1, dtype=np.int64) * (n - 1), col


# ---------------------------------------------------------------- sample sizes of tests/test_gpu_exact_laws.py
N_WALK = 1 << 20          # walkers per walk launch
N_NEG = 1 << 20           # negative items per launch


def n_outcomes(k):
    """outcomes per neighbour-sampling launch at fan-out k: 2^20, fewer above k = 64 so that the four int64 output
    slabs of a launch stay within 2 GiB"""
    p = 1
    while p < k:
        p <<= 1
    return min(1 << 20, (1 << 26) // p)


# ---------------------------------------------------------------- configurations of tests/test_gpu_exact_laws_batches.py
# tests/test_exact_laws_cpu.py asserts their power against the named wrong laws at these sample sizes
LINK_N = 97                                  # the homogeneous graph: not a power of two
LINK_TYPED = (61, 89)                        # n_src, n_dst of the typed relation
LINK_DENSITIES = (0.5, 0.97)
LINK_TRIES = (1, 2, 8)
LINK_SHAPE = (256, 64, 64)                   # E, K, G: G * K * E = N_NEG negatives per launch
LINK_ANCHORS = 4                             # triplet mode: mini-batch g has anchor g mod 4 at every positive
LINK_TRIPLET_LAUNCHES = 2                    # 2^19 negatives per anchor: what try_count 8 against 9 needs at density 0.5


def link_graph(n_src, n_dst, density, seed):
    """A relation in which each ordered pair (s, d), s != d, is an edge independently with probability `density`, so
    edge(s -> d) and edge(d -> s) differ on about half the pairs at 0.5; of the equal-id pairs only 0, 1, 2 are edges (the
    self-loops when both ends are one type), so the `s == d` rule decides every other cell of the diagonal.
    -> (ptrs, indices) of its CSC, M bool [n_src, n_dst]"""
    M = np.random.default_rng(seed).random((n_src, n_dst)) < density
    k = min(n_src, n_dst)
    M[np.arange(k), np.arange(k)] = np.arange(k) < 3
    ptrs = np.concatenate([[0], np.cumsum(M.sum(0))]).astype(np.int64)
    return ptrs, np.nonzero(M.T)[1].astype(np.int64), M


def link_power(wrong, right, admissible, N):
    """the chance that a link-seed test rejects N negatives of the law `wrong`: that of the more powerful of its two
    chi-square tests, the cells' law and the [admissible, inadmissible] fold of it (the unverified total's law; an
    inadmissible cell is rare and pools with its neighbours, so an error in the number of attempts shows in the fold)"""
    adm = np.asarray(admissible, dtype=bool).ravel()
    fold = lambda P: np.array([P[adm].sum(), P[~adm].sum()])
    return max(power(wrong, right, N), power(fold(wrong), fold(right), N))


def link_seed(kind, density):
    """generator seed of the link_graph of a GPU configuration"""
    return (100 if kind == "homo" else 200) + int(round(100 * density))


def link_anchors(M):
    """triplet anchors: source ids 1 (equal-id pair an edge), 4 (not one), and the sources with the fewest and the most
    out-edges among the others"""
    deg = M.sum(1).astype(np.int64)
    deg[[1, 4]] = -1
    rest = np.flatnonzero(deg >= 0)
    return [1, 4, int(rest[np.argmin(deg[rest])]), int(rest[np.argmax(deg[rest])])]


def wedge_graph():
    """9 vertices, every one with two or more out-edges: the triangle 0-1-2, open wedges (0-3-4, 1-5-6, ...) and two
    one-way edges 5 -> 0 and 2 -> 7, so has_edge(next, prev) and has_edge(prev, next) differ (from 0 over 1 to 5: 5 -> 0
    is an edge, 0 -> 5 is not).  -> (ptrs, col, 9), rows ascending"""
    und = [(0, 1), (0, 2), (1, 2), (0, 3), (3, 4), (1, 5), (5, 6), (2, 6), (4, 7), (7, 8), (6, 8), (3, 8), (4, 5)]
    rows = {v: set() for v in range(9)}
    for a, b in und:
        rows[a].add(b)
        rows[b].add(a)
    rows[5].add(0)
    rows[2].add(7)
    ptrs = np.concatenate([[0], np.cumsum([len(rows[v]) for v in range(9)])]).astype(np.int64)
    return ptrs, np.array([u for v in range(9) for u in sorted(rows[v])], dtype=np.int64), 9


MP_COUNTS = (5, 7)                           # node types A, B of the chain test's metapath A-B-A
MP_SINK = 3                                  # the B node without out-edges


def metapath_graph():
    """dense bipartite pair: A -> B where (a + 2 b) mod 5 != 0, B -> A where (a + b) mod 4 != 0, B node MP_SINK without
    out-edges -> [(ptrs, col) of A -> B, (ptrs, col) of B -> A] (CSR, rows ascending)"""
    nA, nB = MP_COUNTS
    ab = [[b for b in range(nB) if (a + 2 * b) % 5] for a in range(nA)]
    ba = [[a for a in range(nA) if (a + b) % 4 and b != MP_SINK] for b in range(nB)]
    out = []
    for rows in (ab, ba):
        ptrs = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        out.append((ptrs, np.array([v for r in rows for v in r], dtype=np.int64)))
    return out


WALK_SHAPE = (256, 64, 64)                   # B, R, G: G * R * B = N_WALK walkers per launch, K = 1 negative row per walker
WALK_STEPS = 3                               # x_1, x_2, x_3 of every walker (the temporal walk: two steps, 36 rank pairs)
NEG_NODES = 31                               # range of the skip-gram negatives; the metapath's types have 31 and 17 nodes
NEG_MP_COUNTS = (31, 17)
NEG_SHAPE = (256, 16, 16, 4, 4)              # B, R, K, G, T: U = R K B = 2^16 rows of L = 5 words per mini-batch, G U (L-1) = N_NEG
