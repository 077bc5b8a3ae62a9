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


def node2vec_step_law(row_ptrs, col, cur, prev, p, q):
    """P(next = position j of cur's row) of the rejection loop random_walk.rs:52-66: a uniform position, accepted with
    prob0 if it is prev, prob1 if it has an edge to prev, prob2 otherwise; prev = -1 before the first step."""
    nb = col[row_ptrs[cur]:row_ptrs[cur + 1]]
    p0, p1, p2 = node2vec_probs(p, q)
    acc = np.empty(nb.size)
    for j, v in enumerate(nb):
        if v == prev:
            acc[j] = p0
        elif prev >= 0 and prev in col[row_ptrs[v]:row_ptrs[v + 1]]:
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


def check_reservoir(E, law, what, replace=False, zero_pos=None, slots=None, positions=None, pairs=None, pair_bins=24):
    """One-sample tests of N sampled outcomes E ([N, k] int64 torch tensor of candidate ranks, any device; counted where
    it lives) against `law` (ReservoirLaw, or ReplacementLaw with replace=True):
      - every slot: ranks in [0, n); without replacement no rank < k but the slot's own and no rank twice in a row;
        zero_pos (bool tensor over ranks, e.g. zero weights) never sampled;
      - each slot of `slots`: its marginal over the n ranks;
      - each rank of `positions` (>= k, without replacement): which slot holds it, or none -- exclusive events;
      - each pair of `pairs`: the joint law of the two slots' (own / tail bin) categories.
    -> number of chi-square tests run (dof > 0)."""
    import torch
    N, k = E.shape
    n = law.n
    assert int(((E < 0) | (E >= n)).sum()) == 0, "%s: ranks outside [0, n)" % what
    if not replace:
        ar = torch.arange(k, device=E.device)
        assert int(((E < k) & (E != ar)).sum()) == 0, "%s: a slot holds an earlier candidate other than its own" % what
        if k > 1:
            srt = E.sort(1).values
            assert int((srt[:, 1:] == srt[:, :-1]).sum()) == 0, "%s: a candidate twice in one outcome" % what
    if zero_pos is not None:
        hit = zero_pos[E] & (E >= (0 if replace else k))
        assert int(hit.sum()) == 0, "%s: a zero-probability candidate was sampled" % what
    tests = 0
    for s in (default_slots(k) if slots is None else slots):
        cnt = torch.bincount(E[:, s], minlength=n).cpu().numpy()
        tests += chi2_gof(cnt, law.marginal(s), "%s slot %d" % (what, s))[1] > 0
    if not replace:
        for q in (sorted({k, (k + n) // 2, n - 1}) if positions is None else positions):
            held = (E == q).sum(0).cpu().numpy()
            pq = law.marginal(0)[q]
            probs = np.concatenate([np.full(k, pq), [max(0.0, 1.0 - k * pq)]])
            probs /= probs.sum()
            tests += chi2_gof(np.concatenate([held, [N - held.sum()]]), probs, "%s which slot holds rank %d" % (what, q))[1] > 0
    if k >= 2:
        nb = int(min(pair_bins, max(1, np.sqrt(N / MIN_EXPECTED) - 1), n - law.tail0))
        edges = law.tail_bins(nb)
        m = len(edges) - 1
        T = law.pair_table(edges)
        et = torch.as_tensor(edges, device=E.device)
        for a, b in (((0, 1), (0, k - 1), (k // 2, k - 1)) if pairs is None else pairs):
            if a == b:
                continue
            ca = torch.bucketize(E[:, a].contiguous(), et, right=True)
            cb = torch.bucketize(E[:, b].contiguous(), et, right=True)
            joint = torch.bincount(ca * (m + 1) + cb, minlength=(m + 1) ** 2).cpu().numpy()
            tests += chi2_gof(joint, (T / T.sum()).ravel(), "%s slots (%d, %d)" % (what, a, b))[1] > 0
    return tests


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
