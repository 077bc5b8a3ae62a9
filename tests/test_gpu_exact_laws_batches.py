"""The batch kernels -- tg_link_seeds, tg_link_seeds_typed, tg_rw_skipgram, tg_mp_skipgram, tg_tempo_skipgram -- and the
walk operators under them against the EXACT output laws of the sequential algorithms (tests/exact_laws.py: the rejection
loop of negative_sampling.rs with the kept last attempt, PyG's randint negatives, products of random_walk.rs' step laws).
Their parity tests compare with NumPy restatements written from the same header text; bit parity cannot see an error the
two have in common, these one-sample tests can: a look-up in the wrong direction, an attempt too many or too few, `s == d`
applied between two node types, a draw address reused across steps, columns, mini-batches or streams.

Ids and graphs are small, the outcomes come from many mini-batches, negatives and walkers: at most N_NEG / N_WALK = 2^20
per launch, counted on the device.  Every test is deterministic (fixed seeds and call ids) and prints N, the pooled bins
and the p-value of each chi-square it runs; tests/test_exact_laws_cpu.py proves the laws by enumeration and asserts the
power of these sample sizes against the named wrong laws."""
import zlib

import numpy as np
import pytest
import torch

import exact_laws as L
from exact_laws import N_NEG, N_WALK

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEED = 0x7E57B47C
BINARY, TRIPLET = 0, 1


@pytest.fixture(scope="module")
def cabi():
    from tch_geometric import _cabi
    return _cabi


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _call_id(*key):
    """a call id of its own for every configuration: no two of them share a draw address"""
    return 1000 + (zlib.crc32(repr(key).encode()) & 0xFFFFF) * 256


def _gof(counts, probs, what):
    counts = counts.cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts, dtype=np.int64)
    probs = np.asarray(probs, dtype=np.float64).ravel()
    stat, dof, pv = L.chi2_gof(counts, probs, what)
    print("LAW %s | N = %d, %d bins, p = %.4g" % (what, int(counts.sum()), dof + 1, pv))
    return dof


def _count(cat, n_cat):
    """counts of the categories cat (any shape, device int64), every one inside [0, n_cat)"""
    cat = cat.reshape(-1)
    assert int(((cat < 0) | (cat >= n_cat)).sum()) == 0, "an outcome outside the law's categories"
    return torch.bincount(cat, minlength=n_cat)


# ---------------------------------------------------------------- link seed rows
class _Rel:
    def __init__(self, cabi, kind, density):
        self.n_src, self.n_dst = (L.LINK_N, L.LINK_N) if kind == "homo" else L.LINK_TYPED
        self.ptrs, self.idx, self.M = L.link_graph(self.n_src, self.n_dst, density, L.link_seed(kind, density))
        self.p_d, self.i_d = _t(self.ptrs), _t(self.idx)
        plain = cabi.graph_view(self.p_d, self.i_d)
        u32 = cabi.graph_view(self.p_d, self.i_d, indices32=self.i_d.to(torch.int32), ptrs32=self.p_d.to(torch.int32))
        self.views = {"search": (plain, None), "u32": (u32, None), "edge_set": (u32, cabi.edge_set(plain, DEV))}
        self.adm = {same: L.link_admissible(self.ptrs, self.idx, self.n_src, same) for same in ((0, 1) if kind == "homo" else (0,))}
        self.adm_d = {same: _t(a.ravel()) for same, a in self.adm.items()}
        es, ed = np.nonzero(self.M)
        pick = np.random.default_rng(5).integers(0, es.size, L.LINK_SHAPE[2] * L.LINK_SHAPE[0])
        shape = (L.LINK_SHAPE[2], L.LINK_SHAPE[0])
        self.pos = _t(es[pick].reshape(shape).astype(np.int64)), _t(ed[pick].reshape(shape).astype(np.int64))
        self.anchors = L.link_anchors(self.M)
        a = np.array(self.anchors, dtype=np.int64)[np.arange(shape[0]) % L.LINK_ANCHORS]
        first = np.array([np.flatnonzero(self.M[s])[0] if self.M[s].any() else 0 for s in a], dtype=np.int64)
        self.tri = _t(np.repeat(a[:, None], shape[1], 1)), _t(np.repeat(first[:, None], shape[1], 1))


@pytest.fixture(scope="module")
def rels(cabi):
    made = {}

    def get(kind, density):
        if (kind, density) not in made:
            made[(kind, density)] = _Rel(cabi, kind, density)
        return made[(kind, density)]
    return get


def _link_launch(cabi, rel, typed, same, variant, mode, tries, call_id):
    """-> (s, d [G, K E] of the negatives, unverified [G]); the positives' words are asserted here"""
    E, K, G = L.LINK_SHAPE
    assert G * K * E == N_NEG
    view, es = rel.views[variant]
    src, dst = rel.pos if mode == BINARY else rel.tri
    P = E + K * E
    if typed:
        srows, drows, unv = cabi.link_seeds_typed(view, src, dst, K, mode, tries, SEED, call_id, rel.n_src, rel.n_dst, same,
                                                  edge_set=es)
        assert torch.equal(srows[:, :E], src) and torch.equal(drows[:, :E], dst)
        s = srows[:, E:] if mode == BINARY else src.repeat_interleave(K, dim=1)
        d = drows[:, E:]
    else:
        rows, unv = cabi.link_seeds(view, src, dst, K, mode, tries, SEED, call_id, rel.n_src, edge_set=es)
        if mode == BINARY:
            r = rows.view(G, 2, P)
            assert torch.equal(r[:, 0, :E], src) and torch.equal(r[:, 1, :E], dst)
            s, d = r[:, 0, E:], r[:, 1, E:]
        else:
            assert torch.equal(rows[:, :E], src) and torch.equal(rows[:, E:2 * E], dst)
            s, d = src.repeat_interleave(K, dim=1), rows[:, 2 * E:]
    assert s.shape == d.shape == (G, K * E)
    assert int(((s < 0) | (s >= rel.n_src)).sum()) == 0, "a source outside [0, n_src)"
    assert int(((d < 0) | (d >= rel.n_dst)).sum()) == 0, "a destination outside [0, n_dst)"
    return s, d, unv


def _check_unverified(unv, bad, adm, tries, what):
    """bad [G]: the emitted negatives that are inadmissible, recounted from the CSC's matrix; unverified must equal it
    (try_count 1 counts nothing), and the total follows Binomial(N, q^tries)"""
    if tries == 1:
        assert int(unv.abs().sum()) == 0, what + ": try_count 1 makes no look-up and counts nothing"
    else:
        assert torch.equal(unv, bad), what + ": unverified[g] is not the number of inadmissible negatives of mini-batch g"
    u = int(unv.sum())
    _gof([N_NEG - u, u], L.link_unverified_law(adm, tries), what + " unverified")


def _link_cases():
    for density in L.LINK_DENSITIES:
        for tries in L.LINK_TRIES:
            for variant in ("search", "u32", "edge_set"):
                yield "homo", 0, 1, density, tries, variant
            for variant in ("search", "edge_set"):
                yield "typed", 1, 0, density, tries, variant
    for tries in (2, 8):
        yield "homo", 1, 1, 0.5, tries, "u32"                            # same_type = 1 on the square graph: the homogeneous law


@pytest.mark.parametrize("kind,typed,same,density,tries,variant", list(_link_cases()))
def test_link_binary_law(cabi, rels, kind, typed, same, density, tries, variant):
    rel = rels(kind, density)
    what = "link binary %s typed=%d same=%d density=%g tries=%d %s" % (kind, typed, same, density, tries, variant)
    s, d, unv = _link_launch(cabi, rel, typed, same, variant, BINARY, tries, _call_id(what))
    cat = s * rel.n_dst + d
    got = _count(cat, rel.n_src * rel.n_dst)
    adm = rel.adm[same]
    assert _gof(got, L.link_binary_law(rel.n_src, rel.n_dst, adm, tries), what) > 0
    if not same:                                                         # equal ids of two types: eligible unless an edge
        diag = got.view(rel.n_src, rel.n_dst).diagonal()
        assert int((diag[3:] > 0).sum()) == diag.numel() - 3, "an equal-id pair of two node types never appears"
    _check_unverified(unv, (~rel.adm_d[same][cat]).sum(1), adm, tries, what)


@pytest.mark.parametrize("kind,typed,same,density,tries,variant", list(_link_cases()))
def test_link_triplet_law(cabi, rels, kind, typed, same, density, tries, variant):
    rel = rels(kind, density)
    what = "link triplet %s typed=%d same=%d density=%g tries=%d %s" % (kind, typed, same, density, tries, variant)
    G, A = L.LINK_SHAPE[2], L.LINK_ANCHORS
    first = _call_id(what)
    got, unvs, bads = 0, [], []
    for launch in range(L.LINK_TRIPLET_LAUNCHES):                        # the second launch continues the call ids
        s, d, unv = _link_launch(cabi, rel, typed, same, variant, TRIPLET, tries, first + launch * G)
        assert torch.equal(s, rel.tri[0].repeat_interleave(L.LINK_SHAPE[1], dim=1))
        got = got + torch.stack([_count(d[i::A], rel.n_dst) for i in range(A)])
        unvs.append(unv)
        bads.append((~rel.adm_d[same][s * rel.n_dst + d]).sum(1))
    unv, bad = torch.stack(unvs), torch.stack(bads)                      # [launches, G]
    adm = rel.adm[same]
    for i, a in enumerate(rel.anchors):
        w = "%s anchor %d" % (what, a)
        dof = _gof(got[i], L.link_triplet_law(rel.n_dst, adm[a], tries), w)
        assert dof > 0 or adm[a].sum() in (0, rel.n_dst)
        N_a = int(got[i].sum())
        assert N_a == L.LINK_TRIPLET_LAUNCHES * N_NEG // A
        if tries == 1:
            assert int(unv[:, i::A].abs().sum()) == 0
        else:
            assert torch.equal(unv[:, i::A], bad[:, i::A]), w + ": unverified[g] is not the number of inadmissible negatives"
        u = int(unv[:, i::A].sum())
        _gof([N_a - u, u], L.link_unverified_law(adm[a], tries), w + " unverified")


# ---------------------------------------------------------------- skip-gram negatives
class _Walkable:
    """complete graph on 7 vertices, every edge with a timestamp of its own inside every walker's window"""

    def __init__(self, cabi):
        self.ptrs, self.col = L.complete_csr(7)
        self.p_d, self.c_d = _t(self.ptrs), _t(self.col)
        self.view = cabi.graph_view(self.p_d, self.c_d)
        self.ets = 5 + np.arange(self.col.size, dtype=np.int64)
        self.ets_d, self.nts_d = _t(self.ets), _t(np.full(7, -1, dtype=np.int64))
        self.start_ts, self.window = 5, (0, 100)


@pytest.fixture(scope="module")
def complete(cabi):
    return _Walkable(cabi)


def _typed_views(cabi, csrs):
    keep = [(_t(p), _t(c)) for p, c in csrs]
    return [cabi.graph_view(p, c) for p, c in keep], keep


def _neg_mp_graph():
    """31 x 17 bipartite pair without dead ends (the negatives test only needs walks that run)"""
    nA, nB = L.NEG_MP_COUNTS
    rs = np.random.default_rng(77)
    out = []
    for n_from, n_to in ((nA, nB), (nB, nA)):
        rows = [np.sort(rs.choice(n_to, int(rs.integers(1, 6)), replace=False)) for _ in range(n_from)]
        out.append((np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64), np.concatenate(rows).astype(np.int64)))
    return out


def _neg_launch(cabi, complete, op, seeds, call_id):
    """-> neg_rw [G, U, L] as LOCAL ids, the ranges of its columns"""
    B, R, K, G, T = L.NEG_SHAPE
    Lc = T + 1
    if op == "rw":
        _, neg = cabi.rw_skipgram(complete.view, seeds, T, Lc, R, K, 1.0, 1.0, SEED, call_id, L.NEG_NODES)
        ranges = [7] + [L.NEG_NODES] * T
    elif op == "tempo":
        cfg = cabi.tempo_skipgram_config(Lc, Lc, complete.window, R, K, L.NEG_NODES)
        _, _, neg = cabi.tempo_skipgram(complete.view, complete.nts_d, complete.ets_d, seeds,
                                        torch.full_like(seeds, complete.start_ts), cfg, SEED, call_id, with_ts=False)
        ranges = [7] + [L.NEG_NODES] * T
    else:
        views, keep = _typed_views(cabi, _neg_mp_graph())
        counts = list(L.NEG_MP_COUNTS)
        start = [0, counts[0]]
        cfg = cabi.mp_skipgram_config(views, [0, 1], [1, 0], counts, T, Lc, R, K, type_start=start, pad_value=sum(counts))
        _, neg = cabi.mp_skipgram(cfg, seeds, SEED, call_id)
        types = [0] + [(l + 1) % 2 for l in range(T)]                    # column 0 is A, column l + 1 has step_dst[l mod 2]
        neg = neg - torch.tensor([start[t] for t in types], device=DEV)  # a word carries its type's start
        ranges = [counts[t] for t in types]
    assert tuple(neg.shape) == (G, R * K * B, Lc)
    for m, n in enumerate(ranges):
        assert int(((neg[:, :, m] < 0) | (neg[:, :, m] >= n)).sum()) == 0, "column %d leaves its range [0, %d)" % (m, n)
    return neg, ranges


@pytest.mark.parametrize("op", ["rw", "mp", "tempo"])
def test_skipgram_negative_words_are_independent_uniform(cabi, complete, op):
    B, R, K, G, T = L.NEG_SHAPE
    assert G * R * K * B * T == N_NEG
    seeds = _t(np.random.default_rng(3).integers(0, 7, (G, B)).astype(np.int64))
    first = _call_id("negatives", op)
    a, ranges = _neg_launch(cabi, complete, op, seeds, first)
    b, _ = _neg_launch(cabi, complete, op, seeds, first + G)              # the next launch continues the call ids
    for x in (a, b):
        assert torch.equal(x[:, :, 0], seeds.repeat(1, R * K)), "column 0 is not the seed of row u mod B"
    what = "negatives " + op
    for m in range(1, T + 1):
        assert _gof(_count(a[:, :, m], ranges[m]), np.full(ranges[m], 1.0 / ranges[m]), "%s word %d" % (what, m)) > 0
    for m in range(1, T):
        law = L.product_uniform_law(ranges[m], ranges[m + 1])
        assert _gof(_count(a[:, :, m] * ranges[m + 1] + a[:, :, m + 1], law.size), law, "%s words %d, %d" % (what, m, m + 1)) > 0
    for n in sorted(set(ranges[1:])):                                    # the same (u, m) in two mini-batches, columns of one range
        cols = [m for m in range(1, T + 1) if ranges[m] == n]
        law = L.product_uniform_law(n, n)
        pair = lambda x, y: _count(x[:, cols] * n + y[:, cols], n * n)
        assert _gof(pair(a[0], a[1]) + pair(a[2], a[3]), law, "%s range %d mini-batches 0|1, 2|3" % (what, n)) > 0
        assert _gof(pair(a[1], a[2]), law, "%s range %d mini-batches 1|2" % (what, n)) > 0
        assert _gof(pair(a[G - 1], b[0]), law, "%s range %d last mini-batch | first of the next launch" % (what, n)) > 0


# ---------------------------------------------------------------- consecutive steps, and the walk's stream against the negatives'
def _chain_counts(x, sizes, ended=None):
    """x [N, m] columns x_1..x_m (`ended`: the value behind an ended walk) -> counts over chain_law's categories"""
    cat = torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)
    for c, s in enumerate(sizes):
        v = x[:, c] if ended is None else torch.where(x[:, c] == ended, torch.full_like(x[:, c], s), x[:, c])
        assert int(((v < 0) | (v > s)).sum()) == 0, "column %d holds neither a vertex nor the padding" % (c + 1)
        cat = cat * (s + 1) + v
    return torch.bincount(cat, minlength=int(np.prod([s + 1 for s in sizes])))


def _streams(x1, step1, word, n_word, what):
    """walker w's first step and word 1 of negative row u = w (K = 1): the product law"""
    law = np.outer(step1, np.full(n_word, 1.0 / n_word))
    assert _gof(_count(x1 * n_word + word, law.size), law, what + " x_1 | negative word 1") > 0


WALK_CASES = [("complete", 1.0, 1.0, "walk", False), ("complete", 1.0, 1.0, "skipgram", False),
              ("complete", 1.0, 1.0, "skipgram-flat", False),
              ("wedge", 0.5, 4.0, "walk", False), ("wedge", 0.5, 4.0, "walk", True),
              ("wedge", 0.5, 4.0, "skipgram", False), ("wedge", 0.5, 4.0, "skipgram", True)]


@pytest.mark.parametrize("graph,p,q,op,edge_set", WALK_CASES)
def test_random_walk_consecutive_steps_law(cabi, graph, p, q, op, edge_set):
    (ptrs, col), n = (L.complete_csr(7), 7) if graph == "complete" else (L.wedge_graph()[:2], 9)
    P, Cc = _t(ptrs), _t(col)
    g = cabi.graph_view(P, Cc)
    es = cabi.edge_set(g, DEV) if edge_set else None
    m = L.WALK_STEPS
    step = L.node2vec_step(ptrs, col, n, p, q) if p != q else L.csr_step(ptrs, col, n)
    law = L.chain_law([step] * m, 0, sizes=(n,) * m)
    what = "%s p=%g q=%g %s%s" % (graph, p, q, op, " edge set" if edge_set else "")
    B, R, G = L.WALK_SHAPE
    assert G * R * B == N_WALK
    if op == "walk":
        w = cabi.random_walk(g, torch.zeros(N_WALK, dtype=torch.int64, device=DEV), m, p, q, SEED, _call_id(what), edge_set=es)
    else:
        seeds = torch.zeros((G, B), dtype=torch.int64, device=DEV)
        pos, neg = cabi.rw_skipgram(g, seeds, m, m + 1, R, 1, p, q, SEED, _call_id(what), L.NEG_NODES, edge_set=es,
                                    form=3 if op == "skipgram-flat" else 0)
        w, neg = pos.view(N_WALK, m + 1), neg.view(N_WALK, m + 1)         # C = L: one window, the slab is the walks
        _streams(w[:, 1], step(-1, 0), neg[:, 1], L.NEG_NODES, what)
    assert tuple(w.shape) == (N_WALK, m + 1) and bool((w[:, 0] == 0).all())
    assert _gof(_chain_counts(w[:, 1:], (n,) * m, ended=-1), law, what + " x_1 x_2 x_3") > 0


def test_metapath_consecutive_steps_law(cabi):
    csrs = L.metapath_graph()
    (pa, ca), (pb, cb) = csrs
    nA, nB = L.MP_COUNTS
    views, keep = _typed_views(cabi, csrs)
    m = L.WALK_STEPS
    B, R, G = L.WALK_SHAPE
    start, dummy = [0, nA], nA + nB
    cfg = cabi.mp_skipgram_config(views, [0, 1], [1, 0], [nA, nB], m, m + 1, R, 1, type_start=start, pad_value=dummy)
    pos, neg = cabi.mp_skipgram(cfg, torch.zeros((G, B), dtype=torch.int64, device=DEV), SEED, _call_id("metapath chain"))
    w, neg = pos.view(N_WALK, m + 1), neg.view(N_WALK, m + 1)
    assert bool((w[:, 0] == 0).all()) and bool((neg[:, 0] == 0).all())
    sizes = (nB, nA, nB)
    local = w[:, 1:] - torch.tensor([start[1], start[0], start[1]], device=DEV)
    x = torch.where(w[:, 1:] == dummy, torch.tensor(sizes, device=DEV).expand_as(local), local)   # dummy_idx: the walk has ended
    steps = [L.csr_step(pa, ca, nB), L.csr_step(pb, cb, nA), L.csr_step(pa, ca, nB)]
    law = L.chain_law(steps, 0, sizes=sizes)
    assert law[L.MP_SINK, nA, nB] > 0.1                                  # the sink's walks: ended, padded in both later columns
    assert _gof(_chain_counts(x, sizes), law, "metapath A-B-A x_1 x_2 x_3") > 0
    word = neg[:, 1] - start[1]
    assert int(((word < 0) | (word >= nB)).sum()) == 0
    _streams(x[:, 0], steps[0](-1, 0), word, nB, "metapath A-B-A")


@pytest.mark.parametrize("op", ["walk", "skipgram"])
def test_temporal_walk_consecutive_steps_law(cabi, complete, op):
    g = complete
    B, R, G = L.WALK_SHAPE
    what = "temporal " + op
    if op == "walk":
        start = torch.zeros(N_WALK, dtype=torch.int64, device=DEV)
        w, ts = cabi.tempo_random_walk(g.view, g.nts_d, g.ets_d, start, torch.full_like(start, g.start_ts), 3, g.window, SEED,
                                       _call_id(what))
    else:
        seeds = torch.zeros((G, B), dtype=torch.int64, device=DEV)
        cfg = cabi.tempo_skipgram_config(3, 3, g.window, R, 1, L.NEG_NODES)
        pos, pts, neg = cabi.tempo_skipgram(g.view, g.nts_d, g.ets_d, seeds, torch.full_like(seeds, g.start_ts), cfg, SEED,
                                            _call_id(what))
        w, ts, neg = pos.view(N_WALK, 3), pts.view(N_WALK, 3), neg.view(N_WALK, 3)
    assert tuple(w.shape) == (N_WALK, 3) and bool((w[:, 0] == 0).all()) and bool((ts[:, 0] == g.start_ts).all())
    step = L.csr_step(g.ptrs, g.col, 7, L.one_slot_walk_law)
    assert _gof(_chain_counts(w[:, 1:], (7, 7)), L.chain_law([step] * 2, 0), what + " x_1 x_2") > 0
    for c in (1, 2):                                                     # rank of x_c in x_{c-1}'s row (complete, ascending)
        prev, cur = w[:, c - 1], w[:, c]
        assert bool((cur != prev).all())
        rank = cur - (cur > prev).to(torch.int64)
        assert torch.equal(ts[:, c], g.ets_d[g.p_d[prev] + rank]), "column %d's timestamp is not the taken edge's" % c
    r1, r2 = w[:, 1] - 1, w[:, 2] - (w[:, 2] > w[:, 1]).to(torch.int64)
    one = L.one_slot_walk_law(6)
    assert _gof(_count(r1 * 6 + r2, 36), np.outer(one, one), what + " ranks of steps 1, 2") > 0
    if op == "skipgram":
        _streams(w[:, 1], step(-1, 0), neg[:, 1], L.NEG_NODES, what)
