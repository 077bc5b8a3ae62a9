"""GraphSAINT's node and edge samplers restated in NumPy (the reference of tests/test_saint_ne_cpu.py, test_gpu_saint_ne.py
and test_gpu_saint_ne_loader.py; include/tchgeo.h at tg_saint_node_nodes / tg_saint_edge_nodes).  It does not import the
library.  The draws are helpers_labor.named_draw's, a mini-batch's node list is helpers_saint.node_list over a walk-shaped
matrix ([B, 1] for nodes, [B, 2] = (source, target) for edges: its step-major positions are exactly i and B + i), and the
exact laws of both samplers stand beside it.  Deliberately plain."""
import numpy as np

from helpers_labor import named_draw
from helpers_saint import node_list

TAG_SAINT_NODE, TAG_SAINT_EDGE = 16, 17
STATUS_RANGE, STATUS_EMPTY = 2, 4


def bounded(x, n):
    """floor(x * n / 2^64) in exact integers; x: uint64 array, n: an int or an int array of x's shape -> int64 array"""
    n = n if np.isscalar(n) else np.asarray(n).astype(object)
    return ((np.asarray(x).astype(object) * n) >> 64).astype(np.int64)


def slot_draws(seed, call_id, G, B, tag):
    """-> (lo, hi) uint64 [G, B]: slot i of mini-batch g takes the draw (seed, call_id + g, tag, id = i, 0, 0); lo = w0 |
    w1 << 32, hi = w2 | w3 << 32"""
    cid = (np.uint64(call_id) + np.arange(G, dtype=np.uint64))[:, None]
    w = named_draw(seed, cid, tag, np.arange(B, dtype=np.uint64)[None, :], 0, 0)
    s = np.uint64(32)
    return w[0] | (w[1] << s), w[2] | (w[3] << s)


def node_draws(indices, G, B, seed, call_id, id_bound):
    """-> (v [G, B] int64, refused [G, B] bool, status): slot i visits indices[floor(lo * E / 2^64)]; a value outside
    [0, id_bound) is refused (status bit 1)"""
    indices = np.asarray(indices, dtype=np.int64)
    lo, _ = slot_draws(seed, call_id, G, B, TAG_SAINT_NODE)
    v = indices[bounded(lo, int(indices.size))]
    refused = (v < 0) | (v >= id_bound)
    return v, refused, STATUS_RANGE if refused.any() else 0


def edge_draws(csc, cols, csr, rows, G, B, seed, call_id, id_bound):
    """csc / csr: (ptrs, indices) (csr None with empty rows); cols / rows: the listed majors.  -> (src [G, B], dst [G, B],
    refused [G, B] bool, status).  t = floor(lo * (n_cols + n_rows) / 2^64) picks the list entry, k = floor(hi * deg / 2^64)
    the entry of that column (source = indices word, target = the column) or row (source = the row, target = indices word).
    Refused: a major outside its graph (bit 1), a major without entries (bit 2), an end outside [0, id_bound) (bit 1)."""
    cols, rows = np.asarray(cols, dtype=np.int64), np.asarray(rows, dtype=np.int64)
    lo, hi = slot_draws(seed, call_id, G, B, TAG_SAINT_EDGE)
    t = bounded(lo, int(cols.size + rows.size))
    side = t >= cols.size
    major = np.where(side, rows[np.clip(t - cols.size, 0, max(rows.size - 1, 0))] if rows.size else 0,
                     cols[np.clip(t, 0, max(cols.size - 1, 0))] if cols.size else 0)
    src, dst = np.zeros((G, B), dtype=np.int64), np.zeros((G, B), dtype=np.int64)
    refused, status = np.zeros((G, B), dtype=bool), 0
    for s, graph in ((False, csc), (True, csr)):
        mine = side == s
        if not mine.any():
            continue
        ptrs, idx = (np.asarray(a, dtype=np.int64) for a in graph)
        inside = mine & (major >= 0) & (major < ptrs.size - 1)
        safe = np.where(inside, major, 0)
        deg = np.where(inside, ptrs[np.minimum(safe + 1, ptrs.size - 1)] - ptrs[safe], 0)
        live = inside & (deg > 0)
        if (mine & ~inside).any():
            status |= STATUS_RANGE
        if (inside & ~live).any():
            status |= STATUS_EMPTY
        other = np.zeros((G, B), dtype=np.int64)
        other[live] = idx[ptrs[safe[live]] + bounded(hi[live], deg[live])]
        bad = live & ((major >= id_bound) | (other < 0) | (other >= id_bound))
        if bad.any():
            status |= STATUS_RANGE
        refused |= mine & (~live | bad)
        src[mine] = (major if s else other)[mine]
        dst[mine] = (other if s else major)[mine]
    return src, dst, refused, status


def lists_of(columns, refused):
    """node lists of G mini-batches from their walk-shaped matrices: columns = (v,) or (src, dst), each [G, B]"""
    return [node_list(np.stack([c[g] for c in columns], axis=1), skip=np.flatnonzero(refused[g]))
            for g in range(refused.shape[0])]


def node_lists(indices, G, B, seed, call_id, id_bound):
    """-> (lists, status): tg_saint_node_nodes"""
    v, refused, status = node_draws(indices, G, B, seed, call_id, id_bound)
    return lists_of((v,), refused), status


def edge_lists(csc, cols, csr, rows, G, B, seed, call_id, id_bound):
    """-> (lists, status): tg_saint_edge_nodes"""
    src, dst, refused, status = edge_draws(csc, cols, csr, rows, G, B, seed, call_id, id_bound)
    return lists_of((src, dst), refused), status


def nonempty(ptrs):
    """the majors with entries: what the edge loader lists"""
    return np.flatnonzero(np.diff(np.asarray(ptrs, dtype=np.int64)) > 0).astype(np.int64)


# ---------------------------------------------------------------- the exact laws
def node_law(indices, n):
    """P(a slot visits v) = (entries that hold v) / E"""
    indices = np.asarray(indices, dtype=np.int64)
    return np.bincount(indices, minlength=n) / float(indices.size)


def edge_entry_law(csc_ptrs, csc_idx, cols, rows, n_rows):
    """per CSC ENTRY e = (u -> v) (u = csc_idx[e], v its column; parallel entries count separately):
    P(e) = (times v is listed in cols / deg_in(v) + times u is listed in rows / deg_out(u)) / (n_cols + n_rows).  With
    the lists = the non-empty columns and rows that is (1 / deg_in(v) + 1 / deg_out(u)) / (n_cols + n_rows)."""
    csc_ptrs, csc_idx = np.asarray(csc_ptrs, dtype=np.int64), np.asarray(csc_idx, dtype=np.int64)
    n_cols = csc_ptrs.size - 1
    deg_in = np.diff(csc_ptrs)
    deg_out = np.bincount(csc_idx, minlength=n_rows)
    col_of = np.repeat(np.arange(n_cols), deg_in)
    listed_c = np.bincount(np.asarray(cols, dtype=np.int64), minlength=n_cols)
    listed_r = np.bincount(np.asarray(rows, dtype=np.int64), minlength=n_rows)
    m = float(len(cols) + len(rows))
    return (listed_c[col_of] / deg_in[col_of] + listed_r[csc_idx] / deg_out[csc_idx]) / m


def uniform_entry_law(csc_idx):
    """named wrong law: every entry alike"""
    e = np.asarray(csc_idx).size
    return np.full(e, 1.0 / e)


def pair_categories(csc_ptrs, csc_idx):
    """-> (cat [E], pairs [n_cat, 2]): the (source, target) pair of every CSC entry as a category id; parallel entries share
    one"""
    csc_ptrs, csc_idx = np.asarray(csc_ptrs, dtype=np.int64), np.asarray(csc_idx, dtype=np.int64)
    col_of = np.repeat(np.arange(csc_ptrs.size - 1), np.diff(csc_ptrs))
    pairs, cat = np.unique(np.stack([csc_idx, col_of], axis=1), axis=0, return_inverse=True)
    return cat.reshape(-1), pairs


def merged(entry_probs, cat, n_cat):
    """the pair law of an entry law: parallel entries merged by adding their probabilities"""
    return np.bincount(cat, weights=entry_probs, minlength=n_cat)


def pair_law_by_enumeration(csc, cols, csr, rows, k_from_lo=False):
    """The law of (source, target) by exhausting t and k: list entry t has probability 1 / M, entry k of its major 1 / deg.
    k_from_lo=True is the named wrong law where k is made from the SAME 64 bits as t (exact_laws.shared_draw_pair_law's
    construction): u in [t / M, (t + 1) / M) gives k = floor(u * deg), a cell's probability the length of the
    intersection of its two intervals.  -> {(source, target): probability}"""
    from fractions import Fraction
    cols, rows = [int(c) for c in cols], [int(r) for r in rows]
    M = len(cols) + len(rows)
    law = {}
    for t in range(M):
        side = t >= len(cols)
        major = rows[t - len(cols)] if side else cols[t]
        ptrs, idx = csr if side else csc
        b, e = int(ptrs[major]), int(ptrs[major + 1])
        d = e - b
        for k in range(d):
            if k_from_lo:
                w = min(Fraction(t + 1, M), Fraction(k + 1, d)) - max(Fraction(t, M), Fraction(k, d))
                w = max(w, Fraction(0))
            else:
                w = Fraction(1, M * d)
            other = int(idx[b + k])
            key = (major, other) if side else (other, major)
            law[key] = law.get(key, Fraction(0)) + w
    return law


def law_vector(law, pairs):
    """a {(source, target): p} law over the categories `pairs` [n_cat, 2]; every key must be a category"""
    index = {(int(u), int(v)): i for i, (u, v) in enumerate(pairs)}
    out = np.zeros(len(pairs))
    for key, p in law.items():
        out[index[key]] += float(p)
    return out


def law_graph():
    """The graph of the law tests: 20 vertices, skewed in- and out-degrees that differ per vertex (so the column term, the
    row term and the uniform law all disagree), self loops, parallel edges, a sink (18), a vertex without in-edges (17) and
    an isolated vertex (19).  Small enough that every (source, target) pair expects well over exact_laws.MIN_EXPECTED
    draws out of 2^16.  -> (edge_index [2, E], n)"""
    n = 20
    rs = np.random.default_rng(20)
    w_out = np.array([9, 1, 6, 2, 8, 1, 5, 3, 7, 2, 4, 1, 6, 2, 3, 1, 2, 5, 0, 0], dtype=np.float64)
    w_in = np.array([1, 8, 2, 7, 1, 9, 3, 5, 2, 6, 1, 4, 2, 6, 1, 3, 5, 0, 4, 0], dtype=np.float64)
    src = rs.choice(n, 150, p=w_out / w_out.sum())
    dst = rs.choice(n, 150, p=w_in / w_in.sum())
    src[:3] = dst[:3] = (0, 2, 4)                           # self loops
    src[3:8], dst[3:8] = src[8:13], dst[8:13]               # parallel edges
    return np.stack([src, dst]).astype(np.int64), n
