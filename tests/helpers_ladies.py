"""The rule of tg_ladies_count / tg_ladies_emit (include/tchgeo_ladies.h) restated in NumPy: layer-wise importance sampling
with replacement.  Integers are uint64 (sums stay below 2^63 by the rule's bounds) with an explicit 128-bit product for the
bounded pick, Philox is helpers_labor's; floating point appears only in the last step, as five single float64 operations.
Also the chunk count, the refusal rule, the workspace formula, LADIESLoader's chained layers, a brute-force dict version
and the test graphs (the reference of tests/test_ladies_cpu.py, tests/test_gpu_ladies.py and tests/test_gpu_ladies_loader.py).
Deliberately plain."""
import numpy as np

from helpers_full import CHUNK, chunk_bound, chunks_of, columns, r256, refused, status_of, table_slots  # noqa: F401
from helpers_labor import named_draw

TAG_LADIES = 18
MAX_SAMPLES = 8192
MAX_NODES = 1 << 22
SCALE_UNWEIGHTED = 1 << 40          # q = max(1, 2^40 / d^2)
SCALE_WEIGHTED = 1 << 32            # q = floor(min(x, 1)^2 * 2^32)
M32 = np.uint64(0xFFFFFFFF)
U32 = np.uint64(32)


def mulhi64(a, b):
    """floor(a * b / 2^64) of uint64 arrays by 32-bit limbs: the explicit 128-bit product"""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    a0, a1, b0, b1 = a & M32, a >> U32, b & M32, b >> U32
    lo_lo, hi_lo, lo_hi, hi_hi = a0 * b0, a1 * b0, a0 * b1, a1 * b1
    mid = (lo_lo >> U32) + (hi_lo & M32) + (lo_hi & M32)          # < 3 * 2^32
    return hi_hi + (hi_lo >> U32) + (lo_hi >> U32) + (mid >> U32)


def draw_t(seed, call_id, s, S):
    """t_j = floor(lo_j * S / 2^64) for the slots j = 0 .. s-1 of one call id (or [n_calls, s] for an array of them)"""
    call_id = np.asarray(call_id, dtype=np.uint64)
    j = np.arange(s, dtype=np.uint64)
    w = named_draw(seed, call_id[..., None], TAG_LADIES, j, 0, 0)
    lo = w[0] | (w[1] << U32)
    return mulhi64(lo, np.uint64(S))


def entry_q(weights32, length_of_entry):
    """-> (q uint64, w_e float64) per triple.  weights32: None (the row-normalised adjacency: the column's length decides)
    or the float32 weight of every triple"""
    if weights32 is None:
        d = np.asarray(length_of_entry, dtype=np.uint64)
        q = np.maximum(np.uint64(1), np.uint64(SCALE_UNWEIGHTED) // np.maximum(d * d, np.uint64(1)))
        return q, 1.0 / d.astype(np.float64)
    x = np.asarray(weights32, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = x > 0                                                 # false for a NaN
        y = np.where(ok, np.minimum(x, 1.0), 0.0)
    return np.floor(y * y * float(SCALE_WEIGHTED)).astype(np.uint64), x


def _lookup(keys, values, queries):
    """values[i] where queries equal the ascending keys[i], -1 elsewhere"""
    if not keys.size:
        return np.full(queries.shape, -1, dtype=np.int64)
    at = np.minimum(np.searchsorted(keys, queries), keys.size - 1)
    return np.where(keys[at] == queries, values[at], -1).astype(np.int64)


class Prepared:
    """everything of a batch that does not depend on the draws"""


def prepare(ptrs, indices, weights, nodes, n_major=None, id_bound=None):
    ptrs, indices, nodes = (np.asarray(a, dtype=np.int64) for a in (ptrs, indices, nodes))
    p = Prepared()
    p.nodes, p.n = nodes, nodes.size
    begin, length = columns(ptrs, nodes, n_major)
    p.m = m = int(length.sum())
    p.cols = np.repeat(np.arange(p.n, dtype=np.int64), length)
    before = np.cumsum(length) - length
    p.edge_index = np.arange(m, dtype=np.int64) - np.repeat(before, length) + np.repeat(begin, length)
    p.src = indices[p.edge_index]
    p.status = status_of(ptrs, nodes, n_major)
    p.chunks = int((-(-length // CHUNK)).sum())
    q, p.w_e = entry_q(None if weights is None else np.asarray(weights, dtype=np.float32)[p.edge_index], np.repeat(length, length))
    ids, first, inv = np.unique(p.src, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                       # candidates by first occurrence in triple order
    rank = np.empty(order.size, dtype=np.int64)
    rank[order] = np.arange(order.size)
    p.cand = ids[order]
    p.inv = rank[inv.reshape(-1)] if m else np.zeros(0, np.int64)  # the candidate of every triple
    p.W = np.zeros(p.cand.size, dtype=np.uint64)
    np.add.at(p.W, p.inv, q)
    p.P = np.cumsum(p.W, dtype=np.uint64) - p.W
    p.S = int(p.W.sum(dtype=np.uint64))
    # the first frontier position of every candidate and the candidate of every frontier position, -1 for none (a
    # frontier id outside [0, id_bound) equals no source)
    bound = (ptrs.size - 1 if n_major is None else n_major) if id_bound is None else id_bound
    fid, fpos = np.unique(nodes, return_index=True)
    keep = (fid >= 0) & (fid < bound)
    p.cand_pos = _lookup(fid[keep], fpos[keep], p.cand)
    by_id = np.argsort(p.cand, kind="stable")
    p.node_cand = np.where((nodes >= 0) & (nodes < bound), _lookup(p.cand[by_id], by_id, nodes), -1)
    return p


def select(p, t):
    """the candidate every pick selects: the last one with P <= t (one of W = 0 shares its P with its successor)"""
    t = np.asarray(t, dtype=np.uint64)
    sel = np.searchsorted(p.P, t, side="right") - 1
    assert (p.W[sel] > 0).all() and (p.P[sel] <= t).all() and (t - p.P[sel] < p.W[sel]).all()
    return sel


def finish(p, s, t, sel=None):
    """the outputs of a prepared batch under the picks t [s] (or the selection they make) -> dict of every output word"""
    n, nc = p.n, p.cand.size
    status = p.status
    c = np.zeros(nc, dtype=np.int64)
    new = np.zeros(0, dtype=np.int64)
    pos = p.cand_pos.copy()
    if nc and p.S == 0:
        status |= 4
    if nc and p.S:
        sel = select(p, t) if sel is None else sel
        c = np.bincount(sel, minlength=nc).astype(np.int64)
        drawn, first_slot = np.unique(sel, return_index=True)
        fresh = p.cand_pos[drawn] < 0
        new = drawn[fresh][np.argsort(first_slot[fresh], kind="stable")]               # by the first selecting slot
        pos[new] = n + np.arange(new.size)
    out_nodes = np.concatenate([p.nodes, p.cand[new]])
    who = np.concatenate([p.node_cand, new]).astype(np.int64)      # the candidate at every position of out_nodes
    node_count = np.where(who >= 0, c[np.maximum(who, 0)] if nc else 0, 0).astype(np.int64)
    node_weight = np.where(who >= 0, p.W[np.maximum(who, 0)].astype(np.int64) if nc else 0, 0).astype(np.int64)
    kept = c[p.inv] > 0 if p.m else np.zeros(0, bool)
    u = p.inv[kept]
    ew = ((c[u].astype(np.float64) * np.float64(p.S)) / (np.float64(s) * p.W[u].astype(np.float64))) * p.w_e[kept]
    return dict(out_nodes=out_nodes, node_count=node_count, node_weight=node_weight, rows=pos[u], cols=p.cols[kept],
                edge_index=p.edge_index[kept], edge_weight=ew.astype(np.float32), total=p.S, n_cand=nc, status=status,
                chunks=p.chunks, m=p.m, n=n)


def ladies_rule(ptrs, indices, weights, nodes, s, seed, call_id, n_major=None, id_bound=None):
    """one batch: weights None or float32 per CSC entry -> dict(out_nodes, node_count, node_weight, rows, cols, edge_index,
    edge_weight (float32), total, n_cand, status, chunks, m, n)"""
    p = prepare(ptrs, indices, weights, nodes, n_major, id_bound)
    return finish(p, s, draw_t(seed, call_id, s, p.S) if p.S else None)


def blocks(ptrs, indices, weights, seeds, num_samples, seed, call_id):
    """LADIESLoader's layers for one mini-batch, layer 0 first -> [(n_id, n_dst, rows, cols, csc offsets, edge_weight)]: F_0 =
    the seeds, layer l draws under call id call_id + l, F_{l+1} = its out_nodes"""
    out, frontier = [], np.asarray(seeds, dtype=np.int64)
    for l, s in enumerate(num_samples):
        r = ladies_rule(ptrs, indices, weights, frontier, s, seed, call_id + l)
        out.append((r["out_nodes"], frontier.size, r["rows"], r["cols"], r["edge_index"], r["edge_weight"]))
        frontier = r["out_nodes"]
    return out


def brute_force(ptrs, indices, weights, nodes, s, t, n_major=None):
    """the rule with dicts, Python integers and loops, under given picks t -> the same dict as finish() (without chunks)"""
    n_major = len(ptrs) - 1 if n_major is None else n_major
    W, order, triples, status = {}, [], [], 0
    for i, v in enumerate(nodes):
        v = int(v)
        if not 0 <= v < n_major:
            status |= 2
            continue
        d = int(ptrs[v + 1] - ptrs[v])
        for e in range(int(ptrs[v]), int(ptrs[v + 1])):
            u = int(indices[e])
            if weights is None:
                q, w_e = max(1, SCALE_UNWEIGHTED // (d * d)), 1.0 / float(d)
            else:
                x = float(np.float32(weights[e]))
                q = int(np.floor(min(x, 1.0) ** 2 * SCALE_WEIGHTED)) if x > 0 else 0
                w_e = x
            if u not in W:
                W[u] = 0
                order.append(u)
            W[u] += q
            triples.append((u, i, e, w_e))
    S = sum(W.values())
    c, first_slot = {u: 0 for u in order}, {}
    if order and S == 0:
        status |= 4
    if order and S:
        for j in range(s):
            acc = 0
            for u in order:
                if acc <= int(t[j]) < acc + W[u]:
                    c[u] += 1
                    first_slot.setdefault(u, j)
                acc += W[u]
    front = {}
    for i, v in enumerate(nodes):
        front.setdefault(int(v), i)
    new = sorted((u for u in first_slot if u not in front), key=lambda u: first_slot[u])
    out_nodes = [int(v) for v in nodes] + new
    pos = dict(front)
    for r, u in enumerate(new):
        pos[u] = len(nodes) + r
    kept = [(u, i, e, w) for u, i, e, w in triples if c[u] > 0]
    ew = [np.float32(((float(c[u]) * float(S)) / (float(s) * float(W[u]))) * w) for u, _, _, w in kept]
    return dict(out_nodes=np.array(out_nodes, np.int64), node_count=np.array([c.get(u, 0) for u in out_nodes], np.int64),
                node_weight=np.array([W.get(u, 0) for u in out_nodes], np.int64),
                rows=np.array([pos[u] for u, _, _, _ in kept], np.int64), cols=np.array([i for _, i, _, _ in kept], np.int64),
                edge_index=np.array([e for _, _, e, _ in kept], np.int64), edge_weight=np.array(ew, np.float32), total=S,
                n_cand=len(order), status=status, m=len(triples), n=len(nodes))


def same(a, b, keys=("out_nodes", "node_count", "node_weight", "rows", "cols", "edge_index", "total", "n_cand", "status", "m", "n")):
    """two result dicts agree in every word (edge_weight as bits)"""
    for k in keys:
        if not np.array_equal(a[k], b[k]):
            return False
    return np.array_equal(np.asarray(a["edge_weight"], np.float32).view(np.uint32), np.asarray(b["edge_weight"], np.float32).view(np.uint32))


def workspace_bytes(n_edges, max_nodes, node_cap, chunk_cap, id_bound, s):
    """one batch of the pair's workspace, the header's formula"""
    key = 4 if id_bound <= 1 << 31 else 8
    T, C = table_slots(node_cap), chunk_bound(max_nodes, n_edges, chunk_cap)
    tiles = -(-max_nodes // 1024) if max_nodes else 1
    t = C // 1024 + 1
    return (256 + r256(T * key) + 3 * r256(4 * T) + r256(8 * T) + 2 * r256(8 * (max_nodes + 1)) + r256(8 * max_nodes)
            + r256(16 * tiles) + 2 * r256(4 * (C + 1)) + r256(8 * (C + 1)) + 2 * r256(4 * t) + r256(8 * t)
            + r256(4 * node_cap) + r256(8 * node_cap) + r256(4 * s))


# ---- the test graph of tests/test_gpu_ladies.py and the loader tests ------------------------------------------------------
N = 1200
HUB, EMPTY0, EMPTY1 = 0, 400, 480


def ladies_test_graph():
    """-> (ptrs, indices): a hub column of six chunks whose sources repeat across its chunks and reappear in other columns,
    a run of 80 empty columns, self loops, parallel edges and sources that are frontier nodes; properties asserted"""
    rs = np.random.default_rng(11)
    cols = []
    for v in range(N):
        cols.append(np.zeros(0, np.int64) if EMPTY0 <= v < EMPTY1 else rs.integers(0, N, int(rs.integers(0, 41))))
    cols[HUB] = 100 + (np.arange(2600) * 7) % 300                # sources 100 .. 399, each eight or nine times, in every chunk
    cols[1] = np.array([1, 1, 0, 150, 150, 2])                   # a self loop twice (parallel), frontier nodes, a hub source twice
    cols[2] = np.array([2, 1, 0, 399])
    ptrs = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int64)
    indices = np.concatenate(cols).astype(np.int64)
    hub = indices[ptrs[HUB]:ptrs[HUB + 1]]
    assert -(-hub.size // CHUNK) == 6
    chunk_of_first = {}
    across = [s for j, s in enumerate(hub.tolist()) if chunk_of_first.setdefault(s, j // CHUNK) != j // CHUNK]
    assert len(set(across)) == 300                               # every hub source is seen again in a later chunk
    assert 150 in hub and 150 in indices[ptrs[1]:ptrs[2]]        # ... and reappears in another column
    assert (np.diff(ptrs)[EMPTY0:EMPTY1] == 0).all() and EMPTY1 - EMPTY0 == 80
    col1 = indices[ptrs[1]:ptrs[2]].tolist()
    assert col1.count(1) == 2 and col1.count(150) == 2           # a self loop; parallel edges
    assert 0 in col1 and 2 in col1                               # sources that are frontier nodes (frontier_order leads with 0, 1, 2)
    return ptrs, indices


def frontier_order():
    """the hub, columns 1 and 2, the empty run, then the rest shuffled: prefixes of it are the frontiers of the tests"""
    rest = [v for v in np.random.default_rng(5).permutation(N).tolist() if v > 2 and not EMPTY0 <= v < EMPTY1]
    return np.array([HUB, 1, 2] + list(range(EMPTY0, EMPTY1)) + rest, dtype=np.int64)


NESTED_LENGTHS = (1, 2, 3, 4, 6, 12)


def nested_graph():
    """12 nodes; column i < 6 holds the sources 0 .. d_i - 1 for d = 1, 2, 3, 4, 6, 12 (nested), the others are empty.
    -> (ptrs, indices, law): law[u] = W_u / S of the frontier 0 .. 5 as exact fractions of Python integers"""
    from fractions import Fraction
    cols = [np.arange(d, dtype=np.int64) for d in NESTED_LENGTHS] + [np.zeros(0, np.int64)] * 6
    ptrs = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int64)
    W = [sum(max(1, SCALE_UNWEIGHTED // (d * d)) for d in NESTED_LENGTHS if d > u) for u in range(12)]
    S = sum(W)
    return ptrs, np.concatenate(cols), [Fraction(w, S) for w in W]
