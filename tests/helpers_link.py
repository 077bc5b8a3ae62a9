"""The seed-row rule of tg_link_seeds (include/tchgeo.h) restated in NumPy and Python integers."""
import numpy as np

import orc

TAG_LINK_NEG = 13
BINARY, TRIPLET = 0, 1


def capacity(E, K, mode):
    """-> (S, P): seeds per row and (src, dst) pairs of a mini-batch of E positives with K negatives each."""
    P = E + K * E
    return (2 * P if mode == BINARY else E + P), P


def candidates(seed, call_id, u, a, n_nodes):
    """The two candidates of attempt a of negative u: floor(half * n_nodes / 2^64) of words 0,1 and of words 2,3."""
    w = orc.philox_named_draw(seed, call_id, TAG_LINK_NEG, u, a, 0)
    lo, hi = int(w[0]) | (int(w[1]) << 32), int(w[2]) | (int(w[3]) << 32)
    return (lo * int(n_nodes)) >> 64, (hi * int(n_nodes)) >> 64


def has_edge(ptrs, indices, s, d):
    """edge(s -> d): s is among indices[ptrs[d] .. ptrs[d + 1]) (sorted, as a CSC column is)."""
    b, e = int(ptrs[d]), int(ptrs[d + 1])
    k = b + int(np.searchsorted(indices[b:e], s))
    return k < e and int(indices[k]) == s


def seed_rows(ptrs, indices, src, dst, K, mode, try_count, seed, call_id, n_nodes, trace=None):
    """-> (rows [G, S], unverified [G]) for the positive edges src[G, E] -> dst[G, E]; mini-batch g draws with call id
    call_id + g.  trace: a list that receives every look-up made as (s, d)."""
    ptrs, indices = np.asarray(ptrs, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    G, E = src.shape
    S, P = capacity(E, K, mode)
    rows = np.empty((G, S), dtype=np.int64)
    unverified = np.zeros(G, dtype=np.int64)
    for g in range(G):
        if mode == BINARY:
            rows[g, :E], rows[g, P:P + E] = src[g], dst[g]
        else:
            rows[g, :E], rows[g, E:2 * E] = src[g], dst[g]
        for u in range(K * E):
            for a in range(try_count):
                c0, c1 = candidates(seed, call_id + g, u, a, n_nodes)
                s, d = (c0, c1) if mode == BINARY else (int(src[g, u // K]), c0)
                if try_count == 1:
                    break
                if s != d:
                    if trace is not None:
                        trace.append((s, d))
                    if not has_edge(ptrs, indices, s, d):
                        break
            else:
                unverified[g] += 1
            if mode == BINARY:
                rows[g, E + u], rows[g, P + E + u] = s, d
            else:
                rows[g, 2 * E + u] = d
    return rows, unverified


def pairs(rows, E, K, mode):
    """The global (src, dst) pairs [2, P] of rows [G, S] -> [G, 2, P]: positives first, then the negatives."""
    rows = np.asarray(rows)
    G = rows.shape[0]
    _, P = capacity(E, K, mode)
    if mode == BINARY:
        return rows.reshape(G, 2, P)
    src = np.concatenate([rows[:, :E], np.repeat(rows[:, :E], K, axis=1)], axis=1)
    return np.stack([src, rows[:, E:]], axis=1)


def csc_of(edges, n):
    """(ptrs, indices) of the CSC of the directed edges [(s, d)]: column d lists its sources in ascending order."""
    edges = sorted(set((int(d), int(s)) for s, d in edges))
    ptrs = np.zeros(n + 1, dtype=np.int64)
    for d, _ in edges:
        ptrs[d + 1] += 1
    return np.cumsum(ptrs), np.array([s for _, s in edges], dtype=np.int64)


def complete_graph(n=6, without_in_edges_of=None):
    """The complete directed graph on n nodes without self-loops, optionally minus every in-edge of one node."""
    return csc_of([(s, d) for s in range(n) for d in range(n) if s != d and d != without_in_edges_of], n)
