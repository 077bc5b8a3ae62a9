"""The seed-row rule of tg_link_seeds_typed (include/tchgeo.h) restated in NumPy and Python integers: tg_link_seeds' law
with two id ranges, `s == d` rejected only when both endpoints are one node type, and two rows per mini-batch."""
import numpy as np

import helpers_link as hl
import orc

BINARY, TRIPLET = hl.BINARY, hl.TRIPLET


def widths(E, K, mode):
    """-> (Ws, Wd): words of the source and of the destination row of a mini-batch of E positives, K negatives each."""
    P = E + K * E
    return (P if mode == BINARY else E), P


def candidates(seed, call_id, u, a, n_src, n_dst, mode):
    """(s, d) candidates of attempt a of negative u; triplet: s is None (the positive's source) and d comes from words 0,1"""
    w = orc.philox_named_draw(seed, call_id, hl.TAG_LINK_NEG, u, a, 0)
    lo, hi = int(w[0]) | (int(w[1]) << 32), int(w[2]) | (int(w[3]) << 32)
    if mode == BINARY:
        return (lo * int(n_src)) >> 64, (hi * int(n_dst)) >> 64
    return None, (lo * int(n_dst)) >> 64


def seed_rows(ptrs, indices, src, dst, K, mode, try_count, seed, call_id, n_src, n_dst, same_type, trace=None, first=None):
    """-> (src rows [G, Ws], dst rows [G, Wd], unverified [G]) for the positive edges src[G, E] -> dst[G, E] of a relation
    whose CSC (n_dst columns, row ids < n_src) is (ptrs, indices); mini-batch g draws with call id call_id + g.
    trace: a list that receives every look-up made as (s, d); first: one that receives attempt 0's (s, d) per negative."""
    ptrs, indices = np.asarray(ptrs, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    assert len(ptrs) - 1 == n_dst and (not same_type or n_src == n_dst)
    G, E = src.shape
    Ws, Wd = widths(E, K, mode)
    srows, drows = np.empty((G, Ws), dtype=np.int64), np.empty((G, Wd), dtype=np.int64)
    unverified = np.zeros(G, dtype=np.int64)
    for g in range(G):
        srows[g, :E], drows[g, :E] = src[g], dst[g]
        for u in range(K * E):
            for a in range(try_count):
                s, d = candidates(seed, call_id + g, u, a, n_src, n_dst, mode)
                if mode == TRIPLET:
                    s = int(src[g, u // K])
                if a == 0 and first is not None:
                    first.append((s, d))
                if try_count == 1:
                    break
                if not (same_type and s == d):
                    if trace is not None:
                        trace.append((s, d))
                    if not hl.has_edge(ptrs, indices, s, d):
                        break
            else:
                unverified[g] += 1
            if mode == BINARY:
                srows[g, E + u] = s
            drows[g, E + u] = d
    return srows, drows, unverified


def joined(srows, drows):
    """tg_link_seeds' row: the destination row directly behind the source row"""
    return np.concatenate([srows, drows], axis=1)


def pairs(srows, drows, E, K, mode):
    """The global (src, dst) pairs [G, 2, P]: positives first, then the negatives (triplet: the source repeated K times)."""
    if mode == BINARY:
        return np.stack([srows, drows], axis=1)
    return np.stack([np.concatenate([srows, np.repeat(srows, K, axis=1)], axis=1), drows], axis=1)


def rect_csc(edges, n_dst):
    """(ptrs, indices) of the CSC of the directed edges [(s, d)] of a relation with n_dst destinations"""
    return hl.csc_of(edges, n_dst)


def complete_bipartite(n_src=3, n_dst=5, without_in_edges_of=None):
    return rect_csc([(s, d) for s in range(n_src) for d in range(n_dst) if d != without_in_edges_of], n_dst)


def tiny_relation():
    """6 destinations x 8 sources (a column of seven distinct sources needs eight of them): column 0 is empty, column 1 has
    one entry, the others two, three, two and seven, with source ids below and above their ends -> (ptrs, indices)"""
    cols = {1: [3], 2: [3, 5], 3: [1, 2, 6], 4: [2, 6], 5: [0, 1, 2, 3, 4, 5, 7]}
    return rect_csc([(s, d) for d, ss in cols.items() for s in ss], 6)


TINY_N_SRC, TINY_N_DST = 8, 6


def empty_relation(n_dst=2):
    return np.zeros(n_dst + 1, dtype=np.int64), np.zeros(0, dtype=np.int64)


def fold(row, col, n_src, n_dst):
    """edges (row, col) folded into an n_src x n_dst relation, as distinct (s, d) pairs -> its CSC"""
    return rect_csc(set(zip((np.asarray(row) % n_src).tolist(), (np.asarray(col) % n_dst).tolist())), n_dst)


def positives(ptrs, indices, G, E):
    """[G, E] edges of the relation (CSC positions drawn with a fixed generator) as (src, dst); of an empty relation: zeros"""
    if len(indices) == 0:
        return np.zeros((G, E), dtype=np.int64), np.zeros((G, E), dtype=np.int64)
    r = np.random.default_rng(1000 * G + E)
    pos = r.integers(0, len(indices), (G, E))
    return np.asarray(indices)[pos].astype(np.int64), (np.searchsorted(ptrs, pos, side="right") - 1).astype(np.int64)
