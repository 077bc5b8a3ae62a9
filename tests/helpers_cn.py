"""The rule of include/tchgeo_cn.h restated in Python sets and ints; imports nothing of the library."""
import numpy as np


def row(ptrs, indices, x):
    return [int(w) for w in indices[int(ptrs[x]):int(ptrs[x + 1])]]


def cn(ptrs, indices, u, v, cn_cap, exclude_ends=True, tables=(), n_major=None):
    """-> dict(count, cn, adjacent, score, status) of one slot: `cn` is the listed part, `score` python ints over the words
    of `tables` (sequences indexed by id)"""
    n = len(ptrs) - 1 if n_major is None else n_major
    if not (0 <= u < n and 0 <= v < n):
        return dict(count=0, cn=[], adjacent=0, score=[0] * len(tables), status=2)
    ru, rv = row(ptrs, indices, u), row(ptrs, indices, v)
    members = set(ru) & set(rv)
    if exclude_ends:
        members -= {u, v}
    members = sorted(members)
    return dict(count=len(members), cn=members[:cn_cap], adjacent=(1 if v in ru else 0) | (2 if u in rv else 0),
                score=[sum(int(t[w]) for w in members) for t in tables], status=1 if len(members) > cn_cap else 0)


def brute(edges, u, v, exclude_ends=True):
    """the members of C straight from an edge list (x -> w: w is an entry of x's row), by the definition"""
    out = []
    for w in sorted({b for _, b in edges}):
        if (u, w) in edges and (v, w) in edges and not (exclude_ends and w in (u, v)):
            out.append(w)
    return out


def distinct_degrees(ptrs, indices):
    return [len(set(row(ptrs, indices, x))) for x in range(len(ptrs) - 1)]


def table_words(degrees, kind):
    """the fixed-point words of cn_tables, by a float64 NumPy loop"""
    words = []
    for d in degrees:
        d = np.float64(d)
        w = (1.0 / np.log(d) if d >= 2 else np.float64(0)) if kind == "aa" else (1.0 / d if d >= 1 else np.float64(0))
        words.append(min(int(np.rint(w * 2.0 ** 32)), 2 ** 32 - 1))
    return words
