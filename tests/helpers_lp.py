"""NumPy restatement of the balanced label-propagation partitioner (the rule: include/tchgeo_lp.h): propose, commit and a
chained run, with helpers_labor's Philox.  Deliberately plain."""
import math

import numpy as np

from helpers_labor import named_draw

TAG_LP = 20
STAY = np.uint64(0xFFFFFFFFFFFFFFFF)


def propose(ptrs, idx, label, P, seed, rnd):
    """-> (skey uint64 [n], cut_entries)"""
    ptrs, idx, label = np.asarray(ptrs, dtype=np.int64), np.asarray(idx, dtype=np.int64), np.asarray(label, dtype=np.int64)
    n = len(ptrs) - 1
    v = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptrs))
    ok = (idx >= 0) & (idx < n) & (idx != v)
    v, l = v[ok], label[idx[ok]]
    cut = int((l != label[v]).sum())
    pair, cnt = np.unique(v * P + l, return_counts=True)             # (v, l) ascending with its count
    pv, pl = pair // P, pair % P
    own = np.zeros(n, dtype=np.int64)
    mine = pl == label[pv]
    own[pv[mine]] = cnt[mine]
    pv, pl, cnt = pv[~mine], pl[~mine], cnt[~mine]
    order = np.lexsort((pl, -cnt, pv))                               # per v: the larger count, then the smaller label
    pv, pl, cnt = pv[order], pl[order], cnt[order]
    first = np.ones(len(pv), dtype=bool)
    first[1:] = pv[1:] != pv[:-1]
    pv, pl, cnt = pv[first], pl[first], cnt[first]
    gain = cnt - own[pv]
    pv, pl, gain = pv[gain > 0], pl[gain > 0], gain[gain > 0]
    h = named_draw(seed, rnd, TAG_LP, pv, 0, 0)[0]
    skey = np.full(n, STAY, dtype=np.uint64)
    skey[pv] = (pl.astype(np.uint64) << np.uint64(44)) | ((4095 - np.minimum(gain, 4095)).astype(np.uint64) << np.uint64(32)) | h
    return skey, cut


def commit(label, size, cap, skey, P):
    """-> (label, size, moved, status): new arrays"""
    label, size, skey = np.array(label, dtype=np.int64), np.array(size, dtype=np.int64), np.asarray(skey, dtype=np.uint64)
    free = np.maximum(0, cap - size)
    v = np.nonzero(skey != STAY)[0]
    target = (skey[v] >> np.uint64(44)).astype(np.int64)
    status = 2 if (target >= P).any() else 0
    v, target = v[target < P], target[target < P]
    order = np.lexsort((v, skey[v]))
    v, target = v[order], target[order]
    start = np.searchsorted(target, target, side="left")             # the first place of each one's target
    admitted = np.arange(len(v)) - start < free[target]
    v, target = v[admitted], target[admitted]
    np.subtract.at(size, label[v], 1)
    np.add.at(size, target, 1)
    label[v] = target
    return label, size, len(v), status


def cap_of(n, P, slack):
    return max(1, math.ceil(slack * n / P))


def run(ptrs, idx, init, P, slack, rounds, seed):
    """the chained run of lp_partition -> (label, dict(cut, moved, sizes, cap))"""
    label = np.asarray(init, dtype=np.int64)
    size, cap = np.bincount(label, minlength=P).astype(np.int64), cap_of(len(label), P, slack)
    cuts, moves = [], []
    for r in range(rounds):
        skey, cut = propose(ptrs, idx, label, P, seed, r)
        label, size, moved, _ = commit(label, size, cap, skey, P)
        cuts.append(cut)
        moves.append(moved)
    return label, dict(cut=cuts, moved=moves, sizes=size, cap=cap)


def csr(n, rows, cols):
    """rows of the entries (rows[i], cols[i]), ascending inside a row as tg_coo_to_csx leaves them"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    order = np.lexsort((cols, rows))
    return np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64), cols[order]


def planted(n=4000, k=16, intra=10, inter=2, seed=1):
    """The planted-partition graph: k communities of n / k scattered vertices; every vertex draws `intra` entries inside
    its community and `inter` outside, and every entry stands in both rows -> (ptrs, idx)"""
    rs = np.random.default_rng(seed)
    comm = rs.permutation(n) % k
    members = [np.nonzero(comm == c)[0] for c in range(k)]
    src, dst = [], []
    for u in range(n):
        inside = rs.choice(members[comm[u]], intra)
        outside = rs.integers(0, n, 4 * inter)
        outside = outside[comm[outside] != comm[u]][:inter]
        dst += [inside, outside]
        src.append(np.full(len(inside) + len(outside), u))
    src, dst = np.concatenate(src), np.concatenate(dst)
    return csr(n, np.concatenate([src, dst]), np.concatenate([dst, src]))
