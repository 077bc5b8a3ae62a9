"""NumPy restatement of tg_pinsage_hop (include/tchgeo.h at the declaration) and of PinSAGELoader's layer composition: the
termination draws on top of a walk matrix, the selection of the most visited vertices, the blocks of a mini-batch.  The
walks themselves are tg_random_walk's (the hop's contract: without termination walker w is row w of that call), so the
device tests take them from _cabi.random_walk and the CPU tests from any matrix with -1 padding.  Deliberately plain."""
from collections import Counter

import numpy as np

from helpers_labor import named_draw

TAG_PINSAGE = 15


def uniform01(w):
    """u32_to_f32_01 of the 32-bit words w (held in any integer type) -> float32 in [0, 1)"""
    w = (np.asarray(w, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return ((w >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1)


def ends_before(seed, call_id, walker, step, alpha, tag=TAG_PINSAGE, bits=32):
    """True where walker `walker` ends before step `step` >= 1: uniform(draw(call key of (seed, call id, tag), walker, step,
    0).w[0]) < alpha.  bits < 32 keeps only the top `bits` of the word (the negative control of the law test)."""
    w = named_draw(seed, call_id, tag, walker, step, 0)[0]
    if bits < 32:
        w = (w >> np.uint64(32 - bits)) << np.uint64(32 - bits)
    return uniform01(w) < np.float32(alpha)


def truncate(walks, seed, call_id, R, alpha, ids=None, tag=TAG_PINSAGE, bits=32):
    """walks [W, T + 1]: row w = walker w of tg_random_walk (column 0 the start, -1 behind a dead end).  Slot i has draw
    id ids[i] (None: i) and call id call_id[i] (or the scalar); its walk r is walker ids[i] * R + r.  -> [m * R, T + 1] in
    SLOT order (row i * R + r), every walk cut where its termination draw says so: the first step is always taken, before
    step l >= 1 (which fills column l + 1) the walk ends if the uniform is below alpha; what follows is -1."""
    walks = np.asarray(walks, dtype=np.int64)
    T = walks.shape[1] - 1
    m = walks.shape[0] // R if ids is None else len(ids)
    ids = np.arange(m, dtype=np.uint64) if ids is None else np.asarray(ids).astype(np.uint64)
    walker = (ids[:, None] * np.uint64(R) + np.arange(R, dtype=np.uint64)[None, :]).reshape(-1)      # [m * R]
    calls = np.repeat(np.broadcast_to(np.asarray(call_id, dtype=np.uint64), (m,)), R)
    out = walks[walker.astype(np.int64)].copy()
    alive = np.ones(m * R, dtype=bool)
    for l in range(1, T):
        alive &= ~ends_before(seed, calls, walker, l, alpha, tag, bits)
        out[~alive, l + 1] = -1                             # `alive` only shrinks: what follows an end is -1 too
    return out


def select(walks_truncated, R, k, skip=()):
    """rows i * R .. i * R + R - 1 are the walks of slot i; its visits are the entries >= 0 of the columns 1.. ; the distinct
    visited vertices are ranked by count descending, then id ascending, and the first k kept.  skip: slots that report
    nothing (empty slots, vertices outside the graph).  -> (cnt [m], neighbors, parents, visits), compact, in the hop's
    order."""
    w = np.asarray(walks_truncated, dtype=np.int64)
    m = w.shape[0] // R
    skip = set(int(s) for s in skip)
    cnt, nbr, par, vis = np.zeros(m, dtype=np.int64), [], [], []
    for i in range(m):
        if i in skip:
            continue
        v = w[i * R:(i + 1) * R, 1:].reshape(-1)
        ids, c = np.unique(v[v >= 0], return_counts=True)
        order = np.lexsort((ids, -c))[:k]
        cnt[i] = len(order)
        nbr.append(ids[order])
        vis.append(c[order])
        par.append(np.full(len(order), i, dtype=np.int64))
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.empty(0, dtype=np.int64)
    return cnt, cat(nbr), cat(par), cat(vis)


def select_brute(walks_truncated, R, k):
    """select with a collections.Counter and a Python sort of (-count, id) tuples"""
    w = np.asarray(walks_truncated, dtype=np.int64)
    m = w.shape[0] // R
    cnt, nbr, par, vis = [], [], [], []
    for i in range(m):
        c = Counter(int(x) for row in w[i * R:(i + 1) * R] for x in row[1:] if x >= 0)
        best = sorted((-n, v) for v, n in c.items())[:k]
        cnt.append(len(best))
        nbr += [v for _, v in best]
        vis += [-n for n, _ in best]
        par += [i] * len(best)
    a = lambda x: np.asarray(x, dtype=np.int64)
    return a(cnt), a(nbr), a(par), a(vis)


def blocks(seeds, hop, n_layers):
    """PinSAGELoader's composition for ONE mini-batch with distinct seeds F_0: for layer l, hop(l, F_l) -> (cnt, neighbors,
    parents, visits) over the frontier F_l; F_{l+1} = F_l followed by the neighbours not yet in it, in order of first
    occurrence in the hop's output; block l = dict(n_id = F_{l+1}, n_dst = |F_l|, edge_index [2, E_l] (row = index in n_id
    of the neighbour, col = index of the frontier slot), edge_weight = the visit counts).  -> ([block_{L-1}, ..., block_0],
    F_L): outermost first."""
    F = np.asarray(seeds, dtype=np.int64)
    out = []
    for l in range(n_layers):
        _, nbr, par, vis = hop(l, F)
        where = {int(v): i for i, v in enumerate(F)}
        nxt = list(F)
        for v in nbr:
            if int(v) not in where:
                where[int(v)] = len(nxt)
                nxt.append(int(v))
        row = np.asarray([where[int(v)] for v in nbr], dtype=np.int64)
        n_id = np.asarray(nxt, dtype=np.int64)
        out.append(dict(n_id=n_id, n_dst=len(F), edge_index=np.stack([row, np.asarray(par, dtype=np.int64)]).reshape(2, -1),
                        edge_weight=np.asarray(vis, dtype=np.int64)))
        F = n_id
    return out[::-1], F


def csx(edge_index, n, by_target):
    """CSC (by_target) or CSR of edge_index [2, E], the minor ids sorted inside a column / row -> (ptrs, idx) int64"""
    ei = np.asarray(edge_index, dtype=np.int64)
    major, minor = (ei[1], ei[0]) if by_target else (ei[0], ei[1])
    order = np.lexsort((minor, major))
    ptrs = np.concatenate([[0], np.cumsum(np.bincount(major, minlength=n))]).astype(np.int64)
    return ptrs, minor[order].astype(np.int64)
