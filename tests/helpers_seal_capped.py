"""The rule of include/tchgeo_seal_capped.h (tg_seal_nodes_capped) restated with sets and Python ints: the node set hop by hop,
a hop's keys through helpers_labor.named_draw, then helpers_seal's bfs and label for the distances and the labels."""
import numpy as np

import helpers_seal as hs
from helpers_labor import named_draw

TAG_SEAL_HOP = 19


def node_set(ptrs, indices, u, v, caps, seed, call_id):
    """-> (N, cut): S_t = the caps[t - 1] members of the fringe of S_{t-1} with the smallest (key, id), all of it at cap 0"""
    N, S, cut = {u, v}, {u, v}, 0
    for t, k in enumerate(caps, 1):
        F = sorted({y for x in S for y in hs.row(ptrs, indices, x)} - N)
        if 0 < k < len(F):
            w = named_draw(seed, call_id, TAG_SEAL_HOP, np.array(F, dtype=np.uint64), t, 0)   # key_t(y) = w1 << 32 | w0
            key = {y: (int(hi) << 32) | int(lo) for y, lo, hi in zip(F, w[0], w[1])}
            F = sorted(F, key=lambda y: (key[y], y))[:k]
            cut |= 1 << (t - 1)
        N, S = N | set(F), set(F)
    return N, cut


def seal_capped(ptrs, indices, u, v, caps, node_cap, seed, call_id, z_max=0):
    """-> helpers_seal.seal's dict of one slot, with `cut`"""
    n = len(ptrs) - 1
    if not (0 <= u < n and 0 <= v < n):
        return dict(refused=2)
    if u == v:
        return dict(refused=4)
    N, cut = node_set(ptrs, indices, u, v, caps, seed, call_id)
    if len(N) > node_cap:
        return dict(refused=1)
    du, dv = hs.bfs(ptrs, indices, [u], N - {v}), hs.bfs(ptrs, indices, [v], N - {u})
    nodes = [u, v] + sorted(N - {u, v})
    a, b = [du.get(x, -1) for x in nodes], [dv.get(x, -1) for x in nodes]
    z = [1, 1] + [hs.label(p, q) for p, q in zip(a[2:], b[2:])]
    if z_max > 0:
        z = [min(w, z_max) for w in z]
    return dict(nodes=nodes, z=z, du=a, dv=b, rounds=max(a + b), cut=cut)
