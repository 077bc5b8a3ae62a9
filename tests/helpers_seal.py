"""The rule of include/tchgeo_seal.h (tg_seal_nodes: the enclosing subgraph of a link, its two restricted distances and the
double-radius node label) restated with sets and a dict BFS over the row lists in Python ints; the reference of
tests/test_seal_cpu.py, test_gpu_seal.py and test_gpu_seal_loader.py.  Imports nothing."""


def row(ptrs, indices, x):
    return [int(t) for t in indices[int(ptrs[x]):int(ptrs[x + 1])]]


def bfs(ptrs, indices, roots, inside=None, depth=None):
    """-> {vertex: distance from the nearest root}, through vertices of `inside` only (None: all), `depth` steps at most"""
    dist = {r: 0 for r in roots}
    frontier, d = list(roots), 0
    while frontier and (depth is None or d < depth):
        d += 1
        reached = []
        for x in frontier:
            for y in row(ptrs, indices, x):
                if y not in dist and (inside is None or y in inside):
                    dist[y] = d
                    reached.append(y)
        frontier = reached
    return dist


def label(du, dv):
    if du < 0 or dv < 0:
        return 0
    d = du + dv
    return 1 + min(du, dv) + (d // 2) * (d // 2 + d % 2 - 1)


def seal(ptrs, indices, u, v, num_hops, node_cap, z_max=0):
    """-> dict(nodes, z, du, dv, rounds) of one slot; dict(refused=1) for more than node_cap vertices, 2 for an endpoint
    outside [0, len(ptrs) - 1), 4 for u == v"""
    n = len(ptrs) - 1
    if not (0 <= u < n and 0 <= v < n):
        return dict(refused=2)
    if u == v:
        return dict(refused=4)
    N = set(bfs(ptrs, indices, [u, v], depth=num_hops))
    if len(N) > node_cap:
        return dict(refused=1)
    du, dv = bfs(ptrs, indices, [u], N - {v}), bfs(ptrs, indices, [v], N - {u})
    nodes = [u, v] + sorted(N - {u, v})
    a, b = [du.get(x, -1) for x in nodes], [dv.get(x, -1) for x in nodes]
    z = [1, 1] + [label(p, q) for p, q in zip(a[2:], b[2:])]
    if z_max > 0:
        z = [min(w, z_max) for w in z]
    return dict(nodes=nodes, z=z, du=a, dv=b, rounds=max(a + b))
