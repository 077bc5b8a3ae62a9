"""The per-group node dedup / relabel rule of tg_ns_homo_unique_grouped (PyG's disjoint=True) restated in NumPy, and the
link loaders' seed -> group and seed -> label-edge maps (the reference of tests/test_disjoint_cpu.py and the GPU tests of
the operator, NeighborLoader(disjoint=True) and the temporal LinkNeighborLoader)."""
import numpy as np

BINARY, TRIPLET = 0, 1


def roots(cols, n, n_seeds):
    """root[p] of every position p < n of a forest whose edge e makes position n_seeds + e with parent cols[e] (an earlier
    position): root(p) = p for a seed, else root(parent(p)).  Pointer jumping: every round doubles the steps taken."""
    n_seeds = min(n_seeds, n)
    parent = np.concatenate([np.arange(n_seeds, dtype=np.int64), np.asarray(cols, dtype=np.int64)[:n - n_seeds]])
    assert parent.size == n and (parent[n_seeds:] < np.arange(n_seeds, n)).all() and (parent >= 0).all()
    root = parent
    while (root >= n_seeds).any():
        root = root[root]
    return root


def disjoint_rule(samples, rows, cols, n_seeds, seed_group=None, layer_starts=()):
    """-> (nodes, group, inverse, rows_u, cols_u, layer_nodes): group(p) = seed_group[root(p)] (None: the identity); nodes
    lists the id of every distinct pair (group(p), samples[p]) ordered by the pair's first position, group[u] is the group
    of nodes[u]; inverse[p] = index of p's pair; rows_u / cols_u = inverse[rows] / inverse[cols]; layer_nodes[h] = distinct
    pairs among the first layer_starts[h] positions."""
    s = np.asarray(samples, dtype=np.int64)
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    n = s.size
    if n == 0:
        e = np.zeros(0, dtype=np.int64)
        return e, e, e, e, e, [0 for _ in layer_starts]
    root = roots(cols, n, n_seeds)
    g = root if seed_group is None else np.asarray(seed_group, dtype=np.int64)[root]
    pair = np.stack([g, s], axis=1)
    _, first, inv = np.unique(pair, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")               # sorted-pair index of the k-th node in first-occurrence order
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    inverse = rank[inv.reshape(-1)].astype(np.int64)
    at = np.sort(first)
    is_first = np.zeros(n + 1, dtype=np.int64)
    is_first[first] = 1
    before = np.concatenate([[0], np.cumsum(is_first[:n])])          # before[L] = first occurrences at positions < L
    layer_nodes = [int(before[min(max(int(L), 0), n)]) for L in layer_starts]
    return s[at], g[at].astype(np.int64), inverse, inverse[rows], inverse[cols], layer_nodes


def brute_force(samples, rows, cols, n_seeds, seed_group=None, layer_starts=()):
    """The same rule with a Python dict and a parent walk per position."""
    n, seen, nodes, group, inverse, layer = len(samples), {}, [], [], [], {}
    for p in range(n):
        for h, L in enumerate(layer_starts):
            if L == p:
                layer[h] = len(nodes)
        q = p
        while q >= n_seeds:
            q = int(cols[q - n_seeds])
        g = q if seed_group is None else int(seed_group[q])
        key = (g, int(samples[p]))
        if key not in seen:
            seen[key] = len(nodes)
            nodes.append(key[1])
            group.append(g)
        inverse.append(seen[key])
    layer_nodes = [layer.get(h, len(nodes)) if L < n else len(nodes) for h, L in enumerate(layer_starts)]
    i64 = lambda x: np.array(x, dtype=np.int64)
    return (i64(nodes), i64(group), i64(inverse), i64([inverse[r] for r in rows]), i64([inverse[c] for c in cols]),
            layer_nodes)


def link_groups(E, K, mode):
    """-> (seed_group [S], time_index [S], n_groups) of a link mini-batch of E positives with K negatives each.  Binary:
    the row is [src of the P pairs | dst of the P pairs], P = E + E K, seed s belongs to pair s mod P, one group per pair;
    triplet: [src i | dst_pos i | dst_neg u], groups i, i, u // K, one group per positive.  time_index[s] is the positive
    whose edge_label_time seed s samples under: pair j < E is positive j, negative u = j - E belongs to positive u // K."""
    P = E + E * K
    of_pair = np.concatenate([np.arange(E), np.arange(E * K) // K]).astype(np.int64)
    if mode == BINARY:
        return np.tile(np.arange(P, dtype=np.int64), 2), np.tile(of_pair, 2), P
    own = np.concatenate([np.arange(E, dtype=np.int64), of_pair])
    return own, own, E


def temporal_graph(n=2000, e=20000, seed=31):
    """A seeded random directed graph for the loader tests: edge_index [2, e], an int64 time per edge in [0, 1000), node
    features [n, 6]."""
    rs = np.random.default_rng(seed)
    ei = np.stack([rs.integers(0, n, e), rs.integers(0, n, e)]).astype(np.int64)
    return ei, rs.integers(0, 1000, e).astype(np.int64), rs.standard_normal((n, 6)).astype(np.float32)
