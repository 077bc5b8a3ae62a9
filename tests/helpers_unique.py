"""The node dedup / relabel rule of tg_ns_homo_unique restated in NumPy (the reference of tests/test_ns_unique_cpu.py and
tests/test_gpu_ns_unique.py)."""
import numpy as np


def unique_rule(samples, rows, cols, layer_starts=()):
    """-> (nodes, inverse, rows_u, cols_u, layer_nodes): nodes = the distinct values of `samples` ordered by their first
    occurrence, nodes[inverse] == samples, rows_u / cols_u = inverse[rows] / inverse[cols], layer_nodes[h] = distinct values
    among the first layer_starts[h] positions."""
    s = np.asarray(samples, dtype=np.int64)
    _, first, inv = np.unique(s, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")               # sorted-value index of the k-th node in first-occurrence order
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    inverse = rank[inv.reshape(-1)].astype(np.int64)
    nodes = s[np.sort(first)]
    is_first = np.zeros(s.size + 1, dtype=np.int64)
    is_first[first] = 1
    before = np.concatenate([[0], np.cumsum(is_first[:s.size])])     # before[L] = first occurrences at positions < L
    layer_nodes = [int(before[min(max(int(L), 0), s.size)]) for L in layer_starts]
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    return nodes, inverse, inverse[rows], inverse[cols], layer_nodes
