"""The induced-subgraph rule of tg_ns_induced_count / tg_ns_induced_emit restated in NumPy (the reference of
tests/test_ns_induced_cpu.py and tests/test_gpu_ns_induced.py)."""
import numpy as np


def induced_rule(nodes, ptrs, indices):
    """-> (rows, cols, edge_index): local(v) = the FIRST position of v in `nodes`; for every position i in list order and
    every CSC offset e of column nodes[i] in ascending order, (local(indices[e]), i, e) where local exists."""
    nodes, ptrs, indices = (np.asarray(a, dtype=np.int64) for a in (nodes, ptrs, indices))
    local = {}
    for p, v in enumerate(nodes.tolist()):
        local.setdefault(v, p)
    rows, cols, edge_index = [], [], []
    for i, v in enumerate(nodes.tolist()):
        e0, e1 = int(ptrs[v]), int(ptrs[v + 1])
        src = indices[e0:e1]
        if src.size <= 64:                                   # the loop, as stated
            for e in range(e0, e1):
                j = local.get(int(indices[e]))
                if j is not None:
                    rows.append(j), cols.append(i), edge_index.append(e)
        else:                                                # the same loop over a long column, vectorised
            keep = np.nonzero(np.isin(src, nodes))[0]
            rows.extend(local[int(s)] for s in src[keep])
            cols.extend([i] * keep.size)
            edge_index.extend((e0 + keep).tolist())
    as64 = lambda x: np.asarray(x, dtype=np.int64)
    return as64(rows), as64(cols), as64(edge_index)


def edges_before(cols, marks, n):
    """edge_marks of the C ABI: induced edges whose col is below clamp(mark, 0, n)"""
    return [int((np.asarray(cols) < min(max(int(L), 0), n)).sum()) for L in marks]


def csc_of(edge_index, n):
    """-> (ptrs, indices, perm): CSC of a COO edge list [2, E] (row = source, col = target), rows ascending in a column,
    parallel edges in COO order; perm[e] = the COO id of CSC offset e"""
    row, col = np.asarray(edge_index[0], dtype=np.int64), np.asarray(edge_index[1], dtype=np.int64)
    perm = np.lexsort((np.arange(row.size), row, col)).astype(np.int64)
    ptrs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(col, minlength=n), out=ptrs[1:])
    return ptrs, row[perm], perm
