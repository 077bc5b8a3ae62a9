"""The per-subgraph induced rule of tg_ns_induced_grouped_count / tg_ns_induced_grouped_emit restated in NumPy (the
reference of tests/test_shadow_cpu.py, tests/test_gpu_ns_induced_grouped.py and tests/test_gpu_shadow_loader.py)."""
import numpy as np

from helpers_recent import FILTER_RELATIVE, admitted

CHUNK = 512


def _ok(nodes, group, n_major, n_groups):
    """positions that take part: the id is a column of the graph and the group word is a group"""
    ok = (nodes >= 0) & (nodes < n_major) & (group >= 0)
    return ok & (group < n_groups) if n_groups is not None else ok


def grouped_induced_rule(nodes, group, ptrs, indices, ts=None, group_time=None, window=None, n_groups=None):
    """-> (rows, cols, edge_index): local(g, v) = the FIRST position p with (group[p], nodes[p]) == (g, v); for every
    position i in list order, g = group[i], and every CSC offset e of column nodes[i] in ascending order,
    (local(g, indices[e]), i, e) where local exists and -- with group_time -- the edge is admitted: the backward relative
    predicate window[0] <= group_time[g] - ts[e] <= window[1] in wrapping int64 arithmetic.  A position whose id is no
    column of the graph, or whose group word is outside [0, n_groups) (n_groups given), is a column of length 0 and
    nobody's local."""
    nodes, group, ptrs, indices = (np.asarray(a, dtype=np.int64) for a in (nodes, group, ptrs, indices))
    ok = _ok(nodes, group, ptrs.size - 1, n_groups)
    local = {}
    for p, (g, v) in enumerate(zip(group.tolist(), nodes.tolist())):
        if ok[p]:
            local.setdefault((g, v), p)
    timed = group_time is not None
    if timed:
        ts, group_time = np.asarray(ts, dtype=np.int64), np.asarray(group_time, dtype=np.int64)
    rows, cols, edge_index, members = [], [], [], {}
    for i, (g, v) in enumerate(zip(group.tolist(), nodes.tolist())):
        if not ok[i]:
            continue
        e0, e1 = int(ptrs[v]), int(ptrs[v + 1])
        if e1 - e0 > 64:                                     # the same loop over a long column: only members are looked up
            if g not in members:
                members[g] = np.array(sorted(u for (h, u) in local if h == g), dtype=np.int64)
            offsets = (e0 + np.nonzero(np.isin(indices[e0:e1], members[g]))[0]).tolist()
        else:
            offsets = range(e0, e1)
        for e in offsets:
            j = local.get((g, int(indices[e])))
            if j is None:
                continue
            if timed and not admitted(ts[e:e + 1], int(group_time[g]), FILTER_RELATIVE, False, window)[0]:
                continue
            rows.append(j), cols.append(i), edge_index.append(e)
    as64 = lambda x: np.asarray(x, dtype=np.int64)
    return as64(rows), as64(cols), as64(edge_index)


def chunks_of(nodes, ptrs, group=None, n_groups=None):
    """the chunk count of a list: the sum over positions of ceil(column length / 512) (a position outside the graph, or --
    group given -- outside the groups, has none)"""
    nodes, ptrs = np.asarray(nodes, dtype=np.int64), np.asarray(ptrs, dtype=np.int64)
    grp = np.zeros_like(nodes) if group is None else np.asarray(group, dtype=np.int64)
    ok = _ok(nodes, grp, ptrs.size - 1, n_groups)
    v = nodes[ok]
    return int((-(-(ptrs[v + 1] - ptrs[v]) // CHUNK)).sum())
