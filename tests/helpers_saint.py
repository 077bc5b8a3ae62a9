"""GraphSAINT's random-walk sampler restated in NumPy (the reference of tests/test_saint_cpu.py, test_gpu_saint_rw.py and
test_gpu_saint_loader.py): the node list of a walk matrix, the coverage counters and the two norms of tg_saint_norm."""
import numpy as np


def node_list(walks, skip=()):
    """nodes of one mini-batch from its walk matrix [B, T + 1] (row i = walker i, -1 behind a dead end, as tg_random_walk
    writes it): the visit of walker i at step l has position l * B + i; -> the distinct visited vertices ordered by the
    position of their first occurrence.  skip: walkers that contribute nothing (roots outside the graph)."""
    walks = np.array(walks, dtype=np.int64)
    if len(skip):
        walks[np.asarray(skip, dtype=np.int64)] = -1
    flat = walks.T.reshape(-1)                              # position order: step-major
    visits = flat[flat >= 0]
    _, first = np.unique(visits, return_index=True)
    return visits[np.sort(first)]


def random_graph(n=300, n_edges=2000, sink_share=0.1, seed=0):
    """-> edge_index [2, E] with self loops, parallel edges and about sink_share of the vertices without out-edges"""
    rs = np.random.default_rng(seed)
    ei = rs.integers(0, n, (2, n_edges)).astype(np.int64)
    ei[1, :20] = ei[0, :20]                                 # self loops
    ei[:, 20:60] = ei[:, 60:100]                            # parallel edges
    sinks = rs.permutation(n)[:int(n * sink_share)]
    return ei[:, ~np.isin(ei[0], sinks)]


def coverage_counts(node_lists, edge_id_lists, n_nodes, n_edges):
    """-> (node_count [n_nodes], edge_count [n_edges]) int64: how often every id is listed; ids outside a table are skipped"""
    node_count, edge_count = np.zeros(n_nodes, dtype=np.int64), np.zeros(n_edges, dtype=np.int64)
    for table, lists in ((node_count, node_lists), (edge_count, edge_id_lists)):
        for ids in lists:
            ids = np.asarray(ids, dtype=np.int64)
            np.add.at(table, ids[(ids >= 0) & (ids < table.size)], 1)
    return node_count, edge_count


def norms(ptrs, node_count, edge_count, n_samples):
    """tg_saint_norm in float32 -> (node_norm [N], edge_norm [E]); ptrs: the CSC offsets (an edge's column = its target)"""
    ptrs = np.asarray(ptrs, dtype=np.int64)
    n = ptrs.size - 1
    f32 = np.float32
    nc, ec = np.asarray(node_count, dtype=np.int64), np.asarray(edge_count, dtype=np.int64)
    col_of = np.repeat(np.arange(n), np.diff(ptrs))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = nc[col_of].astype(f32) / ec.astype(f32)
    edge_norm = np.where(np.isnan(r), f32(0.1), np.minimum(np.maximum(r, f32(0)), f32(1e4))).astype(f32)
    d = np.where(nc == 0, f32(0.1), nc.astype(f32)).astype(f32)
    node_norm = ((f32(n_samples) / d).astype(f32) / f32(n)).astype(f32)
    return node_norm, edge_norm


def presample_launches(sizes_per_launch, n_nodes, sample_coverage):
    """the loader's stopping rule: launches taken until the node lists' sizes add up to n_nodes * sample_coverage;
    sizes_per_launch: an iterable of the per-launch sums"""
    covered = launches = 0
    for s in sizes_per_launch:
        covered += int(s)
        launches += 1
        if covered >= n_nodes * sample_coverage:
            return launches
    raise ValueError("not enough launches to reach the coverage")
