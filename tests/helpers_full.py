"""The rule of tg_ns_full_count / tg_ns_full_emit (include/tchgeo.h) restated in NumPy: every in-edge of a frontier, the
sources deduplicated in first-occurrence order behind it; plus the chunk count, the refusal rule, the workspace formula and
FullNeighborLoader's chained layers (the reference of tests/test_full_cpu.py, tests/test_gpu_ns_full.py and
tests/test_gpu_full_loader.py)."""
import numpy as np

CHUNK = 512
MAX_NODES = 1 << 30
MAX_EDGES = 1 << 31


def columns(ptrs, nodes, n_major=None):
    """-> (begin, length) per position: an id outside [0, n_major) is a column of length 0"""
    ptrs, nodes = np.asarray(ptrs, dtype=np.int64), np.asarray(nodes, dtype=np.int64)
    n_major = ptrs.size - 1 if n_major is None else int(n_major)
    ok = (nodes >= 0) & (nodes < n_major)
    v = np.where(ok, nodes, 0)
    begin = np.where(ok, ptrs[v], 0)
    return begin, np.where(ok, ptrs[v + 1] - ptrs[v], 0)


def status_of(ptrs, nodes, n_major=None):
    """bit 1 (value 2): an id outside [0, n_major)"""
    ptrs, nodes = np.asarray(ptrs, dtype=np.int64), np.asarray(nodes, dtype=np.int64)
    n_major = ptrs.size - 1 if n_major is None else int(n_major)
    return 2 if ((nodes < 0) | (nodes >= n_major)).any() else 0


def chunks_of(ptrs, nodes, n_major=None):
    """the sum over positions of ceil(column length / 512)"""
    _, length = columns(ptrs, nodes, n_major)
    return int((-(-length // CHUNK)).sum())


def edges_of(ptrs, nodes, n_major=None):
    return int(columns(ptrs, nodes, n_major)[1].sum())


def chunk_bound(max_nodes, n_edges, chunk_cap=0):
    return chunk_cap if chunk_cap > 0 else max_nodes + -(-n_edges // CHUNK)


def refused(n, m, chunks, node_cap, bound, id_bound):
    """the capacity rule: decided from the frontier's length, the edge count and the chunk count alone"""
    return n + min(m, id_bound) > node_cap or chunks > bound or m >= MAX_EDGES


def full_rule(ptrs, indices, nodes, n_major=None):
    """-> (out_nodes, rows, cols, edge_index) of one batch: triples in (position, CSC offset) order, out_nodes = the frontier
    followed by the sources that equal no earlier entry in order of first occurrence, row = the FIRST position of the source"""
    ptrs, indices, nodes = (np.asarray(a, dtype=np.int64) for a in (ptrs, indices, nodes))
    n = nodes.size
    begin, length = columns(ptrs, nodes, n_major)
    m = int(length.sum())
    cols = np.repeat(np.arange(n, dtype=np.int64), length)
    before = np.cumsum(length) - length
    edge_index = np.arange(m, dtype=np.int64) - np.repeat(before, length) + np.repeat(begin, length)
    src = indices[edge_index]
    every = np.concatenate([nodes, src])
    ids, first = np.unique(every, return_index=True)            # the first position of every id in frontier + sources
    new = np.sort(first[first >= n])                             # sources that are no frontier node, by first occurrence
    out_nodes = np.concatenate([nodes, every[new]])
    pos = np.where(first < n, first, n + np.searchsorted(new, first))
    rows = pos[np.searchsorted(ids, src)].astype(np.int64)
    return out_nodes, rows, cols, edge_index


def blocks(ptrs, indices, seeds, num_layers):
    """FullNeighborLoader's layers for one mini-batch, layer 0 first -> [(n_id, n_dst, rows, cols, csc offsets)]: F_0 = the
    seeds, F_{l+1} = out_nodes of the rule over F_l, all of it the next frontier"""
    out, frontier = [], np.asarray(seeds, dtype=np.int64)
    for _ in range(num_layers):
        n_id, rows, cols, e = full_rule(ptrs, indices, frontier)
        out.append((n_id, frontier.size, rows, cols, e))
        frontier = n_id
    return out


def r256(x):
    return (x + 255) & ~255


def table_slots(node_cap):
    want, c = (4 * node_cap + 2) // 3, 64
    while c < want:
        c <<= 1
    return c


def workspace_bytes(n_edges, max_nodes, node_cap, chunk_cap, id_bound):
    """one batch of the pair's workspace: header | keys | values (uint32) | chunk prefix, edge prefix (uint64, + 1 each) and
    column begin (int64) per position | two tile sums per tile of positions | new nodes per chunk + 1 (uint32) | tile sums"""
    key = 4 if id_bound <= 1 << 31 else 8
    slots, bound = table_slots(node_cap), chunk_bound(max_nodes, n_edges, chunk_cap)
    tiles = -(-max_nodes // 1024) if max_nodes else 1
    return (256 + r256(slots * key) + r256(slots * 4) + 2 * r256((max_nodes + 1) * 8) + r256(max_nodes * 8) + r256(tiles * 16)
            + r256((bound + 1) * 4) + r256((bound // 1024 + 1) * 4))
