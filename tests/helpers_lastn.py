"""NumPy restatement of include/tchgeo_lastn.h: the state as the header's bytes driven by a per-node loop, `sample` as the
reference's loop over hops (neighbor_sampling.rs:188-223, as helpers_recent.recent_ns_homo) with "newest first" as the
sampler, and the loader's (n_id, edge_index, e_id) through helpers_unique.  Deliberately plain.  Does not import the library."""
import numpy as np

from helpers_unique import unique_rule

MAX_K, MAX_NODES, MAX_EVENTS, LDS_ENTRIES = 64, 1 << 31, 1 << 22, 4096
FORM_AUTO, FORM_LDS, FORM_GRID = 0, 1, 2


def r256(x):
    return (int(x) + 255) // 256 * 256


def state_bytes(n_nodes, k):
    return r256(8 * n_nodes) + 16 * n_nodes * k


def insert_workspace_bytes(n_events, symmetric, form=FORM_AUTO):
    """-> (bytes, form taken), the header's formula"""
    entries = n_events * (2 if symmetric else 1)
    taken = form if form != FORM_AUTO else (FORM_LDS if entries <= LDS_ENTRIES else FORM_GRID)
    if taken == FORM_LDS:
        return 0, taken
    T = 64
    while T < 2 * entries:
        T *= 2
    return r256(8 * T) + 5 * r256(4 * T) + r256(4 * entries), taken


def entries_of(src, dst, e_id=None, e_base=0, symmetric=True):
    """the call's entries in entry order: (node, nbr, e_id)"""
    src, dst = np.asarray(src, dtype=np.int64).reshape(-1), np.asarray(dst, dtype=np.int64).reshape(-1)
    e = e_base + np.arange(src.size, dtype=np.int64) if e_id is None else np.asarray(e_id, dtype=np.int64).reshape(-1)
    out = []
    for j in range(src.size):
        out.append((int(dst[j]), int(src[j]), int(e[j])))
        if symmetric:
            out.append((int(src[j]), int(dst[j]), int(e[j])))
    return out


class State:
    """words: the state as int64 words (the header's bytes); count and slot are views into it"""

    def __init__(self, n_nodes, k):
        assert 1 <= k <= MAX_K and 1 <= n_nodes <= MAX_NODES
        self.n_nodes, self.k = n_nodes, k
        self.words = np.empty(state_bytes(n_nodes, k) // 8, dtype=np.int64)
        pad = r256(8 * n_nodes) // 8
        self.count = self.words[:n_nodes]
        self.slot = self.words[pad:].reshape(n_nodes, k, 2)          # [node, ring position, {nbr, e_id}]
        self.reset()

    def reset(self):
        self.words[:r256(8 * self.n_nodes) // 8] = 0                 # the padding is zeroed with the counts
        self.slot[...] = -1

    def insert(self, src, dst, e_id=None, e_base=0, symmetric=True):
        """-> status"""
        status = 0
        for node, nbr, e in entries_of(src, dst, e_id, e_base, symmetric):
            if not 0 <= node < self.n_nodes:
                status |= 2
                continue
            c = int(self.count[node])
            self.slot[node, c % self.k] = (nbr, e)
            self.count[node] = c + 1
        return status

    def newest(self, v, f):
        """the min(f, count, k) newest entries of node v, newest first -> [(nbr, e_id)]"""
        c = int(self.count[v])
        return [tuple(int(x) for x in self.slot[v, (c - 1 - r) % self.k]) for r in range(min(f, c, self.k))]

    def sample(self, seeds, fanout):
        """-> (samples, rows, cols, edge_index, layer_offsets, counts, status) of one batch"""
        seeds = np.asarray(seeds, dtype=np.int64).reshape(-1)
        n_seeds = seeds.size
        status = 2 if np.any((seeds < 0) | (seeds >= self.n_nodes)) else 0
        samples, rows, cols, eidx, layer_offsets = [int(s) for s in seeds], [], [], [], []
        begin, m = 0, n_seeds
        for f in fanout:
            assert 1 <= f <= self.k
            ne = len(eidx)
            layer_offsets.append((n_seeds + ne, ne, n_seeds + ne))
            for i in range(begin, begin + m):
                v = samples[i]
                if not 0 <= v < self.n_nodes:
                    continue                                         # an empty frontier slot
                for nbr, e in self.newest(v, f):
                    rows.append(n_seeds + len(eidx))
                    cols.append(i)
                    samples.append(nbr)
                    eidx.append(e)
            begin, m = begin + m, len(eidx) - ne
        a = lambda x: np.asarray(x, dtype=np.int64).reshape(-1)
        return a(samples), a(rows), a(cols), a(eidx), layer_offsets, (n_seeds + len(eidx), len(eidx)), status


def capacity(n_seeds, fanout):
    layer, edges = n_seeds, 0
    for f in fanout:
        layer *= f
        edges += layer
    return n_seeds + edges, edges


def loader_view(samples, rows, cols, eidx):
    """-> (n_id, edge_index [2, E], e_id): the inputs first, then new neighbours by first occurrence (tg_ns_homo_unique's
    order); edge_index[0] = the neighbour, edge_index[1] = the query node, both numbered against n_id"""
    nodes, _, rows_u, cols_u, _ = unique_rule(samples, rows, cols)
    return nodes, np.stack([rows_u, cols_u]).astype(np.int64).reshape(2, -1), np.asarray(eidx, dtype=np.int64)


def entries_csc(entries, n_nodes):
    """the CSC whose column v holds the entries of node v in insertion order -> (ptrs, idx = nbr, ts = e_id); entries with a
    node outside the range are dropped as the insert drops them"""
    entries = [t for t in entries if 0 <= t[0] < n_nodes]
    node = np.asarray([t[0] for t in entries], dtype=np.int64).reshape(-1)
    order = np.argsort(node, kind="stable")
    ptrs = np.concatenate([[0], np.cumsum(np.bincount(node, minlength=n_nodes))]).astype(np.int64)
    a = lambda i: np.asarray([t[i] for t in entries], dtype=np.int64).reshape(-1)[order]
    return ptrs, a(1), a(2)
