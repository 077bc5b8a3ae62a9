"""The rule of tg_cluster_count / tg_cluster_emit restated in NumPy: expand the cluster lists to node lists, then apply
helpers_induced.induced_rule; plus ClusterData's renumbering and ClusterLoader's epoch order (the reference of
tests/test_cluster_cpu.py, tests/test_gpu_cluster_induced.py and tests/test_gpu_cluster_loader.py)."""
import numpy as np
import torch

from helpers_induced import csc_of, induced_rule

CHUNK = 512
MAX_PARTS = 1024


def expand(partptr, clusters, n_major=None):
    """-> (node list, status bits): the ranges [partptr[c], partptr[c+1]) of the list's clusters one after the other, in the
    list's order.  A cluster id outside [0, n_parts) contributes nothing (bit 1, value 2); so does a range that is inverted
    or leaves [0, n_major] (bit 2, value 4)."""
    partptr = np.asarray(partptr, dtype=np.int64)
    n_parts = partptr.size - 1
    n_major = int(partptr[-1]) if n_major is None else int(n_major)
    parts, status = [], 0
    for c in np.asarray(clusters, dtype=np.int64).tolist():
        if not 0 <= c < n_parts:
            status |= 2
            continue
        lo, hi = int(partptr[c]), int(partptr[c + 1])
        if lo < 0 or hi > n_major or lo > hi:
            status |= 4
            continue
        parts.append(np.arange(lo, hi, dtype=np.int64))
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)), status


def chunks_of(partptr, clusters, ptrs, n_major=None):
    """the chunks the scan cuts a batch into: ceil(offset range / 512) per named cluster (0 for an empty or refused one)"""
    partptr, ptrs = np.asarray(partptr, dtype=np.int64), np.asarray(ptrs, dtype=np.int64)
    total = 0
    for c in np.asarray(clusters, dtype=np.int64).tolist():
        nodes, _ = expand(partptr, [c], n_major)
        if nodes.size:
            total += -(-int(ptrs[nodes[-1] + 1] - ptrs[nodes[0]]) // CHUNK)
    return total


def chunk_bound(pitch, n_edges):
    return pitch + -(-n_edges // CHUNK)


def cluster_rule(partptr, clusters, ptrs, indices, node_ids=None, pitch=None, n_major=None):
    """-> (nodes, rows, cols, edge_index, status) of one batch.  A batch whose chunk count exceeds the workspace bound
    (pitch + ceil(E / 512); only with repeated clusters) is empty and raises bit 0 (value 1)."""
    pitch = len(clusters) if pitch is None else pitch
    nodes, status = expand(partptr, clusters, n_major)
    if chunks_of(partptr, clusters, ptrs, n_major) > chunk_bound(pitch, len(indices)) or nodes.size >= 2 ** 31:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, z, status | 1
    rows, cols, e = induced_rule(nodes, ptrs, indices)
    out = nodes if node_ids is None else np.asarray(node_ids, dtype=np.int64)[nodes]
    return out, rows, cols, e, status


def r256(x):
    return (x + 255) & ~255


def workspace_bytes(n_edges, pitch):
    """one batch of the pair's workspace: header | the clusters' offset ranges (2 x int64) | chunk prefix per list entry + 1
    and start / size / base (uint32) | the sorted range table (3 x uint32) | hits per chunk + 1 (uint64) | tile sums"""
    bound = chunk_bound(pitch, n_edges)
    return (256 + r256(2 * pitch * 8) + r256((4 * pitch + 1) * 4) + r256(3 * pitch * 4) + r256((bound + 1) * 8)
            + r256((bound // 1024 + 1) * 8))


def renumber(part, num_parts, edge_index):
    """ClusterData's setup -> (node_perm, node_inv, partptr, ptrs, indices, perm): a stable sort of `part` numbers the nodes
    cluster by cluster (node_perm[new] = old), the CSC is that of the renumbered edge list, perm[e] = the original edge"""
    part = np.asarray(part, dtype=np.int64)
    node_perm = np.argsort(part, kind="stable").astype(np.int64)
    node_inv = np.empty_like(node_perm)
    node_inv[node_perm] = np.arange(part.size, dtype=np.int64)
    partptr = np.zeros(num_parts + 1, dtype=np.int64)
    np.cumsum(np.bincount(part, minlength=num_parts), out=partptr[1:])
    ei = np.asarray(edge_index, dtype=np.int64)
    ptrs, indices, perm = csc_of(node_inv[ei], part.size)
    return node_perm, node_inv, partptr, ptrs, indices, perm


def epoch_order(num_parts, seed, epoch, shuffle=True):
    """the clusters in the order epoch `epoch` visits them: torch.randperm from a CPU generator seeded by (seed, epoch)"""
    if not shuffle:
        return np.arange(num_parts, dtype=np.int64)
    g = torch.Generator()
    g.manual_seed((seed * 1000003 + epoch) % (1 << 63))
    return torch.randperm(num_parts, generator=g).numpy().astype(np.int64)


def epoch_lists(num_parts, q, seed, epoch, shuffle=True, drop_last=False):
    """the cluster lists of the epoch's mini-batches"""
    order = epoch_order(num_parts, seed, epoch, shuffle)
    lists = [order[j:j + q] for j in range(0, num_parts, q)]
    return [l for l in lists if not drop_last or l.size == q]
