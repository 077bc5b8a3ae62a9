"""Cluster-GCN mini-batches (tg_cluster_workspace_bytes / _count / _emit, ClusterData, ClusterLoader), host-only parts: the
NumPy restatement against a brute-force dict version, the exports, the workspace formula, every refusal that comes before
a launch, the loader's and ClusterData's argument refusals and the partition helpers.  No GPU: every device pointer handed
over is null or an address that is never read."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from helpers_cluster import (chunk_bound, chunks_of, cluster_rule, epoch_lists, epoch_order, expand, renumber,
                             workspace_bytes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tg_cluster_workspace_bytes", "tg_cluster_count", "tg_cluster_emit")


@pytest.fixture(scope="module")
def cabi():
    if not os.path.exists(os.path.join(ROOT, "tch-geometric_amd", "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tch-geometric_amd"), "-s"])
    from tch_geometric import _cabi
    return _cabi


# ---- the restatement against brute force -------------------------------------------------------------------------------
def brute(partptr, clusters, ptrs, indices):
    """the contract of include/tchgeo.h, loop by loop: base_k, local = the first k whose range holds u"""
    ranges, base = [], 0
    for c in clusters:
        ranges.append((partptr[c], partptr[c + 1], base))
        base += partptr[c + 1] - partptr[c]

    def local(u):
        for lo, hi, b in ranges:
            if lo <= u < hi:
                return b + u - lo
        return None

    nodes, triples = [], []
    for lo, hi, b in ranges:
        for v in range(lo, hi):
            i = len(nodes)
            nodes.append(v)
            for e in range(ptrs[v], ptrs[v + 1]):
                j = local(indices[e])
                if j is not None:
                    triples.append((j, i, e))
    return nodes, triples


def random_case(seed):
    rs = np.random.default_rng(seed)
    n, P = int(rs.integers(5, 40)), int(rs.integers(1, 9))
    cuts = np.sort(rs.integers(0, n + 1, P - 1))                     # empty clusters happen
    partptr = np.concatenate([[0], cuts, [n]]).astype(np.int64)
    deg = rs.integers(0, 6, n)
    ptrs = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = rs.integers(0, n, int(ptrs[-1])).astype(np.int64)      # self loops and parallel edges happen
    return rs, n, P, partptr, ptrs, indices


@pytest.mark.parametrize("seed", range(12))
def test_rule_equals_brute_force(seed):
    rs, n, P, partptr, ptrs, indices = random_case(seed)
    for clusters in (rs.permutation(P)[:max(1, P // 2)], rs.integers(0, P, 5), np.arange(P)[::-1], np.zeros(0, np.int64)):
        nodes, rows, cols, e, status = cluster_rule(partptr, clusters, ptrs, indices)
        want_nodes, want = brute(partptr.tolist(), [int(c) for c in clusters], ptrs.tolist(), indices.tolist())
        assert status == 0 and nodes.tolist() == want_nodes
        assert list(zip(rows.tolist(), cols.tolist(), e.tolist())) == want
    ids = rs.permutation(n) + 100
    assert np.array_equal(cluster_rule(partptr, [0, P - 1], ptrs, indices, node_ids=ids)[0], ids[expand(partptr, [0, P - 1])[0]])


def test_rule_status_bits():
    partptr = np.array([0, 3, 2, 6, 9], dtype=np.int64)                  # cluster 1 = [3, 2) is inverted
    ptrs = np.arange(0, 10 * 600, 600, dtype=np.int64)[:10]              # 9 columns of 600 entries: 2 chunks a column at most
    indices = np.zeros(int(ptrs[-1]), dtype=np.int64)
    assert expand(partptr, [0, -1, 4, 3])[1] == 2 and expand(partptr, [0, -1, 4, 3])[0].tolist() == [0, 1, 2, 6, 7, 8]
    assert expand(partptr, [1, 2])[1] == 4 and expand(partptr, [1, 2])[0].tolist() == [2, 3, 4, 5]
    assert expand(partptr, [3], n_major=8)[1] == 4                       # leaves [0, n_major]
    assert chunks_of(partptr, [0, 3], ptrs) == 2 * 4 and chunk_bound(2, indices.size) == 2 + 11
    assert cluster_rule(partptr, [0, 3], ptrs, indices)[4] == 0
    nodes, rows, cols, e, status = cluster_rule(partptr, [0] * 4, ptrs, indices)      # 16 chunks > 4 + 11
    assert status == 1 and nodes.size == rows.size == 0
    assert cluster_rule(partptr, [0] * 3, ptrs, indices)[4] == 0         # 12 <= 3 + 11: a repeat inside the bound


def test_renumbering_and_epoch_order():
    rs = np.random.default_rng(5)
    n, P, E = 30, 4, 90
    part = rs.integers(0, P, n)
    ei = rs.integers(0, n, (2, E))
    node_perm, node_inv, partptr, ptrs, indices, perm = renumber(part, P, ei)
    assert sorted(node_perm.tolist()) == list(range(n)) and np.array_equal(node_perm[node_inv], np.arange(n))
    for c in range(P):                                                    # cluster c, its members in ascending original id
        assert node_perm[partptr[c]:partptr[c + 1]].tolist() == np.nonzero(part == c)[0].tolist()
    for v in range(n):
        for e in range(ptrs[v], ptrs[v + 1]):
            assert node_perm[v] == ei[1][perm[e]] and node_perm[indices[e]] == ei[0][perm[e]]
    assert sorted(perm.tolist()) == list(range(E))
    a, b = epoch_order(9, 3, 0), epoch_order(9, 3, 1)
    assert sorted(a.tolist()) == list(range(9)) and a.tolist() != b.tolist() and a.tolist() == epoch_order(9, 3, 0).tolist()
    assert epoch_order(9, 3, 1, shuffle=False).tolist() == list(range(9))
    assert [l.size for l in epoch_lists(9, 4, 3, 0)] == [4, 4, 1] and [l.size for l in epoch_lists(9, 4, 3, 0, drop_last=True)] == [4, 4]
    assert np.concatenate(epoch_lists(9, 4, 3, 0)).tolist() == a.tolist()


def test_loader_order_is_the_restatement(cabi):
    from tch_geometric.loader import cluster_epoch_order
    for seed, epoch in ((0, 0), (7, 3), (2 ** 40, 5)):
        assert cluster_epoch_order(33, seed, epoch).tolist() == epoch_order(33, seed, epoch).tolist()
    assert cluster_epoch_order(5, 1, 2, shuffle=False).tolist() == [0, 1, 2, 3, 4]


# ---- exports and the workspace formula ---------------------------------------------------------------------------------------
def test_symbols_and_struct(cabi):
    for name in NAMES:
        assert name in cabi.EXPORTS and hasattr(cabi.lib, name)
    assert [f for f, _ in cabi.TgClusterIn._fields_] == ["partptr", "n_parts", "clusters", "pitch_parts", "n_clusters", "node_ids"]
    header = open(os.path.join(ROOT, "include", "tchgeo.h")).read()
    for name in NAMES:
        assert "TG_API int %s(" % name in header
    assert "#define TG_CLUSTER_MAX_PARTS_PER_BATCH 1024" in header and cabi.CLUSTER_MAX_PARTS_PER_BATCH == 1024


def graph(cabi, n_major=100, n_edges=1000, ptrs=0x10000, indices=0x10000):
    g = cabi.TgGraph()
    g.ptrs, g.indices, g.n_major, g.n_edges = ptrs, indices, n_major, n_edges
    return g


def test_workspace_formula(cabi):
    for E, pitch in ((0, 0), (1000, 1), (40000, 37), (511, 1024), (512, 1024), (513, 3), (1 << 28, 32), (1 << 33, 1024)):
        per = workspace_bytes(E, pitch)
        assert cabi.cluster_workspace_bytes(graph(cabi, n_edges=E), 50, pitch, 7) == (7 * per, per)
        assert cabi.cluster_workspace_bytes(graph(cabi, n_edges=E), 0, pitch, 0) == (0, per)
    # the table of the largest batch is 12 KiB: three 32-bit words per range
    assert 3 * 4 * cabi.CLUSTER_MAX_PARTS_PER_BATCH == 12 * 1024


def test_workspace_query_refusals(cabi):
    lib = cabi.lib
    x, y = C.c_int64(0), C.c_int64(0)
    q = lambda g, P=5, pitch=4, G=1, a=x, b=y: lib.tg_cluster_workspace_bytes(
        C.byref(g) if g is not None else None, C.c_int64(P), C.c_int64(pitch), C.c_int64(G),
        C.byref(a) if a is not None else None, C.byref(b) if b is not None else None)
    g = graph(cabi)
    assert q(g) == 0
    assert q(None) == 1 and q(g, a=None) == 1 and q(g, b=None) == 1
    assert q(g, P=-1) == 1 and q(g, pitch=-1) == 1 and q(g, G=-1) == 1 and q(g, G=1 << 31) == 1
    assert q(g, pitch=1025) == 1 and b"pitch_parts" in lib.tg_last_error()
    assert q(g, pitch=1024) == 0
    assert q(graph(cabi, n_major=-1)) == 1 and q(graph(cabi, n_edges=-1)) == 1
    assert q(graph(cabi, n_major=1 << 31)) == 0
    assert q(graph(cabi, n_major=(1 << 31) + 1)) == 3                     # TG_ERR_UNSUPPORTED
    assert b"2^31" in lib.tg_last_error()
    assert q(graph(cabi, n_edges=1 << 41)) == 1 and b"chunks per batch" in lib.tg_last_error()
    assert q(graph(cabi, n_edges=1 << 39), G=0x7fffffff) == 1 and b"overflow" in lib.tg_last_error()


# ---- refusals before any launch ------------------------------------------------------------------------------------------------
FAKE = 0x10000          # a non-null address that is never read: every call below is refused before anything is launched
BIG = 1 << 40           # a workspace size no shape below needs


def struct(cabi, partptr=FAKE, P=5, clusters=FAKE, pitch=4, n_clusters=None, node_ids=None):
    return cabi.TgClusterIn(partptr, P, clusters, pitch, n_clusters, node_ids)


def call_count(cabi, g="default", s="default", G=2, n_nodes=FAKE, n_edges=FAKE, status=FAKE, ws=FAKE, ws_bytes=BIG, **kw):
    g = graph(cabi, **{k: kw.pop(k) for k in ("n_major", "ptrs", "indices") if k in kw}) if g == "default" else g
    n_edges_graph = kw.pop("graph_edges", None)
    if n_edges_graph is not None:
        g.n_edges = n_edges_graph
    s = struct(cabi, **kw) if s == "default" else s
    p = C.c_void_p
    return cabi.lib.tg_cluster_count(C.byref(g) if g is not None else None, C.byref(s) if s is not None else None, C.c_int64(G),
                                     p(n_nodes), p(n_edges), p(status), p(ws), C.c_int64(ws_bytes), None)


def call_emit(cabi, g="default", s="default", G=2, node_off=FAKE, edge_off=FAKE, nodes=FAKE, rows=FAKE, cols=FAKE,
              eidx=FAKE, ws=FAKE, ws_bytes=BIG, **kw):
    g = graph(cabi, **{k: kw.pop(k) for k in ("n_major", "ptrs", "indices") if k in kw}) if g == "default" else g
    s = struct(cabi, **kw) if s == "default" else s
    p = C.c_void_p
    return cabi.lib.tg_cluster_emit(C.byref(g) if g is not None else None, C.byref(s) if s is not None else None, C.c_int64(G),
                                    p(node_off), p(edge_off), p(nodes), p(rows), p(cols), p(eidx), p(ws), C.c_int64(ws_bytes),
                                    None)


COMMON = [
    (dict(g=None), "null argument"),
    (dict(s=None), "null argument"),
    (dict(G=-1), "n_batches"),
    (dict(G=1 << 31), "n_batches"),
    (dict(n_major=-1), "negative graph size"),
    (dict(P=-1), "n_parts"),
    (dict(pitch=-1), "pitch_parts"),
    (dict(pitch=1025), "pitch_parts"),
    (dict(ws_bytes=-1), "negative"),
    (dict(ws=None), "workspace too small"),
    (dict(ws_bytes=2 * workspace_bytes(1000, 4) - 1), "workspace too small"),
    (dict(ws=FAKE + 4), "8-byte aligned"),
    (dict(ptrs=None), "null ptrs"),
    (dict(indices=None), "null ptrs"),
    (dict(partptr=None), "null partptr"),
    (dict(clusters=None), "null clusters"),
]


def test_the_short_workspace_of_the_table_above_is_one_byte_short(cabi):
    assert cabi.cluster_workspace_bytes(graph(cabi), 5, 4, 2)[0] == 2 * workspace_bytes(1000, 4)
    assert call_count(cabi, G=0, ws_bytes=0) == 0 and call_emit(cabi, G=0, ws_bytes=0) == 0       # nothing to launch


@pytest.mark.parametrize("kw, word", COMMON + [
    (dict(n_nodes=None), "null n_nodes"),
    (dict(n_edges=None), "null n_nodes"),
    (dict(status=None), "null n_nodes"),
])
def test_count_refusals(cabi, kw, word):
    assert call_count(cabi, **kw) == 1                                   # TG_ERR_INVALID
    assert re.search(word, cabi.lib.tg_last_error().decode()), cabi.lib.tg_last_error()


@pytest.mark.parametrize("kw, word", COMMON + [
    (dict(edge_off=None), "null edge_off"),
    (dict(rows=None), "null edge_off"),
    (dict(cols=None), "null edge_off"),
    (dict(eidx=None), "null edge_off"),
    (dict(node_off=None), "without node_off"),
])
def test_emit_refusals(cabi, kw, word):
    assert call_emit(cabi, **kw) == 1
    assert re.search(word, cabi.lib.tg_last_error().decode()), cabi.lib.tg_last_error()


def test_graph_limit_and_empty_launches(cabi):
    assert call_count(cabi, n_major=(1 << 31) + 1) == 3 and call_emit(cabi, n_major=(1 << 31) + 1) == 3   # TG_ERR_UNSUPPORTED
    assert b"2^31" in cabi.lib.tg_last_error()
    assert call_count(cabi, G=0) == 0 and call_emit(cabi, G=0) == 0       # nothing to launch
    assert call_emit(cabi, G=0, nodes=None, node_off=None) == 0           # nodes may be NULL
    assert call_count(cabi, G=0, clusters=None, pitch=0) == 0             # no lists at pitch 0


def test_status_wording(cabi):
    cabi.cluster_status_check(0, "x")
    for bit, word in ((1, "chunk bound"), (2, "cluster id"), (4, "partptr")):
        with pytest.raises(RuntimeError, match=word):
            cabi.cluster_status_check(bit, "x")
    with pytest.raises(RuntimeError, match="status 6 .*cluster id.* and .*partptr"):
        cabi.cluster_status_check(6, "x")


# ---- the partition helpers, ClusterData's and the loader's refusals -----------------------------------------------------------------
def test_partition_helpers(cabi):
    import tch_geometric
    from tch_geometric.loader import random_partition, range_partition
    assert tch_geometric.range_partition is range_partition and tch_geometric.random_partition is random_partition
    for N, P in ((10, 3), (7, 7), (5, 8), (1000, 16), (1, 1)):
        part = range_partition(N, P)
        assert part.dtype == torch.int64 and part.shape == (N,) and part.tolist() == [v * P // N for v in range(N)]
        sizes = np.bincount(part.numpy(), minlength=P)
        assert sizes.max() - sizes.min() <= 1 and (np.diff(part.numpy()) >= 0).all()
    assert range_partition(0, 4).numel() == 0
    a, b, c = random_partition(500, 7, 3), random_partition(500, 7, 3), random_partition(500, 7, 4)
    assert a.dtype == torch.int64 and torch.equal(a, b) and not torch.equal(a, c)
    assert int(a.min()) == 0 and int(a.max()) == 6
    for fn in (range_partition, random_partition):
        with pytest.raises(ValueError):
            fn(10, 0)
        with pytest.raises(ValueError):
            fn(-1, 2)


def _graph(n=5):
    from tch_geometric.transforms import Graph
    ei = torch.tensor([[0, 1, 2, 3, 4, 0], [1, 2, 3, 4, 0, 2]])
    return Graph(edge_index=ei, num_nodes=n)


@pytest.mark.parametrize("n, part, P, word", [
    (5, torch.zeros(4, dtype=torch.int64), None, "4 entries for 5 nodes"),
    (5, torch.zeros(5), None, "integer tensor"),
    (5, torch.zeros((5, 1), dtype=torch.int64), None, "integer tensor"),
    (5, [0, 0, 0, 0, 0], None, "integer tensor"),
    (5, torch.tensor([0, 1, -1, 0, 0]), None, "outside"),
    (5, torch.tensor([0, 1, 3, 0, 0]), 3, "outside"),
    (5, torch.tensor([0, 1, 2, 0, 0]), 0, "num_parts"),
    ((1 << 31) + 1, torch.zeros(5, dtype=torch.int64), None, "2\\^31"),
    (0, torch.zeros(0, dtype=torch.int64), None, "between 1 and"),
])
def test_cluster_data_refusals_need_no_device(cabi, n, part, P, word):
    import tch_geometric
    assert tch_geometric.ClusterData is tch_geometric.loader.ClusterData
    with pytest.raises(ValueError, match=word):
        tch_geometric.ClusterData(_graph(n), part, P, device="cuda:0")


@pytest.mark.parametrize("kw, word", [
    (dict(batch_size=0), "batch_size"),
    (dict(batch_size=-3), "batch_size"),
    (dict(batch_size=1025), "at most 1024"),
    (dict(prefetch=0), "prefetch"),
    (dict(), "ClusterData"),
])
def test_loader_refusals_need_no_device(cabi, kw, word):
    import tch_geometric
    assert tch_geometric.ClusterLoader is tch_geometric.loader.ClusterLoader
    with pytest.raises(ValueError, match=word):
        tch_geometric.ClusterLoader(object(), **kw)
