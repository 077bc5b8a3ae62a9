"""The full-neighbour pair (tg_ns_full_workspace_bytes / _count / _emit, _cabi.NsFull, FullNeighborLoader), host-only parts:
the NumPy restatement against a brute-force dict version, the exports, the workspace formula, every refusal that comes
before a launch and the Python-side ValueErrors.  No GPU: every device pointer handed over is null or an address that is
never read."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from helpers_full import (blocks, chunk_bound, chunks_of, edges_of, full_rule, refused, status_of, table_slots,
                          workspace_bytes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tg_ns_full_workspace_bytes", "tg_ns_full_count", "tg_ns_full_emit")


@pytest.fixture(scope="module")
def cabi():
    if not os.path.exists(os.path.join(ROOT, "tch-geometric_amd", "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tch-geometric_amd"), "-s"])
    from tch_geometric import _cabi
    return _cabi


# ---- the restatement against brute force -------------------------------------------------------------------------------
def brute(ptrs, indices, nodes, n_major):
    """the contract of include/tchgeo.h, loop by loop"""
    out, triples, chunks = list(nodes), [], 0
    for i, v in enumerate(nodes):
        if not 0 <= v < n_major:
            continue
        chunks += -(-(ptrs[v + 1] - ptrs[v]) // 512)
        for e in range(ptrs[v], ptrs[v + 1]):
            src = indices[e]
            if src not in out:
                out.append(src)
            triples.append((out.index(src), i, e))
    return out, triples, chunks


def random_case(seed):
    rs = np.random.default_rng(seed)
    n = int(rs.integers(3, 40))
    deg = rs.integers(0, 6, n)
    deg[rs.integers(0, n, 3)] = 0                                    # empty columns
    ptrs = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = rs.integers(0, n, int(ptrs[-1])).astype(np.int64)      # self loops and parallel edges happen
    return rs, n, ptrs, indices


@pytest.mark.parametrize("seed", range(12))
def test_rule_equals_brute_force(seed):
    rs, n, ptrs, indices = random_case(seed)
    lists = (rs.permutation(n)[:max(1, n // 2)], rs.integers(0, n, 7), np.arange(n)[::-1], np.zeros(0, np.int64),
             np.array([0, n, -1, 0, n - 1]))                         # distinct, with repeats, all, none, out of range
    for nodes in lists:
        out, rows, cols, e = full_rule(ptrs, indices, nodes)
        want_out, want, want_chunks = brute(ptrs.tolist(), indices.tolist(), [int(v) for v in nodes], n)
        assert out.tolist() == want_out and list(zip(rows.tolist(), cols.tolist(), e.tolist())) == want
        assert chunks_of(ptrs, nodes) == want_chunks and edges_of(ptrs, nodes) == len(want)
        assert status_of(ptrs, nodes) == (2 if any(not 0 <= v < n for v in nodes.tolist()) else 0)
        assert np.array_equal(out[rows], indices[e]) and np.array_equal(out[:nodes.size], nodes)


def test_chained_blocks_and_the_refusal_rule():
    _, n, ptrs, indices = random_case(3)
    b = blocks(ptrs, indices, [1, 2], 2)
    assert len(b) == 2 and b[0][1] == 2 and b[1][1] == b[0][0].size
    assert np.array_equal(b[1][0][:b[0][0].size], b[0][0])           # F_1 is the prefix of F_2
    assert np.array_equal(b[1][0], full_rule(ptrs, indices, b[0][0])[0])
    assert chunk_bound(10, 1025) == 13 and chunk_bound(10, 1025, 7) == 7
    assert not refused(4, 10, 3, 14, 3, 100) and refused(4, 10, 3, 13, 3, 100)      # n + m against node_cap
    assert not refused(4, 10, 3, 9, 3, 5) and refused(4, 10, 3, 8, 3, 5)            # min(m, id_bound)
    assert refused(4, 10, 4, 14, 3, 100) and refused(0, 1 << 31, 0, 1 << 30, 1 << 31, 5)
    assert not refused(0, (1 << 31) - 1, 0, 5, 0, 5)


# ---- exports and the workspace formula ---------------------------------------------------------------------------------------
def test_symbols_and_struct(cabi):
    header = open(os.path.join(ROOT, "include", "tchgeo.h")).read()
    for name in NAMES:
        assert name in cabi.EXPORTS and hasattr(cabi.lib, name)
        assert "TG_API int %s(" % name in header
        assert getattr(cabi.lib, name).argtypes
    assert [f for f, _ in cabi.TgNsFullIn._fields_] == ["nodes", "node_ptr", "max_nodes", "node_cap", "chunk_cap"]
    assert cabi.NS_FULL_MAX_NODES == 1 << 30 and cabi.NS_FULL_MAX_CHUNKS == 1 << 31


def graph(cabi, n_major=100, n_edges=1000, ptrs=0x10000, indices=0x10000):
    g = cabi.TgGraph()
    g.ptrs, g.indices, g.n_major, g.n_edges = ptrs, indices, n_major, n_edges
    return g


def test_workspace_formula(cabi):
    q = cabi.ns_full_workspace_bytes
    for E, mx, cap, cc in ((0, 0, 0, 0), (1000, 1, 1, 0), (40000, 37, 900, 0), (511, 1024, 1024, 0), (512, 1025, 5000, 3),
                           (513, 3, 3, 1), (1 << 28, 1024, 1 << 20, 0), (1 << 33, 1 << 20, 1 << 30, 1 << 31)):
        for bound in (100, 1 << 31, (1 << 31) + 1):
            per = workspace_bytes(E, mx, cap, cc, bound)
            assert q(graph(cabi, n_edges=E), bound, mx, cap, cc, 7) == (7 * per, per)          # bytes == n_batches * bytes_min
            assert q(graph(cabi, n_edges=E), bound, mx, cap, cc, 0) == (0, per)
    g = graph(cabi)
    sizes = [q(g, 100, 10, cap, 5, 1)[1] for cap in (10, 100, 1000, 10000, 1 << 20)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]                                     # monotone in node_cap
    sizes = [q(g, 100, 10, 10, cc, 1)[1] for cc in (1, 100, 10000, 1 << 20, 1 << 31)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]                                     # and in chunk_cap
    assert q(g, 100, 10, 10, 0, 1) == q(g, 100, 10, 10, 10 + 2, 1)                             # the default bound: 10 + ceil(1000 / 512)
    # the key width switches at id_bound = 2^31: four more bytes per slot
    narrow, wide = q(g, 1 << 31, 10, 3000, 5, 1)[1], q(g, (1 << 31) + 1, 10, 3000, 5, 1)[1]
    assert table_slots(3000) == 4096 and wide - narrow == 4 * 4096


def test_workspace_query_refusals(cabi):
    lib = cabi.lib
    x, y = C.c_int64(0), C.c_int64(0)

    def q(g, mx=4, cap=8, cc=0, bound=100, G=1, a=x, b=y, s="default"):
        s = cabi.TgNsFullIn(None, None, mx, cap, cc) if s == "default" else s
        return lib.tg_ns_full_workspace_bytes(C.byref(g) if g is not None else None, C.byref(s) if s is not None else None,
                                              C.c_int64(bound), C.c_int64(G), C.byref(a) if a is not None else None,
                                              C.byref(b) if b is not None else None)
    g = graph(cabi)
    assert q(g) == 0
    assert q(None) == 1 and q(g, s=None) == 1 and q(g, a=None) == 1 and q(g, b=None) == 1
    assert q(g, G=-1) == 1 and q(g, G=1 << 31) == 1 and b"n_batches" in lib.tg_last_error()
    assert q(g, mx=-1) == 1 and b"max_nodes" in lib.tg_last_error()
    assert q(g, mx=(1 << 30) + 1, cap=(1 << 30) + 1) == 1 and b"max_nodes" in lib.tg_last_error()
    assert q(g, mx=4, cap=3) == 1 and b"node_cap" in lib.tg_last_error()
    assert q(g, cap=(1 << 30) + 1) == 1 and b"node_cap" in lib.tg_last_error()
    assert q(g, mx=1 << 30, cap=1 << 30, cc=1) == 0
    assert q(g, cc=(1 << 31) + 1) == 1 and b"chunk_cap" in lib.tg_last_error()
    assert q(g, cc=1 << 31) == 0
    assert q(g, bound=99) == 1 and b"below n_major" in lib.tg_last_error()
    assert q(graph(cabi, n_major=0), bound=0) == 1 and b"id_bound" in lib.tg_last_error()
    assert q(graph(cabi, n_major=-1)) == 1 and q(graph(cabi, n_edges=-1)) == 1
    assert q(graph(cabi, n_edges=1 << 41)) == 1 and b"chunks per batch" in lib.tg_last_error()
    assert q(g, cc=1 << 31, G=0x7fffffff) == 1 and b"overflow" in lib.tg_last_error()


# ---- refusals before any launch ------------------------------------------------------------------------------------------------
FAKE = 0x10000          # a non-null address that is never read: every call below is refused before anything is launched
BIG = 1 << 40           # a workspace size no shape below needs


def call(cabi, which, g="default", s="default", G=2, bound=100, ws=FAKE, ws_bytes=BIG, **kw):
    g = graph(cabi, **{k: kw.pop(k) for k in ("n_major", "ptrs", "indices") if k in kw}) if g == "default" else g
    if s == "default":
        s = cabi.TgNsFullIn(kw.pop("nodes", FAKE), kw.pop("node_ptr", FAKE), kw.pop("mx", 4), kw.pop("cap", 8), kw.pop("cc", 0))
    p = C.c_void_p
    gp, sp = (C.byref(g) if g is not None else None), (C.byref(s) if s is not None else None)
    if which == "count":
        out = [p(kw.pop(k, FAKE)) for k in ("n_nodes", "n_edges", "chunks", "status")]
        assert not kw
        return cabi.lib.tg_ns_full_count(gp, sp, C.c_int64(G), C.c_int64(bound), *out, p(ws), C.c_int64(ws_bytes), None)
    out = [p(kw.pop(k, FAKE)) for k in ("node_off", "edge_off", "nodes_out", "rows", "cols", "eidx")]
    assert not kw
    return cabi.lib.tg_ns_full_emit(gp, sp, C.c_int64(G), C.c_int64(bound), *out, p(ws), C.c_int64(ws_bytes), None)


COMMON = [
    (dict(g=None), "null argument"),
    (dict(s=None), "null argument"),
    (dict(G=-1), "n_batches"),
    (dict(G=1 << 31), "n_batches"),
    (dict(n_major=-1), "negative graph size"),
    (dict(mx=-1), "max_nodes"),
    (dict(mx=(1 << 30) + 1), "max_nodes"),
    (dict(cap=3), "node_cap"),
    (dict(cap=(1 << 30) + 1), "node_cap"),
    (dict(cc=(1 << 31) + 1), "chunk_cap"),
    (dict(bound=0), "id_bound"),
    (dict(bound=99), "below n_major"),
    (dict(ws_bytes=-1), "negative"),
    (dict(ws=None), "workspace too small"),
    (dict(ws_bytes=2 * workspace_bytes(1000, 4, 8, 0, 100) - 1), "workspace too small"),
    (dict(ws=FAKE + 4), "8-byte aligned"),
    (dict(ptrs=None), "null ptrs"),
    (dict(indices=None), "null ptrs"),
    (dict(node_ptr=None), "null node_ptr"),
    (dict(nodes=None), "null nodes"),
]


def test_the_short_workspace_of_the_table_above_is_one_byte_short(cabi):
    assert cabi.ns_full_workspace_bytes(graph(cabi), 100, 4, 8, 0, 2)[0] == 2 * workspace_bytes(1000, 4, 8, 0, 100)
    for which in ("count", "emit"):
        assert call(cabi, which, G=0, ws_bytes=0) == 0               # nothing to launch


@pytest.mark.parametrize("kw, word", COMMON + [
    (dict(n_nodes=None), "null n_nodes"),
    (dict(n_edges=None), "null n_nodes"),
    (dict(status=None), "null n_nodes"),
])
def test_count_refusals(cabi, kw, word):
    assert call(cabi, "count", **kw) == 1                            # TG_ERR_INVALID
    assert re.search(word, cabi.lib.tg_last_error().decode()), cabi.lib.tg_last_error()


@pytest.mark.parametrize("kw, word", COMMON + [
    (dict(edge_off=None), "null edge_off"),
    (dict(rows=None), "null edge_off"),
    (dict(cols=None), "null edge_off"),
    (dict(eidx=None), "null edge_off"),
    (dict(node_off=None), "without node_off"),
])
def test_emit_refusals(cabi, kw, word):
    assert call(cabi, "emit", **kw) == 1
    assert re.search(word, cabi.lib.tg_last_error().decode()), cabi.lib.tg_last_error()


def test_empty_launches(cabi):
    assert call(cabi, "count", G=0) == 0 and call(cabi, "emit", G=0) == 0      # nothing to launch
    assert call(cabi, "count", G=0, chunks=None) == 0                          # chunks may be NULL
    assert call(cabi, "emit", G=0, nodes_out=None, node_off=None) == 0         # nodes_out may be NULL
    assert call(cabi, "count", G=0, nodes=None, mx=0, cap=0) == 0              # no lists at max_nodes 0


# ---- the Python-side refusals ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, word", [
    (dict(max_nodes=-1), "max_nodes"),
    (dict(max_nodes=(1 << 30) + 1, node_cap=(1 << 30) + 1), "max_nodes"),
    (dict(node_cap=3), "node_cap"),
    (dict(node_cap=(1 << 30) + 1), "node_cap"),
    (dict(chunk_cap=(1 << 31) + 1), "chunk_cap"),
    (dict(n_batches=-1), "n_batches"),
    (dict(n_batches=1 << 31), "n_batches"),
    (dict(id_bound=99), "id_bound"),
])
def test_ns_full_refusals_need_no_device(cabi, kw, word):
    args = dict(id_bound=100, max_nodes=4, node_cap=8, chunk_cap=0, n_batches=2)
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        cabi.NsFull(graph(cabi), device="cuda:0", **args)
    cabi.ns_full_status_check(0, "x")
    cabi.ns_full_status_check(1, "x")                                # a refused batch is the caller's to answer
    with pytest.raises(RuntimeError, match="outside the graph"):
        cabi.ns_full_status_check(3, "x")


def _graph(n=5):
    from tch_geometric.transforms import Graph
    ei = torch.tensor([[0, 1, 2, 3, 4, 0], [1, 2, 3, 4, 0, 2]])
    return Graph(edge_index=ei, num_nodes=n)


@pytest.mark.parametrize("n, kw, err, word", [
    (5, dict(num_layers=0), ValueError, "num_layers"),
    (5, dict(num_layers=9), ValueError, "num_layers"),
    (5, dict(batch_size=0), ValueError, "batch_size"),
    (5, dict(prefetch=0), ValueError, "prefetch"),
    (5, dict(input_nodes=torch.tensor([0, 5])), IndexError, "outside"),
    (5, dict(input_nodes=torch.tensor([-1, 2])), IndexError, "outside"),
    (5, dict(input_nodes=torch.tensor([0, 1, 2, 2]), batch_size=2), ValueError, "inside one mini-batch"),
    (5, dict(input_nodes=torch.tensor([0, 1, 2, 1]), batch_size=2, shuffle=True), ValueError, "anywhere"),
    ((1 << 31) + 1, dict(), ValueError, "2\\^31"),
    (0, dict(), ValueError, "between 1 and"),
])
def test_loader_refusals_need_no_device(cabi, n, kw, err, word):
    import tch_geometric
    assert tch_geometric.FullNeighborLoader is tch_geometric.loader.FullNeighborLoader
    with pytest.raises(err, match=word):
        tch_geometric.FullNeighborLoader(_graph(n), device="cuda:0", **kw)
