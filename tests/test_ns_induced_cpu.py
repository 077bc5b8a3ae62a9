"""Per-batch induced subgraph (tg_ns_induced_count / tg_ns_induced_emit), host-only parts: the NumPy statement of the rule
against a dense-adjacency statement, transforms.induced_subgraph on CPU tensors against it, the workspace sizes and the
argument checks that run before anything is launched.  No GPU: every device pointer handed over is null or a host buffer
that is never read."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from helpers import load_karate
from helpers_induced import csc_of, induced_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tg_ns_induced_workspace_bytes", "tg_ns_induced_count", "tg_ns_induced_emit")


@pytest.fixture(scope="module")
def cabi():
    if not os.path.exists(os.path.join(ROOT, "tch-geometric_amd", "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tch-geometric_amd"), "-s"])
    from tch_geometric import _cabi
    return _cabi


@pytest.fixture(scope="module")
def karate():
    ei, n = load_karate()
    return (ei, n) + csc_of(ei, n)


def lists(n):
    rs = np.random.default_rng(3)
    out = {"full": np.arange(n), "repeat": np.array([5, 0, 33, 0, 2, 5, 1])}
    for k, size in enumerate((3, 11, 25)):
        out["subset%d" % k] = rs.permutation(n)[:size]
    return out


def brute_force(nodes, ei, n):
    """the dense statement: count[s, t] parallel edges s -> t; for every target position i in order and every source s
    ascending (a CSC column holds its rows ascending), one triple per parallel edge, at consecutive CSC offsets"""
    A = np.zeros((n, n), dtype=np.int64)
    np.add.at(A, (ei[0], ei[1]), 1)
    col_start = np.concatenate([[0], np.cumsum(A.sum(axis=0))])
    first = {}
    for p, v in enumerate(nodes.tolist()):
        first.setdefault(v, p)
    out = []
    for i, t in enumerate(nodes.tolist()):
        e = int(col_start[t])
        for s in range(n):
            for _ in range(A[s, t]):
                if s in first:
                    out.append((first[s], i, e))
                e += 1
    return np.array(out, dtype=np.int64).reshape(-1, 3).T


@pytest.mark.parametrize("which", ["full", "subset0", "subset1", "subset2", "repeat"])
def test_rule_equals_the_dense_statement_on_karate(karate, which):
    ei, n, ptrs, idx, perm = karate
    nodes = lists(n)[which]
    rows, cols, eidx = induced_rule(nodes, ptrs, idx)
    want = brute_force(nodes, ei, n)
    assert np.array_equal(np.stack([rows, cols, eidx]), want)
    assert np.array_equal(ei[0][perm[eidx]], nodes[rows]) and np.array_equal(ei[1][perm[eidx]], nodes[cols])
    if which == "full":
        assert np.array_equal(eidx, np.arange(ei.shape[1]))                   # every edge, in CSC order


@pytest.mark.parametrize("which", ["full", "subset0", "subset1", "subset2", "repeat", "empty"])
def test_induced_subgraph_on_cpu_tensors_matches_the_rule(cabi, karate, which):
    from tch_geometric.transforms import induced_subgraph
    ei, n, ptrs, idx, _ = karate
    nodes = np.zeros(0, dtype=np.int64) if which == "empty" else lists(n)[which].astype(np.int64)
    got = induced_subgraph(torch.from_numpy(nodes), torch.from_numpy(ptrs), torch.from_numpy(idx))
    for g, w in zip(got, induced_rule(nodes, ptrs, idx)):
        assert g.dtype == torch.int64 and np.array_equal(g.numpy(), w)
    with pytest.raises(IndexError):
        induced_subgraph(torch.tensor([0, n]), torch.from_numpy(ptrs), torch.from_numpy(idx))
    with pytest.raises(IndexError):
        induced_subgraph(torch.tensor([-1]), torch.from_numpy(ptrs), torch.from_numpy(idx))
    with pytest.raises(ValueError):
        induced_subgraph(torch.from_numpy(nodes).to(torch.int32), torch.from_numpy(ptrs), torch.from_numpy(idx))


def test_symbols_and_struct(cabi):
    for name in NAMES:
        assert name in cabi.EXPORTS and hasattr(cabi.lib, name)
    assert [f for f, _ in cabi.TgNsInducedIn._fields_] == ["nodes", "pitch_nodes", "counts", "counts_stride", "node_marks",
                                                           "n_marks"]


def test_workspace_sizes(cabi):
    """bytes = n_batches * bytes_min; a batch holds a table of 2^k >= 4/3 pitch slots of (key, u32), a prefix word per
    position and a word per chunk, of which there are at most pitch + ceil(n_edges / chunk) with a chunk of at most 2 048"""
    g = cabi.graph_sizing(1 << 20, 1 << 24)
    total, least = cabi.ns_induced_workspace_bytes(g, 169984, 1 << 20, 16)
    assert total == 16 * least and least % 8 == 0
    assert least >= 262144 * 8 + 169984 * 4 + (169984 + (1 << 24) // 2048) * 4
    assert cabi.ns_induced_workspace_bytes(g, 169984, 1 << 20, 1) == (least, least)
    assert cabi.ns_induced_workspace_bytes(g, 169984, 1 << 20, 0)[0] == 0
    assert cabi.ns_induced_workspace_bytes(g, 2 * 169984, 1 << 20, 16)[1] > least          # grows with the pitch
    bigger = cabi.graph_sizing(1 << 20, 1 << 26)
    assert cabi.ns_induced_workspace_bytes(bigger, 169984, 1 << 20, 16)[1] > least         # ... with the graph's edges
    wide = cabi.ns_induced_workspace_bytes(g, 169984, 1 << 40, 16)[1]
    assert wide >= least + 262144 * 4                                                     # 64-bit keys
    for bad, word in (((g, -1, 1 << 20, 16), "pitch"), ((g, (1 << 30) + 1, 1 << 20, 16), "pitch_nodes"), ((g, 64, 0, 16), "id_bound"),
                      ((g, 64, 1 << 10, 16), "id_bound"), ((g, 64, 1 << 20, -1), "n_batches")):
        with pytest.raises(cabi.TchGeoError, match=word):
            cabi.ns_induced_workspace_bytes(*bad)
    out = C.c_int64(0)
    lib = cabi.lib
    assert lib.tg_ns_induced_workspace_bytes(None, C.c_int64(64), C.c_int64(64), C.c_int64(1), C.byref(out), C.byref(out)) == 1
    assert lib.tg_ns_induced_workspace_bytes(C.byref(g), C.c_int64(64), C.c_int64(1 << 20), C.c_int64(1), None, C.byref(out)) == 1


def _queries(cabi, g, pitch, n_batches):
    return (lambda: cabi.ns_induced_workspace_bytes(g, pitch, 64, n_batches),
            lambda: cabi.ns_induced_grouped_workspace_bytes(g, pitch, 64, 2, 0, n_batches))


def test_workspace_bytes_refuse_an_int64_overflow(cabi):
    """n_batches * bytes_min past 2^63 is refused by both induced queries (a batch of pitch 2^30 takes more than 2^33
    bytes, 2^31 - 1 of them more than 2^64), not answered with a wrapped product; one such batch still has its answer"""
    g = cabi.graph_sizing(64, 64)
    for query in _queries(cabi, g, 1 << 30, 2 ** 31 - 1):
        with pytest.raises(cabi.TchGeoError, match="overflow int64"):
            query()
    for query in _queries(cabi, g, 1 << 30, 1):
        total, least = query()
        assert total == least > 1 << 33


# (n_major, n_edges, pitch_nodes, id_bound) -> bytes_min of one batch, as the build before the shared answer gave it
BYTES_MIN_BEFORE = {(1 << 20, 1 << 24, 169984, 1 << 20): 5083136, (34, 156, 34, 34): 2304,
                    (1 << 16, 1 << 20, 124, 1 << 40): 22272}


@pytest.mark.parametrize("shape", sorted(BYTES_MIN_BEFORE))
def test_workspace_bytes_min_is_unchanged(cabi, shape):
    n_major, n_edges, pitch, id_bound = shape
    g = cabi.graph_sizing(n_major, n_edges)
    assert cabi.ns_induced_workspace_bytes(g, pitch, id_bound, 1) == (BYTES_MIN_BEFORE[shape],) * 2


HOST = C.create_string_buffer(64)                          # stands in for device arrays; never read
P = C.c_void_p(C.addressof(HOST))


def _call(cabi, which, graph=True, arrays=True, src=True, nodes=True, counts=True, outs=True, n_batches=4, id_bound=1 << 20,
          pitch=124, stride=2, n_marks=2, n_major=1 << 16, n_edges=1 << 20, ws="ok", ws_bytes=None):
    g = cabi.graph_sizing(n_major, n_edges)
    if arrays:
        g.ptrs, g.indices = P, P
    si = cabi.TgNsInducedIn()
    si.nodes, si.counts, si.node_marks = (P if nodes else None), (P if counts else None), P
    si.pitch_nodes, si.counts_stride, si.n_marks = pitch, stride, n_marks
    ok = cabi.graph_sizing(1 << 16, 1 << 20)
    least = cabi.ns_induced_workspace_bytes(ok, 124, 1 << 20, 4)[0]
    buf = C.create_string_buffer(16)
    base = (C.addressof(buf) + 7) & ~7
    wsp = {"ok": C.c_void_p(base), "null": None, "odd": C.c_void_p(base + 4)}[ws]
    nb = C.c_int64(least if ws_bytes is None else ws_bytes)
    o = P if outs else None
    gp, sp = (C.byref(g) if graph else None), (C.byref(si) if src else None)
    if which == "count":
        rc = cabi.lib.tg_ns_induced_count(gp, sp, C.c_int64(n_batches), C.c_int64(id_bound), o, o, o, wsp, nb, None)
    else:
        rc = cabi.lib.tg_ns_induced_emit(gp, sp, C.c_int64(n_batches), C.c_int64(id_bound), o, o, o, o, wsp, nb, None)
    return rc, cabi.lib.tg_last_error().decode()


@pytest.mark.parametrize("which", ["count", "emit"])
def test_refusals_before_any_launch(cabi, which):
    """Every bad argument returns TG_ERR_INVALID with a message that names the entry point and the argument.  The
    workspace is 16 host bytes and every array a host buffer: a launch would have faulted, a refusal touches nothing."""
    def refused(word, **kw):
        rc, msg = _call(cabi, which, **kw)
        assert rc == 1, (rc, msg)
        assert "tg_ns_induced_" + which in msg and word in msg, msg
    refused("null", graph=False)
    refused("null", src=False)
    refused("null", arrays=False)
    refused("null", nodes=False)
    refused("null", counts=False)
    refused("null", outs=False)
    refused("n_batches", n_batches=-1)
    refused("pitch", pitch=-5)
    refused("pitch_nodes", pitch=(1 << 30) + 1, ws_bytes=1 << 62)
    refused("negative", n_edges=-1)
    refused("negative", n_major=-1)
    refused("id_bound", id_bound=0)
    refused("id_bound", id_bound=1 << 10)                                     # below n_major
    refused("counts_stride", stride=0)
    refused("n_marks", n_marks=-1)
    refused("n_marks", n_marks=9)
    refused("workspace_bytes", ws_bytes=-1)
    refused("workspace too small", ws_bytes=_least(cabi) - 1)
    refused("workspace too small", ws="null", ws_bytes=1 << 40)               # a size without a workspace
    refused("aligned", ws="odd")


def _least(cabi):
    return cabi.ns_induced_workspace_bytes(cabi.graph_sizing(1 << 16, 1 << 20), 124, 1 << 20, 4)[0]
