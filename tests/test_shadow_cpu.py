"""Induced edges per subgraph (tg_ns_induced_grouped_count / _emit, ShaDowKHopLoader), host-only parts: the NumPy statement
of the rule against a brute-force one and against the ungrouped rule, transforms.induced_subgraph(group=...) on CPU tensors,
the loader's refusals, the workspace query and the argument checks that run before anything is launched.  No GPU: every
device pointer handed over is null or a host buffer that is never read."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from helpers import load_karate
from helpers_induced import csc_of, induced_rule
from helpers_shadow import CHUNK, chunks_of, grouped_induced_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tg_ns_induced_grouped_workspace_bytes", "tg_ns_induced_grouped_count", "tg_ns_induced_grouped_emit")


@pytest.fixture(scope="module")
def cabi():
    if not os.path.exists(os.path.join(ROOT, "tch-geometric_amd", "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tch-geometric_amd"), "-s"])
    from tch_geometric import _cabi
    return _cabi


def random_case(seed, n=12, n_edges=60, length=30, n_groups=4):
    """a small multigraph (parallel edges, self loops) with times, and a list in which nodes repeat inside and across groups"""
    rs = np.random.default_rng(seed)
    ei = rs.integers(0, n, (2, n_edges)).astype(np.int64)
    ptrs, idx, perm = csc_of(ei, n)
    ts = rs.integers(0, 20, n_edges).astype(np.int64)          # in CSC order
    nodes = rs.integers(0, n, length).astype(np.int64)
    group = rs.integers(0, n_groups, length).astype(np.int64)
    group_time = rs.integers(5, 25, n_groups).astype(np.int64)
    return ptrs, idx, ts, nodes, group, group_time


def brute_force(nodes, group, ptrs, idx, ts=None, group_time=None, window=None):
    """every (target position, CSC offset, source position) triple tested on its own: O(n * E * n)"""
    col_of = np.repeat(np.arange(ptrs.size - 1), np.diff(ptrs))
    out = []
    for i in range(nodes.size):
        for e in range(idx.size):
            if col_of[e] != nodes[i]:
                continue
            if group_time is not None and not window[0] <= int(group_time[group[i]]) - int(ts[e]) <= window[1]:
                continue
            for j in range(nodes.size):
                if nodes[j] == idx[e] and group[j] == group[i]:
                    out.append((j, i, e))
                    break                                      # the first position
    return np.array(out, dtype=np.int64).reshape(-1, 3).T


@pytest.mark.parametrize("seed", range(6))
def test_rule_equals_brute_force(seed):
    ptrs, idx, ts, nodes, group, group_time = random_case(seed)
    assert len(set(zip(group.tolist(), nodes.tolist()))) < nodes.size                  # repeats inside a group ...
    assert any(len(set(group[nodes == v].tolist())) > 1 for v in set(nodes.tolist()))  # ... and one node under two groups
    got = np.stack(grouped_induced_rule(nodes, group, ptrs, idx))
    assert got.shape[1] > 0 and np.array_equal(got, brute_force(nodes, group, ptrs, idx))
    assert (group[got[0]] == group[got[1]]).all()
    for window in ((0, 1 << 62), (3, 9), (-4, 0)):
        timed = np.stack(grouped_induced_rule(nodes, group, ptrs, idx, ts, group_time, window))
        assert np.array_equal(timed, brute_force(nodes, group, ptrs, idx, ts, group_time, window)), window
    assert timed.shape[1] < got.shape[1]


@pytest.mark.parametrize("seed", range(4))
def test_rule_against_the_ungrouped_rule(seed):
    ptrs, idx, _, nodes, group, _ = random_case(seed)
    one = grouped_induced_rule(nodes, np.zeros_like(nodes), ptrs, idx)
    for a, b in zip(one, induced_rule(nodes, ptrs, idx)):                              # one group: the ungrouped rule outright
        assert np.array_equal(a, b)
    parts = []
    for g in np.unique(group):                                                         # group g: the rule on g's sub-list ...
        at = np.nonzero(group == g)[0]
        rows, cols, e = induced_rule(nodes[at], ptrs, idx)
        parts.append(np.stack([at[rows], at[cols], e]))                                # ... with positions mapped back
    merged = np.concatenate(parts, axis=1)
    merged = merged[:, np.lexsort((merged[2], merged[1]))]                             # merged by (i, e)
    assert np.array_equal(np.stack(grouped_induced_rule(nodes, group, ptrs, idx)), merged)


def test_rule_skips_bad_positions_and_counts_chunks():
    ptrs = np.array([0, 600, 600, 1113, 1113], dtype=np.int64)                         # columns of 600, 0, 513, 0
    idx = np.concatenate([np.arange(600) % 4, np.arange(513) % 4]).astype(np.int64)
    nodes, group = np.array([0, 2, 0, 4, 1, 2]), np.array([0, 0, 1, 0, 0, 7])
    assert chunks_of(nodes, ptrs) == 2 + 2 + 2 + 0 + 0 + 2
    assert chunks_of(nodes, ptrs, group, n_groups=2) == 2 + 2 + 2                      # position 5: no group, no column
    assert CHUNK == 512
    rows, cols, e = grouped_induced_rule(nodes, group, ptrs, idx, n_groups=2)
    assert 3 not in cols and 5 not in cols and 3 not in rows and 5 not in rows
    assert set(cols.tolist()) == {0, 1, 2} and (group[rows] == group[cols]).all()


@pytest.mark.parametrize("seed", range(4))
def test_transform_on_cpu_tensors(cabi, seed):
    from tch_geometric.transforms import induced_subgraph
    ptrs, idx, ts, nodes, group, group_time = random_case(seed)
    t = torch.from_numpy
    plain = induced_subgraph(t(nodes), t(ptrs), t(idx))
    for a, b in zip(plain, induced_rule(nodes, ptrs, idx)):                            # group=None: today's call
        assert np.array_equal(a.numpy(), b)
    got = induced_subgraph(t(nodes), t(ptrs), t(idx), group=t(group))
    for a, b in zip(got, grouped_induced_rule(nodes, group, ptrs, idx)):
        assert a.dtype == torch.int64 and np.array_equal(a.numpy(), b)
    for window in ((0, 1 << 62), (3, 9), (-4, 0)):
        got = induced_subgraph(t(nodes), t(ptrs), t(idx), group=t(group), group_time=t(group_time), edge_time=t(ts),
                               time_window=window)
        for a, b in zip(got, grouped_induced_rule(nodes, group, ptrs, idx, ts, group_time, window)):
            assert np.array_equal(a.numpy(), b), window
    empty = induced_subgraph(t(nodes[:0]), t(ptrs), t(idx), group=t(group[:0]))
    assert all(x.numel() == 0 for x in empty)
    with pytest.raises(ValueError):
        induced_subgraph(t(nodes), t(ptrs), t(idx), group=t(group[:-1]))
    with pytest.raises(ValueError):
        induced_subgraph(t(nodes), t(ptrs), t(idx), group=t(group), group_time=t(group_time))
    with pytest.raises(ValueError):
        induced_subgraph(t(nodes), t(ptrs), t(idx), time_window=(0, 1))
    with pytest.raises(IndexError):
        induced_subgraph(t(nodes), t(ptrs), t(idx), group=t(group - 1))


def _graph(**attrs):
    from tch_geometric.transforms import Graph
    ei = torch.tensor([[0, 1, 2, 3, 4, 0], [1, 2, 3, 4, 0, 2]])
    return Graph(edge_index=ei, num_nodes=5, time=torch.arange(6), **attrs)


@pytest.mark.parametrize("args, kw, word", [
    ((0, 3), {}, "depth"),
    ((2, 0), {}, "num_neighbors"),
    ((2, 65), dict(time_attr="time", input_time=torch.zeros(5, dtype=torch.int64), temporal_strategy="last"), "up to 64"),
    ((2, 3), dict(chunk_cap=0), "chunk_cap"),
    ((2, 3), dict(time_attr="time"), "come together"),
    ((2, 3), dict(temporal_strategy="first"), "temporal_strategy"),
])
def test_loader_refusals_need_no_device(cabi, args, kw, word):
    from tch_geometric.loader import ShaDowKHopLoader
    with pytest.raises(ValueError, match=word):
        ShaDowKHopLoader(_graph(), *args, device="cuda:0", **kw)


@pytest.mark.parametrize("name", ["batch", "root_n_id"])
def test_loader_refuses_data_that_hides_its_fields(cabi, name):
    import tch_geometric
    assert tch_geometric.ShaDowKHopLoader is tch_geometric.loader.ShaDowKHopLoader
    with pytest.raises(ValueError, match=name):
        tch_geometric.ShaDowKHopLoader(_graph(**{name: torch.zeros(5)}), 2, 3, device="cuda:0")


def test_neighbor_loader_still_refuses_the_combination(cabi):
    from tch_geometric.loader import NeighborLoader, ShaDowKHopLoader
    assert ShaDowKHopLoader.INDUCED_PER_SUBGRAPH and not NeighborLoader.INDUCED_PER_SUBGRAPH
    with pytest.raises(ValueError, match="out of scope"):
        NeighborLoader(_graph(), [2, 2], unique=True, induced=True, disjoint=True, device="cuda:0")


def test_symbols_struct_and_status_text(cabi):
    for name in NAMES:
        assert name in cabi.EXPORTS and hasattr(cabi.lib, name)
    assert [f for f, _ in cabi.TgNsInducedGroupedIn._fields_] == [
        "nodes", "group", "pitch_nodes", "counts", "counts_stride", "node_marks", "n_marks", "n_groups", "group_time",
        "window_lo", "window_hi", "chunk_cap"]
    with pytest.raises(RuntimeError, match="group word"):
        cabi.induced_status_check(4, "x")
    with pytest.raises(RuntimeError, match="chunk bound.*group word"):
        cabi.induced_status_check(5, "x")
    cabi.induced_status_check(0, "x")


def test_workspace_query(cabi):
    """touches no device; the default capacity is the ungrouped bound; grows with chunk_cap, the groups' key width, the pitch"""
    g = cabi.graph_sizing(1 << 20, 1 << 24)
    pitch, idb = 169984, 1 << 20
    plain = cabi.ns_induced_workspace_bytes(g, pitch, idb, 16)
    q = lambda n_groups, cap, nb=16, pitch=pitch, idb=idb: cabi.ns_induced_grouped_workspace_bytes(g, pitch, idb, n_groups, cap, nb)
    assert q(1, 0) == plain and q(1, -5) == plain                                   # one group, the default: the ungrouped size
    default = cabi.ns_induced_default_chunk_cap(g, pitch)
    assert default == pitch + (1 << 24) // CHUNK and q(1, default) == plain
    total, least = q(1024, 0)
    assert total == 16 * least and q(1024, 0, nb=1) == (least, least) and q(1024, 0, nb=0)[0] == 0
    assert least == plain[1]                                                        # 2^10 * 2^20 <= 2^31: still 32-bit keys
    wide = q(4096, 0)[1]
    assert wide >= least + 262144 * 4                                               # 64-bit keys
    small, big = q(1024, 1000)[1], q(1024, 1000 + 4096)[1]
    assert small < least and big - small >= 4096 * 8                                # a word per chunk
    assert q(1024, 1 << 31)[1] > (1 << 31) * 8
    for bad, word in (((1024, (1 << 31) + 1), "chunk_cap"), ((0, 0), "n_groups"), ((-1, 0), "n_groups"),
                      ((1 << 31, 0), "n_groups"), ((1 << 43, 0), "n_groups")):
        with pytest.raises(cabi.TchGeoError, match=word):
            q(*bad)
    with pytest.raises(cabi.TchGeoError, match="2\\^63"):                           # n_groups * id_bound >= 2^63
        q((1 << 31) - 1, 0, idb=1 << 33)
    with pytest.raises(cabi.TchGeoError, match="n_batches"):
        q(4, 0, nb=-1)
    out = C.c_int64(0)
    assert cabi.lib.tg_ns_induced_grouped_workspace_bytes(None, C.c_int64(64), C.c_int64(64), C.c_int64(1), C.c_int64(0),
                                                          C.c_int64(1), C.byref(out), C.byref(out)) == 1


HOST = C.create_string_buffer(64)                          # stands in for device arrays; never read
P = C.c_void_p(C.addressof(HOST))


def _call(cabi, which, graph=True, arrays=True, src=True, nodes=True, group=True, counts=True, outs=True, n_batches=4,
          id_bound=1 << 20, pitch=124, stride=2, n_marks=2, n_groups=8, times=False, graph_times=False, chunk_cap=0,
          ws="ok", ws_bytes=None):
    g = cabi.graph_sizing(1 << 16, 1 << 20)
    if arrays:
        g.ptrs, g.indices = P, P
    if graph_times:
        g.timestamps = P
    si = cabi.TgNsInducedGroupedIn()
    si.nodes, si.group, si.counts, si.node_marks = (P if nodes else None), (P if group else None), (P if counts else None), P
    si.pitch_nodes, si.counts_stride, si.n_marks, si.n_groups = pitch, stride, n_marks, n_groups
    si.group_time, si.window_lo, si.window_hi, si.chunk_cap = (P if times else None), 0, 10, chunk_cap
    least = _least(cabi)
    buf = C.create_string_buffer(16)
    base = (C.addressof(buf) + 7) & ~7
    wsp = {"ok": C.c_void_p(base), "null": None, "odd": C.c_void_p(base + 4)}[ws]
    nb = C.c_int64(least if ws_bytes is None else ws_bytes)
    o = P if outs else None
    gp, sp = (C.byref(g) if graph else None), (C.byref(si) if src else None)
    if which == "count":
        rc = cabi.lib.tg_ns_induced_grouped_count(gp, sp, C.c_int64(n_batches), C.c_int64(id_bound), o, o, o, o, wsp, nb, None)
    else:
        rc = cabi.lib.tg_ns_induced_grouped_emit(gp, sp, C.c_int64(n_batches), C.c_int64(id_bound), o, o, o, o, wsp, nb, None)
    return rc, cabi.lib.tg_last_error().decode()


def _least(cabi, chunk_cap=0):
    return cabi.ns_induced_grouped_workspace_bytes(cabi.graph_sizing(1 << 16, 1 << 20), 124, 1 << 20, 8, chunk_cap, 4)[0]


@pytest.mark.parametrize("which", ["count", "emit"])
def test_refusals_before_any_launch(cabi, which):
    """Every bad argument returns TG_ERR_INVALID with a message that names the entry point and the argument.  The
    workspace is 16 host bytes and every array a host buffer: a launch would have faulted, a refusal touches nothing."""
    def refused(word, **kw):
        rc, msg = _call(cabi, which, **kw)
        assert rc == 1, (rc, msg)
        assert "tg_ns_induced_grouped_" + which in msg and word in msg, msg
    refused("null", graph=False)
    refused("null", src=False)
    refused("null", arrays=False)
    refused("null", nodes=False)
    refused("null group", group=False)
    refused("null", counts=False)
    refused("null", outs=False)
    refused("n_groups", n_groups=0)
    refused("n_groups", n_groups=-3)
    refused("n_groups", n_groups=1 << 31)
    refused("2^63", n_groups=1 << 30, id_bound=1 << 33)
    refused("timestamps", times=True)                                         # times without graph timestamps
    refused("chunk_cap", chunk_cap=(1 << 31) + 1)
    refused("n_batches", n_batches=-1)
    refused("pitch", pitch=-5)
    refused("id_bound", id_bound=0)
    refused("id_bound", id_bound=1 << 10)                                     # below n_major
    refused("counts_stride", stride=0)
    refused("n_marks", n_marks=9)
    refused("workspace too small", ws_bytes=_least(cabi) - 1)
    refused("workspace too small", chunk_cap=1 << 20, ws_bytes=_least(cabi, 1 << 20) - 1)   # the capacity is part of the size
    refused("workspace too small", ws="null", ws_bytes=1 << 40)
    refused("aligned", ws="odd")
