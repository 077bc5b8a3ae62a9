"""Workspace sizing of the window-ordered form and the pipeline it lets a launch take: pure host queries on graph and
output descriptors, so no GPU is needed (nothing is allocated or launched; the pointers are never dereferenced).

include/tchgeo.h promises that a workspace sized without a graph is the larger size; under the default tuning
(staged = 2, AUTO) that has to include the stage slots from 2 048 batches on, or a NeighborLoader-style caller never
reaches the staged pipeline the bench figure measures."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAN = [15, 10]
B = 1024                    # the bench shape: 1 024 seeds per batch, [15, 10]
AUTO_MIN = 2048             # WIN_STAGED_AUTO_MIN_BATCHES


@pytest.fixture(scope="module")
def cabi():
    if not os.path.exists(os.path.join(ROOT, "tch-geometric_amd", "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tch-geometric_amd"), "-s"])
    from tch_geometric import _cabi
    before = _cabi.ns_win_tuning()
    _cabi.ns_win_tuning_set(staged=2)
    yield _cabi
    _cabi.ns_win_tuning_set(staged=before["staged"])


def _graph(cabi, scale, avg_degree, max_degree):
    """An RMAT-like CSC descriptor with u32 shadows (as the loader and the bench build it); max_degree 0 = unknown."""
    g = cabi.TgGraph()
    g.ptrs, g.indices, g.indices32, g.ptrs32 = 0x10000, 0x20000, 0x30000, 0x40000
    g.n_major, g.n_edges, g.max_degree = 1 << scale, (1 << scale) * avg_degree, max_degree
    return g


class _Out:
    """NsBatchedOut's descriptor without the device slabs (the queries read only the pitches)."""

    def __init__(self, cabi, n_seeds, fanout):
        self.cap_nodes, self.cap_edges = cabi.ns_homo_capacity(n_seeds, fanout)

    def struct(self):
        from tch_geometric._cabi import TgNsOut
        s = TgNsOut()
        s.samples, s.rows, s.cols, s.edge_index = 0x100000, 0x200000, 0x300000, 0x400000
        s.layer_offsets, s.counts = 0x500000, 0x600000
        s.cap_nodes, s.cap_edges = self.cap_nodes, self.cap_edges
        return s


def _bytes(cabi, graph, n_batches, staged=None):
    prev = cabi.ns_win_tuning_set(staged=staged) if staged is not None else None
    try:
        n = C.c_int64(0)
        fan = (C.c_int64 * len(FAN))(*FAN)
        cabi.check(cabi.lib.tg_ns_homo_workspace_bytes_for(C.byref(graph) if graph is not None else None,
                                                           C.c_int64(n_batches), C.c_int64(B), fan, C.c_int32(len(FAN)),
                                                           C.byref(n)))
        return n.value
    finally:
        if prev is not None:
            cabi.ns_win_tuning_set(staged=prev["staged"])


class _Ws:
    """What ns_homo_batched_staged reads of a workspace tensor: its size."""

    def __init__(self, nbytes):
        self._n = nbytes // 8 + 1

    def numel(self):
        return self._n


def test_graph_free_size_covers_every_graph_under_auto(cabi):
    one = _graph(cabi, 24, 16, 4096)     # slots fit one chunk: 40 + 10 x (24 + 12) bits <= 512
    two = _graph(cabi, 24, 16, 0)        # max_degree unknown: positions take 28 bits, 40 + 10 x 52 > 512: two chunks
    for G in (AUTO_MIN, 4096):
        free = _bytes(cabi, None, G)
        push = _bytes(cabi, two, G)                       # AUTO refuses two-chunk slots: the push pipeline's size
        assert _bytes(cabi, one, G) > push                # one-chunk slots: the stage slots are included
        assert free >= _bytes(cabi, two, G, staged=1)     # two-chunk slots, the most a graph can ask for
        assert free >= _bytes(cabi, one, G) > push
    # below the AUTO threshold no launch takes the staged pipeline: the graph-free size stays the push size
    assert _bytes(cabi, None, AUTO_MIN - 1) == _bytes(cabi, two, AUTO_MIN - 1)
    # staged = 0: never the stage slots, with or without a graph
    assert _bytes(cabi, None, AUTO_MIN, staged=0) == _bytes(cabi, one, AUTO_MIN, staged=0) == _bytes(cabi, two, AUTO_MIN)


def test_loader_style_launch_reaches_the_staged_pipeline(cabi):
    """The bench shape on an RMAT-24-sized graph under AUTO (form 0): the staged pipeline needs the longest column in the
    graph view AND a workspace with the stage slots; a graph-free workspace now has them."""
    G = AUTO_MIN
    out = _Out(cabi, B, FAN)
    one = _graph(cabi, 24, 16, 4096)
    unknown = _graph(cabi, 24, 16, 0)
    ws_free = _Ws(_bytes(cabi, None, G))
    ws_graph = _Ws(_bytes(cabi, one, G))
    staged = lambda g, ws, n=G: cabi.ns_homo_batched_staged(g, out, n, B, FAN, ws=ws, form=0)
    assert cabi.ns_homo_batched_form(one, out, G, B, FAN, ws=ws_free, form=0)[0] == 1   # the window-ordered form
    assert staged(one, ws_free) and staged(one, ws_graph)
    assert not staged(unknown, ws_free)                   # a view without max_degree: two-chunk slots, push pipeline
    assert not staged(one, _Ws(_bytes(cabi, unknown, G))) # a workspace sized without the stage slots
    assert not staged(one, ws_free, G - 1)                # below the AUTO threshold
