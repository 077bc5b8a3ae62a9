"""tg_saint_node_nodes and tg_saint_edge_nodes on the device.  The yardstick is the NumPy restatement (helpers_saint_ne):
every comparison is exact equality of every output word, output slabs are pre-filled with a sentinel that must survive past
n_unique and around the slab, and the law tests hold 2^16 one-slot mini-batches per form against the exact laws
(exact_laws.chi2_gof; tests/test_saint_ne_cpu.py asserts their power against three named wrong laws)."""
import numpy as np
import pytest
import torch

import exact_laws as L
import helpers_saint_ne as H
from helpers_induced import csc_of
from helpers_saint import random_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7
SEED = 0x5A17
N = 302
HUB = 7
CALL = 1 << 33                                              # call ids past 32 bits


def dev(a, dtype=np.int64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def make_graph():
    """helpers_saint.random_graph (self loops, parallel edges, sinks) on vertices 0..299, plus: vertex 299 without in-edges,
    vertices 300 (isolated) and 301 (a sink with one in-edge), and HUB's column grown past 4 096 entries"""
    ei = random_graph(300, 2000, 0.1, seed=1)
    ei = ei[:, ei[1] != 299]
    rs = np.random.default_rng(2)
    hub = np.stack([rs.choice(np.unique(ei[0]), 5000), np.full(5000, HUB)])
    return np.concatenate([ei, hub, np.array([[5], [301]])], axis=1).astype(np.int64)


class Views:
    """the CSC and the CSR of a COO list on the host and as graph views, with and without the u32 shadows"""

    def __init__(self, edge_index, n):
        from tch_geometric import _cabi
        self.n = n
        self.csc = csc_of(edge_index, n)[:2]
        self.csr = csc_of(edge_index[::-1], n)[:2]
        self.cols, self.rows = H.nonempty(self.csc[0]), H.nonempty(self.csr[0])
        self.view = {}
        for name, (ptrs, idx) in (("csc", self.csc), ("csr", self.csr)):
            tp, ti = dev(ptrs), dev(idx)
            self.view[name, False] = _cabi.graph_view(tp, ti)
            self.view[name, True] = _cabi.graph_view(tp, ti, indices32=ti.to(torch.int32), ptrs32=tp.to(torch.int32))


@pytest.fixture(scope="module")
def views():
    ei = make_graph()
    v = Views(ei, N)
    deg_in, deg_out = np.diff(v.csc[0]), np.diff(v.csr[0])
    assert deg_in[HUB] > 4096 and deg_in[299] == 0 and deg_out[299] > 0 and deg_in[300] == deg_out[300] == 0
    assert (deg_out == 0).sum() >= 10 and (ei[0] == ei[1]).any()
    assert np.unique(ei, axis=1).shape[1] < ei.shape[1]
    return v


class Slab:
    """a node slab with `pad` guard rows before and after it, and the counts at `stride` with guard words between"""

    def __init__(self, G, pitch, stride=1, pad=1):
        self.G, self.pad = G, pad
        self.all_nodes = torch.full((G + 2 * pad, pitch), SENT, dtype=torch.int64, device=DEV)
        self.all_counts = torch.full((G * stride + 2 * pad,), SENT, dtype=torch.int64, device=DEV)
        self.nodes = self.all_nodes[pad:pad + G]
        self.counts = self.all_counts[pad:pad + G * stride][::stride]
        self.stride = stride
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)

    def read(self):
        torch.cuda.synchronize()
        nodes, counts = self.all_nodes.cpu().numpy(), self.all_counts.cpu().numpy()
        p, G, s = self.pad, self.G, self.stride
        assert (nodes[:p] == SENT).all() and (nodes[p + G:] == SENT).all(), "words around the node slab were written"
        assert (counts[:p] == SENT).all() and (counts[p + G * s:] == SENT).all(), "words around the counts were written"
        inner = counts[p:p + G * s].reshape(G, s)
        assert (inner[:, 1:] == SENT).all(), "guard words between the counts were written"
        return nodes[p:p + G], inner[:, 0], int(self.status.item())


def run_node(graph, B, G, call_id, form, id_bound=N, pitch=None, stride=1, ws=None):
    from tch_geometric import _cabi
    slab = Slab(G, B if pitch is None else pitch, stride)
    _cabi.saint_node_nodes(graph, B, G, SEED, call_id, id_bound=id_bound, form=form, ws=ws, out=(slab.nodes, slab.counts),
                           status=slab.status)
    return slab.read()


def run_edge(csc, cols, csr, rows, B, G, call_id, form, id_bound=N, pitch=None, stride=1, ws=None):
    from tch_geometric import _cabi
    slab = Slab(G, 2 * B if pitch is None else pitch, stride)
    _cabi.saint_edge_nodes(csc, dev(cols), csr, None if csr is None else dev(rows), B, G, SEED, call_id, id_bound=id_bound,
                           form=form, ws=ws, out=(slab.nodes, slab.counts), status=slab.status)
    return slab.read()


def check(got, want, status=0):
    nodes, counts, st = got
    lists, want_status = want
    assert want_status == status and st == status
    assert counts.tolist() == [len(w) for w in lists]
    for g, w in enumerate(lists):
        assert np.array_equal(nodes[g, :len(w)], w), "mini-batch %d" % g
        assert (nodes[g, len(w):] == SENT).all(), "mini-batch %d: words past n_unique were written" % g


def forms_of(P):
    """the forms a shape is run in: both where the LDS form fits, then auto"""
    return (1, 2, 0) if P <= 12288 else (2, 0)


# ---- the node sampler ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1024, 12288, 12289])
def test_node_every_form_view_and_shadow(views, B):
    from tch_geometric import _cabi
    assert _cabi.saint_ne_form(B)[0] == (1 if B <= 12288 else 2)        # 12 288: the last LDS size; 12 289: auto goes flat
    G = 3
    for name, host in (("csc", views.csc), ("csr", views.csr)):          # sources by out-degree, targets by in-degree
        want = H.node_lists(host[1], G, B, SEED, CALL, N)
        results = []
        for shadows in (False, True):
            for form in forms_of(B):
                got = run_node(views.view[name, shadows], B, G, CALL, form, pitch=B + 5)
                check(got, want)
                results.append(got[0])
        assert all(np.array_equal(results[0], r) for r in results[1:])  # the forms write identical words
    if B > 12288:
        with pytest.raises(_cabi.TchGeoError, match="does not fit"):
            run_node(views.view["csc", True], B, G, CALL, 1)


@pytest.mark.parametrize("G", [1, 300])
def test_node_many_mini_batches_strided_counts(views, G):
    want = H.node_lists(views.csc[1], G, 65, SEED, 17, N)
    for form in (1, 2):
        check(run_node(views.view["csc", True], 65, G, 17, form, pitch=70, stride=2), want)


def test_node_id_bound_below_a_drawn_id(views):
    want = H.node_lists(views.csc[1], 3, 200, SEED, 5, 120)
    assert want[1] == 2 and all(0 < len(w) and w.max() < 120 for w in want[0])
    for form in (1, 2):
        check(run_node(views.view["csc", False], 200, 3, 5, form, id_bound=120), want, status=2)


# ---- the edge sampler ------------------------------------------------------------------------------------------------------
def edge_want(v, G, B, call_id, cols=None, rows=None, csr=True, id_bound=N):
    cols = v.cols if cols is None else cols
    rows = (v.rows if rows is None else rows) if csr else np.zeros(0, dtype=np.int64)
    return H.edge_lists(v.csc, cols, v.csr if csr else None, rows, G, B, SEED, call_id, id_bound)


@pytest.mark.parametrize("B", [1, 64, 65, 6144, 6145])
def test_edge_every_form_and_shadow(views, B):
    from tch_geometric import _cabi
    assert _cabi.saint_ne_form(2 * B)[0] == (1 if B <= 6144 else 2)     # P = 12 288: the last LDS size
    G = 3
    want = edge_want(views, G, B, CALL)
    results = []
    for shadows in (False, True):
        for form in forms_of(2 * B):
            got = run_edge(views.view["csc", shadows], views.cols, views.view["csr", shadows], views.rows, B, G, CALL, form,
                           pitch=2 * B + 3)
            check(got, want)
            results.append(got[0])
    got = run_edge(views.view["csc", True], views.cols, views.view["csr", False], views.rows, B, G, CALL, 0)   # mixed widths
    check(got, want)
    assert np.array_equal(got[0][:, :2 * B], results[0][:, :2 * B])
    assert all(np.array_equal(results[0], r) for r in results[1:])
    if B > 6144:
        with pytest.raises(_cabi.TchGeoError, match="does not fit"):
            run_edge(views.view["csc", True], views.cols, views.view["csr", True], views.rows, B, G, CALL, 1)


@pytest.mark.parametrize("G", [1, 300])
def test_edge_many_mini_batches_strided_counts(views, G):
    want = edge_want(views, G, 65, 9)
    for form in (1, 2):
        check(run_edge(views.view["csc", True], views.cols, views.view["csr", True], views.rows, 65, G, 9, form, pitch=140,
                       stride=2), want)


def test_edge_one_sided_and_symmetric_use(views):
    """csr null with n_rows = 0: the column law; the same graph and list on both sides: what symmetric=True passes"""
    want = edge_want(views, 3, 200, 21, csr=False)
    for form in (1, 2):
        check(run_edge(views.view["csc", True], views.cols, None, None, 200, 3, 21, form), want)
    want = H.edge_lists(views.csc, views.cols, views.csc, views.cols, 3, 200, SEED, 22, N)
    for form in (1, 2):
        check(run_edge(views.view["csc", True], views.cols, views.view["csc", True], views.cols, 200, 3, 22, form), want)


@pytest.mark.parametrize("side", ["cols", "rows"])
@pytest.mark.parametrize("what, status", [("empty", 4), ("outside", 2)])
def test_edge_refused_majors(views, side, what, status):
    """one listed major without entries / outside its graph among good ones: its slots contribute nothing, the status says
    which, and every other slot is intact (the restatement drops exactly those slots)"""
    empty = {"cols": 299, "rows": 301}[side]                            # no in-edges / no out-edges
    bad = empty if what == "empty" else (N if side == "cols" else -1)
    lists = dict(cols=views.cols[:40].copy(), rows=views.rows[:40].copy())
    lists[side][5] = bad
    B = 400
    src, dst, refused, st = H.edge_draws(views.csc, lists["cols"], views.csr, lists["rows"], 2, B, SEED, 31, N)
    assert st == status and 0 < refused.sum() < refused.size and refused.any(axis=1).all()
    ok_src, ok_dst, ok_refused, _ = H.edge_draws(views.csc, views.cols[:40], views.csr, views.rows[:40], 2, B, SEED, 31, N)
    assert not ok_refused.any()
    assert np.array_equal(src[~refused], ok_src[~refused]) and np.array_equal(dst[~refused], ok_dst[~refused])   # neighbours intact
    want = (H.lists_of((src, dst), refused), st)
    for form in (1, 2):
        check(run_edge(views.view["csc", True], lists["cols"], views.view["csr", True], lists["rows"], B, 2, 31, form), want,
              status=status)


def test_edge_id_bound_below_a_drawn_id(views):
    want = edge_want(views, 3, 200, 41, id_bound=150)
    assert want[1] == 2 and all(0 < len(w) and w.max() < 150 for w in want[0])
    for form in (1, 2):
        check(run_edge(views.view["csc", False], views.cols, views.view["csr", False], views.rows, 200, 3, 41, form,
                       id_bound=150), want, status=2)


# ---- rounds, streams, nothing to do ------------------------------------------------------------------------------------------
def test_flat_form_in_rounds_on_exactly_bytes_min(views):
    """a workspace of one mini-batch runs G = 3 in three rounds, with the one-round result"""
    from tch_geometric import _cabi
    ws = lambda nbytes: torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    nbytes, bmin = _cabi.saint_ne_workspace_bytes(3, 200, form=2)
    assert nbytes == 3 * bmin and bmin % 8 == 0
    want = H.node_lists(views.csc[1], 3, 200, SEED, 51, N)
    check(run_node(views.view["csc", True], 200, 3, 51, 2, ws=ws(nbytes)), want)
    check(run_node(views.view["csc", True], 200, 3, 51, 2, ws=ws(bmin)), want)
    with pytest.raises(_cabi.TchGeoError, match="workspace too small"):
        run_node(views.view["csc", True], 200, 3, 51, 2, ws=ws(bmin - 8))
    nbytes, bmin = _cabi.saint_ne_workspace_bytes(3, 400, form=2)
    want = edge_want(views, 3, 200, 52)
    args = (views.view["csc", True], views.cols, views.view["csr", True], views.rows, 200, 3, 52, 2)
    check(run_edge(*args, ws=ws(nbytes)), want)
    check(run_edge(*args, ws=ws(bmin)), want)
    with pytest.raises(_cabi.TchGeoError, match="workspace too small"):
        run_edge(*args, ws=ws(bmin - 8))


def test_non_default_stream(views):
    stream = torch.cuda.Stream(device=DEV)
    want_n = H.node_lists(views.csc[1], 3, 65, SEED, 61, N)
    want_e = edge_want(views, 3, 65, 62)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for form in (1, 2):
            check(run_node(views.view["csc", True], 65, 3, 61, form), want_n)
            check(run_edge(views.view["csc", True], views.cols, views.view["csr", True], views.rows, 65, 3, 62, form), want_e)


def test_no_mini_batches(views):
    """G = 0 into a slab of two rows: nothing is written"""
    from tch_geometric import _cabi
    for form in (0, 1, 2):
        ws = torch.empty(1 << 16, dtype=torch.int64, device=DEV)
        slab = Slab(2, 130)
        _cabi.saint_node_nodes(views.view["csc", True], 65, 0, SEED, 0, id_bound=N, form=form, ws=ws,
                               out=(slab.nodes, slab.counts), status=slab.status)
        _cabi.saint_edge_nodes(views.view["csc", True], dev(views.cols), views.view["csr", True], dev(views.rows), 65, 0, SEED, 0,
                               id_bound=N, form=form, ws=ws, out=(slab.nodes, slab.counts), status=slab.status)
        nodes, counts, status = slab.read()
        assert (nodes == SENT).all() and (counts == SENT).all() and status == 0


# ---- the laws ------------------------------------------------------------------------------------------------------------------
N_LAW = 1 << 16


@pytest.fixture(scope="module")
def law():
    ei, n = H.law_graph()
    v = Views(ei, n)
    v.cat, v.pairs = H.pair_categories(*v.csc)
    v.pair_law = H.merged(H.edge_entry_law(v.csc[0], v.csc[1], v.cols, v.rows, n), v.cat, len(v.pairs))
    v.node_law = H.node_law(v.csc[1], n)
    return v


@pytest.mark.parametrize("form", [1, 2])
def test_node_law(law, form):
    """2^16 mini-batches of one slot in one launch: nodes[g, 0] follows out-degree / E -- and equals the restatement"""
    nodes, counts, status = run_node(law.view["csc", True], 1, N_LAW, 0, form, id_bound=law.n)
    assert status == 0 and (counts == 1).all()
    want, _, _ = H.node_draws(law.csc[1], N_LAW, 1, SEED, 0, law.n)
    assert np.array_equal(nodes[:, 0], want[:, 0])
    L.chi2_gof(np.bincount(nodes[:, 0], minlength=law.n), law.node_law, "tg_saint_node_nodes form %d" % form)


@pytest.mark.parametrize("form", [1, 2])
def test_edge_law(law, form):
    """(source, target) from nodes[g, :2], counts == 1 on a self loop, against the pair law (parallel entries merged)"""
    nodes, counts, status = run_edge(law.view["csc", True], law.cols, law.view["csr", True], law.rows, 1, N_LAW, 0, form,
                                     id_bound=law.n)
    assert status == 0 and ((counts == 1) | (counts == 2)).all() and (counts == 1).any()
    src, dst = nodes[:, 0], np.where(counts == 2, nodes[:, 1], nodes[:, 0])
    want_src, want_dst, _, _ = H.edge_draws(law.csc, law.cols, law.csr, law.rows, N_LAW, 1, SEED, 0, law.n)
    assert np.array_equal(src, want_src[:, 0]) and np.array_equal(dst, want_dst[:, 0])
    index = {(int(u), int(v)): i for i, (u, v) in enumerate(law.pairs)}
    cats = np.array([index[int(u), int(v)] for u, v in zip(src, dst)])  # a pair that is no edge of the graph: KeyError
    L.chi2_gof(np.bincount(cats, minlength=len(law.pairs)), law.pair_law, "tg_saint_edge_nodes form %d" % form)


@pytest.mark.parametrize("form", [1, 2])
def test_node_slots_are_independent(law, form):
    """B = 2 over 2^16 mini-batches against the product law; counts == 1 means both slots drew the same node"""
    nodes, counts, status = run_node(law.view["csc", True], 2, N_LAW, 1 << 20, form, id_bound=law.n)
    assert status == 0
    first, second = nodes[:, 0], np.where(counts == 2, nodes[:, 1], nodes[:, 0])
    joint = np.bincount(first * law.n + second, minlength=law.n * law.n)
    L.chi2_gof(joint, np.outer(law.node_law, law.node_law).ravel(), "two slots of tg_saint_node_nodes form %d" % form)
