"""tg_saint_rw_nodes, tg_saint_coverage_add and tg_saint_norm on the device.  The yardstick of the node lists is
_cabi.random_walk on the same (seed, call id + g) plus the NumPy restatement (helpers_saint.node_list); every comparison
is exact equality, and output slabs are pre-filled with a sentinel that must survive past n_unique.  The norms are compared
with the float32 restatement for exact equality (IEEE division, no contraction)."""
import numpy as np
import pytest
import torch

from helpers_saint import coverage_counts, node_list, norms, random_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7
SEED = 0x5A1


def dev(a, dtype=np.int64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def csr_view(edge_index, n, shadows):
    """the device ingest's CSR of a COO list as a graph view, with or without the u32 shadows"""
    from tch_geometric import _cabi
    ei = dev(edge_index)
    ptrs, idx, _ = _cabi.coo_to_csx(ei[0], ei[1], n, n, False)
    kw = dict(indices32=idx.to(torch.int32), ptrs32=ptrs.to(torch.int32)) if shadows else {}
    return _cabi.graph_view(ptrs, idx, **kw)


def expected(graph, roots, T, call_id, skip=None):
    """per mini-batch: tg_random_walk under call id + g, restated; skip[g]: walkers whose roots lie outside the graph (they
    walk from vertex 0 here, which changes no other walker's draws, and are dropped)"""
    from tch_geometric import _cabi
    lists = []
    for g in range(roots.shape[0]):
        start = roots[g].clone()
        drop = [] if skip is None else skip[g]
        if drop:
            start[torch.tensor(drop, device=DEV)] = 0
        walks = _cabi.random_walk(graph, start, T, 1.0, 1.0, SEED, call_id + g)
        lists.append(node_list(walks.cpu().numpy(), skip=drop))
    return lists


def run(graph, roots, T, call_id, form, pitch=None, ws=None):
    from tch_geometric import _cabi
    G, B = roots.shape
    pitch = B * (T + 1) if pitch is None else pitch
    nodes = torch.full((G, pitch), SENT, dtype=torch.int64, device=DEV)
    counts = torch.full((G,), SENT, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    _cabi.saint_rw_nodes(graph, roots, T, SEED, call_id, form=form, ws=ws, out=(nodes, counts), status=status)
    torch.cuda.synchronize()
    return nodes.cpu().numpy(), counts.cpu().numpy(), int(status.item())


def check(got, want):
    nodes, counts, _ = got
    assert counts.tolist() == [len(w) for w in want]
    for g, w in enumerate(want):
        assert np.array_equal(nodes[g, :len(w)], w), "mini-batch %d" % g
        assert (nodes[g, len(w):] == SENT).all(), "mini-batch %d: words past n_unique were written" % g


N_RANDOM = 300


@pytest.fixture(scope="module")
def random_views():
    ei = random_graph(N_RANDOM, 2000, 0.1, seed=1)
    return {s: csr_view(ei, N_RANDOM, s) for s in (False, True)}


@pytest.fixture(scope="module")
def random_expected(random_views):
    """the yardstick per (B, T), computed once on the plain view"""
    cache = {}

    def get(B, T):
        if (B, T) not in cache:
            rs = np.random.default_rng(B * 10 + T)
            roots = rs.integers(0, N_RANDOM, (5, B)).astype(np.int64)
            roots[:, B // 2:] = roots[:, :B - B // 2]                   # roots with repeats
            roots = dev(roots)
            cache[B, T] = (roots, expected(random_views[False], roots, T, 11))
        return cache[B, T]
    return get


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 200])
def test_random_graph_every_form_and_view(random_views, random_expected, B, T):
    roots, want = random_expected(B, T)
    results = []
    for shadows in (False, True):
        for form in (1, 2, 0):
            got = run(random_views[shadows], roots, T, 11, form, pitch=B * (T + 1) + 5)
            assert got[2] == 0
            check(got, want)
            results.append(got[0])
    assert all(np.array_equal(results[0], r) for r in results[1:])      # the forms write identical words


def test_dead_ends_are_met(random_views, random_expected):
    """the fixture's walks do stop: some walk matrix has -1 padding, so the stop path ran in the tests above"""
    from tch_geometric import _cabi
    roots, _ = random_expected(200, 3)
    walks = _cabi.random_walk(random_views[False], roots[0], 3, 1.0, 1.0, SEED, 11).cpu().numpy()
    assert (walks[:, 1:] < 0).any() and (walks[:, -1] >= 0).any()


def test_star_graph_heaviest_contention():
    """8 leaves around a hub, edges both ways: 6 144 positions on 9 vertices"""
    leaves = np.arange(1, 9)
    ei = np.stack([np.concatenate([np.zeros(8, dtype=np.int64), leaves]), np.concatenate([leaves, np.zeros(8, dtype=np.int64)])])
    graph = csr_view(ei, 9, False)
    roots = dev(np.random.default_rng(3).integers(0, 9, (2, 1024)))
    want = expected(graph, roots, 5, 0)
    assert all(len(w) == 9 for w in want)
    for form in (1, 2):
        check(run(graph, roots, 5, 0, form), want)


@pytest.fixture(scope="module")
def ring():
    n = 20000
    src = np.arange(n, dtype=np.int64)
    return csr_view(np.stack([src, (src + 1) % n]), n, True)


def test_ring_largest_lds_table(ring):
    """B = 3 072, T = 3: roots 4k, so all 12 288 positions are distinct vertices -- the fullest table the LDS form takes"""
    from tch_geometric import _cabi
    B, T = 3072, 3
    assert _cabi.saint_rw_form(B, T) == _cabi.saint_rw_form(B, T, 160 * 1024) and _cabi.saint_rw_form(B, T)[0] == 1
    roots = dev((np.arange(2 * B, dtype=np.int64) * (T + 1) % 20000).reshape(2, B))
    roots[1] = roots[0].flip(0)
    want = expected(ring, roots, T, 5)
    assert all(len(w) == B * (T + 1) for w in want)
    got1 = run(ring, roots, T, 5, 1)
    check(got1, want)
    assert np.array_equal(got1[0], run(ring, roots, T, 5, 0)[0])        # auto is the LDS form here
    check(run(ring, roots, T, 5, 2), want)


def test_ring_one_root_more_takes_the_flat_form(ring):
    from tch_geometric import _cabi
    B, T = 3073, 3
    assert _cabi.saint_rw_form(B, T)[0] == 2 and _cabi.saint_rw_form(B, T, 160 * 1024)[0] == 2
    assert _cabi.saint_rw_workspace_bytes(1, B, T)[0] == _cabi.saint_rw_workspace_bytes(1, B, T, form=2)[0] > 0
    roots = dev((np.arange(B, dtype=np.int64) * (T + 1)).reshape(1, B))
    want = expected(ring, roots, T, 6)
    assert len(want[0]) == B * (T + 1)
    check(run(ring, roots, T, 6, 0), want)
    with pytest.raises(_cabi.TchGeoError, match="does not fit"):
        run(ring, roots, T, 6, 1)


def test_all_roots_are_sinks(random_views):
    graph = random_views[False]
    ptrs = graph._keep[0].cpu().numpy()
    sinks = np.nonzero(np.diff(ptrs) == 0)[0]
    assert sinks.size >= 10
    roots = dev(np.random.default_rng(5).choice(sinks, (3, 70)))
    want = [np.array(list(dict.fromkeys(r.tolist())), dtype=np.int64) for r in roots.cpu().numpy()]
    for form in (1, 2):
        check(run(graph, roots, 3, 0, form), want)


def test_flat_form_in_rounds(random_views, random_expected):
    """a workspace of one mini-batch runs G = 3 in three rounds, with the one-round result"""
    from tch_geometric import _cabi
    roots, want = random_expected(200, 3)
    roots, want = roots[:3].contiguous(), want[:3]
    nbytes, bmin = _cabi.saint_rw_workspace_bytes(3, 200, 3, form=2)
    assert nbytes == 3 * bmin and bmin % 8 == 0
    one = run(random_views[True], roots, 3, 11, 2, ws=torch.empty(nbytes // 8, dtype=torch.int64, device=DEV))
    rounds = run(random_views[True], roots, 3, 11, 2, ws=torch.empty(bmin // 8, dtype=torch.int64, device=DEV))
    check(one, want)
    assert np.array_equal(one[0], rounds[0]) and np.array_equal(one[1], rounds[1])
    with pytest.raises(_cabi.TchGeoError, match="workspace too small"):
        run(random_views[True], roots, 3, 11, 2, ws=torch.empty(bmin // 8 - 1, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("form", [1, 2])
def test_roots_outside_the_graph(random_views, random_expected, form):
    roots, _ = random_expected(65, 3)
    roots = roots.clone()
    roots[1, 7], roots[3, 0] = -1, N_RANDOM
    skip = [[], [7], [], [0], []]
    want = expected(random_views[False], roots, 3, 11, skip=skip)
    got = run(random_views[False], roots, 3, 11, form)
    assert got[2] == 2                                                  # status bit 1
    check(got, want)


def test_coverage_accumulates_and_skips():
    from tch_geometric import _cabi
    N, E = 50, 80
    rs = np.random.default_rng(9)
    nodes = rs.integers(0, N, (4, 12)).astype(np.int64)
    counts = np.array([12, 0, 5, 9], dtype=np.int64)
    ids = [rs.integers(0, E, 200).astype(np.int64), rs.integers(0, E, 33).astype(np.int64)]
    node_count = torch.zeros(N, dtype=torch.int64, device=DEV)
    edge_count = torch.zeros(E, dtype=torch.int64, device=DEV)
    lists = [nodes[g, :counts[g]] for g in range(4)]
    st = _cabi.saint_coverage_add(dev(nodes), dev(counts), node_count, edge_count, edge_ids=dev(ids[0]))
    _cabi.saint_coverage_add(dev(nodes), dev(counts), node_count, edge_count, edge_ids=dev(ids[1]), status=st)   # accumulates
    want = coverage_counts(lists + lists, ids, N, E)
    assert int(st.item()) == 0
    assert np.array_equal(node_count.cpu().numpy(), want[0]) and np.array_equal(edge_count.cpu().numpy(), want[1])
    # strided counts (the pair layout of tg_ns_unique_out.counts), fewer batches, no edges; ids outside the tables
    pairs = dev(np.stack([counts, np.full(4, SENT)], axis=1))
    _cabi.saint_coverage_add(dev(nodes), pairs[:, 0], node_count, edge_count, n_batches=3)
    want = coverage_counts(lists + lists + lists[:3], ids, N, E)
    assert np.array_equal(node_count.cpu().numpy(), want[0]) and np.array_equal(edge_count.cpu().numpy(), want[1])
    bad_nodes, bad_ids = nodes.copy(), ids[1].copy()
    bad_nodes[0, 3], bad_nodes[2, 1], bad_ids[5], bad_ids[6] = N, -1, E, -3
    for kw in (dict(nodes=bad_nodes, ids=ids[1]), dict(nodes=nodes, ids=bad_ids)):
        nc, ec = torch.zeros(N, dtype=torch.int64, device=DEV), torch.zeros(E, dtype=torch.int64, device=DEV)
        st = _cabi.saint_coverage_add(dev(kw["nodes"]), dev(counts), nc, ec, edge_ids=dev(kw["ids"]))
        want = coverage_counts([kw["nodes"][g, :counts[g]] for g in range(4)], [kw["ids"]], N, E)
        assert int(st.item()) == 2
        assert np.array_equal(nc.cpu().numpy(), want[0]) and np.array_equal(ec.cpu().numpy(), want[1])


@pytest.mark.parametrize("shadows", [False, True])
def test_norm_every_branch(shadows):
    """count 0, 0/0, x/0, a ratio above 1e4, an empty column, a column longer than one chunk of 1 024 offsets (and one that
    straddles a chunk border)"""
    from tch_geometric import _cabi
    rs = np.random.default_rng(4)
    deg = np.array([3, 0, 2500, 1, 0, 0, 700, 5, 1, 0], dtype=np.int64)
    N, E = deg.size, int(deg.sum())
    ptrs = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    nc = np.array([0, 4, 30011, 7, 0, 2, 123456789, 1, 0, 9], dtype=np.int64)
    ec = rs.integers(0, 4, E).astype(np.int64)
    ec[:3] = (0, 1, 2)                                                  # column 0 has count 0: 0/0, 0/1, 0/2
    ec[3:6] = (0, 1, 2)                                                 # column 2: x/0, a ratio above 1e4
    ec[-1] = 0                                                          # column 8 has count 0: 0/0 at the last offset
    idx = rs.integers(0, N, E).astype(np.int64)
    tp, ti = dev(ptrs), dev(idx)
    kw = dict(indices32=ti.to(torch.int32), ptrs32=tp.to(torch.int32)) if shadows else {}
    graph = _cabi.graph_view(tp, ti, **kw)
    node_norm, edge_norm = _cabi.saint_norm(graph, dev(nc), dev(ec), 37)
    want_n, want_e = norms(ptrs, nc, ec, 37)
    got_n, got_e = node_norm.cpu().numpy(), edge_norm.cpu().numpy()
    f32 = np.float32
    assert want_e[0] == f32(0.1) and want_e[1] == 0 and want_e[3] == f32(1e4) and want_e[4] == f32(1e4) and want_e[-1] == f32(0.1)
    assert ((want_e > 0) & (want_e < f32(1e4)) & (want_e != f32(0.1))).any()
    assert got_n.dtype == np.float32 and got_e.dtype == np.float32
    assert np.array_equal(got_n.view(np.uint32), want_n.view(np.uint32))
    assert np.array_equal(got_e.view(np.uint32), want_e.view(np.uint32))
