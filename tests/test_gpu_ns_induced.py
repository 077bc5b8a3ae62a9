"""tg_ns_induced_count / tg_ns_induced_emit on the device: the per-batch induced subgraph word for word against the NumPy
statement of the rule (helpers_induced.induced_rule), with the flat outputs pre-filled with a sentinel and the batches'
ranges set apart so that every word outside them is seen to be untouched; transforms.induced_subgraph on device tensors;
and NeighborLoader(unique=True, induced=True)."""
import numpy as np
import pytest
import torch

from helpers import load_fake_dataset, load_karate
from helpers_induced import edges_before, induced_rule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7                                               # no id, no position, no offset, no count
CHUNK = 512                                             # include/tchgeo.h: the chunk bound is pitch + ceil(n_edges / 512)


class DeviceGraph:
    """A CSC on the device (tg_coo_to_csx, or arrays given) with its host copy."""

    def __init__(self, ptrs, idx, perm=None, shadows=False):
        from tch_geometric import _cabi
        self.ptrs, self.idx, self.perm = ptrs, idx, perm
        self.view = _cabi.graph_view(ptrs, idx, indices32=idx.to(torch.int32) if shadows else None,
                                     ptrs32=ptrs.to(torch.int32) if shadows else None)
        self.n, self.n_edges = ptrs.numel() - 1, idx.numel()
        self.hp, self.hi = ptrs.cpu().numpy(), idx.cpu().numpy()

    @classmethod
    def from_coo(cls, ei, n, shadows=False):
        from tch_geometric import _cabi
        t = torch.as_tensor(ei).to(DEV)
        return cls(*_cabi.coo_to_csx(t[0].contiguous(), t[1].contiguous(), n, n, True), shadows=shadows)

    def with_shadows(self):
        return DeviceGraph(self.ptrs, self.idx, self.perm, shadows=True)


def run(g, lists, pitch=None, stride=2, marks=None, id_bound=None):
    """One count + emit launch over `lists` (one id list per batch) -> (triples per batch [3, m_b], marks per batch or
    None, status).  Nodes past n, counts words between the strides, n_edges and edge_marks start as the sentinel; the flat
    outputs are sentinel-filled with 3 spare words before, 2 between and 5 after the batches' ranges."""
    from tch_geometric import _cabi
    nb = len(lists)
    pitch = pitch or max(max((len(s) for s in lists), default=1), 1)
    nodes = np.full((nb, pitch), SENT, dtype=np.int64)
    counts = np.full(nb * stride, SENT, dtype=np.int64)
    for b, s in enumerate(lists):
        nodes[b, :len(s)] = s
        counts[b * stride] = len(s)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV)
    mk = dev(marks) if marks is not None else None
    launch = _cabi.NsInduced(g.view, dev(nodes), dev(counts), stride, nb, g.n if id_bound is None else id_bound, node_marks=mk)
    launch.state[:-1].fill_(SENT)
    launch.count()
    state = launch.state.cpu().numpy()
    status = int(state[-1])
    m = state[:nb]
    assert (m >= 0).all(), m
    off = 3 + np.concatenate([[0], np.cumsum(m + 2)[:-1]]) if nb else np.zeros(0, dtype=np.int64)
    total = int(3 + (m + 2).sum() + 5)
    flat = torch.full((3, total), SENT, dtype=torch.int64, device=DEV)
    launch.emit(dev(off), flat[0], flat[1], flat[2])
    torch.cuda.synchronize()
    flat = flat.cpu().numpy()
    written = np.zeros(total, dtype=bool)
    out = []
    for b in range(nb):
        written[off[b]:off[b] + m[b]] = True
        out.append(flat[:, off[b]:off[b] + m[b]])
    assert (flat[:, ~written] == SENT).all()              # before, between and after the ranges
    got_marks = launch.edge_marks.cpu().numpy() if marks is not None else None
    return out, got_marks, status


def check(g, lists, out, hp=None):
    hp = g.hp if hp is None else hp
    for b, s in enumerate(lists):
        want = np.stack(induced_rule(s, hp, g.hi))
        assert out[b].shape == want.shape, (b, out[b].shape, want.shape)
        assert np.array_equal(out[b], want), b


@pytest.fixture(scope="module")
def karate():
    return DeviceGraph.from_coo(*load_karate())


@pytest.fixture(scope="module")
def star():
    """vertex 0: in-degree 5 000 from the 1 200 sources 1..1200 (parallel edges; 9 chunks and a ragged tenth); 1201..1300
    are no neighbours of it; 400 more edges among 1..1300"""
    rs = np.random.default_rng(5)
    src = np.concatenate([np.arange(1, 1201), rs.integers(1, 1201, 3800)])
    extra = rs.integers(1, 1301, (2, 400))
    ei = np.concatenate([np.stack([src, np.zeros(5000, dtype=np.int64)]), extra], axis=1).astype(np.int64)
    g = DeviceGraph.from_coo(ei, 1301)
    assert g.hp[1] == 5000 and np.unique(g.hi[:5000]).size == 1200
    return g


def test_karate_ragged_batches_strides_and_marks(karate):
    g, rs = karate, np.random.default_rng(1)
    lists = [np.arange(34), np.zeros(0, dtype=np.int64), np.array([33])]
    lists += [rs.permutation(34)[:n] for n in (1, 5, 33, 34)]
    marks = np.array([[0, len(s) // 2, len(s), len(s) + 5] for s in lists])
    out2, marks2, st2 = run(g, lists, stride=2, marks=marks)
    out3, marks3, st3 = run(g, lists, stride=3, marks=marks, pitch=40)
    assert st2 == 0 and st3 == 0
    check(g, lists, out2)
    assert np.array_equal(out2[0][2], np.arange(g.n_edges))                   # the full set: every edge, in CSC order
    assert out2[1].shape == (3, 0)
    for b, s in enumerate(lists):
        assert np.array_equal(out2[b], out3[b])
        want = edges_before(out2[b][1], marks[b], len(s))
        assert marks2[b].tolist() == want and marks3[b].tolist() == want, (b, marks2[b], want)
    out, got_marks, st = run(g, lists)                                        # no marks asked for
    assert st == 0 and got_marks is None
    check(g, lists, out)


def test_star_hub_with_parallel_edges_across_chunk_borders(star):
    rs = np.random.default_rng(6)
    batch = np.concatenate([[0], rs.permutation(np.arange(1, 1201))[:100], np.arange(1201, 1251)])
    batch = rs.permutation(batch)
    out, _, st = run(star, [batch])
    assert st == 0
    check(star, [batch], out)
    hub = out[0][:, out[0][1] == int(np.nonzero(batch == 0)[0][0])]
    assert hub.shape[1] > 300 and (np.diff(hub[2]) > 0).all() and hub[2].max() > 9 * CHUNK   # hits in the ragged last chunk
    assert np.unique(hub[0]).size < hub.shape[1]                              # parallel offsets: rows repeat


def test_long_hub_column_built_on_the_device():
    """one column of 1 000 003 entries: 1 954 chunks, past one tile of the chunk prefix"""
    n, deg = 200000, 1000003
    gen = torch.Generator(device=DEV)
    gen.manual_seed(7)
    idx = torch.sort(torch.randint(1, n, (deg,), device=DEV, generator=gen)).values
    ptrs = torch.full((n + 1,), deg, dtype=torch.int64, device=DEV)
    ptrs[0] = 0
    g = DeviceGraph(ptrs, idx)
    rs = np.random.default_rng(8)
    batch = np.concatenate([[0], rs.choice(np.unique(g.hi), 1000, replace=False)])
    batch = rs.permutation(batch)
    out, marks, st = run(g, [batch, batch[:7]], marks=np.array([[500, 1001], [0, 7]]))
    assert st == 0
    check(g, [batch, batch[:7]], out)
    assert out[0].shape[1] >= 1000 and out[0][2].max() > 1024 * CHUNK
    for b, s in enumerate([batch, batch[:7]]):
        assert marks[b].tolist() == edges_before(out[b][1], [[500, 1001], [0, 7]][b], len(s))


@pytest.fixture(scope="module")
def rmat12():
    from tch_geometric import _cabi
    row, col = _cabi.rmat_edges(12, 65536, 0x5EED000C, DEV)
    g = DeviceGraph.from_coo(torch.stack([row, col]), 4096)
    assert g.n_edges == 65536 and (g.hi == np.repeat(np.arange(4096), np.diff(g.hp))).any()   # self loops are there
    return g


def test_rmat12_eight_ragged_batches_shadows_and_wide_keys(rmat12):
    g, rs = rmat12, np.random.default_rng(12)
    lists = [rs.permutation(4096)[:n] for n in (0, 1, 63, 64, 65, 1000, 2049)] + [np.arange(4096)]
    marks = np.array([[0, len(s) // 3, len(s)] for s in lists])
    out, got_marks, st = run(g, lists, pitch=4096, marks=marks)
    assert st == 0
    check(g, lists, out)
    assert np.array_equal(out[7][2], np.arange(65536))                        # all vertices: all offsets, in order
    for b, s in enumerate(lists):
        assert got_marks[b].tolist() == edges_before(out[b][1], marks[b], len(s))
    for variant, kw in ((g.with_shadows(), {}), (g, dict(id_bound=1 << 40)), (g.with_shadows(), dict(id_bound=1 << 40))):
        o, mk, st = run(variant, lists, pitch=4096, marks=marks, **kw)
        assert st == 0 and np.array_equal(mk, got_marks)
        for b in range(len(lists)):
            assert np.array_equal(o[b], out[b]), b


def test_repeats_chunk_bound_and_range(star):
    from tch_geometric import _cabi
    g, rs = star, np.random.default_rng(9)
    some = rs.permutation(np.arange(1, 1301))[:40]
    # a repeated id: local is the first position, both positions scan
    rep = np.concatenate([some[:10], [0], some[10:20], [0, some[3]], some[20:]])
    out, _, st = run(g, [rep])
    assert st == 0
    check(g, [rep], out)
    p0, p1 = np.nonzero(rep == 0)[0]
    assert (out[0][1] == p0).sum() == (out[0][1] == p1).sum() > 0 and p1 not in out[0][0]
    # only repeats of the hub: the chunk bound of the workspace is pitch + ceil(n_edges / chunk)
    pitch = 64
    bound = pitch + -(-g.n_edges // CHUNK)
    least = _cabi.ns_induced_workspace_bytes(g.view, pitch, g.n, 1)[1]
    assert least >= 8 * (bound + 1)
    hub_chunks = -(-5000 // CHUNK)
    fits, trips = bound // hub_chunks, bound // hub_chunks + 1
    assert trips <= pitch
    lists = [some, np.zeros(trips, dtype=np.int64), np.zeros(fits, dtype=np.int64), some[::-1]]
    out, marks, st = run(g, lists, pitch=pitch, marks=np.array([[1, 64]] * 4))
    assert st == 1                                                            # bit 0
    assert out[1].shape == (3, 0) and marks[1].tolist() == [0, 0]             # m_b = 0, nothing written
    check(g, [lists[0], lists[2], lists[3]], [out[0], out[2], out[3]])        # the neighbours are exact
    assert out[2].shape[1] == 0                                               # (the hub has no self loop)
    # an id equal to n_major: a column of length 0 that is nobody's row
    lists = [np.concatenate([some[:5], [g.n], [0], some[5:]]), some]
    out, _, st = run(g, lists)
    assert st == 2                                                            # bit 1
    check(g, lists, out, hp=np.concatenate([g.hp, g.hp[-1:]]))
    assert out[0].shape[1] > 0 and 5 not in out[0][0] and 5 not in out[0][1]


def test_behind_the_sampler_and_the_superset_property():
    """tg_ns_homo_batched -> tg_ns_homo_unique -> count -> emit on the fakedataset graph, 64 batches of 16 seeds, [4, 3]"""
    from tch_geometric import _cabi
    g = DeviceGraph.from_coo(*load_fake_dataset())
    nb, H = 64, 2
    seeds = _cabi.seed_batches(21, 0, nb, 16, g.n, DEV)
    slabs = _cabi.NsBatchedOut(nb, 16, [4, 3], DEV)
    _cabi.ns_homo_batched(g.view, seeds, [4, 3], 21, 0, slabs)
    u = _cabi.ns_homo_unique(slabs, nb, g.n)
    launch = _cabi.ns_induced_count(g.view, u.nodes, u.counts, 2, nb, g.n, node_marks=u.layer_nodes)
    rc, eidx, off = _cabi.ns_induced_emit(launch)
    torch.cuda.synchronize()
    assert int(launch.status.cpu()[0]) == 0
    rc, eidx = rc.cpu().numpy(), eidx.cpu().numpy()
    counts, nodes, ln = u.counts.cpu().numpy(), u.nodes.cpu().numpy(), u.layer_nodes.cpu().numpy()
    f_rows, f_cols, f_e = u.rows.cpu().numpy(), u.cols.cpu().numpy(), slabs.edge_index.cpu().numpy()
    marks = launch.edge_marks.cpu().numpy()
    for b in range(nb):
        n, m = counts[b]
        s = nodes[b, :n]
        rows, cols, e = induced_rule(s, g.hp, g.hi)
        got = np.stack([rc[0, off[b]:off[b + 1]], rc[1, off[b]:off[b + 1]], eidx[off[b]:off[b + 1]]])
        assert np.array_equal(got, np.stack([rows, cols, e])), b
        assert marks[b].tolist() == edges_before(cols, ln[b, :H], n)
        induced = set(zip(s[rows].tolist(), s[cols].tolist(), e.tolist()))
        forest = set(zip(s[f_rows[b, :m]].tolist(), s[f_cols[b, :m]].tolist(), f_e[b, :m].tolist()))
        assert m > 0 and forest <= induced, b


def test_transform_on_device_tensors(rmat12):
    from tch_geometric.transforms import induced_subgraph
    g, rs = rmat12, np.random.default_rng(13)
    for nodes in (rs.permutation(4096)[:700], np.array([17]), np.zeros(0, dtype=np.int64)):
        want = induced_rule(nodes, g.hp, g.hi)
        for id_bound in (None, 4096, 1 << 40):
            got = induced_subgraph(torch.from_numpy(nodes).to(DEV), g.ptrs, g.idx, id_bound=id_bound)
            for a, w in zip(got, want):
                assert a.dtype == torch.int64 and a.is_cuda and np.array_equal(a.cpu().numpy(), w)
    with pytest.raises(IndexError):
        induced_subgraph(torch.tensor([0, 4096], device=DEV), g.ptrs, g.idx)


def test_loader_induced_against_the_unique_loader():
    """Two loaders with the same seed over the fakedataset graph with x and an edge attribute, prefetch 4, a ragged last
    mini-batch, two epochs: induced=True hands out unique=True's nodes with the rule's edges."""
    from tch_geometric.loader import NeighborLoader
    from tch_geometric.transforms import Graph
    ei, n = load_fake_dataset()
    rs = np.random.default_rng(2)
    x = rs.standard_normal((n, 12)).astype(np.float32)
    ea = rs.standard_normal((ei.shape[1], 2)).astype(np.float32)
    g = Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=n, x=torch.from_numpy(x).to(DEV),
              edge_attr=torch.from_numpy(ea).to(DEV))
    nodes = torch.from_numpy(rs.integers(0, n, 1000))                 # 1 000 inputs with repeats: 7 x 128 + 104
    kw = dict(input_nodes=nodes, batch_size=128, prefetch=4, seed=9, call_id0=100)
    with pytest.raises(ValueError):
        NeighborLoader(g, [6, 5], induced=True, **kw)
    unique, induced = NeighborLoader(g, [6, 5], unique=True, **kw), NeighborLoader(g, [6, 5], unique=True, induced=True, **kw)
    assert len(induced) == 8 and induced.induced and not unique.induced
    hp, hi = induced.col_ptrs.cpu().numpy(), induced.row_indices.cpu().numpy()
    for epoch in range(2):
        seen = 0
        for j, (u, i) in enumerate(zip(unique, induced)):
            n_id = i.n_id.cpu().numpy()
            assert torch.equal(i.n_id, u.n_id) and torch.equal(i.x, u.x) and np.array_equal(i.x.cpu().numpy(), x[n_id])
            assert i.batch_size == u.batch_size and i.layer_nodes == u.layer_nodes and i.num_nodes == u.num_nodes
            assert i.call_id == u.call_id == 100 + epoch * 8 + j
            rows, cols, _ = induced_rule(n_id, hp, hi)
            assert np.array_equal(i.edge_index.cpu().numpy(), np.stack([rows, cols])) and i.num_edges == rows.size
            e_id = i.e_id.cpu().numpy()
            assert np.array_equal(ei[0][e_id], n_id[rows]) and np.array_equal(ei[1][e_id], n_id[cols])
            assert np.array_equal(i.edge_attr.cpu().numpy(), ea[e_id])
            assert i.layer_edges == edges_before(cols, i.layer_nodes, n_id.size) and u.layer_edges is None
            assert i.layer_offsets is None and u.layer_offsets is not None
            assert i.num_edges >= np.unique(u.e_id.cpu().numpy()).size
            seen += 1
        assert seen == 8
    assert len(induced._pool) == 1 and "ind" in induced._pool[0][0]   # the second epoch reused the slabs and the workspace
    ws = induced._pool[0][0]["ind"].ws
    assert ws.numel() > 0 and "ind" not in unique._pool[0][0]
