"""tg_ns_induced_grouped_count / tg_ns_induced_grouped_emit on the device: the induced edges per subgraph of a disjoint list
word for word against the NumPy statement of the rule (helpers_shadow.grouped_induced_rule), with the flat outputs
pre-filled with a sentinel and the batches' ranges set apart so that every word outside them is seen to be untouched; the
chunk capacity protocol; the time filter at its borders; the pair behind the real samplers; and
transforms.induced_subgraph(group=...) on device tensors."""
import numpy as np
import pytest
import torch

from helpers import load_karate
from helpers_induced import edges_before, induced_rule
from helpers_shadow import CHUNK, chunks_of, grouped_induced_rule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7                                               # no id, no position, no offset, no count, no group


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV)


class DeviceGraph:
    """A CSC on the device (tg_coo_to_csx, or arrays given) with its host copy; ts: timestamps in CSC order or None."""

    def __init__(self, ptrs, idx, ts=None, shadows=False):
        from tch_geometric import _cabi
        self.ptrs, self.idx, self.ts = ptrs, idx, ts
        self.view = _cabi.graph_view(ptrs, idx, timestamps=ts, indices32=idx.to(torch.int32) if shadows else None,
                                     ptrs32=ptrs.to(torch.int32) if shadows else None)
        self.n, self.n_edges = ptrs.numel() - 1, idx.numel()
        self.hp, self.hi = ptrs.cpu().numpy(), idx.cpu().numpy()
        self.hts = ts.cpu().numpy() if ts is not None else None

    @classmethod
    def from_coo(cls, ei, n, ts=None):
        """ts: per COO edge; carried into CSC order"""
        from tch_geometric import _cabi
        t = torch.as_tensor(ei).to(DEV)
        ptrs, idx, perm = _cabi.coo_to_csx(t[0].contiguous(), t[1].contiguous(), n, n, True)
        return cls(ptrs, idx, dev(ts)[perm].contiguous() if ts is not None else None)

    def variant(self, shadows=False, ts="same"):
        return DeviceGraph(self.ptrs, self.idx, self.ts if isinstance(ts, str) else ts, shadows)


def run(g, lists, n_groups, pitch=None, stride=2, marks=None, id_bound=None, group_time=None, window=None, chunk_cap=None):
    """One count + emit launch over `lists` (per batch a (nodes, group) pair) -> (triples per batch [3, m_b], marks per
    batch or None, chunks per batch, status).  Nodes and group words past n, counts words between the strides, n_edges,
    edge_marks and chunks start as the sentinel; the flat outputs are sentinel-filled with 3 spare words before, 2 between
    and 5 after the batches' ranges."""
    from tch_geometric import _cabi
    nb = len(lists)
    pitch = pitch or max(max((len(s) for s, _ in lists), default=1), 1)
    nodes, group = np.full((nb, pitch), SENT, dtype=np.int64), np.full((nb, pitch), SENT, dtype=np.int64)
    counts = np.full(nb * stride, SENT, dtype=np.int64)
    for b, (s, gr) in enumerate(lists):
        nodes[b, :len(s)], group[b, :len(s)] = s, gr
        counts[b * stride] = len(s)
    launch = _cabi.NsInducedGrouped(g.view, dev(nodes), dev(group), dev(counts), stride, nb, g.n if id_bound is None else id_bound,
                                    n_groups, node_marks=dev(marks) if marks is not None else None,
                                    group_time=dev(group_time) if group_time is not None else None, time_window=window,
                                    chunk_cap=chunk_cap)
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
    return out, got_marks, np.asarray(launch.chunks_of(launch.state.cpu())), status


def check(g, lists, out, n_groups=None, group_time=None, window=None, hp=None, only=None):
    hp = g.hp if hp is None else hp
    for b, (s, gr) in enumerate(lists):
        if only is not None and b not in only:
            continue
        want = np.stack(grouped_induced_rule(s, gr, hp, g.hi, g.hts, None if group_time is None else group_time[b], window,
                                             n_groups=n_groups))
        assert out[b].shape == want.shape, (b, out[b].shape, want.shape)
        assert np.array_equal(out[b], want), b
        assert (np.asarray(gr)[out[b][0]] == np.asarray(gr)[out[b][1]]).all()      # both ends share a group


def disjoint_list(rs, members, shuffle=True):
    """members: per group an id array -> (nodes, group) of their concatenation, shuffled as a whole"""
    nodes = np.concatenate([np.asarray(m, dtype=np.int64) for m in members] + [np.zeros(0, dtype=np.int64)])
    group = np.concatenate([np.full(len(m), g, dtype=np.int64) for g, m in enumerate(members)] + [np.zeros(0, dtype=np.int64)])
    order = rs.permutation(nodes.size) if shuffle else np.arange(nodes.size)
    return nodes[order], group[order]


@pytest.fixture(scope="module")
def karate():
    return DeviceGraph.from_coo(*load_karate())


@pytest.fixture(scope="module")
def star():
    """vertex 0: in-degree 5 000 from the 1 200 sources 1..1200 (parallel edges; 9 chunks and a ragged tenth); 400 more
    edges among 1..1300"""
    rs = np.random.default_rng(5)
    src = np.concatenate([np.arange(1, 1201), rs.integers(1, 1201, 3800)])
    extra = rs.integers(1, 1301, (2, 400))
    ei = np.concatenate([np.stack([src, np.zeros(5000, dtype=np.int64)]), extra], axis=1).astype(np.int64)
    g = DeviceGraph.from_coo(ei, 1301)
    assert g.hp[1] == 5000
    return g


def test_karate_ragged_batches_groups_strides_and_marks(karate):
    from tch_geometric import _cabi
    g, rs = karate, np.random.default_rng(1)
    # two seeds per group: group g holds the neighbourhoods of two seeds, so members differ by group and nodes recur
    def group_of_two(a, b):
        return np.unique(np.concatenate([[a, b], g.hi[g.hp[a]:g.hp[a + 1]], g.hi[g.hp[b]:g.hp[b + 1]]]))
    members = [group_of_two(0, 33), group_of_two(1, 2), group_of_two(5, 16), group_of_two(33, 32)]
    big = disjoint_list(rs, members)
    assert any((big[0] == v).sum() > 1 for v in (0, 33, 2))                    # the same node under several groups
    lists = [big, (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)), disjoint_list(rs, [[33], [33, 32], [0]])]
    marks = np.array([[0, len(s) // 2, len(s), len(s) + 5] for s, _ in lists])
    out2, marks2, ch2, st2 = run(g, lists, 4, stride=2, marks=marks)
    out3, marks3, ch3, st3 = run(g, lists, 4, stride=3, marks=marks, pitch=len(big[0]) + 9)
    assert st2 == 0 and st3 == 0
    check(g, lists, out2, n_groups=4)
    assert out2[1].shape == (3, 0) and out2[0].shape[1] > 100
    per_group = [set(out2[0][2][big[1][out2[0][1]] == k].tolist()) for k in range(4)]
    assert per_group[0] != per_group[3] and per_group[0] & per_group[3]        # hits differ by group, and overlap
    for b, (s, _) in enumerate(lists):
        assert np.array_equal(out2[b], out3[b])
        want = edges_before(out2[b][1], marks[b], len(s))
        assert marks2[b].tolist() == want and marks3[b].tolist() == want, (b, marks2[b], want)
        assert ch2[b] == ch3[b] == chunks_of(s, g.hp)
    # one group, no times: tg_ns_induced_* word for word
    plain = [rs.permutation(34)[:n] for n in (34, 0, 7)]
    one = [(s, np.zeros_like(s)) for s in plain]
    pm = np.array([[1, len(s)] for s in plain])
    out, mk, _, st = run(g, one, 1, marks=pm)
    assert st == 0
    pitch = 34
    nodes = np.full((3, pitch), SENT, dtype=np.int64)
    for b, s in enumerate(plain):
        nodes[b, :len(s)] = s
    launch = _cabi.ns_induced_count(g.view, dev(nodes), dev([34, 0, 7]), 1, 3, g.n, node_marks=dev(pm))
    rc, eidx, off = _cabi.ns_induced_emit(launch)
    assert np.array_equal(launch.edge_marks.cpu().numpy(), mk)
    for b in range(3):
        want = np.concatenate([rc[:, off[b]:off[b + 1]].cpu().numpy(), eidx[None, off[b]:off[b + 1]].cpu().numpy()])
        assert np.array_equal(out[b], want) and np.array_equal(want, np.stack(induced_rule(plain[b], g.hp, g.hi)))


def test_star_hub_in_five_groups(star):
    g, rs = star, np.random.default_rng(6)
    members = [np.concatenate([[0], rs.permutation(np.arange(1, 1201))[:60 + 20 * k], np.arange(1201, 1211)]) for k in range(5)]
    lst = disjoint_list(rs, members)
    out, _, chunks, st = run(g, [lst], 5)
    assert st == 0 and chunks[0] == chunks_of(lst[0], g.hp) >= 50
    check(g, [lst], out, n_groups=5)
    hubs = np.nonzero(lst[0] == 0)[0]
    assert hubs.size == 5
    hits = [out[0][:, out[0][1] == p] for p in hubs]
    assert len({h.shape[1] for h in hits}) == 5                                 # every group sees its own members
    for h in hits:
        assert h.shape[1] > 100 and (np.diff(h[2]) > 0).all() and h[2].max() > 9 * CHUNK   # hits in the ragged last chunk
        assert np.unique(h[0]).size < h.shape[1]                                # parallel offsets: rows repeat


def test_long_hub_column_in_thirty_groups():
    """one column of 18 000 entries (36 chunks, more than a unit) under 30 groups of 40 members: 1 080 chunks and 1 230
    positions, two tiles of each prefix"""
    n, deg = 2000, 18000
    gen = torch.Generator(device=DEV)
    gen.manual_seed(7)
    idx = torch.sort(torch.randint(1, n, (deg,), device=DEV, generator=gen)).values
    ptrs = torch.full((n + 1,), deg, dtype=torch.int64, device=DEV)
    ptrs[0] = 0
    g = DeviceGraph(ptrs, idx)
    rs = np.random.default_rng(8)
    members = [np.concatenate([[0], rs.choice(np.arange(1, n), 40, replace=False)]) for _ in range(30)]
    lst = disjoint_list(rs, members)
    marks = np.array([[600, 1100], [0, 3]])
    lists = [lst, (lst[0][:7], lst[1][:7])]
    out, mk, chunks, st = run(g, lists, 30, marks=marks)
    assert st == 0 and chunks[0] == 30 * 36 > 1024 and len(lst[0]) > 1024
    check(g, lists, out, n_groups=30)
    assert out[0].shape[1] > 30 * 300 and out[0][2].max() > 16 * CHUNK
    for b, (s, _) in enumerate(lists):
        assert mk[b].tolist() == edges_before(out[b][1], marks[b], len(s))


@pytest.fixture(scope="module")
def rmat12():
    from tch_geometric import _cabi
    row, col = _cabi.rmat_edges(12, 65536, 0x5EED000C, DEV)
    rs = np.random.default_rng(3)
    return DeviceGraph.from_coo(torch.stack([row, col]), 4096, ts=rs.integers(0, 1000, 65536))


def rmat_lists(g, rs, n_groups=2):
    """per batch n_groups random subsets of different sizes, a node often in both"""
    sizes = (0, 1, 65, 700, 2049)
    return [disjoint_list(rs, [rs.permutation(g.n)[:max(n // (k + 1), min(n, 1))] for k in range(n_groups)]) for n in sizes]


def test_key_widths_and_shadows(rmat12):
    g, rs = rmat12, np.random.default_rng(12)
    lists = rmat_lists(g, rs)
    marks = np.array([[0, len(s) // 3, len(s)] for s, _ in lists])
    out, mk, chunks, st = run(g, lists, 2, marks=marks)
    assert st == 0
    check(g, lists, out, n_groups=2)
    variants = ((g.variant(shadows=True), {}), (g, dict(id_bound=1 << 31)), (g.variant(shadows=True), dict(id_bound=1 << 31)),
                (g, dict(id_bound=1 << 40)))                                     # 2 groups x 2^31: 64-bit keys
    for variant, kw in variants:
        o, m2, c2, st = run(variant, lists, 2, marks=marks, **kw)
        assert st == 0 and np.array_equal(m2, mk) and np.array_equal(c2, chunks)
        for b in range(len(lists)):
            assert np.array_equal(o[b], out[b]), b


def test_chunk_capacity_protocol(star):
    g, rs = star, np.random.default_rng(9)
    some = rs.permutation(np.arange(1, 1301))[:40]
    hubs = lambda k: disjoint_list(rs, [np.concatenate([[0], some[:5 + g_]]) for g_ in range(k)])
    lists = [hubs(2), hubs(6), disjoint_list(rs, [some, some[:9]]), hubs(3)]
    need = np.array([chunks_of(s, g.hp) for s, _ in lists])
    assert need[1] == need.max() and need[1] > need[3] > need[0] > need[2]
    cap = int(need[3])                                                           # below batch 1's need, exactly batch 3's
    marks = np.array([[1, 64]] * 4)
    out, mk, chunks, st = run(g, lists, 6, marks=marks, chunk_cap=cap)
    assert st == 1                                                               # bit 0
    assert np.array_equal(chunks, need)                                          # exact for every batch, the refused one too
    assert out[1].shape == (3, 0) and mk[1].tolist() == [0, 0]                   # m_b = 0, nothing written (run() checks the rest)
    check(g, lists, out, n_groups=6, only=(0, 2, 3))                             # the others are right
    out, mk, chunks, st = run(g, lists, 6, marks=marks, chunk_cap=int(chunks.max()))
    assert st == 0 and np.array_equal(chunks, need)
    check(g, lists, out, n_groups=6)
    assert out[1].shape[1] > 0
    # the default capacity is the ungrouped bound: a hub under many groups goes past it on a small graph
    many = disjoint_list(rs, [[0]] * 150)
    default = 150 + -(-g.n_edges // CHUNK)
    assert chunks_of(many[0], g.hp) == 1500 > default
    out, _, chunks, st = run(g, [many, lists[0]], 150)
    assert st == 1 and chunks.tolist() == [1500, need[0]] and out[0].shape == (3, 0)
    check(g, [many, lists[0]], out, n_groups=150, only=(1,))


def test_times_at_the_window_borders():
    """a column of parallel edges whose times step through the window's borders, group times that differ by group and by
    batch, a negative window"""
    # vertices 0..5; column 0: sources 1, 1, 1, 2, 2, 3 x 4 with times below; column 1: sources 0, 2
    src = np.array([1, 1, 1, 2, 2, 3, 3, 3, 3, 0, 2])
    dst = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1])
    ts = np.array([10, 14, 15, 20, 21, 4, 5, 30, -3, 12, 50])
    g = DeviceGraph.from_coo(np.stack([src, dst]), 6, ts=ts)
    nodes = np.array([0, 1, 2, 3, 0, 1, 2, 3, 0])
    group = np.array([0, 0, 0, 0, 1, 1, 1, 1, 2])
    lists = [(nodes, group), (nodes[::-1].copy(), group[::-1].copy())]
    window = (5, 10)
    group_time = np.array([[20, 25, 0], [14, 2, 40]])                             # T - t = 10, 6, 5 | 4, 11 ... at the borders
    d = group_time[0, 0] - ts[:3]
    assert set(d.tolist()) == {10, 6, 5} and group_time[0, 1] - 14 == 11 and group_time[0, 1] - 21 == 4
    for win in (window, (-30, -1), (0, 0), (-(1 << 62), 1 << 62)):
        out, _, _, st = run(g, lists, 3, group_time=group_time, window=win)
        assert st == 0
        check(g, lists, out, n_groups=3, group_time=group_time, window=win)
    out, _, _, _ = run(g, lists, 3, group_time=group_time, window=window)
    col0 = out[0][:, out[0][1] == 0]                                              # group 0, T = 20: times 10, 14, 15 pass, 20 / 21 do not
    assert g.hts[col0[2]].tolist() == [10, 14, 15]
    col4 = out[0][:, out[0][1] == 4]                                              # group 1, T = 25: 15 (10), 20 (5) pass; 14 (11), 21 (4) do not
    assert sorted(g.hts[col4[2]].tolist()) == [15, 20]
    neg, _, _, _ = run(g, lists, 3, group_time=group_time, window=(-30, -1))
    assert neg[0].shape[1] > 0 and (group_time[0][group[neg[0][1]]] - g.hts[neg[0][2]] < 0).all()
    # no group_time: the graph's timestamps are ignored
    untimed, _, _, st = run(g, lists, 3)
    assert st == 0
    check(g.variant(ts=None), lists, untimed, n_groups=3)
    assert untimed[0].shape[1] > out[0].shape[1]


def test_random_times_on_rmat12(rmat12):
    g, rs = rmat12, np.random.default_rng(14)
    lists = rmat_lists(g, rs, n_groups=3)
    group_time = rs.integers(0, 1000, (len(lists), 3))
    for window in ((0, 1 << 62), (100, 300), (-50, 50)):
        for variant in (g, g.variant(shadows=True)):
            out, _, _, st = run(variant, lists, 3, group_time=group_time, window=window)
            assert st == 0
            check(g, lists, out, n_groups=3, group_time=group_time, window=window)


def test_refusals_launch_nothing(karate):
    from tch_geometric import _cabi
    g = karate
    nodes, group, counts = dev(np.arange(34)[None]), dev(np.zeros((1, 34))), dev([34, 0])
    with pytest.raises(_cabi.TchGeoError, match="timestamps"):                    # times without graph timestamps
        _cabi.NsInducedGrouped(g.view, nodes, group, counts, 2, 1, g.n, 1, group_time=dev([[5]]), time_window=(0, 9)).count()
    with pytest.raises(_cabi.TchGeoError, match="n_groups"):
        _cabi.NsInducedGrouped(g.view, nodes, group, counts, 2, 1, g.n, 0)
    ok = _cabi.NsInducedGrouped(g.view, nodes, group, counts, 2, 1, g.n, 1)
    ok.struct.group = None
    with pytest.raises(_cabi.TchGeoError, match="null group"):
        ok.count()
    ok.struct.group = group.data_ptr()
    ok.ws = ok.ws[:8]                                                             # a short workspace
    with pytest.raises(_cabi.TchGeoError, match="workspace too small"):
        ok.count()
    torch.cuda.synchronize()
    assert int(ok.state.abs().sum()) == 0                                         # nothing ran


def test_status_bits_for_bad_groups_and_ids(karate):
    g, rs = karate, np.random.default_rng(4)
    nodes = rs.permutation(34)[:20]
    group = np.arange(20) % 2
    bad_g = group.copy()
    bad_g[[3, 11]] = [2, -1]                                                      # n_groups and a negative word
    out, _, chunks, st = run(g, [(nodes, bad_g), (nodes, group)], 2)
    assert st == 4                                                                # bit 2
    check(g, [(nodes, bad_g), (nodes, group)], out, n_groups=2)
    assert not np.isin([3, 11], out[0][:2]).any() and chunks[0] == chunks_of(nodes, g.hp, bad_g, 2) == 18
    bad_v = nodes.copy()
    bad_v[[5, 6]] = [g.n, -2]
    out, _, _, st = run(g, [(bad_v, group), (nodes, group)], 2)
    assert st == 2                                                                # bit 1
    check(g, [(bad_v, group), (nodes, group)], out, n_groups=2)
    assert not np.isin([5, 6], out[0][:2]).any()
    out, _, _, st = run(g, [(bad_v, bad_g)], 2)
    assert st == 6
    check(g, [(bad_v, bad_g)], out, n_groups=2)


def _behind_the_sampler(g, timed):
    from tch_geometric import _cabi
    nb, B, fan, H = 8, 16, [4, 3], 2
    rs = np.random.default_rng(21)
    seeds = _cabi.seed_batches(21, 0, nb, B, g.n, DEV)
    seeds[5, 3:] = seeds[5, 0]                                                    # repeated seeds: fewer distinct pairs ...
    seed_group = torch.arange(B, dtype=torch.int32, device=DEV) // 2             # ... two seeds per group
    n_groups, window = B // 2, (0, 400)
    slabs = _cabi.NsBatchedOut(nb, B, fan, DEV, with_states=timed)
    if timed:
        gt = rs.integers(200, 1200, (nb, n_groups))
        seed_times = dev(np.repeat(gt, 2, axis=1))
        _cabi.ns_homo_batched(g.view, seeds, fan, 21, 0, slabs, filter_mode=_cabi.FILTER_RELATIVE, forward=False,
                              window=window, seeds_state=seed_times)
    else:
        _cabi.ns_homo_batched(g.variant(ts=None).view, seeds, fan, 21, 0, slabs)
    u = _cabi.ns_homo_unique_grouped(slabs, nb, g.n, seed_group=seed_group, n_groups=n_groups)
    launch = _cabi.NsInducedGrouped(g.view, u.nodes, u.group, u.counts, 2, nb, g.n, n_groups, node_marks=u.layer_nodes,
                                    group_time=dev(gt) if timed else None, time_window=window if timed else None).count()
    rc, eidx, off = _cabi.ns_induced_emit(launch)
    torch.cuda.synchronize()
    assert int(launch.status.cpu()[0]) == 0
    rc, eidx = rc.cpu().numpy(), eidx.cpu().numpy()
    counts, nodes, grp, ln = (t.cpu().numpy() for t in (u.counts, u.nodes, u.group, u.layer_nodes))
    f_rows, f_cols, f_e = u.rows.cpu().numpy(), u.cols.cpu().numpy(), slabs.edge_index.cpu().numpy()
    marks, chunks = launch.edge_marks.cpu().numpy(), launch.chunks.cpu().numpy()
    assert len(set(counts[:, 0].tolist())) > 1                                    # ragged
    for b in range(nb):
        n, m = counts[b]
        s, gr = nodes[b, :n], grp[b, :n]
        rows, cols, e = grouped_induced_rule(s, gr, g.hp, g.hi, g.hts if timed else None, gt[b] if timed else None,
                                             window if timed else None, n_groups=n_groups)
        got = np.stack([rc[0, off[b]:off[b + 1]], rc[1, off[b]:off[b + 1]], eidx[off[b]:off[b + 1]]])
        assert np.array_equal(got, np.stack([rows, cols, e])), b
        assert marks[b].tolist() == edges_before(cols, ln[b, :H], n) and chunks[b] == chunks_of(s, g.hp)
        induced = set(zip(rows.tolist(), cols.tolist(), e.tolist()))
        forest = set(zip(f_rows[b, :m].tolist(), f_cols[b, :m].tolist(), f_e[b, :m].tolist()))
        assert m > 0 and forest <= induced, b                                     # every relabelled forest edge is induced


def test_behind_the_sampler(rmat12):
    _behind_the_sampler(rmat12, timed=False)


def test_behind_the_temporal_sampler(rmat12):
    _behind_the_sampler(rmat12, timed=True)


def test_transform_on_device_tensors(rmat12):
    from tch_geometric.transforms import induced_subgraph
    g, rs = rmat12, np.random.default_rng(13)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64)).to(DEV)
    for members in ([rs.permutation(4096)[:700], rs.permutation(4096)[:300], rs.permutation(4096)[:5]], [[17]], []):
        nodes, group = disjoint_list(rs, members)
        want = grouped_induced_rule(nodes, group, g.hp, g.hi)
        for id_bound in (None, 1 << 40):
            got = induced_subgraph(t(nodes), g.ptrs, g.idx, id_bound=id_bound, group=t(group))
            for a, w in zip(got, want):
                assert a.dtype == torch.int64 and a.is_cuda and np.array_equal(a.cpu().numpy(), w)
        gt = rs.integers(0, 1000, max(len(members), 1))
        want = grouped_induced_rule(nodes, group, g.hp, g.hi, g.hts, gt, (50, 500))
        got = induced_subgraph(t(nodes), g.ptrs, g.idx, group=t(group), group_time=t(gt), edge_time=g.ts, time_window=(50, 500))
        for a, w in zip(got, want):
            assert np.array_equal(a.cpu().numpy(), w)


def test_transform_retries_past_the_default_capacity(star):
    from tch_geometric.transforms import induced_subgraph
    g = star
    nodes, group = np.zeros(150, dtype=np.int64), np.arange(150)
    nodes[-1], group[-1] = 7, 0                                                   # one member for the first hub
    assert chunks_of(nodes, g.hp) > 150 + -(-g.n_edges // CHUNK)
    got = induced_subgraph(dev(nodes), g.ptrs, g.idx, group=dev(group))
    for a, w in zip(got, grouped_induced_rule(nodes, group, g.hp, g.hi)):
        assert np.array_equal(a.cpu().numpy(), w)
    assert got[0].numel() == int((g.hi[:5000] == 7).sum()) > 0


def test_hub_columns_of_1024_and_1025_chunks_in_two_groups():
    """columns 0 and 1 of exactly 1 024 * 512 and 1 024 * 512 + 1 entries, each named by two groups: 2 048 chunks end with
    the second tile of the chunk prefix, 2 050 leave two chunks (the second one entry long) in a third.  The second
    group's hub starts at chunk 1 024 or 1 025, where a mark reads the prefix; both columns end in a member of every group"""
    n, degs = 20000, [1024 * CHUNK, 1024 * CHUNK + 1]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(17)
    idx = torch.randint(2, n - 1, (sum(degs),), device=DEV, generator=gen)
    idx[degs[0] - 1] = idx[sum(degs) - 1] = n - 1
    ptrs = torch.full((n + 1,), sum(degs), dtype=torch.int64, device=DEV)
    ptrs[0], ptrs[1] = 0, degs[0]
    g = DeviceGraph(ptrs, idx)
    rs = np.random.default_rng(18)
    lists = [disjoint_list(rs, [np.concatenate([[hub, n - 1], rs.choice(np.arange(2, n - 1), 40, replace=False)])
                                for _ in range(2)], shuffle=False) for hub in (0, 1)]
    marks = np.array([[42, 84], [42, 43]])                                      # position 42: the second group's hub
    out, mk, chunks, st = run(g, lists, 2, marks=marks)
    assert st == 0 and chunks.tolist() == [2048, 2050] and all(s[42] == hub for hub, (s, _) in enumerate(lists))
    check(g, lists, out, n_groups=2)
    for b, (s, _) in enumerate(lists):
        assert mk[b].tolist() == edges_before(out[b][1], marks[b], len(s))
        last = out[b][:, out[b][2] == g.hp[b + 1] - 1]                          # the column's last entry, once per group
        assert last[1].tolist() == [0, 42] and last[0].tolist() == [1, 43]
        assert 0 < mk[b][0] < out[b].shape[1] and out[b].shape[1] > 1000
