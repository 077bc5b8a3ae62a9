"""tg_cluster_count / tg_cluster_emit on the GPU: every output word (n_nodes, n_edges, nodes, rows, cols, edge_index, status)
equals the NumPy restatement (helpers_cluster.cluster_rule = expand + helpers_induced.induced_rule) and equals
_cabi.NsInduced on the expanded node lists; the output arrays are filled with a sentinel beforehand and the words past the
written ranges are checked.  One graph of about 2 200 nodes and 38 000 edges whose properties are asserted below, and a
second one of 1 024 clusters of one or two nodes for the widest list."""
import functools

import numpy as np
import pytest
import torch

from helpers_cluster import CHUNK, chunk_bound, chunks_of, cluster_rule, expand

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL, SLACK = -77, 19

SIZES = [513, 0, 1, 63, 64, 65, 0, 100, 7, 300, 40, 2, 130, 90, 3, 50, 64, 200, 11, 120, 75, 33, 66,
         5, 9, 14, 20, 6, 8, 12, 16, 10, 4, 17, 3, 19, 2, 13, 1, 0, 15, 18, 11]
HUB, FULL, SHORT, GAP = 0, 4, 8, 9        # clusters: with the hub column | of exactly 2 chunks | shorter than a chunk | with 70 empty columns


def build_main():
    rs = np.random.default_rng(2024)
    partptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    n = int(partptr[-1])
    deg = rs.integers(0, 33, n)
    deg[partptr[HUB] + 200] = 2500                                       # a hub column inside the first cluster
    deg[partptr[HUB]] = 0                                                # empty columns at a cluster's two ends
    deg[partptr[HUB + 1] - 1] = 0
    lo, hi = partptr[FULL], partptr[FULL + 1]                            # 64 columns of 16 entries: 1 024 = two full chunks
    deg[lo:hi] = 16
    lo, hi = partptr[SHORT], partptr[SHORT + 1]                          # 7 columns, 66 entries
    deg[lo:hi] = [10, 0, 20, 1, 30, 0, 5]
    deg[partptr[GAP] + 20:partptr[GAP] + 90] = 0                         # more column ends than lanes inside one step
    ptrs = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = rs.integers(0, n, int(ptrs[-1])).astype(np.int64)
    for v in rs.permutation(n)[:150]:                                    # self loops, and parallel edges next to them
        if deg[v] >= 3:
            indices[ptrs[v]] = v
            indices[ptrs[v] + 2] = indices[ptrs[v] + 1]
    return partptr, ptrs, indices


def build_wide():
    rs = np.random.default_rng(7)
    sizes = rs.integers(1, 3, 1024)
    partptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(partptr[-1])
    ptrs = np.concatenate([[0], np.cumsum(rs.integers(0, 9, n))]).astype(np.int64)
    return partptr, ptrs, rs.integers(0, n, int(ptrs[-1])).astype(np.int64)


class Fixture:
    def __init__(self, partptr, ptrs, indices):
        from tch_geometric import _cabi
        self.partptr, self.ptrs, self.indices = partptr, ptrs, indices
        self.n, self.P, self.E = int(partptr[-1]), partptr.size - 1, indices.size
        t = lambda a: torch.from_numpy(a).to(DEV)
        self.d_partptr, self.d_ptrs, self.d_indices = t(partptr), t(ptrs), t(indices)
        self.views = dict(i64=_cabi.graph_view(self.d_ptrs, self.d_indices),
                          i32=_cabi.graph_view(self.d_ptrs, self.d_indices, indices32=self.d_indices.to(torch.int32),
                                               ptrs32=self.d_ptrs.to(torch.int32)))
        self.node_ids = np.random.default_rng(1).permutation(self.n).astype(np.int64) * 3 + 5
        self.d_node_ids = t(self.node_ids)
        self.rule = functools.lru_cache(maxsize=None)(self._rule)

    def _rule(self, clusters, pitch, partptr_key):
        partptr = self.partptr if partptr_key is None else np.asarray(partptr_key, dtype=np.int64)
        return cluster_rule(partptr, list(clusters), self.ptrs, self.indices, pitch=pitch, n_major=self.n)


@pytest.fixture(scope="module")
def main():
    fx = Fixture(*build_main())
    partptr, ptrs, indices = fx.partptr, fx.ptrs, fx.indices
    deg = np.diff(ptrs)
    assert 2000 <= fx.n <= 2400 and 36000 <= fx.E <= 44000
    # edge properties
    assert deg.max() > 4 * CHUNK and (deg == 0).any()
    col = np.repeat(np.arange(fx.n), deg)
    assert (indices == col).sum() >= 10                                  # self loops
    same = (indices[1:] == indices[:-1]) & (col[1:] == col[:-1])
    assert same.sum() >= 10                                              # parallel edges
    # cluster sizes
    assert {0, 1, 63, 64, 65, 513} <= set(np.diff(partptr).tolist())
    # boundaries: a cluster's chunks start at its own first offset, so its end is a chunk boundary iff its range is a
    # multiple of 512
    span = ptrs[partptr[1:]] - ptrs[partptr[:-1]]
    assert span[FULL] == 2 * CHUNK                                       # exactly on a chunk boundary
    assert (span % CHUNK != 0).sum() >= 20                               # inside a chunk
    assert 0 < span[SHORT] < CHUNK and SIZES[SHORT] == 7                 # shorter than one chunk, several columns
    assert span[HUB] > 6 * CHUNK                                         # the hub's cluster: many chunks, the hub split
    lo = partptr[GAP]
    assert (deg[lo + 20:lo + 90] == 0).all() and deg[lo + 19] > 0 and deg[lo + 90] > 0 and SIZES[GAP] > 90
    assert deg[partptr[HUB]] == 0 and deg[partptr[HUB + 1] - 1] == 0
    return fx


@pytest.fixture(scope="module")
def wide():
    fx = Fixture(*build_wide())
    assert fx.P == 1024 and set(np.diff(fx.partptr).tolist()) == {1, 2}
    return fx


def run(fx, lists, pitch, view="i32", n_clusters=True, node_ids=False, nodes_null=False, partptr=None, pad=None,
        compare_hash=True):
    """one launch over `lists` (python lists of cluster ids) against the restatement and the hash pair -> the status word"""
    from tch_geometric import _cabi
    G = len(lists)
    pad = fx.P + 3 if pad is None else pad                               # what an entry past n_clusters holds: never read
    cl = np.full((G, pitch), pad, dtype=np.int64)
    for b, l in enumerate(lists):
        assert len(l) <= pitch and (n_clusters or len(l) == pitch)
        cl[b, :len(l)] = l
    d_cl = torch.from_numpy(cl).to(DEV)
    d_nc = torch.tensor([len(l) for l in lists], dtype=torch.int64, device=DEV) if n_clusters else None
    d_pp = fx.d_partptr if partptr is None else torch.from_numpy(partptr).to(DEV)
    key = None if partptr is None else tuple(partptr.tolist())
    launch = _cabi.ClusterInduced(fx.views[view], d_pp, d_cl, d_nc, fx.d_node_ids if node_ids else None)
    launch.count()
    want = [fx.rule(tuple(int(c) for c in l), pitch, key) for l in lists]
    state = launch.state.cpu()
    status = int(state[-1:].view(torch.int32)[0])
    want_status = 0
    for w in want:
        want_status |= w[4]
    assert status == want_status
    n_nodes, n_edges = state[:G].numpy(), state[G:2 * G].numpy()
    assert n_nodes.tolist() == [w[0].size for w in want] and n_edges.tolist() == [w[1].size for w in want]
    tn, te = int(n_nodes.sum()), int(n_edges.sum())
    o = dict(dtype=torch.int64, device=DEV)
    nodes = None if nodes_null else torch.full((tn + SLACK,), SENTINEL, **o)
    rows, cols, eidx = (torch.full((te + SLACK,), SENTINEL, **o) for _ in range(3))
    node_off = torch.cumsum(launch.n_nodes, 0) - launch.n_nodes
    edge_off = torch.cumsum(launch.n_edges, 0) - launch.n_edges
    launch.emit_into(node_off, edge_off, nodes, rows, cols, eidx)
    cat = lambda k: np.concatenate([w[k] for w in want]) if want else np.zeros(0, dtype=np.int64)
    for got, k, total in ((nodes, 0, tn), (rows, 1, te), (cols, 2, te), (eidx, 3, te)):
        if got is None:
            continue
        got = got.cpu().numpy()
        exp = cat(k)
        if k == 0 and node_ids:
            exp = fx.node_ids[exp]
        assert np.array_equal(got[:total], exp), "output %d differs" % k
        assert (got[total:] == SENTINEL).all(), "output %d: written past its range" % k
    if compare_hash:                                                     # the existing pair on the expanded lists
        pp = fx.partptr if partptr is None else partptr
        ex = [np.zeros(0, dtype=np.int64) if w[4] & 1 else expand(pp, l, fx.n)[0] for w, l in zip(want, lists)]
        width = max([1] + [e.size for e in ex])
        slab = np.zeros((G, width), dtype=np.int64)
        for b, e in enumerate(ex):
            slab[b, :e.size] = e
        counts = torch.tensor([e.size for e in ex], dtype=torch.int64, device=DEV)
        ind = _cabi.ns_induced_count(fx.views[view], torch.from_numpy(slab).to(DEV), counts, 1, G, fx.n)
        rc, e_hash, off = _cabi.ns_induced_emit(ind)
        assert off[-1] == te and torch.equal(rc[0], rows[:te]) and torch.equal(rc[1], cols[:te]) and torch.equal(e_hash, eidx[:te])
    return status


def lists_of(fx, q, G, seed, distinct=8):
    """G lists of q distinct clusters, drawn from a few distinct ones so that the restatement is computed once per list"""
    rs = np.random.default_rng(seed)
    pool = [rs.permutation(fx.P)[:q].tolist() for _ in range(min(distinct, G))]
    return [pool[i] for i in rs.integers(0, len(pool), G)]


@pytest.mark.parametrize("view", ["i64", "i32"])
@pytest.mark.parametrize("q", [0, 1, 2, 37])
def test_list_lengths(main, q, view):
    """n_clusters NULL: every list is the pitch wide; q = 37 names the hub's cluster, the two-chunk one and the gap"""
    lists = lists_of(main, q, 3, q)
    if q == 37:
        rest = [c for c in range(main.P) if c not in (HUB, FULL, SHORT, GAP)]
        lists[0] = [GAP, SHORT] + rest[:33] + [FULL, HUB]
    if q == 1:
        lists = [[HUB], [GAP], [FULL]]
    if q == 2:
        lists[0] = [SHORT, 1]                                            # a short cluster beside an empty one
    assert run(main, lists, q, view=view, n_clusters=False) == 0


@pytest.mark.parametrize("view", ["i64", "i32"])
def test_all_clusters_one_by_one_and_together(main, view):
    assert run(main, [[c] for c in range(main.P)], 1, view=view) == 0
    order = list(range(main.P))
    assert run(main, [order, order[::-1]], main.P, view=view) == 0       # the whole graph, sorted and reversed


def test_the_widest_list(wide):
    rs = np.random.default_rng(3)
    lists = [rs.permutation(1024).tolist(), list(range(1024))[::-1], rs.permutation(1024)[:1000].tolist()]
    assert run(wide, lists, 1024, n_clusters=True) == 0
    assert run(wide, lists[:2], 1024, view="i64", n_clusters=False, node_ids=True) == 0


@pytest.mark.parametrize("view", ["i64", "i32"])
def test_short_rows_unsorted_and_reversed(main, view):
    rs = np.random.default_rng(11)
    p = rs.permutation(main.P)
    lists = [p[:20].tolist(), sorted(p[:20].tolist()), sorted(p[:20].tolist())[::-1], [], [HUB], p[20:25].tolist(), [1, 6, 39]]
    assert run(main, lists, 24, view=view, node_ids=True) == 0           # short rows; the last list names only empty clusters
    assert run(main, lists, 24, view=view, nodes_null=True) == 0


def test_repeated_cluster_first_occurrence_and_overflow(main):
    """a cluster named again: local = its first occurrence, every position scans its column; past the workspace's chunk bound
    the batch is empty and bit 0 rises, the other batches of the launch are untouched"""
    pitch = 8
    one = chunks_of(main.partptr, [HUB], main.ptrs)
    bound = chunk_bound(pitch, main.E)
    assert 3 * one + 2 <= bound < 8 * one
    lists = [[HUB] * 8, [FULL, SHORT], [HUB, 5, HUB, 5, HUB], [3, 3]]
    assert run(main, lists, pitch) == 1
    want = main.rule((HUB, 5, HUB, 5, HUB), pitch, None)
    assert want[4] == 0 and want[0].size == 3 * SIZES[HUB] + 2 * SIZES[5] and want[1].max() < SIZES[HUB] + SIZES[5]
    assert run(main, lists[1:], pitch, view="i64") == 0


def test_bad_cluster_ids(main):
    lists = [[3, -1, 7], [main.P, 4], [2, 5]]
    assert run(main, lists, 3) == 2
    assert run(main, [[-1], [main.P]], 1, n_clusters=False) == 2
    assert run(main, [[2 ** 40, 3], [-2 ** 40, 4]], 2, view="i64") == 2


def test_bad_partptr(main):
    c = 20
    inverted = main.partptr.copy()
    inverted[c + 1] = inverted[c] - 3                                    # cluster c = [x, x - 3)
    assert run(main, [[c, 3, 30], [5, 12]], 3, partptr=inverted) == 4
    leaves = main.partptr.copy()
    leaves[-1] += 5                                                      # the last cluster ends past n_major
    assert run(main, [[main.P - 1, 3], [5, 12]], 2, partptr=leaves, view="i64") == 4
    negative = main.partptr.copy()
    negative[0] = -4
    assert run(main, [[0, 3]], 2, partptr=negative) == 4
    assert run(main, [[c, -1, 3]], 3, partptr=inverted) == 6             # both bits


@pytest.mark.parametrize("G", [1, 3, 300])
def test_batch_counts(main, G):
    lists = lists_of(main, 5, G, 100 + G, distinct=12)
    assert run(main, lists, 5, node_ids=True) == 0


def test_more_batches_than_a_grid_round(wide):
    G = 32768 + 5
    lists = lists_of(wide, 2, G, 9, distinct=16)
    lists[-1] = [1023, 0]
    assert run(wide, lists, 2, n_clusters=False) == 0


LONG, LONGER, UNIT, UNIT1, SMALL = 0, 1, 2, 3, 4  # clusters whose offset ranges are 1 024, 1 025, 16, 17 chunks | short columns


@pytest.fixture(scope="module")
def seams():
    """offset ranges at the seams of the chunk prefix, built on the device: 64 columns of 8 192 entries (1 024 * 512: the
    range ends with a tile of chunks), the same with one entry more (a second tile of one chunk of one entry), 4 columns of
    2 048 (16 chunks: one unit) and the same with one entry more; every range's last entry names a node of its cluster"""
    n = 20000
    sizes = [64, 64, 4, 4, 64, n - 200]
    partptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    deg = torch.zeros(n, dtype=torch.int64, device=DEV)
    deg[0:128], deg[127] = 8192, 8193
    deg[128:136], deg[135] = 2048, 2049
    gen = torch.Generator(device=DEV)
    gen.manual_seed(31)
    deg[136:200] = torch.randint(0, 9, (64,), device=DEV, generator=gen)
    ptrs = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(deg, 0)])
    indices = torch.randint(0, n, (int(ptrs[-1]),), device=DEV, generator=gen)
    ends = ptrs[torch.from_numpy(partptr[1:5]).to(DEV)] - 1
    indices[ends] = torch.from_numpy(partptr[:4]).to(DEV)
    fx = Fixture(partptr, ptrs.cpu().numpy(), indices.cpu().numpy())
    span = fx.ptrs[partptr[1:5]] - fx.ptrs[partptr[:4]]
    assert span.tolist() == [1024 * CHUNK, 1024 * CHUNK + 1, 16 * CHUNK, 16 * CHUNK + 1]
    return fx


@pytest.mark.parametrize("view", ["i64", "i32"])
def test_ranges_at_the_tile_and_unit_seams(seams, view):
    lists = [[LONG], [LONGER], [UNIT], [UNIT1], [UNIT1, SMALL, LONGER]]
    assert [chunks_of(seams.partptr, l, seams.ptrs) for l in lists] == [1024, 1025, 16, 17, 17 + 1 + 1025]
    assert run(seams, lists, 3, view=view) == 0
    for l, c in zip(lists[:4], (LONG, LONGER, UNIT, UNIT1)):             # the hit in the range's last entry, its last chunk
        nodes, rows, cols, eidx, _ = seams.rule(tuple(l), 3, None)
        assert eidx[-1] == seams.ptrs[seams.partptr[c + 1]] - 1 and rows[-1] == 0 and cols[-1] == nodes.size - 1
