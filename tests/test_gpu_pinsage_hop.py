"""tg_pinsage_hop on the GPU: every output word against the NumPy restatement (helpers_pinsage.py) on top of the walks
of _cabi.random_walk -- the hop's contract is that, without termination, walker w is row w of that call -- over the tile
sizes, visit counts, fan-outs and frontier sizes at which the kernel takes another path; then the count law of the
termination draws against Binomial(16, 1/2), which does not go through the restatement's Philox."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import exact_laws
from helpers_pinsage import csx, select, truncate
from helpers_saint import random_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 300
SEED = 0x51A6E


def dev(a, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


class View:
    """a graph view on the device with its host arrays"""

    def __init__(self, ptrs, idx, small=False):
        from tch_geometric import _cabi
        self.ptrs, self.idx, self.n = np.asarray(ptrs, dtype=np.int64), np.asarray(idx, dtype=np.int64), len(ptrs) - 1
        self._keep = [dev(self.ptrs), dev(self.idx if len(self.idx) else np.zeros(1, dtype=np.int64))]
        kw = {}
        if small:
            self._keep += [self._keep[0].to(torch.int32), self._keep[1].to(torch.int32)]
            kw = dict(ptrs32=self._keep[2], indices32=self._keep[3])
        self.g = _cabi.graph_view(self._keep[0], self._keep[1], **kw)
        self.g.n_edges = len(self.idx)
        self.deg = np.diff(self.ptrs)


@pytest.fixture(scope="module")
def graphs():
    ei = random_graph(N, 2000, 0.1, seed=3)
    csr, csc = csx(ei, N, False), csx(ei, N, True)
    return dict(ei=ei, csr=View(*csr), csc=View(*csc), csr32=View(*csr, small=True))


def restated(view, vertices, R, T, alpha, k, call_id=0, call_ids=None, ids=None, tag=15, seed=SEED):
    """the hop from _cabi.random_walk's rows: start of walker ids[i] * R + r = vertices[i]; one walk call per call id"""
    from tch_geometric import _cabi
    v = np.asarray(vertices, dtype=np.int64)
    m = len(v)
    ids_ = np.arange(m, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    calls = np.full(m, call_id, dtype=np.int64) if call_ids is None else np.asarray(call_ids, dtype=np.int64)
    bad = (v < 0) | (v >= view.n)
    if m == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, np.zeros(1, dtype=np.int64), z, z, z
    start = np.zeros((int(ids_.max()) + 1) * R, dtype=np.int64)          # walkers nobody owns start at vertex 0
    start[(ids_[:, None] * R + np.arange(R)[None, :]).reshape(-1)] = np.repeat(np.where(bad, 0, v), R)
    cut = np.empty((m * R, T + 1), dtype=np.int64)
    for c in np.unique(calls):
        walks = _cabi.random_walk(view.g, dev(start), T, 1.0, 1.0, seed, int(c)).cpu().numpy()
        t = truncate(walks, seed, np.uint64(c), R, alpha, ids_, tag)
        rows = np.repeat(calls == c, R)
        cut[rows] = t[rows]
    cnt, nbr, par, vis = select(cut, R, k, skip=np.flatnonzero(bad))
    return cnt, np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), nbr, par, vis


def run(view, vertices, R, T, alpha, k, call_id=0, call_ids=None, ids=None, tag=0, seed=SEED):
    from tch_geometric import _cabi
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = _cabi.pinsage_hop(view.g, dev(vertices), k, R, T, alpha, seed, call_id,
                            call_ids=None if call_ids is None else dev(call_ids), ids=None if ids is None else dev(ids),
                            rng_tag=tag, status=status)
    cnt, off, nbr, par, vis = (t.cpu().numpy() for t in out)
    total = int(off[-1])
    return (cnt, off, nbr[:total], par[:total], vis[:total]), int(status.item())


def check(view, vertices, R, T, alpha, k, want_status=0, **kw):
    tag = kw.pop("tag", 0)                                  # 0: the hop takes TG_TAG_PINSAGE
    got, status = run(view, vertices, R, T, alpha, k, tag=tag, **kw)
    want = restated(view, vertices, R, T, alpha, k, tag=tag or 15, **kw)
    for name, g, w in zip(("cnt", "offsets", "neighbors", "parents", "visits"), got, want):
        assert np.array_equal(g, w), (name, R, T, alpha, k)
    assert status == want_status
    return got


def frontier(m, seed=0):
    return np.random.default_rng(seed).integers(0, N, m).astype(np.int64)


@pytest.mark.parametrize("R,T", [(1, 1), (1, 3), (10, 2), (63, 1), (64, 1), (65, 1), (63, 2), (10, 20), (200, 3), (200, 20),
                                 (65, 3), (2048, 2), (64, 64), (1, 20)])
def test_walk_and_visit_shapes(graphs, R, T):
    """R and T around the chunk width, every row size 64 .. 4096 and the limit V = 4096 (one slot per tile)"""
    m = 37 if R * T <= 1024 else 5
    got = check(graphs["csr"], frontier(m, R + T), R, T, 0.5, 3)
    assert got[0].max() <= 3 and (got[4] >= 1).all() and got[4].max() <= R * T


@pytest.mark.parametrize("alpha", [0.0, 0.5, 0.99])
def test_termination(graphs, alpha):
    v = frontier(61, 5)
    got = check(graphs["csr"], v, 10, 3, alpha, 64)
    if alpha == 0.0:                                        # no draw is made: the visits are all of tg_random_walk's rows
        from tch_geometric import _cabi
        walks = _cabi.random_walk(graphs["csr"].g, dev(np.repeat(v, 10)), 3, 1.0, 1.0, SEED, 0).cpu().numpy()
        assert int(got[4].sum()) == int((walks[:, 1:] >= 0).sum())
        assert (walks[:, 1:] < 0).any() and (walks[:, 2][walks[:, 1] >= 0] < 0).any()     # sinks reached mid-walk


@pytest.mark.parametrize("k", [1, 3, 64])
def test_fanouts_and_fewer_distinct_than_k(graphs, k):
    got = check(graphs["csr"], frontier(50, 9), 200, 3, 0.5, k)
    assert got[0].max() == k if k < 64 else got[0].max() <= 64
    got = check(graphs["csr"], frontier(50, 9), 2, 2, 0.5, k)             # at most 4 distinct visits
    assert got[0].max() <= min(k, 4)


@pytest.mark.parametrize("m", [0, 1, 5, 257, 4099])
def test_frontier_sizes(graphs, m):
    got = check(graphs["csr"], frontier(m, m), 10, 2, 0.5, 3)
    assert got[1][0] == 0 and len(got[0]) == m


def test_special_slots_and_status(graphs):
    view = graphs["csr"]
    sink = int(np.flatnonzero(view.deg == 0)[0])
    live = int(np.flatnonzero(view.deg > 0)[0])
    v = np.array([live, -1, sink, live, -7, live], dtype=np.int64)
    got = check(view, v, 10, 3, 0.5, 5)
    assert got[0][1] == got[0][2] == got[0][4] == 0 and got[0][0] > 0
    assert not np.array_equal(got[2][:got[0][0]], got[2][got[1][3]:got[1][4]]) or \
        not np.array_equal(got[4][:got[0][0]], got[4][got[1][3]:got[1][4]])     # the same vertex, other ids: other lists
    bad = np.array([live, N, live + 1, N + 12345, 2 ** 40, live], dtype=np.int64)
    got = check(view, bad, 10, 3, 0.5, 5, want_status=2)
    assert got[0][1] == got[0][3] == got[0][4] == 0 and got[0][0] > 0 and got[0][5] > 0


def test_ties_rank_by_id(graphs):
    # a star: the centre 0 has 40 leaves; R = 40, T = 1: many leaves tie on their count
    ptrs = np.concatenate([[0], np.full(41, 40)]).astype(np.int64)
    star = View(ptrs, np.arange(1, 41, dtype=np.int64))
    got = check(star, np.zeros(3, dtype=np.int64), 40, 1, 0.5, 64)
    for i in range(3):
        nbr, vis = got[2][got[1][i]:got[1][i + 1]], got[4][got[1][i]:got[1][i + 1]]
        assert vis.sum() == 40 and (np.diff(vis) <= 0).all()
        same = np.diff(vis) == 0
        assert same.any() and (np.diff(nbr)[same] > 0).all()
    # parallel edges and self loops
    ptrs = np.array([0, 4, 7, 9], dtype=np.int64)
    idx = np.array([0, 1, 1, 2, 1, 1, 2, 0, 0], dtype=np.int64)
    check(View(ptrs, idx), np.array([0, 1, 2, 0, 1], dtype=np.int64), 30, 4, 0.3, 3)


def test_u32_shadows_and_both_directions(graphs):
    v = frontier(90, 11)
    a = check(graphs["csr"], v, 10, 3, 0.5, 4)
    b = check(graphs["csr32"], v, 10, 3, 0.5, 4)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    c = check(graphs["csc"], v, 10, 3, 0.5, 4)
    assert not np.array_equal(a[2], c[2])                   # an asymmetric graph: walking against the edges differs


def test_call_ids_ids_and_tag(graphs):
    m = 70
    v = frontier(m, 13)
    rs = np.random.default_rng(1)
    calls = rs.choice([5, 6, 2 ** 40 + 1], m).astype(np.int64)
    ids = rs.permutation(m).astype(np.int64)
    check(graphs["csr"], v, 10, 3, 0.5, 3, call_ids=calls)
    check(graphs["csr"], v, 10, 3, 0.5, 3, ids=ids)
    base = check(graphs["csr"], v, 10, 3, 0.5, 3, call_ids=calls, ids=ids)
    tagged = check(graphs["csr"], v, 10, 3, 0.5, 3, call_ids=calls, ids=ids, tag=99)
    assert not np.array_equal(base[4], tagged[4]) or not np.array_equal(base[2], tagged[2])
    other = check(graphs["csr"], v, 10, 3, 0.5, 3, call_id=8)
    assert not np.array_equal(other[2], check(graphs["csr"], v, 10, 3, 0.5, 3, call_id=9)[2])


def test_words_past_the_total_are_untouched(graphs):
    from tch_geometric import _cabi
    view, m, k = graphs["csr"], 33, 7
    v = dev(frontier(m, 17))
    o = dict(dtype=torch.int64, device=DEV)
    cnt, off = torch.full((m,), -5, **o), torch.full((m + 1,), -5, **o)
    nbr, par, vis = (torch.full((m * k,), -5 - j, **o) for j in range(3))
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.empty(_cabi.pinsage_hop_workspace_bytes(m, k) // 8, **o)
    hin, hout = _cabi.TgHopIn(), _cabi.TgHopOut()
    hin.vertices, hin.m, hin.fanout = v.data_ptr(), m, k
    hout.cnt, hout.offsets, hout.neighbors, hout.parents = cnt.data_ptr(), off.data_ptr(), nbr.data_ptr(), par.data_ptr()
    cfg, rng = _cabi.TgPinsageConfig(2, 2, 0.5, 0), _cabi.TgRng(SEED, 0)
    _cabi.check(_cabi.lib.tg_pinsage_hop(C.byref(view.g), C.byref(hin), C.byref(cfg), C.byref(rng), C.byref(hout),
                                         _cabi.ptr(vis), _cabi.ptr(status), _cabi.ptr(ws), C.c_int64(ws.numel() * 8),
                                         _cabi.stream_ptr(torch.device(DEV))))
    total = int(off[m])
    want = restated(view, v.cpu().numpy(), 2, 2, 0.5, k)
    assert 0 < total < m * k and total == want[1][-1]
    for j, (t, w) in enumerate(((nbr, want[2]), (par, want[3]), (vis, want[4]))):
        assert np.array_equal(t[:total].cpu().numpy(), w) and bool((t[total:] == -5 - j).all())


def test_count_law_of_the_termination_draws():
    """s -> a, a -> b, b a sink; 16 384 slots at s, R = 16, T = 2, alpha = 1/2: every slot reports a with count 16, and b's
    count (0 when absent) follows Binomial(16, 1/2) -- the statistic and threshold of the other law tests."""
    from tch_geometric import _cabi
    view = View(np.array([0, 1, 2, 2], dtype=np.int64), np.array([1, 2], dtype=np.int64))
    M, R = 16384, 16
    cnt, off, nbr, par, vis = (t.cpu().numpy() for t in _cabi.pinsage_hop(view.g, dev(np.zeros(M, dtype=np.int64)), 2, R, 2,
                                                                          0.5, 5, 0))
    total = int(off[-1])
    nbr, par, vis = nbr[:total], par[:total], vis[:total]
    assert (cnt >= 1).all() and (nbr[off[:-1]] == 1).all() and (vis[off[:-1]] == R).all()
    b = np.zeros(M, dtype=np.int64)
    second = nbr == 2
    assert second.sum() == (cnt == 2).sum() and total == M + second.sum()
    b[par[second]] = vis[second]
    law = np.array([math.comb(R, c) * 0.5 ** R for c in range(R + 1)])
    exact_laws.chi2_gof(np.bincount(b, minlength=R + 1), law, "count of b over %d slots" % M)
