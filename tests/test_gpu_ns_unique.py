"""tg_ns_homo_unique on the device: per-batch node dedup and relabel of the tg_ns_homo_batched slabs, word for word against
the NumPy statement of the rule (helpers_unique.unique_rule), under the LDS form and the flat form, with every slab
pre-filled with a sentinel so that words past the counts are seen to be untouched; and NeighborLoader(unique=True)."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import load_fake_dataset, load_karate
from helpers_unique import unique_rule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7                                               # no id, no position, no count


class Slabs:
    """Input slabs of tg_ns_homo_unique with NsBatchedOut's field names, written by the test or copied from a sampler."""

    def __init__(self, samples, rows, cols, layer_offsets, counts, n_seeds, n_hops):
        from tch_geometric import _cabi
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV)
        self.samples, self.rows, self.cols = dev(samples), dev(rows), dev(cols)
        self.edge_index = torch.full_like(self.rows, SENT)
        self.layer_offsets, self.counts, self.states = dev(layer_offsets), dev(counts), None
        self.n_batches, self.n_seeds, self.n_hops = self.samples.shape[0], n_seeds, n_hops
        self.host = (np.array(samples, dtype=np.int64), np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64),
                     np.array(layer_offsets, dtype=np.int64), np.array(counts, dtype=np.int64))
        self.struct = lambda: _cabi.NsBatchedOut.struct(self)

    def clone(self):
        return Slabs(*self.host, self.n_seeds, self.n_hops)


def synthetic(batches, n_seeds, n_hops, cap_nodes=None, seed=0):
    """Slabs from per-batch id lists (a batch's list is its samples[:n]; the first n_seeds are its seeds): edges as the
    sampler lays them out -- rows[e] = n_seeds + e, cols[e] = an earlier position -- hop h starting at an increasing
    position, everything past the counts holding the sentinel."""
    rs = np.random.default_rng(seed)
    nb = len(batches)
    cap_nodes = cap_nodes or max(max(len(s) for s in batches), 1)
    cap_edges = max(cap_nodes - n_seeds, 1)
    S, R, Cc = (np.full((nb, c), SENT, dtype=np.int64) for c in (cap_nodes, cap_edges, cap_edges))
    lo, counts = np.zeros((nb, max(n_hops, 1), 3), dtype=np.int64), np.zeros((nb, 2), dtype=np.int64)
    for b, s in enumerate(batches):
        n, m = len(s), max(len(s) - n_seeds, 0)
        S[b, :n] = s
        R[b, :m] = n_seeds + np.arange(m)
        Cc[b, :m] = (rs.random(m) * (n_seeds + np.arange(m))).astype(np.int64)
        counts[b] = (n, m)
        for h in range(n_hops):
            start = min(n, n_seeds) + (m * h) // n_hops
            lo[b, h] = (start, max(start - n_seeds, 0), start)
    return Slabs(S, R, Cc, lo, counts, n_seeds, n_hops)


def run(slabs, id_bound, form=0, ws=None, in_place=False, n_batches=None):
    """One call with sentinel-filled outputs -> the NsUniqueOut, synchronised."""
    from tch_geometric import _cabi
    res = _cabi.NsUniqueOut(slabs, in_place=in_place)
    for t in (res.nodes, res.inverse, res.counts, res.layer_nodes) + (() if in_place else (res.rows, res.cols)):
        t.fill_(SENT)
    _cabi.ns_homo_unique(slabs, slabs.n_batches if n_batches is None else n_batches, id_bound, form=form, ws=ws, result=res)
    torch.cuda.synchronize()
    return res


def host(res):
    return {k: getattr(res, k).cpu().numpy() for k in ("nodes", "inverse", "rows", "cols", "counts", "layer_nodes")}


def check(res, slabs, n_batches=None):
    """Every output word of every batch against the rule; the words past n_unique / n / m still hold the sentinel."""
    S, R, Cc, lo, counts = slabs.host
    got = host(res)
    nb = slabs.n_batches if n_batches is None else n_batches
    for b in range(nb):
        n, m = counts[b]
        nodes, inverse, rows_u, cols_u, layer_nodes = unique_rule(S[b, :n], R[b, :m], Cc[b, :m], lo[b, :slabs.n_hops, 0])
        u = nodes.size
        assert got["counts"][b].tolist() == [u, m], (b, got["counts"][b], u, m)
        assert np.array_equal(got["nodes"][b, :u], nodes), b
        assert np.array_equal(got["inverse"][b, :n], inverse), b
        assert np.array_equal(got["rows"][b, :m], rows_u) and np.array_equal(got["cols"][b, :m], cols_u), b
        assert got["layer_nodes"][b].tolist() == layer_nodes, (b, got["layer_nodes"][b], layer_nodes)
        assert (got["nodes"][b, u:] == SENT).all() and (got["inverse"][b, n:] == SENT).all(), b
        assert (got["rows"][b, m:] == SENT).all() and (got["cols"][b, m:] == SENT).all(), b
    for k in got:
        assert (got[k][nb:] == SENT).all(), k                         # batches the call was not asked for
    assert (res.edge_index.cpu().numpy() == SENT).all()               # edge_index is not touched
    return got


def both_forms(slabs, id_bound):
    """Form 1 and form 2 against the rule, and against each other."""
    a, b = check(run(slabs, id_bound, form=1), slabs), check(run(slabs, id_bound, form=2), slabs)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    return a


def sampled(ei, n, n_batches, n_seeds, fanout, seed):
    """Slabs sampled by tg_ns_homo_batched, the words past the counts overwritten with the sentinel."""
    from tch_geometric import _cabi
    t = torch.from_numpy(ei).to(DEV)
    ptrs, idx, _ = _cabi.coo_to_csx(t[0].contiguous(), t[1].contiguous(), n, n, True)
    g = _cabi.graph_view(ptrs, idx)
    seeds = _cabi.seed_batches(seed, 0, n_batches, n_seeds, n, DEV)
    out = _cabi.NsBatchedOut(n_batches, n_seeds, fanout, DEV)
    _cabi.ns_homo_batched(g, seeds, fanout, seed, 0, out)
    torch.cuda.synchronize()
    counts = out.counts.cpu().numpy()
    S, R, Cc = out.samples.cpu().numpy(), out.rows.cpu().numpy(), out.cols.cpu().numpy()
    for b in range(n_batches):
        S[b, counts[b, 0]:] = SENT
        R[b, counts[b, 1]:] = SENT
        Cc[b, counts[b, 1]:] = SENT
    return Slabs(S, R, Cc, out.layer_offsets.cpu().numpy(), counts, n_seeds, len(fanout))


@pytest.fixture(scope="module")
def karate():
    ei, n = load_karate()
    return sampled(ei, n, 256, 4, [5, 5], 11)


@pytest.fixture(scope="module")
def rmat16():
    from tch_geometric import _cabi
    n = 1 << 16
    row, col = _cabi.rmat_edges(16, n * 16, 0x5EED0010, DEV)
    return sampled(torch.stack([row, col]).cpu().numpy(), n, 8, 1024, [15, 10], 5)


def test_karate_256_batches_both_forms(karate):
    """34 vertices, 124 slots per batch: heavy duplication, one workgroup per batch in LDS or 256 one-tile batches flat."""
    from tch_geometric import _cabi
    assert _cabi.ns_homo_unique_form(karate.samples.shape[1], 34)[0] == 1
    assert _cabi.ns_homo_unique_workspace_bytes(karate.samples.shape[1], 34, 256)[0] == 0    # auto: LDS, no workspace
    got = both_forms(karate, 34)
    assert (got["counts"][:, 0] <= 34).all() and (got["counts"][:, 0] < karate.host[4][:, 0]).any()
    auto = check(run(karate, 34), karate)
    for k in got:
        assert np.array_equal(auto[k], got[k]), k


SYNTH = {
    # every position the same id: every lane contends for one slot; several tiles, several positions per LDS thread
    "all equal": lambda rs: ([np.full(3000, 12345)] * 2, 8, 2, None, 1 << 20),
    # n_unique == n == cap_nodes = 3/4 of the table: the highest load factor
    "all distinct": lambda rs: ([rs.permutation(1 << 16)[:3072], rs.permutation(1 << 16)[:3072]], 64, 2, 3072, 1 << 16),
    "duplicate seeds": lambda rs: ([np.concatenate([[0, 0, 1, 0], rs.integers(0, 6, 40)]), np.array([0, 0, 1, 0])], 4, 2, None, 6),
    "no hops": lambda rs: ([np.array([3, 9, 3, 3, 1]), np.array([7, 7, 7, 7, 7])], 5, 0, None, 10),
    "a batch without edges": lambda rs: ([rs.integers(0, 9, 200), rs.integers(0, 9, 6), np.zeros(0, dtype=np.int64)], 6, 2, None, 9),
    # 37 seeds, [3, 2]: 370 slots; ragged counts that are no multiple of 64 or of the workgroup
    "ragged": lambda rs: ([rs.integers(0, 150, n) for n in (370, 37, 65, 129, 263, 1, 300, 191)], 37, 2, 370, 150),
    # ragged over several tiles of the flat form and several positions per thread of the LDS form
    "ragged tiles": lambda rs: ([rs.integers(0, 2000, n) for n in (5000, 1023, 1024, 1025, 4097, 2049, 3)], 3, 3, 5000, 2000),
    # ids near 2^40: 64-bit keys
    "wide ids": lambda rs: ([(1 << 40) - rs.integers(0, 700, n) * 3 for n in (2500, 1, 777)], 16, 2, None, 1 << 41),
}


@pytest.mark.parametrize("case", list(SYNTH))
def test_synthetic_slabs_both_forms(case):
    batches, n_seeds, n_hops, cap_nodes, id_bound = SYNTH[case](np.random.default_rng(3))
    slabs = synthetic(batches, n_seeds, n_hops, cap_nodes, seed=4)
    got = both_forms(slabs, id_bound)
    if case == "all equal":
        assert got["counts"][:, 0].tolist() == [1, 1] and (got["inverse"][:, :3000] == 0).all()
    if case == "all distinct":
        assert got["counts"][:, 0].tolist() == [3072, 3072]
    if case == "duplicate seeds":
        assert got["nodes"][1, :2].tolist() == [0, 1] and got["layer_nodes"][1, 0] == 2      # the unique seeds lead
    if case == "wide ids":                               # the same ids under 32-bit keys would collide: they differ above 2^32
        assert got["nodes"][0, 0] > 1 << 39


def test_cap_nodes_at_the_lds_bound_and_one_above():
    """Auto takes the LDS form up to the bound the form query reports for this device, the flat form one slot above."""
    from tch_geometric import _cabi
    rs = np.random.default_rng(8)
    bound = _cabi.ns_homo_unique_form(1, 1 << 24)[2]
    assert bound >= 3072
    for cap, want in ((bound, 1), (bound + 1, 2)):
        assert _cabi.ns_homo_unique_form(cap, 1 << 24)[0] == want
        total, least = _cabi.ns_homo_unique_workspace_bytes(cap, 1 << 24, 2)
        assert total == (0 if want == 1 else 2 * least)
        slabs = synthetic([rs.integers(0, 3 * cap, cap), rs.integers(0, cap // 4, cap - 77)], 128, 2, cap, seed=cap)
        res = _cabi.NsUniqueOut(slabs)
        si, su = slabs.struct(), res.unique_struct()
        rc = _cabi.lib.tg_ns_homo_unique(C.byref(si), C.c_int64(2), C.c_int64(128), C.c_int32(2), C.c_int64(1 << 24),
                                         C.byref(su), None, C.c_int64(0), C.c_int32(0), _cabi.stream_ptr(torch.device(DEV)))
        assert rc == (0 if want == 1 else 1)             # without a workspace only the LDS form runs
        if want == 2:
            assert "workspace too small" in _cabi.lib.tg_last_error().decode()
        torch.cuda.synchronize()
        check(run(slabs, 1 << 24), slabs)


def test_rmat16_loader_shape_full_workspace_and_round_by_round(rmat16):
    """8 x 1 024 seeds, [15, 10]: up to 169 984 positions per batch, 166 scan tiles, tables in the workspace -- once with all
    eight tables at once, once with bytes_min (eight rounds of one table), once with room for three (rounds of 3, 3, 2)."""
    from tch_geometric import _cabi
    cap = rmat16.samples.shape[1]
    assert cap == 169984 and _cabi.ns_homo_unique_form(cap, 1 << 16)[0] == 2
    total, least = _cabi.ns_homo_unique_workspace_bytes(cap, 1 << 16, 8)
    assert total == 8 * least
    full = check(run(rmat16, 1 << 16, ws=torch.empty(total // 8, dtype=torch.int64, device=DEV)), rmat16)
    assert (full["counts"][:, 0] < rmat16.host[4][:, 0]).all()               # a skewed graph: duplicates in every batch
    for words in (least // 8, 3 * least // 8 + 5):
        part = host(run(rmat16, 1 << 16, ws=torch.empty(words, dtype=torch.int64, device=DEV)))
        for k in full:
            assert np.array_equal(part[k], full[k]), (words, k)
    some = check(run(rmat16, 1 << 16, n_batches=5), rmat16, n_batches=5)      # fewer batches than the slabs hold
    assert np.array_equal(some["nodes"][:5], full["nodes"][:5])


@pytest.mark.parametrize("which,form", [("karate", 1), ("karate", 2), ("rmat16", 2)])
def test_in_place_equals_out_of_place(karate, rmat16, which, form):
    slabs = {"karate": karate, "rmat16": rmat16}[which]
    id_bound = 1 << 16
    apart = host(run(slabs, id_bound, form=form))
    mine = slabs.clone()
    res = run(mine, id_bound, form=form, in_place=True)
    assert res.rows.data_ptr() == mine.rows.data_ptr() and res.cols.data_ptr() == mine.cols.data_ptr()
    together = check(res, slabs)
    for k in apart:
        assert np.array_equal(apart[k], together[k]), k


def test_unique_view_goes_into_compact(karate):
    """The tg_ns_out view of the result (samples = nodes, relabelled rows / cols, unique counts) is what tg_ns_homo_compact
    flattens."""
    from tch_geometric import _cabi
    res = run(karate, 34)
    got = host(res)
    counts = res.counts.cpu()
    n_id, rows, cols, _ = _cabi.ns_homo_compact(res, 256, counts)
    torch.cuda.synchronize()
    want_n = np.concatenate([got["nodes"][b, :counts[b, 0]] for b in range(256)])
    want_r = np.concatenate([got["rows"][b, :counts[b, 1]] for b in range(256)])
    want_c = np.concatenate([got["cols"][b, :counts[b, 1]] for b in range(256)])
    assert np.array_equal(n_id.cpu().numpy(), want_n)
    assert np.array_equal(rows.cpu().numpy(), want_r) and np.array_equal(cols.cpu().numpy(), want_c)


def test_transform_on_device_tensors(rmat16):
    """transforms.unique_nodes on one call's device tensors: the same entry point, one batch."""
    from tch_geometric.transforms import unique_nodes
    S, R, Cc, _, counts = rmat16.host
    n, m = counts[0]
    dev = lambda a: torch.from_numpy(a.copy()).to(DEV)
    nodes, inverse, rows_u, cols_u, _ = unique_rule(S[0, :n], R[0, :m], Cc[0, :m])
    for id_bound in (None, 1 << 16):
        got = unique_nodes(dev(S[0, :n]), dev(R[0, :m]), dev(Cc[0, :m]), id_bound=id_bound)
        for g, w in zip(got, (nodes, rows_u, cols_u, inverse)):
            assert np.array_equal(g.cpu().numpy(), w)
    got = unique_nodes(dev(np.array([4, 4, 2])), dev(np.zeros(0, dtype=np.int64)), dev(np.zeros(0, dtype=np.int64)))
    assert [g.tolist() for g in got] == [[4, 2], [], [], [0, 0, 1]]


def test_loader_unique_against_the_forest_loader():
    """Two loaders with the same seed over the fakedataset graph with x and an edge attribute, prefetch 4, a ragged last
    mini-batch: unique=True hands out the rule applied to what unique=False hands out, for two epochs."""
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
    forest, unique = NeighborLoader(g, [6, 5], **kw), NeighborLoader(g, [6, 5], unique=True, **kw)
    assert len(unique) == 8 and not forest.unique and unique.unique
    for epoch in range(2):
        seen = 0
        for j, (f, u) in enumerate(zip(forest, unique)):
            s, e = f.n_id.cpu().numpy(), f.edge_index.cpu().numpy()
            starts = [lo[0] for lo in f.layer_offsets]
            w_nodes, _, w_rows, w_cols, w_layers = unique_rule(s, e[0], e[1], starts)
            n_id = u.n_id.cpu().numpy()
            assert np.array_equal(n_id, w_nodes) and u.num_nodes == w_nodes.size < f.num_nodes
            assert np.array_equal(u.edge_index.cpu().numpy(), np.stack([w_rows, w_cols])) and u.num_edges == f.num_edges
            assert u.layer_nodes == w_layers and f.layer_nodes is None
            assert u.batch_size == w_layers[0] == np.unique(s[:f.batch_size]).size <= f.batch_size
            assert np.array_equal(u.x.cpu().numpy(), x[n_id])
            assert torch.equal(u.e_id, f.e_id) and torch.equal(u.edge_attr, f.edge_attr)
            assert u.call_id == f.call_id == 100 + epoch * 8 + j and u.layer_offsets == f.layer_offsets
            seen += 1
        assert seen == 8
    assert unique._unique_ws is None or unique._unique_ws.numel() > 0
    assert len(unique._pool) == 1 and "uniq" in unique._pool[0][0]    # the second epoch reused the slabs
