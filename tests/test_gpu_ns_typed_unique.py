"""tg_ns_typed_unique on the device: per-batch, per-type node dedup and relabel of the typed slabs, word for word against
the NumPy statement of the rule (helpers_unique.unique_rule applied per type, the relations relabelled through the two
inverses here), under the LDS form and the flat form, with every output slab pre-filled with a sentinel so that words
past the counts are seen to be untouched; HeteroNeighborLoader(unique=True); transforms.unique_nodes_hetero."""
import numpy as np
import pytest
import torch

from helpers import load_fake_hetero, rel_key
from helpers_unique import unique_rule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7                                               # no id, no position, no count
LDS = 160 * 1024
REL = ((0, 1), (1, 0), (2, 2), (0, 2))                  # 0->1, 1->0, a self-relation, 0->2


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV)


class TypedSlabs:
    """Input slabs of tg_ns_typed_unique with NsHeteroBatched's field names, written by the test or copied from a sampler.
    samples: [T] arrays [nb, pitch]; rows / cols: [R]; counts [nb, stride]."""

    def __init__(self, samples, rows, cols, counts, rel, n_inputs):
        self.T, self.R, self.nb = len(samples), len(rows), counts.shape[0]
        self.rel_src, self.rel_dst, self.n_inputs = [s for s, _ in rel], [d for _, d in rel], list(n_inputs)
        self.samples, self.rows, self.cols = [dev(x) for x in samples], [dev(x) for x in rows], [dev(x) for x in cols]
        self.edge_index = [torch.full_like(x, SENT) for x in self.rows]
        self.counts = dev(counts)
        self.host = ([np.array(x, dtype=np.int64) for x in samples], [np.array(x, dtype=np.int64) for x in rows],
                     [np.array(x, dtype=np.int64) for x in cols], np.array(counts, dtype=np.int64))
        self.rel = tuple(rel)

    def clone(self):
        return TypedSlabs(*self.host, self.rel, self.n_inputs)


def synthetic(ids, n_edges, rel, n_inputs, pitch_nodes=None, pitch_edges=None, tail=0, seed=0):
    """Slabs from ids[b][t] (a batch's list of type t) and n_edges[b][r]: rows / cols are random positions of the source /
    destination list, everything past the counts holds the sentinel, `tail` extra words close every counts row."""
    rs = np.random.default_rng(seed)
    nb, T, R = len(ids), len(ids[0]), len(rel)
    pn = pitch_nodes or [max(max(len(ids[b][t]) for b in range(nb)), 1) for t in range(T)]
    pe = pitch_edges or [max(max(n_edges[b][r] for b in range(nb)), 1) for r in range(R)]
    S = [np.full((nb, p), SENT, dtype=np.int64) for p in pn]
    Rw, Cl = [np.full((nb, p), SENT, dtype=np.int64) for p in pe], [np.full((nb, p), SENT, dtype=np.int64) for p in pe]
    counts = np.full((nb, T + R + tail), SENT, dtype=np.int64)
    for b in range(nb):
        for t in range(T):
            S[t][b, :len(ids[b][t])] = ids[b][t]
            counts[b, t] = len(ids[b][t])
        for r, (s, d) in enumerate(rel):
            m = n_edges[b][r]
            assert m == 0 or (len(ids[b][s]) and len(ids[b][d]))
            Rw[r][b, :m] = rs.integers(0, max(len(ids[b][s]), 1), m)
            Cl[r][b, :m] = rs.integers(0, max(len(ids[b][d]), 1), m)
            counts[b, T + r] = m
    return TypedSlabs(S, Rw, Cl, counts, rel, n_inputs)


def run(slabs, id_bounds, form=0, ws=None, in_place=False, with_inverse=True, n_batches=None):
    """One call with sentinel-filled outputs -> the NsTypedUniqueOut, synchronised."""
    from tch_geometric import _cabi
    res = _cabi.NsTypedUniqueOut(slabs, in_place=in_place, with_inverse=with_inverse)
    for t in res.nodes + (res.inverse or []) + [res.state] + ([] if in_place else res.rows + res.cols):
        t.fill_(SENT)
    _cabi.ns_typed_unique(slabs, slabs.nb if n_batches is None else n_batches, id_bounds, form=form, ws=ws, result=res)
    torch.cuda.synchronize()
    return res


def host(res):
    got = {k: [x.cpu().numpy() for x in getattr(res, k)] for k in ("nodes", "rows", "cols")}
    got["inverse"] = [x.cpu().numpy() for x in res.inverse] if res.inverse is not None else None
    got["counts"], got["seed_counts"] = (x.numpy() for x in res.read_state())
    return got


def check(res, slabs, n_batches=None):
    """Every output word of every batch against the rule; the words past n_unique / n / m, the tail words of a counts row
    and the batches not asked for still hold the sentinel."""
    S, Rw, Cl, counts = slabs.host
    got = host(res)
    T, R = slabs.T, slabs.R
    nb = slabs.nb if n_batches is None else n_batches
    for b in range(nb):
        inv = []
        for t in range(T):
            n = counts[b, t]
            nodes, inverse, _, _, _ = unique_rule(S[t][b, :n], [], [])
            inv.append(inverse)
            u = nodes.size
            assert got["counts"][b, t] == u, (b, t, got["counts"][b], u)
            assert np.array_equal(got["nodes"][t][b, :u], nodes) and (got["nodes"][t][b, u:] == SENT).all(), (b, t)
            if got["inverse"] is not None:
                assert np.array_equal(got["inverse"][t][b, :n], inverse) and (got["inverse"][t][b, n:] == SENT).all(), (b, t)
            seeds = S[t][b, :min(max(slabs.n_inputs[t], 0), n)]
            assert got["seed_counts"][b, t] == np.unique(seeds).size, (b, t)
        for r, (s, d) in enumerate(slabs.rel):
            m = counts[b, T + r]
            assert got["counts"][b, T + r] == m
            assert np.array_equal(got["rows"][r][b, :m], inv[s][Rw[r][b, :m]]), (b, r)
            assert np.array_equal(got["cols"][r][b, :m], inv[d][Cl[r][b, :m]]), (b, r)
            assert (got["rows"][r][b, m:] == SENT).all() and (got["cols"][r][b, m:] == SENT).all(), (b, r)
        assert (got["counts"][b, T + R:] == SENT).all(), b                    # the tail words of the row
    for k in ("nodes", "rows", "cols", "inverse"):                            # batches the call was not asked for
        for x in got[k] or []:
            assert (x[nb:] == SENT).all(), k
    assert (got["counts"][nb:] == SENT).all() and (got["seed_counts"][nb:] == SENT).all()
    assert all((x.cpu().numpy() == SENT).all() for x in res.edge_index)       # edge_index is never touched
    return got


def same(a, b):
    for k in a:
        if isinstance(a[k], list):
            assert len(a[k]) == len(b[k]) and all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), k
        elif a[k] is not None and b[k] is not None:
            assert np.array_equal(a[k], b[k]), k


def both_forms(slabs, id_bounds, **kw):
    """Form 1 and form 2 against the rule, and against each other."""
    a, b = check(run(slabs, id_bounds, form=1, **kw), slabs), check(run(slabs, id_bounds, form=2, **kw), slabs)
    same(a, b)
    return a


def six_batches():
    rs = np.random.default_rng(5)
    pn, pe = [50, 37, 70], [40, 33, 64, 20]
    ids = [
        [[], [], []],                                                                            # an empty batch
        [rs.integers(0, 20, 31), [], rs.integers(0, 9, 44)],                                     # a type with 0 nodes
        [rs.integers(0, 30, 50), rs.integers(0, 12, 37), rs.integers(0, 1000, 70)],              # every type at its pitch
        [np.concatenate([[3, 3, 5, 3], rs.integers(0, 8, 20)]), rs.integers(0, 5, 9), np.concatenate([[9, 9], rs.integers(0, 40, 30)])],
        [rs.integers(0, 20, 17), rs.integers(0, 20, 5), np.full(61, 12345)],                     # all-equal ids in one type
        [rs.integers(0, 20, 33), rs.integers(0, 20, 21), rs.integers(0, 20, 13)],                # a relation without edges
    ]
    n_edges = [[0, 0, 0, 0], [0, 0, 64, 20], pe, [25, 9, 30, 11], [40, 33, 60, 1], [17, 20, 31, 0]]
    return synthetic(ids, n_edges, REL, n_inputs=[4, 0, 2], pitch_nodes=pn, pitch_edges=pe, tail=3, seed=6)


@pytest.mark.parametrize("with_inverse", [True, False])
def test_six_batches_both_forms_in_and_out_of_place(with_inverse):
    """T = 3, R = 4 (0->1, 1->0, a self-relation, 0->2), counts rows of T + R + 3 words whose tail stays untouched."""
    slabs = six_batches()
    assert slabs.counts.shape[1] == 3 + 4 + 3
    bounds = [1 << 20] * 3
    apart = both_forms(slabs, bounds, with_inverse=with_inverse)
    assert apart["counts"][0, :7].tolist() == [0] * 7 and apart["counts"][4, 2] == 1 and apart["counts"][1, 1] == 0
    assert apart["nodes"][0][3, :2].tolist() == [3, 5] and apart["seed_counts"][3].tolist() == [2, 0, 1]
    if with_inverse:
        assert (apart["inverse"][2][4, :61] == 0).all()
    for form in (1, 2):
        mine = slabs.clone()
        res = run(mine, bounds, form=form, in_place=True, with_inverse=with_inverse)
        assert all(x.data_ptr() == y.data_ptr() for x, y in zip(res.rows + res.cols, mine.rows + mine.cols))
        same(apart, check(res, slabs))


def test_tile_edges_of_the_flat_form():
    """One type with exactly 1 024, 1 025 and 2 500 positions (a tile is 1 024), ids drawn from 300 distinct values."""
    rs = np.random.default_rng(9)
    ids = [[rs.integers(0, 50, 10), rs.integers(0, 300, n), rs.integers(0, 50, 70)] for n in (1024, 1025, 2500)]
    slabs = synthetic(ids, [[100, 100, 90, 33]] * 3, REL, n_inputs=[4, 1030, 0], seed=1)
    got = check(run(slabs, [50, 300, 50], form=2), slabs)
    assert (got["counts"][:, 1] <= 300).all() and got["counts"][2, 1] > 250
    same(got, check(run(slabs, [50, 300, 50], form=1), slabs))


def test_64_bit_keys_on_one_type():
    """id_bound = 2^40 on one type with ids above 2^32 that collide under 32-bit keys; the other types stay 32-bit."""
    rs = np.random.default_rng(10)
    wide = lambda n: (1 << 32) * rs.integers(1, 200, n) + 77
    ids = [[rs.integers(0, 90, 200), wide(1500), rs.integers(0, 40, 64)], [rs.integers(0, 90, 3), wide(1), []]]
    slabs = synthetic(ids, [[300, 300, 10, 50], [5, 5, 0, 0]], REL, n_inputs=[8, 0, 0], seed=2)
    got = both_forms(slabs, [90, 1 << 40, 40])
    assert got["nodes"][1][0, 0] > 1 << 32 and 100 < got["counts"][0, 1] < 200


def test_pitches_at_the_lds_bound_and_one_above():
    """(12 288, q, 500): the largest type's table is 128 KiB, so q decides whether the u16 words of all types still fit
    160 KiB.  Auto takes the LDS form at the last q that fits and the flat form one word further."""
    from tch_geometric import _cabi
    bounds = [1 << 24] * 3
    fits = lambda q: _cabi.ns_typed_unique_form([12288, q, 500], bounds, LDS)[0] == 1
    lo, hi = 0, 1 << 15
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    assert 3000 < lo < 3600                              # 160 KiB - 128 KiB - 256 B = 16 256 u16 words for 12 288 + q + 504
    rs = np.random.default_rng(12)
    for q, want in ((lo, 1), (hi, 2)):
        pitches = [12288, q, 500]
        assert _cabi.ns_typed_unique_form(pitches, bounds)[0] == want          # the device's own limit agrees
        total, least = _cabi.ns_typed_unique_workspace_bytes(pitches, bounds, 2)
        assert total == (0 if want == 1 else 2 * least)
        ids = [[rs.integers(0, 40000, 12288), rs.integers(0, 900, q), rs.integers(0, 1 << 24, 500)],
               [rs.integers(0, 3000, 12288 - 77), rs.integers(0, 1 << 24, q - 5), rs.integers(0, 9, 321)]]
        slabs = synthetic(ids, [[5000, 3000, 700, 2000], [4999, 17, 1, 0]], REL, n_inputs=[128, 0, 0], seed=q)
        check(run(slabs, bounds), slabs)


def test_flat_form_round_by_round_and_on_some_batches():
    """The flat form with a workspace of exactly bytes_min (five rounds of one batch), with room for all, with room for
    two and a bit; and on 3 of 5 batches only, the others' slabs keeping the sentinel."""
    from tch_geometric import _cabi
    rs = np.random.default_rng(13)
    ids = [[rs.integers(0, 500, rs.integers(1, 3000)), rs.integers(0, 100, rs.integers(1, 1200)), rs.integers(0, 2000, rs.integers(1, 700))]
           for _ in range(5)]
    slabs = synthetic(ids, [[900, 400, 300, 1100]] * 5, REL, n_inputs=[16, 0, 0], pitch_nodes=[3000, 1200, 700], tail=2, seed=3)
    bounds = [500, 100, 2000]
    least = _cabi.ns_typed_unique_workspace_bytes([3000, 1200, 700], bounds, 5)[1]
    ws = lambda nbytes: torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    full = check(run(slabs, bounds, form=2, ws=ws(5 * least)), slabs)
    for nbytes in (least, 2 * least + 40):
        same(full, check(run(slabs, bounds, form=2, ws=ws(nbytes)), slabs))
    some = check(run(slabs, bounds, form=2, ws=ws(2 * least), n_batches=3), slabs, n_batches=3)
    assert np.array_equal(some["nodes"][0][:3], full["nodes"][0][:3])
    with pytest.raises(_cabi.TchGeoError, match="workspace too small"):
        run(slabs, bounds, form=2, ws=ws(least - 8))


@pytest.fixture(scope="module")
def fake():
    """The fakehetero fixture ingested as CSC, every relation."""
    from tch_geometric import _cabi
    counts, edges = load_fake_hetero()
    node_types, edge_types = sorted(counts), sorted(edges)
    tix = {t: i for i, t in enumerate(node_types)}
    P, I = {}, {}
    for et in edge_types:
        e = torch.from_numpy(edges[et]).to(DEV)
        P[rel_key(et)], I[rel_key(et)], _ = _cabi.coo_to_csx(e[0].contiguous(), e[1].contiguous(), counts[et[0]], counts[et[2]], True)
    return counts, edges, node_types, edge_types, tix, P, I


def test_real_sampler_output_both_forms(fake):
    """tg_ns_hetero_batched, 64 batches x 4 seeds of v0, fan-out [4, 3]: the forest's tails overwritten with the sentinel,
    both forms against the rule, and every relabelled edge still joining the ids it joined."""
    from tch_geometric import _cabi
    counts, _, node_types, edge_types, tix, P, I = fake
    assert "v0" in tix
    rels = [(tix[et[0]], tix[et[2]], P[rel_key(et)], I[rel_key(et)], [4, 3]) for et in edge_types]
    seeds = _cabi.seed_batches(21, 0, 64, 4, counts["v0"], DEV)
    hb = _cabi.NsHeteroBatched(len(node_types), rels, [seeds if t == "v0" else None for t in node_types], 2, 64, DEV)
    hb.run(3, 0)
    torch.cuda.synchronize()
    T, R = hb.T, hb.R
    c = hb.counts.cpu().numpy()
    S, Rw, Cl = ([x.cpu().numpy() for x in xs] for xs in (hb.samples, hb.rows, hb.cols))
    for b in range(64):
        for t in range(T):
            S[t][b, c[b, t]:] = SENT
        for r in range(R):
            Rw[r][b, c[b, T + r]:] = SENT
            Cl[r][b, c[b, T + r]:] = SENT
    slabs = TypedSlabs(S, Rw, Cl, c, [(r[0], r[1]) for r in rels], [4 if t == "v0" else 0 for t in node_types])
    got = both_forms(slabs, [counts[t] for t in node_types])
    assert c[:, T:].sum() > 64 * 4 and (got["counts"][:, :T] < c[:, :T]).any()           # edges were sampled, nodes repeat
    same(got, check(run(slabs, [counts[t] for t in node_types]), slabs))      # auto
    for r, (s, d) in enumerate(slabs.rel):
        for b in range(64):
            m = c[b, T + r]
            assert np.array_equal(got["nodes"][s][b][got["rows"][r][b, :m]], S[s][b][Rw[r][b, :m]]), (r, b)
            assert np.array_equal(got["nodes"][d][b][got["cols"][r][b, :m]], S[d][b][Cl[r][b, :m]]), (r, b)


def test_loader_unique_against_the_forest_loader(fake):
    """Two loaders with the same seed and call ids over the fixture with an x per type (row i holds i) and an edge
    attribute, batch 4, prefetch 8, 30 inputs with repeats (7 full mini-batches and a ragged one of 2)."""
    from tch_geometric.loader import HeteroNeighborLoader
    from tch_geometric.transforms import HeteroGraph
    counts, edges, node_types, edge_types, _, _, _ = fake
    rs = np.random.default_rng(14)
    data = HeteroGraph()
    for nt in node_types:
        data[nt].num_nodes = counts[nt]
        data[nt].x = torch.arange(counts[nt], dtype=torch.float32, device=DEV).view(-1, 1).repeat(1, 3)
    for et in edge_types:
        data[et].edge_index = torch.from_numpy(edges[et]).to(DEV)
        data[et].edge_attr = torch.from_numpy(rs.standard_normal((edges[et].shape[1], 2)).astype(np.float32)).to(DEV)
    nodes = rs.integers(0, counts["v0"], 30)
    nodes[[1, 6, 7, 29]] = nodes[[0, 4, 4, 28]]                                # repeated seeds inside mini-batches 0, 1 and 7
    kw = dict(input_type="v0", input_nodes=torch.from_numpy(nodes), batch_size=4, prefetch=8, seed=9, call_id0=50)
    forest, unique = HeteroNeighborLoader(data, [4, 3], **kw), HeteroNeighborLoader(data, [4, 3], unique=True, **kw)
    assert len(unique) == 8 and not forest.unique and unique.unique
    seen = shrunk = 0
    for j, (f, u) in enumerate(zip(forest, unique)):
        n_f, n_u = {}, {}
        for nt in node_types:
            n_f[nt], n_u[nt] = f[nt].n_id.cpu().numpy(), u[nt].n_id.cpu().numpy()
            assert np.unique(n_u[nt]).size == n_u[nt].size == u[nt].num_nodes
            assert np.array_equal(n_u[nt], unique_rule(n_f[nt], [], [])[0])   # first-occurrence order of the forest's n_id
            assert np.array_equal(u[nt].x.cpu().numpy()[:, 0], n_u[nt].astype(np.float32)) and u[nt].x.shape == (n_u[nt].size, 3)
            shrunk += n_u[nt].size < n_f[nt].size
        for et in edge_types:
            ei_f, ei_u = f[et].edge_index.cpu().numpy(), u[et].edge_index.cpu().numpy()
            assert ei_f.shape == ei_u.shape
            assert np.array_equal(n_u[et[0]][ei_u[0]], n_f[et[0]][ei_f[0]])
            assert np.array_equal(n_u[et[2]][ei_u[1]], n_f[et[2]][ei_f[1]])
            assert torch.equal(u[et].e_id, f[et].e_id) and torch.equal(u[et].edge_attr, f[et].edge_attr)
            assert u[et].layer_offsets == f[et].layer_offsets
        mine = nodes[4 * j:4 * j + 4]
        assert f["v0"].batch_size == mine.size and u["v0"].batch_size == np.unique(mine).size
        assert np.array_equal(n_u["v0"][:u["v0"].batch_size], unique_rule(mine, [], [])[0])  # the distinct seeds lead, in order
        assert u.call_id == f.call_id == 50 + j
        seen += 1
    assert seen == 8 and shrunk > 0
    assert u["v0"].batch_size == 1 and f["v0"].batch_size == 2                # the ragged last mini-batch: one seed twice


def test_transform_on_device_tensors_against_its_cpu_path(fake):
    """transforms.unique_nodes_hetero on one call's dicts from the operator surface: the device path (a single-batch
    launch) equals the torch implementation on the same tensors."""
    import tch_geometric as tg
    from tch_geometric.transforms import unique_nodes_hetero
    counts, _, node_types, edge_types, _, P, I = fake
    tg.seed(5)
    seeds = torch.from_numpy(np.random.default_rng(15).integers(0, counts["v0"], 16)).to(DEV)
    nn = {rel_key(et): [4, 3] for et in edge_types}
    s, r, c, _, _ = tg.neighbor_sampling_heterogenous(node_types, edge_types, P, I, {"v0": seeds}, nn, 2)
    cpu = lambda d: {k: v.cpu() for k, v in d.items()}
    want = unique_nodes_hetero(cpu(s), cpu(r), cpu(c), edge_types)
    assert sum(v.numel() for v in r.values()) > 16
    for num_nodes in (None, counts):
        got = unique_nodes_hetero(s, r, c, edge_types, num_nodes=num_nodes)
        for g, w in zip(got, want):
            assert list(g) == list(w)
            for k in w:
                assert g[k].is_cuda and torch.equal(g[k].cpu(), w[k]), k
    nodes, rows_u, cols_u, inverse = got
    for et in edge_types:
        k = rel_key(et)
        assert torch.equal(nodes[et[0]][rows_u[k]], s[et[0]][r[k]]) and torch.equal(nodes[et[2]][cols_u[k]], s[et[2]][c[k]])


def test_transform_gives_minus_one_for_an_end_outside_its_list_on_both_paths():
    """An end that is negative or past ITS type's list (also where the other type's list is longer, or empty) gives -1:
    the device path and the torch path of unique_nodes_hetero agree on it."""
    from tch_geometric.transforms import unique_nodes_hetero
    i64 = lambda v: torch.tensor(v, dtype=torch.int64)
    samples = {"a": i64([9, 4, 9, 7, 4]), "b": i64([3, 3]), "c": i64([])}
    edge_types = [("a", "to", "b"), ("b", "to", "c"), ("a", "self", "a")]
    rows = {"a__to__b": i64([0, -1, 4, 5, 2]), "b__to__c": i64([1, 2, -3]), "a__self__a": i64([4, 1 << 40, 3])}
    cols = {"a__to__b": i64([1, 0, 2, 0, -1]), "b__to__c": i64([0, 0, 0]), "a__self__a": i64([-1, 0, 5])}
    want = unique_nodes_hetero(samples, rows, cols, edge_types)
    assert want[1]["a__to__b"].tolist() == [0, -1, 1, -1, 0] and want[2]["b__to__c"].tolist() == [-1, -1, -1]
    dev = lambda d: {k: v.to(DEV) for k, v in d.items()}
    got = unique_nodes_hetero(dev(samples), dev(rows), dev(cols), edge_types)
    for g, w in zip(got, want):
        assert list(g) == list(w)
        for k in w:
            assert g[k].is_cuda and torch.equal(g[k].cpu(), w[k]), k


@pytest.mark.parametrize("prefetch", [1, 2])
def test_loader_unique_over_many_full_launches_and_a_ragged_one(fake, prefetch):
    """The loader keeps the dedup's outputs from one full launch to the next: 30 inputs at batch 4 make several full
    launches (and, at prefetch 1, a ragged launch as long as a full one but narrower) over two epochs, every mini-batch
    against the forest loader's."""
    from tch_geometric.loader import HeteroNeighborLoader
    from tch_geometric.transforms import HeteroGraph
    counts, edges, node_types, edge_types, _, _, _ = fake
    data = HeteroGraph()
    for nt in node_types:
        data[nt].num_nodes = counts[nt]
    for et in edge_types:
        data[et].edge_index = torch.from_numpy(edges[et]).to(DEV)
    nodes = np.random.default_rng(16).integers(0, counts["v0"], 30)
    kw = dict(input_type="v0", input_nodes=torch.from_numpy(nodes), batch_size=4, prefetch=prefetch, seed=2, call_id0=7)
    forest, unique = HeteroNeighborLoader(data, [4, 3], **kw), HeteroNeighborLoader(data, [4, 3], unique=True, **kw)
    seen = 0
    for _ in range(2):
        for j, (f, u) in enumerate(zip(forest, unique)):
            n_u = {}
            for nt in node_types:
                n_u[nt] = u[nt].n_id.cpu().numpy()
                assert np.array_equal(n_u[nt], unique_rule(f[nt].n_id.cpu().numpy(), [], [])[0]), (j, nt)
            for et in edge_types:
                ei_f, ei_u = f[et].edge_index.cpu().numpy(), u[et].edge_index.cpu().numpy()
                assert np.array_equal(n_u[et[0]][ei_u[0]], f[et[0]].n_id.cpu().numpy()[ei_f[0]]), (j, et)
                assert np.array_equal(n_u[et[2]][ei_u[1]], f[et[2]].n_id.cpu().numpy()[ei_f[1]]), (j, et)
            assert u["v0"].batch_size == np.unique(nodes[4 * j:4 * j + 4]).size and u.call_id == f.call_id
            seen += 1
    assert seen == 16 and unique._unique_out is not None and unique._unique_out.nb == prefetch
