"""tg_ns_homo_unique_grouped on the device: per-batch, per-group node dedup and relabel of hand-built forest slabs, word for
word against the NumPy statement of the rule (helpers_disjoint.disjoint_rule) -- both forms, both key widths, a workspace
of bytes_min (rounds) and of bytes, in place and apart, optional outputs null or given, the null map against an explicit
identity, every slab pre-filled with a sentinel so that words past the counts are seen to be untouched.  Every batch keeps
the forest contract (a parent sits before its child, at most n_hops parents to a seed)."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers_disjoint import disjoint_rule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7                                               # no id, no position, no count, no group
COUNTS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)     # 64: a wave; 1 024: NSU_TILE and the LDS form's workgroup
FIELDS = ("nodes", "group", "inverse", "rows", "cols", "counts", "layer_nodes")


def forest(rs, n, n_seeds, n_hops, id_range, empty_from=None):
    """One batch of n positions: min(n, n_seeds) seeds, the others spread over the hops (none from hop `empty_from` on; a
    live hop gets at least one while any are left), every position of hop h with a parent among hop h - 1's, ids drawn
    from [0, id_range).  -> (samples, cols, layer_starts)."""
    seeds = min(n, n_seeds)
    live = n_hops if empty_from is None else empty_from
    extra = n - seeds
    assert extra == 0 or live > 0
    sizes = np.zeros(n_hops, dtype=np.int64)
    if extra:
        base = min(live, extra)
        sizes[:base] = 1
        for x in rs.integers(0, base, extra - base):
            sizes[x] += 1
    cols, starts, prev = [], [], np.arange(seeds)
    for h in range(n_hops):
        starts.append(seeds + len(cols))
        k = int(sizes[h])
        cur = seeds + len(cols) + np.arange(k)
        cols.extend(rs.choice(prev, k).tolist() if k else [])
        prev = cur
    assert seeds + len(cols) == n
    return rs.integers(0, id_range, n), np.array(cols, dtype=np.int64), starts


class Slabs:
    """Input slabs with NsBatchedOut's field names from per-batch (samples, cols, layer_starts)."""

    def __init__(self, batches, n_seeds, n_hops, cap_nodes=None):
        from tch_geometric import _cabi
        nb = len(batches)
        cap_nodes = cap_nodes or max(max(len(b[0]) for b in batches), n_seeds, 1)
        cap_edges = max(cap_nodes - n_seeds, 1)
        S, R, Cc = (np.full((nb, c), SENT, dtype=np.int64) for c in (cap_nodes, cap_edges, cap_edges))
        lo, counts = np.zeros((nb, max(n_hops, 1), 3), dtype=np.int64), np.zeros((nb, 2), dtype=np.int64)
        for b, (s, cols, starts) in enumerate(batches):
            n, m = len(s), len(cols)
            S[b, :n], R[b, :m], Cc[b, :m] = s, n_seeds + np.arange(m), cols
            counts[b] = (n, m)
            for h in range(n_hops):
                lo[b, h] = (starts[h], max(starts[h] - n_seeds, 0), starts[h])
        self.host = (S, R, Cc, lo, counts)
        self.batches, self.n_batches, self.n_seeds, self.n_hops = batches, nb, n_seeds, n_hops
        self.upload()
        self.struct = lambda: _cabi.NsBatchedOut.struct(self)

    def upload(self):
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        S, R, Cc, lo, counts = self.host
        self.samples, self.rows, self.cols, self.layer_offsets, self.counts = dev(S), dev(R), dev(Cc), dev(lo), dev(counts)
        self.edge_index, self.states = torch.full_like(self.rows, SENT), None


def run(slabs, id_bound, seed_group=None, n_groups=None, form=0, ws="bytes", in_place=False, inverse=True, layers=True):
    """One call through the C ABI with sentinel-filled outputs -> {field: host array}; ws: "bytes" (all batches at once),
    "min" (exactly bytes_min: one batch per round) or None."""
    from tch_geometric import _cabi
    if in_place:
        slabs.upload()                                   # an earlier in-place call relabelled the slabs
    res = _cabi.NsUniqueOut(slabs, in_place=in_place, with_group=True)
    for t in (res.nodes, res.group, res.inverse, res.counts, res.layer_nodes) + (() if in_place else (res.rows, res.cols)):
        t.fill_(SENT)
    n_groups = slabs.n_seeds if n_groups is None else n_groups
    sg = None if seed_group is None else torch.from_numpy(np.asarray(seed_group, dtype=np.int32)).to(DEV)
    cap = slabs.samples.shape[1]
    total, least = _cabi.ns_homo_unique_grouped_workspace_bytes(cap, id_bound, n_groups, slabs.n_batches)
    words = {"bytes": least * slabs.n_batches, "min": least, None: 0}[ws] // 8
    wst = torch.empty(words, dtype=torch.int64, device=DEV) if words else None
    si, su = slabs.struct(), res.grouped_struct()
    if not inverse:
        su.inverse = None
    if not layers:
        su.layer_nodes = None
    _cabi.check(_cabi.lib.tg_ns_homo_unique_grouped(
        C.byref(si), C.c_int64(slabs.n_batches), C.c_int64(slabs.n_seeds), C.c_int32(slabs.n_hops), C.c_int64(id_bound),
        _cabi.ptr(sg), C.c_int64(n_groups), C.byref(su), _cabi.ptr(wst), C.c_int64(words * 8), C.c_int32(form),
        _cabi.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    got = {k: getattr(res, k).cpu().numpy() for k in FIELDS}
    got["edge_index"] = slabs.edge_index.cpu().numpy()
    if in_place:
        assert res.rows.data_ptr() == slabs.rows.data_ptr() and res.cols.data_ptr() == slabs.cols.data_ptr()
        slabs.upload()
    return got


def check(got, slabs, seed_group=None, inverse=True, layers=True):
    """Every output word of every batch against the rule; the words past n_unique / n / m still hold the sentinel."""
    for b, (s, cols, starts) in enumerate(slabs.batches):
        n, m = len(s), len(cols)
        nodes, group, inv, rows_u, cols_u, layer_nodes = disjoint_rule(s, slabs.n_seeds + np.arange(m), cols, slabs.n_seeds,
                                                                       seed_group, starts)
        u = nodes.size
        assert got["counts"][b].tolist() == [u, m], (b, got["counts"][b], u, m)
        assert np.array_equal(got["nodes"][b, :u], nodes) and np.array_equal(got["group"][b, :u], group), b
        assert np.array_equal(got["rows"][b, :m], rows_u) and np.array_equal(got["cols"][b, :m], cols_u), b
        assert (got["nodes"][b, u:] == SENT).all() and (got["group"][b, u:] == SENT).all(), b
        assert (got["rows"][b, m:] == SENT).all() and (got["cols"][b, m:] == SENT).all(), b
        if inverse:
            assert np.array_equal(got["inverse"][b, :n], inv) and (got["inverse"][b, n:] == SENT).all(), b
        if layers:
            assert got["layer_nodes"][b].tolist() == layer_nodes, (b, got["layer_nodes"][b], layer_nodes)
    if not inverse:
        assert (got["inverse"] == SENT).all()
    if not layers:
        assert (got["layer_nodes"] == SENT).all()
    assert (got["edge_index"] == SENT).all()                              # edge_index is not touched
    return got


def equal(a, b):
    for k in FIELDS:
        assert np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def nine():
    """Per hop count one launch of nine batches, one per node count of COUNTS, ids drawn from a range a quarter of the count
    wide (duplicates inside a group and across groups in every batch), eight seeds in four groups."""
    rs = np.random.default_rng(21)
    out = {}
    for n_hops in (1, 3):
        out[n_hops] = Slabs([forest(rs, n, 8, n_hops, n // 4 + 2) for n in COUNTS], 8, n_hops)
    # no hops: every position is a seed, so the seed row is as wide as the largest count
    out[0] = Slabs([forest(rs, n, 2049, 0, n // 4 + 2) for n in COUNTS], 2049, 0)
    return out


MAP8 = [0, 1, 1, 2, 3, 0, 2, 2]                         # seeds 1, 2 and 3, 6, 7 share a group


@pytest.mark.parametrize("n_hops", [0, 1, 3])
@pytest.mark.parametrize("form", [1, 2])
def test_nine_counts_every_hop_count_both_forms(nine, n_hops, form):
    slabs = nine[n_hops]
    if n_hops:
        sg, ng = MAP8, 4
    else:
        sg, ng = (np.arange(2049) * 7 % 300).tolist(), 300
    got = check(run(slabs, 1 << 10, sg, ng, form=form), slabs, sg)
    merged = [int(got["counts"][b, 0]) < n for b, n in enumerate(COUNTS)]
    assert any(merged) and not merged[0] and not merged[1]
    apart = check(run(slabs, 1 << 10, form=form), slabs, None)                # the identity: one group per seed
    assert (apart["counts"][:, 0] >= got["counts"][:, 0]).all() and (apart["counts"][2:, 0] > got["counts"][2:, 0]).any()


@pytest.mark.parametrize("form", [1, 2])
def test_null_map_equals_explicit_identity_and_forms_agree(nine, form):
    slabs = nine[3]
    null = run(slabs, 1 << 10, form=form)
    equal(null, run(slabs, 1 << 10, list(range(8)), 8, form=form))
    equal(null, run(slabs, 1 << 10, form=3 - form))
    equal(null, run(slabs, 1 << 10, form=0, ws="bytes"))


@pytest.mark.parametrize("form", [1, 2])
def test_wide_keys(nine, form):
    """id_bound = 2^31 with 8 groups: the pair no longer fits 32 bits.  Ids sit just below 2^31, so a key that lost its high
    word would merge groups."""
    from tch_geometric import _cabi
    rs = np.random.default_rng(22)
    top = (1 << 31) - 1
    batches = [(top - s, c, st) for s, c, st in (forest(rs, n, 8, 3, 40) for n in (65, 1025, 2049))]
    slabs = Slabs(batches, 8, 3)
    assert _cabi.ns_homo_unique_grouped_form(2049, 1 << 31, 8, 160 * 1024)[1] > \
        _cabi.ns_homo_unique_grouped_form(2049, 1 << 28, 8, 160 * 1024)[1]     # 64-bit slots
    wide = check(run(slabs, 1 << 31, form=form), slabs)
    assert (wide["counts"][:, 0] > 40).all()                                  # more entries than distinct ids: groups kept apart
    narrow = Slabs([(s - top + 39, c, st) for s, c, st in batches], 8, 3)     # the same forest, ids in [0, 40): 32-bit keys
    small = check(run(narrow, 40, form=form), narrow)
    for k in ("group", "inverse", "rows", "cols", "counts", "layer_nodes"):
        assert np.array_equal(wide[k], small[k]), k


@pytest.mark.parametrize("ws", ["min", "bytes"])
@pytest.mark.parametrize("in_place", [False, True])
def test_flat_workspace_rounds_and_in_place(nine, ws, in_place):
    slabs = nine[3]
    want = run(slabs, 1 << 10, MAP8, 4, form=1)
    got = check(run(slabs, 1 << 10, MAP8, 4, form=2, ws=ws, in_place=in_place), slabs, MAP8)
    equal(want, got)


@pytest.mark.parametrize("form", [1, 2])
def test_in_place_lds_and_optional_outputs(nine, form):
    slabs = nine[1]
    full = check(run(slabs, 1 << 10, MAP8, 4, form=form, in_place=form == 1), slabs, MAP8)
    for inverse, layers in ((False, True), (True, False), (False, False)):
        part = check(run(slabs, 1 << 10, MAP8, 4, form=form, inverse=inverse, layers=layers), slabs, MAP8, inverse, layers)
        for k in ("nodes", "group", "rows", "cols", "counts"):
            assert np.array_equal(part[k], full[k]), k


def test_three_batches_of_different_counts_and_an_empty_middle_hop():
    """One launch: a batch of seeds only, one whose hops 1 and 2 are empty, one with every hop filled."""
    rs = np.random.default_rng(23)
    batches = [forest(rs, 4, 4, 3, 3), forest(rs, 700, 4, 3, 60, empty_from=1), forest(rs, 1500, 4, 3, 90)]
    assert batches[1][2][1] == batches[1][2][2] == 700                        # hops 1 and 2 start at the end
    slabs = Slabs(batches, 4, 3)
    for sg, ng in ((None, None), ([1, 0, 1, 0], 2)):
        a = check(run(slabs, 90, sg, ng, form=1), slabs, sg)
        equal(a, check(run(slabs, 90, sg, ng, form=2, ws="min"), slabs, sg))
        assert a["layer_nodes"][1, 1] == a["layer_nodes"][1, 2] == a["counts"][1, 0]


def test_placed_duplicates():
    """2 049 distinct ids under two seeds, then duplicates placed by hand: inside one group they merge onto the FIRST
    position whatever tile or lane it sits in, across groups they stay apart, and two seeds of one group with one id
    (src_j == dst_j) are one entry."""
    rs = np.random.default_rng(24)
    n, n_seeds = 2049, 2
    s = rs.permutation(1 << 12)[:n] + 10
    cols = np.concatenate([np.arange(n - n_seeds) % 2])                        # position p hangs on seed p % 2: one hop
    cols = cols.astype(np.int64)
    s[[4, 1500, 2048]] = 1                                                   # even positions: all under seed 0
    s[[1023, 1025]] = 2                                                      # odd: under seed 1, across the tile boundary
    s[[1024, 1027]] = 3                                                      # 1 024 under seed 0, 1 027 under seed 1
    s[[2047, 6]] = 4                                                         # 2 047 (tile 1) under seed 1, 6 (tile 0) under seed 0
    s[[0, 1]] = 5                                                            # the two seeds carry one id
    slabs = Slabs([(s, cols, [2])], n_seeds, 1)
    for form in (1, 2):
        apart = check(run(slabs, 1 << 13, form=form), slabs)
        inv, grp, nodes = apart["inverse"][0], apart["group"][0], apart["nodes"][0]
        assert inv[4] == inv[1500] == inv[2048] == 4 and inv[1023] == inv[1025] and inv[1024] != inv[1027]
        assert inv[2047] != inv[6] and grp[inv[2047]] == 1 and grp[inv[6]] == 0
        assert nodes[:2].tolist() == [5, 5] and grp[:2].tolist() == [0, 1] and apart["counts"][0, 0] == n - 3
        one = check(run(slabs, 1 << 13, [0, 0], 1, form=form), slabs, [0, 0])
        inv = one["inverse"][0]
        assert inv[0] == inv[1] == 0 and inv[1024] == inv[1027] and inv[2047] == inv[6] == 5
        assert one["layer_nodes"][0, 0] == 1 and one["counts"][0, 0] == n - 3 - 3


def run_plain(slabs, id_bound, form):
    """tg_ns_homo_unique on the same slabs, outputs sentinel-filled as run()'s -> {field: host array} (no group)."""
    from tch_geometric import _cabi
    res = _cabi.NsUniqueOut(slabs)
    for t in (res.nodes, res.inverse, res.rows, res.cols, res.counts, res.layer_nodes):
        t.fill_(SENT)
    _cabi.ns_homo_unique(slabs, slabs.n_batches, id_bound, form=form, result=res)
    torch.cuda.synchronize()
    return {k: getattr(res, k).cpu().numpy() for k in FIELDS if k != "group"}


def test_one_group_equals_the_plain_dedup():
    """The two operators are the two instantiations of one set of kernel templates: with every seed in ONE group the pair
    key is the id, so tg_ns_homo_unique_grouped must give tg_ns_homo_unique's words -- both forms, both key widths.  Node
    counts around the flat form's tile (NSU_TILE = 1 024) and up to five positions per thread of the LDS form."""
    rs = np.random.default_rng(26)
    counts = (3, 1023, 1024, 1025, 2049, 4097)
    batches = [forest(rs, n, 8, 3, max(n // 4, 1)) for n in counts]
    up = (1 << 33) - (1 << 10)                                                # ids just below 2^33: 64-bit keys
    for id_bound, slabs in ((1 << 10, Slabs(batches, 8, 3)), (1 << 33, Slabs([(s + up, c, st) for s, c, st in batches], 8, 3))):
        for form in (1, 2):
            plain = run_plain(slabs, id_bound, form)
            one = run(slabs, id_bound, [0] * 8, 1, form=form)
            for k in plain:
                assert np.array_equal(plain[k], one[k]), (id_bound, form, k)
            for b, (s, cols, _) in enumerate(slabs.batches):
                n, m, u = len(s), len(cols), int(plain["counts"][b, 0])
                assert 0 < u <= max(n // 4, 1) and plain["counts"][b, 1] == m
                assert (one["group"][b, :u] == 0).all() and (one["group"][b, u:] == SENT).all(), (id_bound, form, b)
                assert (plain["nodes"][b, u:] == SENT).all() and (plain["inverse"][b, n:] == SENT).all(), (id_bound, form, b)
                assert (plain["rows"][b, m:] == SENT).all() and (plain["cols"][b, m:] == SENT).all(), (id_bound, form, b)


def test_wrapper_and_transform():
    """_cabi.ns_homo_unique_grouped allocates what it needs; transforms.unique_nodes(seed_group=...) on device tensors gives
    the five-tuple, and stays the four-tuple without the map."""
    from tch_geometric import _cabi
    from tch_geometric.transforms import unique_nodes
    rs = np.random.default_rng(25)
    s, cols, starts = forest(rs, 1500, 6, 2, 200)
    slabs = Slabs([(s, cols, starts)], 6, 2)
    sg = np.array([0, 1, 0, 2, 2, 1])
    nodes, group, inv, rows_u, cols_u, layers = disjoint_rule(s, 6 + np.arange(cols.size), cols, 6, sg, starts)
    for form in (0, 1, 2):
        res = _cabi.ns_homo_unique_grouped(slabs, 1, 200, seed_group=torch.from_numpy(sg.astype(np.int32)).to(DEV), n_groups=3,
                                           form=form)
        torch.cuda.synchronize()
        u = int(res.counts[0, 0])
        assert u == nodes.size and np.array_equal(res.nodes[0, :u].cpu().numpy(), nodes)
        assert np.array_equal(res.group[0, :u].cpu().numpy(), group) and res.layer_nodes[0].tolist() == layers
    with pytest.raises(ValueError):
        _cabi.ns_homo_unique_grouped(slabs, 1, 200, seed_group=torch.zeros(6, dtype=torch.int64, device=DEV), n_groups=3)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64)).to(DEV)
    rows = 6 + np.arange(cols.size)
    for id_bound in (None, 200):
        got = unique_nodes(t(s), t(rows), t(cols), id_bound=id_bound, seed_group=t(sg))
        assert len(got) == 5
        for g, w in zip(got, (nodes, rows_u, cols_u, inv, group)):
            assert np.array_equal(g.cpu().numpy(), w)
    assert len(unique_nodes(t(s), t(rows), t(cols))) == 4
