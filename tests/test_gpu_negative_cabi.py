"""tg_neg_sample (csrc/negative.hip) at the C ABI, at the seam between its two rank paths, word for word against the CPU
oracle under orc.rng_philox(seed, call_id).

ranks_of runs one workgroup for an item range of at most 16 384 and flag kernel + library scan + total kernel above it.
Every call here goes through helpers_negative.run_neg: the test owns every buffer, each has exactly the capacity the
header promises between guard words, the workspace is exactly the queried bytes, and nothing outside n_samples / n_edges
may be written.  helpers_negative.check_semantics, which does not know the oracle, runs on every result as well.  Each
case names, in its comment, the defect it would catch."""
import numpy as np
import pytest
import torch

import helpers_negative as hn
import orc

pytestmark = pytest.mark.gpu
SEED = 0x5EA3
ONE_WORKGROUP = 16384                    # negative.hip ranks_of: the largest range neg_rank1_kernel takes


@pytest.fixture(scope="module")
def cabi():
    from tch_geometric import _cabi
    return _cabi


@pytest.fixture(scope="module")
def tg():
    import tch_geometric
    return tch_geometric


def _check(cabi, spec, call_id, want=None, ws_shift=0):
    want = want if want is not None else hn.oracle(spec, SEED, call_id)
    got = hn.run_neg(cabi, spec, SEED, call_id, ws_shift=ws_shift)
    hn.assert_equal(got, want)
    hn.check_semantics(spec, got)
    return got


# ------------------------------------------------------------------------------------------------ homogeneous
N = 1 << 12
HOMO_SHAPES = [(16383, 1),   # the last range of one workgroup: its last chunk is ragged (16 383 = 255 x 64 + 63)
               (16384, 1),   # exactly the limit, still one workgroup: rank[end] is the word past the last whole chunk
               (16385, 1),   # the first device-wide range: one item in the last scan block, total = rank[e - 1] + flag[e - 1]
               (4096, 4),    # the limit reached through num_neg: rows = item / num_neg on the one-workgroup path
               (2341, 7),    # 16 387 items, num_neg no power of two: item -> (row, negative) on the device-wide path
               (4097, 4)]    # 16 388: a last row of four items alone past the limit


@pytest.fixture(scope="module")
def homo_graph():
    row, col = orc.rmat_edges(12, N * 16, 21)
    ptrs, idx, _ = orc.to_csr(np.stack([row, col]), N)
    return ptrs, idx


def _homo_spec(graph, n_inputs, num_neg, node_count, tries):
    inputs = orc.seed_batches(2, 0, 1, n_inputs, 64)[0]                   # 64 distinct values: every slot but 64 is a duplicate
    return hn.NegSpec(1, [(0, 0, graph[0], graph[1], node_count)], [inputs], num_neg, tries, homogeneous=True)


_call_ids = {}


def _call_id(*key):
    return _call_ids.setdefault(key, 100 + len(_call_ids))


def test_the_homogeneous_cases_exercise_what_they_claim(homo_graph):
    """On the oracle alone, over the node_count = n cases: cols into (duplicated) inputs test the last-slot rule, first
    sights test the ranks, rejected items (an RMAT hub among 64 inputs is adjacent to much of the graph) test that an item
    without a negative takes no rank."""
    into_inputs = first_sights = rejected = 0
    for n_inputs, num_neg in HOMO_SHAPES:
        for tries in (1, 4):
            o = hn.oracle(_homo_spec(homo_graph, n_inputs, num_neg, N, tries), SEED, _call_id(n_inputs, num_neg, N, tries))
            into_inputs += int((o["cols"][0] < n_inputs).sum())
            first_sights += o["samples"][0].size - n_inputs
            rejected += n_inputs * num_neg - o["rows"][0].size
    assert into_inputs >= 1000 and first_sights >= 1000 and rejected > 0


@pytest.mark.parametrize("tries", [1, 4])
@pytest.mark.parametrize("node_count", [N,    # most negatives are first sights: the rank of every first sight matters
                                        50,   # few distinct negatives: almost every item repeats an id, min position per id
                                        1])   # one candidate: rejected wherever the input is 0 or adjacent to 0
@pytest.mark.parametrize("n_inputs,num_neg", HOMO_SHAPES)
def test_homogeneous_at_the_rank_seam(cabi, homo_graph, n_inputs, num_neg, node_count, tries):
    spec = _homo_spec(homo_graph, n_inputs, num_neg, node_count, tries)
    assert (spec.items > ONE_WORKGROUP) == (n_inputs * num_neg > 16384)
    _check(cabi, spec, _call_id(n_inputs, num_neg, node_count, tries))


def test_workspace_base_240_bytes_past_a_256_byte_boundary(cabi, homo_graph):
    """The scan storage is aligned up from wherever flag + m ends: with the base 16 bytes short of a boundary the round-up
    is at its longest for this layout, and the exact workspace must still hold it."""
    spec = _homo_spec(homo_graph, 4097, 4, N, 4)
    _check(cabi, spec, _call_id(4097, 4, N, 4), ws_shift=240)


def test_the_surface_returns_the_c_abi_result(cabi, tg, homo_graph):
    """The operator adds a word of slack to every buffer; the exact-capacity call must give the same words."""
    spec = _homo_spec(homo_graph, 2341, 7, N, 4)
    P, I = torch.from_numpy(homo_graph[0]).cuda(), torch.from_numpy(homo_graph[1]).cuda()
    tg.seed(SEED)
    call = tg.rng_state()[1]
    s, r, c, sc = tg.negative_sample_neighbors_homogenous(P, I, (N, N), torch.from_numpy(spec.inputs[0]).cuda(), 7, 4)
    got = hn.run_neg(cabi, spec, SEED, call)
    assert sc == 2341
    hn.assert_equal(dict(samples=[s.cpu().numpy()], rows=[r.cpu().numpy()], cols=[c.cpu().numpy()], panic=0), got)


@pytest.mark.parametrize("what", ["num_neg = 0", "try_count = 0", "n_inputs = 0"])
def test_degenerate_calls_on_exact_buffers(cabi, homo_graph, what):
    """No items (rows and cols of capacity 0, samples of exactly n_inputs) or no tries: the inputs are copied, the counts
    are written, and nothing else is."""
    n_inputs, num_neg, tries = {"num_neg = 0": (300, 0, 4), "try_count = 0": (300, 3, 0), "n_inputs = 0": (0, 3, 4)}[what]
    spec = _homo_spec(homo_graph, n_inputs, num_neg, N, tries)
    got = _check(cabi, spec, 7)
    assert got["samples"][0].size == n_inputs and got["rows"][0].size == 0


def test_workspace_query_laws_on_the_device(cabi):
    hn.check_workspace_law(cabi)


# ------------------------------------------------------------------------------------------------ heterogeneous
SIZES = [3000, 3000, 2000]                               # A, B, C
PATTERN = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 2), (2, 2)]   # A-A, A-B, A-C, B-A, B-C, C-C: dst <= src everywhere


def _random_rel(key, s, d, deg=12):
    rng = np.random.default_rng([0x4E47, key])
    row = np.repeat(np.arange(SIZES[s], dtype=np.int64), deg)
    ptrs, idx, _ = orc.to_csr(np.stack([row, rng.integers(0, SIZES[d], row.size)]), (SIZES[s], SIZES[d]))
    return ptrs, idx


@pytest.fixture(scope="module")
def het_base():
    """A 6 000, B 5 500, C 100 inputs from the lowest tenth of each range, 3 negatives: item ranges of 18 000 (device-wide
    from b = 0), 16 500 (device-wide from b = 18 000) and 300 (one workgroup from b = 34 500) in one call."""
    rng = np.random.default_rng(0x4E48)
    rels = [(s, d) + _random_rel(k, s, d) + (SIZES[d],) for k, (s, d) in enumerate(PATTERN)]
    inputs = [rng.integers(0, SIZES[t] // 10, n) for t, n in enumerate((6000, 5500, 100))]
    return hn.NegSpec(3, rels, inputs, 3, 4)


def _variant(base, name):
    ins = list(base.inputs)
    none, empty = None, np.zeros(0, dtype=np.int64)
    if name == "inbound":
        return base.replace(inbound=True)
    if name == "C absent":
        ins[2] = none
    elif name == "C empty":
        ins[2] = empty
    elif name == "A absent":
        ins[0] = none
    elif name == "A absent, C empty":
        ins[0], ins[2] = none, empty
    return base.replace(inputs=ins)


HET_VARIANTS = ["outbound",            # flags at begin + i, scanned from flag + b into erank + b; A-A, A-B, A-C share erank
                "inbound",             # has_edge(w, v): the row is the candidate
                "C absent",            # n_inputs < 0: no items, no input map, every sample of C a first sight
                "C empty",             # n_inputs = 0 must do what n_inputs < 0 does
                "A absent",            # the first range is empty: b = 0 now belongs to B, and m = 16 800
                "A absent, C empty"]   # 0 beside < 0; A and C receive only first sights


@pytest.mark.parametrize("name", HET_VARIANTS)
def test_heterogeneous_ranges_on_both_rank_paths(cabi, het_base, name):
    spec = _variant(het_base, name)
    want = hn.oracle(spec, SEED, 40 + HET_VARIANTS.index(name))
    ranges = [spec.item_range(t) for t in range(3)]
    wide = [e - b > ONE_WORKGROUP for b, e in ranges]
    if name in ("outbound", "inbound"):
        assert ranges == [(0, 18000), (18000, 34500), (34500, 34800)] and wide == [True, True, False]
    assert any(w and b > 0 for w, (b, e) in zip(wide, ranges)) or name.startswith("A absent")
    for r, (s, d, _, _, _) in enumerate(spec.rels):       # every relation is drawn and keeps pairs
        assert (want["rows"][r].size > 0) == (spec.n_in(s) > 0), r
    for t in range(3):          # every type that items reach receives first sights, and cols into its inputs if it has any
        n_in = spec.n_in(t)     # (with A absent nothing reaches B: A-B is its only way in)
        reached = any(d == t and spec.n_in(s) > 0 for s, d, _, _, _ in spec.rels)
        assert reached or name.startswith("A absent")
        assert (want["samples"][t].size > n_in) == reached
        into = sum(int((want["cols"][r] < n_in).sum()) for r, rel in enumerate(spec.rels) if rel[1] == t)
        assert (into > 0) == (reached and n_in > 0)
    _check(cabi, spec, 40 + HET_VARIANTS.index(name), want=want)


def test_the_surface_returns_the_c_abi_result_heterogeneous(cabi, tg, het_base):
    names = ["A", "B", "C"]
    ets = [(names[s], "r%d" % k, names[d]) for k, (s, d, _, _, _) in enumerate(het_base.rels)]
    keys = ["%s__%s__%s" % et for et in ets]
    P = {k: torch.from_numpy(rel[2]).cuda() for k, rel in zip(keys, het_base.rels)}
    I = {k: torch.from_numpy(rel[3]).cuda() for k, rel in zip(keys, het_base.rels)}
    S = {k: (SIZES[rel[0]], rel[4]) for k, rel in zip(keys, het_base.rels)}
    ins = {n: torch.from_numpy(x).cuda() for n, x in zip(names, het_base.inputs)}
    tg.seed(SEED)
    call = tg.rng_state()[1]
    s, r, c, sc = tg.negative_sample_neighbors_heterogenous(names, ets, P, I, S, ins, 3, 4, False)
    got = hn.run_neg(cabi, het_base, SEED, call)
    assert sc == {"A": 6000, "B": 5500, "C": 100}
    surface = dict(samples=[s[n].cpu().numpy() for n in names], rows=[r[k].cpu().numpy() for k in keys],
                   cols=[c[k].cpu().numpy() for k in keys], panic=0)
    hn.assert_equal(surface, got)


def test_inbound_panic_on_the_device_wide_path(cabi, het_base):
    """One relation A-C whose node range (4 000) exceeds the CSR's 3 000 rows, 6 000 x 3 items: has_edge(w, v) would index
    ptrs[w] past the end, where the reference panics.  The flag must be raised without that read, copied out behind the
    device-wide ranks, and the call must still stay inside its buffers."""
    s, d, ptrs, idx, _ = het_base.rels[2]
    spec = hn.NegSpec(3, [(s, d, ptrs, idx, 4000)], [het_base.inputs[0], None, None], 3, 4, inbound=True)
    assert spec.items == 18000 > ONE_WORKGROUP and ptrs.size - 1 == 3000
    with pytest.raises(RuntimeError, match="panic"):
        hn.oracle(spec, SEED, 60)
    assert hn.run_neg(cabi, spec, SEED, 60)["panic"] == 1
    fits = hn.NegSpec(3, [(s, d, ptrs, idx, 3000)], [het_base.inputs[0], None, None], 3, 4, inbound=True)
    assert _check(cabi, fits, 60)["panic"] == 0           # candidates up to the last row: no panic, and the oracle's words


def test_a_full_relation_table(cabi):
    """NEG_MAX_RELS = 32 relations out of one source type into four destination types, 200 inputs x 5: the relation draw
    over 32 entries, rel[31] of the table, and 32 edge-rank passes over one item range that share erank."""
    sizes = [400, 300, 200, 100]                          # the source type is a destination too: cols into its inputs
    rng = np.random.default_rng(0x4E49)
    rels = []
    for k in range(32):
        d = k % 4
        row = np.repeat(np.arange(sizes[0], dtype=np.int64), 3)
        ptrs, idx, _ = orc.to_csr(np.stack([row, rng.integers(0, sizes[d], row.size)]), (sizes[0], sizes[d]))
        rels.append((0, d, ptrs, idx, sizes[d]))
    spec = hn.NegSpec(4, rels, [rng.integers(0, 40, 200), None, np.zeros(0, dtype=np.int64), None], 5, 4)
    got = _check(cabi, spec, 70)
    assert sum(1 for r in got["rows"] if r.size) >= 30    # 1 000 items over 32 relations: the draw reaches the whole table


def test_refusals_leave_the_buffers_alone(cabi, het_base):
    """A type with inputs and no outgoing relation (the reference panics on an empty range), and a table of 33."""
    s, d, ptrs, idx, nc = het_base.rels[1]                # A-B only: B has inputs and nowhere to go
    spec = hn.NegSpec(3, [(s, d, ptrs, idx, nc)], [het_base.inputs[0][:50], het_base.inputs[1][:50], None], 3, 4)
    assert "no outgoing relation" in hn.run_neg(cabi, spec, SEED, 80, expect_rc=1)
    spec = hn.NegSpec(3, [(s, d, ptrs, idx, nc)] * 33, [het_base.inputs[0][:50], None, None], 3, 4)
    assert "33 relations" in hn.run_neg(cabi, spec, SEED, 80, expect_rc=1)
