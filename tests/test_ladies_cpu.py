"""The layer-wise pair (tg_ladies_workspace_bytes / _count / _emit, _cabi_ladies.Ladies, LADIESLoader), host-only parts: the
NumPy restatement against a brute-force dict version, the integer draw on a total above 2^54, unbiasedness and the one-slot
law by enumeration with exact fractions, the power of the GPU law tests against three wrong laws, the workspace formula,
every refusal that comes before a launch, the Python-side ValueErrors, the header under C99 and the exports.  No GPU: every
device pointer handed over is null or an address that is never read."""
import ctypes as C
import itertools
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import exact_laws
import helpers_ladies as hl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tchgeo_ladies.h")
NAMES = ["tg_ladies_workspace_bytes", "tg_ladies_count", "tg_ladies_emit"]


@pytest.fixture(scope="module")
def ops():
    if not os.path.exists(os.path.join(ROOT, "tch-geometric_amd", "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tch-geometric_amd"), "-s"])
    from tch_geometric import _cabi_ladies
    return _cabi_ladies


# ---- the restatement against brute force -------------------------------------------------------------------------------
def random_case(seed):
    rs = np.random.default_rng(seed)
    n = int(rs.integers(3, 40))
    deg = rs.integers(0, 6, n)
    deg[rs.integers(0, n, 3)] = 0                                    # empty columns
    ptrs = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = rs.integers(0, n, int(ptrs[-1])).astype(np.int64)      # self loops and parallel edges happen
    w = (rs.random(indices.size) * 1.5 - 0.25).astype(np.float32)    # some negative, some above 1
    w[rs.integers(0, max(w.size, 1), 4) % max(w.size, 1)] = np.nan if w.size else 0
    return rs, n, ptrs, indices, w


@pytest.mark.parametrize("seed", range(12))
def test_rule_equals_brute_force(seed):
    rs, n, ptrs, indices, w = random_case(seed)
    lists = (rs.permutation(n)[:max(1, n // 2)], rs.integers(0, n, 7), np.arange(n)[::-1], np.zeros(0, np.int64),
             np.array([0, n, -1, 0, n - 1]))                         # distinct, with repeats, all, none, out of range
    for nodes, weights, s in itertools.product(lists, (None, w, np.zeros_like(w)), (1, 5, 64)):
        p = hl.prepare(ptrs, indices, weights, nodes)
        t = hl.draw_t(seed, 7 + s, s, p.S) if p.S else None
        got = hl.finish(p, s, t)
        want = hl.brute_force(ptrs, indices, weights, nodes, s, t)
        assert hl.same(got, want), (seed, nodes, s)
        assert np.array_equal(got["out_nodes"][got["rows"]], indices[got["edge_index"]])
        assert got["chunks"] == hl.chunks_of(ptrs, nodes) and got["m"] == hl.columns(ptrs, nodes)[1].sum()
        if p.S:
            assert int(got["node_count"][np.unique(got["out_nodes"], return_index=True)[1]].sum()) == s
        elif p.cand.size:
            assert got["status"] & 4 and got["rows"].size == 0
        full = hl.ladies_rule(ptrs, indices, weights, nodes, s, seed, 7 + s)
        assert hl.same(full, got)


def test_chained_blocks():
    _, n, ptrs, indices, w = random_case(3)
    b = hl.blocks(ptrs, indices, None, [1, 2], [4, 3], 9, 100)
    assert len(b) == 2 and b[0][1] == 2 and b[1][1] == b[0][0].size
    assert np.array_equal(b[1][0][:b[0][0].size], b[0][0])           # F_1 is the prefix of F_2
    assert b[0][0].size <= 2 + 4 and b[1][0].size <= b[0][0].size + 3   # a layer adds at most its budget
    second = hl.ladies_rule(ptrs, indices, None, b[0][0], 3, 9, 101)    # layer l draws under call id + l
    assert np.array_equal(second["out_nodes"], b[1][0]) and np.array_equal(second["edge_weight"], b[1][5])


# ---- the draw is integer: a total above 2^54 ------------------------------------------------------------------------------------
def test_prefix_and_pick_above_2_54():
    n = 1 << 15                                                      # columns of length 1: W = 2^40 each, S = 2^55
    ptrs = np.arange(n + 1, dtype=np.int64)
    indices = (np.arange(n, dtype=np.int64) * 5 + 1) % n             # distinct sources, not in column order
    p = hl.prepare(ptrs, indices, None, np.arange(n, dtype=np.int64))
    assert p.S == 1 << 55 and p.S > 2 ** 54 and p.cand.size == n
    assert [int(x) for x in p.P[[0, 1, n - 1]]] == [0, 1 << 40, (n - 1) << 40]      # exact: 2^55 - 2^40 is no double... it is,
    odd = hl.prepare(ptrs, indices, None, np.arange(n - 1, dtype=np.int64))         # ... so also a total with 15 set bits
    assert odd.S == (n - 1) << 40
    s = 4096
    for q, cid in ((p, 3), (odd, 4)):
        w = hl.named_draw(11, np.uint64(cid), hl.TAG_LADIES, np.arange(s, dtype=np.uint64), 0, 0)
        lo = [int(a) | int(b) << 32 for a, b in zip(w[0], w[1])]
        t = hl.draw_t(11, cid, s, q.S)
        exact = [x * q.S >> 64 for x in lo]                          # Python integers: the 128-bit product
        assert [int(x) for x in t] == exact
        sel = hl.select(q, t)
        assert sel.tolist() == [x >> 40 for x in exact]
        # the check has power: the same pick through doubles differs in some slot
        assert any(int(float(x) * float(q.S) / 2.0 ** 64) != e for x, e in zip(lo, exact))
    # a total that needs more than 53 bits: weights that make S odd above 2^54
    W = np.array([(1 << 54) + 1, 3, (1 << 54) + 5], dtype=np.uint64)
    fake = hl.Prepared()
    fake.W, fake.P, fake.S = W, np.cumsum(W, dtype=np.uint64) - W, int(W.sum(dtype=np.uint64))
    assert fake.S == (1 << 55) + 9 and float(fake.S) != fake.S
    edges = np.array([0, (1 << 54), (1 << 54) + 1, (1 << 54) + 3, (1 << 54) + 4, fake.S - 1], dtype=np.uint64)
    assert hl.select(fake, edges).tolist() == [0, 0, 1, 1, 2, 2]    # boundaries one apart beyond a double's precision


# ---- unbiasedness and the one-slot law, by enumeration -------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2])
def test_unbiased_by_enumeration(s):
    ptrs, indices, law = hl.nested_graph()
    p = hl.prepare(ptrs, indices, None, np.arange(6, dtype=np.int64))
    W, S = [int(x) for x in p.W], p.S
    assert [Fraction(w, S) for w in W] == law and p.cand.tolist() == list(range(12))
    est = {}                                                         # (column, csc offset) -> the expectation of its weight
    worst = 0.0
    for sel in itertools.product(range(12), repeat=s):
        prob = Fraction(1)
        for u in sel:
            prob *= law[u]
        r = hl.finish(p, s, None, sel=np.array(sel, dtype=np.int64))
        assert int(r["node_count"].sum()) == s
        for row, col, e, w32 in zip(r["rows"].tolist(), r["cols"].tolist(), r["edge_index"].tolist(), r["edge_weight"].tolist()):
            u = int(r["out_nodes"][row])
            c = int(r["node_count"][row])
            exact = Fraction(c * S, s * W[u]) * Fraction(1, hl.NESTED_LENGTHS[col])
            worst = max(worst, abs(w32 / float(exact) - 1.0))
            est[(col, e)] = est.get((col, e), 0) + prob * exact
    for col, d in enumerate(hl.NESTED_LENGTHS):                      # every entry of the row-normalised adjacency: 1 / d
        for e in range(int(ptrs[col]), int(ptrs[col + 1])):
            assert est[(col, e)] == Fraction(1, d)
    assert worst < 2.0 ** -23                                        # float32 of a double within four roundings of exact


def test_one_slot_law_by_enumeration():
    ptrs, indices, law = hl.nested_graph()
    p = hl.prepare(ptrs, indices, None, np.arange(6, dtype=np.int64))
    for u in range(12):                                              # exactly W_u of the S values of t select u
        lo, hi = int(p.P[u]), int(p.P[u]) + int(p.W[u])
        assert hl.select(p, np.array([lo, hi - 1], dtype=np.uint64)).tolist() == [u, u]
        assert hi == (int(p.P[u + 1]) if u < 11 else p.S)
    # t = floor(lo S / 2^64) over all 2^64 words: every t has floor(2^64 / S) or one more of them
    assert Fraction(p.S, 2 ** 64) < Fraction(1, 10 ** 6)
    # the fixed-point law against the real one, sum over columns with d > u of 1 / d^2
    real = [sum(Fraction(1, d * d) for d in hl.NESTED_LENGTHS if d > u) for u in range(12)]
    real = [x / sum(real) for x in real]
    assert max(abs(float(a - b)) for a, b in zip(law, real)) < 1.3e-11


def test_law_tests_have_power():
    _, _, law = hl.nested_graph()
    N = 1 << 16
    law = np.array([float(x) for x in law])
    d = hl.NESTED_LENGTHS
    uniform = np.full(12, 1 / 12)
    linear = np.array([sum(1.0 / x for x in d if x > u) for u in range(12)])
    entries = np.array([sum(1.0 for x in d if x > u) for u in range(12)])
    for wrong in (uniform, linear / linear.sum(), entries / entries.sum()):
        assert exact_laws.power(wrong, law, N) >= 0.999
    assert (law * N).min() >= 195


# ---- exports, the header and the workspace formula -----------------------------------------------------------------------------
def test_header_is_c99():
    src = "#include \"tchgeo_ladies.h\"\nint main(void) { tg_ladies_in in; in.n_samples = TG_LADIES_MAX_SAMPLES; return (int)in.n_samples - 8192 + (TG_TAG_LADIES != 18u); }\n"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    "-x", "c", "-"], input=src.encode(), check=True)


def test_exports_equal_the_header(ops):
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"TG_API\s+[\w\s\*]+?\b(tg_\w+)\s*\(", text)
    assert sorted(declared) == sorted(ops.EXPORTS) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(ops.lib, name) and getattr(ops.lib, name).argtypes
    assert [f for f, _ in ops.TgLadiesIn._fields_] == ["nodes", "node_ptr", "max_nodes", "node_cap", "chunk_cap", "n_samples",
                                                       "weights", "call_stride"]
    assert "#define TG_TAG_LADIES 18u" in text and ops.TG_TAG_LADIES == hl.TAG_LADIES == 18
    assert ops.LADIES_MAX_SAMPLES == hl.MAX_SAMPLES == 8192 and ops.LADIES_MAX_NODES == hl.MAX_NODES == 1 << 22
    main = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tchgeo.h")).read(), flags=re.S)
    used = set(int(x) for x in re.findall(r"#define TG_TAG_\w+ (\d+)u", main))
    assert 18 not in used and max(used) == 17                       # the first number no tag uses


def graph(ops, n_major=100, n_edges=1000, ptrs=0x10000, indices=0x10000):
    from tch_geometric import _cabi
    g = _cabi.TgGraph()
    g.ptrs, g.indices, g.n_major, g.n_edges = ptrs, indices, n_major, n_edges
    return g


def test_workspace_formula(ops):
    q = ops.ladies_workspace_bytes
    for E, mx, cap, cc in ((0, 0, 0, 0), (1000, 1, 1, 0), (40000, 37, 900, 0), (511, 1024, 1024, 0), (512, 1025, 5000, 3),
                           (513, 3, 3, 1), (1 << 28, 1024, 1 << 20, 0), (1 << 33, 1 << 20, 1 << 30, 1 << 31)):
        for bound in (100, 1 << 31, (1 << 31) + 1):
            for s in (1, 64, 65, 8192):
                per = hl.workspace_bytes(E, mx, cap, cc, bound, s)
                assert q(graph(ops, n_edges=E), bound, mx, cap, cc, s, 7) == (7 * per, per)
                assert q(graph(ops, n_edges=E), bound, mx, cap, cc, s, 0) == (0, per)
    g = graph(ops)
    sizes = [q(g, 100, 10, cap, 5, 9, 1)[1] for cap in (10, 100, 1000, 10000, 1 << 20)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]                                     # monotone in node_cap
    sizes = [q(g, 100, 10, 10, cc, 9, 1)[1] for cc in (1, 100, 10000, 1 << 20, 1 << 31)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]                                     # and in chunk_cap
    narrow, wide = q(g, 1 << 31, 10, 3000, 5, 9, 1)[1], q(g, (1 << 31) + 1, 10, 3000, 5, 9, 1)[1]
    assert hl.table_slots(3000) == 4096 and wide - narrow == 4 * 4096


# ---- refusals before any launch ------------------------------------------------------------------------------------------------
FAKE = 0x10000          # a non-null address that is never read: every call below is refused before anything is launched
BIG = 1 << 40           # a workspace size no shape below needs


def call(ops, which, g="default", s="default", rng="default", G=2, bound=100, ws=FAKE, ws_bytes=BIG, **kw):
    from tch_geometric import _cabi
    g = graph(ops, **{k: kw.pop(k) for k in ("n_major", "ptrs", "indices") if k in kw}) if g == "default" else g
    if s == "default":
        s = ops.TgLadiesIn(kw.pop("nodes", FAKE), kw.pop("node_ptr", FAKE), kw.pop("mx", 4), kw.pop("cap", 8), kw.pop("cc", 0),
                           kw.pop("ns", 16), kw.pop("weights", None), 0)
    rng = _cabi.TgRng(1, 2) if rng == "default" else rng
    p = C.c_void_p
    gp, sp, rp = ((C.byref(x) if x is not None else None) for x in (g, s, rng))
    if which == "count":
        out = [p(kw.pop(k, FAKE)) for k in ("n_nodes", "n_edges", "n_cand", "total", "chunks", "status")]
        assert not kw
        return ops.lib.tg_ladies_count(gp, sp, rp, C.c_int64(G), C.c_int64(bound), *out, p(ws), C.c_int64(ws_bytes), None)
    out = [p(kw.pop(k, FAKE)) for k in ("node_off", "edge_off", "nodes_out", "node_count", "node_weight", "rows", "cols",
                                        "eidx", "ew")]
    assert not kw
    return ops.lib.tg_ladies_emit(gp, sp, rp, C.c_int64(G), C.c_int64(bound), *out, p(ws), C.c_int64(ws_bytes), None)


COMMON = [
    (dict(g=None), "null argument"),
    (dict(s=None), "null argument"),
    (dict(rng=None), "null rng"),
    (dict(G=-1), "n_batches"),
    (dict(G=1 << 31), "n_batches"),
    (dict(n_major=-1), "negative graph size"),
    (dict(mx=-1), "max_nodes"),
    (dict(mx=(1 << 22) + 1, cap=1 << 23), "max_nodes"),
    (dict(cap=3), "node_cap"),
    (dict(cap=(1 << 30) + 1), "node_cap"),
    (dict(ns=0), "n_samples"),
    (dict(ns=8193), "n_samples"),
    (dict(cc=(1 << 31) + 1), "chunk_cap"),
    (dict(bound=0), "id_bound"),
    (dict(bound=99), "below n_major"),
    (dict(ws_bytes=-1), "negative"),
    (dict(ws=None), "workspace too small"),
    (dict(ws_bytes=2 * hl.workspace_bytes(1000, 4, 8, 0, 100, 16) - 1), "workspace too small"),
    (dict(ws=FAKE + 4), "8-byte aligned"),
    (dict(ptrs=None), "null ptrs"),
    (dict(indices=None), "null ptrs"),
    (dict(node_ptr=None), "null node_ptr"),
    (dict(nodes=None), "null nodes"),
]


def test_the_short_workspace_of_the_table_above_is_one_byte_short(ops):
    assert ops.ladies_workspace_bytes(graph(ops), 100, 4, 8, 0, 16, 2)[0] == 2 * hl.workspace_bytes(1000, 4, 8, 0, 100, 16)
    for which in ("count", "emit"):
        assert call(ops, which, G=0, ws_bytes=0) == 0                # nothing to launch


@pytest.mark.parametrize("kw, word", COMMON + [(dict([(k, None)]), "null n_nodes") for k in ("n_nodes", "n_edges", "n_cand", "total", "status")])
def test_count_refusals(ops, kw, word):
    assert call(ops, "count", **kw) == 1                             # TG_ERR_INVALID
    assert re.search(word, ops.lib.tg_last_error().decode()), ops.lib.tg_last_error()


@pytest.mark.parametrize("kw, word", COMMON + [(dict([(k, None)]), "null edge_off") for k in ("edge_off", "rows", "cols", "eidx", "ew")]
                         + [(dict(node_off=None), "without node_off")])
def test_emit_refusals(ops, kw, word):
    assert call(ops, "emit", **kw) == 1
    assert re.search(word, ops.lib.tg_last_error().decode()), ops.lib.tg_last_error()


def test_empty_launches(ops):
    assert call(ops, "count", G=0) == 0 and call(ops, "emit", G=0) == 0        # nothing to launch
    assert call(ops, "count", G=0, chunks=None) == 0                           # chunks may be NULL
    assert call(ops, "emit", G=0, nodes_out=None, node_count=None, node_weight=None, node_off=None) == 0
    assert call(ops, "emit", G=0, node_count=None) == 0                        # each per-node output on its own
    assert call(ops, "count", G=0, nodes=None, mx=0, cap=0) == 0               # no lists at max_nodes 0
    assert call(ops, "count", G=0, mx=1 << 22, cap=1 << 22, ns=8192) == 0      # the limits themselves


# ---- the Python-side refusals ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, word", [
    (dict(max_nodes=-1), "max_nodes"),
    (dict(max_nodes=(1 << 22) + 1, node_cap=1 << 23), "max_nodes"),
    (dict(node_cap=3), "node_cap"),
    (dict(node_cap=(1 << 30) + 1), "node_cap"),
    (dict(chunk_cap=(1 << 31) + 1), "chunk_cap"),
    (dict(n_samples=0), "n_samples"),
    (dict(n_samples=8193), "n_samples"),
    (dict(n_batches=-1), "n_batches"),
    (dict(n_batches=1 << 31), "n_batches"),
    (dict(id_bound=99), "id_bound"),
    (dict(weights=torch.zeros(1000, dtype=torch.float64)), "float32"),
    (dict(weights=torch.zeros(999)), "float32"),
])
def test_launch_object_refusals_need_no_device(ops, kw, word):
    args = dict(id_bound=100, max_nodes=4, node_cap=8, chunk_cap=0, n_samples=16, n_batches=2)
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        ops.Ladies(graph(ops), device="cuda:0", **args)
    ops.ladies_status_check(0, "x")
    ops.ladies_status_check(1, "x")                                  # a refused batch is the caller's to answer
    ops.ladies_status_check(4, "x")                                  # nothing to draw from: an empty block, unless asked
    with pytest.raises(RuntimeError, match="outside the graph"):
        ops.ladies_status_check(3, "x")
    with pytest.raises(RuntimeError, match="weight 0"):
        ops.ladies_status_check(4, "x", mask=6)


def _graph(n=5, **attrs):
    from tch_geometric.transforms import Graph
    ei = torch.tensor([[0, 1, 2, 3, 4, 0], [1, 2, 3, 4, 0, 2]])
    return Graph(edge_index=ei, num_nodes=n, **attrs)


@pytest.mark.parametrize("n, kw, err, word", [
    (5, dict(num_samples=[]), ValueError, "at least one layer"),
    (5, dict(num_samples=[4, 0]), ValueError, "num_samples"),
    (5, dict(num_samples=[8193]), ValueError, "num_samples"),
    (5, dict(batch_size=0), ValueError, "batch_size"),
    (5, dict(prefetch=0), ValueError, "prefetch"),
    (5, dict(weight_attr="missing"), ValueError, "weight_attr"),
    (5, dict(weight_attr="short"), ValueError, "weight_attr"),
    (5, dict(weight_attr="matrix"), ValueError, "weight_attr"),
    (5, dict(weight_attr="ints"), ValueError, "weight_attr"),
    (5, dict(input_nodes=torch.tensor([0, 5])), IndexError, "outside"),
    (5, dict(input_nodes=torch.tensor([0, 1, 2, 2]), batch_size=2, shuffle=False), ValueError, "inside one mini-batch"),
    (5, dict(input_nodes=torch.tensor([0, 1, 2, 1]), batch_size=2), ValueError, "anywhere"),
    ((1 << 31) + 1, dict(), ValueError, "2\\^31"),
])
def test_loader_refusals_need_no_device(ops, n, kw, err, word):
    import tch_geometric
    assert tch_geometric.LADIESLoader is tch_geometric.loader.LADIESLoader
    data = _graph(n, short=torch.zeros(5), matrix=torch.zeros(6, 2), ints=torch.zeros(6, dtype=torch.int64))
    args = dict(num_samples=[4, 4])
    args.update(kw)
    with pytest.raises(err, match=word):
        tch_geometric.LADIESLoader(data, device="cuda:0", **args)
