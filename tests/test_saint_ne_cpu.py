"""GraphSAINT's node and edge samplers (tg_saint_node_nodes, tg_saint_edge_nodes, GraphSAINTNodeLoader,
GraphSAINTEdgeLoader), host-only parts: the NumPy restatement against a brute-force dict version, the exact laws against
the formula by exhausting t and k, the restatement's own draws against the laws, the power of the GPU law tests against
three named wrong laws, the form / workspace queries around the largest LDS table, every refusal that comes before a
launch and the loaders' argument refusals.  No GPU: every device pointer handed over is null or an address that is never
read."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import exact_laws as L
import helpers_saint_ne as H
from helpers_induced import csc_of
from helpers_labor import named_draw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tg_saint_ne_form", "tg_saint_ne_workspace_bytes", "tg_saint_node_nodes", "tg_saint_edge_nodes")
LDS = 160 * 1024
N_LAW = 1 << 16                                             # mini-batches of the GPU law tests


@pytest.fixture(scope="module")
def cabi():
    if not os.path.exists(os.path.join(ROOT, "tch-geometric_amd", "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tch-geometric_amd"), "-s"])
    from tch_geometric import _cabi
    return _cabi


def views(edge_index, n):
    """-> (csc, csr) as (ptrs, indices) pairs"""
    csc = csc_of(edge_index, n)[:2]
    csr = csc_of(np.asarray(edge_index)[::-1], n)[:2]
    return csc, csr


# ---- the restatement against brute force -------------------------------------------------------------------------------
def scalar_draw(seed, call_id, tag, i):
    w = [int(x) for x in named_draw(seed, call_id, tag, i, 0, 0)]
    return w[0] | w[1] << 32, w[2] | w[3] << 32


def dedup(positions):
    """{position: vertex} -> the distinct vertices by first position, with a dict: the definition"""
    first = {}
    for p in sorted(positions):
        first.setdefault(positions[p], p)
    return [v for v, _ in sorted(first.items(), key=lambda kv: kv[1])]


def brute_node(indices, B, seed, call_id, id_bound):
    positions, status = {}, 0
    for i in range(B):
        lo, _ = scalar_draw(seed, call_id, H.TAG_SAINT_NODE, i)
        v = int(indices[lo * len(indices) >> 64])
        if 0 <= v < id_bound:
            positions[i] = v
        else:
            status |= 2
    return dedup(positions), status


def brute_edge(csc, cols, csr, rows, B, seed, call_id, id_bound):
    positions, status = {}, 0
    for i in range(B):
        lo, hi = scalar_draw(seed, call_id, H.TAG_SAINT_EDGE, i)
        t = lo * (len(cols) + len(rows)) >> 64
        side = t >= len(cols)
        major = int(rows[t - len(cols)] if side else cols[t])
        ptrs, idx = csr if side else csc
        if not 0 <= major < len(ptrs) - 1:
            status |= 2
            continue
        b, e = int(ptrs[major]), int(ptrs[major + 1])
        if e <= b:
            status |= 4
            continue
        other = int(idx[b + (hi * (e - b) >> 64)])
        src, dst = (major, other) if side else (other, major)
        if not (0 <= src < id_bound and 0 <= dst < id_bound):
            status |= 2
            continue
        positions[i], positions[B + i] = src, dst
    return dedup(positions), status


@pytest.mark.parametrize("seed", range(6))
def test_restatement_equals_brute_force(seed):
    rs = np.random.default_rng(seed)
    n, B, G = int(rs.integers(4, 12)), int(rs.integers(1, 40)), 3
    ei = rs.integers(0, n, (2, int(rs.integers(3, 40))))
    ei = ei[:, ei[0] != 0]                                  # vertex 0 is a sink
    if ei.shape[1] == 0:
        ei = np.array([[1], [0]])
    csc, csr = views(ei, n)
    cols, rows = H.nonempty(csc[0]), H.nonempty(csr[0])
    for id_bound in (n, max(1, n - 2)):                     # the second refuses what touches the last two vertices
        got, status = H.node_lists(csc[1], G, B, 5 + seed, 1000, id_bound)
        want = [brute_node(csc[1], B, 5 + seed, 1000 + g, id_bound) for g in range(G)]
        assert [x.tolist() for x in got] == [w[0] for w in want]
        assert status == (2 if any(w[1] for w in want) else 0)
        # the lists as the loader makes them, then with an empty major, one outside the graph and a repeat in each list
        for c, r in ((cols, rows), (np.concatenate([cols, [0, n, cols[0]]]), np.concatenate([rows, [-1, 0, rows[0]]]))):
            got, status = H.edge_lists(csc, c, csr, r, G, B, 5 + seed, 1 << 40, id_bound)
            want = [brute_edge(csc, c, csr, r, B, 5 + seed, (1 << 40) + g, id_bound) for g in range(G)]
            assert [x.tolist() for x in got] == [w[0] for w in want]
            assert status == int(np.bitwise_or.reduce([w[1] for w in want]))
        got, status = H.edge_lists(csc, cols, None, np.zeros(0, dtype=np.int64), G, B, seed, 7, n)      # one-sided
        want = [brute_edge(csc, cols, None, [], B, seed, 7 + g, n) for g in range(G)]
        assert [x.tolist() for x in got] == [w[0] for w in want] and status == 0


def test_positions_are_i_and_b_plus_i():
    """every source before every target: a target that is also a later slot's source keeps the SOURCE's position"""
    csc, csr = views(np.array([[0, 1, 2], [1, 2, 0]]), 3)
    src, dst, refused, _ = H.edge_draws(csc, H.nonempty(csc[0]), csr, H.nonempty(csr[0]), 1, 6, 3, 0, 3)
    want = list(dict.fromkeys(src[0].tolist() + dst[0].tolist()))
    assert H.lists_of((src, dst), refused)[0].tolist() == want


# ---- the laws ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def law():
    ei, n = H.law_graph()
    csc, csr = views(ei, n)
    cols, rows = H.nonempty(csc[0]), H.nonempty(csr[0])
    cat, pairs = H.pair_categories(*csc)
    entry = H.edge_entry_law(csc[0], csc[1], cols, rows, n)
    return dict(n=n, ei=ei, csc=csc, csr=csr, cols=cols, rows=rows, cat=cat, pairs=pairs, entry=entry,
                pair=H.merged(entry, cat, len(pairs)))


def test_law_graph_has_what_the_laws_need(law):
    ei, n = law["ei"], law["n"]
    assert (ei[0] == ei[1]).any() and len(law["pairs"]) < ei.shape[1]                   # self loops, parallel edges
    assert 18 not in ei[0] and 18 in ei[1] and 17 not in ei[1] and 17 in ei[0] and 19 not in ei
    assert abs(law["entry"].sum() - 1) < 1e-12 and abs(law["pair"].sum() - 1) < 1e-12
    # every category of the three GPU law tests expects at least MIN_EXPECTED of the 2^16 outcomes
    assert (law["pair"] * N_LAW).min() >= L.MIN_EXPECTED
    node = H.node_law(law["csc"][1], n)
    assert (node[node > 0] * N_LAW).min() >= L.MIN_EXPECTED


def test_edge_law_is_the_formula_by_exhausting_t_and_k(law):
    """the mixture, enumerated, is (1 / deg_in(v) + 1 / deg_out(u)) / (n_cols + n_rows) per entry"""
    csc, csr, n = law["csc"], law["csr"], law["n"]
    deg_in, deg_out = np.diff(csc[0]), np.diff(csr[0])
    col_of = np.repeat(np.arange(n), deg_in)
    formula = (1.0 / deg_in[col_of] + 1.0 / deg_out[csc[1]]) / (len(law["cols"]) + len(law["rows"]))
    assert np.allclose(law["entry"], formula, rtol=1e-14, atol=0)
    enumerated = H.pair_law_by_enumeration(csc, law["cols"], csr, law["rows"])
    assert sum(enumerated.values()) == 1
    assert np.allclose(H.law_vector(enumerated, law["pairs"]), law["pair"], rtol=1e-13, atol=0)
    one_sided = H.pair_law_by_enumeration(csc, law["cols"], None, [])
    want = H.merged(H.edge_entry_law(csc[0], csc[1], law["cols"], [], n), law["cat"], len(law["pairs"]))
    assert np.allclose(H.law_vector(one_sided, law["pairs"]), want, rtol=1e-13, atol=0)
    tiny = views(np.array([[0, 0, 1, 2, 2], [1, 1, 2, 0, 2]]), 3)                    # by hand: parallel 0 -> 1, loop 2 -> 2
    got = H.pair_law_by_enumeration(tiny[0], [0, 1, 2], tiny[1], [0, 1, 2])
    from fractions import Fraction as F
    assert got == {(0, 1): F(1, 6) + F(1, 6), (1, 2): F(1, 12) + F(1, 6), (2, 0): F(1, 6) + F(1, 12),
                   (2, 2): F(1, 12) + F(1, 12)}


def test_node_law_is_degree_over_edges(law):
    node = H.node_law(law["csc"][1], law["n"])
    assert np.allclose(node, np.diff(law["csr"][0]) / law["ei"].shape[1]) and node[18] == 0 and node[19] == 0


def pair_counts(src, dst, pairs):
    index = {(int(u), int(v)): i for i, (u, v) in enumerate(pairs)}
    return np.bincount([index[int(u), int(v)] for u, v in zip(src, dst)], minlength=len(pairs))


def test_the_restatements_draws_follow_the_laws(law):
    """2^16 call ids of B = 1, as the GPU tests launch them"""
    v, refused, status = H.node_draws(law["csc"][1], N_LAW, 1, 0xC0FFEE, 0, law["n"])
    assert status == 0 and not refused.any()
    L.chi2_gof(np.bincount(v[:, 0], minlength=law["n"]), H.node_law(law["csc"][1], law["n"]), "node restatement")
    src, dst, refused, status = H.edge_draws(law["csc"], law["cols"], law["csr"], law["rows"], N_LAW, 1, 0xC0FFEE, 0, law["n"])
    assert status == 0 and not refused.any()
    L.chi2_gof(pair_counts(src[:, 0], dst[:, 0], law["pairs"]), law["pair"], "edge restatement")


def test_power_against_three_named_wrong_laws(law):
    """what the GPU law test would certainly catch at its N: (a) uniform over entries, (b) the column term only, (c) k made
    from lo instead of hi"""
    right, n_cat = law["pair"], len(law["pairs"])
    uniform = H.merged(H.uniform_entry_law(law["csc"][1]), law["cat"], n_cat)
    column = H.merged(H.edge_entry_law(law["csc"][0], law["csc"][1], law["cols"], [], law["n"]), law["cat"], n_cat)
    shared = H.law_vector(H.pair_law_by_enumeration(law["csc"], law["cols"], law["csr"], law["rows"], k_from_lo=True), law["pairs"])
    for name, wrong in (("uniform over entries", uniform), ("column term only", column), ("k from lo", shared)):
        assert abs(wrong.sum() - 1) < 1e-9, name
        assert L.power(wrong, right, N_LAW) >= 0.999, name


# ---- exports and the queries' arithmetic -------------------------------------------------------------------------------------
def test_symbols_struct_and_tags(cabi):
    header = open(os.path.join(ROOT, "include", "tchgeo.h")).read()
    for name in NAMES:
        assert name in cabi.EXPORTS and hasattr(cabi.lib, name) and "TG_API int %s(" % name in header
    assert [f for f, _ in cabi.TgSaintEdgeIn._fields_] == ["csc", "cols", "n_cols", "csr", "rows", "n_rows"]
    assert "#define TG_TAG_SAINT_NODE 16u" in header and "#define TG_TAG_SAINT_EDGE 17u" in header
    assert (H.TAG_SAINT_NODE, H.TAG_SAINT_EDGE) == (16, 17)


def r256(x):
    return (x + 255) & ~255


def test_form_and_workspace_arithmetic(cabi):
    """P = 12 288 is the largest LDS table of 160 KiB; one position more takes the flat form whatever the limit says,
    because a lane of the LDS form holds at most 12 slots.  Nothing here touches a device."""
    assert cabi.saint_ne_form(12288, LDS) == (1, 16384 * 8 + 2 * 12288 + 256)
    assert cabi.saint_ne_form(12288, LDS) == cabi.saint_rw_form(3072, 3, LDS)        # the plan is tg_saint_rw_form's
    assert cabi.saint_ne_form(12288, 16384 * 8 + 2 * 12288 + 255)[0] == 2            # one byte short
    form, lds = cabi.saint_ne_form(12289, LDS)
    assert form == 2 and lds == 32768 * 8 + ((2 * 12289 + 15) & ~15) + 256
    assert cabi.saint_ne_form(12289, 1 << 30)[0] == 2 and cabi.saint_ne_form(1 << 30, 1 << 40)[0] == 2
    assert cabi.saint_ne_form(1, 1024) == (1, 64 * 8 + 16 + 256) and cabi.saint_ne_form(0, 1024)[0] == 1
    last = 0
    for P in (1, 2, 47, 48, 49, 63, 64, 65, 1024, 6144, 12287, 12288):                # monotone, sized by P
        form, lds = cabi.saint_ne_form(P, LDS)
        assert form == 1 and lds >= last
        last = lds
    assert cabi.saint_ne_form(64, LDS)[1] < 4096                                       # small P: many workgroups per CU
    for P in (12289, 12290, 20000, 1 << 20):
        assert cabi.saint_ne_form(P, LDS)[0] == 2
    last = 0
    for P in (1, 63, 12288, 12289, 24578):
        cap = 64
        while cap < (4 * P + 2) // 3:
            cap *= 2
        per = r256(cap * 4) + r256(cap * 4) + r256(P * 4) + r256(((P + 1023) // 1024) * 4) + r256(P * 4)
        assert cabi.saint_ne_workspace_bytes(5, P, form=2) == (5 * per, per)
        assert cabi.saint_ne_workspace_bytes(5, P, form=1) == (0, per)
        assert cabi.saint_ne_workspace_bytes(0, P, form=2) == (0, per)
        assert per >= last
        last = per


def test_query_refusals(cabi):
    lib = cabi.lib
    x, y, f = C.c_int64(0), C.c_int64(0), C.c_int32(0)
    assert lib.tg_saint_ne_form(C.c_int64(-1), C.c_int64(LDS), C.byref(f), C.byref(x)) == 1
    assert lib.tg_saint_ne_form(C.c_int64((1 << 30) + 1), C.c_int64(LDS), C.byref(f), C.byref(x)) == 1
    assert lib.tg_saint_ne_form(C.c_int64(4), C.c_int64(LDS), None, C.byref(x)) == 1
    assert lib.tg_saint_ne_form(C.c_int64(4), C.c_int64(LDS), C.byref(f), None) == 1
    assert lib.tg_saint_ne_workspace_bytes(C.c_int64(-1), C.c_int64(4), C.c_int32(2), C.byref(x), C.byref(y)) == 1
    assert lib.tg_saint_ne_workspace_bytes(C.c_int64(1), C.c_int64(4), C.c_int32(5), C.byref(x), C.byref(y)) == 1
    assert lib.tg_saint_ne_workspace_bytes(C.c_int64(1), C.c_int64(-4), C.c_int32(2), C.byref(x), C.byref(y)) == 1
    assert lib.tg_saint_ne_workspace_bytes(C.c_int64(1), C.c_int64(4), C.c_int32(2), None, C.byref(y)) == 1
    assert lib.tg_saint_ne_workspace_bytes(C.c_int64(0x7fffffff), C.c_int64(1 << 30), C.c_int32(2), C.byref(x), C.byref(y)) == 1
    assert b"overflow" in lib.tg_last_error()


# ---- refusals before any launch ------------------------------------------------------------------------------------------------
FAKE = 0x10000          # a non-null address that is never read: every call below is refused before anything is launched


def fake_graph(cabi, n_major=100, n_edges=10, ptrs=FAKE, indices=FAKE):
    g = cabi.TgGraph()
    g.ptrs, g.indices, g.n_major, g.n_edges = ptrs, indices, n_major, n_edges
    return g


def call_node(cabi, graph=True, id_bound=100, G=2, B=4, rng=True, out=True, nodes=FAKE, pitch=None, counts=FAKE, stride=1,
              status=FAKE, ws=None, ws_bytes=0, form=2, **gkw):
    g = fake_graph(cabi, **gkw)
    o = cabi.TgSaintRwOut(nodes, B if pitch is None else pitch, counts, stride)
    r = cabi.TgRng(1, 2)
    return cabi.lib.tg_saint_node_nodes(C.byref(g) if graph else None, C.c_int64(id_bound), C.c_int64(G), C.c_int64(B),
                                        C.byref(r) if rng else None, C.byref(o) if out else None, C.c_void_p(status),
                                        C.c_void_p(ws), C.c_int64(ws_bytes), C.c_int32(form), None)


def call_edge(cabi, arg=True, csc=True, csr=True, cols=FAKE, n_cols=3, rows=FAKE, n_rows=3, id_bound=100, G=2, B=4, rng=True,
              out=True, nodes=FAKE, pitch=None, counts=FAKE, stride=1, status=FAKE, ws=None, ws_bytes=0, form=2, csc_kw={},
              csr_kw={}):
    g1, g2 = fake_graph(cabi, **csc_kw), fake_graph(cabi, **csr_kw)
    a = cabi.TgSaintEdgeIn(C.pointer(g1) if csc else None, cols, n_cols, C.pointer(g2) if csr else None, rows, n_rows)
    o = cabi.TgSaintRwOut(nodes, 2 * B if pitch is None else pitch, counts, stride)
    r = cabi.TgRng(1, 2)
    return cabi.lib.tg_saint_edge_nodes(C.byref(a) if arg else None, C.c_int64(id_bound), C.c_int64(G), C.c_int64(B),
                                        C.byref(r) if rng else None, C.byref(o) if out else None, C.c_void_p(status),
                                        C.c_void_p(ws), C.c_int64(ws_bytes), C.c_int32(form), None)


COMMON = [
    (dict(rng=False), "null argument"),
    (dict(out=False), "null argument"),
    (dict(nodes=None), "null nodes"),
    (dict(counts=None), "null nodes"),
    (dict(status=None), "null nodes"),
    (dict(B=-1), "batch_size"),
    (dict(pitch=3), "pitch_nodes"),
    (dict(stride=0), "counts_stride"),
    (dict(form=3), "unknown form"),
    (dict(G=-1), "n_batches"),
    (dict(G=1 << 31), "n_batches"),
    (dict(id_bound=0), "id_bound"),
    (dict(ws=None, ws_bytes=0), "workspace too small"),
    (dict(ws=FAKE, ws_bytes=100), "workspace too small"),
    (dict(ws=FAKE, ws_bytes=-1), "workspace_bytes"),
    (dict(ws=FAKE + 4, ws_bytes=1 << 30), "8-byte aligned"),
]


@pytest.mark.parametrize("kw, word", COMMON + [
    (dict(graph=False), "null argument"),
    (dict(indices=None), "null the graph"),
    (dict(n_edges=-1), "negative"),
    (dict(n_edges=0, indices=None), "nothing to draw"),
    (dict(B=(1 << 30) + 1), "batch_size"),
    (dict(B=12289, form=1), "does not fit"),
])
def test_node_refusals(cabi, kw, word):
    assert call_node(cabi, **kw) == 1                                    # TG_ERR_INVALID
    assert re.search(word, cabi.lib.tg_last_error().decode()), cabi.lib.tg_last_error()


@pytest.mark.parametrize("kw, word", COMMON + [
    (dict(arg=False), "null argument"),
    (dict(csc=False), "without its graph"),
    (dict(csr=False), "without its graph"),
    (dict(cols=None), "null cols / rows"),
    (dict(rows=None), "null cols / rows"),
    (dict(n_cols=-1), "negative list size"),
    (dict(n_rows=-1), "negative list size"),
    (dict(n_cols=0, n_rows=0), "nothing to draw"),
    (dict(csc_kw=dict(ptrs=None)), "null csc graph"),
    (dict(csr_kw=dict(ptrs=None)), "null csr graph"),
    (dict(csc_kw=dict(indices=None)), "null csc graph"),
    (dict(csr_kw=dict(n_major=-1)), "negative csr graph"),
    (dict(B=(1 << 29) + 1), "batch_size"),
    (dict(B=6145, form=1), "does not fit"),
])
def test_edge_refusals(cabi, kw, word):
    assert call_edge(cabi, **kw) == 1
    assert re.search(word, cabi.lib.tg_last_error().decode()), cabi.lib.tg_last_error()


def test_id_limit_and_empty_launches(cabi):
    big = dict(ws=FAKE, ws_bytes=1 << 30)
    for call in (call_node, call_edge):
        assert call(cabi, id_bound=(1 << 31) + 1, **big) == 3            # TG_ERR_UNSUPPORTED
        assert b"32-bit hash keys" in cabi.lib.tg_last_error()
        assert call(cabi, id_bound=1 << 31, G=0, **big) == 0
        assert call(cabi, G=0, **big) == 0 and call(cabi, B=0, **big) == 0           # nothing to launch
        assert call(cabi, G=0, form=0) == 0 and call(cabi, G=0, form=1) == 0        # before any question to a device
        assert call(cabi, G=0, form=2) == 1                                           # the flat form's workspace is still checked
    assert call_node(cabi, B=0, n_edges=0, indices=None, **big) == 0                 # no entries, but nothing to draw either
    assert call_edge(cabi, B=0, n_cols=0, n_rows=0, **big) == 0
    assert call_edge(cabi, G=0, csr=False, rows=None, n_rows=0, **big) == 0          # the one-sided call is legal
    assert call_edge(cabi, G=0, csc_kw=dict(n_edges=0, indices=None), **big) == 0    # a graph without entries needs no indices


# ---- the loaders' refusals ---------------------------------------------------------------------------------------------------------
def _graph(**attrs):
    from tch_geometric.transforms import Graph
    ei = torch.tensor([[0, 1, 2, 3, 4, 0], [1, 2, 3, 4, 0, 2]])
    return Graph(edge_index=ei, num_nodes=5, **attrs)


@pytest.mark.parametrize("which", ["GraphSAINTNodeLoader", "GraphSAINTEdgeLoader"])
@pytest.mark.parametrize("args, kw, word", [
    ((0, 3), {}, "batch_size"),
    ((4, 0), {}, "num_steps"),
    ((4, 3), dict(sample_coverage=-1), "sample_coverage"),
    ((4, 3), dict(prefetch=0), "prefetch"),
    ((4, 3), dict(form=3), "form"),
    (((1 << 30) + 1, 3), {}, "2\\^30"),
    ((4, 3), dict(call_id0=-1), "call_id0"),
    ((4, 3), dict(call_id0=1 << 62), "call_id0"),
])
def test_loader_refusals_need_no_device(cabi, which, args, kw, word):
    import tch_geometric
    cls = getattr(tch_geometric, which)
    assert cls is getattr(tch_geometric.loader, which)
    with pytest.raises(ValueError, match=word):
        cls(_graph(), *args, device="cuda:0", **kw)


def test_edge_loader_counts_two_positions_per_edge(cabi):
    import tch_geometric
    with pytest.raises(ValueError, match="2 \\* batch_size = %d positions" % ((1 << 30) + 2)):
        tch_geometric.GraphSAINTEdgeLoader(_graph(), (1 << 29) + 1, 3, device="cuda:0")


@pytest.mark.parametrize("which", ["GraphSAINTNodeLoader", "GraphSAINTEdgeLoader"])
@pytest.mark.parametrize("name, n", [("node_norm", 5), ("edge_norm", 6)])
def test_loaders_refuse_data_that_hides_their_norms(cabi, which, name, n):
    import tch_geometric
    with pytest.raises(ValueError, match=name):
        getattr(tch_geometric, which)(_graph(**{name: torch.zeros(n)}), 4, 3, sample_coverage=1, device="cuda:0")
