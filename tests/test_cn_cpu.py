"""tg_cn_links without a GPU: the restatement (helpers_cn) against brute force on three hand graphs; every refusal happens
before a launch; the workspace formula; the header is C99; the exports equal the header; the loader's ValueErrors;
cn_tables and distinct_degree against a float64 NumPy loop.  Only test_restatement_against_brute_force needs nothing but
the helper."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import helpers_cn as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tchgeo_cn.h")
FAKE, BIG = 0x10000, 1 << 50   # a non-null address that is never read: every call below is refused before a launch

sym = lambda pairs: [e for a, b in pairs for e in ((a, b), (b, a))]
HAND = {   # directed entries (x, w): w stands in x's row
    "triangle": (4, sym([(0, 1), (1, 2), (0, 2), (0, 3)]) + [(0, 1), (2, 2)]),   # (0, 1) twice, a self loop at 2
    "star": (6, sym([(0, i) for i in range(1, 6)])),
    "components": (7, sym([(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5), (5, 6)])),
}


def csr(n, edges):
    rows = [sorted(w for x, w in edges if x == r) for r in range(n)]
    return np.cumsum([0] + [len(r) for r in rows]), np.array([w for r in rows for w in r], dtype=np.int64)


@pytest.fixture(scope="module")
def ops():
    from tch_geometric import _cabi_cn
    _cabi_cn.lib.tg_last_error.restype = C.c_char_p
    return _cabi_cn


@pytest.mark.parametrize("name", list(HAND))
@pytest.mark.parametrize("exclude", [False, True])
def test_restatement_against_brute_force(name, exclude):
    n, edges = HAND[name]
    ptrs, indices = csr(n, edges)
    table = [3 * x + 1 for x in range(n)]
    for u in range(n):
        for v in range(n):
            want = hc.brute(set(edges), u, v, exclude)
            got = hc.cn(ptrs, indices, u, v, 2, exclude, [table])
            assert got["count"] == len(want) and got["cn"] == want[:2] and got["status"] == (len(want) > 2)
            assert got["score"] == [sum(table[w] for w in want)]
            assert got["adjacent"] == ((u, v) in edges) + 2 * ((v, u) in edges)
    assert hc.cn(ptrs, indices, 0, n, 2)["status"] == hc.cn(ptrs, indices, -1, 0, 2)["status"] == 2
    if name == "triangle":   # the self loop makes 2 a neighbour of itself: a member of C(1, 2) unless the ends are excluded
        assert hc.cn(ptrs, indices, 1, 2, 9, exclude)["cn"] == ([0] if exclude else [0, 2])


def call(ops, g="default", n_major=100, inp="default", out="default", m=4, form=0, status=FAKE, ws=FAKE, ws_bytes=BIG, **kw):
    from tch_geometric import _cabi
    if g == "default":
        g = _cabi.TgGraph()
        g.ptrs, g.indices, g.n_major, g.n_edges = kw.pop("ptrs", FAKE), FAKE, n_major, 500
    if inp == "default":
        inp = ops.TgCnIn(kw.pop("src", FAKE), kw.pop("dst", FAKE), kw.pop("tables", None), kw.pop("id_bound", 0),
                         kw.pop("cn_cap", 16), kw.pop("n_tables", 0), kw.pop("exclude_ends", 1), kw.pop("wave_max", 0))
    if out == "default":
        out = ops.TgCnOut(kw.pop("count", FAKE), kw.pop("cn", FAKE), None, kw.pop("score", None))
    assert not kw, kw
    ref = lambda s: C.byref(s) if s is not None else None
    return ops.lib.tg_cn_links(ref(g), ref(inp), ref(out), m, form, status, ws, ws_bytes, None)


REFUSALS = [
    (dict(g=None), "null graph"), (dict(inp=None), "null graph"), (dict(out=None), "null graph"),
    (dict(m=-1), "m = -1"), (dict(m=1 << 31), "m = "), (dict(form=3), "unknown form"), (dict(form=-1), "unknown form"),
    (dict(cn_cap=0), "cn_cap = 0"), (dict(cn_cap=(1 << 20) + 1), "cn_cap"),
    (dict(n_tables=-1), "n_tables = -1"), (dict(n_tables=5, tables=FAKE, id_bound=9), "n_tables = 5"),
    (dict(n_tables=1, id_bound=9, score=FAKE), "tables need"), (dict(n_tables=1, tables=FAKE, score=FAKE), "id_bound"),
    (dict(n_tables=2, tables=FAKE, id_bound=9), "null score"),
    (dict(exclude_ends=2), "exclude_ends"), (dict(wave_max=-1), "wave_max"),
    (dict(n_major=-1), "negative graph"), (dict(ws_bytes=-1), "workspace_bytes"), (dict(ptrs=None), "null graph arrays"),
    (dict(src=None), "null src"), (dict(dst=None), "null src"), (dict(count=None), "null src"), (dict(cn=None), "null src"),
    (dict(status=None), "null src"),
    (dict(ws=None), "workspace"), (dict(ws_bytes=511), "workspace"), (dict(form=2, ws_bytes=511), "workspace"),
    (dict(ws=FAKE + 2), "4-byte aligned"),
]


@pytest.mark.parametrize("kw, word", REFUSALS)
def test_refusals_before_any_launch(ops, kw, word):
    assert call(ops, **kw) == 1                              # TG_ERR_INVALID
    assert re.search(word, ops.lib.tg_last_error().decode()), ops.lib.tg_last_error()


def test_unsupported_ids_empty_calls_and_the_binding_s_own_refusals(ops):
    assert call(ops, n_major=(1 << 31) + 1) == 3             # TG_ERR_UNSUPPORTED
    assert call(ops, m=0, src=None, dst=None, count=None, cn=None, status=None, ws=None, ws_bytes=0) == 0   # launches nothing
    for kw in (dict(cn_cap=0), dict(cn_cap=(1 << 20) + 1), dict(n_tables=5), dict(n_tables=-1), dict(form=3),
               dict(wave_max=-1)):
        with pytest.raises(ValueError):
            ops.CommonNeighbors(**kw)
    links = torch.zeros(3, dtype=torch.int64)
    for kw in (dict(src=links.to(torch.int32)), dict(dst=links[:2]), dict(tables=torch.zeros(3, dtype=torch.int32)),
               dict(tables=torch.zeros((1, 3), dtype=torch.int64)), dict(tables=torch.zeros((5, 3), dtype=torch.int32))):
        with pytest.raises(ValueError):
            ops.cn_links(None, **dict(dict(src=links, dst=links), **kw))
    with pytest.raises(ValueError):
        ops.cn_tables(torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), kinds=("cn",))
    with pytest.raises(RuntimeError, match="cn_cap lists and a link's endpoint outside the graph"):
        ops.cn_status_check(3, "here")
    ops.cn_status_check(0, "here")


def test_workspace_formula(ops):
    for m in (0, 1, 63, 64, 65, 5000, (1 << 31) - 1):
        for form in (0, 1, 2):
            want = 0 if form == 1 else (256 + 4 * m + 255) // 256 * 256
            assert ops.CommonNeighbors.workspace_bytes(m, form) == (want, form), (m, form)
    assert ops.CommonNeighbors.workspace_bytes(4) == (512, 0)


def test_header_is_c99_and_the_exports_equal_it(ops):
    src = ('#include "tchgeo_cn.h"\nint main(void) { tg_cn_in i; tg_cn_out o; i.cn_cap = TG_CN_WINDOW; (void)o; '
           'return i.cn_cap == 512 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    "-x", "c", "-"], input=src.encode(), check=True)
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"TG_API\s+[\w\s\*]+?\b(tg_\w+)\s*\(", text)
    assert sorted(declared) == sorted(ops.EXPORTS) == ["tg_cn_links", "tg_cn_workspace_bytes"]
    for name in declared:
        assert hasattr(ops.lib, name) and getattr(ops.lib, name).argtypes
    assert [f for f, _ in ops.TgCnOut._fields_] == ["count", "cn", "adjacent", "score"]
    assert [f for f, _ in ops.TgCnIn._fields_] == ["src", "dst", "tables", "id_bound", "cn_cap", "n_tables", "exclude_ends",
                                                   "wave_max"]
    defines = dict(re.findall(r"#define TG_CN_(\w+) (\d+)", text))
    for name in ("MAX_CAP", "MAX_TABLES", "WINDOW", "WAVE_MAX", "GROUP_TILES", "WAVE_GROUPS", "GROUP_GROUPS"):
        assert int(defines[name]) == getattr(ops, "CN_" + name), name


def test_tables_and_distinct_degree_against_a_numpy_loop(ops):
    rs = np.random.default_rng(3)
    n = 40
    edges = [(int(a), int(b)) for a, b in rs.integers(0, n, (300, 2))] + [(5, 7)] * 4 + [(1, 2)]
    # row 0 is empty, row 1 holds one distinct entry twice, row 2 two
    edges = [e for e in edges if e[0] > 2] + [(1, 2), (1, 2), (2, 3), (2, 9)]
    ptrs, indices = csr(n, edges)
    deg = hc.distinct_degrees(ptrs, indices)
    assert deg[:3] == [0, 1, 2] and len(hc.row(ptrs, indices, 5)) > deg[5]
    tp, ti = torch.from_numpy(ptrs), torch.from_numpy(indices)
    assert ops.distinct_degree(tp, ti).tolist() == deg
    tables = ops.cn_tables(tp, ti)
    assert tables.dtype == torch.int32 and tables.shape == (2, n)
    for k, kind in enumerate(("aa", "ra")):
        assert (tables[k].to(torch.int64) & 0xFFFFFFFF).tolist() == hc.table_words(deg, kind), kind
    assert hc.table_words([0, 1, 2], "aa")[:2] == [0, 0] and hc.table_words([0, 1], "ra") == [0, 2 ** 32 - 1]   # the clamp
    assert ops.cn_tables(tp, ti, kinds=("ra",)).tolist() == tables[1:].tolist()


def test_the_loader_refuses_before_any_device_work():
    import tch_geometric
    from tch_geometric.transforms import Graph
    assert tch_geometric.CommonNeighborLoader is tch_geometric.loader.CommonNeighborLoader
    data = Graph(edge_index=torch.tensor([[0, 1, 2], [1, 2, 0]]), num_nodes=3)
    links = torch.tensor([[0, 1], [1, 2]])
    for kw in (dict(cn_cap=0), dict(cn_cap=(1 << 20) + 1), dict(batch_size=0), dict(prefetch=0), dict(scores=("cn", "katz")),
               dict(edge_label_index=links[0]), dict(edge_label_index=links.to(torch.int32)),
               dict(edge_label_index=torch.tensor([[0, 3], [1, 2]])), dict(edge_label_index=torch.tensor([[0, -1], [1, 2]])),
               dict(edge_label=torch.ones(3))):
        with pytest.raises(ValueError):
            tch_geometric.CommonNeighborLoader(data, **dict(dict(edge_label_index=links, device="cuda:0"), **kw))
