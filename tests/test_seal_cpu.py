"""tg_seal_nodes without a GPU: the restatement (helpers_seal) on three hand graphs whose answers are written out here and on
the header's six label values; every refusal happens before a launch; the workspace formula; the header is C99; the exports
equal the header; the loader's ValueErrors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import helpers_seal as hs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tchgeo_seal.h")
FAKE, BIG = 0x10000, 1 << 50   # a non-null address that is never read: every call below is refused before a launch

PATH = [(i, i + 1) for i in range(5)]                        # 0 - 1 - 2 - 3 - 4 - 5
CYCLE8 = [(i, (i + 1) % 8) for i in range(8)]
CYCLE5 = [(0, 2), (2, 3), (3, 4), (4, 1), (1, 0)]            # 0 - 2 - 3 - 4 - 1 - 0
HAND = [   # (edges, n, link, h, nodes, z, du, dv, rounds)
    (PATH, 6, (2, 3), 1, [2, 3, 1, 4], [1, 1, 0, 0], [0, -1, 1, -1], [-1, 0, -1, 1], 1),
    # 2 and 3 are reached from 0 only through 1 or round the far side, which leaves N = {0, 1, 2, 3, 6, 7}
    (CYCLE8, 8, (0, 1), 2, [0, 1, 2, 3, 6, 7], [1, 1, 0, 0, 0, 0], [0, -1, -1, -1, 2, 1], [-1, 0, 1, 2, -1, -1], 2),
    (CYCLE5, 5, (0, 1), 2, [0, 1, 2, 3, 4], [1, 1, 4, 5, 4], [0, -1, 1, 2, 3], [-1, 0, 3, 2, 1], 3),   # du(4) = 3 > h
]


def symmetric_csr(edges, n):
    rows = [[] for _ in range(n)]
    for a, b in edges:
        rows[a].append(b)
        rows[b].append(a)
    return np.cumsum([0] + [len(r) for r in rows]), np.array([t for r in rows for t in r])


@pytest.fixture(scope="module")
def ops():
    from tch_geometric import _cabi_seal
    _cabi_seal.lib.tg_last_error.restype = C.c_char_p
    return _cabi_seal


@pytest.mark.parametrize("edges, n, link, h, nodes, z, du, dv, rounds", HAND)
def test_restatement_on_the_hand_graphs(edges, n, link, h, nodes, z, du, dv, rounds):
    ptrs, indices = symmetric_csr(edges, n)
    assert hs.seal(ptrs, indices, *link, h, n) == dict(nodes=nodes, z=z, du=du, dv=dv, rounds=rounds)
    assert hs.seal(ptrs, indices, *link, h, n, z_max=3)["z"] == [min(w, 3) for w in z]
    assert hs.seal(ptrs, indices, *link, h, len(nodes) - 1) == dict(refused=1)
    assert hs.seal(ptrs, indices, link[0], n, h, n) == dict(refused=2) and hs.seal(ptrs, indices, 1, 1, h, n) == dict(refused=4)


def test_the_six_label_values():
    pairs = [(1, 1), (1, 2), (1, 3), (2, 2), (1, 4), (2, 3)]
    assert [hs.label(a, b) for a, b in pairs] == [hs.label(b, a) for a, b in pairs] == [2, 3, 4, 5, 6, 7]
    assert hs.label(-1, 2) == hs.label(2, -1) == 0


def call(ops, g="default", n_major=100, inp="default", out="default", m=4, form=0, status=FAKE, ws=FAKE, ws_bytes=BIG, **kw):
    from tch_geometric import _cabi
    if g == "default":
        g = _cabi.TgGraph()
        g.ptrs, g.indices, g.n_major, g.n_edges = kw.pop("ptrs", FAKE), FAKE, n_major, 500
    if inp == "default":
        inp = ops.TgSealIn(kw.pop("src", FAKE), kw.pop("dst", FAKE), kw.pop("num_hops", 2), kw.pop("node_cap", 100),
                           kw.pop("z_max", 0))
    if out == "default":
        out = ops.TgSealOut(*(kw.pop(name, FAKE) for name in ("count", "nodes", "z")))   # the optional outputs stay NULL
    assert not kw, kw
    ref = lambda s: C.byref(s) if s is not None else None
    return ops.lib.tg_seal_nodes(ref(g), ref(inp), ref(out), m, form, status, ws, ws_bytes, None)


WS_BYTES = 4 * (16 * 8192 + 8192 // 4 + 4096 * 4)   # node_cap 4096, m = 4
REFUSALS = [
    (dict(g=None), "null graph"), (dict(inp=None), "null graph"), (dict(out=None), "null graph"),
    (dict(m=-1), "m = -1"), (dict(m=1 << 31), "m = "),
    (dict(node_cap=1), "node_cap = 1"), (dict(node_cap=(1 << 20) + 1), "node_cap"),
    (dict(num_hops=0), "num_hops = 0"), (dict(num_hops=65), "num_hops = 65"), (dict(z_max=-1), "z_max"),
    (dict(form=3), "unknown form"), (dict(form=-1), "unknown form"), (dict(form=1, node_cap=2049), "LDS form"),
    (dict(n_major=-1), "negative graph"), (dict(ws_bytes=-1), "workspace_bytes"),
    (dict(ptrs=None), "null graph arrays"), (dict(src=None), "null src"), (dict(dst=None), "null src"),
    (dict(count=None), "null src"), (dict(nodes=None), "null src"), (dict(z=None), "null src"), (dict(status=None), "null src"),
    (dict(node_cap=4096, ws=None), "workspace"), (dict(node_cap=4096, ws_bytes=WS_BYTES - 1), "workspace"),
    (dict(node_cap=4096, ws=FAKE + 4), "8-byte aligned"), (dict(form=2, ws_bytes=4 * (16 * 1024 + 256 + 512) - 1), "workspace"),
]


@pytest.mark.parametrize("kw, word", REFUSALS)
def test_refusals_before_any_launch(ops, kw, word):
    assert call(ops, **kw) == 1                              # TG_ERR_INVALID
    assert re.search(word, ops.lib.tg_last_error().decode()), ops.lib.tg_last_error()


def test_unsupported_ids_empty_calls_and_the_binding_s_own_refusals(ops):
    assert call(ops, n_major=(1 << 31) + 1) == 3             # TG_ERR_UNSUPPORTED
    assert call(ops, m=0, src=None, dst=None, count=None, status=None, ws=None, ws_bytes=0, node_cap=4096) == 0   # launches nothing
    for kw in (dict(num_hops=0), dict(num_hops=65), dict(node_cap=1), dict(node_cap=(1 << 20) + 1), dict(z_max=-1),
               dict(form=3), dict(node_cap=2049, form=1)):
        with pytest.raises(ValueError):
            ops.Seal(**kw)
    with pytest.raises(RuntimeError, match="node_cap holds and a link from a vertex to itself"):
        ops.seal_status_check(5, "here")
    ops.seal_status_check(0, "here")


def test_workspace_formula(ops):
    r256 = lambda x: (x + 255) & ~255
    for m in (0, 1, 127, 128, 129, 5000):
        for cap in (2, 512, 513, 2048, 2049, 4096, 4097, 1 << 20):
            for form in (0, 2):
                T = 1024
                while T < 2 * cap:
                    T *= 2
                lds = form == 0 and cap <= ops.SEAL_LDS_CAP
                want = 0 if lds else min(m, ops.SEAL_WS_GROUPS) * (16 * T + T // 4 + r256(4 * cap))
                assert ops.Seal.workspace_bytes(m, cap, form) == (want, 1 if lds else 2), (m, cap, form)
    assert ops.Seal.workspace_bytes(4, 4096) == (WS_BYTES, 2) and ops.Seal.workspace_bytes(9, 2048, 1) == (0, 1)


def test_header_is_c99_and_the_exports_equal_it(ops):
    src = ('#include "tchgeo_seal.h"\nint main(void) { tg_seal_in i; tg_seal_out o; i.node_cap = TG_SEAL_LDS_CAP; (void)o; '
           'return i.node_cap == 2048 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    "-x", "c", "-"], input=src.encode(), check=True)
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"TG_API\s+[\w\s\*]+?\b(tg_\w+)\s*\(", text)
    assert sorted(declared) == sorted(ops.EXPORTS) == ["tg_seal_nodes", "tg_seal_workspace_bytes"]
    for name in declared:
        assert hasattr(ops.lib, name) and getattr(ops.lib, name).argtypes
    assert [f for f, _ in ops.TgSealOut._fields_] == ["count", "nodes", "z", "du", "dv", "rounds"]
    assert [f for f, _ in ops.TgSealIn._fields_] == ["src", "dst", "num_hops", "node_cap", "z_max"]


def test_the_loader_refuses_before_any_device_work():
    import tch_geometric
    from tch_geometric.transforms import Graph
    assert tch_geometric.SEALLoader is tch_geometric.loader.SEALLoader
    data = Graph(edge_index=torch.tensor([[0, 1, 2], [1, 2, 0]]), num_nodes=3)
    links = torch.tensor([[0, 1], [1, 2]])
    for kw in (dict(num_hops=0), dict(num_hops=65), dict(node_cap=1), dict(z_max=-1), dict(batch_size=0), dict(prefetch=0),
               dict(chunk_cap=0), dict(edge_label_index=links[0]), dict(edge_label_index=links.to(torch.int32)),
               dict(edge_label_index=torch.tensor([[0, 3], [1, 2]])), dict(edge_label_index=torch.tensor([[0, 2], [1, 2]])),
               dict(edge_label=torch.ones(3))):
        with pytest.raises(ValueError):
            tch_geometric.SEALLoader(data, **dict(dict(edge_label_index=links, device="cuda:0"), **kw))
