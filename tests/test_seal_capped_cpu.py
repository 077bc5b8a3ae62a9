"""tg_seal_nodes_capped without a GPU: the restatement (helpers_seal_capped) against a brute-force selection on hand graphs,
with a vertex dropped at hop 1 and found again at hop 2, and against helpers_seal when no cap binds; every refusal happens
before a launch; the workspace query; the header is C99 and the exports equal it; the loader's ValueErrors."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import helpers_seal as hs
import helpers_seal_capped as hc
from helpers_labor import named_draw
from test_seal_cpu import BIG, FAKE, HAND, REFUSALS as SEAL_REFUSALS, ROOT, symmetric_csr

HEADER = os.path.join(ROOT, "include", "tchgeo_seal_capped.h")
TWIN = [(0, 2), (0, 3), (2, 3), (1, 4)]      # link (0, 1), cap 1: whichever of 2 and 3 is dropped is the other's neighbour
SEED = 0x5EA1


def brute(ptrs, indices, u, v, caps, seed, call_id):
    """the node set with every key drawn on its own and every vertex of the graph asked whether it is in the fringe"""
    N, S = {u, v}, {u, v}
    for t, k in enumerate(caps, 1):
        F = [y for y in range(len(ptrs) - 1) if y not in N and any(y in hs.row(ptrs, indices, x) for x in S)]
        if 0 < k < len(F):
            w = {y: named_draw(seed, call_id, 19, y, t, 0) for y in F}
            F = sorted(F, key=lambda y: ((int(w[y][1]) << 32) | int(w[y][0]), y))[:k]
        N, S = N | set(F), set(F)
    return N


def test_restatement_against_brute_force_and_a_vertex_found_again():
    again = 0
    for (ptrs, indices), (u, v) in [(symmetric_csr(TWIN, 5), (0, 1))] + [(symmetric_csr(e, n), link) for e, n, link, *_ in HAND]:
        for caps in ([1], [1, 0], [2, 1], [1, 1, 1]):
            for call_id in range(6):
                N, cut = hc.node_set(ptrs, indices, u, v, caps, SEED, call_id)
                assert N == brute(ptrs, indices, u, v, caps, SEED, call_id) and len(N) <= 2 + sum(k or 99 for k in caps)
                first = hc.node_set(ptrs, indices, u, v, caps[:1], SEED, call_id)[0]
                again += len(ptrs) == 6 and caps == [1, 0] and first in ({0, 1, 2}, {0, 1, 3}) and N == {0, 1, 2, 3} and cut == 1
    assert again > 0                                         # TWIN: dropped at hop 1, found again at hop 2


@pytest.mark.parametrize("edges, n, link, h, nodes, z, du, dv, rounds", HAND)
def test_caps_above_every_fringe_give_the_exhaustive_rule(edges, n, link, h, nodes, z, du, dv, rounds):
    ptrs, indices = symmetric_csr(edges, n)
    for caps in ([n] * h, [0] * h):
        got = hc.seal_capped(ptrs, indices, *link, caps, n, SEED, 3, z_max=3)
        assert got.pop("cut") == 0 and got == hs.seal(ptrs, indices, *link, h, n, z_max=3)
    assert hc.seal_capped(ptrs, indices, *link, [n] * h, len(nodes) - 1, SEED, 3) == dict(refused=1)
    assert hc.seal_capped(ptrs, indices, link[0], n, [1] * h, n, SEED, 3) == dict(refused=2)
    assert hc.seal_capped(ptrs, indices, 1, 1, [1] * h, n, SEED, 3) == dict(refused=4)


@pytest.fixture(scope="module")
def ops():
    from tch_geometric import _cabi_seal_capped
    _cabi_seal_capped.lib.tg_last_error.restype = C.c_char_p
    return _cabi_seal_capped


def call(ops, hops=(4, 0), caps="default", g="default", inp="default", out="default", m=4, form=0, ws=FAKE, ws_bytes=BIG,
         status=FAKE, **kw):
    """test_seal_cpu's call with the caps: every keyword of its REFUSALS means here what it means there"""
    from tch_geometric import _cabi, _cabi_seal
    if g == "default":
        g = _cabi.TgGraph()
        g.ptrs, g.indices, g.n_major, g.n_edges = kw.pop("ptrs", FAKE), FAKE, kw.pop("n_major", 100), 500
    if inp == "default":
        inp = _cabi_seal.TgSealIn(*(kw.pop(n, d) for n, d in (("src", FAKE), ("dst", FAKE), ("num_hops", 2), ("node_cap", 100), ("z_max", 0))))
    if out == "default":
        out = _cabi_seal.TgSealOut(*(kw.pop(name, FAKE) for name in ("count", "nodes", "z")))
    keep = (C.c_int32 * 64)(*hops)           # a host array, read before the call returns
    if caps == "default":
        caps = ops.TgSealCaps(C.cast(keep, C.c_void_p) if hops else None, 1, None, 0, None)
    assert not kw, kw
    ref = lambda s: C.byref(s) if s is not None else None
    return ops.lib.tg_seal_nodes_capped(ref(g), ref(inp), ref(caps), ref(out), m, form, status, ws, ws_bytes, None)


REFUSALS = SEAL_REFUSALS + [                 # everything tg_seal_nodes refuses, and the caps
    (dict(caps=None), "null caps"), (dict(hops=()), "null caps"), (dict(hops=(4, -1)), "cap of -1"),
    (dict(hops=(1025, 0)), "cap of 1025"), (dict(hops=(0, 0, 2000), num_hops=3), "cap of 2000")]


@pytest.mark.parametrize("kw, word", REFUSALS)
def test_refusals_before_any_launch(ops, kw, word):
    assert call(ops, **kw) == 1                              # TG_ERR_INVALID
    assert re.search(word, ops.lib.tg_last_error().decode()), ops.lib.tg_last_error()


def test_empty_calls_the_workspace_query_and_the_binding_s_own_refusals(ops):
    from tch_geometric import _cabi_seal
    assert call(ops, n_major=(1 << 31) + 1) == 3             # TG_ERR_UNSUPPORTED
    assert call(ops, m=0, src=None, count=None, status=None, ws=None, ws_bytes=0, node_cap=4096) == 0   # launches nothing
    for m in (0, 1, 129):
        for cap in (2, 512, 2048, 2049, 1 << 20):
            for form in (0, 2):
                for k in (0, 1, 1024):                       # tg_seal_nodes' formula and form at every cap of a hop
                    assert ops.workspace_bytes(m, cap, k, form) == _cabi_seal.Seal.workspace_bytes(m, cap, form)
    for bad in (dict(max_cap=-1), dict(max_cap=1025), dict(node_cap=1), dict(form=1, node_cap=2049)):
        with pytest.raises(RuntimeError):
            ops.workspace_bytes(**dict(dict(m=4, node_cap=100, max_cap=4, form=0), **bad))
    assert ops.hop_caps(7, 3) == [7, 7, 7] and ops.hop_caps((1, 0), 2) == [1, 0]
    for bad in (-1, 1025, [1], [1, 2, 3], 1.5, True, [1, None]):
        with pytest.raises(ValueError):
            ops.hop_caps(bad, 2)
    assert [ops.pool_cap(k) for k in (1, 256, 257, 512, 513, 1024)] == [512, 512, 1024, 1024, 2048, 2048]


def test_header_is_c99_and_the_exports_equal_it(ops):
    src = ('#include "tchgeo_seal_capped.h"\nint main(void) { tg_seal_caps c; c.seed = TG_TAG_SEAL_HOP; return '
           'TG_SEAL_POOL_CAP(1) == 512 && TG_SEAL_POOL_CAP(1024) == 2048 && TG_SEAL_HOP_CAP_MAX == 1024 && c.seed == 19 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-x", "c", "-",
                    "-o", os.devnull], input=src.encode(), check=True)
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"TG_API\s+[\w\s\*]+?\b(tg_\w+)\s*\(", text)
    assert sorted(declared) == sorted(ops.EXPORTS) == ["tg_seal_capped_workspace_bytes", "tg_seal_nodes_capped"]
    for name in declared:
        assert hasattr(ops.lib, name) and getattr(ops.lib, name).argtypes
    assert [f for f, _ in ops.TgSealCaps._fields_] == ["max_per_hop", "seed", "call_ids", "call_id0", "cut"]
    assert ops.TAG_SEAL_HOP == hc.TAG_SEAL_HOP == 19 and ops.SEAL_HOP_CAP_MAX == 1024


def test_the_loader_refuses_bad_caps_before_any_device_work():
    import tch_geometric
    from tch_geometric.transforms import Graph
    data = Graph(edge_index=torch.tensor([[0, 1, 2], [1, 2, 0]]), num_nodes=3)
    links = torch.tensor([[0, 1], [1, 2]])
    for bad in (-1, 1025, [4], [4, 4, 4], 2.5, "8"):
        with pytest.raises(ValueError):
            tch_geometric.SEALLoader(data, links, num_hops=2, device="cuda:0", max_nodes_per_hop=bad)
