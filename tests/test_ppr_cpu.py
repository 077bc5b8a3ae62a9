"""tg_ppr_topk without a GPU: the restatement (helpers_ppr) keeps the header's two properties against a float64 dense solve;
every refusal happens before a launch; the workspace formula; the header is C99; the exports equal the header."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import helpers_ppr as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tchgeo_ppr.h")
FAKE, BIG = 0x10000, 1 << 50   # a non-null address that is never read: every call below is refused before a launch


@pytest.fixture(scope="module")
def ops():
    from tch_geometric import _cabi_ppr
    _cabi_ppr.lib.tg_last_error.restype = C.c_char_p
    return _cabi_ppr


def exact_ppr(ptrs, indices, alpha):
    """alpha (I - (1 - alpha) P^T)^-1 with a self loop at every empty row: column s is ppr_s"""
    n = len(ptrs) - 1
    Pm = np.zeros((n, n))
    for v in range(n):
        row = indices[ptrs[v]:ptrs[v + 1]]
        if len(row) == 0:
            Pm[v, v] = 1.0
        for t in row:
            Pm[v, t] += 1.0 / len(row)
    return alpha * np.linalg.inv(np.eye(n) - (1.0 - alpha) * Pm.T)


def small_graph(n, sink):
    rs = np.random.default_rng(n)
    rows = [sorted(rs.integers(0, n, rs.integers(1, 6)).tolist()) for _ in range(n)]   # parallel entries and self loops happen
    if sink:
        rows[3] = []
    ptrs = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return ptrs, np.array([t for r in rows for t in r], dtype=np.int64)


@pytest.mark.parametrize("n, sink", [(40, True), (33, False)])
@pytest.mark.parametrize("alpha_q, eps_q, max_rounds", [(644245094, 1, 65536), (1 << 31, 1 << 12, 64), (644245094, 1 << 20, 3)])
def test_restatement_conserves_mass_and_stays_inside_the_bound(n, sink, alpha_q, eps_q, max_rounds):
    ptrs, indices = small_graph(n, sink)
    exact = exact_ppr(ptrs, indices, alpha_q / 2.0 ** 32)
    for seed in (0, 3, n - 1):
        for rounds in (1, max_rounds):                      # conservation after the first round as after the last
            st = hp.push(ptrs, indices, seed, alpha_q, eps_q, rounds, n)
            assert st["mass"] + st["residual"] == hp.U and st["touched"] == len(st["p"]) <= n
        assert st["rounds"] <= max_rounds and st["activations"] >= st["rounds"]
        for v in range(n):
            gap = hp.U * exact[v, seed] - st["p"].get(v, 0)
            assert -st["activations"] - 1e-3 <= gap <= st["residual"] + st["activations"] + 1e-3, (seed, v)   # 1e-3: the solve
    assert hp.push(ptrs, indices, 0, alpha_q, eps_q, max_rounds, 1) == dict(refused=1)
    assert hp.push(ptrs, indices, n, alpha_q, eps_q, max_rounds, n) == dict(refused=2)


def call(ops, g="default", n_major=100, inp="default", out="default", m=4, form=0, status=FAKE, ws=FAKE, ws_bytes=BIG, **kw):
    from tch_geometric import _cabi
    if g == "default":
        g = _cabi.TgGraph()
        g.ptrs, g.indices, g.n_major, g.n_edges = kw.pop("ptrs", FAKE), FAKE, n_major, 500
    if inp == "default":
        inp = ops.TgPprIn(kw.pop("seeds", FAKE), kw.pop("alpha_q", 1 << 30), kw.pop("eps_q", 1 << 10), kw.pop("max_rounds", 8),
                          kw.pop("k", 4), kw.pop("node_cap", 100))
    if out == "default":
        out = ops.TgPprOut(*(kw.pop(name, FAKE) for name in ("count", "nodes", "score")))   # the optional outputs stay NULL
    assert not kw, kw
    ref = lambda s: C.byref(s) if s is not None else None
    return ops.lib.tg_ppr_topk(ref(g), ref(inp), ref(out), m, form, status, ws, ws_bytes, None)


WS_BYTES = 4 * (16 * 8192 + 4096 * 4)   # node_cap 4096, m = 4
REFUSALS = [
    (dict(g=None), "null graph"), (dict(inp=None), "null graph"), (dict(out=None), "null graph"),
    (dict(m=-1), "m = -1"), (dict(m=1 << 31), "m = "),
    (dict(node_cap=0), "node_cap = 0"), (dict(node_cap=(1 << 20) + 1), "node_cap"),
    (dict(k=0), "k = 0"), (dict(k=101), "k = 101"),
    (dict(form=3), "unknown form"), (dict(form=-1), "unknown form"), (dict(form=1, node_cap=2049), "LDS form"),
    (dict(alpha_q=0), "alpha_q"), (dict(eps_q=0), "eps_q"), (dict(eps_q=(1 << 31) + 1), "eps_q"),
    (dict(max_rounds=0), "max_rounds"), (dict(max_rounds=65537), "max_rounds"),
    (dict(n_major=-1), "negative graph"), (dict(ws_bytes=-1), "workspace_bytes"),
    (dict(ptrs=None), "null graph arrays"), (dict(seeds=None), "null seeds"), (dict(count=None), "null seeds"),
    (dict(nodes=None), "null seeds"), (dict(score=None), "null seeds"), (dict(status=None), "null seeds"),
    (dict(node_cap=4096, ws=None), "workspace"), (dict(node_cap=4096, ws_bytes=WS_BYTES - 1), "workspace"),
    (dict(node_cap=4096, ws=FAKE + 4), "8-byte aligned"), (dict(form=2, ws_bytes=4 * (16 * 1024 + 512) - 1), "workspace"),
]


@pytest.mark.parametrize("kw, word", REFUSALS)
def test_refusals_before_any_launch(ops, kw, word):
    assert call(ops, **kw) == 1                              # TG_ERR_INVALID
    assert re.search(word, ops.lib.tg_last_error().decode()), ops.lib.tg_last_error()


def test_unsupported_ids_empty_calls_and_the_binding_s_own_refusals(ops):
    assert call(ops, n_major=(1 << 31) + 1) == 3             # TG_ERR_UNSUPPORTED
    assert call(ops, m=0, seeds=None, count=None, status=None, ws=None, ws_bytes=0, node_cap=4096) == 0   # launches nothing
    for kw in (dict(k=0, node_cap=4), dict(k=5, node_cap=4), dict(k=1, node_cap=0), dict(k=1, node_cap=4, alpha_q=0),
               dict(k=1, node_cap=4, eps_q=0), dict(k=1, node_cap=4, max_rounds=0), dict(k=1, node_cap=2049, form=1)):
        with pytest.raises(ValueError):
            ops.PPR(**kw)
    assert (ops.alpha_to_q(0.15), ops.alpha_to_q(0.0), ops.alpha_to_q(1.0)) == (644245094, 1, 2 ** 32 - 1)
    assert (ops.eps_to_q(1e-4), ops.eps_to_q(0.0)) == (214748, 1)


def test_workspace_formula(ops):
    r256 = lambda x: (x + 255) & ~255
    for m in (0, 1, 127, 128, 129, 5000):
        for cap in (1, 512, 513, 2048, 2049, 4096, 4097, 1 << 20):
            for form in (0, 2):
                T = 1024
                while T < 2 * cap:
                    T *= 2
                lds = form == 0 and cap <= ops.PPR_LDS_CAP
                want = 0 if lds else min(m, ops.PPR_WS_GROUPS) * (16 * T + r256(4 * cap))
                assert ops.PPR.workspace_bytes(m, 1, cap, form) == (want, 1 if lds else 2), (m, cap, form)
    assert ops.PPR.workspace_bytes(4, 1, 4096) == (WS_BYTES, 2) and ops.PPR.workspace_bytes(9, 9, 2048, 1) == (0, 1)


def test_header_is_c99_and_the_exports_equal_it(ops):
    src = '#include "tchgeo_ppr.h"\nint main(void) { tg_ppr_in i; tg_ppr_out o; i.k = TG_PPR_LDS_CAP; (void)o; return i.k == 2048 ? 0 : 1; }\n'
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    "-x", "c", "-"], input=src.encode(), check=True)
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"TG_API\s+[\w\s\*]+?\b(tg_\w+)\s*\(", text)
    assert sorted(declared) == sorted(ops.EXPORTS) == ["tg_ppr_topk", "tg_ppr_workspace_bytes"]
    for name in declared:
        assert hasattr(ops.lib, name) and getattr(ops.lib, name).argtypes
    assert [f for f, _ in ops.TgPprOut._fields_] == ["count", "nodes", "score", "weight"] + list(ops.DIAGNOSTICS)
