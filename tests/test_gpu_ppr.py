"""tg_ppr_topk on the GPU: every output word equals the restatement (helpers_ppr), with sentinels round every array and behind
every count; both forms on the same input; one float case against the float64 solve inside the header's bound."""
import numpy as np
import pytest
import torch

import helpers_ppr as hp
from helpers_saint import random_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, HUB, SINK, ALONE = 300, 7, 11, 13
A15, GUARD, MARK = 644245094, 8, -7      # round(0.15 * 2^32)
BASE = dict(k=8, node_cap=512, alpha_q=A15, eps_q=1 << 20, max_rounds=64, form=0)
POOL = [HUB, SINK, ALONE, 0, 1, 2, 5, 17, 100, 299]


def csr(ei, n):
    order = np.lexsort((ei[1], ei[0]))
    ptrs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(ei[0], minlength=n), out=ptrs[1:])
    return ptrs, ei[1][order].astype(np.int64)


def edges():
    ei = random_graph(N, 2000, seed=4)
    ei = ei[:, (ei[0] != SINK) & (ei[0] != ALONE)]
    rs = np.random.default_rng(5)
    ei = np.concatenate([ei, np.stack([np.full(1100, HUB), rs.integers(0, N, 1100)]), [[0, 1], [SINK, SINK]]], axis=1)
    return ei[:, ei[1] != ALONE].astype(np.int64)


@pytest.fixture(scope="module")
def graphs():
    """-> {"csr" | "csc": (view, ptrs, indices)} of the multigraph: a hub row, a sink with in-edges, an isolated vertex"""
    from tch_geometric import _cabi
    ei = edges()
    out = {}
    for name, e in (("csr", ei), ("csc", ei[::-1])):
        ptrs, indices = csr(e, N)
        tp, ti = torch.from_numpy(ptrs).to(DEV), torch.from_numpy(indices).to(DEV)
        out[name] = (_cabi.graph_view(tp, ti), ptrs, indices)
    ptrs = out["csr"][1]
    assert ptrs[HUB + 1] - ptrs[HUB] > 4 * 256 and ptrs[SINK + 1] == ptrs[SINK] and ptrs[ALONE + 1] == ptrs[ALONE]
    assert SINK in out["csr"][2] and ALONE not in out["csr"][2] and len(set(zip(*ei.tolist()))) < ei.shape[1]   # parallel entries
    return out


MEMO = {}


def reference(key, ptrs, indices, seed, p):
    k = (key, seed, p["alpha_q"], p["eps_q"], p["max_rounds"], p["node_cap"])
    if k not in MEMO:
        MEMO[k] = hp.push(ptrs, indices, seed, p["alpha_q"], p["eps_q"], p["max_rounds"], p["node_cap"])
    return MEMO[k]


def guarded(shape, dtype):
    """a tensor of MARKs with GUARD words before and behind the part handed to the library"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), MARK, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + n].view(shape)


def run(graph, seeds, key="g", optional=True, **over):
    """one call against the restatement, word for word -> (the call's dict as numpy, the restatement's states)"""
    from tch_geometric import _cabi_ppr as ops
    view, ptrs, indices = graph
    p = dict(BASE, **over)
    m, k = len(seeds), p["k"]
    names = ("count", "nodes", "score") + ((("weight",) + ops.DIAGNOSTICS) if optional else ())
    whole, out = {}, {name: None for name in ("weight",) + ops.DIAGNOSTICS}
    for name in names:
        shape = (m, k) if name in ("nodes", "score", "weight") else (m,)
        whole[name], out[name] = guarded(shape, torch.float32 if name == "weight" else torch.int64)
    res = ops.ppr_topk(view, torch.tensor(seeds, dtype=torch.int64, device=DEV), out=out, **p)
    got = {name: out[name].cpu().numpy() for name in names}
    states, status = [], 0
    for i, s in enumerate(seeds):
        st = reference(key, ptrs, indices, s, p)
        states.append(st)
        if "refused" in st:
            status |= st["refused"]
            assert got["count"][i] == 0
            assert all((got[name][i] == MARK).all() for name in names if name != "count"), (i, s)   # nothing else is written
            continue
        nodes, score = hp.top(st, s, k)
        c = len(nodes)
        assert got["count"][i] == c and c == min(k, 1 + sum(1 for v, pv in st["p"].items() if v != s and pv > 0))
        assert got["nodes"][i][:c].tolist() == nodes and got["score"][i][:c].tolist() == score, (i, s)
        assert (got["nodes"][i][c:] == MARK).all() and (got["score"][i][c:] == MARK).all()
        if optional:
            assert np.array_equal(got["weight"][i][:c], np.array(score, dtype=np.float32) * np.float32(2.0 ** -31))
            assert (got["weight"][i][c:] == MARK).all()
            assert [int(got[name][i]) for name in ops.DIAGNOSTICS] == [st[name] for name in ops.DIAGNOSTICS], (i, s)
            assert st["mass"] + st["residual"] == hp.U
    assert int(res["status"].item()) == status
    for name in names:
        w = whole[name].cpu().numpy()
        assert (w[:GUARD] == MARK).all() and (w[-GUARD:] == MARK).all(), name
    return got, states


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("k", [1, 3, 64, 65, 400])
def test_k_on_both_sides_of_the_two_selections_in_both_forms(graphs, form, k):
    got, states = run(graphs["csr"], POOL, k=k, form=form)
    assert 64 < max(st["touched"] for st in states) < 400 and got["count"].max() <= k


@pytest.mark.parametrize("form", [1, 2])
def test_cap_below_at_and_above_a_slot_s_touched_count(graphs, form):
    tc = reference("g", graphs["csr"][1], graphs["csr"][2], 5, BASE)["touched"]
    assert tc > 64
    for cap, refused in ((tc - 1, True), (tc, False), (tc + 1, False)):
        _, states = run(graphs["csr"], [SINK, 5, ALONE, 5, SINK], node_cap=cap, form=form)   # the neighbours stay intact
        assert [("refused" in st) for st in states] == [False, refused, False, refused, False]


@pytest.mark.parametrize("cap", [512, 513, 2048, 2049])
def test_the_cap_at_each_table_size_and_one_past_the_last(graphs, cap):
    from tch_geometric import _cabi_ppr as ops
    assert ops.PPR.workspace_bytes(len(POOL), 8, cap)[1] == (1 if cap <= 2048 else 2)
    run(graphs["csr"], POOL, node_cap=cap)


@pytest.mark.parametrize("over", [dict(max_rounds=1), dict(max_rounds="one short"), dict(alpha_q=1 << 31), dict(alpha_q=2 ** 32 - 1),
                                  dict(eps_q=1, max_rounds=65536)], ids=str)
def test_rounds_alpha_and_eps(graphs, over):
    if over.get("max_rounds") == "one short":
        over = dict(max_rounds=reference("g", graphs["csr"][1], graphs["csr"][2], 5, BASE)["rounds"] - 1)
    got, states = run(graphs["csr"], POOL, **over)
    if over.get("alpha_q") == 2 ** 32 - 1:                   # q = 0 on every row: nothing but a seed without one is active
        rows = np.array([s not in (SINK, ALONE) for s in POOL])
        assert (got["count"] == 1).all() and (got["score"][rows, 0] == 0).all() and (got["rounds"][rows] == 0).all()
        assert (got["score"][~rows, 0] == hp.U).all() and (got["rounds"][~rows] == 1).all()
    if "max_rounds" in over and over["max_rounds"] < 100:
        assert states[6]["rounds"] == over["max_rounds"] == got["rounds"][6]   # seed 5


def test_a_star_whose_leaves_tie_is_ordered_by_id():
    from tch_geometric import _cabi
    leaves = [9, 2, 7, 4, 5, 3, 8, 6, 1]
    ptrs, indices = np.array([0, 9] + [9] * 9, dtype=np.int64), np.array(leaves, dtype=np.int64)
    view = _cabi.graph_view(torch.from_numpy(ptrs).to(DEV), torch.from_numpy(indices).to(DEV))
    for form in (1, 2):
        got, _ = run((view, ptrs, indices), [0, 3], key="star", k=6, form=form)
        assert got["nodes"][0].tolist() == [0, 1, 2, 3, 4, 5] and len(set(got["score"][0][1:].tolist())) == 1
        assert got["count"].tolist() == [6, 1]


def test_seeds_on_the_sink_the_isolated_vertex_and_out_of_range(graphs):
    got, states = run(graphs["csr"], [SINK, -1, ALONE, N, 0, 2 ** 40])
    assert got["count"].tolist()[:4] == [1, 0, 1, 0] and got["score"][0, 0] == got["score"][2, 0] == hp.U
    assert got["weight"][0, 0] == 1.0 and [st.get("refused") for st in states] == [None, 2, None, 2, None, 2]


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 1025])
def test_slot_counts(graphs, m):
    run(graphs["csr"], [POOL[(3 * i) % len(POOL)] for i in range(m)], form=2 if m == 65 else 0)


def test_views_shadows_and_null_outputs(graphs):   # a non-default stream: tests/test_gpu_stream_order_ppr.py
    from tch_geometric import _cabi
    run(graphs["csc"], POOL, key="csc", k=65)
    view = graphs["csr"][0]
    small = _cabi.graph_view(*view._keep[:2], indices32=view._keep[1].to(torch.int32), ptrs32=view._keep[0].to(torch.int32))
    run((small,) + graphs["csr"][1:], POOL, k=65)
    run(graphs["csr"], POOL, optional=False, form=2)


def test_weight_against_the_float64_solve_inside_the_bound(graphs):
    from test_ppr_cpu import exact_ppr
    _, ptrs, indices = graphs["csr"]
    got, states = run(graphs["csr"], [5], k=400)             # residual and activations are asserted equal in there
    exact = exact_ppr(ptrs, indices, A15 / 2.0 ** 32)[:, 5]
    A, R, c = states[0]["activations"], states[0]["residual"], got["count"][0]
    assert got["activations"][0] == A and got["residual"][0] == R and c > 64
    gap = exact[got["nodes"][0][:c]] - got["weight"][0][:c].astype(np.float64)
    slack = 2.0 ** -24 + 1e-9                                # the one float32 conversion of p / U <= 1; the solve
    assert (gap >= -A / hp.U - slack).all() and (gap <= (R + A) / hp.U + slack).all()
