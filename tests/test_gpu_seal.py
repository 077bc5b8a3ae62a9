"""tg_seal_nodes on the GPU: every output word equals the restatement (helpers_seal), with sentinels round every array and
behind every count; both forms on the same slots."""
import numpy as np
import pytest
import torch

import helpers_seal as hs
from test_seal_cpu import CYCLE5, CYCLE8, PATH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, HUB, SINK, ALONE, PATH0, RING0, PENT0 = 300, 7, 11, 299, 280, 286, 294
GUARD, MARK = 8, -7
BASE = dict(num_hops=2, node_cap=512, z_max=0, form=0)
NAMES = ("count", "nodes", "z", "du", "dv", "rounds")
# adjacent with parallel entries both ways, not adjacent, on the hub, the three hand links, between two components, one end
# isolated, u == v, an end at -1 and at n_major
LINKS = [(0, 1), (2, 250), (HUB, 3), (PATH0 + 2, PATH0 + 3), (RING0, RING0 + 1), (PENT0, PENT0 + 1), (PATH0 + 1, RING0 + 2),
         (ALONE, 5), (5, SINK), (4, 4), (-1, 3), (3, N), (-1, -1)]


def edges():
    rs = np.random.default_rng(6)
    ei = rs.integers(0, PATH0, (2, 700))
    ei = ei[:, (ei[0] != SINK)]
    parts = [ei, np.stack([np.full(1100, HUB), rs.integers(0, PATH0, 1100)]), [[0, 0, 0, 1, 1, 5], [1, 1, 1, 0, 0, SINK]]]
    for base, hand in ((PATH0, PATH), (RING0, CYCLE8), (PENT0, CYCLE5)):   # the hand graphs as components, both directions
        e = np.array(hand).T + base
        parts += [e, e[::-1]]
    return np.concatenate(parts, axis=1).astype(np.int64)


@pytest.fixture(scope="module")
def graphs():
    """-> {"csr" | "csc": (view, ptrs, indices)} of the multigraph, built by tg_coo_to_csx"""
    from tch_geometric import _cabi
    ei = torch.from_numpy(edges()).to(DEV)
    out = {}
    for name, csc in (("csr", False), ("csc", True)):
        tp, ti, _ = _cabi.coo_to_csx(ei[0], ei[1], N, N, csc)
        out[name] = (_cabi.graph_view(tp, ti), tp.cpu().numpy(), ti.cpu().numpy())
    _, ptrs, indices = out["csr"]
    deg = np.diff(ptrs)
    assert deg[HUB] > 4 * 256 and deg[SINK] == 0 and SINK in indices                 # a hub row, a sink,
    assert deg[ALONE] == 0 and ALONE not in indices                                  # an isolated vertex,
    assert hs.row(ptrs, indices, 0).count(1) == 3 and hs.row(ptrs, indices, 1).count(0) == 2   # parallel entries of (0, 1)
    return out


MEMO = {}


def reference(key, ptrs, indices, link, p):
    k = (key, link, p["num_hops"], p["node_cap"], p["z_max"])
    if k not in MEMO:
        MEMO[k] = hs.seal(ptrs, indices, link[0], link[1], p["num_hops"], p["node_cap"], p["z_max"])
    return MEMO[k]


def run(graph, links, key="g", optional=True, ws=None, **over):
    """one call against the restatement, word for word -> (the call's dict, the restatement's states)"""
    from tch_geometric import _cabi_seal as ops
    view, ptrs, indices = graph
    p = dict(BASE, **over)
    m, cap = len(links), p["node_cap"]
    names = NAMES if optional else NAMES[:3]
    whole, out = {}, {name: None for name in NAMES}
    for name in names:
        n = m * (cap if name in ops.ROWS else 1)
        whole[name] = torch.full((n + 2 * GUARD,), MARK, dtype=torch.int64, device=DEV)   # GUARD words before and behind
        out[name] = whole[name][GUARD:GUARD + n].view((m, cap) if name in ops.ROWS else (m,))
    at = torch.tensor(links, dtype=torch.int64, device=DEV).reshape(m, 2).t().contiguous()
    res = ops.seal_nodes(view, at[0], at[1], out=out, ws=ws, **p)
    got = {name: out[name].cpu().numpy() for name in names}
    states, status = [], 0
    for i, link in enumerate(links):
        st = reference(key, ptrs, indices, link, p)
        states.append(st)
        if "refused" in st:
            status |= st["refused"]
            assert got["count"][i] == 0
            assert all((got[name][i] == MARK).all() for name in names if name != "count"), (i, link)   # nothing else is written
            continue
        c = len(st["nodes"])
        assert got["count"][i] == c
        for name in names[1:]:
            if name == "rounds":
                assert got[name][i] == st[name], (i, link)
            else:
                assert got[name][i][:c].tolist() == st[name] and (got[name][i][c:] == MARK).all(), (name, i, link)
    assert int(res["status"].item()) == status
    for name in names:
        w = whole[name].cpu().numpy()
        assert (w[:GUARD] == MARK).all() and (w[-GUARD:] == MARK).all(), name
    return res, states


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("num_hops", [1, 2, 3])
def test_hops_and_every_kind_of_link_in_both_forms(graphs, form, num_hops):
    _, states = run(graphs["csr"], LINKS, num_hops=num_hops, form=form)
    assert [st.get("refused") for st in states[-4:]] == [4, 2, 2, 2] and len(states[2]["nodes"]) > 256   # the hub's link
    assert states[7]["nodes"][0] == ALONE and states[7]["du"][2:] == [-1] * (len(states[7]["nodes"]) - 2)


@pytest.mark.parametrize("form", [1, 2])
def test_cap_below_at_and_above_a_link_s_node_count(graphs, form):
    c = len(reference("g", graphs["csr"][1], graphs["csr"][2], (HUB, 3), BASE)["nodes"])
    assert c > 64
    small = (PATH0 + 2, PATH0 + 3)
    for cap, refused in ((c - 1, True), (c, False), (c + 1, False)):
        _, states = run(graphs["csr"], [small, (HUB, 3), small, (HUB, 3), small], node_cap=cap, form=form)   # the neighbours stay
        assert [("refused" in st) for st in states] == [False, refused, False, refused, False]


@pytest.mark.parametrize("cap", [512, 513, 2048, 2049])
def test_the_cap_at_each_table_size_and_one_past_the_last(graphs, cap):
    from tch_geometric import _cabi_seal as ops
    assert ops.Seal.workspace_bytes(len(LINKS), cap)[1] == (1 if cap <= 2048 else 2)
    run(graphs["csr"], LINKS, node_cap=cap, z_max=3)


@pytest.mark.parametrize("m, over", [(0, {}), (1, {}), (63, {}), (64, {}), (65, dict(form=2)), (1025, dict(node_cap=513)),
                                     (1025, dict(form=2))], ids=str)
def test_slot_counts_up_to_past_the_grid(graphs, m, over):
    run(graphs["csr"], [LINKS[(3 * i) % len(LINKS)] for i in range(m)], **over)   # 1 025: past 512 and past 128 workgroups


def test_views_shadows_null_outputs_and_a_second_call_over_the_workspace(graphs):   # a non-default stream: test_gpu_stream_order_seal.py
    from tch_geometric import _cabi
    run(graphs["csc"], LINKS, key="csc", num_hops=3)
    view = graphs["csr"][0]
    small = _cabi.graph_view(*view._keep[:2], indices32=view._keep[1].to(torch.int32), ptrs32=view._keep[0].to(torch.int32))
    run((small,) + graphs["csr"][1:], LINKS, num_hops=3)
    res, _ = run(graphs["csr"], LINKS, optional=False, form=2)
    run(graphs["csr"], LINKS[::-1], form=2, ws=res["ws"], num_hops=3)   # the tables of the first call were left clean
