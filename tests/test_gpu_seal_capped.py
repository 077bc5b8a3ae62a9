"""tg_seal_nodes_capped on the GPU: every output word, `cut` included, equals the restatement (helpers_seal_capped), with
sentinels round every array and behind every count; the forms on the same slots; the kept pair against the uniform law."""
import numpy as np
import pytest
import torch

import exact_laws
import helpers_seal as hs
import helpers_seal_capped as hc
from test_gpu_seal import ALONE, GUARD, HUB, LINKS, MARK, PATH0, graphs  # noqa: F401  (graphs: the fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0xCA99ED
NAMES = ("count", "nodes", "z", "du", "dv", "rounds", "cut")
KS = (1, 2, 64, 100, 1024)
P, W = 2100, 40                              # the fan: targets 0 .. P - 1, their shared neighbours P .. P + W - 1, then the hubs


def pool_cap(k):
    from tch_geometric import _cabi_seal_capped
    return _cabi_seal_capped.pool_cap(k)


@pytest.fixture(scope="module")
def fan():
    """-> (view, ptrs, indices, {size: hub}, sink): a hub per size s whose row is s distinct targets, 70 of them twice, and a
    self loop; every target has two of the W shared neighbours, every shared neighbour six targets; the sink's row is empty"""
    from tch_geometric import _cabi
    rows = {p: [P + p % W, P + (3 * p + 1) % W] for p in range(P)}
    rows.update({P + w: [(w * 53 + j * 211) % P for j in range(6)] for w in range(W)})
    sizes = sorted({s for k in KS for c in (k, pool_cap(k)) for s in (c - 1, c, c + 1)} | {20})
    hub = {s: P + W + i for i, s in enumerate(sizes)}
    rows.update({h: list(range(s)) + list(range(min(s, 70))) + [h] for s, h in hub.items()})
    sink = P + W + len(hub)
    ei = torch.tensor([[x, y] for x, r in rows.items() for y in r], dtype=torch.int64, device=DEV).t().contiguous()
    tp, ti, _ = _cabi.coo_to_csx(ei[0], ei[1], sink + 1, sink + 1, False)
    ptrs, indices = tp.cpu().numpy(), ti.cpu().numpy()
    for k in KS:                             # at least one compaction at every k: more distinct new vertices than the pool lists
        assert len(set(hs.row(ptrs, indices, hub[pool_cap(k) + 1])) - {hub[pool_cap(k) + 1]}) == pool_cap(k) + 1 > pool_cap(k)
    return _cabi.graph_view(tp, ti), ptrs, indices, hub, sink


MEMO = {}


def run(graph, links, caps, key="g", call_ids=None, call_id0=0, optional=True, ws=None, node_cap=512, z_max=0, form=0):
    """one call against the restatement, word for word -> (the call's dict, the restatement's states, the arrays)"""
    from tch_geometric import _cabi_seal, _cabi_seal_capped as ops
    view, ptrs, indices = graph[:3]
    m, cap = len(links), node_cap
    names = NAMES if optional else NAMES[:3]
    whole, out = {}, {name: None for name in NAMES}
    for name in names:
        n = m * (cap if name in _cabi_seal.ROWS else 1)
        whole[name] = torch.full((n + 2 * GUARD,), MARK, dtype=torch.int64, device=DEV)   # GUARD words before and behind
        out[name] = whole[name][GUARD:GUARD + n].view((m, cap) if name in _cabi_seal.ROWS else (m,))
    at = torch.tensor(links, dtype=torch.int64, device=DEV).reshape(m, 2).t().contiguous()
    ids = None if call_ids is None else torch.tensor(call_ids, dtype=torch.int64, device=DEV)
    res = ops.seal_nodes_capped(view, at[0], at[1], _cabi_seal.Seal(len(caps), cap, z_max, form), list(caps), SEED,
                                call_ids=ids, call_id0=call_id0, out=out, ws=ws)
    got = {name: out[name].cpu().numpy() for name in names}
    states, status = [], 0
    for i, link in enumerate(links):
        c_i = call_id0 + i if call_ids is None else call_ids[i]
        k = (key, tuple(link), tuple(caps), cap, z_max, c_i)
        if k not in MEMO:
            MEMO[k] = hc.seal_capped(ptrs, indices, link[0], link[1], caps, cap, SEED, c_i, z_max)
        st = MEMO[k]
        states.append(st)
        if "refused" in st:
            status |= st["refused"]
            assert got["count"][i] == 0 and (not optional or got["cut"][i] == 0)
            assert all((got[name][i] == MARK).all() for name in names if name not in ("count", "cut")), (i, link)
            continue
        c = len(st["nodes"])
        assert got["count"][i] == c, (i, link, got["count"][i], c)
        for name in names[1:]:
            if name in ("rounds", "cut"):
                assert got[name][i] == st[name], (name, i, link)
            else:
                assert got[name][i][:c].tolist() == st[name] and (got[name][i][c:] == MARK).all(), (name, i, link)
    assert int(res["status"].item()) == status
    for name in names:
        w = whole[name].cpu().numpy()
        assert (w[:GUARD] == MARK).all() and (w[-GUARD:] == MARK).all(), name
    return res, states, got


@pytest.mark.parametrize("form, node_cap", [(1, 512), (1, 2048), (2, 2048)])
@pytest.mark.parametrize("k", KS)
def test_fringes_round_every_cap_and_every_pool_size(fan, k, form, node_cap):
    hub, sink = fan[3], fan[4]
    ss = [s for c in (k, pool_cap(k)) for s in (c - 1, c, c + 1)]
    links = [(hub[s], sink) for s in ss] + [(sink, hub[3]), (-1, 3), (5, 5), (3, sink + 1)]
    _, states, _ = run(fan, links, [k, k], key="fan", node_cap=node_cap, form=form)
    assert all((st["cut"] & 1) == (s > k) for st, s in zip(states, ss) if "refused" not in st)
    assert [("refused" in st) for st in states[:3]] == [k + 1 > node_cap] * 3      # 2 + k and at least one of the second hop


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("caps", [[5], [0, 4], [8, 0], [3, 0, 2], [64, 1, 1024]], ids=str)
def test_hops_differing_caps_and_every_kind_of_link(graphs, fan, form, caps):  # noqa: F811
    _, states, _ = run(graphs["csr"], LINKS, caps, form=form)
    assert [st.get("refused") for st in states[-4:]] == [4, 2, 2, 2] and (states[2]["cut"] & 1) == (caps[0] > 0)   # the hub's link
    assert states[7]["nodes"][0] == ALONE
    run(fan, [(fan[3][513], fan[4]), (fan[3][2049], fan[3][100])], caps, key="fan", form=form, node_cap=2048, z_max=3)


@pytest.mark.parametrize("form", [1, 2])
def test_node_cap_below_at_and_above_a_link_s_node_count(graphs, form):  # noqa: F811
    small, big = (PATH0 + 2, PATH0 + 3), (HUB, 3)
    links, ids = [small, big, small, big, small], [0, 9, 1, 9, 2]
    c = len(run(graphs["csr"], links, [40, 30], call_ids=ids, form=form)[1][1]["nodes"])
    assert 42 < c <= 72
    for cap, refused in ((c - 1, True), (c, False), (c + 1, False)):
        _, states, _ = run(graphs["csr"], links, [40, 30], call_ids=ids, node_cap=cap, form=form)   # the neighbours stay
        assert [("refused" in st) for st in states] == [False, refused, False, refused, False]


@pytest.mark.parametrize("form, node_cap", [(1, 512), (1, 513), (2, 512)])
def test_call_ids_and_a_slot_past_the_grid(fan, form, node_cap):
    hub, sink = fan[3], fan[4]
    link = (hub[513], hub[2049])
    _, _, one = run(fan, [link], [100, 7], key="fan", call_ids=[77], node_cap=node_cap, form=form)
    _, _, off = run(fan, [link] * 3, [100, 7], key="fan", call_id0=76, node_cap=node_cap, form=form)
    links = [((hub[513], sink), link, (sink, sink), (hub[1025], hub[2]))[i % 4] for i in range(1024)] + [link]
    _, _, many = run(fan, links, [100, 7], key="fan", call_ids=[i % 4 for i in range(1024)] + [77], node_cap=node_cap, form=form)
    for name in NAMES:                       # the same (link, call id): slot 0 of 1, slot 1 of 3, slot 1 024 of 1 025
        assert np.array_equal(one[name][0], many[name][1024]) and np.array_equal(one[name][0], off[name][1]), name


def test_views_shadows_null_outputs_and_a_second_call_over_the_workspace(graphs):  # noqa: F811
    from tch_geometric import _cabi
    run(graphs["csc"], LINKS, [6, 0, 6], key="csc")
    view = graphs["csr"][0]
    small = _cabi.graph_view(*view._keep[:2], indices32=view._keep[1].to(torch.int32), ptrs32=view._keep[0].to(torch.int32))
    run((small,) + graphs["csr"][1:], LINKS, [6, 0, 6])
    res, _, _ = run(graphs["csr"], LINKS, [6, 9], optional=False, form=2)
    run(graphs["csr"], LINKS[::-1], [6, 0, 6], form=2, ws=res["ws"])   # the tables of the first call were left clean


@pytest.mark.parametrize("form", [1, 2])
def test_caps_above_every_fringe_give_seal_nodes_words(graphs, form):  # noqa: F811
    from tch_geometric import _cabi_seal
    _, _, got = run(graphs["csr"], LINKS, [1024, 1024], form=form)
    at = torch.tensor(LINKS, dtype=torch.int64, device=DEV).t().contiguous()
    out = {name: torch.full((len(LINKS), 512) if name in _cabi_seal.ROWS else (len(LINKS),), MARK, dtype=torch.int64, device=DEV)
           for name in NAMES[:6]}
    _cabi_seal.seal_nodes(graphs["csr"][0], at[0], at[1], 2, 512, form=form, out=out)
    assert all(np.array_equal(got[name], out[name].cpu().numpy()) for name in NAMES[:6]) and not got["cut"].any()


def test_the_kept_pair_is_uniform_over_the_190(fan):
    from tch_geometric import _cabi_seal, _cabi_seal_capped as ops
    view, ptrs, indices, hub, sink = fan
    m = 1 << 16
    src, dst = torch.full((m,), hub[20], device=DEV), torch.full((m,), sink, device=DEV)
    res = ops.seal_nodes_capped(view, src, dst, _cabi_seal.Seal(1, 4), [2], SEED)
    nodes = res["nodes"].cpu().numpy()
    assert (res["count"] == 4).all() and (res["cut"] == 1).all() and int(res["status"].item()) == 0
    a, b = nodes[:, 2], nodes[:, 3]
    assert (a < b).all() and (b < 20).all() and (nodes[:, 0] == hub[20]).all() and (nodes[:, 1] == sink).all()
    counts = np.bincount((b * (b - 1) // 2 + a).astype(np.int64), minlength=190)   # about 345 expected per pair
    exact_laws.chi2_gof(counts, np.full(190, 1 / 190), "the kept pair of tg_seal_nodes_capped")
    for i in (0, 1, m - 1):
        assert nodes[i].tolist() == hc.seal_capped(ptrs, indices, hub[20], sink, [2], 4, SEED, i)["nodes"]
