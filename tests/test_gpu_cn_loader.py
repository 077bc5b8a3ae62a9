"""CommonNeighborLoader: every mini-batch has the lists, counts and adjacency words of the restatement (helpers_cn) per link
on the CSC and the four scores of a float64 loop, over two epochs, prefetch 1 against 4, shuffled with drop_last; a list cut
by cn_cap raises unless truncate=True."""
import math

import numpy as np
import pytest
import torch

import helpers_cn as hc
from helpers_induced import csc_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, HUB, B, L, CAP = 300, 7, 16, 100, 128


@pytest.fixture(scope="module")
def graph():
    from tch_geometric.transforms import Graph
    rs = np.random.default_rng(8)
    half = np.concatenate([rs.integers(0, N, (2, 1500)), np.stack([np.full(200, HUB), rs.integers(0, N, 200)]),
                           [[0, 0, 4, 9], [1, 1, 4, 9]]], axis=1)        # a hub, the edge (0, 1) twice, two self loops
    ei = np.concatenate([half, half[::-1]], axis=1).astype(np.int64)     # symmetric
    x = rs.standard_normal((N, 3)).astype(np.float32)
    data = Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=N, x=torch.from_numpy(x).to(DEV))
    links = rs.integers(0, N, (2, L)).astype(np.int64)   # 100 links: 6 mini-batches of 16 and a ragged one of 4
    links[:, :5] = [[0, HUB, 4, 9, 9], [1, 3, 4, 9, 4]]  # an edge with parallel entries, the hub, u == v on a loop, loop ends
    ptrs, indices, _ = csc_of(ei, N)
    deg = hc.distinct_degrees(ptrs, indices)
    return dict(data=data, x=x, links=links, label=(np.arange(L) % 2).astype(np.float32), ptrs=ptrs, indices=indices, deg=deg,
                sets=[set(hc.row(ptrs, indices, v)) for v in range(N)])


def loader(g, **kw):
    from tch_geometric.loader import CommonNeighborLoader
    kw = dict(dict(edge_label_index=torch.from_numpy(g["links"]), edge_label=torch.from_numpy(g["label"]), cn_cap=CAP,
                   batch_size=B, prefetch=4, device=DEV), **kw)
    return CommonNeighborLoader(g["data"], **kw)


def same(g, mb, picked, cap=CAP, labelled=True):
    """mini-batch mb against the restatement over the links at the positions `picked`"""
    links = g["links"][:, picked]
    slots = [hc.cn(g["ptrs"], g["indices"], u, v, cap) for u, v in links.T.tolist()]
    cn_index = np.array([w for st in slots for w in st["cn"]], dtype=np.int64)
    assert np.array_equal(mb.cn_index.cpu().numpy(), cn_index)
    assert mb.cn_ptr.tolist() == np.cumsum([0] + [len(st["cn"]) for st in slots]).tolist()
    assert mb.cn_count.tolist() == [st["count"] for st in slots] and mb.adjacent.tolist() == [st["adjacent"] for st in slots]
    assert np.array_equal(mb.edge_label_index.cpu().numpy(), links) and mb.batch_size == len(picked)
    assert np.array_equal(mb.edge_label.cpu().numpy(), g["label"][picked]) if labelled else mb.edge_label is None
    assert np.array_equal(mb.x.cpu().numpy(), g["x"][cn_index])
    got = {k: t.cpu().numpy() for k, t in mb.scores.items()}
    assert sorted(got) == ["aa", "cn", "jaccard", "ra"] and all(t.dtype == np.float32 for t in got.values())
    for i, (u, v) in enumerate(links.T.tolist()):
        members = sorted((g["sets"][u] & g["sets"][v]) - {u, v})         # all of C, also where the list is cut
        union = len((g["sets"][u] | g["sets"][v]) - {u, v})
        want = dict(cn=float(len(members)), jaccard=len(members) / union if union else 0.0,
                    aa=math.fsum(1.0 / math.log(g["deg"][w]) for w in members if g["deg"][w] >= 2),
                    ra=math.fsum(1.0 / g["deg"][w] for w in members))
        for name, w in want.items():
            # a table word is its weight in units of 2^-32, rounded to nearest or clamped one unit down: 2^-32 per member at
            # most; the integer sum and its scaling are exact; one rounding to float32 (2^-24 relative); the reference's own
            # float64 arithmetic (2^-50 relative, generously)
            fixed = len(members) * 2.0 ** -32 if name in ("aa", "ra") else 0.0
            assert abs(float(got[name][i]) - w) <= fixed + abs(w) * (2.0 ** -24 + 2.0 ** -50), (name, u, v)
    return slots


@pytest.mark.parametrize("prefetch", [1, 4])
def test_two_epochs_full_and_ragged_mini_batches(graph, prefetch):
    ld = loader(graph, prefetch=prefetch)
    assert len(ld) == 7
    for epoch in range(2):
        seen = 0
        for j, mb in enumerate(ld):
            slots = same(graph, mb, np.arange(j * B, min((j + 1) * B, L)))
            assert mb.call_id == epoch * 7 + j
            if j == 0:   # the edge (0, 1) both ways; the hub's long row; the loop at 4 is no member of its own link
                assert slots[0]["adjacent"] == 3 and slots[1]["count"] > 0 and 4 not in slots[2]["cn"] and slots[2]["count"] > 0
            seen += 1
        assert seen == 7
    assert ld.slab_allocations == 1                      # the second epoch reused the slab set


def test_shuffle_with_drop_last(graph):
    ld = loader(graph, shuffle=True, drop_last=True, seed=5, edge_label=None)
    assert len(ld) == 6
    for epoch in range(2):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(5 * 1000003 + epoch)
        order = torch.randperm(L, device=DEV, generator=gen).cpu().numpy()
        assert sum(1 for j, mb in enumerate(ld) if same(graph, mb, order[j * B:(j + 1) * B], labelled=False)) == 6


def test_a_cut_list_raises_naming_cn_cap_unless_truncate(graph):
    longest = max(hc.cn(graph["ptrs"], graph["indices"], u, v, CAP)["count"] for u, v in graph["links"].T.tolist())
    assert 3 < longest <= CAP
    with pytest.raises(RuntimeError, match="cn_cap = 3"):
        list(loader(graph, cn_cap=3))
    for j, mb in enumerate(loader(graph, cn_cap=3, truncate=True)):
        slots = same(graph, mb, np.arange(j * B, min((j + 1) * B, L)), cap=3)
        assert max(len(st["cn"]) for st in slots) <= 3
