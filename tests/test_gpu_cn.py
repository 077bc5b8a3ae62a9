"""tg_cn_links on the GPU: every output word equals the restatement (helpers_cn), with sentinels round every array and
behind every listed member; the three forms on the same slots."""
import numpy as np
import pytest
import torch

import helpers_cn as hc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WINDOW, TILES, WAVE_GROUPS, GROUP_GROUPS = 512, 256, 2048, 1024   # tchgeo_cn.h (test_cn_cpu.py holds them to the header)
N, GUARD, MARK = 50000, 8, -7
HUB_LEN = 64 * TILES + 65
FORMS = [dict(form=1), dict(form=2), dict(form=0, wave_max=64)]    # WAVE, GROUP, AUTO with both kernels in one call
F = {S: 1000 * (S - WINDOW + 3) for S in (WINDOW - 1, WINDOW, WINDOW + 1)}   # where the window pairs' spans begin


def rows():
    """vertex -> the entries of its row, in any order; every vertex below is a row of its own"""
    r = {1: [100]}                                                       # 0: the empty row
    for L in (63, 64, 65, 128, 129):
        r[L] = list(range(100, 100 + 2 * L, 2))                          # 63 .. 129 entries: the evens from 100
    r[130] = list(range(100, 700, 3))                                    # overlaps them in every sixth id
    r[140] = list(range(101, 401, 2))                                    # overlapping range, no member in common
    r[141] = list(range(5000, 5100))                                     # a range of its own
    for S, f in F.items():                                               # one tile of a whose span of b is S entries
        r[200 + S] = [f - 9] + [f + 2 * k for k in range(S)] + [f + 2 * S + 7]
        r[800 + S] = [f, f + 1, f + 2, f + 5, f + 64, f + 2 * S - 3, f + 2 * S - 2]   # first and last word of the window match
    r[150] = list(range(300, 362)) + [362] * 5 + list(range(363, 393))   # a parallel run over places 62 .. 66
    r[151] = list(range(242, 362, 2)) + [362] * 8 + list(range(423, 473))   # and over places 60 .. 67
    r[152] = list(range(200, 600))                                       # longer than both: either run lies in a
    r[160] = [10] + list(range(2000, 2400, 7)) + [9000]                  # first and last entry of both rows match
    r[161] = [10] + list(range(2000, 2400, 5)) + [9000]
    r[170] = [3, 170, 171, 171, 900]                                     # rows that hold u and v themselves
    r[171] = [3, 170, 170, 171, 901]
    r[180] = list(range(0, 2 * HUB_LEN, 2))                              # more than one group round, a short last tile
    r[181] = list(range(0, 3 * HUB_LEN, 3))
    return r


LINKS = [(63, 64), (64, 65), (128, 129), (129, 63), (0, 64), (1, 65), (0, 0), (130, 129), (140, 128), (141, 65)] + \
        [(800 + S, 200 + S) for S in F] + [(150, 151), (151, 150), (150, 152), (152, 151), (160, 161), (170, 171), (171, 170),
                                           (170, 170), (180, 181), (160, 180), (181, 129), (-1, 64), (64, N), (-1, -1)]


@pytest.fixture(scope="module")
def graphs():
    """-> {"csr" | "csc": (view, ptrs, indices)} of the multigraph, built by tg_coo_to_csx, and the table words"""
    from tch_geometric import _cabi
    r = rows()
    src = np.concatenate([np.full(len(e), x) for x, e in r.items()])
    dst = np.concatenate([np.array(e) for e in r.values()])
    perm = np.random.default_rng(4).permutation(src.size)                # the ingest sorts
    ei = torch.from_numpy(np.stack([src, dst])[:, perm].astype(np.int64)).to(DEV)
    out = {}
    for name, csc in (("csr", False), ("csc", True)):
        tp, ti, _ = _cabi.coo_to_csx(ei[0], ei[1], N, N, csc)
        out[name] = (_cabi.graph_view(tp, ti), tp.cpu().numpy(), ti.cpu().numpy())
    _, ptrs, indices = out["csr"]
    deg = np.diff(ptrs)
    assert [deg[x] for x in (0, 1, 63, 64, 65, 128, 129)] == [0, 1, 63, 64, 65, 128, 129] and deg[180] == deg[181] == HUB_LEN
    assert all(np.all(np.diff(indices[ptrs[x]:ptrs[x + 1]]) >= 0) for x in r)
    for S, f in F.items():                                               # the span of b between a's first and last entry
        b = indices[ptrs[200 + S]:ptrs[201 + S]]
        assert np.searchsorted(b, f + 2 * S - 2, "right") - np.searchsorted(b, f, "left") == S and deg[800 + S] <= 64
    assert len(set(indices[ptrs[150] + 62:ptrs[150] + 67])) == 1 and len(set(indices[ptrs[151] + 60:ptrs[151] + 68])) == 1
    assert not set(hc.row(ptrs, indices, 140)) & set(hc.row(ptrs, indices, 128))
    assert hc.row(ptrs, indices, 160)[0] == hc.row(ptrs, indices, 161)[0] and 170 in hc.row(ptrs, indices, 170)
    words = np.random.default_rng(5).integers(0, 2 ** 32, (4, N), dtype=np.uint64)
    words[:, ::6] = 2 ** 32 - 1                                          # the hub pair's sums pass 2^44
    out["words"] = words
    out["tables"] = torch.from_numpy(words.astype(np.uint32).view(np.int32)).to(DEV)
    return out


MEMO = {}


def run(graphs, links, key="csr", cap=256, exclude=True, n_tables=4, optional=True, shadows=False, ws=None, **form):
    """one call against the restatement, word for word -> (the call's dict, the restatement's slots)"""
    from tch_geometric import _cabi, _cabi_cn as ops
    view, ptrs, indices = graphs[key]
    if shadows:
        view = _cabi.graph_view(*view._keep[:2], indices32=view._keep[1].to(torch.int32), ptrs32=view._keep[0].to(torch.int32))
    m = len(links)
    shapes = dict(count=(m,), cn=(m, cap), adjacent=(m,) if optional else None, score=(m, n_tables) if n_tables else None)
    whole, out = {}, {}
    for name, shape in shapes.items():
        out[name] = None
        if shape is not None:
            n = int(np.prod(shape))
            whole[name] = torch.full((n + 2 * GUARD,), MARK, dtype=torch.int64, device=DEV)   # GUARD words before and behind
            out[name] = whole[name][GUARD:GUARD + n].view(shape)
    at = torch.tensor(links, dtype=torch.int64, device=DEV).reshape(m, 2).t().contiguous()
    tables = graphs["tables"][:n_tables].contiguous() if n_tables else None
    res = ops.cn_links(view, at[0], at[1], cap, tables=tables, exclude_ends=exclude, out=out, ws=ws, **form)
    want = {name: np.full(shape, MARK, dtype=np.int64) for name, shape in shapes.items() if shape is not None}
    slots, status = [], 0
    for i, (u, v) in enumerate(links):
        k = (key, u, v, cap, exclude, n_tables)
        if k not in MEMO:
            MEMO[k] = hc.cn(ptrs, indices, u, v, cap, exclude, graphs["words"][:n_tables], N)
        st = MEMO[k]
        slots.append(st)
        status |= st["status"]
        want["count"][i] = st["count"]
        want["cn"][i, :len(st["cn"])] = st["cn"]                         # the sentinels stay behind the listed members
        if optional:
            want["adjacent"][i] = st["adjacent"]
        if n_tables:
            want["score"][i] = np.array(st["score"], dtype=np.uint64).view(np.int64)
    for name in want:
        assert np.array_equal(out[name].cpu().numpy(), want[name]), name
        w = whole[name].cpu().numpy()
        assert (w[:GUARD] == MARK).all() and (w[-GUARD:] == MARK).all(), name
    assert int(res["status"].item()) == status
    return res, slots


@pytest.mark.parametrize("form", FORMS, ids=str)
@pytest.mark.parametrize("exclude", [False, True])
def test_every_kind_of_link_in_every_form(graphs, form, exclude):
    _, slots = run(graphs, LINKS, exclude=exclude, cap=8192, **form)
    by = dict(zip(LINKS, slots))
    assert [st["status"] for st in slots[-3:]] == [2, 2, 2]
    assert by[180, 181]["count"] == len(range(0, 2 * HUB_LEN, 6)) - exclude   # 180 is a member unless the ends are excluded
    assert by[140, 128]["count"] == by[141, 65]["count"] == by[0, 64]["count"] == 0 and by[0, 0]["count"] == 0
    assert by[150, 151]["cn"].count(362) == 1 and by[170, 171]["cn"] == ([3] if exclude else [3, 170, 171])
    assert by[170, 171]["adjacent"] == 3 and by[160, 161]["cn"][0] == 10 and by[160, 161]["cn"][-1] == 9000
    for S, f in F.items():
        assert by[800 + S, 200 + S]["cn"] == [f, f + 2, f + 64, f + 2 * S - 2]


@pytest.mark.parametrize("form", FORMS, ids=str)
def test_cap_below_at_and_above_a_link_s_count(graphs, form):
    c = len(set(range(100, 700, 3)) & set(range(100, 358, 2)) - {130, 129})   # the link (130, 129) without its ends
    assert c > 8
    for cap, cut in ((c - 1, 1), (c, 0), (c + 1, 0), (1, 1)):
        _, slots = run(graphs, [(63, 64), (130, 129), (1, 65), (130, 129), (170, 171)], cap=cap, **form)   # the neighbours stay
        assert slots[1]["count"] == c and slots[1]["status"] == cut
    run(graphs, [(180, 181), (63, 64)], cap=300, **form)                 # the cut falls inside the group kernel's first round


@pytest.mark.parametrize("form", FORMS, ids=str)
@pytest.mark.parametrize("m", [0, 1, 255, 256, 257, 1025, 4 * WAVE_GROUPS + 1])
def test_slot_counts_up_to_past_both_grids(graphs, form, m):
    assert 1025 > GROUP_GROUPS                                           # one link per workgroup there, per wavefront here
    run(graphs, [LINKS[(5 * i) % len(LINKS)] for i in range(m)], cap=16, n_tables=1, **form)


@pytest.mark.parametrize("form", FORMS, ids=str)
def test_views_shadows_tables_null_outputs_and_a_second_call_over_the_workspace(graphs, form):
    run(graphs, LINKS, key="csc", **form)
    run(graphs, LINKS, shadows=True, **form)
    run(graphs, LINKS, n_tables=1, **form)
    res, _ = run(graphs, LINKS, n_tables=0, optional=False, **form)
    run(graphs, LINKS[::-1], ws=res["ws"], **form)                       # the counter of the first call is cleared by the second
