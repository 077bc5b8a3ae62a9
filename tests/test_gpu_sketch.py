"""tg_sketch_init / _propagate / _links on the GPU: every word equals the restatement (helpers_sketch), with sentinel words
before and after every array and a workspace of exactly the queried bytes; every form on the same graph."""
import numpy as np
import pytest
import torch

import helpers_sketch as hk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, GUARD, MARK, SEED = 700, 64, -7, 0x1234567887654321
WAVE_GROUPS = 2048                                                        # tchgeo_sketch.h (test_sketch_cpu.py holds it to the header)
PARAMS = [(64, 8), (128, 8), (256, 10), (192, 9)]
FORMS = [dict(form=1), dict(form=2), dict(form=3, split_seg=64), dict(form=0, wave_max=64, group_max=256, split_seg=64)]
LONG, ISOLATED = (63, 64, 65, 257, 300), 699


def rows():
    """vertex -> the entries of its row; 0 has none, nobody names ISOLATED"""
    r = {1: [5], 2: [2, 2, 9]}                                            # a self loop, twice
    for L in LONG:
        r[L] = [(L * 7 + 3 * k) % 690 for k in range(L)]
    r[300] = [k // 2 for k in range(298)] + [300, 257]                    # parallel entries, a self loop, the hub
    return r


@pytest.fixture(scope="module")
def graphs():
    """-> {"csr" | "csc": (view, ptrs, indices)} built by tg_coo_to_csx, "raw": the CSR with an entry n and an entry -1"""
    from tch_geometric import _cabi
    r = rows()
    src = np.concatenate([np.full(len(e), x) for x, e in r.items()])
    dst = np.concatenate([np.array(e) for e in r.values()])
    ei = torch.from_numpy(np.stack([src, dst])[:, np.random.default_rng(4).permutation(src.size)].astype(np.int64)).to(DEV)
    out = {}
    for name, csc in (("csr", False), ("csc", True)):
        tp, ti, _ = _cabi.coo_to_csx(ei[0], ei[1], N, N, csc)
        out[name] = (_cabi.graph_view(tp, ti), tp.cpu().numpy(), ti.cpu().numpy())
    _, ptrs, indices = out["csr"]
    deg = np.diff(ptrs)
    assert [deg[x] for x in (0, 1, 63, 64, 65, 257, ISOLATED)] == [0, 1, 63, 64, 65, 257, 0] and deg[257] > 2 * 64
    assert ISOLATED not in indices and 2 in indices[ptrs[2]:ptrs[3]] and len(set(indices[ptrs[300]:ptrs[301]])) < deg[300]
    ti = out["csr"][0]._keep[1].clone()
    ti[int(ptrs[65]) + 7], ti[int(ptrs[257]) + 200] = N, -1
    out["raw"] = (_cabi.graph_view(out["csr"][0]._keep[0], ti), ptrs, ti.cpu().numpy())
    return out


MEMO = {}


def chain(graphs, key, n_perm, hll_p, h=3):
    """the restatement's hops 0..h on graph `key` -> [(M, R)], shared by every test"""
    k = (key, n_perm, hll_p)
    if k not in MEMO:
        MEMO[k] = [hk.init(N, n_perm, hll_p, SEED)]
    while len(MEMO[k]) <= h:
        MEMO[k].append(hk.propagate(graphs[key][1], graphs[key][2], *MEMO[k][-1])[:2])
    return MEMO[k][:h + 1]


def guarded(shape, dtype=torch.int32):
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), MARK, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + n].view(shape)


def intact(whole):
    w = whole.cpu().numpy()
    return (w[:GUARD] == MARK).all() and (w[-GUARD:] == MARK).all()


def words(t):
    return t.cpu().numpy().view(np.uint32)


def hop(graphs, key, n_perm, hll_p, shadows=False, ws=None, want_status=0, **form):
    """one tg_sketch_propagate of the restatement's hop 0 on graph `key`, word for word -> the workspace's whole tensor"""
    from tch_geometric import _cabi, _cabi_sketch as ops
    view, ptrs, indices = graphs[key]
    if shadows:
        view = _cabi.graph_view(*view._keep[:2], indices32=view._keep[1].to(torch.int32), ptrs32=view._keep[0].to(torch.int32))
    sizes = ops.Sketch(1, n_perm, hll_p, SEED, **form)
    M0, R0 = chain(graphs, "csr", n_perm, hll_p, 0)[0]
    prev_whole, prev = guarded((N, sizes.row_words))
    prev.copy_(torch.from_numpy(hk.pack(M0, R0).view(np.int32)))
    next_whole, nxt = guarded((N, sizes.row_words))
    need, taken = sizes.workspace_bytes(N, len(indices))
    assert taken == sizes.form and (need == 0) == (sizes.form in (1, 2))
    if ws is None:
        ws = torch.full((need // 4 + 2 * GUARD,), MARK, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.sketch_propagate(view, sizes, prev, nxt, status, ws[GUARD:GUARD + need // 4])     # exactly the queried bytes
    M1, R1, st = hk.propagate(ptrs, indices, M0, R0)
    assert np.array_equal(words(nxt), hk.pack(M1, R1)) and int(status.item()) == st == want_status
    assert intact(next_whole) and intact(prev_whole) and intact(ws)
    return ws


@pytest.mark.parametrize("form", FORMS, ids=str)
@pytest.mark.parametrize("n_perm, hll_p", PARAMS)
@pytest.mark.parametrize("key", ["csr", "csc"])
@pytest.mark.parametrize("shadows", [False, True])
def test_a_hop_in_every_form(graphs, form, n_perm, hll_p, key, shadows):
    hop(graphs, key, n_perm, hll_p, shadows, **form)


@pytest.mark.parametrize("form", FORMS, ids=str)
def test_entries_outside_the_graph_are_skipped_and_a_second_call_over_the_workspace(graphs, form):
    ws = hop(graphs, "raw", 128, 8, want_status=2, **form)
    if form["form"] in (0, 3):
        hop(graphs, "csr", 128, 8, ws=ws, **form)                         # the same bytes: the counters are cleared by the call


@pytest.mark.parametrize("n_perm, hll_p", PARAMS)
def test_init_and_three_chained_hops_give_equal_bytes_in_every_form(graphs, n_perm, hll_p):
    from tch_geometric import _cabi, _cabi_sketch as ops
    want = np.stack([hk.pack(M, R) for M, R in chain(graphs, "csr", n_perm, hll_p)])
    for form in FORMS:
        sketch, status = ops.sketch_build(graphs["csr"][0], ops.Sketch(3, n_perm, hll_p, SEED, **form))
        assert np.array_equal(words(sketch), want) and int(status.item()) == 0, form
    whole, hop0 = guarded((N, want.shape[2]))
    ops.sketch_init(ops.Sketch(1, n_perm, hll_p, SEED), hop0)
    assert np.array_equal(words(hop0), want[0]) and intact(whole)
    loops = torch.zeros(3, dtype=torch.int64, device=DEV)                 # n = 1: a closed ball of one vertex at every hop
    tp, ti, _ = _cabi.coo_to_csx(loops, loops, 1, 1, True)
    for form in FORMS:
        sketch, _ = ops.sketch_build(_cabi.graph_view(tp, ti), ops.Sketch(2, n_perm, hll_p, 9, **form))
        assert np.array_equal(words(sketch), np.stack([hk.pack(*hk.init(1, n_perm, hll_p, 9))] * 3)), form


LINKS = [(63, 64), (257, 300), (300, 300), (ISOLATED, 65), (0, 1), (2, 257), (-1, 64), (64, N), (-1, -1), (65, 63)]


@pytest.mark.parametrize("h", [1, 2, 3])
@pytest.mark.parametrize("n_perm, hll_p", PARAMS)
def test_links(graphs, h, n_perm, hll_p):
    from tch_geometric import _cabi_sketch as ops
    hops = chain(graphs, "csr", n_perm, hll_p, h)
    sizes = ops.Sketch(h, n_perm, hll_p, SEED)
    sketch = torch.from_numpy(np.stack([hk.pack(M, R) for M, R in hops]).view(np.int32)).to(DEV)
    ref = hk.links(hops, *zip(*LINKS))
    assert ref["status"] == 2 and ref["match"][2].diagonal().min() == n_perm and not ref["usum"][6:9].any() and ref["usum"][9].all()
    for m in (0, 1, 63, 64, 65, 4 * WAVE_GROUPS + 1):                     # the last: one slot past the grid's wavefronts
        pick = np.arange(m) % len(LINKS) if m != 1 else np.array([6])     # alone: a refused slot
        at = torch.tensor([LINKS[i] for i in pick], dtype=torch.int64, device=DEV).reshape(m, 2).t().contiguous()
        wholes, out = {}, {}
        for name in ops.LINK_OUTPUTS:
            wholes[name], out[name] = guarded((m,) + ref[name].shape[1:], torch.int64 if name in ("usum", "nsum") else torch.int32)
        res = ops.sketch_links(sizes, sketch, at[0], at[1], out=out)
        for name in ops.LINK_OUTPUTS:
            got = out[name].cpu().numpy()
            assert np.array_equal(got.view(ref[name].dtype), ref[name][pick]) and intact(wholes[name]), (name, m)
        assert int(res["status"].item()) == (2 if m == 1 or m > 6 else 0)
