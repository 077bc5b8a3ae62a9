"""tg_lp_sizes / tg_lp_propose / tg_lp_commit on the device, every output word against the restatement (helpers_lp), with
guard words round every array the kernels write."""
import numpy as np
import pytest
import torch

import helpers_lp as hl

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, WAVE_MAX, GUARD = 10000, 64, 16
PARTS = (1, 2, 64, 65, 1024, 3000)          # 3000 > TG_LP_LDS_LABELS: the dense table
FORMS = (1, 2, 0)                           # WAVE, GROUP, AUTO
SEED, ROUND = 0x1B0C5EED, 7
# crafted rows, as (vertex, entries): lengths round a tile, round wave_max = 64 and round TG_LP_WAVE_MAX = 512
HUB_LABELS, HUB_ONE, GAIN_4095, TIE_TWO, TIE_OWN, ISOLATED = 9000, 9001, 9002, 9003, 9004, 9005
LENGTHS = {9010 + i: d for i, d in enumerate((1, 63, 64, 65, 511, 512, 513, 1100))}


def crafted_edges(rs):
    rows = {HUB_LABELS: np.concatenate([np.arange(3000), [7, 7]]),   # 3000 distinct labels at P = 3000, label 7 thrice
            HUB_ONE: np.full(4200, 5), GAIN_4095: np.full(4095, 5),   # parallel entries: both clamp to the gain field 0
            TIE_TWO: np.array([12, 12, 11, 11, 13]),          # two labels twice: the smaller wins
            TIE_OWN: np.array([3004, 12]),                    # one entry of its own label at P = 3000, one foreign: stays
            ISOLATED: np.array([], dtype=np.int64)}
    rows.update({v: rs.integers(0, N, d) for v, d in LENGTHS.items()})
    rows[9012] = np.concatenate([rows[9012][:60], [9012, 9012, 9012, 9012]])   # self loops inside a full tile
    return rows


@pytest.fixture(scope="module")
def graphs():
    """name -> (ptrs, indices) on the device: the ingest's CSR and CSC of one edge list, and a raw CSR with entries of -1
    and n, self loops and rows that do not ascend"""
    from tch_geometric import _cabi
    rs = np.random.default_rng(5)
    crafted = crafted_edges(rs)
    src = [rs.integers(0, 9000, 60000)] + [np.full(len(w), v) for v, w in crafted.items()]
    dst = [rs.integers(0, 9000, 60000)] + list(crafted.values())
    row, col = (torch.from_numpy(np.concatenate(a).astype(np.int64)).to(DEV) for a in (src, dst))
    out = {"csr": _cabi.coo_to_csx(row, col, N, N, False)[:2], "csc": _cabi.coo_to_csx(col, row, N, N, True)[:2]}
    n = 300
    deg = rs.integers(0, 140, n)
    idx = rs.integers(-1, n + 1, int(deg.sum()))             # -1 and n among them
    out["raw"] = (torch.from_numpy(np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)).to(DEV),
                  torch.from_numpy(idx.astype(np.int64)).to(DEV))
    return out


def guarded(n, dtype, fill):
    """a tensor of n words with GUARD words of `fill` on either side -> (whole, the view in the middle)"""
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + n]


def guards_intact(whole, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[-GUARD:] == fill).all())


_want = {}


def want_propose(graphs, kind, P):
    if (kind, P) not in _want:
        ptrs, idx = (t.cpu().numpy() for t in graphs[kind])
        _want[kind, P] = hl.propose(ptrs, idx, np.arange(len(ptrs) - 1) % P, P, SEED, ROUND)
    return _want[kind, P]


@pytest.mark.parametrize("P", PARTS)
@pytest.mark.parametrize("form", FORMS)
def test_propose_equals_the_restatement(graphs, form, P):
    from tch_geometric import _cabi, _cabi_lp as lp
    for kind, (ptrs, idx) in graphs.items():
        n = ptrs.numel() - 1
        skey_want, cut_want = want_propose(graphs, kind, P)
        label = (torch.arange(n, device=DEV) % P).to(torch.int32)
        ws = lp.lp_workspace(n, P, DEV, form, WAVE_MAX)       # exactly the queried bytes
        for shadows in (False, True):
            g = _cabi.graph_view(ptrs, idx, indices32=idx.to(torch.int32) if shadows else None,
                                 ptrs32=ptrs.to(torch.int32) if shadows else None)
            whole, skey = guarded(n, torch.int64, 0x5A)
            state = torch.tensor([3, 0, 77], dtype=torch.int64, device=DEV)    # cut (added to 3), status, a guard
            for call in (1, 2):                               # the second call finds the workspace the first one left
                lp.lp_propose(g, label, P, SEED, ROUND, skey, state[:1], state[1:2].view(torch.int32)[:1], ws, form, WAVE_MAX)
            assert np.array_equal(skey.cpu().numpy().view(np.uint64), skey_want), (kind, shadows)
            assert state.tolist() == [3 + 2 * cut_want, 0, 77] and guards_intact(whole, 0x5A), (kind, shadows)
    if P == 3000:                                             # the crafted cases are what they claim to be
        s = want_propose(graphs, "csr", P)[0]
        field = lambda v: (int(s[v]) >> 44, (int(s[v]) >> 32) & 4095)
        assert field(HUB_ONE) == field(GAIN_4095) == (5, 0) and field(TIE_TWO)[0] == 11
        assert s[TIE_OWN] == s[ISOLATED] == hl.STAY and field(HUB_LABELS) == (7, 4095 - 2)


def skeys(pairs, n):
    s = np.full(n, hl.STAY, dtype=np.uint64)
    for v, word in pairs:
        s[v] = np.uint64(word)
    return s


key = lambda target, gain_field=0, h=0: (target << 44) | (gain_field << 32) | h
COMMIT_N, COMMIT_P = 1000, 8
COMMITS = {   # name -> (movers [(v, skey)], sizes [P], cap)
    "none": ([], [80] * 8, 100),
    **{"movers_%d" % m: ([(3 * i, key(i % 3, i % 5, 1000 - i)) for i in range(m)], [80] * 8, 100) for m in (1, 63, 64, 65, 257)},
    "free_0": ([(i, key(2, 0, i)) for i in range(5)], [80, 80, 100] + [80] * 5, 100),
    **{"free_4_wanted_%d" % m: ([(2 * i, key(6, 9 - i, 5)) for i in range(m)], [80] * 6 + [96, 80], 100) for m in (3, 4, 5)},
    "equal_keys": ([(v, key(1, 7, 7)) for v in (400, 9, 250)], [80, 99] + [80] * 6, 100),      # one place: v = 9 takes it
    "above_cap": ([(i, key(0, 0, i)) for i in range(3)], [120] + [80] * 7, 100),             # free is 0, not negative
    "bad_target": ([(10, key(1, 0, 3)), (11, key(8, 0, 1)), (12, key(1, 0, 2)), (13, key(1 << 19, 0, 0))], [80, 98] + [80] * 6, 100),
    "all_full": ([(i, key(i % 8, 0, i)) for i in range(40)], [100] * 8, 100),
}


@pytest.mark.parametrize("name", list(COMMITS))
def test_commit_equals_the_restatement(name):
    from tch_geometric import _cabi_lp as lp
    movers, sizes, cap = COMMITS[name]
    label0 = np.arange(COMMIT_N) % COMMIT_P
    skey = skeys(movers, COMMIT_N)
    label_want, size_want, moved_want, status_want = hl.commit(label0, sizes, cap, skey, COMMIT_P)
    assert (name == "bad_target") == (status_want == 2)
    lw, label = guarded(COMMIT_N, torch.int32, -7)
    sw, size = guarded(COMMIT_P, torch.int64, -7)
    label.copy_(torch.from_numpy(label0).to(DEV))
    size.copy_(torch.tensor(sizes, device=DEV))
    state = torch.tensor([5, 0, 77], dtype=torch.int64, device=DEV)            # moved (added to 5), status, a guard
    ws = lp.lp_workspace(COMMIT_N, COMMIT_P, DEV)
    lp.lp_commit(label, size, COMMIT_P, cap, torch.from_numpy(skey.view(np.int64)).to(DEV), state[:1],
                 state[1:2].view(torch.int32)[:1], ws)
    assert label.tolist() == label_want.tolist() and size.tolist() == size_want.tolist()
    assert state.tolist() == [5 + moved_want, status_want, 77] and guards_intact(lw, -7) and guards_intact(sw, -7)


@pytest.mark.parametrize("P", (5, 3000))                     # the histogram in LDS, and device atomics
def test_sizes_counts_and_flags_a_label_out_of_range(P):
    from tch_geometric import _cabi_lp as lp
    label = np.random.default_rng(P).integers(0, P, 5000)
    for bad in ((), (17, 4000)):
        host = label.copy()
        host[list(bad)] = (P, -1)[:len(bad)]
        whole, size = guarded(P, torch.int64, 9)              # tg_lp_sizes clears what it counts into
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        lp.lp_sizes(torch.from_numpy(host).to(DEV, torch.int32), P, size, status)
        keep = np.ones(5000, dtype=bool)
        keep[list(bad)] = False
        assert size.tolist() == np.bincount(label[keep], minlength=P).tolist()
        assert status.item() == (1 if bad else 0) and guards_intact(whole, 9)
