"""Every device sampler against the EXACT output law of the reference's algorithm (tests/exact_laws.py), on long
columns and large fan-outs: the sizes where the counter-addressed restatements the kernels share with the oracle
(reservoir by tickets, the blocked f64 running sum, the chunked one-slot reservoir, the 32-bit slot draw and its 64-bit
fallback) stop being the literal loop.  Bit parity with the oracle cannot see an error the two have in common; these
one-sample tests can.

One launch per configuration: the hub vertex is every seed, so N outcomes use N distinct draw addresses (call id = batch,
draw id = seed slot); counts are reduced on the device.  The tests are deterministic: a failure reproduces exactly.
Sample sizes: exact_laws.n_outcomes(k) (2^20, fewer above k = 64), N_WALK walkers, N_NEG negative items."""
import ctypes as C

import numpy as np
import pytest
import torch

import exact_laws as L
from exact_laws import N_NEG, N_WALK, n_outcomes
from test_exact_laws_cpu import node2vec_graph, tempo_graph, walk_row, weights_wide

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FUSED = 2
B = 256                                                         # seeds per batch of the batched launches
HUB = 3_000_001                                                 # the slot-draw fallback hub: 2^32 mod 3 000 000 is large


@pytest.fixture(scope="module")
def cabi():
    from tch_geometric import _cabi
    return _cabi


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _columns(lengths):
    """CSC of one column per length (row ids 0: only positions matter) -> (ptrs numpy, ptrs, indices)"""
    ptrs = np.zeros(len(lengths) + 1, dtype=np.int64)
    ptrs[1:] = np.cumsum(lengths)
    return ptrs, _t(ptrs), torch.zeros(int(ptrs[-1]), dtype=torch.int64, device=DEV)


_LAWS = {}


def _law(n, k, replace=False):
    key = (n, k, replace)
    if key not in _LAWS:
        if len(_LAWS) > 8:
            _LAWS.clear()
        _LAWS[key] = L.ReplacementLaw(n, k) if replace else L.uniform_law(n, k)
    return _LAWS[key]


def _cap(N, n_raw, budget=1 << 33):
    """outcomes of a launch whose every outcome reads a whole column of n_raw edges: at most `budget` edges read in all"""
    while N > 1024 and N * n_raw > budget:
        N //= 2
    return N


def _check_uniform(E, n, k, replace, what):
    if not replace and n <= k:
        assert torch.equal(E, torch.arange(n, device=DEV).expand_as(E)), what + ": n <= k takes every candidate in order"
        return
    L.check_reservoir(E, _law(n, k, replace), what, replace=replace)


# ---------------------------------------------------------------- the fused per-batch kernel
FUSED_K = [1, 15, 16, 17, 32, 33, 60, 128, 129, 191]        # 191: the largest fan-out whose ticket strips fit the LDS


def _fused_cases():
    for sampler in (0, 1):
        for k in FUSED_K:
            for n in sorted({k + 1, 64, 65, 1000, 70000}):
                if n > k:
                    yield sampler, k, n
        for k in (1, 16, 129, 191):
            yield sampler, k, HUB


@pytest.fixture(scope="module")
def fused_graph(cabi):
    lengths = sorted({k + 1 for k in FUSED_K} | {64, 65, 1000, 70000, HUB})
    ptrs, P, I = _columns(lengths)
    g = cabi.graph_view(P, I, indices32=I.to(torch.int32), ptrs32=P.to(torch.int32), max_degree="auto")
    return g, ptrs, {n: v for v, n in enumerate(lengths)}


@pytest.mark.parametrize("sampler,k,n", list(_fused_cases()))
def test_fused_kernel_law(cabi, fused_graph, sampler, k, n):
    g, ptrs, vertex = fused_graph
    v = vertex[n]
    N = n_outcomes(k)
    nb = N // B
    seeds = torch.full((nb, B), v, dtype=torch.int64, device=DEV)
    out = cabi.NsBatchedOut(nb, B, [k], DEV)
    assert cabi.ns_homo_batched_form(g, out, nb, B, [k], form=FUSED, sampler=sampler)[0] == FUSED
    cabi.ns_homo_batched(g, seeds, [k], 0x1A3, 11, out, sampler=sampler)
    cnt = k if sampler == 1 else min(k, n)
    assert bool((out.counts[:, 1] == B * cnt).all())
    E = (out.edge_index[:, :B * cnt].reshape(N, cnt) - int(ptrs[v])).contiguous()
    del out
    _check_uniform(E, n, k, sampler == 1, "fused sampler %d k=%d n=%d" % (sampler, k, n))


# ---------------------------------------------------------------- the flat hop
HOP_K = [16, 32, 128, 129, 256, 1000, 4096]


@pytest.fixture(scope="module")
def hop_graph(cabi):
    lengths = sorted({k + 1 for k in HOP_K} | {2 * k for k in HOP_K} | {70000})
    ptrs, P, I = _columns(lengths)
    return cabi.graph_view(P, I), ptrs, {n: v for v, n in enumerate(lengths)}


@pytest.mark.parametrize("k,n", [(k, n) for k in HOP_K for n in sorted({k + 1, 2 * k, 70000})] + [(33, 70000)])
def test_flat_hop_law(cabi, hop_graph, k, n):
    g, ptrs, vertex = hop_graph
    sampler = 1 if (k, n) == (33, 70000) else 0
    v = vertex[n] if n in vertex else vertex[70000]
    N = n_outcomes(k) // 2                                      # three int64 slabs and the workspace
    cnt, off, nbr, ep, par = cabi.ns_hop(g, torch.full((N,), v, dtype=torch.int64, device=DEV), k, 0x2B4, call_id=5,
                                         sampler=sampler)
    assert bool((cnt == k).all()) and int(off[N]) == N * k
    E = (ep[:N * k].reshape(N, k) - int(ptrs[v])).contiguous()
    del cnt, off, nbr, ep, par
    _check_uniform(E, n, k, sampler == 1, "flat hop sampler %d k=%d n=%d" % (sampler, k, n))


# ---------------------------------------------------------------- the filtered hop and the batched scan kernel
SCAN_LEN = [200, 5000, 200000]
WINDOW = (10, 40)                                               # FILTER_STATIC: admitted iff 10 <= t <= 40


@pytest.fixture(scope="module")
def scan_graph(cabi):
    ptrs, P, I = _columns(SCAN_LEN)
    ts = np.random.default_rng(21).integers(0, 90, int(ptrs[-1]))   # about a third admitted, scattered
    g = cabi.graph_view(P, I, None, _t(ts))
    return g, ptrs, ts


def _ranks(ptrs, v, adm_raw):
    """rank of every raw position of column v among its admitted ones, -1 where not admitted"""
    lo, hi = int(ptrs[v]), int(ptrs[v + 1])
    a = adm_raw[lo:hi]
    r = np.full(hi - lo, -1, dtype=np.int64)
    r[a] = np.arange(int(a.sum()))
    return _t(r), int(a.sum())


@pytest.mark.parametrize("form,k", [("flat", k) for k in (1, 15, 64, 65, 200)] +
                         [("batched", k) for k in (1, 15, 64)])          # the batched scan kernel takes k <= 64
@pytest.mark.parametrize("n_raw", SCAN_LEN)
def test_filtered_hop_law(cabi, scan_graph, form, k, n_raw):
    g, ptrs, ts = scan_graph
    v = SCAN_LEN.index(n_raw)
    rank, n = _ranks(ptrs, v, (ts >= WINDOW[0]) & (ts <= WINDOW[1]))
    N = _cap(n_outcomes(k) // 2, n_raw)
    cnt_each = min(k, n)
    if form == "flat":
        verts, st = torch.full((N,), v, dtype=torch.int64, device=DEV), torch.zeros(N, dtype=torch.int64, device=DEV)
        cnt, off, nbr, ep, par, st_out, status = cabi.ns_hop_scan(g, verts, st, k, 0x3C5, 0, WINDOW, call_id=3,
                                                                  group_cap=N * (n_raw // 512 + 2) + 1024)
        assert int(status) == 0 and bool((cnt == cnt_each).all())
        raw = ep[:N * cnt_each].reshape(N, cnt_each)
    else:
        nb = N // B
        out = cabi.NsBatchedOut(nb, B, [k], DEV, with_states=True)
        cabi.ns_homo_batched(g, torch.full((nb, B), v, dtype=torch.int64, device=DEV), [k], 0x3C5, 3, out, filter_mode=0,
                             window=WINDOW, seeds_state=torch.zeros((nb, B), dtype=torch.int64, device=DEV))
        assert bool((out.counts[:, 1] == B * cnt_each).all())
        raw = out.edge_index[:, :B * cnt_each].reshape(N, cnt_each)
    E = rank[raw - int(ptrs[v])].contiguous()
    _check_uniform(E, n, k, False, "filtered %s hop k=%d column %d (%d admitted)" % (form, k, n_raw, n))


# ---------------------------------------------------------------- weighted: batched, flat and group forms
W_LEN = [63, 64, 65, 513, 5000, 100000]


@pytest.fixture(scope="module")
def weighted_graph(cabi):
    ptrs, P, I = _columns(W_LEN)
    w = np.concatenate([weights_wide(n, 100 + n) for n in W_LEN])
    ts = np.random.default_rng(22).integers(0, 90, int(ptrs[-1]))
    ts[ptrs[:-1]] = 20                                          # every column's first candidate is admitted (positive)
    return cabi.graph_view(P, I, _t(w), _t(ts)), ptrs, w, ts


def _weighted_flat(cabi, graph, V, k, mode, groups, group_cap):
    """tg_ns_hop_weighted (a wavefront / workgroup per column) or tg_ns_hop_weighted_groups (512-edge groups)"""
    m = V.numel()
    o = dict(dtype=torch.int64, device=DEV)
    cnt, offsets = torch.empty(m, **o), torch.empty(m + 1, **o)
    nbr, ep, par, st_out = (torch.empty(m * k, **o) for _ in range(4))
    S, IDS = torch.zeros(m, **o), torch.arange(m, **o)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    hin, hout, flt = cabi.TgHopIn(), cabi.TgHopOut(), cabi.TgHopFilter()
    hin.vertices, hin.ids, hin.m, hin.fanout, hin.sampler, hin.rng_tag = V.data_ptr(), IDS.data_ptr(), m, k, 2, 0x31
    hout.cnt, hout.offsets = cnt.data_ptr(), offsets.data_ptr()
    hout.neighbors, hout.edge_ptrs, hout.parents = nbr.data_ptr(), ep.data_ptr(), par.data_ptr()
    flt.filter_mode, flt.forward, flt.win_lo, flt.win_hi, flt.states = mode, 0, WINDOW[0], WINDOW[1], S.data_ptr()
    nbytes = C.c_int64(0)
    cabi.check(cabi.lib.tg_ns_hop_weighted_workspace_bytes(C.c_int64(m), C.c_int32(k), C.c_int64(group_cap), C.byref(nbytes)))
    ws = torch.empty(nbytes.value // 8 + 1, **o)
    rng = cabi.TgRng(0x4D6, 9)
    args = (C.byref(graph), C.byref(hin), C.byref(flt), C.byref(rng), C.byref(hout), cabi.ptr(st_out), cabi.ptr(status),
            cabi.ptr(ws), C.c_int64(nbytes.value))
    if groups:
        cabi.check(cabi.lib.tg_ns_hop_weighted_groups(*args, C.c_int64(group_cap), cabi.stream_ptr(DEV)))
    else:
        cabi.check(cabi.lib.tg_ns_hop_weighted(*args, cabi.stream_ptr(DEV)))
    assert int(status.item()) == 0
    return cnt, ep


def _weighted_cases():
    for k in (1, 5, 64):                                        # the batched kernel takes k <= 64
        for n in W_LEN:
            for filtered in (False, True):
                yield "batched", k, n, filtered
    for form in ("flat", "groups"):
        for k in (1, 5, 65):
            for n in (65, 5000, 100000):
                yield form, k, n, n == 5000


@pytest.mark.parametrize("form,k,n_raw,filtered", list(_weighted_cases()))
def test_weighted_law(cabi, weighted_graph, form, k, n_raw, filtered):
    g, ptrs, w, ts = weighted_graph
    v = W_LEN.index(n_raw)
    lo = int(ptrs[v])
    adm = (ts >= WINDOW[0]) & (ts <= WINDOW[1]) if filtered else np.ones(ts.size, dtype=bool)
    rank, n = _ranks(ptrs, v, adm)
    wa = w[lo:lo + n_raw][adm[lo:lo + n_raw]]
    mode = 0 if filtered else -1
    N = _cap(n_outcomes(k) // (2 if form == "batched" else 4), n_raw)
    cnt_each = min(k, n)
    if form == "batched":
        nb = N // B
        out = cabi.NsBatchedOut(nb, B, [k], DEV, with_states=filtered)
        kw = dict(filter_mode=0, window=WINDOW, seeds_state=torch.zeros((nb, B), dtype=torch.int64, device=DEV)) \
            if filtered else {}
        cabi.ns_homo_batched(g, torch.full((nb, B), v, dtype=torch.int64, device=DEV), [k], 0x4D6, 9, out, sampler=2, **kw)
        assert bool((out.counts[:, 1] == B * cnt_each).all())
        raw = out.edge_index[:, :B * cnt_each].reshape(N, cnt_each)
    else:
        cnt, ep = _weighted_flat(cabi, g, torch.full((N,), v, dtype=torch.int64, device=DEV), k, mode, form == "groups",
                                 N * ((n_raw + 511) // 512 + 1) + 1024)
        assert bool((cnt == cnt_each).all())
        raw = ep[:N * cnt_each].reshape(N, cnt_each)
    E = rank[raw - lo].contiguous()
    what = "weighted %s k=%d column %d%s" % (form, k, n_raw, " filtered" if filtered else "")
    if n <= k:
        assert torch.equal(E, torch.arange(n, device=DEV).expand_as(E)), what
        return
    L.check_reservoir(E, L.weighted_law(wa, k), what, zero_pos=_t(wa == 0))


# ---------------------------------------------------------------- walks
@pytest.mark.parametrize("length,pattern", [(2, "all"), (63, "scatter"), (64, "all"), (65, "edges"), (129, "edges"),
                                            (5000, "edges"), (5000, "scatter")])
def test_tempo_walk_step_law(cabi, length, pattern):
    adm = walk_row(length, pattern)
    ptrs, idx, nts, ets = tempo_graph(length, adm)
    g = cabi.graph_view(_t(ptrs), _t(idx))
    start = torch.zeros(N_WALK, dtype=torch.int64, device=DEV)
    w, _ = cabi.tempo_random_walk(g, _t(nts), _t(ets), start, torch.full_like(start, 5), 2, (0, 20), 0x5E7, 1)
    rank = np.full(length + 1, -1)
    rank[adm + 1] = np.arange(adm.size)
    got = torch.bincount(_t(rank)[w[:, 1]] + 1, minlength=adm.size + 1).cpu().numpy()
    assert got[0] == 0, "a walker took a candidate that is not admissible"
    L.chi2_gof(got[1:], L.one_slot_walk_law(adm.size), "tempo walk row %d (%s)" % (length, pattern))
    if pattern == "edges":                                      # the draws reached every chunk that holds a candidate
        assert set((adm[1:] >> 6).tolist()) <= set((adm[np.flatnonzero(got[1:])] >> 6).tolist())


@pytest.mark.parametrize("variant", ["plain", "edge_set", "u32"])
@pytest.mark.parametrize("row", [100, 10000])
def test_node2vec_step_law(cabi, row, variant):
    ptrs, col, n = node2vec_graph(row)
    P, I = _t(ptrs), _t(col)
    g = cabi.graph_view(P, I, indices32=I.to(torch.int32), ptrs32=P.to(torch.int32)) if variant == "u32" \
        else cabi.graph_view(P, I)
    es = cabi.edge_set(g, DEV) if variant == "edge_set" else None
    start = torch.zeros(N_WALK, dtype=torch.int64, device=DEV)
    for p, q in ((0.5, 4.0), (3.0, 0.25)):
        w = cabi.random_walk(g, start, 2, p, q, 0x6F8, 2, edge_set=es)
        assert bool((w[:, 1] == 1).all())
        law = L.node2vec_step_law(ptrs, col, 1, 0, p, q)
        V = np.bincount(col[ptrs[1]:ptrs[2]], weights=law, minlength=n)
        L.chi2_gof(torch.bincount(w[:, 2], minlength=n).cpu().numpy(), V / V.sum(),
                   "node2vec row %d %s p=%g q=%g" % (row, variant, p, q))


@pytest.mark.parametrize("bias", ["uniform", "linear", "exponential"])
@pytest.mark.parametrize("row", [65, 1025, 5000])
def test_biased_walk_step_law(cabi, row, bias):
    times = 5 + np.random.default_rng(row).permutation(row)
    times[[0, np.argmin(times)]] = times[[np.argmin(times), 0]]  # candidate 0 weighs > 0 (else the reference panics)
    ptrs = np.zeros(row + 2, dtype=np.int64)
    ptrs[1:] = row
    g = cabi.graph_view(_t(ptrs), _t(np.arange(1, row + 1)))
    N = N_WALK
    while N > 1024 and N * row * 40 > 1 << 31:                  # the global sort slab: ~40 B per (walker, candidate)
        N //= 2
    start = torch.zeros(N, dtype=torch.int64, device=DEV)
    w, _, status = cabi.biased_tempo_random_walk(g, _t(np.full(row + 1, -1)), _t(times), start, torch.full_like(start, 5),
                                                 2, bias, True, 1, 0x7A9, 3, max_degree=row)
    assert int(status.item()) == 0
    got = torch.bincount(w[:, 1] - 1, minlength=row).cpu().numpy()
    L.chi2_gof(got, L.biased_step_law(times, 5, bias), "biased walk row %d %s" % (row, bias))


# ---------------------------------------------------------------- negative sampling
@pytest.mark.parametrize("tries", [1, 3, 10])
@pytest.mark.parametrize("cover", [0.5, 0.99])
@pytest.mark.parametrize("size", [1000, 100000])
def test_negative_item_law(size, cover, tries):
    import tch_geometric as tg
    rs = np.random.default_rng(size + tries)
    row = np.sort(rs.choice(size, int(cover * size), replace=False))
    ptrs = np.zeros(size + 1, dtype=np.int64)
    ptrs[1:] = row.size
    num_neg = 4
    inputs = torch.zeros(N_NEG // num_neg, dtype=torch.int64, device=DEV)
    tg.seed(0x8B0 + tries)
    s, r, c, _ = tg.negative_sample_neighbors_homogenous(_t(ptrs), _t(row), (size, size), inputs, num_neg, tries)
    got = torch.bincount(s[c], minlength=size + 1).cpu().numpy()
    got[size] = N_NEG - c.numel()
    adm = np.ones(size, dtype=bool)
    adm[row] = False
    adm[0] = False
    L.chi2_gof(got, L.negative_item_law(size, adm, tries), "negatives size %d cover %g tries %d" % (size, cover, tries))
