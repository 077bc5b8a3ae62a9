"""Every entry point's stream-order contract (include/tchgeo.h, the first convention), checked deterministically with
tests/helpers_stream.py: each case runs on a side stream that a blocker holds back, behind device-to-device copies of its
real inputs over decoys and a zero-fill of all its outputs and workspaces, and must leave what the default-stream run
left, bit for bit; a case of class ASYNC must also return while the blocker is still running.  Stream bugs are per launch
site, so the shapes are the smallest that reach each launch chain; values are checked against the oracle elsewhere.

CASES is the table tests/test_stream_contract_cpu.py holds against include/tchgeo.h and _cabi.py; EXEMPT names what has
no case, with the reason."""
import ctypes as C

import pytest
import torch

import helpers_stream as hs
from helpers_stream import ASYNC, READS_BACK, Case

pytestmark = pytest.mark.gpu

_cache = {}


def _cabi():
    from tch_geometric import _cabi
    return _cabi


def _rand(shape, lo, hi, seed, dev, dtype=torch.int64):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g, dtype=dtype).to(dev)


def _graph(dev, key):
    """The graphs of the table, made once on the default stream (tensors are cloned per case):
    "hub": RMAT-13, 2^18 edges, column 0 with 40 000 of them (above TG_LABOR_LONG_COLUMN), column 1 with 20 000 (above the
    16 384 of the long-column lists), as CSC with weights and timestamps and as CSR;
    "r14": RMAT-14, 16 edges per vertex, CSC with its 32-bit shadows (the window-ordered launch);
    "r10": RMAT-10 CSR and CSC with timestamps (walks, skip-gram, link seeds)."""
    if key in _cache:
        return _cache[key]
    cabi = _cabi()
    if key == "hub":
        n = 1 << 13
        row, col = cabi.rmat_edges(13, 1 << 18, 0x51DE, dev)
        col[:40000] = 0
        col[40000:60000] = 1
    elif key == "r14":
        n = 1 << 14
        row, col = cabi.rmat_edges(14, n * 16, 0x5EED0A11, dev)
    else:
        n = 1 << 10
        row, col = cabi.rmat_edges(10, n * 16, 0xA11CE, dev)
    ptrs, idx, _ = cabi.coo_to_csx(row, col, n, n, True)
    rptrs, ridx, _ = cabi.coo_to_csx(row, col, n, n, False)
    E = idx.numel()
    gen = torch.Generator().manual_seed(n)
    d = dict(n=n, E=E, row=row, col=col, ptrs=ptrs, idx=idx, rptrs=rptrs, ridx=ridx,
             w=(torch.rand(E, generator=gen, dtype=torch.float64) * 4 + 0.05).to(dev),
             ts=torch.randint(0, 100, (E,), generator=gen).to(dev),
             node_ts=torch.randint(0, 100, (n,), generator=gen).to(dev),
             idx32=idx.to(torch.int32), ptrs32=ptrs.to(torch.int32),
             max_degree=int((ptrs[1:] - ptrs[:-1]).max()), rmax_degree=int((rptrs[1:] - rptrs[:-1]).max()))
    torch.cuda.synchronize()
    _cache[key] = d
    return d


def _pick(d, *keys, **more):
    out = {k: d[k] for k in keys}
    out.update(more)
    return out


def _view(inp, csr=False, weights=False, ts=False, shadows=False, max_degree=None):
    """A tg_graph over the case's own copies of the arrays (the struct only borrows them)."""
    cabi = _cabi()
    p, i = ("rptrs", "ridx") if csr else ("ptrs", "idx")
    return cabi.graph_view(inp[p], inp[i], inp["w"] if weights else None, inp["ts"] if ts else None,
                           indices32=inp["idx32"] if shadows else None, ptrs32=inp["ptrs32"] if shadows else None,
                           max_degree=max_degree)


def _frontier(d, m, seed, dev, hubs=True):
    v = _rand((m,), 0, d["n"], seed, dev)
    if hubs:
        v[:2] = torch.tensor([0, 1], device=dev)
    return v


# ------------------------------------------------------------------------------------------------ the flat hops
def _hop_case(m, k):
    def make(dev):
        d = _graph(dev, "hub")
        return _pick(d, "ptrs", "idx", v=_frontier(d, m, 100 + m + k, dev))

    def call(inp, T):
        return _cabi().ns_hop(_view(inp), inp["v"], k, 11, call_id=3)
    return Case("ns_hop[m=%d,k=%d]" % (m, k), ["tg_ns_hop", "ns_hop"], ASYNC, make, call, vary=["v"])


def _raw_hop_weighted(T, g, v, states, k, mode, window, group_cap=None):
    """tg_ns_hop_weighted (group_cap None) / tg_ns_hop_weighted_groups, which _cabi does not wrap"""
    cabi = _cabi()
    lib = cabi.lib
    m, dev = v.numel(), v.device
    o = dict(dtype=torch.int64, device=dev)
    cnt, offsets = T.empty(m, **o), T.empty(m + 1, **o)
    nbr, ep, par, st_out = (T.empty(m * k, **o) for _ in range(4))
    status = T.zeros(1, dtype=torch.int32, device=dev)
    hin, hout, flt = cabi.TgHopIn(), cabi.TgHopOut(), cabi.TgHopFilter()
    hin.vertices, hin.m, hin.fanout, hin.sampler, hin.rng_tag = v.data_ptr(), m, k, cabi.SAMPLER_WEIGHTED, 0x31
    hout.cnt, hout.offsets = cnt.data_ptr(), offsets.data_ptr()
    hout.neighbors, hout.edge_ptrs, hout.parents = nbr.data_ptr(), ep.data_ptr(), par.data_ptr()
    flt.filter_mode, flt.forward, flt.win_lo, flt.win_hi, flt.states = mode, 0, window[0], window[1], states.data_ptr()
    nbytes = C.c_int64(0)
    rng = cabi.TgRng(5, 9)
    if group_cap is None:
        cabi.check(lib.tg_ns_hop_scan_workspace_bytes(C.c_int64(m), C.c_int32(k), C.c_int64(1), C.byref(nbytes)))
        ws = T.empty(nbytes.value // 8 + 1, **o)
        cabi.check(lib.tg_ns_hop_weighted(C.byref(g), C.byref(hin), C.byref(flt), C.byref(rng), C.byref(hout), cabi.ptr(st_out),
                                          cabi.ptr(status), cabi.ptr(ws), C.c_int64(nbytes.value), cabi.stream_ptr(dev)))
    else:
        cabi.check(lib.tg_ns_hop_weighted_workspace_bytes(C.c_int64(m), C.c_int32(k), C.c_int64(group_cap), C.byref(nbytes)))
        ws = T.empty(nbytes.value // 8 + 1, **o)
        cabi.check(lib.tg_ns_hop_weighted_groups(C.byref(g), C.byref(hin), C.byref(flt), C.byref(rng), C.byref(hout),
                                                 cabi.ptr(st_out), cabi.ptr(status), cabi.ptr(ws), C.c_int64(nbytes.value),
                                                 C.c_int64(group_cap), cabi.stream_ptr(dev)))
    return cnt, offsets, nbr, ep, par, st_out, status


def _filtered_hop_case(kind, m=600, k=9):
    """the hops under a filter / with weights over the hub graph: columns 0 and 1 are longer than 16 384 edges"""
    cabi_names = {"scan": ["tg_ns_hop_scan", "ns_hop_scan"], "weighted": ["tg_ns_hop_weighted"],
                  "weighted_groups": ["tg_ns_hop_weighted_groups"], "segments": ["tg_ns_hop_segments", "ns_hop_segments"],
                  "segments_weighted": ["tg_ns_hop_segments", "ns_hop_segments"],
                  "recent": ["tg_ns_hop_recent", "ns_hop_recent"], "recent_filtered": ["tg_ns_hop_recent", "ns_hop_recent"],
                  "labor": ["tg_ns_hop_labor", "ns_hop_labor"], "labor_filtered": ["tg_ns_hop_labor", "ns_hop_labor"]}[kind]

    def make(dev):
        d = _graph(dev, "hub")
        return _pick(d, "ptrs", "idx", "w", "ts", v=_frontier(d, m, 7 + len(kind), dev), st=_rand((m,), 20, 80, 3, dev))

    def call(inp, T):
        cabi = _cabi()
        v, st = inp["v"], inp["st"]
        if kind == "scan":
            return cabi.ns_hop_scan(_view(inp, ts=True), v, st, k, 5, cabi.FILTER_STATIC, (10, 60), call_id=9)
        if kind == "weighted":
            return _raw_hop_weighted(T, _view(inp, weights=True, ts=True), v, st, k, cabi.FILTER_DYNAMIC, (0, 30))
        if kind == "weighted_groups":
            return _raw_hop_weighted(T, _view(inp, weights=True, ts=True), v, st, k, cabi.FILTER_DYNAMIC, (0, 30), group_cap=8192)
        if kind in ("segments", "segments_weighted"):
            weighted = kind == "segments_weighted"
            g = _view(inp, weights=weighted, ts=True)
            segs = [(g, 0, k, 0x21), (g, m // 2, 3, 0x22)]
            return cabi.ns_hop_segments(segs, v, st, 5, filter_mode=cabi.FILTER_STATIC, window=(10, 60), call_id=9,
                                        sampler=cabi.SAMPLER_WEIGHTED if weighted else cabi.SAMPLER_UNIFORM)
        if kind == "recent":
            return cabi.ns_hop_recent(_view(inp, ts=True), v, k)
        if kind == "recent_filtered":
            return cabi.ns_hop_recent(_view(inp, ts=True), v, k, states=st, filter_mode=cabi.FILTER_STATIC, window=(10, 60))
        if kind == "labor":
            return cabi.ns_hop_labor(_view(inp), v, k, 5, 9)
        return cabi.ns_hop_labor(_view(inp, ts=True), v, k, 5, 9, states=st, filter_mode=cabi.FILTER_STATIC, window=(10, 60))
    return Case("ns_hop_%s" % kind, cabi_names, ASYNC, make, call, vary=["v"])


# ------------------------------------------------------------------------------------------------ the batched launch
WINDOWED, FUSED, WINDOWED_WIDE = 1, 2, 3


def _homo_outputs(out):
    return (out.samples, out.rows, out.cols, out.edge_index, out.layer_offsets, out.counts, out.states)


def _homo_fused_case(k):
    fan = [k, 3]

    def make(dev):
        d = _graph(dev, "hub")
        return _pick(d, "ptrs", "idx", seeds=_rand((5, 33), 0, d["n"], k, dev))

    def call(inp, T):
        cabi = _cabi()
        out = cabi.NsBatchedOut(5, 33, fan, inp["seeds"].device)
        cabi.ns_homo_batched(_view(inp), inp["seeds"], fan, 17, 300, out, form=FUSED)
        return _homo_outputs(out)
    return Case("ns_homo_batched[fused,k=%d]" % k, ["tg_ns_homo_batched", "ns_homo_batched", "tg_ns_rows_fill", "ns_rows_fill"],
                ASYNC, make, call, vary=["seeds"])


def _homo_flat_case(kind):
    """few batches with a workspace of tg_ns_homo_batched_workspace_bytes: the flat path (a chain of flat hops)"""
    fan = [4, 3]

    def make(dev):
        d = _graph(dev, "hub")
        return _pick(d, "ptrs", "idx", "w", "ts", seeds=_rand((6, 20), 0, d["n"], 9, dev), st=_rand((6, 20), 20, 80, 4, dev))

    def call(inp, T):
        cabi = _cabi()
        sampler, mode = {"plain": (cabi.SAMPLER_UNIFORM, cabi.FILTER_NONE), "filtered": (cabi.SAMPLER_UNIFORM, cabi.FILTER_DYNAMIC),
                         "weighted": (cabi.SAMPLER_WEIGHTED, cabi.FILTER_NONE), "recent": (cabi.SAMPLER_RECENT, cabi.FILTER_STATIC),
                         "labor": (cabi.SAMPLER_LABOR, cabi.FILTER_NONE)}[kind]
        dev = inp["seeds"].device
        g = _view(inp, weights=sampler == cabi.SAMPLER_WEIGHTED, ts=True)
        ws = cabi.ns_homo_batched_workspace(g, 6, 20, fan, dev, sampler=sampler, filter_mode=mode)
        assert ws is not None
        out = cabi.NsBatchedOut(6, 20, fan, dev, with_states=True)
        cabi.ns_homo_batched(g, inp["seeds"], fan, 17, 300, out, sampler=sampler, filter_mode=mode, window=(0, 40),
                             seeds_state=inp["st"] if mode != cabi.FILTER_NONE else None, ws=ws)
        return _homo_outputs(out)
    return Case("ns_homo_batched_ws[flat,%s]" % kind, ["tg_ns_homo_batched_ws", "ns_homo_batched"], ASYNC, make, call,
                vary=["seeds"])


def _homo_windowed_case(label, tuning, form, ptrs32=True):
    """the window-ordered forms on RMAT-14 with 16 KiB windows, as test_gpu_slab_alignment.py: the push form (its
    optional fusions off, narrow and wide items), the staged pipeline (narrow items only; its first kernel with 32-bit
    and, without the ptrs32 shadow, 64-bit column starts) and its parts / concurrent / split / coarse-only branches"""
    nb, B, fan = 6, 1023, [15, 10]
    staged = tuning.get("staged") == 1

    def make(dev):
        d = _graph(dev, "r14")
        return _pick(d, "ptrs", "idx", "idx32", "ptrs32", seeds=_rand((nb, B), 0, d["n"], 31, dev))

    def call(inp, T):
        cabi = _cabi()
        dev = inp["seeds"].device
        g = cabi.graph_view(inp["ptrs"], inp["idx"], indices32=inp["idx32"], ptrs32=inp["ptrs32"] if ptrs32 else None,
                            max_degree=_graph(dev, "r14")["max_degree"])
        before = cabi.ns_win_tuning_set(window_bytes=1 << 14, **tuning)
        try:
            out = cabi.NsBatchedOut(nb, B, fan, dev)
            ws = cabi.ns_homo_workspace(nb, B, fan, dev, staged=staged, graph=g)
            assert cabi.ns_homo_batched_form(g, out, nb, B, fan, ws=ws, form=form)[0] == form
            assert cabi.ns_homo_batched_staged(g, out, nb, B, fan, ws=ws, form=form) == staged
            cabi.ns_homo_batched(g, inp["seeds"], fan, 17, 300, out, ws=ws, form=form)
        finally:
            cabi.ns_win_tuning_set(**before)
        return _homo_outputs(out)
    return Case("ns_homo_batched_ws[%s]" % label, ["tg_ns_homo_batched_ws", "ns_homo_batched", "ns_homo_workspace"], ASYNC,
                make, call, vary=["seeds"])


WINDOWED_FORMS = [
    ("push", dict(staged=0), WINDOWED),
    ("push_wide", dict(staged=0), WINDOWED_WIDE),
    ("push_plain", dict(staged=0, fold_hist=0, fuse_first_hops=0, direct_hop0=0), WINDOWED),
    ("staged", dict(staged=1), WINDOWED),
    ("staged_cols64", dict(staged=1), WINDOWED, False),
    ("staged_parts", dict(staged=1, stage_parts=2, stage_part_min_batches=1), WINDOWED),
    ("staged_parts_concurrent", dict(staged=1, stage_parts=2, stage_part_min_batches=1, stage_concurrent=1), WINDOWED),
    ("staged_split", dict(staged=1, stage_split=1), WINDOWED),
    ("staged_coarse", dict(staged=1, stage_fine=0), WINDOWED),
]


# ------------------------------------------------------------------------------------------------ walks
def _walk_case(label, p, q, with_set=False):
    def make(dev):
        d = _graph(dev, "r10")
        return _pick(d, "rptrs", "ridx", start=_rand((300,), 0, d["n"], 12, dev))

    def call(inp, T):
        cabi = _cabi()
        g = _view(inp, csr=True)
        es = cabi.edge_set(g, inp["start"].device) if with_set else None
        return (cabi.random_walk(g, inp["start"], 12, p, q, 5, 8, edge_set=es),)
    names = ["tg_random_walk_es", "tg_edge_set_build", "edge_set", "random_walk"] if with_set else ["tg_random_walk", "random_walk"]
    return Case("random_walk[%s]" % label, names, ASYNC, make, call, vary=["start"])


def _edge_set_case():
    """the set's layout may depend on insertion order: its sorted words are what the call determines"""
    def make(dev):
        return _pick(_graph(dev, "r10"), "rptrs", "ridx")

    def call(inp, T):
        return (torch.sort(_cabi().edge_set(_view(inp, csr=True), inp["ridx"].device))[0],)
    return Case("edge_set_build", ["tg_edge_set_build", "edge_set"], ASYNC, make, call, vary=["ridx"])


def _tempo_walk_case(biased):
    def make(dev):
        d = _graph(dev, "r10")
        ts = d["ts"][:d["ridx"].numel()]
        return _pick(d, "rptrs", "ridx", "node_ts", ets=ts, start=_rand((300,), 0, d["n"], 13, dev), sts=_rand((300,), 0, 50, 14, dev))

    def call(inp, T):
        cabi = _cabi()
        g = _view(inp, csr=True)
        if biased:
            return cabi.biased_tempo_random_walk(g, inp["node_ts"], inp["ets"], inp["start"], inp["sts"], 10, "exponential", True,
                                                 3, 5, 8, max_degree=_graph(inp["start"].device, "r10")["rmax_degree"])
        return cabi.tempo_random_walk(g, inp["node_ts"], inp["ets"], inp["start"], inp["sts"], 10, (0, 60), 5, 8)
    name = "biased_tempo_random_walk" if biased else "tempo_random_walk"
    return Case(name, ["tg_" + name, name], ASYNC, make, call, vary=["start"])


# ------------------------------------------------------------------------------------------------ plumbing
def _ingest_case(csc):
    def make(dev):
        d = _graph(dev, "r10")
        return _pick(d, "row", "col")

    def call(inp, T):
        n = 1 << 10
        return _cabi().coo_to_csx(inp["row"], inp["col"], n, n, csc)
    return Case("coo_to_csx[%s]" % ("csc" if csc else "csr"), ["tg_coo_to_csx", "coo_to_csx"], ASYNC, make, call,
                vary=["row"])


def _plumbing_cases():
    cases = []

    def make_sorted(dev):
        return dict(ind=torch.sort(_rand((5000,), 0, 700, 21, dev))[0])

    # a permuted `ind` would not be sorted: the zero-fill carries the check
    cases.append(Case("ind2ptr", ["tg_ind2ptr", "ind2ptr"], ASYNC, make_sorted,
                      lambda inp, T: (_cabi().ind2ptr(inp["ind"], 700),)))

    def make_values(dev):
        v = _rand((4097,), 0, 1000, 22, dev)
        v[::7] = 5000                                      # outside [0, 1000): the flag and the replaced words are not zero
        return dict(v=v)

    def check_range(inp, T):
        cabi = _cabi()
        flag = T.zeros(2, dtype=torch.int32, device=inp["v"].device)
        cabi.check(cabi.lib.tg_check_range(cabi.ptr(inp["v"]), C.c_int64(inp["v"].numel()), C.c_int64(0), C.c_int64(1000),
                                           cabi.ptr(flag), cabi.stream_ptr(inp["v"].device)))
        return (flag,)

    def sanitize_range(inp, T):
        cabi = _cabi()
        v = inp["v"]
        out, flag = T.empty(v.numel(), dtype=torch.int64, device=v.device), T.zeros(1, dtype=torch.int64, device=v.device)
        cabi.check(cabi.lib.tg_sanitize_range(cabi.ptr(v), C.c_int64(v.numel()), C.c_int64(3), C.c_int64(1000), cabi.ptr(out),
                                              cabi.ptr(flag), cabi.stream_ptr(v.device)))
        return out, flag
    # tg_check_range: the decoy is a permutation, so its flag is the same word; the zero-fill carries the check
    cases.append(Case("check_range", ["tg_check_range"], ASYNC, make_values, check_range))
    cases.append(Case("sanitize_range", ["tg_sanitize_range"], ASYNC, make_values, sanitize_range, vary=["v"]))

    def make_graph(dev):
        return _pick(_graph(dev, "hub"), "ptrs", "idx", "ptrs32")

    def max_degree(inp, T):
        cabi = _cabi()
        dev = inp["ptrs"].device
        out = T.zeros(1, dtype=torch.int64, device=dev)
        g = cabi.graph_view(inp["ptrs"], inp["idx"])
        cabi.check(cabi.lib.tg_graph_max_degree(C.byref(g), cabi.ptr(out), cabi.stream_ptr(dev)))
        return (out,)
    # a permuted ptrs array would not be a graph: the zero-fill carries the check
    cases.append(Case("graph_max_degree", ["tg_graph_max_degree"], ASYNC, make_graph, max_degree))
    cases.append(Case("graph_max_degree[wrapper]", ["graph_max_degree"], READS_BACK, make_graph,
                      lambda inp, T: (torch.tensor([_cabi().graph_max_degree(_cabi().graph_view(inp["ptrs"], inp["idx"]),
                                                                             inp["ptrs"].device)], device=inp["ptrs"].device),)))

    def make_slab(dev):
        lens = _rand((37,), 0, 50, 23, dev)
        return dict(slab=_rand((37, 50), 1, 1 << 40, 24, dev), lens=lens)

    def compact_rows(inp, T):
        return (_cabi().compact_rows(inp["slab"], inp["lens"], _cache["compact_total"]),)

    def make_slab_total(dev):
        inp = make_slab(dev)
        _cache["compact_total"] = int(inp["lens"].sum())
        return inp
    cases.append(Case("compact_rows", ["tg_compact_rows", "compact_rows"], ASYNC, make_slab_total, compact_rows, vary=["slab"]))

    for row_bytes, dtype, cols in ((16, torch.int64, 2), (8, torch.int64, 1), (4, torch.int32, 1), (1, torch.uint8, 3)):
        def make_rows(dev, dtype=dtype, cols=cols):
            hi = 200 if dtype == torch.uint8 else 1 << 30
            return dict(src=_rand((999, cols), 1, hi, 25, dev, dtype=dtype), index=_rand((3001,), 0, 999, 26, dev))
        cases.append(Case("gather_rows[%d-byte]" % row_bytes, ["tg_gather_rows", "gather_rows"], ASYNC, make_rows,
                          lambda inp, T: _cabi().gather_rows(inp["src"], inp["index"]), vary=["index"]))

    # no device input: the zero-fill alone carries the check
    cases.append(Case("rmat_edges", ["tg_rmat_edges", "rmat_edges"], ASYNC, lambda dev: {},
                      lambda inp, T: _cabi().rmat_edges(12, 50001, 77, torch.device("cuda", torch.cuda.current_device()))))
    cases.append(Case("rmat_edges_rect", ["tg_rmat_edges_rect", "rmat_edges_rect"], ASYNC, lambda dev: {},
                      lambda inp, T: _cabi().rmat_edges_rect(9, 12, 50001, 78, torch.device("cuda", torch.cuda.current_device()))))
    cases.append(Case("seed_batches", ["tg_seed_batches", "seed_batches"], ASYNC, lambda dev: {},
                      lambda inp, T: (_cabi().seed_batches(5, 3, 7, 129, 1 << 20, torch.device("cuda", torch.cuda.current_device())),)))

    def rows_fill(inp, T):
        rows = T.empty((7, 333), dtype=torch.int64, device=torch.device("cuda", torch.cuda.current_device()))
        _cabi().ns_rows_fill(rows, 40)
        return (rows,)
    cases.append(Case("ns_rows_fill", ["tg_ns_rows_fill", "ns_rows_fill"], ASYNC, lambda dev: {}, rows_fill))
    return cases


# ------------------------------------------------------------------------------------------------ behind the forest
def _sized(key, chain):
    """A chain whose flat outputs are sized by counts the host must know: make() runs it once on the default stream and
    keeps the sizes, so that the measured run needs no read-back.  chain(inp, T, sizes) -> (outputs, sizes)."""
    def remember(make):
        def made(dev):
            real = make(dev)
            _cache[key] = chain({k: v.clone() for k, v in real.items()}, torch, None)[1]
            torch.cuda.synchronize()
            return real
        return made
    return remember, lambda inp, T: chain(inp, T, _cache[key])[0]


NB, B, FAN = 5, 33, [6, 3]


def _forest_inputs(dev):
    d = _graph(dev, "r10")
    return _pick(d, "ptrs", "idx", "ts", seeds=_rand((NB, B), 0, d["n"], 41, dev))


def _forest(inp):
    cabi = _cabi()
    out = cabi.NsBatchedOut(NB, B, FAN, inp["seeds"].device)
    cabi.ns_homo_batched(_view(inp), inp["seeds"], FAN, 17, 300, out, form=FUSED)
    return out


def _prefix(n):
    return torch.cumsum(n, 0) - n


def _compact_case():
    def chain(inp, T, sizes):
        cabi = _cabi()
        out = _forest(inp)
        if sizes is None:
            sizes = out.counts.cpu()
        return cabi.ns_homo_compact(out, NB, sizes), sizes
    remember, call = _sized("compact", chain)
    return Case("ns_homo_compact", ["tg_ns_homo_compact", "ns_homo_compact"], ASYNC, remember(_forest_inputs), call, vary=["seeds"])


def _unique_case(grouped, form):
    def call(inp, T):
        cabi = _cabi()
        out = _forest(inp)
        n = inp["ptrs"].numel() - 1
        res = (cabi.ns_homo_unique_grouped if grouped else cabi.ns_homo_unique)(out, NB, n, form=form)
        return res.nodes, res.inverse, res.rows, res.cols, res.counts, res.layer_nodes, res.group
    name = "ns_homo_unique_grouped" if grouped else "ns_homo_unique"
    return Case("%s[form=%d]" % (name, form), ["tg_" + name, name], ASYNC, _forest_inputs, call, vary=["seeds"])


def _induced_case(grouped):
    def chain(inp, T, total):
        cabi = _cabi()
        out = _forest(inp)
        n, dev = inp["ptrs"].numel() - 1, inp["seeds"].device
        if grouped:
            res = cabi.ns_homo_unique_grouped(out, NB, n)
            ind = cabi.NsInducedGrouped(_view(inp), res.nodes, res.group, res.counts, 2, NB, n, n_groups=B).count()
        else:
            res = cabi.ns_homo_unique(out, NB, n)
            ind = cabi.NsInduced(_view(inp), res.nodes, res.counts, 2, NB, n).count()
        if total is None:
            total = int(ind.n_edges.sum())
        trip = T.empty((3, max(total, 1)), dtype=torch.int64, device=dev)
        ind.emit(_prefix(ind.n_edges), trip[0], trip[1], trip[2])
        return (ind.state, trip), total
    name = "ns_induced_grouped" if grouped else "ns_induced"
    remember, call = _sized(name, chain)
    wrappers = ["NsInducedGrouped.count", "NsInducedGrouped.emit"] if grouped else ["NsInduced.count", "NsInduced.emit"]
    return Case(name, ["tg_%s_count" % name, "tg_%s_emit" % name] + wrappers, ASYNC, remember(_forest_inputs), call,
                vary=["seeds"])


def _full_case():
    def make(dev):
        d = _graph(dev, "r10")
        g = torch.Generator().manual_seed(5)
        return _pick(d, "ptrs", "idx", nodes=torch.randperm(d["n"], generator=g)[:205].to(dev),
                     node_ptr=torch.tensor([0, 40, 105, 205], device=dev))

    def chain(inp, T, totals):
        cabi = _cabi()
        n, dev = inp["ptrs"].numel() - 1, inp["nodes"].device
        op = cabi.NsFull(_view(inp), n, 128, 2048, 0, 3, dev)
        n_nodes, n_edges, _, _ = op.count(inp["nodes"], inp["node_ptr"])
        if totals is None:
            totals = (int(n_nodes.sum()), int(n_edges.sum()))
        nodes_out = T.empty(max(totals[0], 1), dtype=torch.int64, device=dev)
        trip = T.empty((3, max(totals[1], 1)), dtype=torch.int64, device=dev)
        op.emit(_prefix(n_nodes), _prefix(n_edges), nodes_out, trip[0], trip[1], trip[2])
        return (op.state, nodes_out, trip), totals
    remember, call = _sized("ns_full", chain)
    return Case("ns_full", ["tg_ns_full_count", "tg_ns_full_emit", "NsFull.count", "NsFull.emit"], ASYNC, remember(make), call,
                vary=["nodes"])


def _cluster_case():
    def make(dev):
        d = _graph(dev, "r10")
        g = torch.Generator().manual_seed(6)
        return _pick(d, "ptrs", "idx", partptr=torch.arange(0, d["n"] + 1, 64, device=dev),
                     clusters=torch.randperm(16, generator=g)[:12].view(3, 4).contiguous().to(dev))

    def chain(inp, T, totals):
        cabi = _cabi()
        dev = inp["clusters"].device
        cl = cabi.ClusterInduced(_view(inp), inp["partptr"], inp["clusters"]).count()
        if totals is None:
            totals = (int(cl.n_nodes.sum()), int(cl.n_edges.sum()))
        nodes = T.empty(max(totals[0], 1), dtype=torch.int64, device=dev)
        trip = T.empty((3, max(totals[1], 1)), dtype=torch.int64, device=dev)
        cl.emit_into(_prefix(cl.n_nodes), _prefix(cl.n_edges), nodes, trip[0], trip[1], trip[2])
        return (cl.state, nodes, trip), totals
    remember, call = _sized("cluster", chain)
    return Case("cluster", ["tg_cluster_count", "tg_cluster_emit", "ClusterInduced.count", "ClusterInduced.emit_into"], ASYNC,
                remember(make), call, vary=["clusters"])


# ------------------------------------------------------------------------------------------------ typed samplers
def _typed_inputs(dev):
    d = _graph(dev, "r10")
    return _pick(d, "ptrs", "idx", "rptrs", "ridx", "ts", a=_rand((4, 8), 0, d["n"], 51, dev), b=_rand((4, 5), 0, d["n"], 52, dev),
                 a_ts=_rand((4, 8), 0, 100, 53, dev))


def _typed_rels(inp, tail):
    """two node types of 2^10 nodes each, three relations: a->a, a->b, b->a"""
    return [(0, 0, inp["ptrs"], inp["idx"], tail(0)), (0, 1, inp["rptrs"], inp["ridx"], tail(1)), (1, 0, inp["ptrs"], inp["idx"], tail(2))]


def _flat(*lists):
    return [t for x in lists for t in (x if isinstance(x, (list, tuple)) else [x])]


def _hetero_batched(inp):
    cabi = _cabi()
    fan = [[3, 2], [2, 2], [2, 1]]
    hb = cabi.NsHeteroBatched(2, _typed_rels(inp, lambda r: fan[r]), [inp["a"], inp["b"]], 2, 4, inp["a"].device)
    hb.run(17, 300)
    return hb


def _hetero_batched_case():
    def call(inp, T):
        hb = _hetero_batched(inp)
        return _flat(hb.samples, hb.rows, hb.cols, hb.edge_index, hb.layer_offsets, hb.counts)
    return Case("ns_hetero_batched", ["tg_ns_hetero_batched", "NsHeteroBatched.run"], ASYNC, _typed_inputs, call, vary=["a", "b"])


def _typed_unique_case(form):
    def call(inp, T):
        n = inp["ptrs"].numel() - 1
        res = _cabi().ns_typed_unique(_hetero_batched(inp), 4, [n, n], form=form)
        return _flat(res.nodes, res.inverse, res.rows, res.cols, res.state)
    return Case("ns_typed_unique[form=%d]" % form, ["tg_ns_typed_unique", "ns_typed_unique"], ASYNC, _typed_inputs, call,
                vary=["a", "b"])


def _batched_typed_case(kind):
    def call(inp, T):
        cabi = _cabi()
        dev = inp["a"].device
        n = inp["ptrs"].numel() - 1
        if kind == "hgt":
            op = cabi.HgtBatched(2, _typed_rels(inp, lambda r: inp["ts"] if r == 0 else None), [inp["a"], None], [[6, 4], [5, 3]], 2, 4,
                                 dev, input_ts=[inp["a_ts"], None])
        elif kind == "budget":
            op = cabi.BudgetBatched(2, _typed_rels(inp, lambda r: inp["ts"] if r == 0 else None), [inp["a"], None], [[4, 2], [3, 2]],
                                    2, 4, dev, input_ts=[inp["a_ts"], None], window=(0, 50))
        else:
            op = cabi.NegBatched(2, [(0, 0, inp["rptrs"], inp["ridx"], n), (0, 1, inp["rptrs"], inp["ridx"], n),
                                     (1, 0, inp["rptrs"], inp["ridx"], n)], [inp["a"], inp["b"]], 3, 4, 4, dev)
        op.run(17, 300)
        return _flat(*[getattr(op, k) for k in op.NODE_SLABS + op.EDGE_SLABS], op.state)
    name = {"hgt": "tg_hgt_sample_batched", "budget": "tg_budget_sample_batched", "neg": "tg_neg_sample_batched"}[kind]
    return Case(name[3:], [name, "_Batched.run"], ASYNC, _typed_inputs, call, vary=["a", "b"])


def _budget_layer_case():
    def call(inp, T):
        rels = [(0, 0, inp["ptrs"], inp["idx"], inp["ts"]), (1, 0, inp["ptrs"], inp["idx"], None)]
        return _cabi().budget_layer(rels, [0, 2], 0, 4, inp["a"].view(-1), inp["a_ts"].view(-1), 17, 300, window=(0, 50))
    return Case("budget_layer", ["tg_budget_layer", "budget_layer"], ASYNC, _typed_inputs, call, vary=["a"])


class TgHgtOut(C.Structure):
    _fields_ = [("samples", C.POINTER(C.c_void_p)), ("sample_ts", C.POINTER(C.c_void_p)), ("rows", C.POINTER(C.c_void_p)),
                ("cols", C.POINTER(C.c_void_p)), ("edge_index", C.POINTER(C.c_void_p)), ("n_samples", C.c_void_p),
                ("n_edges", C.c_void_p), ("panic", C.c_void_p)]


class TgBudgetOut(C.Structure):
    _fields_ = [("samples", C.POINTER(C.c_void_p)), ("sample_ts", C.POINTER(C.c_void_p)), ("cap_nodes", C.POINTER(C.c_int64)),
                ("rows", C.POINTER(C.c_void_p)), ("cols", C.POINTER(C.c_void_p)), ("edge_index", C.POINTER(C.c_void_p)),
                ("cap_edges", C.POINTER(C.c_int64)), ("counts", C.c_void_p)]


class TgNegOut(C.Structure):
    _fields_ = [("samples", C.POINTER(C.c_void_p)), ("rows", C.POINTER(C.c_void_p)), ("cols", C.POINTER(C.c_void_p)),
                ("n_samples", C.c_void_p), ("n_edges", C.c_void_p), ("panic", C.c_void_p)]


def _single_typed_case(kind, graph="r10", quota=None):
    """the single-call operators at the C ABI (the operator surface calls them): one node type, one relation.  hgt with a
    quota above 20 971 plans layers of more than 16 384 chunks of 64 candidates: the library scan with its workspace."""
    def make(dev):
        d = _graph(dev, graph)
        return _pick(d, "ptrs", "idx", "rptrs", "ridx", a=_rand((64,), 0, d["n"], 61, dev))

    def call(inp, T):
        cabi = _cabi()
        lib, dev = cabi.lib, inp["a"].device
        n = inp["ptrs"].numel() - 1
        o = dict(dtype=torch.int64, device=dev)
        nbytes = C.c_int64(0)
        rng = cabi.TgRng(17, 300)
        vp = cabi._vp
        if kind == "hgt":
            q = [quota, 10] if quota else [20, 10]
            p = cabi.hgt_problem(1, [(0, 0, inp["ptrs"], inp["idx"], None)], [64], [q], 2, inputs=[inp["a"]])
            cap = 64 + sum(q)
            S, TS = T.empty(cap, **o), T.empty(cap, **o)
            trip = T.empty((3, 50 * cap), **o)
            counts, panic = T.zeros(2, **o), T.zeros(1, dtype=torch.int32, device=dev)
            keep = [vp([S]), vp([TS]), vp([trip[0]]), vp([trip[1]]), vp([trip[2]])]
            out = TgHgtOut(*keep, counts[:1].data_ptr(), counts[1:].data_ptr(), panic.data_ptr())
            cabi.check(lib.tg_hgt_workspace_bytes(C.byref(p), C.byref(nbytes)))
            ws = T.empty(nbytes.value // 8 + 1, **o)
            cabi.check(lib.tg_hgt_sample(C.byref(p), C.byref(rng), C.byref(out), cabi.ptr(ws), C.c_int64(nbytes.value),
                                         cabi.stream_ptr(dev)))
            return S, TS, trip, counts, panic
        if kind == "budget":
            p = cabi.budget_problem(1, [(0, 0, inp["ptrs"], inp["idx"], None)], [64], [[5, 3]], 2, inputs=[inp["a"]])
            cn, ce = cabi.budget_capacity(p)
            S, TS = T.empty(max(cn[0], 1), **o), T.empty(max(cn[0], 1), **o)
            trip = T.empty((3, max(ce[0], 1)), **o)
            counts = T.zeros(2, **o)
            keep = [vp([S]), vp([TS]), cabi._i64(cn), vp([trip[0]]), vp([trip[1]]), vp([trip[2]]), cabi._i64(ce)]
            out = TgBudgetOut(*keep, counts.data_ptr())
            cabi.check(lib.tg_budget_workspace_bytes(C.byref(p), C.byref(nbytes)))
            ws = T.empty(nbytes.value // 8 + 1, **o)
            cabi.check(lib.tg_budget_sample(C.byref(p), C.byref(rng), C.byref(out), cabi.ptr(ws), C.c_int64(nbytes.value),
                                            cabi.stream_ptr(dev)))
            return S, TS, trip, counts
        p = cabi.neg_problem(1, [(0, 0, inp["rptrs"], inp["ridx"], n)], [64], 3, 4, inputs=[inp["a"]], homogeneous=True)
        S = T.empty(64 + 64 * 3, **o)
        pair = T.empty((2, 64 * 3), **o)
        counts, panic = T.zeros(2, **o), T.zeros(1, dtype=torch.int32, device=dev)
        keep = [vp([S]), vp([pair[0]]), vp([pair[1]])]
        out = TgNegOut(*keep, counts[:1].data_ptr(), counts[1:].data_ptr(), panic.data_ptr())
        cabi.check(lib.tg_neg_workspace_bytes(C.byref(p), C.byref(nbytes)))
        ws = T.empty(nbytes.value // 8 + 1, **o)
        cabi.check(lib.tg_neg_sample(C.byref(p), C.byref(rng), C.byref(out), cabi.ptr(ws), cabi.stream_ptr(dev)))
        return S, pair, counts, panic
    label = "%s_sample%s" % (kind, "[library scan]" if quota else "")
    return Case(label, ["tg_%s_sample" % kind], ASYNC, make, call, vary=["a"])


# ------------------------------------------------------------------------------------------------ skip-gram, PinSAGE
def _skipgram_case(kind, form):
    def make(dev):
        d = _graph(dev, "r10")
        return _pick(d, "rptrs", "ridx", "node_ts", "ts", seeds=_rand((3, 20), 0, d["n"], 71, dev), sts=_rand((3, 20), 0, 50, 72, dev))

    def call(inp, T):
        cabi = _cabi()
        g = _view(inp, csr=True)
        n = g.n_major
        if kind == "rw":
            return cabi.rw_skipgram(g, inp["seeds"], 8, 4, 2, 1, 1.0, 1.0, 17, 300, n, form=form)
        if kind == "mp":
            cfg = cabi.mp_skipgram_config([g, g], [0, 1], [1, 0], [n, n], 6, 3, 1, 1, type_start=[0, n], pad_value=2 * n)
            return cabi.mp_skipgram(cfg, inp["seeds"], 17, 300, form=form)
        cfg = cabi.tempo_skipgram_config(6, 3, (0, 60), 1, 1, n)
        return cabi.tempo_skipgram(g, inp["node_ts"], inp["ts"], inp["seeds"], inp["sts"], cfg, 17, 300)
    name = "%s_skipgram" % {"rw": "rw", "mp": "mp", "tempo": "tempo"}[kind]
    return Case("%s[form=%d]" % (name, form), ["tg_" + name, name], ASYNC, make, call, vary=["seeds"])


def _pinsage_case():
    def make(dev):
        d = _graph(dev, "r10")
        return _pick(d, "ptrs", "idx", v=_frontier(d, 300, 73, dev, hubs=False))

    def call(inp, T):
        return _cabi().pinsage_hop(_view(inp), inp["v"], 5, 8, 3, 0.3, 17, 300)
    return Case("pinsage_hop", ["tg_pinsage_hop", "pinsage_hop"], ASYNC, make, call, vary=["v"])


# ------------------------------------------------------------------------------------------------ seeds and node lists
def _link_case(typed, with_set):
    def make(dev):
        d = _graph(dev, "r10")
        return _pick(d, "ptrs", "idx", src=d["row"][:120].view(3, 40).contiguous(), dst=d["col"][:120].view(3, 40).contiguous())

    def call(inp, T):
        cabi = _cabi()
        g = _view(inp)
        n = g.n_major
        es = cabi.edge_set(g, inp["src"].device) if with_set else None
        if typed:
            return cabi.link_seeds_typed(g, inp["src"], inp["dst"], 2, cabi.LINK_TRIPLET, 5, 17, 300, n, n, True, edge_set=es)
        return cabi.link_seeds(g, inp["src"], inp["dst"], 2, cabi.LINK_BINARY, 5, 17, 300, n, edge_set=es)
    name = "link_seeds_typed" if typed else "link_seeds"
    return Case("%s[%s]" % (name, "edge_set" if with_set else "rows"), ["tg_" + name, name], ASYNC, make, call, vary=["src", "dst"])


def _saint_case(kind, form):
    def make(dev):
        d = _graph(dev, "r10")
        deg, rdeg = d["ptrs"][1:] - d["ptrs"][:-1], d["rptrs"][1:] - d["rptrs"][:-1]
        return _pick(d, "ptrs", "idx", "rptrs", "ridx", roots=_rand((3, 20), 0, d["n"], 81, dev),
                     cols=torch.nonzero(deg).view(-1).contiguous(), rows=torch.nonzero(rdeg).view(-1).contiguous())

    def call(inp, T):
        cabi = _cabi()
        if kind == "rw":
            return cabi.saint_rw_nodes(_view(inp, csr=True), inp["roots"], 4, 17, 300, form=form)
        if kind == "node":
            return cabi.saint_node_nodes(_view(inp), 50, 3, 17, 300, form=form)
        return cabi.saint_edge_nodes(_view(inp), inp["cols"], _view(inp, csr=True), inp["rows"], 40, 3, 17, 300, form=form)
    name = "saint_%s_nodes" % kind
    return Case("%s[form=%d]" % (name, form), ["tg_" + name, name], ASYNC, make, call,
                vary={"rw": ["roots"], "node": ["idx"], "edge": ["cols", "rows"]}[kind])


def _saint_coverage_case():
    def make(dev):
        d = _graph(dev, "r10")
        return dict(nodes=_rand((4, 50), 0, d["n"], 82, dev), counts=_rand((4,), 10, 40, 83, dev), ids=_rand((500,), 0, d["E"], 84, dev),
                    node_count=torch.zeros(d["n"], dtype=torch.int64, device=dev), edge_count=torch.zeros(d["E"], dtype=torch.int64, device=dev))

    def call(inp, T):
        status = _cabi().saint_coverage_add(inp["nodes"], inp["counts"], inp["node_count"], inp["edge_count"], edge_ids=inp["ids"])
        return inp["node_count"], inp["edge_count"], status
    return Case("saint_coverage_add", ["tg_saint_coverage_add", "saint_coverage_add"], ASYNC, make, call, vary=["nodes"])


def _saint_norm_case():
    def make(dev):
        d = _graph(dev, "r10")
        return _pick(d, "ptrs", "idx", node_count=_rand((d["n"],), 1, 30, 85, dev), edge_count=_rand((d["E"],), 1, 30, 86, dev))

    def call(inp, T):
        return _cabi().saint_norm(_view(inp), inp["node_count"], inp["edge_count"], 30)
    return Case("saint_norm", ["tg_saint_norm", "saint_norm"], ASYNC, make, call, vary=["node_count", "edge_count"])


# ------------------------------------------------------------------------------------------------ the tg_het_* steps
class TgHetEntry(C.Structure):
    _fields_ = [("rel", C.c_int32), ("src", C.c_int32), ("dst", C.c_int32), ("segment", C.c_int32),
                ("begin", C.c_int64), ("cap", C.c_int64),
                ("list_dst", C.c_void_p), ("state_dst", C.c_void_p), ("list_src", C.c_void_p), ("state_src", C.c_void_p),
                ("cap_list_src", C.c_int64), ("rows", C.c_void_p), ("cols", C.c_void_p), ("edge_index", C.c_void_p),
                ("cap_edges", C.c_int64)]


def _het_steps_case(all_at_once):
    """One hop of the device-side bookkeeping of neighbor_sampling_heterogenous at the C ABI, one node type and one
    relation: tg_het_step_begin -> tg_ns_hop -> tg_het_step_end -> tg_het_hop_end, and (all_at_once, under a filter, packed
    frontier) tg_het_hop_begin_all -> tg_ns_hop_segments -> tg_het_hop_end_all.  The sample list, its filter states and
    `meta` are caller-initialised state: inputs of the case, written with the other inputs, and outputs."""
    n_in, k = 40, 3
    cap_list, cap_e = n_in + n_in * k, n_in * k

    def make(dev):
        d = _graph(dev, "r10")
        words = C.c_int64(0)
        _cabi().check(_cabi().lib.tg_het_meta_words(C.c_int32(1), C.c_int32(1), C.c_int32(1), C.byref(words)))
        meta = torch.zeros(words.value, dtype=torch.int64)
        meta[0] = meta[2] = n_in                            # len | fbeg | fend | ne: len = fend = the number of inputs
        lst, st = torch.zeros(cap_list, dtype=torch.int64), torch.zeros(cap_list, dtype=torch.int64)
        lst[:n_in], st[:n_in] = _rand((n_in,), 0, d["n"], 97, "cpu"), _rand((n_in,), 20, 80, 98, "cpu")
        return _pick(d, "ptrs", "idx", "ts", meta=meta.to(dev), lst=lst.to(dev), st=st.to(dev))

    def call(inp, T):
        cabi = _cabi()
        lib, ptr = cabi.lib, cabi.ptr
        dev = inp["lst"].device
        o = dict(dtype=torch.int64, device=dev)
        meta, lst, st = inp["meta"], inp["lst"], inp["st"]
        trip = T.empty((3, cap_e), **o)
        F, ids, fst = T.empty(n_in, **o), T.empty(n_in, **o), T.empty(n_in, **o)
        stream = cabi.stream_ptr(dev)
        one = C.c_int32(1)
        hout = cabi.TgHopOut()
        if not all_at_once:
            status = T.zeros(1, dtype=torch.int32, device=dev)
            cabi.check(lib.tg_het_step_begin(ptr(lst), None, ptr(meta), one, one, one, C.c_int32(0), C.c_int32(0), C.c_int32(0),
                                             C.c_int32(0), C.c_int64(n_in), ptr(F), None, ptr(ids), stream))
            cnt, off, nbr, ep, par = cabi.ns_hop(_view(inp), F, k, 17, call_id=300, ids=ids, rng_tag=0x17)
            hout.cnt, hout.offsets = cnt.data_ptr(), off.data_ptr()
            hout.neighbors, hout.edge_ptrs, hout.parents = nbr.data_ptr(), ep.data_ptr(), par.data_ptr()
            cabi.check(lib.tg_het_step_end(C.byref(hout), None, C.c_int64(n_in), C.c_int32(k), ptr(meta), one, one, one,
                                           C.c_int32(0), C.c_int32(0), ptr(lst), None, C.c_int64(cap_list), ptr(trip[0]),
                                           ptr(trip[1]), ptr(trip[2]), C.c_int64(cap_e), ptr(status), stream))
            cabi.check(lib.tg_het_hop_end(ptr(meta), one, one, one, stream))
            return lst, meta, trip, status
        g = _view(inp, ts=True)
        ent = (TgHetEntry * 1)()
        e = ent[0]
        e.rel, e.src, e.dst, e.segment, e.begin, e.cap = 0, 0, 0, 0, 0, n_in
        e.list_dst = e.list_src = lst.data_ptr()
        e.state_dst = e.state_src = st.data_ptr()
        e.cap_list_src, e.cap_edges = cap_list, cap_e
        e.rows, e.cols, e.edge_index = trip[0].data_ptr(), trip[1].data_ptr(), trip[2].data_ptr()
        layout = T.empty(2, **o)
        cabi.check(lib.tg_het_hop_begin_all(ent, one, ptr(meta), one, one, one, C.c_int64(n_in), ptr(F), ptr(fst), ptr(ids),
                                            ptr(layout), stream))
        cnt, off, nbr, ep, par, st_out, status = cabi.ns_hop_segments(
            [(g, 0, k, 0x17)], F, fst, 17, filter_mode=cabi.FILTER_STATIC, window=(10, 60), call_id=300, ids=ids, layout=layout)
        hout.cnt, hout.offsets = cnt.data_ptr(), off.data_ptr()
        hout.neighbors, hout.edge_ptrs, hout.parents = nbr.data_ptr(), ep.data_ptr(), par.data_ptr()
        cabi.check(lib.tg_het_hop_end_all(ent, one, C.byref(hout), ptr(st_out), C.c_int64(n_in), C.c_int64(cap_e), ptr(layout),
                                          ptr(meta), one, one, one, C.c_int32(0), one, ptr(status), stream))
        return lst, st, meta, trip, status, layout
    if all_at_once:
        return Case("het_steps[all at once]", ["tg_het_hop_begin_all", "tg_ns_hop_segments", "tg_het_hop_end_all"], ASYNC, make,
                    call, vary=["lst"])
    return Case("het_steps[per relation]", ["tg_het_step_begin", "tg_ns_hop", "tg_het_step_end", "tg_het_hop_end"], ASYNC, make,
                call, vary=["lst"])


# ------------------------------------------------------------------------------------------------ the tg_part_* protocol
def _part_case(world, packed=None, slots=None, filtered=False):
    """world 1: PartitionedSampler (tg_part_sample_ws on the owner side); world 3: the all-to-alls emulated in one process
    (tests/helpers_part.py).  Both read the split sizes back every hop."""
    nb, Bp, fan = 3, 50, [4, 3]

    def make(dev):
        d = _graph(dev, "r10")
        return _pick(d, "ptrs", "idx", "ts", seeds=_rand((nb, Bp), 0, d["n"], 91, dev), st=_rand((nb, Bp), 20, 80, 92, dev))

    def call(inp, T):
        import helpers_part
        from tch_geometric import partitioned
        cabi = _cabi()
        kw = dict(filter_mode=cabi.FILTER_STATIC, window=(10, 60), seeds_state=inp["st"]) if filtered else {}
        ts = inp["ts"] if filtered else None
        shards = [partitioned.CscShard.from_full(inp["ptrs"], inp["idx"], r, world, timestamps=ts) for r in range(world)]
        if world == 1:
            out = partitioned.ns_homo_partitioned_device(shards[0], inp["seeds"], fan, 17, 300, packed_replies=packed,
                                                         slot_replies=slots, **kw)
        else:
            out, _ = helpers_part.emulated_world_sample(cabi, shards, inp["seeds"], fan, 17, 300, packed=bool(packed),
                                                        slots=bool(slots), **kw)
        return _homo_outputs(out)
    names = ["tg_part_begin", "tg_part_requests"]
    if filtered:
        names += ["tg_part_unpack", "tg_part_pack", "tg_part_emit", "tg_ns_hop_scan"]
    elif slots or (world == 1 and slots is None):
        names += ["tg_part_sample_slots", "tg_part_emit_slots"]
    else:
        names += ["tg_part_count", "tg_part_sample_ws" if world == 1 else "tg_part_sample", "tg_part_emit"]
    label = "part[world=%d,slots=%s,packed=%s%s]" % (world, slots, packed, ",filtered" if filtered else "")
    return Case(label, names, READS_BACK, make, call, vary=["seeds"], modules=("helpers_part", "tch_geometric.partitioned"))


# ------------------------------------------------------------------------------------------------ the operator surface
def _surface_case(kind):
    """One call of the Python operator (host/python_module*.cpp): C++ allocates through ATen and reads sizes back."""
    def make(dev):
        g = "hub" if kind == "hgt[library scan]" else "r10"
        d = _graph(dev, g)
        return _pick(d, "ptrs", "idx", "rptrs", "ridx", "ts", "w", "row", "col", a=_rand((64,), 0, d["n"], 95, dev),
                     st=_rand((64,), 20, 80, 96, dev))

    def call(inp, T):
        import tch_geometric as tg
        tg.set_rng_state(77, 5)
        P, I, a = inp["ptrs"], inp["idx"], inp["a"]
        n = P.numel() - 1
        et = [("a", "to", "a")]
        k = "a__to__a"
        if kind == "homo":
            return tg.neighbor_sampling_homogenous(P, I, a, [5, 3])[:4]
        if kind == "homo[filtered]":
            flt = (tg.TemporalEdgeFilter((10, 60), inp["ts"], False, tg.TEMPORAL_SAMPLE_STATIC), inp["st"])
            return tg.neighbor_sampling_homogenous(P, I, a, [5, 3], None, flt)[:4]
        if kind == "homo[weighted]":
            return tg.neighbor_sampling_homogenous(P, I, a, [5, 3], tg.WeightedEdgeSampler(inp["w"]))[:4]
        if kind in ("hetero", "hetero[filtered]", "hetero[flat steps]"):
            flt = None
            if kind == "hetero[filtered]":
                flt = (tg.TemporalEdgeFilter((10, 60), {k: inp["ts"]}, False, tg.TEMPORAL_SAMPLE_STATIC), {"a": inp["st"]})
            fan = [300, 2] if kind == "hetero[flat steps]" else [5, 3]
            s, r, c, e, _ = tg.neighbor_sampling_heterogenous(["a"], et, {k: P}, {k: I}, {"a": a}, {k: fan}, 2, None, flt)
            return s["a"], r[k], c[k], e[k]
        if kind.startswith("hgt"):
            q = [21000] if kind == "hgt[library scan]" else [20, 10]
            s, t, r, c, e = tg.hgt_sampling(["a"], et, {k: P}, {k: I}, None, {"a": a}, None, {"a": q}, len(q))
            return s["a"], t["a"], r[k], c[k], e[k]
        if kind == "budget":
            s, t, r, c, e = tg.budget_sampling(["a"], et, {k: P}, {k: I}, None, {"a": a}, None, {"a": [5, 3]}, 2, None, False, False)
            return s["a"], t["a"], r[k], c[k], e[k]
        if kind == "negative":
            return tg.negative_sample_neighbors_homogenous(inp["rptrs"], inp["ridx"], (n, n), a, 3, 4)[:3]
        if kind == "random_walk":
            return (tg.random_walk(inp["rptrs"], inp["ridx"], a, 10, 0.5, 2.0),)
        return tg.to_csc(torch.stack([inp["row"], inp["col"]]), n)
    names = {"homo": ["tch_geometric.neighbor_sampling_homogenous"], "homo[filtered]": ["tch_geometric.neighbor_sampling_homogenous"],
             "homo[weighted]": ["tch_geometric.neighbor_sampling_homogenous"],
             "hetero": ["tch_geometric.neighbor_sampling_heterogenous"],
             "hetero[filtered]": ["tch_geometric.neighbor_sampling_heterogenous", "tg_het_hop_begin_all", "tg_het_hop_end_all"],
             "hetero[flat steps]": ["tch_geometric.neighbor_sampling_heterogenous", "tg_het_step_begin", "tg_het_step_end",
                                    "tg_het_hop_end"],
             "hgt": ["tch_geometric.hgt_sampling"], "hgt[library scan]": ["tch_geometric.hgt_sampling"],
             "budget": ["tch_geometric.budget_sampling"], "negative": ["tch_geometric.negative_sampling"],
             "random_walk": ["tch_geometric.random_walk"], "to_csc": ["tch_geometric.to_csc"]}[kind]
    vary = ["row"] if kind == "to_csc" else ["a"]
    return Case("surface:%s" % kind, names, READS_BACK, make, call, vary=vary, own_buffers=False)


CASES = ([_hop_case(m, k) for m, k in ((700, 8), (700, 20), (700, 100), (700, 200), (16385, 8))] +
         [_filtered_hop_case(kind) for kind in ("scan", "weighted", "weighted_groups", "segments", "segments_weighted", "recent",
                                                "recent_filtered", "labor", "labor_filtered")] +
         [_homo_fused_case(k) for k in (5, 20, 40)] +
         [_homo_flat_case(kind) for kind in ("plain", "filtered", "weighted", "recent", "labor")] +
         [_homo_windowed_case(*f) for f in WINDOWED_FORMS] +
         [_walk_case("p=q=1", 1.0, 1.0), _walk_case("p!=q", 0.5, 2.0), _walk_case("p!=q,edge_set", 0.5, 2.0, with_set=True)] +
         [_edge_set_case(), _tempo_walk_case(False), _tempo_walk_case(True)] +
         [_ingest_case(True), _ingest_case(False)] + _plumbing_cases() +
         [_compact_case()] + [_unique_case(g, f) for g in (False, True) for f in (1, 2)] +
         [_induced_case(False), _induced_case(True), _full_case(), _cluster_case()] +
         [_hetero_batched_case(), _typed_unique_case(1), _typed_unique_case(2)] +
         [_batched_typed_case(k) for k in ("hgt", "budget", "neg")] + [_budget_layer_case()] +
         [_single_typed_case("hgt"), _single_typed_case("hgt", "hub", 21000), _single_typed_case("budget"),
          _single_typed_case("neg"), _het_steps_case(False), _het_steps_case(True)] +
         [_skipgram_case("rw", 1), _skipgram_case("rw", 3), _skipgram_case("mp", 1), _skipgram_case("mp", 3),
          _skipgram_case("tempo", 0), _pinsage_case()] +
         [_link_case(t, e) for t in (False, True) for e in (False, True)] +
         [_saint_case(k, f) for k in ("rw", "node", "edge") for f in (1, 2)] + [_saint_coverage_case(), _saint_norm_case()] +
         [_part_case(1), _part_case(1, packed=False, slots=False), _part_case(1, slots=False), _part_case(1, filtered=True),
          _part_case(3, packed=False), _part_case(3, packed=True), _part_case(3, slots=True), _part_case(3, filtered=True)] +
         [_surface_case(k) for k in ("homo", "homo[filtered]", "homo[weighted]", "hetero", "hetero[filtered]",
                                     "hetero[flat steps]", "hgt", "hgt[library scan]", "budget", "negative", "random_walk",
                                     "to_csc")])

# no case, with the reason (test_stream_contract_cpu.py reads this).  The pure queries -- *_workspace_bytes, *_capacity, *_form,
# *_pipeline, the tg_ns_win_* getters and setters -- take no stream and launch nothing: nothing to order.
EXEMPT = {
    "tg_ns_win_stage_times": "documents its wait: it synchronises the events of the last timed launch",
    "ns_win_stage_times": "documents its wait (tg_ns_win_stage_times)",
    "tg_probe_random_gather": "microbenchmark probe, not part of the sampling path",
    "tg_probe_ns_sol": "microbenchmark probe, not part of the sampling path",
    "probe_random_gather": "microbenchmark wrapper",
    "probe_ns_sol": "microbenchmark wrapper",
}


# ------------------------------------------------------------------------------------------------ the detector itself
@pytest.fixture(scope="module", autouse=True)
def _report_enqueue_times():
    yield
    if hs.enqueue_ms:
        slowest = max(hs.enqueue_ms, key=hs.enqueue_ms.get)
        print("\nslowest host-side enqueue of a case: %.3f ms (%s); lag %.0f ms" % (hs.enqueue_ms[slowest], slowest, hs.LAG_MS))


def _fake(bug):
    """an "entry point" made of torch ops: b = a * 3; c = b + 1"""
    def make(dev):
        return dict(a=_rand((1 << 16,), 1, 1000, 1, dev))

    def call(inp, T):
        a = inp["a"]
        b = T.empty(a.numel(), dtype=torch.int64, device=a.device)
        c = T.empty(a.numel(), dtype=torch.int64, device=a.device)
        if bug == "first_op_on_default_stream":
            with torch.cuda.stream(torch.cuda.default_stream()):
                torch.mul(a, 3, out=b)
        else:
            torch.mul(a, 3, out=b)
        if bug == "last_op_on_default_stream":
            with torch.cuda.stream(torch.cuda.default_stream()):
                torch.add(b, 1, out=c)
        else:
            torch.add(b, 1, out=c)
        if bug == "synchronises":
            torch.cuda.current_stream().synchronize()
        return (c,)
    return Case("fake[%s]" % bug, [], ASYNC, make, call, vary=["a"])


def test_detector_passes_a_stream_ordered_fake():
    r = hs.run_lagging(_fake(None))
    assert r["returned_early"] and not r["mismatches"]


@pytest.mark.parametrize("bug", ["first_op_on_default_stream", "last_op_on_default_stream"])
def test_detector_catches_an_op_on_the_default_stream(bug):
    r = hs.run_lagging(_fake(bug))
    assert r["mismatches"] == [0] and r["returned_early"]
    with pytest.raises(AssertionError, match="not on the caller's stream"):
        hs.check(_fake(bug))


def test_detector_catches_a_host_wait():
    r = hs.run_lagging(_fake("synchronises"))
    assert not r["returned_early"] and not r["mismatches"]
    with pytest.raises(AssertionError, match="waits on the host"):
        hs.check(_fake("synchronises"))


def test_detector_refuses_a_case_without_power():
    dead = Case("dead", [], ASYNC, lambda dev: dict(a=torch.ones(64, dtype=torch.int64, device=dev)),
                lambda inp, T: (T.zeros(64, dtype=torch.int64, device=inp["a"].device),), vary=["a"])
    with pytest.raises(hs.StreamOrderError, match="no power"):
        hs.run_lagging(dead)
    same = Case("same", [], ASYNC, lambda dev: dict(a=torch.ones(64, dtype=torch.int64, device=dev)),
                lambda inp, T: (inp["a"] + 1,), vary=["a"])
    with pytest.raises(hs.StreamOrderError, match="no power"):
        hs.run_lagging(same)


def test_a_null_stream_launch_overtakes_the_blocked_stream():
    """The premise of every case: tg_ns_rows_fill with stream = NULL runs while `s` is blocked.  If the runtime ordered
    the NULL stream behind torch's streams, a launch on it would be indistinguishable and every case would be vacuous."""
    cabi = _cabi()
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = torch.zeros((3, 500), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ev = hs.block(hs.side_stream())
    cabi.check(cabi.lib.tg_ns_rows_fill(cabi.ptr(rows), C.c_int64(3), C.c_int64(500), C.c_int64(40), C.c_void_p(0)))
    torch.cuda.default_stream().synchronize()
    still_blocked = not ev.query()
    got = rows.cpu()                                        # the null stream again: still no wait for `s`
    still_blocked_after_copy = not ev.query()
    hs.side_stream().synchronize()
    assert torch.equal(got, (40 + torch.arange(500)).expand(3, 500))
    assert still_blocked and still_blocked_after_copy, "a NULL-stream launch waited for the blocked stream: every case is vacuous"


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_stream_order(case):
    r = hs.check(case)
    print("%s: host enqueue %.3f ms, %d outputs" % (case.id, r["host_ms"], r["n_outputs"]))
