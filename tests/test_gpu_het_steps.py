"""One hop of the hetero filtered / weighted driver at the C ABI with the frontier layout chosen by hand:
tg_het_hop_begin_all -> tg_ns_hop_segments -> tg_het_hop_end_all on one small problem, once with a device-side layout
(packed frontier) and once without (padded frontier).  Both must leave the same lists, states, edge lists, lengths, layer
offsets and next-hop frontier slices, write nothing past the lengths they record, and equal one hop of the oracle --
whatever thresholds the Python operator's driver uses to choose between the two."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
from helpers_hetero import FILTER_DYNAMIC, FILTER_RELATIVE, FILTER_STATIC, rel_key

FILTER_NONE = orc.FILTER_NONE

pytestmark = pytest.mark.gpu

SENTINEL = -7777
SLACK = 16                                                   # words behind every capacity that must stay untouched
WINDOW = (0, 5)
NODE_TYPES = ["a", "b", "c", "d"]
COUNTS = {"a": 40, "b": 30, "c": 20, "d": 10}
# in edge_types order: a segment, an entry without a frontier ("d" has no inputs), two more segments
EDGE_TYPES = [("b", "x", "a"), ("a", "v", "d"), ("a", "z", "b"), ("c", "self", "c")]
FANOUT = {"b__x__a": 3, "a__v__d": 2, "a__z__b": 70, "c__self__c": 1}
INPUTS = {"a": [5, 1, 17, 5, 39], "b": [0, 29, 7], "c": [3, 3]}
CAPS = {"a": 9, "b": 6, "c": 4}                              # worst-case frontier sizes: all above the real ones, unequal


class TgHetEntry(C.Structure):
    _fields_ = [("rel", C.c_int32), ("src", C.c_int32), ("dst", C.c_int32), ("segment", C.c_int32),
                ("begin", C.c_int64), ("cap", C.c_int64),
                ("list_dst", C.c_void_p), ("state_dst", C.c_void_p), ("list_src", C.c_void_p), ("state_src", C.c_void_p),
                ("cap_list_src", C.c_int64), ("rows", C.c_void_p), ("cols", C.c_void_p), ("edge_index", C.c_void_p),
                ("cap_edges", C.c_int64)]


def _problem():
    rs = np.random.default_rng(4242)
    P, I, TS, W = {}, {}, {}, {}
    for et in EDGE_TYPES:
        k = rel_key(et)
        deg = rs.poisson(3.0, COUNTS[et[2]])
        if k == "a__z__b":
            deg[[0, 29]] = [69, 400]                          # on both sides of the fan-out of 70, also under a filter
        P[k] = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        I[k] = rs.integers(0, COUNTS[et[0]], int(P[k][-1])).astype(np.int64)
        TS[k] = rs.integers(0, 12, len(I[k]))
        W[k] = rs.uniform(0.1, 4.0, len(I[k]))
    inputs = {t: np.asarray(v, dtype=np.int64) for t, v in INPUTS.items()}
    states = {t: rs.integers(0, 12, len(v)) for t, v in inputs.items()}
    states["b"][1] = 6                                       # the long column keeps half its edges in either direction
    return P, I, TS, W, inputs, states


def _one_hop(cabi, prob, weighted, mode, forward, packed, seed, call_id):
    """-> everything the three calls left on the device, as NumPy"""
    P, I, TS, W, inputs, states = prob
    dev = torch.device("cuda:0")
    lib = cabi.lib
    T, R, H = len(NODE_TYPES), len(EDGE_TYPES), 1
    filtered = mode != FILTER_NONE
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    full = lambda n: torch.full((n + SLACK,), SENTINEL, dtype=torch.int64, device=dev)
    tix = {name: i for i, name in enumerate(NODE_TYPES)}
    rels = [rel_key(et) for et in EDGE_TYPES]
    n_in = {name: len(inputs.get(name, ())) for name in NODE_TYPES}
    cap_f = [CAPS.get(et[2], 0) for et in EDGE_TYPES]
    cap_e = [max(cf * FANOUT[k], 1) for cf, k in zip(cap_f, rels)]
    cap_list = {name: n_in[name] + sum(ce for ce, et, cf in zip(cap_e, EDGE_TYPES, cap_f) if et[0] == name and cf)
                for name in NODE_TYPES}
    lists = {name: full(cap_list[name]) for name in NODE_TYPES}
    st_lists = {name: full(cap_list[name]) for name in NODE_TYPES}
    for name, v in inputs.items():
        lists[name][:len(v)] = t(v)
        st_lists[name][:len(v)] = t(states[name])
    RW, CL, EI = ([full(ce) for ce in cap_e] for _ in range(3))
    words = C.c_int64(0)
    cabi.check(lib.tg_het_meta_words(C.c_int32(T), C.c_int32(R), C.c_int32(H), C.byref(words)))
    meta_h = np.full(words.value, SENTINEL, dtype=np.int64)
    meta_h[:3 * T + R] = 0                                    # len | fbeg | fend | ne
    for name, n in n_in.items():
        meta_h[tix[name]] = meta_h[2 * T + tix[name]] = n     # len = fend = number of inputs
    meta = torch.cat([t(meta_h), full(0)])
    graphs = [cabi.graph_view(t(P[k]), t(I[k]), t(W[k]) if weighted else None, t(TS[k]) if filtered else None) for k in rels]
    ent = (TgHetEntry * R)()
    segs, m_total, o_total = [], 0, 0
    for r, et in enumerate(EDGE_TYPES):
        e = ent[r]
        e.rel, e.src, e.dst, e.segment = r, tix[et[0]], tix[et[2]], -1
        e.list_dst, e.list_src = lists[et[2]].data_ptr(), lists[et[0]].data_ptr()
        if filtered:
            e.state_dst, e.state_src = st_lists[et[2]].data_ptr(), st_lists[et[0]].data_ptr()
        e.cap_list_src = cap_list[et[0]]
        e.rows, e.cols, e.edge_index, e.cap_edges = RW[r].data_ptr(), CL[r].data_ptr(), EI[r].data_ptr(), cap_e[r]
        if cap_f[r]:
            e.segment, e.begin, e.cap = len(segs), m_total, cap_f[r]
            segs.append((graphs[r], m_total, FANOUT[rels[r]], orc.TAG_NS_HETERO | (r << 8)))
            m_total += cap_f[r]
            o_total += cap_f[r] * FANOUT[rels[r]]
    assert [e.segment for e in ent] == [0, -1, 1, 2] and m_total == sum(CAPS.values())
    F, ids, fst = full(m_total), full(m_total), full(m_total)
    layout = full(len(segs) + 1) if packed else None
    stream = cabi.stream_ptr(dev)
    cabi.check(lib.tg_het_hop_begin_all(ent, C.c_int32(R), cabi.ptr(meta), C.c_int32(T), C.c_int32(R), C.c_int32(H),
                                        C.c_int64(m_total), cabi.ptr(F), cabi.ptr(fst) if filtered else None, cabi.ptr(ids),
                                        cabi.ptr(layout), stream))
    cnt, off, nbr, ep, par, st_out, status = cabi.ns_hop_segments(
        segs, F[:m_total], fst[:m_total] if filtered else None, seed, filter_mode=mode, window=WINDOW, forward=forward,
        call_id=call_id, sampler=orc.SAMPLER_WEIGHTED if weighted else orc.SAMPLER_UNIFORM, ids=ids[:m_total], layout=layout)
    hout = cabi.TgHopOut()
    hout.cnt, hout.offsets = cnt.data_ptr(), off.data_ptr()
    hout.neighbors, hout.edge_ptrs, hout.parents = nbr.data_ptr(), ep.data_ptr(), par.data_ptr()
    cabi.check(lib.tg_het_hop_end_all(ent, C.c_int32(R), C.byref(hout), cabi.ptr(st_out) if filtered else None,
                                      C.c_int64(m_total), C.c_int64(o_total), cabi.ptr(layout), cabi.ptr(meta), C.c_int32(T),
                                      C.c_int32(R), C.c_int32(H), C.c_int32(0), C.c_int32(1), cabi.ptr(status), stream))
    torch.cuda.synchronize()
    h = lambda x: x.cpu().numpy()
    return dict(lists={k: h(v) for k, v in lists.items()}, states={k: h(v) for k, v in st_lists.items()},
                rows=[h(x) for x in RW], cols=[h(x) for x in CL], eidx=[h(x) for x in EI], meta=h(meta), F=h(F), ids=h(ids),
                fst=h(fst), layout=None if layout is None else h(layout), status=int(status), m_total=m_total,
                cap_list=cap_list, cap_e=cap_e, n_in=n_in)


@pytest.mark.parametrize("variant", ["static", "relative-backward", "dynamic-forward", "weighted", "weighted+dynamic-backward"])
def test_packed_and_padded_hop_leave_the_same_state_and_equal_the_oracle(variant):
    from tch_geometric import _cabi as cabi
    weighted, mode, forward = {"static": (False, FILTER_STATIC, True), "relative-backward": (False, FILTER_RELATIVE, False),
                               "dynamic-forward": (False, FILTER_DYNAMIC, True), "weighted": (True, FILTER_NONE, False),
                               "weighted+dynamic-backward": (True, FILTER_DYNAMIC, False)}[variant]
    filtered = mode != FILTER_NONE
    prob = _problem()
    P, I, TS, W, inputs, states = prob
    T, R = len(NODE_TYPES), len(EDGE_TYPES)
    rels = [rel_key(et) for et in EDGE_TYPES]
    seed, call_id = 31, 4
    packed = _one_hop(cabi, prob, weighted, mode, forward, True, seed, call_id)
    padded = _one_hop(cabi, prob, weighted, mode, forward, False, seed, call_id)
    kw = {}
    if weighted:
        kw.update(sampler=orc.SAMPLER_WEIGHTED, weights=W)
    if filtered:
        kw.update(filter_mode=mode, forward=forward, window=WINDOW, timestamps=TS, inputs_state=states)
    nn = {k: [FANOUT[k]] for k in rels}
    o = orc.ns_hetero(NODE_TYPES, EDGE_TYPES, P, I, inputs, nn, 1, orc.rng_philox(seed, call_id), **kw)
    assert len(o[3]["a__z__b"]) > 70 and len(o[3]["b__x__a"]) > 0                  # the problem is not trivial

    for run in (packed, padded):
        assert run["status"] == 0
        meta = run["meta"]
        ln, fbeg, fend, ne = meta[:T], meta[T:2 * T], meta[2 * T:3 * T], meta[3 * T:3 * T + R]
        lo = meta[3 * T + R:3 * T + R + 3 * R].reshape(R, 3)
        assert np.all(meta[-SLACK:] == SENTINEL)
        for i, name in enumerate(NODE_TYPES):
            # lengths and the next hop's frontier slice: what this hop appended
            assert ln[i] == len(o[0].get(name, ())) and fbeg[i] == run["n_in"][name] and fend[i] == ln[i], name
            assert np.array_equal(run["lists"][name][:ln[i]], o[0][name]), name
            assert np.all(run["lists"][name][ln[i]:] == SENTINEL), name
            if filtered:
                assert np.array_equal(run["states"][name][:run["n_in"][name]], states.get(name, [])), name
                assert np.all(run["states"][name][:ln[i]] != SENTINEL), name
            assert np.all(run["states"][name][ln[i] if filtered else run["n_in"][name]:] == SENTINEL), name
        for r, k in enumerate(rels):
            assert ne[r] == len(o[3][k]), k
            assert tuple(lo[r]) == tuple(o[4][k][0]), k
            for got, want in ((run["rows"][r], o[1][k]), (run["cols"][r], o[2][k]), (run["eidx"][r], o[3][k])):
                assert np.array_equal(got[:ne[r]], want), k
                assert np.all(got[ne[r]:] == SENTINEL), k
    # the frontier itself: real entries back to back, or every segment padded to its capacity with -1
    real = [len(inputs[et[2]]) for et in EDGE_TYPES if et[2] in inputs]
    caps = [CAPS[et[2]] for et in EDGE_TYPES if et[2] in inputs]
    assert list(packed["layout"][:len(real) + 1]) == list(np.concatenate([[0], np.cumsum(real)]))
    assert np.all(packed["layout"][len(real) + 1:] == SENTINEL)
    want_packed = np.concatenate([inputs[et[2]] for et in EDGE_TYPES if et[2] in inputs])
    want_padded = np.concatenate([np.concatenate([inputs[et[2]], np.full(CAPS[et[2]] - len(inputs[et[2]]), -1)])
                                  for et in EDGE_TYPES if et[2] in inputs])
    assert np.array_equal(packed["F"][:sum(real)], want_packed) and np.all(packed["F"][sum(real):] == SENTINEL)
    assert np.array_equal(padded["F"][:sum(caps)], want_padded) and np.all(padded["F"][sum(caps):] == SENTINEL)
    assert np.all(packed["ids"][sum(real):] == SENTINEL) and np.all(padded["ids"][sum(caps):] == SENTINEL)
    if not filtered:
        assert np.all(packed["fst"] == SENTINEL) and np.all(padded["fst"] == SENTINEL)

    # and the two layouts agree word for word on everything a later hop or the caller reads
    words = 3 * T + R + 3 * R
    assert np.array_equal(packed["meta"][:words], padded["meta"][:words])
    for name in NODE_TYPES:
        assert np.array_equal(packed["lists"][name], padded["lists"][name]), name
        assert np.array_equal(packed["states"][name], padded["states"][name]), name
    for r in range(R):
        for key in ("rows", "cols", "eidx"):
            assert np.array_equal(packed[key][r], padded[key][r]), (key, rels[r])
