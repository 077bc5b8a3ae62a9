"""Batched budget_sampling, host-only queries: tg_budget_batched_workspace_bytes, the per-call capacities the batched form
uses (tg_budget_capacity's) and the argument checks of tg_budget_sample_batched that run before anything is launched.
No GPU: the graph pointers are never read."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cabi():
    if not os.path.exists(os.path.join(ROOT, "tch-geometric_amd", "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tch-geometric_amd"), "-s"])
    from tch_geometric import _cabi
    return _cabi


CFG4_RELS = [(0, 0), (0, 1), (1, 0), (1, 2), (2, 0)]    # A->A, A->B, B->A, B->C, C->A


def _rels(pattern=CFG4_RELS):
    P, I = torch.zeros(11, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)   # tiny host arrays stand in for graphs
    return [(s, d, P, I, None) for s, d in pattern]


def _problem(cabi, n_in=(1024, 0, 0), nn=([15, 10],) * 3, hops=2, n_types=3, pattern=CFG4_RELS):
    return cabi.budget_problem(n_types, _rels(pattern), list(n_in), list(nn), hops)


def _plan(n_in, nn, hops, pattern):
    """tg_budget_capacity restated: per hop, a node of type t may take all of its k picks from any one relation into t."""
    T = len(n_in)
    front, cap_n, cap_e = list(n_in), list(n_in), [0] * len(pattern)
    for h in range(hops):
        fresh = [0] * T
        for t in range(T):
            cells = front[t] * nn[t][h]
            for s in sorted({s for s, d in pattern if d == t}):
                fresh[s] += cells
            for r, (s, d) in enumerate(pattern):
                if d == t:
                    cap_e[r] += cells
        front = fresh
        cap_n = [a + b for a, b in zip(cap_n, fresh)]
    return cap_n, cap_e


def test_symbols_exported(cabi):
    for name in ("tg_budget_batched_workspace_bytes", "tg_budget_sample_batched"):
        assert name in cabi.EXPORTS
        assert hasattr(cabi.lib, name)


@pytest.mark.parametrize("shape", [((1024, 0, 0), ([15, 10],) * 3, 2), ((4, 0, 7), ([20, 15], [0, 3], [3, 0]), 2),
                                   ((60, 60, 60), ([], [], []), 0)])
def test_workspace_linear_in_calls(cabi, shape):
    p = _problem(cabi, *shape)
    stride = cabi.budget_batched_workspace_bytes(p, 1)
    assert stride > 0 and stride % 8 == 0
    single = C.c_int64(0)
    assert cabi.lib.tg_budget_workspace_bytes(C.byref(p), C.byref(single)) == 0
    assert stride == single.value                                       # one call's region is the single call's workspace
    for n in (2, 3, 64, 257, 512, 65535):
        assert cabi.budget_batched_workspace_bytes(p, n) == n * stride  # n regions, no shared part


def test_capacity_is_the_single_calls(cabi):
    """The batched form takes tg_budget_capacity's per-call capacities; at cfg4 (1 024 seeds of A, [15, 10]) that is
    about 0.8 M node and 0.8 M edge words per call, far above a typical call's ~20 K nodes and ~19 K edges."""
    cap_n, cap_e = cabi.budget_capacity(_problem(cabi))
    assert (cap_n, cap_e) == _plan((1024, 0, 0), ([15, 10],) * 3, 2, CFG4_RELS)
    assert cap_n == [323584, 322560, 168960] and cap_e == [168960, 153600, 168960, 153600, 168960]
    n_in, nn = (4, 0, 7), ([20, 15], [0, 3], [3, 0])
    assert cabi.budget_capacity(_problem(cabi, n_in, nn)) == _plan(n_in, nn, 2, CFG4_RELS)
    bb = cabi.BudgetBatched(3, _rels(), [torch.zeros((5, 4), dtype=torch.int64), None, torch.zeros((5, 7), dtype=torch.int64)],
                            list(nn), 2, 5, torch.device("cpu"), pad=3)   # allocation only: nothing is launched
    assert (bb.cap_nodes, bb.cap_edges) == _plan(n_in, nn, 2, CFG4_RELS)
    assert bb.node_pitch == [c + 3 for c in bb.cap_nodes] and bb.edge_pitch == [c + 3 for c in bb.cap_edges]
    assert bb.launch_bytes == bb.workspace_bytes + 8 * 5 * (2 * sum(bb.node_pitch) + 3 * sum(bb.edge_pitch) + 3 + 5)


def _call(cabi, p, n_calls, out, ws=0x100000, ws_bytes=1 << 62):
    rng = cabi.TgRng(1, 0)
    return cabi.lib.tg_budget_sample_batched(C.byref(p) if p is not None else None, C.c_int64(n_calls), C.byref(rng),
                                             C.byref(out) if out is not None else None, C.c_void_p(ws), C.c_int64(ws_bytes),
                                             C.c_void_p(0))


def _out(cabi, p, extra=0, counts=0x200000):
    cap_n, cap_e = cabi.budget_capacity(p)
    T, R = len(cap_n), max(len(cap_e), 1)
    keep = [(C.c_void_p * T)(*[0x300000 + 0x1000 * t for t in range(T)]),
            (C.c_void_p * T)(*[0x400000 + 0x1000 * t for t in range(T)]), (C.c_int64 * T)(*[c + extra for c in cap_n]),
            (C.c_void_p * R)(*[0x500000 + 0x1000 * r for r in range(R)]),
            (C.c_void_p * R)(*[0x600000 + 0x1000 * r for r in range(R)]),
            (C.c_void_p * R)(*[0x700000 + 0x1000 * r for r in range(R)]), (C.c_int64 * R)(*[c + extra for c in cap_e])]
    o = cabi.TgBudgetBatchedOut(*keep, counts)
    o._keep = keep
    return o


def _refused(cabi, rc, what):
    assert rc == 1, what                                                 # TG_ERR_INVALID, before any launch
    msg = cabi.lib.tg_last_error().decode()
    assert "tg_budget" in msg, msg
    return msg


def test_bad_arguments_rejected(cabi):
    p = _problem(cabi)
    out = _out(cabi, p)
    nbytes = C.c_int64(0)
    ws4 = cabi.budget_batched_workspace_bytes(p, 4)
    for n in (0, -1, 65536):
        _refused(cabi, cabi.lib.tg_budget_batched_workspace_bytes(C.byref(p), C.c_int64(n), C.byref(nbytes)), n)
        assert "65535" in _refused(cabi, _call(cabi, p, n, out), n)
    _refused(cabi, cabi.lib.tg_budget_batched_workspace_bytes(None, C.c_int64(1), C.byref(nbytes)), "null problem")
    _refused(cabi, cabi.lib.tg_budget_batched_workspace_bytes(C.byref(p), C.c_int64(1), None), "null output")
    _refused(cabi, _call(cabi, None, 4, out), "null problem")
    _refused(cabi, _call(cabi, p, 4, None), "null outputs")
    _refused(cabi, _call(cabi, p, 4, out, ws=0), "null workspace")
    _refused(cabi, _call(cabi, p, 4, out, ws=0x100004), "workspace not 8-byte aligned")
    assert "workspace too small" in _refused(cabi, _call(cabi, p, 4, out, ws_bytes=ws4 - 1), "workspace one byte short")
    _refused(cabi, _call(cabi, p, 4, _out(cabi, p, counts=0)), "null counts")
    _refused(cabi, _call(cabi, p, 4, _out(cabi, p, counts=0x200004)), "counts not 8-byte aligned")
    for i in range(3 + 5):                                               # every pitch one short, one at a time
        o = _out(cabi, p)
        arr = o._keep[2] if i < 3 else o._keep[6]
        arr[i % 3 if i < 3 else i - 3] -= 1
        assert "too small" in _refused(cabi, _call(cabi, p, 4, o), ("pitch", i))
    for field in ("samples", "sample_ts", "rows", "cols", "edge_index"):  # a whole array missing
        o = _out(cabi, p)
        setattr(o, field, None)
        _refused(cabi, _call(cabi, p, 4, o), field)
    for arr, i in ((0, 1), (1, 0), (3, 4), (4, 2), (5, 0)):              # one null slab
        o = _out(cabi, p)
        o._keep[arr][i] = None
        assert "null" in _refused(cabi, _call(cabi, p, 4, o), ("slab", arr, i))
    o = _out(cabi, p)
    o._keep[3][1] = 0x500004                                             # a misaligned slab
    assert "aligned" in _refused(cabi, _call(cabi, p, 4, o), "misaligned slab")
    p_in = _problem(cabi)
    p_in.inputs = (C.c_void_p * 3)()                                     # n_inputs > 0 without a pointer
    _refused(cabi, _call(cabi, p_in, 4, out), "inputs")
    assert cabi.budget_batched_workspace_bytes(p, 4) == ws4              # the checks leave the problem as it was


def test_fused_limits_refused_with_their_names(cabi):
    """9 node types, 17 relations, num_neighbors 65: refused by all three functions with a message naming the limit."""
    cases = [(dict(n_in=(1,) * 9, nn=([1],) * 9, hops=1, n_types=9, pattern=[(0, 0)]), "<= 8"),
             (dict(n_in=(1, 0, 0), nn=([1],) * 3, hops=1, pattern=[(0, 0)] * 17), "<= 16"),
             (dict(n_in=(1, 0, 0), nn=([65], [1], [1]), hops=1), r"\[0, 64\]")]
    for kw, limit in cases:
        p = _problem(cabi, **kw)
        with pytest.raises(cabi.TchGeoError, match=limit) as e:
            cabi.budget_batched_workspace_bytes(p, 1)
        assert "error 1:" in str(e.value)
        with pytest.raises(cabi.TchGeoError, match=limit):
            cabi.budget_capacity(p)
        T, R = p.n_types, max(p.n_rels, 1)
        slabs = lambda n, at: (C.c_void_p * n)(*[at + 0x1000 * i for i in range(n)])
        big = lambda n: (C.c_int64 * n)(*[1 << 30] * n)
        o = cabi.TgBudgetBatchedOut(slabs(T, 0x300000), slabs(T, 0x400000), big(T), slabs(R, 0x500000),
                                    slabs(R, 0x600000), slabs(R, 0x700000), big(R), 0x200000)
        o._keep = (o.samples, o.sample_ts, o.pitch_nodes, o.rows, o.cols, o.edge_index, o.pitch_edges)
        assert _call(cabi, p, 2, o) == 1
        assert re.search(limit, cabi.lib.tg_last_error().decode())
    ok = _problem(cabi, (1, 0, 0), ([64], [64], [64]), 1)                # the limits themselves pass
    assert cabi.budget_batched_workspace_bytes(ok, 1) > 0
