"""Batched hgt_sampling, host-only queries: tg_hgt_batched_capacity / tg_hgt_batched_workspace_bytes and the argument
checks of tg_hgt_sample_batched that run before anything is launched.  No GPU: the graph pointers are never read."""
import ctypes as C
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_WORKGROUP_SCAN = 16384      # tchgeo.h TG_HGT_ONE_WORKGROUP_SCAN


@pytest.fixture(scope="module")
def cabi():
    if not os.path.exists(os.path.join(ROOT, "tch-geometric_amd", "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tch-geometric_amd"), "-s"])
    from tch_geometric import _cabi
    return _cabi


def _rels():
    """cfg4's relation pattern over three types: A->A, A->B, B->A, B->C, C->A (tiny host arrays stand in for graphs)."""
    P, I = torch.zeros(11, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)
    return [(0, 0, P, I, None), (0, 1, P, I, None), (1, 0, P, I, None), (1, 2, P, I, None), (2, 0, P, I, None)]


def _problem(cabi, n_in=(1024, -1, -1), ns=([512, 512],) * 3, hops=2):
    return cabi.hgt_problem(3, _rels(), list(n_in), list(ns), hops)


def test_symbols_exported(cabi):
    for name in ("tg_hgt_batched_capacity", "tg_hgt_batched_workspace_bytes", "tg_hgt_sample_batched"):
        assert name in cabi.EXPORTS
        assert hasattr(cabi.lib, name)


@pytest.mark.parametrize("shape", [((1024, -1, -1), ([512, 512],) * 3, 2), ((4, 0, 7), ([20, 15], None, [3, 0]), 2),
                                   ((60, 60, 60), ([], [], []), 0)])
def test_workspace_linear_in_calls(cabi, shape):
    p = _problem(cabi, *shape)
    stride = cabi.hgt_batched_workspace_bytes(p, 1)
    assert stride > 0 and stride % 256 == 0
    for n in (2, 3, 64, 257, 512, 65535):
        assert cabi.hgt_batched_workspace_bytes(p, n) == n * stride     # n regions, no shared part


def test_capacity_equals_single_call_binding(cabi):
    """python_module_hgt.cpp sizes a call's buffers as max(n_inputs, 0) + the type's quotas and 50 x that of the
    relation's destination type (at least one node)."""
    n_in, ns = (4, 0, -1), ([20, 15], None, [3, 9])
    cap_n, cap_e = cabi.hgt_batched_capacity(_problem(cabi, n_in, ns))
    want_n = [max(n_in[t], 0) + sum(max(k, 0) for k in (ns[t] or [])) for t in range(3)]
    assert cap_n == want_n
    assert cap_e == [50 * max(want_n[d], 1) for (_, d, *_) in _rels()]


def test_scan_limit_refused(cabi):
    """The batched form keeps every scan in one workgroup per call: a type with more nodes than that is refused with
    TG_ERR_INVALID and a message naming the limit (the single call falls back to library scans instead)."""
    p = _problem(cabi, (ONE_WORKGROUP_SCAN + 1, -1, -1), ([0], [0], [0]), 1)
    with pytest.raises(cabi.TchGeoError, match="one-workgroup scan limit") as e:
        cabi.hgt_batched_workspace_bytes(p, 1)
    assert "error 1:" in str(e.value)
    with pytest.raises(cabi.TchGeoError, match="one-workgroup scan limit"):
        cabi.hgt_batched_capacity(p)
    ok = _problem(cabi, (ONE_WORKGROUP_SCAN, -1, -1), ([0], [0], [0]), 1)
    assert cabi.hgt_batched_workspace_bytes(ok, 1) > 0


def _call(cabi, p, n_calls, out, ws=0x100000, ws_bytes=1 << 62):
    rng = cabi.TgRng(1, 0)
    return cabi.lib.tg_hgt_sample_batched(C.byref(p) if p is not None else None, C.c_int64(n_calls), C.byref(rng),
                                          C.byref(out) if out is not None else None, C.c_void_p(ws), C.c_int64(ws_bytes),
                                          C.c_void_p(0))


def _out(cabi, p, extra=0, counts=0x200000):
    cap_n, cap_e = cabi.hgt_batched_capacity(p)
    T, R = len(cap_n), len(cap_e)
    keep = [(C.c_void_p * T)(*[0x300000 + 0x1000 * t for t in range(T)]),
            (C.c_void_p * T)(*[0x400000 + 0x1000 * t for t in range(T)]), (C.c_int64 * T)(*[c + extra for c in cap_n]),
            (C.c_void_p * R)(*[0x500000 + 0x1000 * r for r in range(R)]),
            (C.c_void_p * R)(*[0x600000 + 0x1000 * r for r in range(R)]),
            (C.c_void_p * R)(*[0x700000 + 0x1000 * r for r in range(R)]), (C.c_int64 * R)(*[c + extra for c in cap_e])]
    o = cabi.TgHgtBatchedOut(*keep, counts)
    o._keep = keep
    return o


def test_bad_arguments_rejected(cabi):
    p = _problem(cabi)
    out = _out(cabi, p)
    nbytes = C.c_int64(0)
    for n in (0, -1, 65536):
        assert cabi.lib.tg_hgt_batched_workspace_bytes(C.byref(p), C.c_int64(n), C.byref(nbytes)) == 1
        assert _call(cabi, p, n, out) == 1
    assert cabi.lib.tg_hgt_batched_workspace_bytes(None, C.c_int64(1), C.byref(nbytes)) == 1
    assert cabi.lib.tg_hgt_batched_workspace_bytes(C.byref(p), C.c_int64(1), None) == 1
    assert _call(cabi, None, 4, out) == 1                                              # null problem
    assert _call(cabi, p, 4, None) == 1                                                # null outputs
    assert _call(cabi, p, 4, out, ws=0) == 1                                           # null workspace
    assert _call(cabi, p, 4, out, ws=0x100004) == 1                                    # workspace not 8-byte aligned
    assert _call(cabi, p, 4, out, ws_bytes=cabi.hgt_batched_workspace_bytes(p, 4) - 8) == 1   # workspace too small
    assert _call(cabi, p, 4, _out(cabi, p, counts=0)) == 1                             # null counts
    assert _call(cabi, p, 4, _out(cabi, p, extra=-1)) == 1                             # pitches below the capacity
    for field in ("samples", "rows", "edge_index"):
        o = _out(cabi, p)
        setattr(o, field, None)
        assert _call(cabi, p, 4, o) == 1, field
    p_in = _problem(cabi)
    p_in.inputs = (C.c_void_p * 3)()                                                   # n_inputs > 0 without a pointer
    assert _call(cabi, p_in, 4, out) == 1
    assert "tg_hgt_sample_batched" in cabi.lib.tg_last_error().decode()
