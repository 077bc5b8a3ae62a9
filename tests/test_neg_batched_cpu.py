"""Batched negative sampling, host-only queries: tg_neg_batched_capacity, tg_neg_batched_form with a stated LDS limit,
tg_neg_batched_workspace_bytes and the argument checks of tg_neg_sample_batched that run before anything is launched.
No GPU: the graph pointers are never read and every device pointer handed over is null."""
import ctypes as C
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = 160 * 1024                                        # a gfx950 workgroup's LDS


@pytest.fixture(scope="module")
def cabi():
    if not os.path.exists(os.path.join(ROOT, "tch-geometric_amd", "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tch-geometric_amd"), "-s"])
    from tch_geometric import _cabi
    return _cabi


CFG4_RELS = [(0, 0), (0, 1), (1, 0), (1, 2), (2, 0)]    # A->A, A->B, B->A, B->C, C->A


def _homo(cabi, n_in=1024, num_neg=5, tries=5, node_count=1 << 24):
    P, I = torch.zeros(11, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)   # tiny host arrays stand in for graphs
    return cabi.neg_problem(1, [(0, 0, P, I, node_count)], [n_in], num_neg, tries, homogeneous=True)


def _hetero(cabi, n_in=(1024, -1, -1), num_neg=5, tries=5, pattern=CFG4_RELS, n_types=3, inbound=False):
    P, I = torch.zeros(11, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)
    return cabi.neg_problem(n_types, [(s, d, P, I, 1000) for s, d in pattern], list(n_in), num_neg, tries, inbound=inbound)


def test_symbols_exported(cabi):
    for name in ("tg_neg_batched_capacity", "tg_neg_batched_form", "tg_neg_batched_workspace_bytes", "tg_neg_sample_batched"):
        assert name in cabi.EXPORTS
        assert hasattr(cabi.lib, name)


@pytest.mark.parametrize("case", ["homogeneous", "cfg4 one input type", "a type without an inputs entry"])
def test_capacities_are_the_documented_formulas(cabi, case):
    """tg_neg_out's capacities per call: max(n_inputs[t], 0) + total items for a type, n_inputs[src] * num_neg for a relation."""
    if case == "homogeneous":
        n_in, num_neg, pattern, p = [1024], 5, [(0, 0)], _homo(cabi, 1024, 5)
    elif case == "cfg4 one input type":
        n_in, num_neg, pattern = [1024, 0, 0], 5, CFG4_RELS
        p = _hetero(cabi, n_in, num_neg)
    else:
        n_in, num_neg, pattern = [100, -1, 7], 3, CFG4_RELS
        p = _hetero(cabi, n_in, num_neg)
    items = sum(max(n, 0) * num_neg for n in n_in)
    cap_n, cap_e = cabi.neg_batched_capacity(p)
    assert cap_n == [max(n, 0) + items for n in n_in]
    assert cap_e == [max(n_in[s], 0) * num_neg for s, _ in pattern]


def test_workspace_of_the_call_by_call_form_covers_a_single_call(cabi):
    """The call-by-call form runs tg_neg_sample in the first workspace region, so it needs at least that call's workspace.
    tg_neg_workspace_bytes asks the scan library for its temporary storage, which needs a device: where there is none both
    queries report that failure (neither guesses a size), and tests/test_gpu_neg_batched.py repeats the comparison on the
    device."""
    p = _homo(cabi, 65536, 5)                            # past the fused limit on any device
    assert cabi.neg_batched_form(p, LDS)[0] == 0
    single, batched = C.c_int64(-1), C.c_int64(-1)
    rc1 = cabi.lib.tg_neg_workspace_bytes(C.byref(p), C.byref(single))
    rc2 = cabi.lib.tg_neg_batched_workspace_bytes(C.byref(p), C.c_int64(3), C.byref(batched))
    if rc1 == 0:
        assert rc2 == 0 and batched.value >= single.value > 0
    else:
        assert rc2 == rc1 and b"device" in cabi.lib.tg_last_error()


def test_form_query_with_a_stated_lds_limit(cabi):
    """With 160 KiB of LDS the two shapes a training loop asks for take the fused kernel; 65 536 inputs x 5 and node ids
    past 32 bits run call by call.  The query touches no device."""
    form, lds = cabi.neg_batched_form(_homo(cabi, 1024, 5), LDS)
    assert form == 1 and 0 < lds <= LDS
    # u32 candidate + u32 id + u8 relation per item, 8 192 slots of (u32 key, u32 value): about 110 KiB
    assert lds >= 5120 * 9 + 8192 * 8
    form, lds_h = cabi.neg_batched_form(_hetero(cabi, (1024, -1, -1), 5), LDS)
    assert form == 1 and 0 < lds_h <= LDS
    assert cabi.neg_batched_form(_hetero(cabi, (1024, 0, 0), 5), LDS)[0] == 1
    assert cabi.neg_batched_form(_homo(cabi, 65536, 5), LDS)[0] == 0
    assert cabi.neg_batched_form(_homo(cabi, 1024, 5, node_count=1 << 33), LDS)[0] == 0
    assert cabi.neg_batched_form(_homo(cabi, 1024, 5), 64 * 1024)[0] == 0        # a device with less LDS
    assert cabi.neg_batched_form(_homo(cabi, 34, 10), 64 * 1024)[0] == 1


class _Out:
    """tg_neg_batched_out with null device pointers; pitches as given (default: the capacities)."""

    def __init__(self, cabi, p, pitch_nodes=None, pitch_edges=None, counts=0, panic=0):
        T, R = p.n_types, p.n_rels
        cap_n, cap_e = ([0] * T, [0] * R)
        try:
            cap_n, cap_e = cabi.neg_batched_capacity(p)
        except cabi.TchGeoError:
            pass
        self.keep = [(C.c_void_p * T)(), (C.c_int64 * T)(*(pitch_nodes or cap_n)), (C.c_void_p * R)(), (C.c_void_p * R)(),
                     (C.c_int64 * R)(*(pitch_edges or cap_e))]
        self.out = cabi.TgNegBatchedOut(*self.keep, counts, panic)


def _refused(cabi, p, word, n_calls=4, out=None, rng=True, ws_bytes=1 << 40):
    o = out if out is not None else (_Out(cabi, p) if p is not None else None)
    r = cabi.TgRng(1, 0)
    rc = cabi.lib.tg_neg_sample_batched(C.byref(p) if p is not None else None, C.c_int64(n_calls),
                                        C.byref(r) if rng else None, C.byref(o.out) if o is not None else None, None,
                                        C.c_int64(ws_bytes), None)
    msg = cabi.lib.tg_last_error().decode()
    assert rc == 1, (rc, msg)
    assert "tg_neg_sample_batched" in msg and word in msg, msg


def test_refusals_before_any_launch(cabi):
    """Every bad argument returns TG_ERR_INVALID with a message that names it.  All device pointers are null (inputs, slabs,
    counts, panic, workspace), so nothing can have been launched."""
    good = _homo(cabi, 64, 5)
    _refused(cabi, None, "null", out=_Out(cabi, good))                      # null problem
    _refused(cabi, good, "null", rng=False)                                 # null rng
    rc = cabi.lib.tg_neg_sample_batched(C.byref(good), C.c_int64(4), C.byref(cabi.TgRng(1, 0)), None, None, C.c_int64(0), None)
    assert rc == 1 and "null" in cabi.lib.tg_last_error().decode()          # null out
    _refused(cabi, good, "n_calls", n_calls=0)
    _refused(cabi, good, "n_calls", n_calls=-3)
    _refused(cabi, good, "n_calls", n_calls=cabi.TG_NEG_MAX_CALLS + 1)
    many = _hetero(cabi, [8] + [-1] * 2, 2, pattern=[(0, 1)] * 33)          # more than NEG_MAX_RELS = 32 relations
    _refused(cabi, many, "relations")
    _refused(cabi, _homo(cabi, 64, -1), "num_neg")
    _refused(cabi, _homo(cabi, 64, 5, tries=-2), "try_count")
    # type 2 of this pattern has inputs and no outgoing relation (the reference panics on it)
    _refused(cabi, _hetero(cabi, (8, -1, 8), 2, pattern=[(0, 1), (1, 2)]), "no outgoing relation")
    cap_n, cap_e = cabi.neg_batched_capacity(good)
    _refused(cabi, good, "pitch_nodes", out=_Out(cabi, good, pitch_nodes=[cap_n[0] - 1]))
    _refused(cabi, good, "pitch_edges", out=_Out(cabi, good, pitch_edges=[cap_e[0] - 1]))
    het = _hetero(cabi, (1024, -1, -1), 5)
    cap_n, cap_e = cabi.neg_batched_capacity(het)
    _refused(cabi, het, "pitch_nodes", out=_Out(cabi, het, pitch_nodes=cap_n[:2] + [cap_n[2] - 1]))
    _refused(cabi, het, "pitch_edges", out=_Out(cabi, het, pitch_edges=[cap_e[0], cap_e[1] - 1] + cap_e[2:]))
    # a well-formed problem with null device buffers does not get through either, whatever form it would take
    for p in (good, _homo(cabi, 65536, 5)):
        o = _Out(cabi, p)
        assert cabi.lib.tg_neg_sample_batched(C.byref(p), C.c_int64(4), C.byref(cabi.TgRng(1, 0)), C.byref(o.out), None,
                                              C.c_int64(0), None) != 0


def test_short_workspace_is_refused(cabi):
    """The call-by-call form needs tg_neg_workspace_bytes; a shorter (here: absent) workspace is refused by name.  Without a
    device that size cannot be asked for, and the call fails on that query instead -- before anything is launched either
    way."""
    p = _homo(cabi, 65536, 5)
    o = _Out(cabi, p)
    r = cabi.TgRng(1, 0)
    rc = cabi.lib.tg_neg_sample_batched(C.byref(p), C.c_int64(2), C.byref(r), C.byref(o.out), None, C.c_int64(0), None)
    msg = cabi.lib.tg_last_error().decode()
    single = C.c_int64(-1)
    if cabi.lib.tg_neg_workspace_bytes(C.byref(p), C.byref(single)) == 0:
        assert rc == 1 and "workspace too small" in msg, msg
    else:
        assert rc != 0 and "device" in msg, msg


def test_capacity_and_form_refuse_malformed_problems(cabi):
    for fn in (cabi.neg_batched_capacity, lambda p: cabi.neg_batched_form(p, LDS)):
        with pytest.raises(cabi.TchGeoError, match="num_neg"):
            fn(_homo(cabi, 64, -1))
        with pytest.raises(cabi.TchGeoError, match="relations"):
            fn(_hetero(cabi, [8, -1, -1], 2, pattern=[(0, 1)] * 33))
        with pytest.raises(cabi.TchGeoError, match="no outgoing relation"):
            fn(_hetero(cabi, (8, -1, 8), 2, pattern=[(0, 1), (1, 2)]))
