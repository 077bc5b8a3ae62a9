"""ctypes binding of include/tchgeo_lp.h: the balanced label-propagation partitioner (tg_lp_sizes, tg_lp_propose,
tg_lp_commit; csrc/lp.hip) in the library _cabi.py loads.  A module of its own, as the header is a header of its own."""
import ctypes as C

import torch

from ._cabi import _status_check, check, lib, ptr, stream_ptr

EXPORTS = ["tg_lp_workspace_bytes", "tg_lp_sizes", "tg_lp_propose", "tg_lp_commit"]

TAG_LP = 20                          # tchgeo_lp.h
LP_MAX_PARTS = 1 << 20
LP_WAVE_MAX, LP_LDS_LABELS = 512, 2048
LP_WAVE_GROUPS, LP_GROUP_GROUPS, LP_DENSE_GROUPS = 2048, 1024, 32
FORM_AUTO, FORM_WAVE, FORM_GROUP = 0, 1, 2
STATUS_LABEL, STATUS_TARGET = 1, 2
STAY = -1                            # the all-ones skey of a vertex that stays, as the int64 torch holds

_P, _I64, _I32, _U64 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint64
lib.tg_lp_workspace_bytes.argtypes = [_I64, _I32, _I32, _I32, _P, _P]
lib.tg_lp_sizes.argtypes = [_P, _I64, _I32, _P, _P, _P]
lib.tg_lp_propose.argtypes = [_P, _P, _I32, _U64, _U64, _I32, _I32, _P, _P, _P, _P, _I64, _P]
lib.tg_lp_commit.argtypes = [_P, _P, _I64, _I32, _I64, _P, _P, _P, _P, _I64, _P]
for _n in EXPORTS:
    getattr(lib, _n).restype = C.c_int


def lp_workspace_bytes(n, n_parts, form=FORM_AUTO, wave_max=0):
    """-> (bytes, form taken): one workspace that serves tg_lp_propose and tg_lp_commit over n vertices; no device is
    touched"""
    b, f = C.c_int64(-1), C.c_int32(-1)
    check(lib.tg_lp_workspace_bytes(int(n), int(n_parts), int(form), int(wave_max), C.byref(b), C.byref(f)))
    return b.value, f.value


def lp_workspace(n, n_parts, device, form=FORM_AUTO, wave_max=0):
    """an int64 tensor of exactly the queried bytes"""
    return torch.empty(lp_workspace_bytes(n, n_parts, form, wave_max)[0] // 8, dtype=torch.int64, device=device)


def lp_sizes(label, n_parts, size, status):
    """size[l] = |{v: label[v] = l}| (tg_lp_sizes) on the current stream; label int32 [n], size int64 [P], status int32 [1]"""
    check(lib.tg_lp_sizes(ptr(label) if label.numel() else None, label.numel(), int(n_parts), ptr(size), ptr(status),
                          stream_ptr(size.device)))


def lp_propose(graph, label, n_parts, seed, round, skey, cut, status, ws, form=FORM_AUTO, wave_max=0):
    """tg_lp_propose on the current stream: skey int64 [n] (the uint64 words), cut a one-element int64 view (added to), ws
    an int64 tensor (lp_workspace).  Does not synchronise."""
    check(lib.tg_lp_propose(C.byref(graph), ptr(label), int(n_parts), int(seed), int(round), int(form), int(wave_max),
                            ptr(skey), ptr(cut), ptr(status), ptr(ws), ws.numel() * 8, stream_ptr(skey.device)))


def lp_commit(label, size, n_parts, cap, skey, moved, status, ws):
    """tg_lp_commit on the current stream: label and size are updated in place, moved (a one-element int64 view) is added
    to.  Does not synchronise."""
    check(lib.tg_lp_commit(ptr(label), ptr(size), label.numel(), int(n_parts), int(cap), ptr(skey), ptr(moved), ptr(status),
                           ptr(ws), ws.numel() * 8, stream_ptr(label.device)))


def lp_status_check(status, who, mask=-1):
    """the status word after its read-back: bit 0 = a label outside [0, num_parts), bit 1 = an skey whose target is"""
    _status_check(status, who, ((STATUS_LABEL, "a label outside [0, num_parts)"),
                                (STATUS_TARGET, "a proposal whose target is outside [0, num_parts)")), mask=mask)
