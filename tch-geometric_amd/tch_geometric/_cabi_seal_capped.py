"""ctypes binding of include/tchgeo_seal_capped.h: SEAL enclosing subgraphs with a cap on the new vertices of every hop
(tg_seal_nodes_capped, csrc/seal_capped.hip) in the library _cabi.py loads.  A module of its own, as the header is a header of
its own; the sizes, the structs and the status word are _cabi_seal's."""
import ctypes as C

import torch

from ._cabi import check, lib, ptr, stream_ptr
from ._cabi_seal import FORM_AUTO, OUTPUTS, Seal, TgSealOut

EXPORTS = ["tg_seal_capped_workspace_bytes", "tg_seal_nodes_capped"]

TAG_SEAL_HOP = 19                    # tchgeo_seal_capped.h
SEAL_HOP_CAP_MAX = 1024


def pool_places(k):
    """TG_SEAL_POOL_PLACES(k)"""
    return 1024 if k <= 256 else 2048 if k <= 512 else 4096


def pool_cap(k):
    """TG_SEAL_POOL_CAP(k): the candidates of a capped hop that the pool lists before it is compacted"""
    return pool_places(k) // 2


class TgSealCaps(C.Structure):
    _fields_ = [("max_per_hop", C.c_void_p), ("seed", C.c_uint64), ("call_ids", C.c_void_p), ("call_id0", C.c_int64),
                ("cut", C.c_void_p)]


_P, _I64, _I32 = C.c_void_p, C.c_int64, C.c_int32
lib.tg_seal_capped_workspace_bytes.argtypes = [_I64, _I32, _I32, _I32, _P, _P]
lib.tg_seal_nodes_capped.argtypes = [_P, _P, _P, _P, _I64, _I32, _P, _P, _I64, _P]
for _n in EXPORTS:
    getattr(lib, _n).restype = C.c_int


def hop_caps(max_per_hop, num_hops):
    """an int or one int per hop -> a list of num_hops caps in [0, SEAL_HOP_CAP_MAX]; ValueError otherwise"""
    if not isinstance(max_per_hop, (int, list, tuple)):
        raise ValueError("max_per_hop must be an int or one int per hop, got %r" % (max_per_hop,))
    caps = [max_per_hop] * num_hops if isinstance(max_per_hop, int) else list(max_per_hop)
    if len(caps) != num_hops or not all(isinstance(k, int) and not isinstance(k, bool) for k in caps):
        raise ValueError("max_per_hop must be an int or %d ints, got %r" % (num_hops, max_per_hop))
    if not all(0 <= k <= SEAL_HOP_CAP_MAX for k in caps):
        raise ValueError("max_per_hop = %r outside [0, %d]" % (max_per_hop, SEAL_HOP_CAP_MAX))
    return caps


def workspace_bytes(m, node_cap, max_cap, form=FORM_AUTO):
    """-> (bytes, form taken) of a call over m slots (tg_seal_capped_workspace_bytes); no device is touched"""
    b, f = C.c_int64(-1), C.c_int32(-1)
    check(lib.tg_seal_capped_workspace_bytes(int(m), int(node_cap), int(max_cap), int(form), C.byref(b), C.byref(f)))
    return b.value, f.value


def seal_nodes_capped(graph, src, dst, sizes, max_per_hop, seed, call_ids=None, call_id0=0, ws=None, out=None, status=None,
                      distances=True, cut=True):
    """tg_seal_nodes_capped over the links (src[i], dst[i]) (int64 [m], device) on the current stream: `sizes` is a
    _cabi_seal.Seal, max_per_hop an int or one int per hop (0: the hop is not capped), slot i's call id call_ids[i] (int64 [m],
    device) or call_id0 + i.  -> _cabi_seal.seal_nodes' dict plus cut [m] (bit t - 1: hop t was cut; None when out has none
    or cut is False).  Nothing behind count[i] in a row is written; the call does not synchronise."""
    if not isinstance(sizes, Seal):
        raise ValueError("seal_nodes_capped: sizes must be a _cabi_seal.Seal")
    caps = hop_caps(max_per_hop, sizes.num_hops)
    for t in (src, dst) + (() if call_ids is None else (call_ids,)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError("seal_nodes_capped: src, dst and call_ids must be contiguous flat int64 tensors")
        if t.shape != src.shape or t.device != src.device:
            raise ValueError("seal_nodes_capped: src, dst and call_ids must have one length and one device")
    dev, m, cap = src.device, src.numel(), sizes.node_cap
    if out is None:
        i64 = dict(dtype=torch.int64, device=dev)
        out = dict(count=torch.empty(m, **i64), nodes=torch.empty((m, cap), **i64), z=torch.empty((m, cap), **i64),
                   du=torch.empty((m, cap), **i64) if distances else None,
                   dv=torch.empty((m, cap), **i64) if distances else None,
                   rounds=torch.empty(m, **i64) if distances else None, cut=torch.empty(m, **i64) if cut else None)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    need = workspace_bytes(m, cap, max(caps), sizes.form)[0]
    if need and (ws is None or ws.numel() * 8 < need or ws.device != dev):
        ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    address = lambda t: t.data_ptr() if t is not None and t.numel() else None
    so = TgSealOut(*(address(out[name]) for name in OUTPUTS))
    si = sizes.struct(src, dst)
    hops = (C.c_int32 * len(caps))(*caps)
    sc = TgSealCaps(C.cast(hops, C.c_void_p), int(seed) & (2 ** 64 - 1), address(call_ids), int(call_id0), address(out.get("cut")))
    check(lib.tg_seal_nodes_capped(C.byref(graph), C.byref(si), C.byref(sc), C.byref(so), m, sizes.form, ptr(status),
                                   ptr(ws) if need else None, ws.numel() * 8 if need else 0, stream_ptr(dev)))
    out.update(status=status, ws=ws)
    out.setdefault("cut", None)
    return out
