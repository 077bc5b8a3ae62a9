"""ctypes binding of include/tchgeo_seal.h: SEAL enclosing subgraphs with double-radius node labels per link (tg_seal_nodes,
csrc/seal.hip) in the library _cabi.py loads.  A module of its own, as the header is a header of its own."""
import ctypes as C

import torch

from ._cabi import _status_check, check, lib, ptr, stream_ptr

EXPORTS = ["tg_seal_workspace_bytes", "tg_seal_nodes"]

SEAL_MAX_HOPS = 64                   # tchgeo_seal.h
SEAL_MAX_CAP = 1 << 20
SEAL_LDS_CAP_SMALL, SEAL_LDS_CAP = 512, 2048
SEAL_WS_GROUPS = 128
FORM_AUTO, FORM_LDS, FORM_WORKSPACE = 0, 1, 2
STATUS_CAP, STATUS_RANGE, STATUS_SAME = 1, 2, 4
ROWS = ("nodes", "z", "du", "dv")    # [m, node_cap] each; du / dv optional
OUTPUTS = ("count",) + ROWS + ("rounds",)


class TgSealIn(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("num_hops", C.c_int32), ("node_cap", C.c_int32),
                ("z_max", C.c_int64)]


class TgSealOut(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in OUTPUTS]


_P, _I64, _I32 = C.c_void_p, C.c_int64, C.c_int32
lib.tg_seal_workspace_bytes.argtypes = [_I64, _I32, _I32, _P, _P]
lib.tg_seal_nodes.argtypes = [_P, _P, _P, _I64, _I32, _P, _P, _I64, _P]
for _n in EXPORTS:
    getattr(lib, _n).restype = C.c_int


class Seal:
    """The sizes of tg_seal_nodes calls: num_hops, node_cap vertices per link at most (the pitch of the output rows), z_max
    (0: labels are not clamped).  Refuses what needs no device as ValueError."""

    def __init__(self, num_hops=1, node_cap=1024, z_max=0, form=FORM_AUTO):
        self.num_hops, self.node_cap, self.z_max, self.form = int(num_hops), int(node_cap), int(z_max), int(form)
        if not 1 <= self.num_hops <= SEAL_MAX_HOPS:
            raise ValueError("Seal: num_hops = %d outside [1, %d]" % (self.num_hops, SEAL_MAX_HOPS))
        if not 2 <= self.node_cap <= SEAL_MAX_CAP:
            raise ValueError("Seal: node_cap = %d outside [2, 2^20]" % self.node_cap)
        if not 0 <= self.z_max < 2 ** 63:
            raise ValueError("Seal: z_max = %d outside [0, 2^63)" % self.z_max)
        if self.form not in (FORM_AUTO, FORM_LDS, FORM_WORKSPACE):
            raise ValueError("Seal: unknown form %d" % self.form)
        if self.form == FORM_LDS and self.node_cap > SEAL_LDS_CAP:
            raise ValueError("Seal: node_cap = %d exceeds the LDS form's %d" % (self.node_cap, SEAL_LDS_CAP))

    @staticmethod
    def workspace_bytes(m, node_cap, form=FORM_AUTO):
        """-> (bytes, form taken) of a call over m slots (tg_seal_workspace_bytes); no device is touched"""
        b, f = C.c_int64(-1), C.c_int32(-1)
        check(lib.tg_seal_workspace_bytes(int(m), int(node_cap), int(form), C.byref(b), C.byref(f)))
        return b.value, f.value

    def struct(self, src, dst):
        return TgSealIn(src.data_ptr() if src.numel() else None, dst.data_ptr() if dst.numel() else None, self.num_hops,
                        self.node_cap, self.z_max)


def seal_nodes(graph, src, dst, num_hops=1, node_cap=1024, z_max=0, form=FORM_AUTO, ws=None, out=None, status=None,
               distances=True):
    """tg_seal_nodes over the links (src[i], dst[i]) (int64 [m], device) on the current stream -> dict(count [m], nodes / z
    [m, node_cap], du / dv [m, node_cap] or None, rounds [m] or None, status [1] int32, ws).  Nothing behind count[i] in a
    row is written; the call does not synchronise.  out: a dict of an earlier call with the same shapes, written again; ws:
    an int64 tensor, reused when large enough."""
    sizes = num_hops if isinstance(num_hops, Seal) else Seal(num_hops, node_cap, z_max, form)
    for t in (src, dst):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError("seal_nodes: src and dst must be contiguous flat int64 tensors")
    if src.shape != dst.shape or src.device != dst.device:
        raise ValueError("seal_nodes: src and dst must have one length and one device")
    dev, m, cap = src.device, src.numel(), sizes.node_cap
    if out is None:
        i64 = dict(dtype=torch.int64, device=dev)
        out = dict(count=torch.empty(m, **i64), nodes=torch.empty((m, cap), **i64), z=torch.empty((m, cap), **i64),
                   du=torch.empty((m, cap), **i64) if distances else None,
                   dv=torch.empty((m, cap), **i64) if distances else None,
                   rounds=torch.empty(m, **i64) if distances else None)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    need = Seal.workspace_bytes(m, cap, sizes.form)[0]
    if need and (ws is None or ws.numel() * 8 < need or ws.device != dev):
        ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    so = TgSealOut(*(out[name].data_ptr() if out[name] is not None and out[name].numel() else None for name in OUTPUTS))
    si = sizes.struct(src, dst)
    check(lib.tg_seal_nodes(C.byref(graph), C.byref(si), C.byref(so), m, sizes.form, ptr(status), ptr(ws) if need else None,
                            ws.numel() * 8 if need else 0, stream_ptr(dev)))
    out.update(status=status, ws=ws)
    return out


def seal_status_check(status, who, mask=-1):
    """the status word of tg_seal_nodes after its read-back: bit 0 = a link's enclosing subgraph has more than node_cap
    vertices, bit 1 = an endpoint outside the graph, bit 2 = a link from a vertex to itself"""
    _status_check(status, who, ((STATUS_CAP, "a link's enclosing subgraph has more vertices than node_cap holds"),
                                (STATUS_RANGE, "a link's endpoint outside the graph"),
                                (STATUS_SAME, "a link from a vertex to itself")), mask=mask)
