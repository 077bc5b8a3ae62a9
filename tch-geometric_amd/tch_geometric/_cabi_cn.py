"""ctypes binding of include/tchgeo_cn.h: the common neighbours of every candidate link (tg_cn_links, csrc/cn.hip) in the
library _cabi.py loads, and the two once-per-graph helpers in plain torch (distinct_degree, cn_tables).  A module of its
own, as the header is a header of its own."""
import ctypes as C

import torch

from ._cabi import _status_check, check, lib, ptr, stream_ptr

EXPORTS = ["tg_cn_workspace_bytes", "tg_cn_links"]

CN_MAX_CAP = 1 << 20                 # tchgeo_cn.h
CN_MAX_TABLES = 4
CN_WINDOW, CN_WAVE_MAX, CN_GROUP_TILES = 512, 4096, 256
CN_WAVE_GROUPS, CN_GROUP_GROUPS = 2048, 1024
FORM_AUTO, FORM_WAVE, FORM_GROUP = 0, 1, 2
STATUS_CAP, STATUS_RANGE = 1, 2
OUTPUTS = ("count", "cn", "adjacent", "score")
KINDS = ("aa", "ra")                 # the tables cn_tables builds: Adamic-Adar 1 / log d, resource allocation 1 / d


class TgCnIn(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("tables", C.c_void_p), ("id_bound", C.c_int64),
                ("cn_cap", C.c_int32), ("n_tables", C.c_int32), ("exclude_ends", C.c_int32), ("wave_max", C.c_int32)]


class TgCnOut(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in OUTPUTS]


_P, _I64, _I32 = C.c_void_p, C.c_int64, C.c_int32
lib.tg_cn_workspace_bytes.argtypes = [_I64, _I32, _P, _P]
lib.tg_cn_links.argtypes = [_P, _P, _P, _I64, _I32, _P, _P, _I64, _P]
for _n in EXPORTS:
    getattr(lib, _n).restype = C.c_int


class CommonNeighbors:
    """The sizes of tg_cn_links calls: cn_cap listed members per link at most (the pitch of the cn rows), the number of
    score tables, exclude_ends, the form and AUTO's wave_max (0: the header's).  Refuses what needs no device as
    ValueError."""

    def __init__(self, cn_cap=256, n_tables=0, exclude_ends=True, form=FORM_AUTO, wave_max=0):
        self.cn_cap, self.n_tables, self.exclude_ends = int(cn_cap), int(n_tables), int(bool(exclude_ends))
        self.form, self.wave_max = int(form), int(wave_max)
        if not 1 <= self.cn_cap <= CN_MAX_CAP:
            raise ValueError("CommonNeighbors: cn_cap = %d outside [1, 2^20]" % self.cn_cap)
        if not 0 <= self.n_tables <= CN_MAX_TABLES:
            raise ValueError("CommonNeighbors: n_tables = %d outside [0, %d]" % (self.n_tables, CN_MAX_TABLES))
        if self.form not in (FORM_AUTO, FORM_WAVE, FORM_GROUP):
            raise ValueError("CommonNeighbors: unknown form %d" % self.form)
        if not 0 <= self.wave_max < 2 ** 31:
            raise ValueError("CommonNeighbors: wave_max = %d outside [0, 2^31)" % self.wave_max)

    @staticmethod
    def workspace_bytes(m, form=FORM_AUTO):
        """-> (bytes, form taken) of a call over m slots (tg_cn_workspace_bytes); no device is touched"""
        b, f = C.c_int64(-1), C.c_int32(-1)
        check(lib.tg_cn_workspace_bytes(int(m), int(form), C.byref(b), C.byref(f)))
        return b.value, f.value

    def struct(self, src, dst, tables):
        return TgCnIn(src.data_ptr() if src.numel() else None, dst.data_ptr() if dst.numel() else None,
                      tables.data_ptr() if tables is not None else None, tables.shape[1] if tables is not None else 0,
                      self.cn_cap, self.n_tables, self.exclude_ends, self.wave_max)


def cn_links(graph, src, dst, cn_cap=256, tables=None, exclude_ends=True, form=FORM_AUTO, wave_max=0, ws=None, out=None,
             status=None):
    """tg_cn_links over the links (src[i], dst[i]) (int64 [m], device) on the current stream -> dict(count [m], cn
    [m, cn_cap], adjacent [m], score [m, n_tables] uint64 words in an int64 tensor or None, status [1] int32, ws).  tables:
    a contiguous int32 / uint32-worded tensor [n_tables, id_bound] (cn_tables makes one) or None.  Nothing behind
    min(count[i], cn_cap) in a row is written; the call does not synchronise.  out: a dict of an earlier call with the same
    shapes, written again (adjacent may be None); ws: an int32 tensor, reused when large enough."""
    if tables is not None and (not isinstance(tables, torch.Tensor) or tables.dtype != torch.int32 or tables.dim() != 2
                               or not tables.is_contiguous() or tables.shape[1] < 1 or tables.device != src.device):
        raise ValueError("cn_links: tables must be a contiguous int32 tensor [n_tables, id_bound] on the links' device")
    sizes = cn_cap if isinstance(cn_cap, CommonNeighbors) else CommonNeighbors(
        cn_cap, 0 if tables is None else tables.shape[0], exclude_ends, form, wave_max)
    if sizes.n_tables != (0 if tables is None else tables.shape[0]):
        raise ValueError("cn_links: the sizes object counts %d tables" % sizes.n_tables)
    for t in (src, dst):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError("cn_links: src and dst must be contiguous flat int64 tensors")
    if src.shape != dst.shape or src.device != dst.device:
        raise ValueError("cn_links: src and dst must have one length and one device")
    dev, m, cap, T = src.device, src.numel(), sizes.cn_cap, sizes.n_tables
    if out is None:
        i64 = dict(dtype=torch.int64, device=dev)
        out = dict(count=torch.empty(m, **i64), cn=torch.empty((m, cap), **i64), adjacent=torch.empty(m, **i64),
                   score=torch.empty((m, T), **i64) if T else None)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    need = CommonNeighbors.workspace_bytes(m, sizes.form)[0]
    if need and (ws is None or ws.numel() * 4 < need or ws.device != dev):
        ws = torch.empty(need // 4, dtype=torch.int32, device=dev)
    so = TgCnOut(*(out[name].data_ptr() if out[name] is not None and out[name].numel() else None for name in OUTPUTS))
    si = sizes.struct(src, dst, tables)
    check(lib.tg_cn_links(C.byref(graph), C.byref(si), C.byref(so), m, sizes.form, ptr(status), ptr(ws) if need else None,
                          ws.numel() * 4 if need else 0, stream_ptr(dev)))
    out.update(status=status, ws=ws)
    return out


def cn_status_check(status, who, mask=-1):
    """the status word of tg_cn_links after its read-back: bit 0 = a link has more common neighbours than cn_cap lists
    (its count and scores are still exact), bit 1 = an endpoint outside the graph"""
    _status_check(status, who, ((STATUS_CAP, "a link has more common neighbours than cn_cap lists"),
                                (STATUS_RANGE, "a link's endpoint outside the graph")), mask=mask)


def distinct_degree(ptrs, indices):
    """|A(x)| of every row: its entries with parallel ones counted once (rows ascend) -> int64 [n_major].  Plain torch, once
    per graph."""
    n, e = ptrs.numel() - 1, indices.numel()
    if e == 0:
        return torch.zeros(n, dtype=torch.int64, device=ptrs.device)
    row = torch.repeat_interleave(torch.arange(n, device=ptrs.device), ptrs[1:] - ptrs[:-1])
    new = torch.ones(e, dtype=torch.bool, device=ptrs.device)
    new[1:] = (indices[1:] != indices[:-1]) | (row[1:] != row[:-1])
    return torch.zeros(n, dtype=torch.int64, device=ptrs.device).index_add_(0, row, new.to(torch.int64))


def cn_tables(ptrs, indices, kinds=KINDS):
    """The fixed-point weight tables tg_cn_links sums, one row per kind over the vertices of a square graph: "aa" 1 / log d
    (0 for d < 2), "ra" 1 / d (0 for d < 1), with d the DISTINCT degree, in float64, times 2^32, rounded to nearest and
    clamped to 2^32 - 1 -> int32 [len(kinds), n_major] holding the uint32 words.  Plain torch, once per graph."""
    for kind in kinds:
        if kind not in KINDS:
            raise ValueError("cn_tables: unknown kind %r (known: %s)" % (kind, ", ".join(KINDS)))
    if not 1 <= len(kinds) <= CN_MAX_TABLES:
        raise ValueError("cn_tables: between 1 and %d kinds, got %d" % (CN_MAX_TABLES, len(kinds)))
    d = distinct_degree(ptrs, indices).to(torch.float64)
    rows = []
    for kind in kinds:
        if kind == "aa":
            w = torch.where(d >= 2, 1.0 / torch.log(d.clamp(min=2.0)), torch.zeros_like(d))
        else:
            w = torch.where(d >= 1, 1.0 / d.clamp(min=1.0), torch.zeros_like(d))
        words = torch.round(w * 2.0 ** 32).clamp(max=2.0 ** 32 - 1).to(torch.int64)
        rows.append(torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32))   # the same 32 bits
    return torch.stack(rows).contiguous()
