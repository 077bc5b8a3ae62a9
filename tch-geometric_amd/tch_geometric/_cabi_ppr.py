"""ctypes binding of include/tchgeo_ppr.h: approximate personalised PageRank by forward push, top-k per seed (tg_ppr_topk,
csrc/ppr.hip) in the library _cabi.py loads.  A module of its own, as the header is a header of its own."""
import ctypes as C

import torch

from ._cabi import _status_check, check, lib, ptr, stream_ptr

EXPORTS = ["tg_ppr_workspace_bytes", "tg_ppr_topk"]

PPR_UNIT = 1 << 31                   # tchgeo_ppr.h: U
PPR_MAX_ROUNDS = 65536
PPR_MAX_CAP = 1 << 20
PPR_LDS_CAP_SMALL, PPR_LDS_CAP = 512, 2048
PPR_WS_GROUPS = 128
FORM_AUTO, FORM_LDS, FORM_WORKSPACE = 0, 1, 2
DIAGNOSTICS = ("touched", "rounds", "activations", "residual", "mass")


class TgPprIn(C.Structure):
    _fields_ = [("seeds", C.c_void_p), ("alpha_q", C.c_uint32), ("eps_q", C.c_uint32), ("max_rounds", C.c_int32),
                ("k", C.c_int32), ("node_cap", C.c_int32)]


class TgPprOut(C.Structure):
    _fields_ = [("count", C.c_void_p), ("nodes", C.c_void_p), ("score", C.c_void_p), ("weight", C.c_void_p)] + [
        (name, C.c_void_p) for name in DIAGNOSTICS]


_P, _I64, _I32 = C.c_void_p, C.c_int64, C.c_int32
lib.tg_ppr_workspace_bytes.argtypes = [_I64, _I32, _I32, _I32, _P, _P]
lib.tg_ppr_topk.argtypes = [_P, _P, _P, _I64, _I32, _P, _P, _I64, _P]
for _n in EXPORTS:
    getattr(lib, _n).restype = C.c_int


def alpha_to_q(alpha):
    """restart probability -> alpha_q = round(alpha * 2^32) inside [1, 2^32 - 1]"""
    return min(max(int(round(float(alpha) * 2.0 ** 32)), 1), 2 ** 32 - 1)


def eps_to_q(eps):
    """push threshold per unit of degree -> eps_q = max(1, round(eps * 2^31))"""
    return max(1, int(round(float(eps) * 2.0 ** 31)))


class PPR:
    """The sizes of tg_ppr_topk calls: k rows per slot, node_cap touched vertices per slot at most, alpha / eps as floats
    (converted once) or alpha_q / eps_q directly.  Refuses what needs no device as ValueError."""

    def __init__(self, k, node_cap, alpha=0.15, eps=1e-4, max_rounds=64, alpha_q=None, eps_q=None, form=FORM_AUTO):
        self.k, self.node_cap, self.max_rounds, self.form = int(k), int(node_cap), int(max_rounds), int(form)
        self.alpha_q = alpha_to_q(alpha) if alpha_q is None else int(alpha_q)
        self.eps_q = eps_to_q(eps) if eps_q is None else int(eps_q)
        if not 1 <= self.node_cap <= PPR_MAX_CAP:
            raise ValueError("PPR: node_cap = %d outside [1, 2^20]" % self.node_cap)
        if not 1 <= self.k <= self.node_cap:
            raise ValueError("PPR: k = %d outside [1, node_cap = %d]" % (self.k, self.node_cap))
        if not 1 <= self.alpha_q <= 2 ** 32 - 1:
            raise ValueError("PPR: alpha_q = %d outside [1, 2^32 - 1]" % self.alpha_q)
        if not 1 <= self.eps_q <= PPR_UNIT:
            raise ValueError("PPR: eps_q = %d outside [1, 2^31]" % self.eps_q)
        if not 1 <= self.max_rounds <= PPR_MAX_ROUNDS:
            raise ValueError("PPR: max_rounds = %d outside [1, %d]" % (self.max_rounds, PPR_MAX_ROUNDS))
        if self.form not in (FORM_AUTO, FORM_LDS, FORM_WORKSPACE):
            raise ValueError("PPR: unknown form %d" % self.form)
        if self.form == FORM_LDS and self.node_cap > PPR_LDS_CAP:
            raise ValueError("PPR: node_cap = %d exceeds the LDS form's %d" % (self.node_cap, PPR_LDS_CAP))

    @staticmethod
    def workspace_bytes(m, k, node_cap, form=FORM_AUTO):
        """-> (bytes, form taken) of a call over m slots (tg_ppr_workspace_bytes); no device is touched"""
        b, f = C.c_int64(-1), C.c_int32(-1)
        check(lib.tg_ppr_workspace_bytes(int(m), int(k), int(node_cap), int(form), C.byref(b), C.byref(f)))
        return b.value, f.value

    def struct(self, seeds):
        return TgPprIn(seeds.data_ptr() if seeds.numel() else None, self.alpha_q, self.eps_q, self.max_rounds, self.k,
                       self.node_cap)


def ppr_topk(graph, seeds, k, node_cap, alpha=0.15, eps=1e-4, max_rounds=64, alpha_q=None, eps_q=None, form=FORM_AUTO,
             ws=None, out=None, status=None, with_weight=True, diagnostics=True):
    """tg_ppr_topk over seeds [m] (int64, device) on the current stream -> dict(count [m], nodes / score [m, k], weight
    [m, k] float32 or None, touched / rounds / activations / residual / mass [m] or None, status [1] int32, ws).  Nothing
    behind count[i] in a row is written; the call does not synchronise.  out: a dict of an earlier call with the same
    shapes, written again; ws: an int64 tensor, reused when large enough."""
    sizes = k if isinstance(k, PPR) else PPR(k, node_cap, alpha, eps, max_rounds, alpha_q, eps_q, form)
    if not isinstance(seeds, torch.Tensor) or seeds.dtype != torch.int64 or seeds.dim() != 1 or not seeds.is_contiguous():
        raise ValueError("ppr_topk: seeds must be a contiguous flat int64 tensor")
    dev, m, K = seeds.device, seeds.numel(), sizes.k
    if out is None:
        out = dict(count=torch.empty(m, dtype=torch.int64, device=dev),
                   nodes=torch.empty((m, K), dtype=torch.int64, device=dev),
                   score=torch.empty((m, K), dtype=torch.int64, device=dev),
                   weight=torch.empty((m, K), dtype=torch.float32, device=dev) if with_weight else None)
        for name in DIAGNOSTICS:
            out[name] = torch.empty(m, dtype=torch.int64, device=dev) if diagnostics else None
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    need = PPR.workspace_bytes(m, K, sizes.node_cap, sizes.form)[0]
    if need and (ws is None or ws.numel() * 8 < need or ws.device != dev):
        ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    so = TgPprOut(*(out[name].data_ptr() if out[name] is not None and out[name].numel() else None
                    for name in ("count", "nodes", "score", "weight") + DIAGNOSTICS))
    si = sizes.struct(seeds)
    check(lib.tg_ppr_topk(C.byref(graph), C.byref(si), C.byref(so), m, sizes.form, ptr(status), ptr(ws) if need else None,
                          ws.numel() * 8 if need else 0, stream_ptr(dev)))
    out.update(status=status, ws=ws)
    return out


def compact_rows_at(src, lens, off, n_rows, dst):
    """tg_compact_rows with the caller's offsets: dst.reshape(-1)[off[r] + c] = src[r, c] for c < lens[r], r < n_rows (int64
    tensors; src [>= n_rows, pitch]).  A launch's [slots, k] rows go to per-mini-batch lists of a fixed pitch this way."""
    check(lib.tg_compact_rows(ptr(src), C.c_int64(src.stride(0)), ptr(lens), C.c_int64(1), ptr(off), C.c_int64(n_rows),
                              ptr(dst), stream_ptr(src.device)))


def ppr_status_check(status, who, mask=-1):
    """the status word of tg_ppr_topk after its read-back: bit 0 = a slot touched more than node_cap vertices, bit 1 = a
    seed outside the graph"""
    _status_check(status, who, ((1, "a seed's push touched more vertices than node_cap holds"),
                                (2, "a seed outside the graph")), mask=mask)
