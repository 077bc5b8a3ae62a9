"""ctypes binding of include/tchgeo_sketch.h: MinHash / HyperLogLog subgraph sketches (tg_sketch_init, tg_sketch_propagate,
tg_sketch_links, csrc/sketch.hip) in the library _cabi.py loads, and the cardinality and structure-feature formulas of ELPH /
BUDDY over their integers in plain elementwise torch.  A module of its own, as the header is a header of its own."""
import ctypes as C
import math

import torch

from ._cabi import _status_check, check, lib, ptr, stream_ptr

EXPORTS = ["tg_sketch_bytes", "tg_sketch_init", "tg_sketch_propagate_workspace_bytes", "tg_sketch_propagate", "tg_sketch_links"]

SKETCH_MAX_HOPS = 3                  # tchgeo_sketch.h
SKETCH_WAVE_MAX, SKETCH_GROUP_MAX, SKETCH_SPLIT_SEG, SKETCH_SPLIT_SEG_MIN = 64, 4096, 2048, 64
SKETCH_WAVE_GROUPS, SKETCH_GROUP_GROUPS = 2048, 2048
FORM_AUTO, FORM_WAVE, FORM_GROUP, FORM_SPLIT = 0, 1, 2, 3
STATUS_RANGE, STATUS_GRAPH = 2, 4
LINK_OUTPUTS = ("match", "usum", "uzero", "nsum", "nzero")


class TgSketchParams(C.Structure):
    _fields_ = [("n_perm", C.c_int32), ("hll_p", C.c_int32), ("hops", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64)]


class TgSketchTuning(C.Structure):
    _fields_ = [("wave_max", C.c_int32), ("group_max", C.c_int32), ("split_seg", C.c_int32)]


class TgSketchLinkOut(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in LINK_OUTPUTS]


_P, _I64, _I32 = C.c_void_p, C.c_int64, C.c_int32
lib.tg_sketch_bytes.argtypes = [_P, _I64, _P, _P]
lib.tg_sketch_init.argtypes = [_P, _I64, _P, _P]
lib.tg_sketch_propagate_workspace_bytes.argtypes = [_P, _I64, _I64, _I32, _P, _P, _P]
lib.tg_sketch_propagate.argtypes = [_P, _P, _P, _P, _I32, _P, _P, _P, _I64, _P]
lib.tg_sketch_links.argtypes = [_P, _I64, _P, _P, _P, _P, _I64, _P, _P]
for _n in EXPORTS:
    getattr(lib, _n).restype = C.c_int


class Sketch:
    """The parameters of a sketch: n_perm MinHash words (a multiple of 64 in [64, 256]), 2^hll_p HyperLogLog registers
    (hll_p in [8, 10]), hops in [1, 3], a uint64 seed; the form of a hop and AUTO's thresholds (0: the header's).  Refuses
    what needs no device as ValueError."""

    def __init__(self, hops=2, n_perm=128, hll_p=8, seed=0, form=FORM_AUTO, wave_max=0, group_max=0, split_seg=0):
        self.hops, self.n_perm, self.hll_p, self.seed, self.form = int(hops), int(n_perm), int(hll_p), int(seed), int(form)
        self.wave_max, self.group_max, self.split_seg = int(wave_max), int(group_max), int(split_seg)
        if not (64 <= self.n_perm <= 256 and self.n_perm % 64 == 0):
            raise ValueError("Sketch: n_perm = %d is no multiple of 64 in [64, 256]" % self.n_perm)
        if not 8 <= self.hll_p <= 10:
            raise ValueError("Sketch: hll_p = %d outside [8, 10]" % self.hll_p)
        if not 1 <= self.hops <= SKETCH_MAX_HOPS:
            raise ValueError("Sketch: hops = %d outside [1, %d]" % (self.hops, SKETCH_MAX_HOPS))
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("Sketch: seed = %d is no uint64" % self.seed)
        if self.form not in (FORM_AUTO, FORM_WAVE, FORM_GROUP, FORM_SPLIT):
            raise ValueError("Sketch: unknown form %d" % self.form)
        if not (0 <= self.wave_max <= 2 ** 30 and 0 <= self.group_max <= 2 ** 30):
            raise ValueError("Sketch: wave_max = %d, group_max = %d outside [0, 2^30]" % (self.wave_max, self.group_max))
        if self.split_seg and not SKETCH_SPLIT_SEG_MIN <= self.split_seg <= SKETCH_SPLIT_SEG:
            raise ValueError("Sketch: split_seg = %d outside [%d, %d]" % (self.split_seg, SKETCH_SPLIT_SEG_MIN, SKETCH_SPLIT_SEG))
        self.m_reg = 1 << self.hll_p
        self.row_words = self.n_perm + self.m_reg // 4
        self.params = TgSketchParams(self.n_perm, self.hll_p, self.hops, 0, self.seed)
        self.tuning = TgSketchTuning(self.wave_max, self.group_max, self.split_seg)

    def key(self):
        return (self.hops, self.n_perm, self.hll_p, self.seed)

    def bytes(self, n):
        """-> (bytes of the [hops + 1, n, W] array, W) (tg_sketch_bytes); no device is touched"""
        b, w = C.c_int64(-1), C.c_int64(-1)
        check(lib.tg_sketch_bytes(C.byref(self.params), int(n), C.byref(b), C.byref(w)))
        return b.value, w.value

    def workspace_bytes(self, n, n_edges):
        """-> (bytes, form taken) of a hop over n rows with n_edges entries; no device is touched"""
        b, f = C.c_int64(-1), C.c_int32(-1)
        check(lib.tg_sketch_propagate_workspace_bytes(C.byref(self.params), int(n), int(n_edges), self.form, C.byref(self.tuning),
                                                      C.byref(b), C.byref(f)))
        return b.value, f.value


def sketch_init(sizes, hop0):
    """tg_sketch_init into hop0 (int32 [n, W], device) on the current stream"""
    check(lib.tg_sketch_init(C.byref(sizes.params), hop0.shape[0], ptr(hop0), stream_ptr(hop0.device)))


def sketch_propagate(graph, sizes, prev, nxt, status, ws=None):
    """tg_sketch_propagate of prev into nxt (int32 [n, W] each) on the current stream -> the workspace (an int32 tensor, reused
    when large enough)"""
    need = sizes.workspace_bytes(graph.n_major, graph.n_edges)[0]
    if need and (ws is None or ws.numel() * 4 < need or ws.device != prev.device):
        ws = torch.empty(need // 4, dtype=torch.int32, device=prev.device)
    check(lib.tg_sketch_propagate(C.byref(graph), C.byref(sizes.params), ptr(prev), ptr(nxt), sizes.form, C.byref(sizes.tuning),
                                  ptr(status), ptr(ws) if need else None, ws.numel() * 4 if need else 0, stream_ptr(prev.device)))
    return ws


def sketch_build(view, hops=2, n_perm=128, hll_p=8, seed=0, form=FORM_AUTO, device=None, status=None, **tuning):
    """An init, then `hops` propagates over the graph view into one tensor -> (sketch int32 [hops + 1, n, W] holding the uint32
    words, status [1] int32).  hops may be a Sketch.  Stream-ordered; nothing is read back."""
    sizes = hops if isinstance(hops, Sketch) else Sketch(hops, n_perm, hll_p, seed, form, **tuning)
    n = int(view.n_major)
    if not 1 <= n <= 2 ** 31:
        raise ValueError("sketch_build: n = %d outside [1, 2^31]" % n)
    dev = torch.device(device) if device is not None else view._keep[0].device
    sketch = torch.empty((sizes.hops + 1, n, sizes.row_words), dtype=torch.int32, device=dev)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    sketch_init(sizes, sketch[0])
    ws = None
    for hop in range(sizes.hops):
        ws = sketch_propagate(view, sizes, sketch[hop], sketch[hop + 1], status, ws)
    return sketch, status


def sketch_links(sizes, sketch, src, dst, out=None, status=None):
    """tg_sketch_links over the links (src[i], dst[i]) (int64 [m], device) on the current stream -> dict(match [m, h, h]
    int32, usum [m, h, h] int64 holding the uint64 words (below 2^44), uzero [m, h, h] int32, nsum [m, 2, h], nzero [m, 2, h],
    status [1] int32).  out: the dict of an earlier call with the same shapes, written again."""
    for t in (src, dst):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError("sketch_links: src and dst must be contiguous flat int64 tensors")
    if src.shape != dst.shape or src.device != dst.device:
        raise ValueError("sketch_links: src and dst must have one length and one device")
    h, W = sizes.hops, sizes.row_words
    if (not isinstance(sketch, torch.Tensor) or sketch.dtype != torch.int32 or sketch.dim() != 3 or sketch.shape[0] != h + 1
            or sketch.shape[2] != W or not sketch.is_contiguous()):
        raise ValueError("sketch_links: the sketch must be a contiguous int32 tensor [%d, n, %d]" % (h + 1, W))
    dev, m = src.device, src.numel()
    if out is None:
        i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
        out = dict(match=torch.empty((m, h, h), **i32), usum=torch.empty((m, h, h), **i64), uzero=torch.empty((m, h, h), **i32),
                   nsum=torch.empty((m, 2, h), **i64), nzero=torch.empty((m, 2, h), **i32))
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    so = TgSketchLinkOut(*(out[name].data_ptr() if out[name].numel() else None for name in LINK_OUTPUTS))
    check(lib.tg_sketch_links(C.byref(sizes.params), sketch.shape[1], ptr(sketch), ptr(src) if m else None, ptr(dst) if m else None,
                              C.byref(so), m, ptr(status), stream_ptr(dev)))
    out["status"] = status
    return out


def sketch_status_check(status, who, mask=-1):
    """the status word after its read-back: bit 1 = an id outside the graph, bit 2 = row pointers that contradict n_edges"""
    _status_check(status, who, ((STATUS_RANGE, "an id outside the graph"),
                                (STATUS_GRAPH, "row pointers that contradict n_edges")), mask=mask)


def cardinality(S, Z, m_reg):
    """HyperLogLog's estimate from the integers of tg_sketch_links, float32 elementwise: E = alpha m^2 / (S / 2^33) with
    alpha = 0.7213 / (1 + 1.079 / m), replaced by m ln(m / Z) where E <= 2.5 m and Z > 0.  No large-range correction: index and
    rank come from separate 32-bit words."""
    alpha = 0.7213 / (1.0 + 1.079 / m_reg)
    E = (alpha * m_reg * m_reg) / (S.to(torch.float32) * 2.0 ** -33)
    Zf = Z.to(torch.float32)
    linear = m_reg * (math.log(m_reg) - torch.log(Zf.clamp(min=1.0)))
    return torch.where((E <= 2.5 * m_reg) & (Z > 0), linear, E)


def structure_features(out, n_perm, m_reg):
    """ELPH / BUDDY's structure features from tg_sketch_links' integers -> (structure float32 [L, h (h + 2)], card float32
    [L, 2, h]).  I[a][b] = match / n_perm x card(usum, uzero) estimates |N_a(u) n N_b(v)| (Jaccard x union);
    A[a][b] = I[a][b] - I[a-1][b] - I[a][b-1] + I[a-1][b-1] with I[0][.] = I[.][0] = 0 the vertices at distance exactly (a, b)
    -- the balls are closed, so the ends themselves fall into the a = 1 or b = 1 bins --; B[s][a] = card_s[a] - card_s[a-1] -
    (the sum of A[a][.] over the other end's hops), card_s[0] = 0.  Laid out as A row-major, then B of u, then B of v."""
    L, h = out["match"].shape[0], out["match"].shape[1]
    inter = out["match"].to(torch.float32) / n_perm * cardinality(out["usum"], out["uzero"], m_reg)
    card = cardinality(out["nsum"], out["nzero"], m_reg)
    pad = torch.zeros((L, h + 1, h + 1), dtype=torch.float32, device=inter.device)
    pad[:, 1:, 1:] = inter
    A = pad[:, 1:, 1:] - pad[:, :-1, 1:] - pad[:, 1:, :-1] + pad[:, :-1, :-1]
    ring = card.clone()
    ring[:, :, 1:] -= card[:, :, :-1]
    B = torch.stack([ring[:, 0] - A.sum(2), ring[:, 1] - A.sum(1)], 1)
    return torch.cat([A.reshape(L, h * h), B.reshape(L, 2 * h)], 1), card
