"""ctypes binding of include/tchgeo_lastn.h: the streaming last-k neighbour state (tg_lastn_reset / _insert / _sample /
_replay, csrc/lastn.hip) in the library _cabi.py loads.  A module of its own, as the header is a header of its own; `LastN`
holds the state tensor and launches on the current stream."""
import ctypes as C

import torch

from ._cabi import NsBatchedOut, TG_MAX_HOPS, _status_check, check, lib, ns_rows_unmark, ptr, stream_ptr

EXPORTS = ["tg_lastn_state_bytes", "tg_lastn_reset", "tg_lastn_insert_workspace_bytes", "tg_lastn_insert",
           "tg_lastn_sample", "tg_lastn_replay_workspace_bytes", "tg_lastn_replay"]

LASTN_MAX_K = 64                     # tchgeo_lastn.h
LASTN_MAX_NODES = 1 << 31
LASTN_MAX_EVENTS = 1 << 22
LASTN_LDS_ENTRIES = 4096
FORM_AUTO, FORM_LDS, FORM_GRID = 0, 1, 2


class TgLastN(C.Structure):
    _fields_ = [("state", C.c_void_p), ("state_bytes", C.c_int64), ("n_nodes", C.c_int64), ("k", C.c_int32)]


_P, _I64, _I32 = C.c_void_p, C.c_int64, C.c_int32
lib.tg_lastn_state_bytes.argtypes = [_I64, _I32, _P]
lib.tg_lastn_reset.argtypes = [_P, _P]
lib.tg_lastn_insert_workspace_bytes.argtypes = [_I64, _I32, _I32, _P, _P]
lib.tg_lastn_insert.argtypes = [_P, _P, _P, _P, _I64, _I64, _I32, _P, _P, _I64, _I32, _P]
lib.tg_lastn_sample.argtypes = [_P, _P, _I64, _I64, _P, _I32, _P, _P, _P]
lib.tg_lastn_replay_workspace_bytes.argtypes = [_I64, _P]
lib.tg_lastn_replay.argtypes = [_P, _P, _P, _I64, _I64, _I64, _P, _I64, _P, _I32, _P, _P, _P, _I64, _P]
for _n in EXPORTS:
    getattr(lib, _n).restype = C.c_int


def lastn_state_bytes(n_nodes, k):
    """the bytes of a state of n_nodes rings of k slots (tg_lastn_state_bytes); no device is touched"""
    b = C.c_int64(-1)
    check(lib.tg_lastn_state_bytes(int(n_nodes), int(k), C.byref(b)))
    return b.value


def lastn_insert_workspace_bytes(n_events, symmetric=True, form=FORM_AUTO):
    """-> (bytes, form taken) of an insert of n_events events; 0 bytes where the one-workgroup form is taken"""
    b, f = C.c_int64(-1), C.c_int32(-1)
    check(lib.tg_lastn_insert_workspace_bytes(int(n_events), int(bool(symmetric)), int(form), C.byref(b), C.byref(f)))
    return b.value, f.value


def lastn_replay_workspace_bytes(step_events):
    b = C.c_int64(-1)
    check(lib.tg_lastn_replay_workspace_bytes(int(step_events), C.byref(b)))
    return b.value


def _sizes(who, n_nodes, k):
    n_nodes, k = int(n_nodes), int(k)
    if not 1 <= k <= LASTN_MAX_K:
        raise ValueError("%s: size = %d outside [1, %d]" % (who, k, LASTN_MAX_K))
    if not 1 <= n_nodes <= LASTN_MAX_NODES:
        raise ValueError("%s: num_nodes = %d outside [1, 2^31]" % (who, n_nodes))
    return n_nodes, k


def _fanout(who, fanout, k):
    fanout = [int(f) for f in fanout]
    if len(fanout) > TG_MAX_HOPS:
        raise ValueError("%s: %d hops, at most %d" % (who, len(fanout), TG_MAX_HOPS))
    for f in fanout:
        if not 1 <= f <= k:
            raise ValueError("%s: fan-out %d outside [1, size = %d]" % (who, f, k))
    return fanout


class LastN:
    """The state of tchgeo_lastn.h for n_nodes nodes with rings of k slots: one int64 tensor `state` (its bytes are the
    header's layout: counts, padding, slots), reset at construction, and one int32 status word the launches OR into.
    reset / insert / sample / replay run on the current stream and do not synchronise; status_check() reads the word back."""

    def __init__(self, n_nodes, k, device):
        self.n_nodes, self.k = _sizes("LastN", n_nodes, k)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.state_bytes = lastn_state_bytes(self.n_nodes, self.k)
        self.state = torch.empty(self.state_bytes // 8, dtype=torch.int64, device=self.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.ws = None
        self.reset()

    insert_workspace_bytes = staticmethod(lastn_insert_workspace_bytes)      # the workspace queries, as the module has them
    replay_workspace_bytes = staticmethod(lastn_replay_workspace_bytes)

    def struct(self):
        return TgLastN(self.state.data_ptr(), self.state_bytes, self.n_nodes, self.k)

    def _workspace(self, need):
        if need and (self.ws is None or self.ws.numel() * 8 < need):
            self.ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=self.device)
        return (ptr(self.ws), self.ws.numel() * 8) if need else (None, 0)

    def _ids(self, who, **tensors):
        for name, t in tensors.items():
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or not t.is_contiguous() or t.device != self.device:
                raise ValueError("LastN.%s: %s must be a contiguous int64 tensor on %s" % (who, name, self.device))

    def reset(self):
        """counts = 0, every slot = {-1, -1}, status = 0"""
        st = self.struct()
        check(lib.tg_lastn_reset(C.byref(st), stream_ptr(self.device)))
        self.status.zero_()

    def insert(self, src, dst, e_id=None, e_base=0, symmetric=True, form=FORM_AUTO):
        """appends the events (src[j], dst[j]) with ids e_id[j] (None: e_base + j) to the rings of dst (and of src under
        `symmetric`)"""
        self._ids("insert", src=src, dst=dst, **({} if e_id is None else {"e_id": e_id}))
        n = src.numel()
        if dst.numel() != n or (e_id is not None and e_id.numel() != n):
            raise ValueError("LastN.insert: src, dst and e_id differ in length")
        if n > LASTN_MAX_EVENTS:
            raise ValueError("LastN.insert: %d events, at most 2^22 per call" % n)
        need, _ = lastn_insert_workspace_bytes(n, symmetric, form)
        ws, ws_bytes = self._workspace(need)
        st = self.struct()
        check(lib.tg_lastn_insert(C.byref(st), ptr(src), ptr(dst), ptr(e_id), int(e_base), n, int(bool(symmetric)),
                                  ptr(self.status), ws, ws_bytes, int(form), stream_ptr(self.device)))

    def sample(self, seeds, fanout, out=None):
        """seeds [n_batches, n_seeds] -> an NsBatchedOut (tg_ns_homo_batched's slabs): per seed and hop the newest
        min(fanout[h], entries) entries, newest first"""
        self._ids("sample", seeds=seeds)
        if seeds.dim() != 2:
            raise ValueError("LastN.sample: seeds must be [n_batches, n_seeds]")
        fanout = _fanout("LastN.sample", fanout, self.k)
        if out is None:
            out = NsBatchedOut(seeds.shape[0], seeds.shape[1], fanout, self.device)
        so = self._out_struct(out, seeds.shape[1])
        st = self.struct()
        fan = (C.c_int64 * max(len(fanout), 1))(*fanout)
        check(lib.tg_lastn_sample(C.byref(st), ptr(seeds), seeds.shape[0], seeds.shape[1], fan, len(fanout), C.byref(so),
                                  ptr(self.status), stream_ptr(self.device)))
        return out

    @staticmethod
    def _out_struct(out, n_seeds):
        so = out.struct()
        if so.rows_prefilled != n_seeds + 1:
            so.rows_prefilled = 0
            ns_rows_unmark(out.rows)              # a launch with another n_seeds writes ITS rows into the slab
        return so

    def replay(self, src, dst, seeds, fanout, step_events, e_base=0, out=None):
        """G = ceil(len(src) / step_events) steps in one call: step g samples seeds[g] into batch g of `out`, then inserts
        its events symmetrically with e_id = e_base + index (tg_lastn_replay)"""
        self._ids("replay", src=src, dst=dst, seeds=seeds)
        n, step_events = src.numel(), int(step_events)
        if dst.numel() != n:
            raise ValueError("LastN.replay: src and dst differ in length")
        if step_events < 1:
            raise ValueError("LastN.replay: step_events = %d must be >= 1" % step_events)
        if n > LASTN_MAX_EVENTS:
            raise ValueError("LastN.replay: %d events, at most 2^22 per call" % n)
        G = (n + step_events - 1) // step_events
        if seeds.dim() != 2 or seeds.shape[0] != G:
            raise ValueError("LastN.replay: seeds must be [%d, n_seeds]" % G)
        fanout = _fanout("LastN.replay", fanout, self.k)
        if out is None:
            out = NsBatchedOut(G, seeds.shape[1], fanout, self.device)
        so = self._out_struct(out, seeds.shape[1])
        ws, ws_bytes = self._workspace(lastn_replay_workspace_bytes(min(step_events, LASTN_MAX_EVENTS)))
        st = self.struct()
        fan = (C.c_int64 * max(len(fanout), 1))(*fanout)
        check(lib.tg_lastn_replay(C.byref(st), ptr(src), ptr(dst), int(e_base), n, step_events, ptr(seeds), seeds.shape[1],
                                  fan, len(fanout), C.byref(so), ptr(self.status), ws, ws_bytes, stream_ptr(self.device)))
        return out

    def state_dict(self):
        """a copy of the state: its bytes are a pure function of the insertion history"""
        return {"state": self.state.clone(), "n_nodes": self.n_nodes, "k": self.k}

    def load_state_dict(self, d):
        if int(d["n_nodes"]) != self.n_nodes or int(d["k"]) != self.k or d["state"].numel() != self.state.numel():
            raise ValueError("LastN.load_state_dict: the state is of %d nodes with k = %d, this one of %d with k = %d" %
                             (int(d["n_nodes"]), int(d["k"]), self.n_nodes, self.k))
        self.state.copy_(d["state"])

    def status_check(self, who="LastN"):
        """reads the status word back (one synchronisation), clears it, and raises on a node outside [0, n_nodes)"""
        status = int(self.status.item())
        self.status.zero_()
        _status_check(status, who, ((2, "a node outside [0, num_nodes)"),))
