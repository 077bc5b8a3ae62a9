"""ctypes binding of include/tchgeo_ladies.h: layer-wise importance sampling (tg_ladies_count / tg_ladies_emit,
csrc/ladies.hip) in the library _cabi.py loads.  A module of its own, as the header is a header of its own; the launch
object `Ladies` stands on _cabi.py's count / emit base."""
import ctypes as C

import torch

from ._cabi import TgRng, _CountEmit, _status_check, _two_i64, check, lib, ptr, stream_ptr

EXPORTS = ["tg_ladies_workspace_bytes", "tg_ladies_count", "tg_ladies_emit"]

TG_TAG_LADIES = 18
LADIES_MAX_SAMPLES = 8192            # tchgeo_ladies.h: n_samples
LADIES_MAX_NODES = 1 << 22           # max_nodes
LADIES_MAX_NODE_CAP = 1 << 30        # node_cap
LADIES_MAX_CHUNKS = 1 << 31


class TgLadiesIn(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("node_ptr", C.c_void_p), ("max_nodes", C.c_int64), ("node_cap", C.c_int64),
                ("chunk_cap", C.c_int64), ("n_samples", C.c_int64), ("weights", C.c_void_p), ("call_stride", C.c_int64)]


_P, _I64 = C.c_void_p, C.c_int64
lib.tg_ladies_workspace_bytes.argtypes = [_P, _P, _I64, _I64, _P, _P]
lib.tg_ladies_count.argtypes = [_P, _P, _P, _I64, _I64, _P, _P, _P, _P, _P, _P, _P, _I64, _P]
lib.tg_ladies_emit.argtypes = [_P, _P, _P, _I64, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]
for _f in (lib.tg_ladies_workspace_bytes, lib.tg_ladies_count, lib.tg_ladies_emit):
    _f.restype = C.c_int


def _ladies_sizes(who, graph, id_bound, max_nodes, node_cap, chunk_cap, n_samples, n_batches):
    """the refusals of the pair that need no device, as ValueError"""
    id_bound, max_nodes, node_cap, chunk_cap, n_samples, n_batches = (
        int(x) for x in (id_bound, max_nodes, node_cap, chunk_cap, n_samples, n_batches))
    if not 1 <= n_samples <= LADIES_MAX_SAMPLES:
        raise ValueError("%s: n_samples = %d outside [1, %d]" % (who, n_samples, LADIES_MAX_SAMPLES))
    if not 0 <= max_nodes <= LADIES_MAX_NODES:
        raise ValueError("%s: max_nodes = %d outside [0, 2^22]" % (who, max_nodes))
    if not max_nodes <= node_cap <= LADIES_MAX_NODE_CAP:
        raise ValueError("%s: node_cap = %d outside [max_nodes = %d, 2^30]" % (who, node_cap, max_nodes))
    if chunk_cap > LADIES_MAX_CHUNKS:
        raise ValueError("%s: chunk_cap = %d above 2^31" % (who, chunk_cap))
    if not 0 <= n_batches < 2 ** 31:
        raise ValueError("%s: n_batches = %d outside [0, 2^31)" % (who, n_batches))
    if id_bound < max(1, graph.n_major):
        raise ValueError("%s: id_bound = %d below max(1, n_major = %d)" % (who, id_bound, graph.n_major))
    return id_bound, max_nodes, node_cap, chunk_cap, n_samples, n_batches


def ladies_workspace_bytes(graph, id_bound, max_nodes, node_cap, chunk_cap, n_samples, n_batches):
    """-> (bytes, bytes_min): the pair's workspace for n_batches batches at once (n_batches * bytes_min) and for one batch;
    graph: a tg_graph view (only n_major and n_edges are read).  No device is touched."""
    si = TgLadiesIn(None, None, int(max_nodes), int(node_cap), int(chunk_cap), int(n_samples), None, 0)
    return _two_i64(lib.tg_ladies_workspace_bytes, C.byref(graph), C.byref(si), int(id_bound), int(n_batches))


class Ladies(_CountEmit):
    """The layer-wise pair (tg_ladies_count / tg_ladies_emit) for up to n_batches frontiers of at most max_nodes nodes each
    over `graph` (a CSC view): n_samples draws per batch, a table for node_cap distinct nodes and room for chunk_cap chunks
    per batch (<= 0: the bound of a frontier of distinct nodes); weights: float32 per CSC entry, or None for the
    row-normalised adjacency.  Owns what the passes share: n_nodes, n_edges, n_cand, total, chunks [n_batches each] and
    status [1] in one tensor `state` (a loader reads it back in one copy) and the workspace (`ws`: an int64 tensor of an
    earlier launch, reused when large enough).  count(nodes, node_ptr, seed, call_id) then emit(...) run on the current
    stream over the node_ptr.numel() - 1 lists; batch b draws under call id call_id + b; neither synchronises."""

    def __init__(self, graph, id_bound, max_nodes, node_cap, chunk_cap, n_samples, n_batches, device, weights=None, ws=None):
        (self.id_bound, self.max_nodes, self.node_cap, self.chunk_cap, self.n_samples, self.n_batches) = _ladies_sizes(
            "Ladies", graph, id_bound, max_nodes, node_cap, chunk_cap, n_samples, n_batches)
        self.graph, self.device = graph, torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if weights is not None:
            if (not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or weights.dim() != 1
                    or not weights.is_contiguous() or weights.numel() != graph.n_edges):
                raise ValueError("Ladies: weights must be a contiguous float32 tensor with one entry per CSC entry (%d)" %
                                 graph.n_edges)
            if weights.device != self.device:
                raise ValueError("Ladies: weights is on %s, the launch on %s" % (weights.device, self.device))
        self.weights = weights
        self.struct = TgLadiesIn(None, None, self.max_nodes, self.node_cap, self.chunk_cap, self.n_samples,
                                 weights.data_ptr() if weights is not None and weights.numel() else None, 0)
        need = ladies_workspace_bytes(graph, self.id_bound, self.max_nodes, self.node_cap, self.chunk_cap, self.n_samples,
                                      self.n_batches)[0]
        G = self.n_batches
        self._own(need, ws, self.device, [("n_nodes", G), ("n_edges", G), ("n_cand", G), ("total", G), ("chunks", G)],
                  same_device=True)
        self.rng = TgRng(0, 0)
        self.live = None

    def count(self, nodes, node_ptr, seed, call_id, call_stride=1):
        """pass 1 over the lists nodes[node_ptr[b] : node_ptr[b + 1]] -> (n_nodes, n_edges, n_cand, total, chunks [live
        each], status [1]), device tensors; the caller reads them back.  List b draws under call id call_id + b * call_stride"""
        for name, t in (("nodes", nodes), ("node_ptr", node_ptr)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
                raise ValueError("Ladies.count: %s must be a contiguous flat int64 tensor" % name)
            if t.device != self.device:
                raise ValueError("Ladies.count: %s is on %s, the launch on %s" % (name, t.device, self.device))
        live = node_ptr.numel() - 1
        if not 0 <= live <= self.n_batches:
            raise ValueError("Ladies.count: node_ptr names %d lists, outside [0, %d]" % (live, self.n_batches))
        self.live, self._lists = live, (nodes, node_ptr)
        self.struct.nodes = nodes.data_ptr() if nodes.numel() else None
        self.struct.node_ptr = node_ptr.data_ptr()
        if self.max_nodes and not nodes.numel():
            self.struct.nodes = self.ws.data_ptr()       # never read: every list is empty
        self.rng = TgRng(int(seed) & (2 ** 64 - 1), int(call_id) & (2 ** 64 - 1))
        self.struct.call_stride = int(call_stride)
        self._begin_count()
        check(lib.tg_ladies_count(C.byref(self.graph), C.byref(self.struct), C.byref(self.rng), live, self.id_bound,
                                  ptr(self.n_nodes), ptr(self.n_edges), ptr(self.n_cand), ptr(self.total), ptr(self.chunks),
                                  ptr(self.status), ptr(self.ws), self.ws.numel() * 8, stream_ptr(self.device)))
        return self.n_nodes[:live], self.n_edges[:live], self.n_cand[:live], self.total[:live], self.chunks[:live], self.status

    def emit(self, node_off, edge_off, nodes_out, node_count, node_weight, rows, cols, edge_index, edge_weight):
        """pass 2 into the caller's flat arrays; node_off / edge_off: device [live], the exclusive prefixes of n_nodes /
        n_edges; nodes_out, node_count and node_weight may each be None; edge_weight is float32.  It only reads the
        workspace: it may be repeated after one count()"""
        if self.live is None:
            raise ValueError("Ladies.emit: no counted launch (count() first)")
        per_node = (("nodes_out", nodes_out), ("node_count", node_count), ("node_weight", node_weight))
        any_node = any(t is not None for _, t in per_node)
        for name, t in (("node_off", node_off), ("edge_off", edge_off)) + per_node + (
                ("rows", rows), ("cols", cols), ("edge_index", edge_index)):
            if t is None and (name in ("nodes_out", "node_count", "node_weight") or (name == "node_off" and not any_node)):
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or not t.is_contiguous() or t.device != self.device:
                raise ValueError("Ladies.emit: %s must be a contiguous int64 tensor on %s" % (name, self.device))
        if (not isinstance(edge_weight, torch.Tensor) or edge_weight.dtype != torch.float32 or not edge_weight.is_contiguous()
                or edge_weight.device != self.device):
            raise ValueError("Ladies.emit: edge_weight must be a contiguous float32 tensor on %s" % (self.device,))
        for name, t in (("node_off", node_off), ("edge_off", edge_off)):
            if t is not None and t.numel() < self.live:
                raise ValueError("Ladies.emit: %s is shorter than the %d counted lists" % (name, self.live))
        check(lib.tg_ladies_emit(C.byref(self.graph), C.byref(self.struct), C.byref(self.rng), self.live, self.id_bound,
                                 ptr(node_off), ptr(edge_off), ptr(nodes_out), ptr(node_count), ptr(node_weight), ptr(rows),
                                 ptr(cols), ptr(edge_index), ptr(edge_weight), ptr(self.ws), self.ws.numel() * 8,
                                 stream_ptr(self.device)))


def ladies_status_check(status, who, mask=2):
    """the status word of tg_ladies_count after its read-back: bit 1 raises (bit 0, a refused batch, is the caller's to
    answer with a larger workspace; bit 2, a batch whose candidates all have weight 0 and which therefore keeps no edge,
    raises under mask=6)"""
    _status_check(status, who, ((2, "a frontier node outside the graph"),
                                (4, "a mini-batch whose candidates all have weight 0")), mask=mask)
