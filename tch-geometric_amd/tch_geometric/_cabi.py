"""ctypes binding of the C ABI declared in include/tchgeo.h (libtchgeo_hip.so).

There is no CPU fallback: if the gfx950 library is missing this module raises
at import, and every wrapper raises on a non-zero status code.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TCHGEO_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libtchgeo_hip.so")  # TCHGEO_LIB: A/B builds

TG_OK = 0
TG_MAX_HOPS = 8
TG_MAX_FANOUT = 32
SAMPLER_UNIFORM, SAMPLER_UNIFORM_REPL, SAMPLER_WEIGHTED = 0, 1, 2
SAMPLER_RECENT = 3   # additive: the k most recent admitted edges (tchgeo.h TG_SAMPLER_RECENT); deterministic
PART_REPLY_PACKED, PART_REPLY_PAIRS, PART_REPLY_TRIPLES, PART_REPLY_PACKED_STATE = 1, 2, 3, 4   # tchgeo.h TG_PART_REPLY_*
SAMPLER_LABOR, SAMPLER_LABOR_SHARED = 4, 5   # additive: layer-neighbor sampling (tchgeo.h TG_SAMPLER_LABOR[_SHARED])
LABOR_LONG_COLUMN = 32768   # tchgeo.h TG_LABOR_LONG_COLUMN: longer columns go to the 16-wavefront kernel
FILTER_NONE, FILTER_STATIC, FILTER_RELATIVE, FILTER_DYNAMIC = -1, 0, 1, 2

EXPORTS = ["tg_version", "tg_last_error", "tg_ns_homo_capacity", "tg_ns_homo_batched", "tg_random_walk",
           "tg_edge_set_bytes", "tg_edge_set_build", "tg_random_walk_es",
           "tg_tempo_random_walk", "tg_rmat_edges", "tg_seed_batches", "tg_ind2ptr", "tg_probe_random_gather",
           "tg_neg_workspace_bytes", "tg_neg_sample", "tg_hgt_workspace_bytes", "tg_hgt_sample", "tg_ns_hop_workspace_bytes", "tg_ns_hop", "tg_rmat_edges_rect",
           "tg_coo_to_csx_workspace_bytes", "tg_coo_to_csx", "tg_budget_layer", "tg_check_range",
           "tg_ns_hop_scan_workspace_bytes", "tg_ns_hop_scan", "tg_ns_hop_weighted", "tg_ns_hop_weighted_groups", "tg_ns_hop_weighted_workspace_bytes", "tg_gather_rows",
           "tg_biased_walk_workspace_bytes", "tg_biased_tempo_random_walk", "tg_ns_hetero_capacity",
           "tg_ns_hetero_batched", "tg_ns_homo_compact", "tg_part_workspace_bytes", "tg_part_begin",
           "tg_sanitize_range", "tg_ns_hop_segments", "tg_het_hop_begin_all", "tg_het_hop_end_all", "tg_part_requests", "tg_part_count", "tg_part_scan_workspace_bytes", "tg_part_sample", "tg_part_emit", "tg_part_slot_words", "tg_part_sample_slots", "tg_part_emit_slots", "tg_part_unpack", "tg_part_pack", "tg_compact_rows", "tg_budget_capacity",
           "tg_budget_workspace_bytes", "tg_budget_sample", "tg_ns_homo_workspace_bytes", "tg_ns_homo_batched_ws", "tg_het_meta_words", "tg_het_step_begin",
           "tg_het_step_end", "tg_het_hop_end", "tg_ns_homo_batched_form", "tg_ns_win_tuning_get", "tg_ns_win_tuning_set",
           "tg_ns_win_stage_timing", "tg_ns_win_stage_times", "tg_ns_win_first_lds_bytes", "tg_ns_win_first_launch", "tg_probe_ns_sol",
           "tg_debug_bounds_set_flag", "tg_part_sample_workspace_bytes", "tg_part_sample_ws",
           "tg_part_sample_order_thresholds", "tg_ns_homo_batched_pipeline", "tg_graph_max_degree",
           "tg_ns_homo_workspace_bytes_for", "tg_ns_homo_batched_workspace_bytes", "tg_hgt_batched_capacity",
           "tg_hgt_batched_workspace_bytes", "tg_hgt_sample_batched", "tg_budget_batched_workspace_bytes",
           "tg_budget_sample_batched", "tg_neg_batched_capacity", "tg_neg_batched_form", "tg_neg_batched_workspace_bytes",
           "tg_neg_sample_batched", "tg_ns_homo_unique_form", "tg_ns_homo_unique_workspace_bytes", "tg_ns_homo_unique",
           "tg_ns_typed_unique_form", "tg_ns_typed_unique_workspace_bytes", "tg_ns_typed_unique",
           "tg_ns_induced_workspace_bytes", "tg_ns_induced_count", "tg_ns_induced_emit", "tg_rw_skipgram_capacity",
           "tg_rw_skipgram_form", "tg_rw_skipgram_workspace_bytes", "tg_rw_skipgram", "tg_ns_rows_fill",
           "tg_link_seeds_capacity", "tg_link_seeds", "tg_link_seeds_typed", "tg_mp_skipgram_capacity",
           "tg_mp_skipgram_form", "tg_mp_skipgram_workspace_bytes", "tg_mp_skipgram", "tg_tempo_skipgram_capacity",
           "tg_tempo_skipgram_lds_bytes", "tg_tempo_skipgram", "tg_ns_hop_recent", "tg_ns_homo_unique_grouped_form",
           "tg_ns_homo_unique_grouped_workspace_bytes", "tg_ns_homo_unique_grouped",
           "tg_ns_induced_grouped_workspace_bytes", "tg_ns_induced_grouped_count", "tg_ns_induced_grouped_emit",
           "tg_saint_rw_capacity", "tg_saint_rw_form", "tg_saint_rw_workspace_bytes", "tg_saint_rw_nodes",
           "tg_saint_coverage_add", "tg_saint_norm", "tg_ns_hop_labor_workspace_bytes", "tg_ns_hop_labor",
           "tg_ns_hop_labor_long_column", "tg_pinsage_hop_workspace_bytes", "tg_pinsage_hop",
           "tg_cluster_workspace_bytes", "tg_cluster_count", "tg_cluster_emit",
           "tg_ns_full_workspace_bytes", "tg_ns_full_count", "tg_ns_full_emit",
           "tg_saint_ne_form", "tg_saint_ne_workspace_bytes", "tg_saint_node_nodes", "tg_saint_edge_nodes"]


class TgGraph(C.Structure):
    _fields_ = [("ptrs", C.c_void_p), ("indices", C.c_void_p), ("weights", C.c_void_p), ("timestamps", C.c_void_p),
                ("n_major", C.c_int64), ("n_edges", C.c_int64), ("indices32", C.c_void_p), ("ptrs32", C.c_void_p),
                ("max_degree", C.c_int64)]


class TgRng(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("call_id", C.c_uint64)]


class TgNsConfig(C.Structure):
    _fields_ = [("sampler", C.c_int32), ("filter_mode", C.c_int32), ("forward", C.c_int32), ("rng_tag", C.c_uint32),
                ("win_lo", C.c_int64), ("win_hi", C.c_int64), ("seeds_state", C.c_void_p), ("id_base", C.c_int64),
                ("seed_ids", C.c_void_p), ("seed_call_ids", C.c_void_p)]


class TgNsOut(C.Structure):
    _fields_ = [("samples", C.c_void_p), ("rows", C.c_void_p), ("cols", C.c_void_p), ("edge_index", C.c_void_p),
                ("layer_offsets", C.c_void_p), ("counts", C.c_void_p), ("states", C.c_void_p),
                ("cap_nodes", C.c_int64), ("cap_edges", C.c_int64), ("rows_prefilled", C.c_int64)]


if not os.path.exists(LIB_PATH):
    raise ImportError("tch_geometric: %s is missing -- build it with `make -C tch-geometric_amd` "
                      "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
lib = C.CDLL(LIB_PATH)
lib.tg_version.restype = C.c_char_p
lib.tg_last_error.restype = C.c_char_p


class TgHopIn(C.Structure):
    _fields_ = [("vertices", C.c_void_p), ("ids", C.c_void_p), ("call_ids", C.c_void_p), ("m", C.c_int64),
                ("id_base", C.c_int64), ("fanout", C.c_int32), ("sampler", C.c_int32), ("rng_tag", C.c_uint32),
                ("_reserved", C.c_uint32)]


class TgHopOut(C.Structure):
    _fields_ = [("cnt", C.c_void_p), ("offsets", C.c_void_p), ("neighbors", C.c_void_p), ("edge_ptrs", C.c_void_p),
                ("parents", C.c_void_p)]


class TgHopSegment(C.Structure):
    _fields_ = [("graph", C.c_void_p), ("begin", C.c_int64), ("fanout", C.c_int32), ("rng_tag", C.c_uint32)]


class TgHopFilter(C.Structure):
    _fields_ = [("filter_mode", C.c_int32), ("forward", C.c_int32), ("win_lo", C.c_int64), ("win_hi", C.c_int64),
                ("states", C.c_void_p)]


class TchGeoError(RuntimeError):
    pass


def check(rc):
    if rc != TG_OK:
        raise TchGeoError("tchgeo error %d: %s" % (rc, lib.tg_last_error().decode()))


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _two_i64(fn, *args):
    """fn(*args, &a, &b) -> (a, b): the two int64 out-params of a size query (bytes, bytes_min)"""
    a, b = C.c_int64(-1), C.c_int64(-1)
    check(fn(*args, C.byref(a), C.byref(b)))
    return a.value, b.value


def _host_prefix(counts):
    """the exclusive prefix of host counts with the total behind it, as a python list"""
    off = [0]
    for m in counts:
        off.append(off[-1] + int(m))
    return off


def _status_check(status, who, bits, mask=-1):
    """raises where the status word of a count pass has a bit of `mask`, naming every raised bit of the table `bits`"""
    if status & mask:
        raise RuntimeError("%s: status %d (%s)" % (who, status, " and ".join(t for bit, t in bits if status & bit)))


class _CountEmit:
    """What the count / emit launch objects share: the workspace `ws` (an int64 tensor of an earlier launch, reused when
    large enough), one int64 tensor `state` carved into the named fields with the status word behind them (a loader reads
    everything back in one copy), and the zeroing of that word before pass 1."""

    def _own(self, need, ws, device, fields, same_device=False):
        if ws is None or ws.numel() * 8 < need or (same_device and ws.device != device):
            ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=device)
        self.ws = ws
        self.state = torch.zeros(sum(words for _, words in fields) + 1, dtype=torch.int64, device=device)
        o = 0
        for name, words in fields:
            setattr(self, name, self.state[o:o + words])
            o += words
        self.status = self.state[-1:].view(torch.int32)[:1]

    def _begin_count(self):
        self.state[-1:].zero_()

    def _ws_args(self):
        return ptr(self.ws), C.c_int64(self.ws.numel() * 8)


def graph_max_degree(g, device):
    """The longest column (row) of a graph view, computed on the device (tg_graph_max_degree); one read-back."""
    out = torch.zeros(1, dtype=torch.int64, device=device)
    check(lib.tg_graph_max_degree(C.byref(g), ptr(out), stream_ptr(device)))
    return int(out.item())


def graph_view(ptrs, indices, weights=None, timestamps=None, indices32=None, ptrs32=None, max_degree=None):
    """max_degree: None = unknown (0 in the struct: the window-ordered launch then assumes n_edges), "auto" = computed on the
    device here (one read-back, once per view), or the caller's number."""
    g = TgGraph()
    g.ptrs, g.indices = ptrs.data_ptr(), indices.data_ptr()
    g.weights = weights.data_ptr() if weights is not None else None
    g.timestamps = timestamps.data_ptr() if timestamps is not None else None
    g.n_major, g.n_edges = ptrs.numel() - 1, indices.numel()
    g.indices32 = indices32.data_ptr() if indices32 is not None else None
    g.ptrs32 = ptrs32.data_ptr() if ptrs32 is not None else None
    g._keep = (ptrs, indices, weights, timestamps, indices32, ptrs32)  # the struct only borrows the device memory
    g.max_degree = 0
    if max_degree == "auto":
        g.max_degree = graph_max_degree(g, ptrs.device) if ptrs.is_cuda else int((ptrs[1:] - ptrs[:-1]).max()) if ptrs.numel() > 1 else 0
    elif max_degree is not None:
        g.max_degree = int(max_degree)
    return g


def graph_sizing(n_major, n_edges, max_degree=0):
    """A tg_graph that carries only sizes (no arrays): enough for ns_homo_workspace(graph=...) before the graph exists."""
    g = TgGraph()
    g.n_major, g.n_edges, g.max_degree = int(n_major), int(n_edges), int(max_degree)
    return g


def _rel_arrays(rels, timestamps=False):
    """rels (src type index, dst type index, ptrs, indices, ...) -> the (rel_src, rel_dst, graphs) arrays of a typed
    problem.  timestamps: r[4] holds the relation's row timestamps or None (the hgt and budget problems; elsewhere r[4]
    means something else)."""
    R = len(rels)
    rel_src = (C.c_int32 * max(R, 1))(*[r[0] for r in rels])
    rel_dst = (C.c_int32 * max(R, 1))(*[r[1] for r in rels])
    graphs = (TgGraph * max(R, 1))()
    for i, r in enumerate(rels):
        graphs[i] = graph_view(r[2], r[3], timestamps=r[4] if timestamps and len(r) > 4 else None)
    return rel_src, rel_dst, graphs


def _vp(tensors):
    """One pointer per tensor (per node type, or per slab), null for None and for a tensor without elements."""
    return (C.c_void_p * max(len(tensors), 1))(*[None if x is None or x.numel() == 0 else x.data_ptr() for x in tensors])


def _i64(xs):
    return (C.c_int64 * max(len(xs), 1))(*[int(x) for x in xs])


def ns_homo_capacity(n_seeds, fanout):
    cn, ce = C.c_int64(0), C.c_int64(0)
    fan = (C.c_int64 * max(len(fanout), 1))(*fanout)
    check(lib.tg_ns_homo_capacity(C.c_int64(n_seeds), fan, C.c_int32(len(fanout)), C.byref(cn), C.byref(ce)))
    return cn.value, ce.value


_ROWS_MARK = "_tg_rows_prefilled"   # on a `rows` TENSOR: (n_seeds it was filled for, its _version at that moment)


def ns_rows_fill(rows, n_seeds):
    """rows[b, e] = n_seeds + e over the whole slab (tg_ns_rows_fill, current stream), and the mark on the tensor object that
    lets NsBatchedOut.struct() state tg_ns_out.rows_prefilled: launches with this n_seeds then leave the slab alone.  The
    mark is on the tensor, not on who holds it: an output object assembled from another's slabs keeps it, a view has none."""
    assert rows.dtype == torch.int64 and rows.dim() == 2 and rows.is_contiguous()
    check(lib.tg_ns_rows_fill(ptr(rows), C.c_int64(rows.shape[0]), C.c_int64(rows.shape[1]), C.c_int64(n_seeds),
                              stream_ptr(rows.device)))
    try:
        setattr(rows, _ROWS_MARK, (int(n_seeds), rows._version))
    except RuntimeError:                      # an inference tensor keeps no version: filled, but nothing is stated about it
        setattr(rows, _ROWS_MARK, None)


def ns_rows_unmark(rows):
    """Called by whoever writes a `rows` slab through its raw pointer with anything but n_seeds + e (in-place torch writes
    need not: they bump the tensor's _version, which ends the mark by itself)."""
    if getattr(rows, _ROWS_MARK, None) is not None:
        setattr(rows, _ROWS_MARK, None)


def _rows_prefilled(rows, n_seeds):
    """The value of tg_ns_out.rows_prefilled for this tensor and n_seeds: n_seeds + 1 while the mark holds, else 0."""
    mark = getattr(rows, _ROWS_MARK, None)
    if mark is None or n_seeds is None:
        return 0
    try:
        version = rows._version
    except RuntimeError:                      # inference tensors keep no version: nothing can be stated about them
        return 0
    return n_seeds + 1 if mark == (n_seeds, version) else 0


class NsBatchedOut:
    """Per-batch output slabs (device) of tg_ns_homo_batched.  `rows` is filled once, here (rows[b, e] = n_seeds + e whatever
    is sampled), and marked; struct() then sets tg_ns_out.rows_prefilled and the plain launches skip that stream."""

    def __init__(self, n_batches, n_seeds, fanout, device, with_states=False):
        self.n_batches, self.n_seeds, self.n_hops = n_batches, n_seeds, len(fanout)
        self.cap_nodes, self.cap_edges = ns_homo_capacity(n_seeds, fanout)
        o = dict(dtype=torch.int64, device=device)
        self.samples = torch.empty((n_batches, max(self.cap_nodes, 1)), **o)
        self.rows = torch.empty((n_batches, max(self.cap_edges, 1)), **o)
        self.cols = torch.empty((n_batches, max(self.cap_edges, 1)), **o)
        self.edge_index = torch.empty((n_batches, max(self.cap_edges, 1)), **o)
        self.layer_offsets = torch.zeros((n_batches, max(self.n_hops, 1), 3), **o)
        self.counts = torch.zeros((n_batches, 2), **o)
        self.states = torch.empty((n_batches, max(self.cap_nodes, 1)), **o) if with_states else None
        if self.rows.is_cuda:
            ns_rows_fill(self.rows, n_seeds)

    def struct(self):
        s = TgNsOut()
        s.samples, s.rows, s.cols = self.samples.data_ptr(), self.rows.data_ptr(), self.cols.data_ptr()
        s.edge_index, s.layer_offsets = self.edge_index.data_ptr(), self.layer_offsets.data_ptr()
        s.counts = self.counts.data_ptr()
        s.states = self.states.data_ptr() if self.states is not None else None
        s.cap_nodes, s.cap_edges = self.samples.shape[1], self.rows.shape[1]
        s.rows_prefilled = _rows_prefilled(self.rows, getattr(self, "n_seeds", None))
        return s

    def batch(self, b, counts=None):
        """-> (samples, rows, cols, edge_index, layer_offsets) of batch b, trimmed (host sync)."""
        c = (counts if counts is not None else self.counts.cpu())[b]
        ns, ne = int(c[0]), int(c[1])
        lo = [tuple(int(x) for x in row) for row in self.layer_offsets[b, :self.n_hops].cpu()]
        return self.samples[b, :ns], self.rows[b, :ne], self.cols[b, :ne], self.edge_index[b, :ne], lo


def ns_homo_workspace(n_batches, n_seeds, fanout, device, staged=None, graph=None):
    """Workspace of tg_ns_homo_batched_ws (the window-ordered gather of many-batch launches), as an int64 tensor.
    staged: True = sized for the staged pipeline too (its stage slots), False = push pipeline only, None = as the current
    tuning says.  graph: size the stage slots for this graph's bit widths (else the larger, graph-free size)."""
    nbytes = C.c_int64(0)
    fan = (C.c_int64 * max(len(fanout), 1))(*fanout)
    prev = ns_win_tuning_set(staged=int(staged)) if staged is not None else None
    try:
        check(lib.tg_ns_homo_workspace_bytes_for(C.byref(graph) if graph is not None else None, C.c_int64(n_batches),
                                                 C.c_int64(n_seeds), fan, C.c_int32(len(fanout)), C.byref(nbytes)))
    finally:
        if prev is not None:
            ns_win_tuning_set(staged=prev["staged"])
    return torch.empty(nbytes.value // 8 + 1, dtype=torch.int64, device=device)


def ns_homo_batched_workspace(graph, n_batches, n_seeds, fanout, device, sampler=SAMPLER_UNIFORM, filter_mode=FILTER_NONE):
    """The workspace tg_ns_homo_batched_ws wants for THIS configuration (tg_ns_homo_batched_workspace_bytes): the
    window-ordered form's for the plain samplers, the flat path's for few filtered / weighted batches; None when the launch
    takes none."""
    cfg = TgNsConfig()
    cfg.sampler, cfg.filter_mode = sampler, filter_mode
    nbytes = C.c_int64(0)
    fan = (C.c_int64 * max(len(fanout), 1))(*fanout)
    check(lib.tg_ns_homo_batched_workspace_bytes(C.byref(graph), C.c_int64(n_batches), C.c_int64(n_seeds), fan,
                                                 C.c_int32(len(fanout)), C.byref(cfg), C.byref(nbytes)))
    return torch.empty(nbytes.value // 8 + 1, dtype=torch.int64, device=device) if nbytes.value > 0 else None


def ns_homo_batched(graph, seeds, fanout, seed, call_id, out, sampler=SAMPLER_UNIFORM, filter_mode=FILTER_NONE,
                    forward=False, window=(0, 0), seeds_state=None, rng_tag=0, id_base=0, seed_ids=None,
                    seed_call_ids=None, ws=None, form=0):
    """seeds: [n_batches, n_seeds] int64 on the graph's device; `out` an NsBatchedOut; `ws` (ns_homo_workspace) lets a
    many-batch launch take the window-ordered form (same outputs); form: 0 auto, 1 windowed when applicable, 2 fused."""
    assert seeds.dtype == torch.int64 and seeds.is_contiguous() and seeds.dim() == 2
    cfg = TgNsConfig()
    cfg.sampler, cfg.filter_mode, cfg.forward = sampler, filter_mode, int(bool(forward))
    cfg.win_lo, cfg.win_hi = window
    cfg.seeds_state = seeds_state.data_ptr() if seeds_state is not None else None
    cfg.rng_tag, cfg.id_base = rng_tag, id_base
    cfg.seed_ids = seed_ids.data_ptr() if seed_ids is not None else None
    cfg.seed_call_ids = seed_call_ids.data_ptr() if seed_call_ids is not None else None
    rng = TgRng(seed, call_id)
    fan = (C.c_int64 * max(len(fanout), 1))(*fanout)
    so = out.struct()
    mark = getattr(out.rows, _ROWS_MARK, None)
    if mark is not None and mark[0] != seeds.shape[1]:
        ns_rows_unmark(out.rows)              # a launch with another n_seeds writes ITS rows (n_seeds + e) into the slab
    if ws is not None:
        check(lib.tg_ns_homo_batched_ws(C.byref(graph), ptr(seeds), C.c_int64(seeds.shape[0]),
                                        C.c_int64(seeds.shape[1]), fan, C.c_int32(len(fanout)), C.byref(cfg),
                                        C.byref(rng), C.byref(so), ptr(ws), C.c_int64(ws.numel() * 8), C.c_int32(form),
                                        stream_ptr(seeds.device)))
        return out
    check(lib.tg_ns_homo_batched(C.byref(graph), ptr(seeds), C.c_int64(seeds.shape[0]), C.c_int64(seeds.shape[1]),
                                 fan, C.c_int32(len(fanout)), C.byref(cfg), C.byref(rng), C.byref(so),
                                 stream_ptr(seeds.device)))
    return out


def ns_homo_batched_form(graph, out, n_batches, n_seeds, fanout, ws=None, form=0, sampler=SAMPLER_UNIFORM,
                         filter_mode=FILTER_NONE):
    """Which form ns_homo_batched(..., ws=ws, form=form) runs -> (form taken: 1 windowed / 2 fused / 3 windowed with wide
    items, number of windows).  A query: nothing is launched."""
    cfg = TgNsConfig()
    cfg.sampler, cfg.filter_mode = sampler, filter_mode
    fan = (C.c_int64 * max(len(fanout), 1))(*fanout)
    so = out.struct()
    taken, n_win = C.c_int32(0), C.c_int32(0)
    check(lib.tg_ns_homo_batched_form(C.byref(graph), C.c_int64(n_batches), C.c_int64(n_seeds), fan,
                                      C.c_int32(len(fanout)), C.byref(cfg), C.byref(so),
                                      C.c_int64(ws.numel() * 8 if ws is not None else 0), C.c_int32(form),
                                      C.byref(taken), C.byref(n_win)))
    return taken.value, n_win.value


def ns_homo_batched_staged(graph, out, n_batches, n_seeds, fanout, ws=None, form=0, sampler=SAMPLER_UNIFORM):
    """True if ns_homo_batched(..., ws=ws, form=form) would take the STAGED pipeline of the window-ordered form under the
    current tuning (it needs the workspace sized while `staged` was on: ns_homo_workspace(..., staged=True))."""
    cfg = TgNsConfig()
    cfg.sampler, cfg.filter_mode = sampler, FILTER_NONE
    fan = (C.c_int64 * max(len(fanout), 1))(*fanout)
    so = out.struct()
    st = C.c_int32(0)
    check(lib.tg_ns_homo_batched_pipeline(C.byref(graph), C.c_int64(n_batches), C.c_int64(n_seeds), fan,
                                          C.c_int32(len(fanout)), C.byref(cfg), C.byref(so),
                                          C.c_int64(ws.numel() * 8 if ws is not None else 0), C.c_int32(form), C.byref(st)))
    return bool(st.value)


class TgNsWinTuning(C.Structure):
    _fields_ = [("window_bytes", C.c_int64), ("gather_blocks", C.c_int32), ("gather_threads", C.c_int32),
                ("emit_threads", C.c_int32), ("direct_hop0", C.c_int32), ("fuse_first_hops", C.c_int32),
                ("fold_hist", C.c_int32), ("emit_blocks", C.c_int32), ("staged", C.c_int32),
                ("stage_round_chunks", C.c_int32), ("stage_gather_threads", C.c_int32), ("stage_gather_blocks", C.c_int32),
                ("stage_emit_threads", C.c_int32), ("stage_parts", C.c_int32),
                ("stage_part_min_batches", C.c_int32), ("stage_sort_blocks", C.c_int32), ("stage_fine", C.c_int32),
                ("stage_concurrent", C.c_int32), ("stage_split", C.c_int32),
                ("stage_split_round_chunks", C.c_int32), ("store_align64", C.c_int32),
                ("stage_fine_sub_bits", C.c_int32),
                ("stage_fine_blocks", C.c_int32)]


def ns_win_tuning():
    t = TgNsWinTuning()
    check(lib.tg_ns_win_tuning_get(C.byref(t)))
    return {k: getattr(t, k) for k, _ in TgNsWinTuning._fields_}


def ns_win_tuning_set(**kw):
    """Process-wide tuning of the window-ordered launch (outputs never depend on it); -> the previous values."""
    before = ns_win_tuning()
    t = TgNsWinTuning(0, 0, 0, 0, -1, -1, -1, 0, -1, 0, 0, 0, 0, 0, 0, 0, -1, -1, -1, 0, -1, 0, 0)
    for k, v in kw.items():
        assert k in before, k
        setattr(t, k, int(v))
    check(lib.tg_ns_win_tuning_set(C.byref(t)))
    return before


STAGE_SORT_BLOCKS_AUTO = -1   # ns_win_tuning_set(stage_sort_blocks=...): as many persistent workgroups as stay resident (the default)


def ns_win_first_lds_bytes(emit_threads, kmax, n_coarse_buckets, n_windows, narrow):
    """-> (workgroup size, dynamic LDS bytes) of the staged pipeline's first kernel for these shapes; pure arithmetic."""
    th, nbytes = C.c_int32(0), C.c_int64(0)
    check(lib.tg_ns_win_first_lds_bytes(C.c_int32(emit_threads), C.c_int32(kmax), C.c_int32(n_coarse_buckets),
                                        C.c_int32(n_windows), C.c_int32(int(bool(narrow))), C.byref(th), C.byref(nbytes)))
    return th.value, nbytes.value


def ns_win_first_launch():
    """What the last staged launch gave its first kernel: dict(rows, workgroups_per_cu (0 when stage_sort_blocks was forced),
    threads, narrow, lds_bytes)."""
    r, w, th, nw, nbytes = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int64(0)
    check(lib.tg_ns_win_first_launch(C.byref(r), C.byref(w), C.byref(th), C.byref(nw), C.byref(nbytes)))
    return dict(rows=r.value, workgroups_per_cu=w.value, threads=th.value, narrow=bool(nw.value), lds_bytes=nbytes.value)


def ns_win_stage_timing(enable):
    check(lib.tg_ns_win_stage_timing(C.c_int32(int(bool(enable)))))


def ns_win_stage_times():
    """Stage durations (ms) of the last window-ordered launch recorded under ns_win_stage_timing(True); waits for it."""
    cap = 80
    ms, names, n = (C.c_float * cap)(), C.create_string_buffer(24 * cap), C.c_int32(0)
    check(lib.tg_ns_win_stage_times(ms, names, C.c_int32(cap), C.byref(n)))
    return [(names.raw[24 * i:24 * i + 24].split(b"\0", 1)[0].decode(), float(ms[i])) for i in range(min(n.value, cap))]


def edge_set(graph, device):
    """hash set of the CSR's edges for tg_random_walk_es (has_edge as one probe): a uint64 tensor"""
    nbytes = C.c_int64(0)
    check(lib.tg_edge_set_bytes(C.byref(graph), C.byref(nbytes)))
    es = torch.empty(nbytes.value // 8, dtype=torch.int64, device=device)
    check(lib.tg_edge_set_build(C.byref(graph), ptr(es), nbytes, stream_ptr(device)))
    return es


def random_walk(graph, start, walk_length, p, q, seed, call_id, edge_set=None):
    walks = torch.empty((start.numel(), walk_length + 1), dtype=torch.int64, device=start.device)
    rng = TgRng(seed, call_id)
    if edge_set is None:
        check(lib.tg_random_walk(C.byref(graph), ptr(start), C.c_int64(start.numel()), C.c_int64(walk_length),
                                 C.c_float(p), C.c_float(q), C.byref(rng), ptr(walks), stream_ptr(start.device)))
    else:
        check(lib.tg_random_walk_es(C.byref(graph), ptr(edge_set), C.c_int64(edge_set.numel() * 8), ptr(start),
                                    C.c_int64(start.numel()), C.c_int64(walk_length), C.c_float(p), C.c_float(q),
                                    C.byref(rng), ptr(walks), stream_ptr(start.device)))
    return walks


class TgRwSkipgramConfig(C.Structure):
    _fields_ = [("walk_length", C.c_int64), ("context_size", C.c_int64), ("walks_per_node", C.c_int64),
                ("num_negative_samples", C.c_int64), ("n_nodes", C.c_int64), ("p", C.c_float), ("q", C.c_float)]


class TgRwSkipgramOut(C.Structure):
    _fields_ = [("pos_rw", C.c_void_p), ("neg_rw", C.c_void_p)]


RW_SKIPGRAM_AUTO, RW_SKIPGRAM_LDS32, RW_SKIPGRAM_LDS64, RW_SKIPGRAM_FLAT = 0, 1, 2, 3   # tg_rw_skipgram's `form`


def rw_skipgram_config(walk_length, context_size, walks_per_node=1, num_negative_samples=1, n_nodes=0, p=1.0, q=1.0):
    return TgRwSkipgramConfig(int(walk_length), int(context_size), int(walks_per_node), int(num_negative_samples),
                              int(n_nodes), float(p), float(q))


def rw_skipgram_capacity(cfg, batch_size):
    """-> (rows of pos_rw, rows of neg_rw) per mini-batch of batch_size seeds: nw * R * B and nw * R * K * B."""
    pos, neg = C.c_int64(-1), C.c_int64(-1)
    check(lib.tg_rw_skipgram_capacity(C.byref(cfg), C.c_int64(batch_size), C.byref(pos), C.byref(neg)))
    return pos.value, neg.value


def rw_skipgram_form(cfg, id_bound, lds_limit_bytes=0):
    """-> (form, lds_bytes): the form an auto tg_rw_skipgram call takes for ids in [0, id_bound) (1 = rows staged in LDS as
    uint32, 2 = as int64, 3 = flat through a workspace) and the LDS a workgroup of the LDS form asks for.  lds_limit_bytes
    > 0 replaces the library's limit.  No device is touched."""
    form, nbytes = C.c_int32(-1), C.c_int64(0)
    check(lib.tg_rw_skipgram_form(C.byref(cfg), C.c_int64(id_bound), C.c_int64(lds_limit_bytes), C.byref(form),
                                  C.byref(nbytes)))
    return form.value, nbytes.value


def rw_skipgram_workspace_bytes(cfg, n_batches, batch_size, id_bound, form=0):
    """The workspace a launch of n_batches x batch_size seeds needs in this form (0: the one auto takes): 0 for the LDS
    forms, the [G * W, L] int64 walks for the flat form."""
    nbytes = C.c_int64(-1)
    check(lib.tg_rw_skipgram_workspace_bytes(C.byref(cfg), C.c_int64(n_batches), C.c_int64(batch_size), C.c_int64(id_bound),
                                             C.c_int32(form), C.byref(nbytes)))
    return nbytes.value


def rw_skipgram(graph, seeds, walk_length, context_size, walks_per_node, num_negative_samples, p, q, seed, call_id, n_nodes,
                edge_set=None, form=0, ws=None, out=None):
    """Node2Vec skip-gram batches (tg_rw_skipgram) of the G mini-batches seeds[G, B] in one launch on the current stream:
    -> (pos_rw [G, nw * R * B, C], neg_rw [G, nw * R * K * B, C]); mini-batch g draws with call id call_id + g and is a
    free view.  Dead ends keep their -1 padding: mask with (pos_rw >= 0).all(-1).  form: 0 auto, 1 / 2 LDS (uint32 /
    int64 staging), 3 flat; ws: the flat form's workspace, allocated here when needed and not given; out: (pos_rw,
    neg_rw) of an earlier call of the same shape, reused."""
    if seeds.dim() != 2 or seeds.dtype != torch.int64 or not seeds.is_contiguous():
        raise ValueError("rw_skipgram: seeds must be a contiguous int64 [n_batches, batch_size] tensor")
    G, B = seeds.shape
    cfg = rw_skipgram_config(walk_length, context_size, walks_per_node, num_negative_samples, n_nodes, p, q)
    pos_rows, neg_rows = rw_skipgram_capacity(cfg, B)
    dev = seeds.device
    if out is None:
        out = (torch.empty((G, pos_rows, cfg.context_size), dtype=torch.int64, device=dev),
               torch.empty((G, neg_rows, cfg.context_size), dtype=torch.int64, device=dev))
    pos, neg = out
    if tuple(pos.shape) != (G, pos_rows, cfg.context_size) or tuple(neg.shape) != (G, neg_rows, cfg.context_size) \
            or not (pos.is_contiguous() and neg.is_contiguous()):
        raise ValueError("rw_skipgram: out does not have this launch's shapes")
    need = rw_skipgram_workspace_bytes(cfg, G, B, max(graph.n_major, cfg.n_nodes), form)
    if need and (ws is None or ws.numel() * ws.element_size() < need):
        ws = torch.empty(need // 8, dtype=torch.int64, device=dev)
    o = TgRwSkipgramOut(pos.data_ptr() if pos.numel() else None, neg.data_ptr() if neg.numel() else None)
    rng = TgRng(seed, call_id)
    check(lib.tg_rw_skipgram(C.byref(graph), ptr(edge_set), C.c_int64(edge_set.numel() * 8 if edge_set is not None else 0),
                             ptr(seeds), C.c_int64(G), C.c_int64(B), C.byref(cfg), C.byref(rng), C.byref(o),
                             ptr(ws) if need else C.c_void_p(0), C.c_int64(ws.numel() * ws.element_size() if need else 0),
                             C.c_int32(form), stream_ptr(dev)))
    return pos, neg


TG_MP_MAX_STEPS = 16


class TgMpSkipgramConfig(C.Structure):
    _fields_ = [("n_types", C.c_int32), ("n_steps", C.c_int32), ("graphs", C.POINTER(TgGraph)),
                ("step_src", C.POINTER(C.c_int32)), ("step_dst", C.POINTER(C.c_int32)),
                ("type_count", C.POINTER(C.c_int64)), ("type_start", C.POINTER(C.c_int64)), ("walk_length", C.c_int64),
                ("context_size", C.c_int64), ("walks_per_node", C.c_int64), ("num_negative_samples", C.c_int64),
                ("pad_value", C.c_int64)]


def mp_skipgram_lds_bytes(L, word_bytes):
    """tchgeo.h TG_MP_SKIPGRAM_LDS_BYTES: 64 rows at the odd pitch, the 64 per-walker offsets, the L column starts."""
    return 64 * (L | 1) * word_bytes + 512 + 8 * L


def mp_skipgram_config(graphs, step_src, step_dst, type_count, walk_length, context_size, walks_per_node=1,
                       num_negative_samples=1, type_start=None, pad_value=-1):
    """The tg_mp_skipgram_config of a metapath: graphs[m] is the tg_graph (graph_view / graph_sizing) of the CSR of step m,
    step_src / step_dst its node-type indices, type_count the nodes per type, type_start the offset added to every id of a
    type on output (None: local ids), pad_value what an ended walk is padded with.  The struct borrows the views."""
    M, n_types = len(graphs), len(type_count)
    if not (len(step_src) == len(step_dst) == M) or (type_start is not None and len(type_start) != n_types):
        raise ValueError("mp_skipgram_config: graphs, step_src and step_dst are per step, type_count and type_start per type")
    arrays = ((TgGraph * max(M, 1))(), (C.c_int32 * max(M, 1))(*[int(x) for x in step_src]),
              (C.c_int32 * max(M, 1))(*[int(x) for x in step_dst]), (C.c_int64 * max(n_types, 1))(*[int(x) for x in type_count]),
              (C.c_int64 * n_types)(*[int(x) for x in type_start]) if type_start is not None else None)
    for m, g in enumerate(graphs):
        C.memmove(C.byref(arrays[0], m * C.sizeof(TgGraph)), C.byref(g), C.sizeof(TgGraph))
    cfg = TgMpSkipgramConfig(n_types, M, arrays[0], arrays[1], arrays[2], arrays[3], arrays[4], int(walk_length),
                             int(context_size), int(walks_per_node), int(num_negative_samples), int(pad_value))
    cfg._keep = (arrays, list(graphs))                                # the struct only borrows them
    return cfg


def mp_skipgram_capacity(cfg, batch_size):
    """-> (rows of pos_rw, rows of neg_rw) per mini-batch of batch_size seeds: nw * R * B and nw * R * K * B."""
    pos, neg = C.c_int64(-1), C.c_int64(-1)
    check(lib.tg_mp_skipgram_capacity(C.byref(cfg), C.c_int64(batch_size), C.byref(pos), C.byref(neg)))
    return pos.value, neg.value


def mp_skipgram_form(cfg, lds_limit_bytes=0):
    """-> (form, lds_bytes): the form an auto tg_mp_skipgram call takes (1 = rows staged in LDS as uint32 local ids, needs
    max(type_count) < 2^32 - 1; 2 = as int64; 3 = flat through a workspace) and the LDS a workgroup of the LDS form asks
    for.  lds_limit_bytes > 0 replaces the library's limit.  No device is touched."""
    form, nbytes = C.c_int32(-1), C.c_int64(0)
    check(lib.tg_mp_skipgram_form(C.byref(cfg), C.c_int64(lds_limit_bytes), C.byref(form), C.byref(nbytes)))
    return form.value, nbytes.value


def mp_skipgram_workspace_bytes(cfg, n_batches, batch_size, form=0):
    """The workspace a launch of n_batches x batch_size seeds needs in this form (0: the one auto takes): 0 for the LDS
    forms, the [G * W, L] int64 walks for the flat form."""
    nbytes = C.c_int64(-1)
    check(lib.tg_mp_skipgram_workspace_bytes(C.byref(cfg), C.c_int64(n_batches), C.c_int64(batch_size), C.c_int32(form),
                                             C.byref(nbytes)))
    return nbytes.value


def mp_skipgram(cfg, seeds, seed, call_id, form=0, ws=None, out=None):
    """MetaPath2Vec skip-gram batches (tg_mp_skipgram) of the G mini-batches seeds[G, B] (local ids of the metapath's first
    node type) in one launch on the current stream: -> (pos_rw [G, nw * R * B, C], neg_rw [G, nw * R * K * B, C]);
    mini-batch g draws with call id call_id + g and is a free view.  Every word is a local id plus its column type's
    start; the columns behind an ended walk hold cfg.pad_value.  form, ws, out as rw_skipgram."""
    if seeds.dim() != 2 or seeds.dtype != torch.int64 or not seeds.is_contiguous():
        raise ValueError("mp_skipgram: seeds must be a contiguous int64 [n_batches, batch_size] tensor")
    G, B = seeds.shape
    pos_rows, neg_rows = mp_skipgram_capacity(cfg, B)
    dev = seeds.device
    if out is None:
        out = (torch.empty((G, pos_rows, cfg.context_size), dtype=torch.int64, device=dev),
               torch.empty((G, neg_rows, cfg.context_size), dtype=torch.int64, device=dev))
    pos, neg = out
    if neg is None:
        neg = torch.empty((G, 0, cfg.context_size), dtype=torch.int64, device=dev)
    if tuple(pos.shape) != (G, pos_rows, cfg.context_size) or tuple(neg.shape) != (G, neg_rows, cfg.context_size) \
            or not (pos.is_contiguous() and neg.is_contiguous()):
        raise ValueError("mp_skipgram: out does not have this launch's shapes")
    need = mp_skipgram_workspace_bytes(cfg, G, B, form)
    if need and (ws is None or ws.numel() * ws.element_size() < need):
        ws = torch.empty(need // 8, dtype=torch.int64, device=dev)
    o = TgRwSkipgramOut(pos.data_ptr() if pos.numel() else None, neg.data_ptr() if neg.numel() else None)
    rng = TgRng(seed, call_id)
    check(lib.tg_mp_skipgram(C.byref(cfg), ptr(seeds), C.c_int64(G), C.c_int64(B), C.byref(rng), C.byref(o),
                             ptr(ws) if need else C.c_void_p(0), C.c_int64(ws.numel() * ws.element_size() if need else 0),
                             C.c_int32(form), stream_ptr(dev)))
    return pos, neg


LINK_BINARY, LINK_TRIPLET = 0, 1   # tg_link_seeds' `mode`


def link_seeds_capacity(n_edges, n_neg, mode=LINK_BINARY):
    """-> (S, P) of a mini-batch of n_edges positives with n_neg negatives each: seeds per row and (src, dst) pairs."""
    S, P = C.c_int64(-1), C.c_int64(-1)
    check(lib.tg_link_seeds_capacity(C.c_int64(n_edges), C.c_int64(n_neg), C.c_int32(mode), C.byref(S), C.byref(P)))
    return S.value, P.value


def link_seeds(graph, src, dst, K, mode, try_count, seed, call_id, n_nodes, edge_set=None, out=None, unverified=None):
    """Seed rows of the G mini-batches of positive edges src[G, E] -> dst[G, E] with K checked negatives each
    (tg_link_seeds), one launch on the current stream, nothing read back: -> (seeds [G, S], unverified [G]).  `graph` is the
    CSC the sampler walks, `edge_set` the optional set built over it (_cabi.edge_set); mini-batch g draws with call id
    call_id + g.  mode LINK_BINARY: seeds[g].view(2, P) is the global edge_label_index; LINK_TRIPLET: [src | dst_pos |
    dst_neg [E, K]].  The endpoints are not range-checked here (a loader checks them once); out / unverified: tensors of an
    earlier call of the same shape, reused."""
    for name, t in (("src", src), ("dst", dst)):
        if t.dim() != 2 or t.dtype != torch.int64 or not t.is_contiguous():
            raise ValueError("link_seeds: %s must be a contiguous int64 [n_batches, n_edges] tensor" % name)
    if src.shape != dst.shape or src.device != dst.device:
        raise ValueError("link_seeds: src and dst differ in shape or device")
    G, E = src.shape
    S, _ = link_seeds_capacity(E, K, mode)
    dev = src.device
    if out is None:
        out = torch.empty((G, S), dtype=torch.int64, device=dev)
    if unverified is None:
        unverified = torch.zeros(G, dtype=torch.int64, device=dev)
    if tuple(out.shape) != (G, S) or out.dtype != torch.int64 or not out.is_contiguous() or out.device != dev:
        raise ValueError("link_seeds: out is not a contiguous int64 [%d, %d] tensor on %s" % (G, S, dev))
    if tuple(unverified.shape) != (G,) or unverified.dtype != torch.int64 or not unverified.is_contiguous() \
            or unverified.device != dev:
        raise ValueError("link_seeds: unverified is not a contiguous int64 [%d] tensor on %s" % (G, dev))
    rng = TgRng(seed, call_id)
    check(lib.tg_link_seeds(C.byref(graph), ptr(edge_set), C.c_int64(edge_set.numel() * 8 if edge_set is not None else 0),
                            ptr(src), ptr(dst), C.c_int64(G), C.c_int64(E), C.c_int64(K), C.c_int32(mode),
                            C.c_int32(try_count), C.byref(rng), C.c_int64(n_nodes), ptr(out), ptr(unverified),
                            stream_ptr(dev)))
    return out, unverified


class TgLinkRel(C.Structure):
    _fields_ = [("csc", C.POINTER(TgGraph)), ("edge_set", C.c_void_p), ("edge_set_bytes", C.c_int64), ("n_src", C.c_int64),
                ("n_dst", C.c_int64), ("same_type", C.c_int32)]


def link_rel(graph, n_src, n_dst, same_type, edge_set=None):
    """The tg_link_rel of a relation's CSC `graph` (n_dst columns, row ids below n_src) and its optional edge set."""
    rel = TgLinkRel(C.pointer(graph), edge_set.data_ptr() if edge_set is not None else None,
                    edge_set.numel() * 8 if edge_set is not None else 0, int(n_src), int(n_dst), int(bool(same_type)))
    rel._keep = (graph, edge_set)                                     # the struct only borrows them
    return rel


def _link_rows(name, t, G, W, dev):
    """A [G, W] int64 view whose rows are contiguous (row stride >= W: the pitch) -> its pitch in words."""
    if t.dim() != 2 or tuple(t.shape) != (G, W) or t.dtype != torch.int64 or t.device != dev \
            or (W > 1 and t.stride(1) != 1) or (G > 1 and t.stride(0) < W):
        raise ValueError("link_seeds_typed: %s is not an int64 [%d, %d] view with contiguous rows on %s" % (name, G, W, dev))
    return t.stride(0) if G > 1 else max(t.stride(0), W)


def link_seeds_typed(graph, src, dst, K, mode, try_count, seed, call_id, n_src, n_dst, same_type, edge_set=None,
                     src_out=None, dst_out=None, unverified=None):
    """Typed seed rows (tg_link_seeds_typed) of the G mini-batches of positive edges src[G, E] -> dst[G, E] of ONE relation
    with K checked negatives each, one launch on the current stream, nothing read back: -> (src rows [G, Ws], dst rows
    [G, Wd], unverified [G]).  `graph` is the relation's CSC (n_dst columns, row ids < n_src), `edge_set` the optional set
    built over it; same_type: both endpoints are one node type, s == d is then rejected.  LINK_BINARY: Ws = Wd = P, rows
    [pos | neg]; LINK_TRIPLET: Ws = E [src], Wd = P [dst_pos | dst_neg [E, K]].  src_out / dst_out may be strided 2-D views
    with contiguous rows (the pitch is the view's row stride), e.g. out[:, :Ws] and out[:, Ws:] of one [G, S] tensor, which
    is tg_link_seeds' layout; they are allocated when not given.  The endpoints are not range-checked here."""
    for name, t in (("src", src), ("dst", dst)):
        if t.dim() != 2 or t.dtype != torch.int64 or not t.is_contiguous():
            raise ValueError("link_seeds_typed: %s must be a contiguous int64 [n_batches, n_edges] tensor" % name)
    if src.shape != dst.shape or src.device != dst.device:
        raise ValueError("link_seeds_typed: src and dst differ in shape or device")
    G, E = src.shape
    _, P = link_seeds_capacity(E, K, mode)
    Ws, Wd = (P if mode == LINK_BINARY else E), P
    dev = src.device
    if src_out is None:
        src_out = torch.empty((G, Ws), dtype=torch.int64, device=dev)
    if dst_out is None:
        dst_out = torch.empty((G, Wd), dtype=torch.int64, device=dev)
    if unverified is None:
        unverified = torch.zeros(G, dtype=torch.int64, device=dev)
    sp, dp = _link_rows("src_out", src_out, G, Ws, dev), _link_rows("dst_out", dst_out, G, Wd, dev)
    if tuple(unverified.shape) != (G,) or unverified.dtype != torch.int64 or not unverified.is_contiguous() \
            or unverified.device != dev:
        raise ValueError("link_seeds_typed: unverified is not a contiguous int64 [%d] tensor on %s" % (G, dev))
    rel, rng = link_rel(graph, n_src, n_dst, same_type, edge_set), TgRng(seed, call_id)
    check(lib.tg_link_seeds_typed(C.byref(rel), ptr(src), ptr(dst), C.c_int64(G), C.c_int64(E), C.c_int64(K), C.c_int32(mode),
                                  C.c_int32(try_count), C.byref(rng), ptr(src_out), C.c_int64(sp), ptr(dst_out),
                                  C.c_int64(dp), ptr(unverified), stream_ptr(dev)))
    return src_out, dst_out, unverified


def tempo_random_walk(graph, node_ts, edge_ts, start, start_ts, walk_length, window, seed, call_id):
    walks = torch.empty((start.numel(), walk_length), dtype=torch.int64, device=start.device)
    wts = torch.empty((start.numel(), walk_length), dtype=torch.int64, device=start.device)
    rng = TgRng(seed, call_id)
    check(lib.tg_tempo_random_walk(C.byref(graph), ptr(node_ts), ptr(edge_ts), ptr(start), ptr(start_ts),
                                   C.c_int64(start.numel()), C.c_int64(walk_length), C.c_int64(window[0]),
                                   C.c_int64(window[1]), C.byref(rng), ptr(walks), ptr(wts),
                                   stream_ptr(start.device)))
    return walks, wts


class TgTempoSkipgramConfig(C.Structure):
    _fields_ = [("walk_length", C.c_int64), ("context_size", C.c_int64), ("walks_per_node", C.c_int64),
                ("num_negative_samples", C.c_int64), ("n_nodes", C.c_int64), ("win0", C.c_int64), ("win1", C.c_int64)]


class TgTempoSkipgramOut(C.Structure):
    _fields_ = [("pos_rw", C.c_void_p), ("pos_ts", C.c_void_p), ("neg_rw", C.c_void_p)]


def tempo_skipgram_config(walk_length, context_size, window, walks_per_node=1, num_negative_samples=1, n_nodes=0):
    """walk_length counts COLUMNS of a row, as tempo_random_walk (rw_skipgram_config's counts steps)."""
    return TgTempoSkipgramConfig(int(walk_length), int(context_size), int(walks_per_node), int(num_negative_samples),
                                 int(n_nodes), int(window[0]), int(window[1]))


def tempo_skipgram_capacity(cfg, batch_size):
    """-> (rows of pos_rw / pos_ts, rows of neg_rw) per mini-batch of batch_size seeds: nw * R * B and nw * R * K * B."""
    pos, neg = C.c_int64(-1), C.c_int64(-1)
    check(lib.tg_tempo_skipgram_capacity(C.byref(cfg), C.c_int64(batch_size), C.byref(pos), C.byref(neg)))
    return pos.value, neg.value


def tempo_skipgram_lds_bytes(cfg):
    """-> (walkers_per_workgroup, lds_bytes) of a tg_tempo_skipgram launch: walkers * ((2 L | 1) + 1) * 8 bytes.  Raises
    (TG_ERR_UNSUPPORTED) when one walker's rows do not fit.  No device is touched."""
    walkers, nbytes = C.c_int32(-1), C.c_int64(-1)
    check(lib.tg_tempo_skipgram_lds_bytes(C.byref(cfg), C.byref(walkers), C.byref(nbytes)))
    return walkers.value, nbytes.value


def tempo_skipgram(graph, node_ts, edge_ts, seeds, seeds_ts, cfg, seed, call_id, with_ts=True, out=None):
    """Temporal skip-gram batches (tg_tempo_skipgram) of the G mini-batches seeds[G, B] with start times seeds_ts[G, B] in
    one launch on the current stream: -> (pos_rw [G, nw * R * B, C], pos_ts of the same shape or None, neg_rw [G, nw * R *
    K * B, C]); mini-batch g draws with call id call_id + g and is a free view.  pos_ts holds the timestamp of every word
    of pos_rw (-1: none).  graph: the CSR, edge_ts in its edge order, node_ts per node.  out: the triple of an earlier call
    of the same shape (and with_ts), reused."""
    for name, t in (("seeds", seeds), ("seeds_ts", seeds_ts)):
        if t.dim() != 2 or t.dtype != torch.int64 or not t.is_contiguous():
            raise ValueError("tempo_skipgram: %s must be a contiguous int64 [n_batches, batch_size] tensor" % name)
    if seeds.shape != seeds_ts.shape or seeds.device != seeds_ts.device:
        raise ValueError("tempo_skipgram: seeds and seeds_ts differ in shape or device")
    G, B = seeds.shape
    pos_rows, neg_rows = tempo_skipgram_capacity(cfg, B)
    dev, Cs = seeds.device, cfg.context_size
    if out is None:
        out = (torch.empty((G, pos_rows, Cs), dtype=torch.int64, device=dev),
               torch.empty((G, pos_rows, Cs), dtype=torch.int64, device=dev) if with_ts else None,
               torch.empty((G, neg_rows, Cs), dtype=torch.int64, device=dev))
    pos, pts, neg = out
    if neg is None:
        neg = torch.empty((G, 0, Cs), dtype=torch.int64, device=dev)
    shapes = [(pos, pos_rows), (neg, neg_rows)] + ([(pts, pos_rows)] if with_ts else [])
    if (pts is None) == bool(with_ts) or any(t is None or tuple(t.shape) != (G, rows, Cs) or t.dtype != torch.int64
                                             or not t.is_contiguous() for t, rows in shapes):
        raise ValueError("tempo_skipgram: out does not have this launch's shapes")
    o = TgTempoSkipgramOut(pos.data_ptr() if pos.numel() else None, pts.data_ptr() if with_ts and pts.numel() else None,
                           neg.data_ptr() if neg.numel() else None)
    rng = TgRng(seed, call_id)
    check(lib.tg_tempo_skipgram(C.byref(graph), ptr(node_ts), ptr(edge_ts), ptr(seeds), ptr(seeds_ts), C.c_int64(G),
                                C.c_int64(B), C.byref(cfg), C.byref(rng), C.byref(o), stream_ptr(dev)))
    return pos, pts, neg


class TgHetProblem(C.Structure):
    _fields_ = [("n_types", C.c_int32), ("n_rels", C.c_int32), ("n_hops", C.c_int32), ("sampler", C.c_int32),
                ("rel_src", C.POINTER(C.c_int32)), ("rel_dst", C.POINTER(C.c_int32)), ("graphs", C.POINTER(TgGraph)),
                ("fanout", C.POINTER(C.c_int64)), ("inputs", C.POINTER(C.c_void_p)), ("n_inputs", C.POINTER(C.c_int64))]


class TgHetOut(C.Structure):
    _fields_ = [("samples", C.POINTER(C.c_void_p)), ("cap_nodes", C.POINTER(C.c_int64)),
                ("rows", C.POINTER(C.c_void_p)), ("cols", C.POINTER(C.c_void_p)), ("edge_index", C.POINTER(C.c_void_p)),
                ("cap_edges", C.POINTER(C.c_int64)), ("layer_offsets", C.c_void_p), ("counts", C.c_void_p)]


class NsHeteroBatched:
    """Problem description + output slabs of tg_ns_hetero_batched.  rels: list of (src type index, dst type index,
    ptrs, indices, [fanout per hop]); inputs: list over node types of [n_batches, n_inputs] tensors or None."""

    def __init__(self, n_types, rels, inputs, n_hops, n_batches, device, sampler=SAMPLER_UNIFORM):
        T, R = n_types, len(rels)
        self.T, self.R, self.H, self.nb, self.dev = T, R, n_hops, n_batches, device
        self._keep = [rels, inputs]
        self.rel_src, self.rel_dst, self.graphs = _rel_arrays(rels)
        self.fanout = _i64([k for r in rels for k in r[4]])
        self.n_inputs = _i64([0 if x is None else x.shape[1] for x in inputs])
        self.inputs = _vp(inputs)
        self.problem = TgHetProblem(T, R, n_hops, sampler, self.rel_src, self.rel_dst, self.graphs, self.fanout,
                                    self.inputs, self.n_inputs)
        self.cap_nodes, self.cap_edges = (C.c_int64 * T)(), (C.c_int64 * max(R, 1))()
        check(lib.tg_ns_hetero_capacity(C.byref(self.problem), self.cap_nodes, self.cap_edges))
        o = dict(dtype=torch.int64, device=device)
        self.samples = [torch.empty((n_batches, max(self.cap_nodes[t], 1)), **o) for t in range(T)]
        self.rows = [torch.empty((n_batches, max(self.cap_edges[r], 1)), **o) for r in range(R)]
        self.cols = [torch.empty((n_batches, max(self.cap_edges[r], 1)), **o) for r in range(R)]
        self.edge_index = [torch.empty((n_batches, max(self.cap_edges[r], 1)), **o) for r in range(R)]
        self.layer_offsets = torch.zeros((n_batches, max(R, 1), max(n_hops, 1), 3), **o)
        self.counts = torch.zeros((n_batches, T + R), **o)
        # the slabs are allocated with at least one column; tell the library their true pitch
        self.cap_nodes_alloc = _i64([max(self.cap_nodes[t], 1) for t in range(T)])
        self.cap_edges_alloc = _i64([max(self.cap_edges[r], 1) for r in range(R)])
        self._ptrs = [_vp(self.samples), _vp(self.rows), _vp(self.cols), _vp(self.edge_index)]
        self.out = TgHetOut(self._ptrs[0], self.cap_nodes_alloc, self._ptrs[1], self._ptrs[2], self._ptrs[3],
                            self.cap_edges_alloc, self.layer_offsets.data_ptr(), self.counts.data_ptr())

    def run(self, seed, call_id):
        rng = TgRng(seed, call_id)
        check(lib.tg_ns_hetero_batched(C.byref(self.problem), C.c_int64(self.nb), C.byref(rng), C.byref(self.out),
                                       stream_ptr(self.dev)))


class TgHgtProblem(C.Structure):
    _fields_ = [("n_types", C.c_int32), ("n_rels", C.c_int32), ("n_hops", C.c_int32), ("has_timerange", C.c_int32),
                ("rel_src", C.POINTER(C.c_int32)), ("rel_dst", C.POINTER(C.c_int32)), ("graphs", C.POINTER(TgGraph)),
                ("inputs", C.POINTER(C.c_void_p)), ("input_ts", C.POINTER(C.c_void_p)), ("n_inputs", C.POINTER(C.c_int64)),
                ("num_samples", C.POINTER(C.c_int64)), ("tr_lo", C.c_int64), ("tr_hi", C.c_int64)]


class TgHgtBatchedOut(C.Structure):
    _fields_ = [("samples", C.POINTER(C.c_void_p)), ("sample_ts", C.POINTER(C.c_void_p)), ("cap_nodes", C.POINTER(C.c_int64)),
                ("rows", C.POINTER(C.c_void_p)), ("cols", C.POINTER(C.c_void_p)), ("edge_index", C.POINTER(C.c_void_p)),
                ("cap_edges", C.POINTER(C.c_int64)), ("counts", C.c_void_p)]


def _typed_problem(p, n_types, rels, n_inputs, inputs, input_ts=None, timestamps=False, **arrays):
    """Fills what the hgt, budget and negative problem structs share -- the type and relation counts, the relation
    arrays, the per-type inputs (and input timestamps, where the struct has them and the caller gives some) -- and the
    further ctypes arrays in `arrays`, by field name.  The struct only borrows all of it: p._keep holds it alive."""
    p.n_types, p.n_rels = n_types, len(rels)
    rel = _rel_arrays(rels, timestamps)
    p.rel_src, p.rel_dst, p.graphs = rel
    ins, n_in = _vp(inputs if inputs is not None else [None] * n_types), _i64(n_inputs)
    p.inputs, p.n_inputs = ins, n_in
    its = _vp(input_ts) if input_ts is not None else None
    if its is not None:
        p.input_ts = its
    for field, array in arrays.items():
        setattr(p, field, array)
    p._keep = (rels, inputs, input_ts, rel, ins, n_in, its, arrays)
    return p


def _call_major(tensors, n_calls, missing):
    """Per-type inputs of a batched launch as contiguous [n_calls, n_inputs] tensors -> (tensors, n_inputs per type);
    `missing` is the n_inputs of a type without an entry."""
    n_in = [missing if x is None else int(x.shape[-1]) for x in tensors]
    return [None if x is None else x.reshape(n_calls, n_in[t]).contiguous() for t, x in enumerate(tensors)], n_in


class _Batched:
    """The output slabs, counts and workspace of a batched typed operator (hgt, budget, negative): n_calls calls of one
    shape per launch.  A subclass names its per-node-type and per-relation slab lists, the state words each call has
    behind its T + R counts, the out struct (slab pointers, node pitches, slab pointers, edge pitches, counts[, ...] in
    that order) and the library's capacity / workspace / launch functions; this class allocates the slabs with row pitch
    capacity + pad (at least one word), the state block and the workspace, and gives run() and call()."""
    NODE_SLABS, EDGE_SLABS, TAIL = ("samples", "sample_ts"), ("rows", "cols", "edge_index"), 0
    OUT = LAUNCH = capacity = workspace_bytes_of = None

    @classmethod
    def pitches(cls, problem, pad=0):
        """Row pitches (per type, per relation) of the slabs: the capacity + pad words, at least one."""
        cap_n, cap_e = cls.capacity(problem)
        return [max(c + pad, 1) for c in cap_n], [max(c + pad, 1) for c in cap_e]

    @classmethod
    def bytes_of(cls, problem, n_calls, pad=0):
        """Device bytes of one launch as this class allocates it: the workspace, the output slabs (sized for the worst
        case) and the state block."""
        return cls.workspace_bytes_of(problem, n_calls) + 8 * n_calls * cls._call_words(*cls.pitches(problem, pad))

    @classmethod
    def _call_words(cls, node_pitch, edge_pitch):
        """int64 words of one call: its row in every slab, its T + R counts and its tail words"""
        return (len(cls.NODE_SLABS) * sum(node_pitch) + len(cls.EDGE_SLABS) * sum(edge_pitch) + len(node_pitch) +
                len(edge_pitch) + cls.TAIL)

    def __init__(self, problem, n_calls, device, pad=0):
        T, R, n = problem.n_types, problem.n_rels, int(n_calls)
        self.problem, self.T, self.R, self.nc, self.dev = problem, T, R, n, device
        self.cap_nodes, self.cap_edges = self.capacity(problem)
        self.node_pitch, self.edge_pitch = self.pitches(problem, pad)
        o = dict(dtype=torch.int64, device=device)
        self._arrays = []
        for names, pitch in ((self.NODE_SLABS, self.node_pitch), (self.EDGE_SLABS, self.edge_pitch)):
            for name in names:
                setattr(self, name, [torch.empty((n, p), **o) for p in pitch])
                self._arrays.append(_vp(getattr(self, name)))
            self._arrays.append(_i64(pitch))
        self.state = torch.zeros(n * (T + R + self.TAIL), **o)
        self.workspace_bytes = self.workspace_bytes_of(problem, n)
        self.workspace = torch.empty(self.workspace_bytes // 8 + 1, **o)
        self.launch_bytes = self.workspace_bytes + 8 * n * self._call_words(self.node_pitch, self.edge_pitch)
        self.out = self.OUT(*self._arrays, *self._state_fields())

    def _state_fields(self):
        """Cuts `state` into what the library writes -> the out struct's fields behind the pitches.  Here: one
        [n_calls, T + R + TAIL] counts block (a call's tail words are the last columns of its row)."""
        self.counts = self.state.view(self.nc, -1)
        return (self.counts.data_ptr(),)

    def run(self, seed, call_id):
        rng = TgRng(seed, call_id)
        check(self.LAUNCH(C.byref(self.problem), C.c_int64(self.nc), C.byref(rng), C.byref(self.out), ptr(self.workspace),
                          C.c_int64(self.workspace_bytes), stream_ptr(self.dev)))

    def call(self, b, counts=None):
        """Call b's results trimmed to its counts -> one list per node slab ([T]), one per edge slab ([R]), then the tail
        words of its counts row (counts: the counts block already read back, else it is read here)."""
        c = (self.counts[b].tolist() if counts is None else [int(x) for x in counts[b]])
        T, R = self.T, self.R
        return (tuple([getattr(self, k)[t][b, :c[t]] for t in range(T)] for k in self.NODE_SLABS) +
                tuple([getattr(self, k)[r][b, :c[T + r]] for r in range(R)] for k in self.EDGE_SLABS) + tuple(c[T + R:]))


def hgt_problem(n_types, rels, n_inputs, num_samples, n_hops, inputs=None, input_ts=None, timerange=None):
    """A tg_hgt_problem.  rels: list of (src type index, dst type index, ptrs, indices, row timestamps or None);
    n_inputs: per type (< 0: no entry in `inputs`); num_samples: per type a list of n_hops quotas, or None (no entry);
    inputs / input_ts: per type a device tensor or None (input_ts None: no input timestamps at all)."""
    ns = _i64([q[h] if q is not None else -1 for q in num_samples for h in range(n_hops)])
    p = _typed_problem(TgHgtProblem(), n_types, rels, n_inputs, inputs, input_ts, timestamps=True, num_samples=ns)
    p.n_hops = n_hops
    if timerange is not None:
        p.has_timerange, p.tr_lo, p.tr_hi = 1, int(timerange[0]), int(timerange[1])
    return p


def hgt_batched_capacity(problem):
    """-> (cap_nodes [T], cap_edges [R]) of one call (tg_hgt_batched_capacity)."""
    cn, ce = (C.c_int64 * problem.n_types)(), (C.c_int64 * max(problem.n_rels, 1))()
    check(lib.tg_hgt_batched_capacity(C.byref(problem), cn, ce))
    return list(cn), list(ce)[:problem.n_rels]


def hgt_batched_workspace_bytes(problem, n_calls):
    nbytes = C.c_int64(0)
    check(lib.tg_hgt_batched_workspace_bytes(C.byref(problem), C.c_int64(n_calls), C.byref(nbytes)))
    return nbytes.value


class HgtBatched(_Batched):
    """Problem description, output slabs and workspace of tg_hgt_sample_batched: n_calls hgt_sampling calls of one shape
    per launch chain.  inputs / input_ts: per node type a [n_calls, n_inputs] tensor or None (no entry in `inputs`);
    num_samples: per type a list of n_hops quotas or None; rels as in hgt_problem.  pad: extra words per slab row (the
    pitches then exceed the capacities).  Call b of run(seed, call_id) equals hgt_sampling with call id call_id + b;
    call(b) -> (samples [T], sample_ts [T], rows [R], cols [R], edge_index [R], panic): the panic word is the last
    column of `counts` ([n_calls, T + R + 1])."""
    TAIL, OUT, LAUNCH = 1, TgHgtBatchedOut, lib.tg_hgt_sample_batched
    capacity, workspace_bytes_of = staticmethod(hgt_batched_capacity), staticmethod(hgt_batched_workspace_bytes)

    def __init__(self, n_types, rels, inputs, num_samples, n_hops, n_calls, device, input_ts=None, timerange=None, pad=0):
        self.H = n_hops
        self.inputs, n_in = _call_major(inputs, n_calls, -1)
        self.input_ts = _call_major(input_ts, n_calls, -1)[0] if input_ts is not None else None
        super().__init__(hgt_problem(n_types, rels, n_in, num_samples, n_hops, self.inputs, self.input_ts, timerange),
                         n_calls, device, pad)


class TgBudgetProblem(C.Structure):
    _fields_ = [("n_types", C.c_int32), ("n_rels", C.c_int32), ("n_hops", C.c_int32), ("filter_on", C.c_int32),
                ("forward", C.c_int32), ("relative", C.c_int32), ("win_lo", C.c_int64), ("win_hi", C.c_int64),
                ("rel_src", C.POINTER(C.c_int32)), ("rel_dst", C.POINTER(C.c_int32)), ("graphs", C.POINTER(TgGraph)),
                ("num_neighbors", C.POINTER(C.c_int64)), ("inputs", C.POINTER(C.c_void_p)),
                ("input_ts", C.POINTER(C.c_void_p)), ("n_inputs", C.POINTER(C.c_int64))]


class TgBudgetBatchedOut(C.Structure):
    _fields_ = [("samples", C.POINTER(C.c_void_p)), ("sample_ts", C.POINTER(C.c_void_p)),
                ("pitch_nodes", C.POINTER(C.c_int64)), ("rows", C.POINTER(C.c_void_p)), ("cols", C.POINTER(C.c_void_p)),
                ("edge_index", C.POINTER(C.c_void_p)), ("pitch_edges", C.POINTER(C.c_int64)), ("counts", C.c_void_p)]


def budget_problem(n_types, rels, n_inputs, num_neighbors, n_hops, inputs=None, input_ts=None, window=None, forward=False,
                   relative=False):
    """A tg_budget_problem.  rels: list of (src type index, dst type index, ptrs, indices, row timestamps or None);
    n_inputs: per type; num_neighbors: per type a list of n_hops quotas; inputs / input_ts: per type a device tensor or
    None (input_ts None: no input timestamps at all); window = (lo, hi) turns the temporal filter on (python.rs:541-548)."""
    nn = _i64([q[h] for q in num_neighbors for h in range(n_hops)])
    p = _typed_problem(TgBudgetProblem(), n_types, rels, n_inputs, inputs, input_ts, timestamps=True, num_neighbors=nn)
    p.n_hops = n_hops
    if window is not None:
        p.filter_on, p.forward, p.relative = 1, int(bool(forward)), int(bool(relative))
        p.win_lo, p.win_hi = int(window[0]), int(window[1])
    return p


def budget_capacity(problem):
    """-> (cap_nodes [T], cap_edges [R]) of one call (tg_budget_capacity: the worst case of every list)."""
    cn, ce = (C.c_int64 * problem.n_types)(), (C.c_int64 * max(problem.n_rels, 1))()
    check(lib.tg_budget_capacity(C.byref(problem), cn, ce))
    return list(cn), list(ce)[:problem.n_rels]


def budget_batched_workspace_bytes(problem, n_calls):
    nbytes = C.c_int64(0)
    check(lib.tg_budget_batched_workspace_bytes(C.byref(problem), C.c_int64(n_calls), C.byref(nbytes)))
    return nbytes.value


class BudgetBatched(_Batched):
    """Problem description, output slabs and workspace of tg_budget_sample_batched: n_calls budget_sampling calls of one
    shape per launch chain.  inputs / input_ts: per node type a [n_calls, n_inputs] tensor or None (no inputs);
    num_neighbors: per type a list of n_hops quotas; rels as in budget_problem.  pad: extra words per slab row (the pitches
    then exceed the capacities).  Call b of run(seed, call_id) equals budget_sampling with call id call_id + b; call(b) ->
    (samples [T], sample_ts [T], rows [R], cols [R], edge_index [R]).  The slabs are sized for the worst case, far above
    typical counts, and are most of launch_bytes."""
    OUT, LAUNCH = TgBudgetBatchedOut, lib.tg_budget_sample_batched
    capacity, workspace_bytes_of = staticmethod(budget_capacity), staticmethod(budget_batched_workspace_bytes)

    def __init__(self, n_types, rels, inputs, num_neighbors, n_hops, n_calls, device, input_ts=None, window=None,
                 forward=False, relative=False, pad=0):
        self.H = n_hops
        self.inputs, n_in = _call_major(inputs, n_calls, 0)
        self.input_ts = _call_major(input_ts, n_calls, 0)[0] if input_ts is not None else None
        super().__init__(budget_problem(n_types, rels, n_in, num_neighbors, n_hops, self.inputs, self.input_ts, window,
                                        forward, relative), n_calls, device, pad)


budget_batched_pitches, budget_batched_bytes = BudgetBatched.pitches, BudgetBatched.bytes_of


class TgBudgetLayerIn(C.Structure):
    _fields_ = [("graphs", C.POINTER(TgGraph)), ("rel_ids", C.POINTER(C.c_int32)), ("n_rels", C.c_int32),
                ("node_type", C.c_int32), ("fanout", C.c_int32), ("filter_on", C.c_int32), ("forward", C.c_int32),
                ("relative", C.c_int32), ("win_lo", C.c_int64), ("win_hi", C.c_int64), ("nodes", C.c_void_p),
                ("nodes_ts", C.c_void_p), ("n_front", C.c_int64), ("id_base", C.c_int64)]


class TgBudgetLayerOut(C.Structure):
    _fields_ = [("sel_v", C.c_void_p), ("sel_ts", C.c_void_p), ("sel_rel", C.c_void_p), ("sel_i", C.c_void_p)]


def budget_layer(rels, rel_ids, node_type, fanout, nodes, nodes_ts, seed, call_id, id_base=0, window=None, forward=False,
                 relative=False):
    """tg_budget_layer: Budget::update + Budget::sample for every frontier node of one node type, one (layer, type)
    step.  rels: the relations INTO the type as (src type index, dst type index, ptrs, indices, row timestamps or None),
    rel_ids their indices in the caller's relation list; nodes / nodes_ts: [n_front] device tensors.
    -> (sel_v, sel_ts, sel_rel, sel_i), each [n_front, fanout]; sel_rel < 0 marks an empty slot."""
    n = nodes.numel()
    _, _, graphs = _rel_arrays(rels, timestamps=True)
    lin = TgBudgetLayerIn()
    lin.graphs, lin.rel_ids, lin.n_rels = graphs, (C.c_int32 * max(len(rels), 1))(*rel_ids), len(rels)
    lin.node_type, lin.fanout = node_type, fanout
    if window is not None:
        lin.filter_on, lin.forward, lin.relative = 1, int(bool(forward)), int(bool(relative))
        lin.win_lo, lin.win_hi = int(window[0]), int(window[1])
    lin.nodes, lin.nodes_ts, lin.n_front, lin.id_base = nodes.data_ptr(), nodes_ts.data_ptr(), n, id_base
    sel = [torch.empty((n, fanout), dtype=torch.int64, device=nodes.device) for _ in range(4)]
    out = TgBudgetLayerOut(*[x.data_ptr() for x in sel])
    rng = TgRng(seed, call_id)
    check(lib.tg_budget_layer(C.byref(lin), C.byref(rng), C.byref(out), stream_ptr(nodes.device)))
    return tuple(sel)


class TgNegProblem(C.Structure):
    _fields_ = [("n_types", C.c_int32), ("n_rels", C.c_int32), ("homogeneous", C.c_int32), ("inbound", C.c_int32),
                ("rel_src", C.POINTER(C.c_int32)), ("rel_dst", C.POINTER(C.c_int32)), ("graphs", C.POINTER(TgGraph)),
                ("node_count", C.POINTER(C.c_int64)), ("inputs", C.POINTER(C.c_void_p)), ("n_inputs", C.POINTER(C.c_int64)),
                ("num_neg", C.c_int64), ("try_count", C.c_int64)]


class TgNegBatchedOut(C.Structure):
    _fields_ = [("samples", C.POINTER(C.c_void_p)), ("pitch_nodes", C.POINTER(C.c_int64)), ("rows", C.POINTER(C.c_void_p)),
                ("cols", C.POINTER(C.c_void_p)), ("pitch_edges", C.POINTER(C.c_int64)), ("counts", C.c_void_p),
                ("panic", C.c_void_p)]


TG_NEG_MAX_CALLS = 65535
NEG_LDS_160K = 160 * 1024   # a gfx950 workgroup's LDS limit, for form queries that touch no device


def neg_problem(n_types, rels, n_inputs, num_neg, try_count, inputs=None, inbound=False, homogeneous=False):
    """A tg_neg_problem.  rels: list of (src type index, dst type index, CSR ptrs, CSR indices, node_count) with
    node_count = the size of the range the negatives are drawn from (sizes[rel][1]); n_inputs: per type, < 0 where the type
    has no entry in `inputs`; inputs: per type a device tensor ([n_calls, n_inputs] for the batched form) or None."""
    p = _typed_problem(TgNegProblem(), n_types, rels, n_inputs, inputs, node_count=_i64([r[4] for r in rels]))
    p.homogeneous, p.inbound = int(bool(homogeneous)), int(bool(inbound))
    p.num_neg, p.try_count = int(num_neg), int(try_count)
    return p


def neg_batched_capacity(problem):
    """-> (cap_nodes [T], cap_edges [R]) of one call: max(n_inputs[t], 0) + total items; n_inputs[src] * num_neg."""
    cn, ce = (C.c_int64 * max(problem.n_types, 1))(), (C.c_int64 * max(problem.n_rels, 1))()
    check(lib.tg_neg_batched_capacity(C.byref(problem), cn, ce))
    return list(cn)[:problem.n_types], list(ce)[:problem.n_rels]


def neg_batched_form(problem, lds_limit_bytes=0):
    """-> (form, lds_bytes): 1 = one workgroup runs one whole call in LDS, 0 = call by call; the LDS the fused kernel asks
    for.  lds_limit_bytes > 0: taken as the workgroup's limit, no device is touched; otherwise the current device is asked."""
    form, nbytes = C.c_int32(-1), C.c_int64(0)
    check(lib.tg_neg_batched_form(C.byref(problem), C.c_int64(lds_limit_bytes), C.byref(form), C.byref(nbytes)))
    return form.value, nbytes.value


def neg_batched_workspace_bytes(problem, n_calls):
    nbytes = C.c_int64(0)
    check(lib.tg_neg_batched_workspace_bytes(C.byref(problem), C.c_int64(n_calls), C.byref(nbytes)))
    return nbytes.value


class NegBatched(_Batched):
    """Problem description, input and output slabs and workspace of tg_neg_sample_batched: n_calls negative-sampling calls of
    one shape per launch.  inputs: per node type a [n_calls, n_inputs] tensor or None (no entry in `inputs`); rels as in
    neg_problem.  pad: extra words per slab row (the pitches then exceed the capacities).  Call b of run(seed, call_id)
    equals the single operator with call id call_id + b; call(b) -> (samples [T], rows [R], cols [R]).  counts and panic
    share one tensor (`state`, n_calls x (T + R + 1) words, the panic words last), so one read-back fetches both."""
    NODE_SLABS, EDGE_SLABS, TAIL = ("samples",), ("rows", "cols"), 1
    OUT, LAUNCH = TgNegBatchedOut, lib.tg_neg_sample_batched
    capacity, workspace_bytes_of = staticmethod(neg_batched_capacity), staticmethod(neg_batched_workspace_bytes)

    def __init__(self, n_types, rels, inputs, num_neg, try_count, n_calls, device, inbound=False, homogeneous=False, pad=0):
        self.inputs, n_in = _call_major(inputs, n_calls, -1)
        problem = neg_problem(n_types, rels, n_in, num_neg, try_count, self.inputs, inbound, homogeneous)
        self.form, self.lds_bytes = neg_batched_form(problem)
        super().__init__(problem, n_calls, device, pad)

    def _state_fields(self):
        # counts [n_calls, T + R] first (its own contiguous block, as the C ABI wants it), the panic words behind it
        n = self.nc * (self.T + self.R)
        self.counts = self.state[:n].view(self.nc, self.T + self.R)
        self.panic = self.state[n:].view(torch.int32)[:self.nc]
        return self.counts.data_ptr(), self.panic.data_ptr()

    def read_state(self):
        """ONE read-back -> (counts [n_calls, T + R], panic [n_calls]) as host tensors."""
        h = self.state.cpu()
        n = self.nc * (self.T + self.R)
        return h[:n].view(self.nc, self.T + self.R), h[n:].view(torch.int32)[:self.nc]


neg_batched_pitches, neg_batched_bytes = NegBatched.pitches, NegBatched.bytes_of


BIAS = {"uniform": 0, "linear": 1, "exponential": 2}


def biased_tempo_random_walk(graph, node_ts, edge_ts, start, start_ts, walk_length, bias, forward, retry_count, seed,
                             call_id, max_degree=None):
    """-> (walks, walks_ts, status word)."""
    dev, n = start.device, start.numel()
    walks = torch.empty((n, walk_length), dtype=torch.int64, device=dev)
    wts = torch.empty((n, walk_length), dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = C.c_int64(0)
    if max_degree is None:
        max_degree = 0
    check(lib.tg_biased_walk_workspace_bytes(C.c_int64(n), C.c_int64(max_degree), C.c_int32(BIAS[bias]), C.byref(nbytes)))
    ws = torch.empty(nbytes.value // 8 + 1, dtype=torch.int64, device=dev)
    rng = TgRng(seed, call_id)
    check(lib.tg_biased_tempo_random_walk(C.byref(graph), ptr(node_ts), ptr(edge_ts), ptr(start), ptr(start_ts),
                                          C.c_int64(n), C.c_int64(walk_length), C.c_int32(BIAS[bias]),
                                          C.c_int32(int(forward)), C.c_int64(retry_count), C.c_int64(max_degree),
                                          C.byref(rng), ptr(walks), ptr(wts), ptr(status), ptr(ws),
                                          C.c_int64(nbytes.value), stream_ptr(dev)))
    return walks, wts, status


def rmat_edges(scale, n_edges, seed, device):
    row = torch.empty(n_edges, dtype=torch.int64, device=device)
    col = torch.empty(n_edges, dtype=torch.int64, device=device)
    check(lib.tg_rmat_edges(C.c_int32(scale), C.c_int64(n_edges), C.c_uint64(seed), ptr(row), ptr(col),
                            stream_ptr(device)))
    return row, col


def rmat_edges_rect(row_scale, col_scale, n_edges, seed, device):
    row = torch.empty(n_edges, dtype=torch.int64, device=device)
    col = torch.empty(n_edges, dtype=torch.int64, device=device)
    check(lib.tg_rmat_edges_rect(C.c_int32(row_scale), C.c_int32(col_scale), C.c_int64(n_edges), C.c_uint64(seed),
                                 ptr(row), ptr(col), stream_ptr(device)))
    return row, col


def seed_batches(seed, first_batch, n_batches, n_seeds, n_nodes, device):
    out = torch.empty((n_batches, n_seeds), dtype=torch.int64, device=device)
    check(lib.tg_seed_batches(C.c_uint64(seed), C.c_int64(first_batch), C.c_int64(n_batches), C.c_int64(n_seeds),
                              C.c_int64(n_nodes), ptr(out), stream_ptr(device)))
    return out


def ind2ptr(ind, m):
    out = torch.empty(m + 1, dtype=torch.int64, device=ind.device)
    check(lib.tg_ind2ptr(ptr(ind), C.c_int64(ind.numel()), C.c_int64(m), ptr(out), stream_ptr(ind.device)))
    return out


def coo_to_csx(row, col, size0, size1, csc):
    """Device ingest (tg_coo_to_csx): stable radix sort by the reference's key (storage.rs:112,119), then
    ptrs / indices.  Returns (ptrs, indices, perm)."""
    nnz, dev = row.numel(), row.device
    o = dict(dtype=torch.int64, device=dev)
    m = size1 if csc else size0
    ptrs, indices, perm = torch.empty(m + 1, **o), torch.empty(nnz, **o), torch.empty(nnz, **o)
    nbytes = C.c_int64(0)
    check(lib.tg_coo_to_csx_workspace_bytes(C.c_int64(nnz), C.c_int64(size0), C.c_int64(size1), C.byref(nbytes)))
    ws = torch.empty(nbytes.value // 8 + 1, **o)
    row, col = row.contiguous(), col.contiguous()
    check(lib.tg_coo_to_csx(ptr(row) if nnz else None, ptr(col) if nnz else None, C.c_int64(nnz), C.c_int64(size0),
                            C.c_int64(size1), C.c_int32(int(csc)), ptr(ptrs), ptr(indices), ptr(perm), ptr(ws),
                            C.c_int64(nbytes.value), stream_ptr(dev)))
    return ptrs, indices, perm


def ns_homo_compact(out, n_batches, counts_host, stacked=False):
    """Flat batch-major (samples, rows, cols, edge_index) of the first n_batches of an NsBatchedOut; counts_host: the
    [n_batches, 2] counts already read back (sizes the flat arrays).  stacked: rows and cols are the two rows of ONE
    [2, E] tensor (what a loader hands out as edge_index) -> (samples, [rows; cols], edge_index)."""
    dev = out.samples.device
    total_n, total_e = int(counts_host[:, 0].sum()), int(counts_host[:, 1].sum())
    c = out.counts[:n_batches]
    off = torch.zeros((2, n_batches + 1), dtype=torch.int64, device=dev)
    off[:, 1:] = torch.cumsum(c.t(), dim=1)
    o = dict(dtype=torch.int64, device=dev)
    pad = max(total_e, 1)                     # no hops, no edges: the library refuses null edge buffers, and an empty
    fs, fe = torch.empty(total_n, **o), torch.empty(pad, **o)       # tensor's data_ptr() is null
    rc = torch.empty((2, pad), **o)
    fr, fc = rc[0], rc[1]
    so = out.struct()
    check(lib.tg_ns_homo_compact(C.byref(so), C.c_int64(n_batches), ptr(off[0]), ptr(off[1]), ptr(fs), ptr(fr), ptr(fc),
                                 ptr(fe), stream_ptr(dev)))
    if total_e == 0:
        fe, rc = fe[:0], rc[:, :0]
        fr, fc = rc[0], rc[1]
    return (fs, rc, fe) if stacked else (fs, fr, fc, fe)


class TgNsUniqueOut(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("inverse", C.c_void_p), ("rows", C.c_void_p), ("cols", C.c_void_p),
                ("counts", C.c_void_p), ("layer_nodes", C.c_void_p)]


def ns_homo_unique_form(cap_nodes, id_bound, lds_limit_bytes=0):
    """-> (form, lds_bytes, bound): the form an auto tg_ns_homo_unique call takes for slabs of pitch cap_nodes (1 = one
    workgroup per batch with the table in LDS, 2 = flat over all batches' positions), the LDS the LDS form asks for, and
    the largest cap_nodes that still takes the LDS form under the same limit (found by bisection over the same query).
    lds_limit_bytes > 0: taken as the workgroup's limit, no device is touched; otherwise the current device is asked."""
    def ask(cn):
        form, nbytes = C.c_int32(-1), C.c_int64(0)
        check(lib.tg_ns_homo_unique_form(C.c_int64(cn), C.c_int64(id_bound), C.c_int64(lds_limit_bytes), C.byref(form),
                                         C.byref(nbytes)))
        return form.value, nbytes.value
    form, nbytes = ask(cap_nodes)
    lo, hi = -1, 1 << 30                      # the form is monotone in cap_nodes: LDS up to the bound, flat above
    if ask(hi)[0] == 1:
        lo = hi
    while hi - lo > 1 and lo != hi:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ask(mid)[0] == 1 else (lo, mid)
    return form, nbytes, lo


def ns_homo_unique_workspace_bytes(cap_nodes, id_bound, n_batches):
    """-> (bytes, bytes_min): what an auto call wants for all batches at once (0 where it takes the LDS form) and the
    flat form's workspace of one batch (the least a flat call runs with, round by round)."""
    return _two_i64(lib.tg_ns_homo_unique_workspace_bytes, C.c_int64(cap_nodes), C.c_int64(id_bound), C.c_int64(n_batches))


def ns_homo_unique_workspace(cap_nodes, id_bound, n_batches, device, form=0):
    """The workspace of ns_homo_unique for n_batches batches at once as an int64 tensor; None where the call takes none
    (the LDS form).  form=2 sizes it for the flat form whatever auto would take."""
    nbytes, bmin = ns_homo_unique_workspace_bytes(cap_nodes, id_bound, n_batches)
    if form == 2:
        nbytes = bmin * n_batches
    return torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=device) if nbytes > 0 and form != 1 else None


class NsUniqueOut:
    """Output slabs of tg_ns_homo_unique for the slabs `src` (an NsBatchedOut or another object with its fields): nodes,
    inverse [n_batches, cap_nodes], rows, cols [n_batches, cap_edges] (src's own under in_place), counts [n_batches, 2],
    layer_nodes [n_batches, n_hops].  struct() is a tg_ns_out view (samples = nodes, the relabelled rows / cols, src's
    edge_index and layer_offsets, the unique counts) that ns_homo_compact accepts.  with_group: also `group`
    [n_batches, cap_nodes], the output slab of tg_ns_homo_unique_grouped (the group of every entry of nodes: PyG's `batch`)."""

    def __init__(self, src, in_place=False, with_inverse=True, with_group=False):
        self.src, self.n_batches, self.n_seeds, self.n_hops = src, src.samples.shape[0], src.n_seeds, src.n_hops
        o = dict(dtype=torch.int64, device=src.samples.device)
        self.samples = self.nodes = torch.empty_like(src.samples)
        self.group = torch.empty_like(src.samples) if with_group else None   # tg_ns_homo_unique_grouped: PyG's `batch`
        self.inverse = torch.empty_like(src.samples) if with_inverse else None
        self.rows = src.rows if in_place else torch.empty_like(src.rows)
        self.cols = src.cols if in_place else torch.empty_like(src.cols)
        if in_place:
            ns_rows_unmark(src.rows)          # the relabelled rows replace the arange: launches write the slab again
        self.edge_index, self.layer_offsets, self.states = src.edge_index, src.layer_offsets, None
        self.counts = torch.zeros((self.n_batches, 2), **o)
        self.layer_nodes = torch.zeros((self.n_batches, max(self.n_hops, 1)), **o)[:, :self.n_hops]
        self.cap_nodes, self.cap_edges = src.samples.shape[1], src.rows.shape[1]

    struct = NsBatchedOut.struct
    batch = NsBatchedOut.batch

    def unique_struct(self):
        u = TgNsUniqueOut()
        u.nodes, u.rows, u.cols, u.counts = self.nodes.data_ptr(), self.rows.data_ptr(), self.cols.data_ptr(), self.counts.data_ptr()
        u.inverse = self.inverse.data_ptr() if self.inverse is not None else None
        u.layer_nodes = self.layer_nodes.data_ptr() if self.n_hops else None
        return u

    def grouped_struct(self):
        u = TgNsUniqueGroupedOut()
        u.nodes, u.rows, u.cols, u.counts = self.nodes.data_ptr(), self.rows.data_ptr(), self.cols.data_ptr(), self.counts.data_ptr()
        u.inverse = self.inverse.data_ptr() if self.inverse is not None else None
        u.layer_nodes = self.layer_nodes.data_ptr() if self.n_hops else None
        u.group = self.group.data_ptr()
        return u


def ns_homo_unique(out, n_batches, id_bound, form=0, ws=None, in_place=False, result=None, with_inverse=True):
    """Per-batch node dedup and relabel of the first n_batches batches of `out` (an NsBatchedOut, or a NsUniqueOut-like
    object with samples / rows / cols / layer_offsets / counts slabs): tg_ns_homo_unique on the current stream, no host
    synchronisation.  id_bound: every id is in [0, id_bound).  form: 0 auto, 1 LDS, 2 flat; ws: the workspace
    (ns_homo_unique_workspace), allocated here when the call needs one and none is given; in_place: the relabelled rows /
    cols replace out's.  result: an NsUniqueOut of an earlier call on the same slabs, reused.  -> the NsUniqueOut."""
    res = result if result is not None else NsUniqueOut(out, in_place, with_inverse)
    if ws is None:
        ws = ns_homo_unique_workspace(out.samples.shape[1], id_bound, n_batches, out.samples.device, form)
    si, su = out.struct(), res.unique_struct()
    ns_rows_unmark(res.rows)                  # written through the raw pointer (under in_place: out's own slab)
    check(lib.tg_ns_homo_unique(C.byref(si), C.c_int64(n_batches), C.c_int64(out.n_seeds), C.c_int32(out.n_hops),
                                C.c_int64(id_bound), C.byref(su), ptr(ws), C.c_int64(ws.numel() * 8 if ws is not None else 0),
                                C.c_int32(form), stream_ptr(out.samples.device)))
    res._ws = ws                              # the launch borrows it: alive as long as the result
    return res


class TgNsUniqueGroupedOut(C.Structure):
    _fields_ = TgNsUniqueOut._fields_ + [("group", C.c_void_p)]


def ns_homo_unique_grouped_form(cap_nodes, id_bound, n_groups, lds_limit_bytes=0):
    """-> (form, lds_bytes): the form an auto tg_ns_homo_unique_grouped call takes for slabs of pitch cap_nodes and keys
    group * id_bound + id (1 = LDS, 2 = flat) and the LDS the LDS form asks for.  lds_limit_bytes > 0: taken as the
    workgroup's limit, no device is touched; otherwise the current device is asked."""
    form, nbytes = C.c_int32(-1), C.c_int64(0)
    check(lib.tg_ns_homo_unique_grouped_form(C.c_int64(cap_nodes), C.c_int64(id_bound), C.c_int64(n_groups),
                                             C.c_int64(lds_limit_bytes), C.byref(form), C.byref(nbytes)))
    return form.value, nbytes.value


def ns_homo_unique_grouped_workspace_bytes(cap_nodes, id_bound, n_groups, n_batches):
    """-> (bytes, bytes_min) of tg_ns_homo_unique_grouped, as ns_homo_unique_workspace_bytes: a batch's part also holds a
    group word per position."""
    return _two_i64(lib.tg_ns_homo_unique_grouped_workspace_bytes, C.c_int64(cap_nodes), C.c_int64(id_bound),
                    C.c_int64(n_groups), C.c_int64(n_batches))


def ns_homo_unique_grouped_workspace(cap_nodes, id_bound, n_groups, n_batches, device, form=0):
    """The workspace of ns_homo_unique_grouped for n_batches batches at once as an int64 tensor; None where the call takes
    none (the LDS form).  form=2 sizes it for the flat form whatever auto would take."""
    nbytes, bmin = ns_homo_unique_grouped_workspace_bytes(cap_nodes, id_bound, n_groups, n_batches)
    if form == 2:
        nbytes = bmin * n_batches
    return torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=device) if nbytes > 0 and form != 1 else None


def ns_homo_unique_grouped(out, n_batches, id_bound, seed_group=None, n_groups=None, form=0, ws=None, in_place=False,
                           result=None, with_inverse=True):
    """ns_homo_unique per GROUP of seeds (tg_ns_homo_unique_grouped; PyG's disjoint=True): seed_group, an int32 device
    tensor [out.n_seeds] with values in [0, n_groups), puts every seed in a group (None: every seed its own, n_groups =
    out.n_seeds); a node is listed once per group that reaches it, and result.group [n_batches, cap_nodes] names the group
    of every entry of result.nodes.  The other arguments and the result are ns_homo_unique's; id_bound * n_groups < 2^63."""
    if seed_group is None:
        n_groups = out.n_seeds if n_groups is None else n_groups
    else:
        if seed_group.dtype != torch.int32 or seed_group.numel() != out.n_seeds or not seed_group.is_contiguous():
            raise ValueError("seed_group must be a contiguous int32 tensor with one entry per seed (%d)" % out.n_seeds)
        if n_groups is None:
            raise ValueError("seed_group comes with n_groups")
    res = result if result is not None else NsUniqueOut(out, in_place, with_inverse, with_group=True)
    if res.group is None:
        raise ValueError("result carries no group slab: NsUniqueOut(..., with_group=True)")
    if ws is None:
        ws = ns_homo_unique_grouped_workspace(out.samples.shape[1], id_bound, n_groups, n_batches, out.samples.device, form)
    si, su = out.struct(), res.grouped_struct()
    ns_rows_unmark(res.rows)                  # written through the raw pointer (under in_place: out's own slab)
    check(lib.tg_ns_homo_unique_grouped(C.byref(si), C.c_int64(n_batches), C.c_int64(out.n_seeds), C.c_int32(out.n_hops),
                                        C.c_int64(id_bound), ptr(seed_group), C.c_int64(n_groups), C.byref(su), ptr(ws),
                                        C.c_int64(ws.numel() * 8 if ws is not None else 0), C.c_int32(form),
                                        stream_ptr(out.samples.device)))
    res._ws, res._seed_group = ws, seed_group  # the launch borrows them: alive as long as the result
    return res


class TgNsInducedIn(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("pitch_nodes", C.c_int64), ("counts", C.c_void_p), ("counts_stride", C.c_int64),
                ("node_marks", C.c_void_p), ("n_marks", C.c_int32)]


def ns_induced_workspace_bytes(graph, pitch_nodes, id_bound, n_batches):
    """-> (bytes, bytes_min): the workspace of the induced pair for n_batches batches at once (n_batches * bytes_min) and
    for one batch; graph: a tg_graph view (only n_major and n_edges are read)."""
    return _two_i64(lib.tg_ns_induced_workspace_bytes, C.byref(graph), C.c_int64(pitch_nodes), C.c_int64(id_bound),
                    C.c_int64(n_batches))


class NsInduced(_CountEmit):
    """The induced pair over the node slab `nodes` [>= n_batches, pitch] with n of batch b at
    counts.reshape(-1)[b * counts_stride]; node_marks: [n_batches, n_marks] positions or None.  Owns what the passes share:
    n_edges [n_batches], edge_marks [n_batches, n_marks], status [1] and the workspace (`ws`: an int64 tensor of an earlier
    launch of the same shape, reused when large enough).  count() then emit() run on the current stream; neither
    synchronises."""
    _struct = TgNsInducedIn

    def __init__(self, graph, nodes, counts, counts_stride, n_batches, id_bound, node_marks=None, ws=None):
        self._slabs(graph, nodes, counts, counts_stride, n_batches, id_bound, node_marks)
        self._carve(ns_induced_workspace_bytes(graph, self.struct.pitch_nodes, self.id_bound, self.n_batches)[0], ws)

    def _slabs(self, graph, nodes, counts, counts_stride, n_batches, id_bound, node_marks):
        self.graph, self.n_batches, self.id_bound = graph, int(n_batches), int(id_bound)
        self.nodes, self.counts, self.node_marks = nodes, counts, node_marks
        si = self.struct = self._struct()
        si.nodes, si.pitch_nodes = nodes.data_ptr(), nodes.shape[-1]
        si.counts, si.counts_stride = counts.data_ptr(), int(counts_stride)
        self.n_marks = 0 if node_marks is None else int(node_marks.shape[-1])
        si.node_marks, si.n_marks = (node_marks.data_ptr() if self.n_marks else None), self.n_marks

    def _carve(self, need, ws, more=()):
        # n_edges, the marks (and what a derived pair adds) and the status word in one tensor
        nb, nm = self.n_batches, self.n_marks
        self._own(need, ws, self.nodes.device, [("n_edges", nb), ("edge_marks", nb * nm)] + list(more))
        self.edge_marks = self.edge_marks.view(nb, nm)

    def _count(self, fn, stream, n_batches, *more):
        # pass 1 of either pair; more: what the grouped entry point takes between edge_marks and status
        self.live = self.n_batches if n_batches is None else int(n_batches)
        self._begin_count()
        check(fn(C.byref(self.graph), C.byref(self.struct), C.c_int64(self.live), C.c_int64(self.id_bound), ptr(self.n_edges),
                 ptr(self.edge_marks) if self.n_marks else None, *more, ptr(self.status), *self._ws_args(), stream))
        return self

    def _emit(self, fn, stream, edge_off, rows, cols, edge_index):
        check(fn(C.byref(self.graph), C.byref(self.struct), C.c_int64(self.live), C.c_int64(self.id_bound), ptr(edge_off),
                 ptr(rows), ptr(cols), ptr(edge_index), *self._ws_args(), stream))

    def count(self, n_batches=None):
        """pass 1 over the first n_batches batches (all when None); emit() then runs the same ones"""
        return self._count(lib.tg_ns_induced_count, stream_ptr(self.nodes.device), n_batches)

    def emit(self, edge_off, rows, cols, edge_index):
        """pass 2 into the caller's flat arrays; edge_off: device [n_batches], the exclusive prefix of n_edges"""
        self._emit(lib.tg_ns_induced_emit, stream_ptr(self.nodes.device), edge_off, rows, cols, edge_index)


def induced_status_check(status, who):
    """the status word of tg_ns_induced_count after its read-back: non-zero raises"""
    _status_check(status, who, ((1, "a list with repeats exceeds the chunk bound"), (2, "a node id outside the graph"),
                                (4, "a group word outside [0, n_groups)")))


CLUSTER_MAX_PARTS_PER_BATCH = 1024   # tchgeo.h TG_CLUSTER_MAX_PARTS_PER_BATCH


class TgClusterIn(C.Structure):
    _fields_ = [("partptr", C.c_void_p), ("n_parts", C.c_int64), ("clusters", C.c_void_p), ("pitch_parts", C.c_int64),
                ("n_clusters", C.c_void_p), ("node_ids", C.c_void_p)]


def cluster_workspace_bytes(graph, n_parts, pitch_parts, n_batches):
    """-> (bytes, bytes_min): the workspace of the cluster pair for n_batches batches at once (n_batches * bytes_min) and
    for one batch; graph: a tg_graph view (only n_major and n_edges are read)."""
    return _two_i64(lib.tg_cluster_workspace_bytes, C.byref(graph), C.c_int64(n_parts), C.c_int64(pitch_parts),
                    C.c_int64(n_batches))


class ClusterInduced(_CountEmit):
    """The cluster pair (tg_cluster_count / tg_cluster_emit) over the cluster lists `clusters` [>= n_batches, pitch] of the
    partition `partptr` [n_parts + 1] of `graph` (a CSC whose clusters are id ranges); n_clusters: [>= n_batches] entries
    per batch or None (the pitch each); node_ids: [n_major] what `nodes` receives for a vertex, or None.  Owns what the
    passes share: n_nodes, n_edges [n_batches each] and status [1] in one tensor `state` (a loader reads it back in one
    copy) and the workspace (`ws`: an int64 tensor of an earlier launch, reused when large enough).  count(G) then
    emit(...) run on the current stream over the first G batches; neither synchronises."""

    def __init__(self, graph, partptr, clusters, n_clusters=None, node_ids=None, ws=None):
        if clusters.dim() != 2 or clusters.dtype != torch.int64 or not clusters.is_contiguous():
            raise ValueError("ClusterInduced: clusters must be a contiguous int64 [n_batches, pitch] tensor")
        if partptr.dtype != torch.int64 or partptr.dim() != 1 or partptr.numel() < 1 or not partptr.is_contiguous():
            raise ValueError("ClusterInduced: partptr must be a contiguous int64 [n_parts + 1] tensor")
        for name, t in (("n_clusters", n_clusters), ("node_ids", node_ids)):
            if t is not None and (t.dtype != torch.int64 or not t.is_contiguous()):
                raise ValueError("ClusterInduced: %s must be a contiguous int64 tensor" % name)
        if n_clusters is not None and n_clusters.numel() < clusters.shape[0]:
            raise ValueError("ClusterInduced: n_clusters is shorter than the batches")
        if node_ids is not None and node_ids.numel() < graph.n_major:
            raise ValueError("ClusterInduced: node_ids is shorter than the graph")
        dev = clusters.device
        self.graph, self.partptr, self.clusters, self.n_clusters, self.node_ids = graph, partptr, clusters, n_clusters, node_ids
        self.n_batches = self.live = int(clusters.shape[0])
        si = self.struct = TgClusterIn()
        si.partptr, si.n_parts = partptr.data_ptr(), partptr.numel() - 1
        si.clusters, si.pitch_parts = clusters.data_ptr(), int(clusters.shape[1])
        si.n_clusters = None if n_clusters is None else n_clusters.data_ptr()
        si.node_ids = None if node_ids is None else node_ids.data_ptr()
        self._own(cluster_workspace_bytes(graph, si.n_parts, si.pitch_parts, self.n_batches)[0], ws, dev,
                  [("n_nodes", self.n_batches), ("n_edges", self.n_batches)])

    def count(self, G=None):
        """pass 1 over the first G batches (all when None); emit() then runs the same ones"""
        self.live = self.n_batches if G is None else int(G)
        if not 0 <= self.live <= self.n_batches:
            raise ValueError("ClusterInduced.count: G = %d outside [0, %d]" % (self.live, self.n_batches))
        self._begin_count()
        check(lib.tg_cluster_count(C.byref(self.graph), C.byref(self.struct), C.c_int64(self.live), ptr(self.n_nodes),
                                   ptr(self.n_edges), ptr(self.status), *self._ws_args(), stream_ptr(self.clusters.device)))
        return self

    def emit_into(self, node_off, edge_off, nodes, rows, cols, edge_index):
        """pass 2 into the caller's flat arrays; node_off / edge_off: device [n_batches], the exclusive prefixes of n_nodes
        / n_edges; nodes may be None"""
        check(lib.tg_cluster_emit(C.byref(self.graph), C.byref(self.struct), C.c_int64(self.live), ptr(node_off),
                                  ptr(edge_off), None if nodes is None else ptr(nodes), ptr(rows), ptr(cols),
                                  ptr(edge_index), *self._ws_args(), stream_ptr(self.clusters.device)))

    def emit(self, n_nodes_host=None, n_edges_host=None, with_nodes=True):
        """pass 2 of a counted launch into exact flat arrays -> (nodes [sum n_b] or None, [2, M] rows over cols, edge_index
        [M], node_off, edge_off [live + 1] as python lists).  n_nodes_host / n_edges_host: the counts already read back;
        read here (one synchronisation) when not given, together with the status word, which raises when non-zero."""
        G = self.live
        if n_nodes_host is None or n_edges_host is None:
            state = self.state.cpu()
            cluster_status_check(int(state[-1:].view(torch.int32)[0]), "ClusterInduced.emit")
            n_nodes_host = state[:G].tolist()
            n_edges_host = state[self.n_batches:self.n_batches + G].tolist()
        noff, eoff = _host_prefix(n_nodes_host), _host_prefix(n_edges_host)
        dev = self.clusters.device
        nodes = torch.empty(noff[-1], dtype=torch.int64, device=dev) if with_nodes else None
        rc = torch.empty((2, eoff[-1]), dtype=torch.int64, device=dev)
        eidx = torch.empty(eoff[-1], dtype=torch.int64, device=dev)
        if G and (noff[-1] or eoff[-1]):
            node_off = torch.cumsum(self.n_nodes[:G], 0) - self.n_nodes[:G]
            edge_off = torch.cumsum(self.n_edges[:G], 0) - self.n_edges[:G]
            self.emit_into(node_off, edge_off, nodes, rc[0], rc[1], eidx)
        return nodes, rc, eidx, noff, eoff


def cluster_status_check(status, who):
    """the status word of tg_cluster_count after its read-back: non-zero raises"""
    _status_check(status, who, ((1, "a batch with repeated clusters exceeds the chunk bound, or has 2^31 nodes or more"),
                                (2, "a cluster id outside [0, n_parts)"),
                                (4, "a partptr pair that is inverted or leaves the graph")))


class TgNsFullIn(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("node_ptr", C.c_void_p), ("max_nodes", C.c_int64), ("node_cap", C.c_int64),
                ("chunk_cap", C.c_int64)]


_P, _I64 = C.c_void_p, C.c_int64
lib.tg_ns_full_workspace_bytes.argtypes = [_P, _P, _I64, _I64, _P, _P]
lib.tg_ns_full_count.argtypes = [_P, _P, _I64, _I64, _P, _P, _P, _P, _P, _I64, _P]
lib.tg_ns_full_emit.argtypes = [_P, _P, _I64, _I64, _P, _P, _P, _P, _P, _P, _P, _I64, _P]
for _f in (lib.tg_ns_full_workspace_bytes, lib.tg_ns_full_count, lib.tg_ns_full_emit):
    _f.restype = C.c_int
NS_FULL_MAX_NODES = 1 << 30          # tchgeo.h: max_nodes and node_cap
NS_FULL_MAX_CHUNKS = 1 << 31


def _ns_full_sizes(who, graph, id_bound, max_nodes, node_cap, chunk_cap, n_batches):
    """the refusals of the full-neighbour pair that need no device, as ValueError"""
    id_bound, max_nodes, node_cap, chunk_cap, n_batches = (int(x) for x in (id_bound, max_nodes, node_cap, chunk_cap, n_batches))
    if not 0 <= max_nodes <= NS_FULL_MAX_NODES:
        raise ValueError("%s: max_nodes = %d outside [0, 2^30]" % (who, max_nodes))
    if not max_nodes <= node_cap <= NS_FULL_MAX_NODES:
        raise ValueError("%s: node_cap = %d outside [max_nodes = %d, 2^30]" % (who, node_cap, max_nodes))
    if chunk_cap > NS_FULL_MAX_CHUNKS:
        raise ValueError("%s: chunk_cap = %d above 2^31" % (who, chunk_cap))
    if not 0 <= n_batches < 2 ** 31:
        raise ValueError("%s: n_batches = %d outside [0, 2^31)" % (who, n_batches))
    if id_bound < max(1, graph.n_major):
        raise ValueError("%s: id_bound = %d below max(1, n_major = %d)" % (who, id_bound, graph.n_major))
    return id_bound, max_nodes, node_cap, chunk_cap, n_batches


def ns_full_workspace_bytes(graph, id_bound, max_nodes, node_cap, chunk_cap, n_batches):
    """-> (bytes, bytes_min): the workspace of the full-neighbour pair for n_batches batches at once (n_batches * bytes_min)
    and for one batch; graph: a tg_graph view (only n_major and n_edges are read).  No device is touched."""
    si = TgNsFullIn(None, None, int(max_nodes), int(node_cap), int(chunk_cap))
    return _two_i64(lib.tg_ns_full_workspace_bytes, C.byref(graph), C.byref(si), int(id_bound), int(n_batches))


class NsFull(_CountEmit):
    """The full-neighbour pair (tg_ns_full_count / tg_ns_full_emit) for up to n_batches frontiers of at most max_nodes nodes
    each over `graph` (a CSC view): a table for node_cap distinct nodes and room for chunk_cap chunks per batch (<= 0: the
    bound of a frontier of distinct nodes).  Owns what the passes share: n_nodes, n_edges, chunks [n_batches each] and
    status [1] in one tensor `state` (a loader reads it back in one copy) and the workspace (`ws`: an int64 tensor of an
    earlier launch, reused when large enough).  count(nodes, node_ptr) then emit(...) run on the current stream over the
    node_ptr.numel() - 1 lists; neither synchronises.  emit() consumes the workspace: count() again before another."""

    def __init__(self, graph, id_bound, max_nodes, node_cap, chunk_cap, n_batches, device, ws=None):
        self.id_bound, self.max_nodes, self.node_cap, self.chunk_cap, self.n_batches = _ns_full_sizes(
            "NsFull", graph, id_bound, max_nodes, node_cap, chunk_cap, n_batches)
        self.graph, self.device = graph, torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.struct = TgNsFullIn(None, None, self.max_nodes, self.node_cap, self.chunk_cap)
        need = ns_full_workspace_bytes(graph, self.id_bound, self.max_nodes, self.node_cap, self.chunk_cap, self.n_batches)[0]
        G = self.n_batches
        self._own(need, ws, self.device, [("n_nodes", G), ("n_edges", G), ("chunks", G)], same_device=True)
        self.live = None

    def count(self, nodes, node_ptr):
        """pass 1 over the lists nodes[node_ptr[b] : node_ptr[b + 1]] -> (n_nodes, n_edges, chunks [live each], status [1]),
        device tensors; the caller reads them back"""
        for name, t in (("nodes", nodes), ("node_ptr", node_ptr)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
                raise ValueError("NsFull.count: %s must be a contiguous flat int64 tensor" % name)
            if t.device != self.device:
                raise ValueError("NsFull.count: %s is on %s, the launch on %s" % (name, t.device, self.device))
        live = node_ptr.numel() - 1
        if not 0 <= live <= self.n_batches:
            raise ValueError("NsFull.count: node_ptr names %d lists, outside [0, %d]" % (live, self.n_batches))
        self.live, self._lists = live, (nodes, node_ptr)
        self.struct.nodes = nodes.data_ptr() if nodes.numel() else None
        self.struct.node_ptr = node_ptr.data_ptr()
        if self.max_nodes and not nodes.numel():
            self.struct.nodes = self.ws.data_ptr()       # never read: every list is empty
        self._begin_count()
        check(lib.tg_ns_full_count(C.byref(self.graph), C.byref(self.struct), live, self.id_bound, ptr(self.n_nodes),
                                   ptr(self.n_edges), ptr(self.chunks), ptr(self.status), ptr(self.ws), self.ws.numel() * 8,
                                   stream_ptr(self.device)))
        return self.n_nodes[:live], self.n_edges[:live], self.chunks[:live], self.status

    def emit(self, node_off, edge_off, nodes_out, rows, cols, edge_index):
        """pass 2 into the caller's flat arrays; node_off / edge_off: device [live], the exclusive prefixes of n_nodes /
        n_edges; nodes_out may be None"""
        if self.live is None:
            raise ValueError("NsFull.emit: no counted launch (emit() consumes the workspace: count() first)")
        for name, t in (("node_off", node_off), ("edge_off", edge_off), ("nodes_out", nodes_out), ("rows", rows),
                        ("cols", cols), ("edge_index", edge_index)):
            if t is None and name in ("nodes_out", "node_off") and nodes_out is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or not t.is_contiguous() or t.device != self.device:
                raise ValueError("NsFull.emit: %s must be a contiguous int64 tensor on %s" % (name, self.device))
        for name, t in (("node_off", node_off), ("edge_off", edge_off)):
            if t is not None and t.numel() < self.live:
                raise ValueError("NsFull.emit: %s is shorter than the %d counted lists" % (name, self.live))
        live, self.live = self.live, None
        check(lib.tg_ns_full_emit(C.byref(self.graph), C.byref(self.struct), live, self.id_bound, ptr(node_off),
                                  ptr(edge_off), ptr(nodes_out), ptr(rows), ptr(cols), ptr(edge_index), ptr(self.ws),
                                  self.ws.numel() * 8, stream_ptr(self.device)))


def ns_full_status_check(status, who):
    """the status word of tg_ns_full_count after its read-back: bit 1 raises (bit 0, a refused batch, is the caller's to
    answer with a larger workspace)"""
    _status_check(status, who, ((2, "a frontier node outside the graph"),), mask=2)


class TgNsInducedGroupedIn(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("group", C.c_void_p), ("pitch_nodes", C.c_int64), ("counts", C.c_void_p),
                ("counts_stride", C.c_int64), ("node_marks", C.c_void_p), ("n_marks", C.c_int32), ("n_groups", C.c_int64),
                ("group_time", C.c_void_p), ("window_lo", C.c_int64), ("window_hi", C.c_int64), ("chunk_cap", C.c_int64)]


def ns_induced_grouped_workspace_bytes(graph, pitch_nodes, id_bound, n_groups, chunk_cap, n_batches):
    """-> (bytes, bytes_min) of the grouped induced pair: as ns_induced_workspace_bytes with the pair key's table and room
    for chunk_cap chunks per batch (<= 0: the ungrouped bound pitch_nodes + ceil(n_edges / 512)).  No device is touched."""
    return _two_i64(lib.tg_ns_induced_grouped_workspace_bytes, C.byref(graph), C.c_int64(pitch_nodes), C.c_int64(id_bound),
                    C.c_int64(n_groups), C.c_int64(chunk_cap), C.c_int64(n_batches))


def ns_induced_default_chunk_cap(graph, pitch_nodes):
    """the capacity chunk_cap <= 0 stands for: the ungrouped pair's bound"""
    return int(pitch_nodes) + (int(graph.n_edges) + 511) // 512


class NsInducedGrouped(NsInduced):
    """The grouped induced pair (tg_ns_induced_grouped_count / _emit) over `nodes` / `group` slabs [>= n_batches, pitch]:
    NsInduced with a group word per entry, n_groups groups per batch, optional group_time [n_batches, n_groups] with
    time_window = (lo, hi) (the graph view then carries timestamps), and chunk_cap chunks of workspace per batch (None: the
    ungrouped bound).  `state` holds n_edges [n_batches], edge_marks [n_batches, n_marks], chunks [n_batches] and the status
    word, so one copy reads everything back; a batch whose chunks exceed chunk_cap has status bit 0 and n_edges 0."""
    _struct = TgNsInducedGroupedIn

    def __init__(self, graph, nodes, group, counts, counts_stride, n_batches, id_bound, n_groups, node_marks=None,
                 group_time=None, time_window=None, chunk_cap=None, ws=None):
        self._slabs(graph, nodes, counts, counts_stride, n_batches, id_bound, node_marks)
        self.n_groups, self.group, self.group_time = int(n_groups), group, group_time
        si = self.struct
        si.group, si.n_groups = group.data_ptr(), self.n_groups
        si.group_time = group_time.data_ptr() if group_time is not None else None
        if group_time is not None and time_window is None:
            raise ValueError("group_time comes with a time_window")
        si.window_lo, si.window_hi = (int(time_window[0]), int(time_window[1])) if time_window is not None else (0, 0)
        self.chunk_cap = ns_induced_default_chunk_cap(graph, si.pitch_nodes) if chunk_cap is None or chunk_cap <= 0 else int(chunk_cap)
        si.chunk_cap = self.chunk_cap
        need = ns_induced_grouped_workspace_bytes(graph, si.pitch_nodes, self.id_bound, self.n_groups, self.chunk_cap,
                                                  self.n_batches)[0]
        self._carve(need, ws, [("chunks", self.n_batches)])

    def count(self, n_batches=None):
        """pass 1 over the first n_batches batches (all when None); emit() then runs the same ones"""
        return self._count(lib.tg_ns_induced_grouped_count, stream_ptr(self.nodes.device), n_batches, ptr(self.chunks))

    def emit(self, edge_off, rows, cols, edge_index):
        """pass 2 into the caller's flat arrays; edge_off: device [n_batches], the exclusive prefix of n_edges"""
        self._emit(lib.tg_ns_induced_grouped_emit, stream_ptr(self.nodes.device), edge_off, rows, cols, edge_index)

    def chunks_of(self, state_host):
        """the chunk counts inside a host copy of `state`"""
        nb, nm = self.n_batches, self.n_marks
        return state_host[nb * (1 + nm):nb * (2 + nm)].tolist()

    def grown(self, chunk_cap):
        """a launch object over the same slabs with room for chunk_cap chunks per batch"""
        return NsInducedGrouped(self.graph, self.nodes, self.group, self.counts, self.struct.counts_stride, self.n_batches,
                                self.id_bound, self.n_groups, self.node_marks, self.group_time,
                                (self.struct.window_lo, self.struct.window_hi), chunk_cap)


def ns_induced_count(graph, nodes, counts, counts_stride, n_batches, id_bound, node_marks=None, ws=None):
    """tg_ns_induced_count on the current stream -> the NsInduced launch (n_edges, edge_marks, status on the device)."""
    return NsInduced(graph, nodes, counts, counts_stride, n_batches, id_bound, node_marks, ws).count()


def ns_induced_emit(launch, n_edges_host=None):
    """tg_ns_induced_emit of a counted launch into exact flat arrays -> ([2, M] rows over cols, edge_index [M], edge_off
    [n_batches + 1] as a python list).  n_edges_host: the counts already read back; read here (one synchronisation) when
    not given, together with the status word, which raises when non-zero."""
    if n_edges_host is None:
        state = launch.state.cpu()
        induced_status_check(int(state[-1:].view(torch.int32)[0]), "ns_induced_emit")
        n_edges_host = state[:launch.n_batches].tolist()
    off = _host_prefix(n_edges_host)
    dev = launch.nodes.device
    rc = torch.empty((2, off[-1]), dtype=torch.int64, device=dev)
    eidx = torch.empty(off[-1], dtype=torch.int64, device=dev)
    if off[-1]:
        edge_off = torch.cumsum(launch.n_edges, 0) - launch.n_edges
        launch.emit(edge_off, rc[0], rc[1], eidx)
    return rc, eidx, off


class TgSaintRwOut(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("pitch_nodes", C.c_int64), ("counts", C.c_void_p), ("counts_stride", C.c_int64)]


def saint_rw_capacity(batch_size, walk_length):
    """-> positions of a mini-batch, batch_size * (walk_length + 1): the least pitch of tg_saint_rw_nodes' node slab."""
    positions = C.c_int64(-1)
    check(lib.tg_saint_rw_capacity(C.c_int64(batch_size), C.c_int64(walk_length), C.byref(positions)))
    return positions.value


def saint_rw_form(batch_size, walk_length, lds_limit_bytes=0):
    """-> (form, lds_bytes): the form an auto tg_saint_rw_nodes call takes (1 = one workgroup per mini-batch with the table
    in LDS, 2 = flat through a workspace) and the LDS the LDS form asks for.  lds_limit_bytes > 0: taken as the workgroup's
    limit, no device is touched; otherwise the current device is asked."""
    form, nbytes = C.c_int32(-1), C.c_int64(0)
    check(lib.tg_saint_rw_form(C.c_int64(batch_size), C.c_int64(walk_length), C.c_int64(lds_limit_bytes), C.byref(form),
                               C.byref(nbytes)))
    return form.value, nbytes.value


def saint_rw_workspace_bytes(n_batches, batch_size, walk_length, form=0):
    """-> (bytes, bytes_min): the workspace of n_batches mini-batches at once in this form (0: the one auto takes on the
    current device; 0 bytes for the LDS form) and of one mini-batch of the flat form, the least a flat call runs with."""
    return _two_i64(lib.tg_saint_rw_workspace_bytes, C.c_int64(n_batches), C.c_int64(batch_size), C.c_int64(walk_length),
                    C.c_int32(form))


def saint_rw_nodes(graph, roots, walk_length, seed, call_id, form=0, ws=None, out=None, status=None):
    """GraphSAINT's random-walk node lists (tg_saint_rw_nodes) of the G mini-batches roots[G, B] in one launch on the current
    stream -> (nodes [G, pitch], counts [G]): nodes[g, :counts[g]] = the distinct vertices the walks of roots[g] visit
    (walk_length uniform steps over the CSR `graph`, call id call_id + g), first visit first; words past counts[g] are not
    written.  form: 0 auto, 1 LDS, 2 flat; ws: the flat form's workspace (an int64 tensor; from bytes_min up it runs in
    rounds), allocated here when needed and not given; out: (nodes [G, pitch >= B * (walk_length + 1)], counts [G]) of an
    earlier call, reused; status: a zeroed device int32 word, bit 1 (value 2) = a root outside the graph (allocated here
    when not given; not read back)."""
    if roots.dim() != 2 or roots.dtype != torch.int64 or not roots.is_contiguous():
        raise ValueError("saint_rw_nodes: roots must be a contiguous int64 [n_batches, batch_size] tensor")
    G, B = roots.shape
    dev = roots.device
    P = saint_rw_capacity(B, walk_length)
    if out is None:
        out = (torch.empty((G, P), dtype=torch.int64, device=dev), torch.empty(G, dtype=torch.int64, device=dev))
    nodes, counts = out
    if nodes.dim() != 2 or nodes.shape[0] < G or nodes.stride(1) != 1 or counts.dim() != 1 or counts.numel() < G \
            or nodes.dtype != torch.int64 or counts.dtype != torch.int64:
        raise ValueError("saint_rw_nodes: out must be (int64 nodes [>= n_batches, pitch], int64 counts [>= n_batches])")
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    need = saint_rw_workspace_bytes(G, B, walk_length, form)[0]
    if need and ws is None:
        ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    o = TgSaintRwOut(nodes.data_ptr(), nodes.stride(0), counts.data_ptr(), counts.stride(0))
    rng = TgRng(seed, call_id)
    check(lib.tg_saint_rw_nodes(C.byref(graph), ptr(roots), C.c_int64(G), C.c_int64(B), C.c_int64(walk_length), C.byref(rng),
                                C.byref(o), ptr(status), ptr(ws), C.c_int64(ws.numel() * ws.element_size() if ws is not None else 0),
                                C.c_int32(form), stream_ptr(dev)))
    return nodes, counts


def saint_coverage_add(nodes, counts, node_count, edge_count, edge_ids=None, status=None, n_batches=None):
    """GraphSAINT's coverage counters (tg_saint_coverage_add) on the current stream: node_count[v] += 1 for every node of
    nodes[g, :counts[g]], g < n_batches (all rows when None), edge_count[e] += 1 for every entry of the flat edge_ids (CSC
    offsets, or None).  Both tables are int64 device tensors the caller zeroed.  -> status: a device int32 word (the one
    given, else a fresh zeroed one), bit 1 (value 2) = an id outside its table was skipped."""
    dev = node_count.device
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    G = nodes.shape[0] if n_batches is None else int(n_batches)
    n_ids = 0 if edge_ids is None else edge_ids.numel()
    if edge_ids is not None:
        edge_ids = edge_ids.contiguous()
    check(lib.tg_saint_coverage_add(ptr(nodes), C.c_int64(nodes.stride(0)), ptr(counts), C.c_int64(counts.stride(0)),
                                    C.c_int64(G), ptr(edge_ids) if n_ids else None, C.c_int64(n_ids), ptr(node_count),
                                    C.c_int64(node_count.numel()), ptr(edge_count), C.c_int64(edge_count.numel()),
                                    ptr(status), stream_ptr(dev)))
    return status


def saint_norm(graph, node_count, edge_count, n_samples):
    """GraphSAINT's normalisation vectors (tg_saint_norm) of n_samples pre-sampled mini-batches over the CSC `graph` ->
    (node_norm [n_major], edge_norm [n_edges], float32, edge_norm in CSC order)."""
    dev = node_count.device
    node_norm = torch.empty(graph.n_major, dtype=torch.float32, device=dev)
    edge_norm = torch.empty(graph.n_edges, dtype=torch.float32, device=dev)
    check(lib.tg_saint_norm(C.byref(graph), ptr(node_count), ptr(edge_count), C.c_int64(n_samples),
                            ptr(node_norm) if graph.n_major else None, ptr(edge_norm) if graph.n_edges else None,
                            stream_ptr(dev)))
    return node_norm, edge_norm


class TgSaintEdgeIn(C.Structure):
    _fields_ = [("csc", C.POINTER(TgGraph)), ("cols", C.c_void_p), ("n_cols", C.c_int64),
                ("csr", C.POINTER(TgGraph)), ("rows", C.c_void_p), ("n_rows", C.c_int64)]


def saint_ne_form(positions, lds_limit_bytes=0):
    """-> (form, lds_bytes): the form an auto tg_saint_node_nodes / tg_saint_edge_nodes call of `positions` positions per
    mini-batch takes (batch_size for the node sampler, 2 * batch_size for the edge sampler; 1 = one workgroup per
    mini-batch with the table in LDS, 2 = flat through a workspace) and the LDS the LDS form asks for.  lds_limit_bytes > 0:
    taken as the workgroup's limit, no device is touched; otherwise the current device is asked."""
    form, nbytes = C.c_int32(-1), C.c_int64(0)
    check(lib.tg_saint_ne_form(C.c_int64(positions), C.c_int64(lds_limit_bytes), C.byref(form), C.byref(nbytes)))
    return form.value, nbytes.value


def saint_ne_workspace_bytes(n_batches, positions, form=0):
    """-> (bytes, bytes_min): the workspace of n_batches mini-batches of `positions` positions at once in this form (0: the
    one auto takes on the current device; 0 bytes for the LDS form) and of one mini-batch of the flat form, the least a
    flat call runs with."""
    return _two_i64(lib.tg_saint_ne_workspace_bytes, C.c_int64(n_batches), C.c_int64(positions), C.c_int32(form))


def _saint_ne_buffers(who, dev, G, P, form, ws, out, status):
    """the output pair, the status word and the workspace of a tg_saint_node_nodes / tg_saint_edge_nodes call"""
    if out is None:
        out = (torch.empty((G, P), dtype=torch.int64, device=dev), torch.empty(G, dtype=torch.int64, device=dev))
    nodes, counts = out
    if nodes.dim() != 2 or nodes.shape[0] < G or nodes.stride(1) != 1 or counts.dim() != 1 or counts.numel() < G \
            or nodes.dtype != torch.int64 or counts.dtype != torch.int64:
        raise ValueError("%s: out must be (int64 nodes [>= n_batches, pitch], int64 counts [>= n_batches])" % who)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    need = saint_ne_workspace_bytes(G, P, form)[0]
    if need and ws is None:
        ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    o = TgSaintRwOut(nodes.data_ptr(), nodes.stride(0), counts.data_ptr(), counts.stride(0))
    return nodes, counts, o, status, ws, C.c_int64(ws.numel() * ws.element_size() if ws is not None else 0)


def saint_node_nodes(graph, batch_size, n_batches, seed, call_id, id_bound=None, form=0, ws=None, out=None, status=None):
    """GraphSAINT's node sampler (tg_saint_node_nodes): G = n_batches mini-batches in one launch on the current stream ->
    (nodes [G, pitch], counts [G]).  Slot i < batch_size of mini-batch g picks an entry of `graph` uniformly (call id
    call_id + g) and visits indices[entry]: given the CSC a source with probability out-degree / E, given the CSR a target
    with probability in-degree / E.  nodes[g, :counts[g]] = the distinct visited vertices, first visit first; words past
    counts[g] are not written.  id_bound: ids are in [0, id_bound) (None: graph.n_major, a square graph); form, ws, out,
    status as saint_rw_nodes (status bit 1, value 2 = a vertex outside [0, id_bound)).  `graph` is a graph_view: buffers
    are allocated where its indices live."""
    G, B = int(n_batches), int(batch_size)
    dev = out[0].device if out is not None else graph._keep[1].device
    nodes, counts, o, status, ws, ws_bytes = _saint_ne_buffers("saint_node_nodes", dev, G, B, form, ws, out, status)
    rng = TgRng(seed, call_id)
    check(lib.tg_saint_node_nodes(C.byref(graph), C.c_int64(graph.n_major if id_bound is None else id_bound), C.c_int64(G),
                                  C.c_int64(B), C.byref(rng), C.byref(o), ptr(status), ptr(ws), ws_bytes, C.c_int32(form),
                                  stream_ptr(dev)))
    return nodes, counts


def saint_edge_nodes(csc, cols, csr, rows, batch_size, n_batches, seed, call_id, id_bound=None, form=0, ws=None, out=None,
                     status=None):
    """GraphSAINT's edge sampler (tg_saint_edge_nodes): G = n_batches mini-batches of batch_size EDGES in one launch on the
    current stream -> (nodes [G, pitch >= 2 * batch_size], counts [G]).  Slot i picks an entry of the concatenated lists
    cols (columns of `csc`) | rows (rows of `csr`; csr = rows = None: columns only) and then a uniform entry of that column
    / row; with the lists = the non-empty columns and rows of one graph the edge (u -> v) is drawn with probability
    (1 / deg_in(v) + 1 / deg_out(u)) / (len(cols) + len(rows)).  Draws are independent, with replacement (PyG takes a
    Gumbel top-k over all edges per mini-batch).  The source sits at position i, the target at batch_size + i;
    nodes[g, :counts[g]] = the distinct ends, first position first.  status: bit 1 (value 2) = a listed major outside its
    graph or an end >= id_bound (None: csc.n_major), bit 2 (value 4) = a listed major without entries; form, ws, out as
    saint_rw_nodes."""
    G, B = int(n_batches), int(batch_size)
    for name, t in (("cols", cols), ("rows", rows)):
        if t is not None and (t.dim() != 1 or t.dtype != torch.int64 or not t.is_contiguous()):
            raise ValueError("saint_edge_nodes: %s must be a contiguous int64 vector" % name)
    if (csr is None) != (rows is None):
        raise ValueError("saint_edge_nodes: csr and rows go together")
    dev = cols.device
    nodes, counts, o, status, ws, ws_bytes = _saint_ne_buffers("saint_edge_nodes", dev, G, 2 * B, form, ws, out, status)
    arg = TgSaintEdgeIn(C.pointer(csc), cols.data_ptr(), cols.numel(), C.pointer(csr) if csr is not None else None,
                        rows.data_ptr() if rows is not None else None, rows.numel() if rows is not None else 0)
    rng = TgRng(seed, call_id)
    check(lib.tg_saint_edge_nodes(C.byref(arg), C.c_int64(csc.n_major if id_bound is None else id_bound), C.c_int64(G),
                                  C.c_int64(B), C.byref(rng), C.byref(o), ptr(status), ptr(ws), ws_bytes, C.c_int32(form),
                                  stream_ptr(dev)))
    return nodes, counts


class TgNsTypedIn(C.Structure):
    _fields_ = [("n_types", C.c_int32), ("n_rels", C.c_int32), ("rel_src", C.POINTER(C.c_int32)),
                ("rel_dst", C.POINTER(C.c_int32)), ("samples", C.POINTER(C.c_void_p)), ("pitch_nodes", C.POINTER(C.c_int64)),
                ("rows", C.POINTER(C.c_void_p)), ("cols", C.POINTER(C.c_void_p)), ("pitch_edges", C.POINTER(C.c_int64)),
                ("counts", C.c_void_p), ("counts_stride", C.c_int64), ("n_inputs", C.POINTER(C.c_int64)),
                ("id_bound", C.POINTER(C.c_int64))]


class TgNsTypedUniqueOut(C.Structure):
    _fields_ = [("nodes", C.POINTER(C.c_void_p)), ("inverse", C.POINTER(C.c_void_p)), ("rows", C.POINTER(C.c_void_p)),
                ("cols", C.POINTER(C.c_void_p)), ("counts", C.c_void_p), ("seed_counts", C.c_void_p)]


def ns_typed_unique_form(pitch_nodes, id_bounds, lds_limit_bytes=0):
    """-> (form, lds_bytes): the form an auto tg_ns_typed_unique call takes for node slabs of these pitches (1 = one
    workgroup per batch with the table and every type's per-position words in LDS, 2 = flat over all batches' positions)
    and the LDS the LDS form asks for.  lds_limit_bytes > 0: taken as the workgroup's limit, no device is touched;
    otherwise the current device is asked."""
    form, nbytes = C.c_int32(-1), C.c_int64(0)
    check(lib.tg_ns_typed_unique_form(C.c_int32(len(pitch_nodes)), _i64(pitch_nodes), _i64(id_bounds),
                                      C.c_int64(lds_limit_bytes), C.byref(form), C.byref(nbytes)))
    return form.value, nbytes.value


def ns_typed_unique_workspace_bytes(pitch_nodes, id_bounds, n_batches):
    """-> (bytes, bytes_min): what an auto call wants for all batches at once (0 where it takes the LDS form) and the
    flat form's workspace of one batch (the least a flat call runs with, round by round)."""
    return _two_i64(lib.tg_ns_typed_unique_workspace_bytes, C.c_int32(len(pitch_nodes)), _i64(pitch_nodes), _i64(id_bounds),
                    C.c_int64(n_batches))


class NsTypedUniqueOut:
    """Output slabs of tg_ns_typed_unique for the typed slabs `src` (an NsHeteroBatched, or another object with its
    fields: T, R, rel_src, rel_dst, n_inputs, per-type `samples`, per-relation `rows` / `cols` / `edge_index`, `counts`
    [n_batches, >= T + R]): per type nodes and inverse, per relation rows and cols (src's own under in_place), counts (src's
    row pitch, the unique node counts and the edge counts) and seed_counts [n_batches, T].  counts and seed_counts share one
    tensor (`state`), so read_state() fetches both in one read-back.  It reads like the slabs it was made from -- samples
    (= nodes), rows, cols, edge_index, counts, layer_offsets -- so a loader flattens either."""

    def __init__(self, src, in_place=False, with_inverse=True):
        self.T, self.R, self.in_place = src.T, src.R, in_place
        self.nb, self.stride = src.counts.shape[0], src.counts.shape[1]
        self.samples = self.nodes = [torch.empty_like(x) for x in src.samples]
        self.inverse = [torch.empty_like(x) for x in src.samples] if with_inverse else None
        self.rows = self.cols = None
        self.rebind(src)
        self.state = torch.zeros(self.nb * (self.stride + self.T), dtype=torch.int64, device=src.counts.device)
        self.counts = self.state[:self.nb * self.stride].view(self.nb, self.stride)
        self.seed_counts = self.state[self.nb * self.stride:].view(self.nb, self.T)
        self._ws = None

    def rebind(self, src):
        """Takes other source slabs of the same shapes: nodes, inverse and the state tensor are kept (every word a launch
        hands out is written by that launch), and so are rows / cols unless they are the source's own (in_place)."""
        if [x.shape for x in src.samples] != [x.shape for x in self.nodes] or src.counts.shape != (self.nb, self.stride):
            raise ValueError("NsTypedUniqueOut.rebind: the slabs differ in shape")
        self.src = src
        if self.in_place or self.rows is None:
            self.rows = src.rows if self.in_place else [torch.empty_like(x) for x in src.rows]
            self.cols = src.cols if self.in_place else [torch.empty_like(x) for x in src.cols]
        self.edge_index, self.layer_offsets = src.edge_index, getattr(src, "layer_offsets", None)
        return self

    def read_state(self):
        """ONE read-back -> (counts [n_batches, stride], seed_counts [n_batches, T]) as host tensors."""
        h = self.state.cpu()
        n = self.nb * self.stride
        return h[:n].view(self.nb, self.stride), h[n:].view(self.nb, self.T)

    def structs(self, id_bounds):
        """-> (tg_ns_typed_in, tg_ns_typed_unique_out); the arrays they borrow stay alive on self."""
        src = self.src
        pitch_n, pitch_e = _i64([x.shape[1] for x in src.samples]), _i64([x.shape[1] for x in src.rows])
        arrays = [_vp(src.samples), _vp(src.rows), _vp(src.cols), _vp(self.nodes), _vp(self.rows), _vp(self.cols),
                  _vp(self.inverse) if self.inverse is not None else None, pitch_n, pitch_e, _i64(id_bounds),
                  _i64(list(src.n_inputs)[:self.T])]
        rel = [(C.c_int32 * max(self.R, 1))(*list(x)[:self.R]) for x in (src.rel_src, src.rel_dst)]
        arrays += rel
        si = TgNsTypedIn(self.T, self.R, rel[0], rel[1], arrays[0], pitch_n, arrays[1], arrays[2], pitch_e,
                         src.counts.data_ptr(), self.stride, arrays[10], arrays[9])
        so = TgNsTypedUniqueOut(arrays[3], arrays[6], arrays[4], arrays[5], self.counts.data_ptr(),
                                self.seed_counts.data_ptr())
        self._arrays = arrays
        return si, so


def ns_typed_unique(slabs, n_batches, id_bounds, form=0, ws=None, in_place=False, result=None, with_inverse=True):
    """Per-batch, per-type node dedup and relabel of the first n_batches batches of the typed slabs `slabs` (an
    NsHeteroBatched or a look-alike, see NsTypedUniqueOut): tg_ns_typed_unique on the current stream, no host
    synchronisation.  id_bounds: per node type, every id of the type is in [0, id_bounds[t]).  form: 0 auto, 1 LDS, 2 flat;
    ws: the workspace (an int64 tensor of ns_typed_unique_workspace_bytes), allocated here when the call needs one and none
    is given.  result: a NsTypedUniqueOut on the same slabs (else one is made from in_place / with_inverse).
    -> the NsTypedUniqueOut."""
    res = result if result is not None else NsTypedUniqueOut(slabs, in_place, with_inverse)
    dev = slabs.counts.device
    if ws is None and form != 1:
        pitches = [x.shape[1] for x in slabs.samples]
        nbytes, bmin = ns_typed_unique_workspace_bytes(pitches, id_bounds, n_batches)
        if form == 2:
            nbytes = bmin * n_batches
        ws = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=dev) if nbytes > 0 else None
    si, so = res.structs(id_bounds)
    check(lib.tg_ns_typed_unique(C.byref(si), C.c_int64(n_batches), C.byref(so), ptr(ws),
                                 C.c_int64(ws.numel() * 8 if ws is not None else 0), C.c_int32(form), stream_ptr(dev)))
    res._ws = ws                              # the launch borrows it: alive as long as the result
    return res


def compact_rows(slab, lens, total):
    """Flat concatenation of slab[r, :lens[r]] (slab: [n_rows, pitch] int64; lens: device view, any stride; total: their
    sum, known to the host)."""
    n_rows = slab.shape[0]
    off = torch.cumsum(lens, 0) - lens
    dst = torch.empty(int(total), dtype=torch.int64, device=slab.device)
    check(lib.tg_compact_rows(ptr(slab), C.c_int64(slab.stride(0)), ptr(lens), C.c_int64(lens.stride(0) if lens.dim() else 1),
                              ptr(off), C.c_int64(n_rows), ptr(dst), stream_ptr(slab.device)))
    return dst


def gather_rows(src, index, status=None):
    """dst[i] = src[index[i]] over dim 0 (tg_gather_rows).  `src` may be strided over dim 0 only.  Returns
    (dst, status): status is a device int32 word, 1 when an index fell outside [0, src.shape[0])."""
    dev = src.device
    if src.dim() == 0:
        raise ValueError("gather_rows needs at least one dimension")
    inner = src[0].is_contiguous() if src.shape[0] else True
    if not inner or (src.dim() > 1 and src.shape[0] > 1 and src.stride(0) < src[0].numel()):
        src = src.contiguous()
    row_elems = 1
    for d in src.shape[1:]:
        row_elems *= d
    item = src.element_size()
    stride = src.stride(0) * item if src.shape[0] > 1 else row_elems * item
    index = index.contiguous()
    dst = torch.empty((index.numel(),) + tuple(src.shape[1:]), dtype=src.dtype, device=dev)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib.tg_gather_rows(C.c_void_p(src.data_ptr()), C.c_int64(src.shape[0]), C.c_int64(row_elems * item),
                             C.c_int64(max(stride, row_elems * item)), ptr(index), C.c_int64(index.numel()),
                             C.c_void_p(dst.data_ptr()), C.c_void_p(status.data_ptr()), stream_ptr(dev)))
    return dst, status


def probe_random_gather(table, n_threads, per_thread, seed=1):
    sink = torch.empty(n_threads, dtype=torch.int64, device=table.device)
    check(lib.tg_probe_random_gather(ptr(table), C.c_int64(table.numel()), C.c_int64(n_threads),
                                     C.c_int64(per_thread), C.c_uint64(seed), ptr(sink), stream_ptr(table.device)))
    return sink


def probe_ns_sol(src, dst, seeds, n_hops):
    """The algorithmic bytes of the finished launch `src` moved as pure streams into `dst` (tg_probe_ns_sol)."""
    sink = torch.zeros(seeds.shape[0], dtype=torch.int64, device=seeds.device)
    a, b = src.struct(), dst.struct()
    ns_rows_unmark(dst.rows)                  # the probe copies src's streams over dst's
    check(lib.tg_probe_ns_sol(C.byref(a), C.byref(b), ptr(seeds), C.c_int64(seeds.shape[0]), C.c_int64(seeds.shape[1]),
                              C.c_int32(n_hops), ptr(sink), stream_ptr(seeds.device)))
    return sink


def ns_hop(graph, vertices, fanout, seed, call_id=0, sampler=SAMPLER_UNIFORM, ids=None, call_ids=None, id_base=0,
           rng_tag=0):
    """One flat hop (tg_ns_hop).  -> (cnt[m], offsets[m+1], neighbors, edge_ptrs, parents), the last three sized
    m*fanout with offsets[m] valid entries; no host synchronisation."""
    m, dev = vertices.numel(), vertices.device
    o = dict(dtype=torch.int64, device=dev)
    cnt, offsets = torch.empty(max(m, 1), **o), torch.empty(m + 1, **o)
    nbr, ep, par = (torch.empty(max(m * fanout, 1), **o) for _ in range(3))
    hin, hout = TgHopIn(), TgHopOut()
    hin.vertices = vertices.data_ptr() if m else None
    hin.ids = ids.data_ptr() if ids is not None else None
    hin.call_ids = call_ids.data_ptr() if call_ids is not None else None
    hin.m, hin.id_base, hin.fanout, hin.sampler, hin.rng_tag = m, id_base, fanout, sampler, rng_tag
    hout.cnt, hout.offsets = cnt.data_ptr(), offsets.data_ptr()
    hout.neighbors, hout.edge_ptrs, hout.parents = nbr.data_ptr(), ep.data_ptr(), par.data_ptr()
    nbytes = C.c_int64(0)
    check(lib.tg_ns_hop_workspace_bytes(C.c_int64(m), C.byref(nbytes)))
    ws = torch.empty(nbytes.value // 8 + 1, **o)
    rng = TgRng(seed, call_id)
    check(lib.tg_ns_hop(C.byref(graph), C.byref(hin), C.byref(rng), C.byref(hout), ptr(ws), C.c_int64(nbytes.value),
                        stream_ptr(dev)))
    return cnt[:m], offsets, nbr, ep, par


def ns_hop_segments(segments, vertices, states, seed, filter_mode=FILTER_NONE, window=(0, 0), forward=False, call_id=0,
                    sampler=SAMPLER_UNIFORM, ids=None, call_ids=None, id_base=0, layout=None, group_cap=None):
    """One flat hop over a frontier made of segments (tg_ns_hop_segments).  segments: list of (graph view, begin,
    fanout, rng_tag); layout: optional device tensor [len(segments) + 1] = real segment starts, then the real length.
    -> (cnt[m], offsets[m+1], neighbors, edge_ptrs, parents, states_out, status) -- no host synchronisation."""
    m, dev = vertices.numel(), vertices.device
    o = dict(dtype=torch.int64, device=dev)
    kmax = max(f for _, _, f, _ in segments)
    if group_cap is None:
        group_cap = max(1024, sum(g.n_edges for g, _, _, _ in segments) // 512 + 2 * m + 2)
    cnt, offsets = torch.empty(max(m, 1), **o), torch.empty(m + 1, **o)
    nbr, ep, par, st_out = (torch.empty(max(m * kmax, 1), **o) for _ in range(4))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    segs = (TgHopSegment * len(segments))()
    for j, (g, begin, fanout, tag) in enumerate(segments):
        segs[j].graph, segs[j].begin, segs[j].fanout, segs[j].rng_tag = C.addressof(g), begin, fanout, tag
    hin, hout, flt = TgHopIn(), TgHopOut(), TgHopFilter()
    hin.vertices = vertices.data_ptr() if m else None
    hin.ids = ids.data_ptr() if ids is not None else None
    hin.call_ids = call_ids.data_ptr() if call_ids is not None else None
    hin.m, hin.id_base, hin.fanout, hin.sampler, hin.rng_tag = m, id_base, kmax, sampler, 0
    hout.cnt, hout.offsets = cnt.data_ptr(), offsets.data_ptr()
    hout.neighbors, hout.edge_ptrs, hout.parents = nbr.data_ptr(), ep.data_ptr(), par.data_ptr()
    flt.filter_mode, flt.forward = filter_mode, int(bool(forward))
    flt.win_lo, flt.win_hi = window
    flt.states = states.data_ptr() if (m and states is not None) else None
    nbytes = C.c_int64(0)
    size_of = lib.tg_ns_hop_weighted_workspace_bytes if sampler == SAMPLER_WEIGHTED else lib.tg_ns_hop_scan_workspace_bytes
    check(size_of(C.c_int64(m), C.c_int32(kmax), C.c_int64(group_cap), C.byref(nbytes)))
    ws = torch.empty(nbytes.value // 8 + 1, **o)
    rng = TgRng(seed, call_id)
    check(lib.tg_ns_hop_segments(segs, C.c_int32(len(segments)), C.byref(hin), ptr(layout) if layout is not None else None,
                                 C.byref(flt), C.byref(rng), C.byref(hout), ptr(st_out), ptr(status), ptr(ws),
                                 C.c_int64(nbytes.value), C.c_int64(group_cap), stream_ptr(dev)))
    return cnt[:m], offsets, nbr, ep, par, st_out, status


def ns_hop_scan(graph, vertices, states, fanout, seed, filter_mode, window, forward=False, call_id=0,
                sampler=SAMPLER_UNIFORM, ids=None, call_ids=None, id_base=0, rng_tag=0, group_cap=None):
    """One flat hop under a temporal filter (tg_ns_hop_scan).
    -> (cnt[m], offsets[m+1], neighbors, edge_ptrs, parents, states_out, status) -- no host synchronisation."""
    m, dev = vertices.numel(), vertices.device
    o = dict(dtype=torch.int64, device=dev)
    if group_cap is None:
        group_cap = max(1024, graph.n_edges // 512 + 2 * m + 2)
    cnt, offsets = torch.empty(max(m, 1), **o), torch.empty(m + 1, **o)
    nbr, ep, par, st_out = (torch.empty(max(m * fanout, 1), **o) for _ in range(4))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    hin, hout, flt = TgHopIn(), TgHopOut(), TgHopFilter()
    hin.vertices = vertices.data_ptr() if m else None
    hin.ids = ids.data_ptr() if ids is not None else None
    hin.call_ids = call_ids.data_ptr() if call_ids is not None else None
    hin.m, hin.id_base, hin.fanout, hin.sampler, hin.rng_tag = m, id_base, fanout, sampler, rng_tag
    hout.cnt, hout.offsets = cnt.data_ptr(), offsets.data_ptr()
    hout.neighbors, hout.edge_ptrs, hout.parents = nbr.data_ptr(), ep.data_ptr(), par.data_ptr()
    flt.filter_mode, flt.forward = filter_mode, int(bool(forward))
    flt.win_lo, flt.win_hi = window
    flt.states = states.data_ptr() if m else None
    nbytes = C.c_int64(0)
    check(lib.tg_ns_hop_scan_workspace_bytes(C.c_int64(m), C.c_int32(fanout), C.c_int64(group_cap), C.byref(nbytes)))
    ws = torch.empty(nbytes.value // 8 + 1, **o)
    rng = TgRng(seed, call_id)
    check(lib.tg_ns_hop_scan(C.byref(graph), C.byref(hin), C.byref(flt), C.byref(rng), C.byref(hout), ptr(st_out),
                             ptr(status), ptr(ws), C.c_int64(nbytes.value), C.c_int64(group_cap), stream_ptr(dev)))
    return cnt[:m], offsets, nbr, ep, par, st_out, status


def ns_hop_recent(graph, vertices, fanout, states=None, filter_mode=FILTER_NONE, window=(0, 0), forward=False):
    """One flat hop of the most-recent-k sampler (tg_ns_hop_recent; the graph view carries the edge timestamps).  `states`
    [m] is the filter state of every frontier vertex (None without a filter; `forward` then still picks the direction).
    -> (cnt[m], offsets[m+1], neighbors, edge_ptrs, parents, states_out or None) -- no host synchronisation."""
    m, dev = vertices.numel(), vertices.device
    o = dict(dtype=torch.int64, device=dev)
    cnt, offsets = torch.empty(max(m, 1), **o), torch.empty(m + 1, **o)
    nbr, ep, par = (torch.empty(max(m * fanout, 1), **o) for _ in range(3))
    st_out = torch.empty(max(m * fanout, 1), **o) if filter_mode != FILTER_NONE else None
    hin, hout, flt = TgHopIn(), TgHopOut(), TgHopFilter()
    hin.vertices = vertices.data_ptr() if m else None
    hin.m, hin.fanout, hin.sampler = m, fanout, SAMPLER_RECENT
    hout.cnt, hout.offsets = cnt.data_ptr(), offsets.data_ptr()
    hout.neighbors, hout.edge_ptrs, hout.parents = nbr.data_ptr(), ep.data_ptr(), par.data_ptr()
    flt.filter_mode, flt.forward = filter_mode, int(bool(forward))
    flt.win_lo, flt.win_hi = window
    flt.states = states.data_ptr() if (m and states is not None) else None
    check(lib.tg_ns_hop_recent(C.byref(graph), C.byref(hin), C.byref(flt), C.byref(hout), ptr(st_out), stream_ptr(dev)))
    return cnt[:m], offsets, nbr, ep, par, st_out


def ns_hop_labor(graph, vertices, fanout, seed, call_id, layer=0, call_ids=None, states=None, filter_mode=FILTER_NONE,
                 window=(0, 0), forward=False, sampler=SAMPLER_LABOR, rng_tag=0):
    """One flat hop of layer-neighbor sampling (tg_ns_hop_labor): every frontier vertex keeps the `fanout` admitted edges
    whose neighbours have the smallest variates of (seed, call id, layer).  `call_ids` [m] names a call id per frontier
    vertex (else `call_id`); `states` [m] is the filter state (None without a filter).
    -> (cnt[m], offsets[m+1], neighbors, edge_ptrs, parents, states_out or None) -- no host synchronisation."""
    m, dev = vertices.numel(), vertices.device
    o = dict(dtype=torch.int64, device=dev)
    cnt, offsets = torch.empty(max(m, 1), **o), torch.empty(m + 1, **o)
    nbr, ep, par = (torch.empty(max(m * fanout, 1), **o) for _ in range(3))
    st_out = torch.empty(max(m * fanout, 1), **o) if filter_mode != FILTER_NONE else None
    hin, hout, flt = TgHopIn(), TgHopOut(), TgHopFilter()
    hin.vertices = vertices.data_ptr() if m else None
    hin.call_ids = call_ids.data_ptr() if call_ids is not None else None
    hin.m, hin.fanout, hin.sampler, hin.rng_tag = m, fanout, sampler, rng_tag
    hout.cnt, hout.offsets = cnt.data_ptr(), offsets.data_ptr()
    hout.neighbors, hout.edge_ptrs, hout.parents = nbr.data_ptr(), ep.data_ptr(), par.data_ptr()
    flt.filter_mode, flt.forward = filter_mode, int(bool(forward))
    flt.win_lo, flt.win_hi = window
    flt.states = states.data_ptr() if (m and states is not None) else None
    nbytes = C.c_int64(0)
    check(lib.tg_ns_hop_labor_workspace_bytes(C.c_int64(m), C.byref(nbytes)))
    ws = torch.empty(nbytes.value // 8, **o)
    rng = TgRng(seed, call_id)
    check(lib.tg_ns_hop_labor(C.byref(graph), C.byref(hin), C.byref(flt), C.byref(rng), C.c_int32(layer), C.byref(hout),
                              ptr(st_out), ptr(ws), C.c_int64(nbytes.value), stream_ptr(dev)))
    return cnt[:m], offsets, nbr, ep, par, st_out


def ns_hop_labor_long_column(edges=0):
    """Measurement and tests: the long-column threshold of later tg_ns_hop_labor launches (0 = LABOR_LONG_COLUMN).
    -> the value it replaces."""
    prev = C.c_int64(0)
    check(lib.tg_ns_hop_labor_long_column(C.c_int64(edges), C.byref(prev)))
    return prev.value


TAG_PINSAGE = 15             # tchgeo.h TG_TAG_PINSAGE: the tag of the termination draws
PINSAGE_MAX_VISITS = 4096    # n_walks * walk_length at most


class TgPinsageConfig(C.Structure):
    _fields_ = [("n_walks", C.c_int32), ("walk_length", C.c_int32), ("termination", C.c_float), ("_reserved", C.c_int32)]


def pinsage_hop_workspace_bytes(m, fanout):
    nbytes = C.c_int64(-1)
    check(lib.tg_pinsage_hop_workspace_bytes(C.c_int64(m), C.c_int32(fanout), C.byref(nbytes)))
    return nbytes.value


def pinsage_hop(graph, vertices, fanout, n_walks, walk_length, termination, seed, call_id, call_ids=None, ids=None,
                rng_tag=0, status=None):
    """One flat hop of PinSAGE's random-walk neighbour sampler (tg_pinsage_hop): every frontier vertex starts `n_walks`
    walks of up to `walk_length` uniform steps over the rows of `graph` (the CSC walks against edge direction, the CSR along
    it), each ending before a step l >= 1 with probability `termination`; its neighbours are the `fanout` most visited
    vertices, count descending then id ascending.  `ids` [m] names a draw id and `call_ids` [m] a call id per frontier
    vertex (else the slot's index and `call_id`); status: a zeroed int32 device word (bit 1: a vertex outside the graph),
    made here when None.  -> (cnt[m], offsets[m+1], neighbors, parents, visits) -- no host synchronisation."""
    m, dev = vertices.numel(), vertices.device
    o = dict(dtype=torch.int64, device=dev)
    cnt = torch.empty(max(m, 1), **o)
    offsets = torch.empty(m + 1, **o) if m else torch.zeros(1, **o)   # m = 0 launches nothing
    nbr, par, vis = (torch.empty(max(m * fanout, 1), **o) for _ in range(3))
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    hin, hout = TgHopIn(), TgHopOut()
    hin.vertices = vertices.data_ptr() if m else None
    hin.ids = ids.data_ptr() if ids is not None else None
    hin.call_ids = call_ids.data_ptr() if call_ids is not None else None
    hin.m, hin.fanout, hin.rng_tag = m, fanout, rng_tag
    hout.cnt, hout.offsets = cnt.data_ptr(), offsets.data_ptr()
    hout.neighbors, hout.edge_ptrs, hout.parents = nbr.data_ptr(), None, par.data_ptr()
    cfg = TgPinsageConfig(n_walks, walk_length, termination, 0)
    nbytes = pinsage_hop_workspace_bytes(m, fanout)
    ws = torch.empty(max(nbytes // 8, 1), **o)
    rng = TgRng(seed, call_id)
    check(lib.tg_pinsage_hop(C.byref(graph), C.byref(hin), C.byref(cfg), C.byref(rng), C.byref(hout), ptr(vis), ptr(status),
                             ptr(ws), C.c_int64(nbytes), stream_ptr(dev)))
    return cnt[:m], offsets, nbr, par, vis
