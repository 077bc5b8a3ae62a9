"""Mini-batch materialisation on the device: the step AFTER the sampling path.

The reference's examples name a `tch_geometric.transforms` package (examples/neighbor_sampling_typed.py:5,
examples/hgt_sampling.py:5-6, examples/negative_sampling.py:5) that its tree does not contain, and hand the sampled
index tensors to PyG's `filter_data` (examples/neighbor_sampling.py:24).  This module provides those names over the
operator surface with the feature / attribute row gather done by `tg_gather_rows` (csrc/gather.hip) -- nothing
here touches host memory, and nothing needs torch_geometric.

Graph containers are duck-typed:
  homogeneous    an object with `.edge_index` i64[2, E] and `.num_nodes` (or `.x`); every other tensor attribute whose
                 first dimension is num_nodes is a node attribute, E an edge attribute (PyG's rule in
                 torch_geometric.loader.utils.filter_data);
  heterogeneous  an object with `.node_types`, `.edge_types` and `data[node_type]` / `data[edge_type]` stores that look
                 like the homogeneous object (`HeteroGraph` below is the minimal one).
"""
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor

from . import _cabi
from . import tch_geometric as native

EdgeType = Tuple[str, str, str]


def rel_key(edge_type: EdgeType) -> str:
    """relation dictionary key of the operator surface (neighbor_sampling.rs:257)"""
    return "__".join(edge_type)


def gather_rows(src: Tensor, index: Tensor) -> Tensor:
    """src[index] over dim 0 on the device; IndexError when an index is out of range."""
    if not src.is_cuda:
        raise ValueError("gather_rows runs on the HIP device; got a %s tensor" % src.device)
    if index.dtype != torch.int64:
        raise ValueError("Tensor must be a is of invalid type. Expected Int64 but got %s" % index.dtype)
    out, status = _cabi.gather_rows(src, index.to(src.device))
    if int(status.item()) != 0:
        raise IndexError("gather_rows: index out of range for %d rows" % src.shape[0])
    return out


class Graph(SimpleNamespace):
    """Minimal homogeneous container: Graph(edge_index=..., num_nodes=..., x=..., edge_attr=...)."""

    def tensor_items(self):
        return [(k, v) for k, v in vars(self).items() if isinstance(v, Tensor)]


class HeteroGraph:
    """Minimal heterogeneous container: stores keyed by node type (str) or edge type (src, rel, dst)."""

    def __init__(self):
        self._nodes: Dict[str, Graph] = {}
        self._edges: Dict[EdgeType, Graph] = {}

    def __getitem__(self, key):
        table = self._nodes if isinstance(key, str) else self._edges
        if key not in table:
            table[key] = Graph()
        return table[key]

    @property
    def node_types(self) -> List[str]:
        return list(self._nodes)

    @property
    def edge_types(self) -> List[EdgeType]:
        return list(self._edges)


def _tensor_items(store):
    if hasattr(store, "tensor_items"):
        return store.tensor_items()
    if hasattr(store, "items"):  # PyG storages
        return [(k, v) for k, v in store.items() if isinstance(v, Tensor)]
    return [(k, v) for k, v in vars(store).items() if isinstance(v, Tensor)]


def _num_nodes(store) -> int:
    n = getattr(store, "num_nodes", None)
    if n is not None:
        return int(n)
    return int(store.x.shape[0])


def _attr_kind(key: str, value: Tensor, n_nodes: int, n_edges: int) -> Optional[str]:
    """PyG's attribute rule: names containing "edge" (and per-edge timestamps / weights) are edge attributes when
    their first dimension is E; otherwise first dimension N -> node attribute, E -> edge attribute."""
    if key == "edge_index" or value.dim() == 0:
        return None
    edge_named = "edge" in key or key in ("timestamps", "weights")
    if edge_named and value.shape[0] == n_edges:
        return "edge"
    if value.shape[0] == n_nodes and not edge_named:
        return "node"
    return "edge" if value.shape[0] == n_edges else None


def to_csc(data, device=None):
    """(col_ptrs, row_indices, perm) of a homogeneous container (what the examples call thg.loader.to_csc)."""
    ei = data.edge_index if device is None else data.edge_index.to(device)
    return native.to_csc(ei, _num_nodes(data))


def to_hetero_csc(data, device=None):
    ptrs, idx, perm = {}, {}, {}
    for et in data.edge_types:
        ei = data[et].edge_index if device is None else data[et].edge_index.to(device)
        size = (_num_nodes(data[et[0]]), _num_nodes(data[et[2]]))
        ptrs[rel_key(et)], idx[rel_key(et)], perm[rel_key(et)] = native.to_csc(ei, size)
    return ptrs, idx, perm


def filter_data(data, samples: Tensor, rows: Tensor, cols: Tensor, edge_index: Tensor, perm: Optional[Tensor] = None):
    """Sub-graph container of one sampled batch: node attributes gathered by `samples`, edge attributes by
    `perm[edge_index]` (COO order of the source graph), `edge_index` = [rows; cols] in batch-local numbering."""
    n_nodes = _num_nodes(data)
    n_edges = int(data.edge_index.shape[1])
    edge = gather_rows(perm, edge_index) if perm is not None else edge_index
    out = Graph(num_nodes=int(samples.numel()), edge_index=torch.stack([rows, cols]), n_id=samples, e_id=edge)
    for key, value in _tensor_items(data):
        kind = _attr_kind(key, value, n_nodes, n_edges)
        if kind == "node":
            setattr(out, key, gather_rows(value.to(samples.device), samples))
        elif kind == "edge":
            setattr(out, key, gather_rows(value.to(samples.device), edge))
    return out


def filter_hetero_data(data, samples: Dict[str, Tensor], rows, cols, edge_index, perm: Optional[Dict[str, Tensor]] = None):
    out = HeteroGraph()
    for nt in data.node_types:
        s = samples[nt]
        store = out[nt]
        store.num_nodes, store.n_id = int(s.numel()), s
        n_nodes = _num_nodes(data[nt])
        for key, value in _tensor_items(data[nt]):
            if value.dim() > 0 and value.shape[0] == n_nodes:
                setattr(store, key, gather_rows(value.to(s.device), s))
    for et in data.edge_types:
        k = rel_key(et)
        store = out[et]
        edge = gather_rows(perm[k], edge_index[k]) if perm is not None else edge_index[k]
        store.edge_index, store.e_id = torch.stack([rows[k], cols[k]]), edge
        n_edges = int(data[et].edge_index.shape[1])
        for key, value in _tensor_items(data[et]):
            if key != "edge_index" and value.dim() > 0 and value.shape[0] == n_edges:
                setattr(store, key, gather_rows(value.to(edge.device), edge))
    return out


class _OneCallSlabs:
    """One call's (samples, rows, cols) as the single-batch slabs tg_ns_homo_unique reads."""

    def __init__(self, samples: Tensor, rows: Tensor, cols: Tensor):
        n, m, dev = samples.numel(), rows.numel(), samples.device
        pad = lambda x: (x if x.numel() else torch.zeros(1, dtype=torch.int64, device=dev)).contiguous().view(1, -1)
        self.samples, self.rows, self.cols = pad(samples), pad(rows), pad(cols)
        self.edge_index = self.rows
        self.layer_offsets = torch.zeros((1, 1, 3), dtype=torch.int64, device=dev)
        self.counts = torch.tensor([[n, m]], dtype=torch.int64).to(dev)
        self.states, self.n_seeds, self.n_hops = None, 0, 0

    struct = _cabi.NsBatchedOut.struct


def _unique_nodes_grouped(samples: Tensor, rows: Tensor, cols: Tensor, id_bound, seed_group: Tensor, n_seeds):
    """unique_nodes per group of seeds: -> (nodes, rows_u, cols_u, inverse, batch)."""
    n, m = samples.numel(), rows.numel()
    n_seeds = seed_group.numel() if n_seeds is None else int(n_seeds)
    if seed_group.dtype not in (torch.int32, torch.int64) or seed_group.numel() != n_seeds:
        raise ValueError("seed_group must be an int32 or int64 tensor with one entry per seed (%d)" % n_seeds)
    if n != n_seeds + m:
        raise ValueError("a forest of %d seeds and %d edges has %d samples, got %d" % (n_seeds, m, n_seeds + m, n))
    seed_group = seed_group.reshape(-1)
    if n_seeds and (int(seed_group.min()) < 0):
        raise ValueError("seed_group holds a negative group")
    n_groups = int(seed_group.max()) + 1 if n_seeds else 1
    if n == 0:
        return samples, rows, cols, samples, samples
    if not samples.is_cuda:
        cols = cols.cpu()
        if m and (bool((cols < 0).any()) or bool((cols >= torch.arange(n_seeds, n)).any())):
            raise ValueError("cols[e] must be a position before n_seeds + e")
        root = torch.cat([torch.arange(n_seeds), cols])
        while bool((root >= n_seeds).any()):                       # pointer jumping: a parent sits before its child
            root = root[root]
        group = seed_group.cpu().to(torch.int64)[root]
        pairs, inv = torch.unique(torch.stack([group, samples], 1), dim=0, return_inverse=True)
        first = torch.full((pairs.shape[0],), n, dtype=torch.int64).scatter_reduce_(0, inv, torch.arange(n), "amin")
        order = torch.argsort(first)
        rank = torch.empty_like(order)
        rank[order] = torch.arange(order.numel())
        inverse = rank[inv]
        return pairs[order, 1], inverse[rows], inverse[cols], inverse, pairs[order, 0]
    dev = samples.device
    if id_bound is None:                                           # the pair key needs a real bound: one read-back
        id_bound = int(samples.max()) + 1 if n else 1
    slabs = _OneCallSlabs(samples, rows.to(dev), cols.to(dev))
    slabs.n_seeds, slabs.n_hops = n_seeds, _cabi.TG_MAX_HOPS       # the hop count is not known here: the deepest forest
    slabs.layer_offsets = torch.zeros((1, _cabi.TG_MAX_HOPS, 3), dtype=torch.int64, device=dev)
    u = _cabi.ns_homo_unique_grouped(slabs, 1, int(id_bound), seed_group=seed_group.to(dev).to(torch.int32).contiguous(),
                                     n_groups=n_groups)
    n_unique = int(u.counts[0, 0])
    return u.nodes[0, :n_unique], u.rows[0, :m], u.cols[0, :m], u.inverse[0, :n], u.group[0, :n_unique]


def unique_nodes(samples: Tensor, rows: Tensor, cols: Tensor, id_bound: Optional[int] = None,
                 seed_group: Optional[Tensor] = None, n_seeds: Optional[int] = None):
    """Node dedup and relabel of ONE sampled batch (what neighbor_sampling_homogenous returns: a forest, a vertex reached
    along two paths holds two slots) -> (nodes, rows_u, cols_u, inverse): `nodes` lists each value of `samples` once, in
    order of first occurrence (distinct seeds stay first, in order), nodes[inverse] == samples, rows_u = inverse[rows],
    cols_u = inverse[cols]; edges are not merged.  Device tensors run tg_ns_homo_unique (csrc/ns_unique.hip; one read-back
    of the unique count); CPU tensors take a torch implementation of the same rule.  id_bound: every id is in
    [0, id_bound) (at most 2^31 takes 32-bit hash keys); None assumes nothing beyond non-negative int64 ids.

    seed_group (int tensor [n_seeds], values >= 0; n_seeds defaults to its length) asks for the disjoint form, PyG's
    disjoint=True: the first n_seeds samples are the seeds, edge e made sample n_seeds + e from the earlier position
    cols[e] (what the sampler returns), every sample belongs to the group of the seed its parents lead to, and a node is
    listed once per GROUP that reaches it -> (nodes, rows_u, cols_u, inverse, batch), batch[u] the group of nodes[u]
    (tg_ns_homo_unique_grouped, csrc/ns_unique.hip; forests of up to TG_MAX_HOPS hops)."""
    for t in (samples, rows, cols):
        if t.dtype != torch.int64:
            raise ValueError("Tensor must be a is of invalid type. Expected Int64 but got %s" % t.dtype)
    samples, rows, cols = samples.reshape(-1), rows.reshape(-1), cols.reshape(-1)
    if rows.numel() != cols.numel():
        raise ValueError("rows and cols differ in length")
    if seed_group is not None:
        return _unique_nodes_grouped(samples, rows, cols, id_bound, seed_group, n_seeds)
    if not samples.is_cuda:
        n = samples.numel()
        values, inv = torch.unique(samples, return_inverse=True)
        first = torch.full((values.numel(),), n, dtype=torch.int64).scatter_reduce_(0, inv, torch.arange(n), "amin")
        order = torch.argsort(first)
        rank = torch.empty_like(order)
        rank[order] = torch.arange(order.numel())
        inverse = rank[inv]
        return values[order], inverse[rows], inverse[cols], inverse
    slabs = _OneCallSlabs(samples, rows.to(samples.device), cols.to(samples.device))
    u = _cabi.ns_homo_unique(slabs, 1, (1 << 62) if id_bound is None else int(id_bound))
    n_unique, m = int(u.counts[0, 0]), rows.numel()
    return u.nodes[0, :n_unique], u.rows[0, :m], u.cols[0, :m], u.inverse[0, :samples.numel()]


def induced_subgraph(nodes: Tensor, col_ptrs: Tensor, row_indices: Tensor, id_bound: Optional[int] = None,
                     group: Optional[Tensor] = None, group_time: Optional[Tensor] = None, edge_time: Optional[Tensor] = None,
                     time_window: Optional[Tuple[int, int]] = None):
    """Every edge of the CSC graph (col_ptrs, row_indices) between two nodes of ONE list (PyG's directed=False /
    subgraph_type="induced") -> (rows, cols, edge_index): for every position i of `nodes` in order and every CSC offset e of
    column nodes[i] in ascending order, (local(row_indices[e]), i, e) where local(v), the FIRST position of v in `nodes`,
    exists.  Parallel edges and self loops are kept.  `nodes` is meant to be a list of distinct ids (unique_nodes'); with
    repeats every position scans its column.  Device tensors run tg_ns_induced_count / tg_ns_induced_emit as a single-batch
    launch (csrc/ns_induced.hip; one read-back of the edge count); CPU tensors take a torch implementation of the same
    rule.  An id outside the graph raises IndexError.  id_bound: every id is in [0, id_bound) (at most 2^31 takes 32-bit
    hash keys); None takes the graph's node count.

    group (int64, one word per entry of `nodes`, values >= 0) makes the list a DISJOINT one, one subgraph per group
    (unique_nodes' grouped form, ShaDow's k-hop sampler): local(g, v) is the first position of the PAIR, position i looks up
    (group[i], row_indices[e]), so both ends of every edge share a group and the same node under two groups is two entries.
    With group_time (int64 [max(group) + 1]), edge_time (int64, one per CSC offset) and time_window = (lo, hi), an edge is
    kept only where lo <= group_time[group[i]] - edge_time[e] <= hi (wrapping int64: the backward relative filter of the
    temporal hops).  Device tensors run tg_ns_induced_grouped_count / _emit; if the list needs more chunks than the default
    capacity, the count is repeated once with the exact capacity it reported."""
    for t in (nodes, col_ptrs, row_indices):
        if t.dtype != torch.int64:
            raise ValueError("Tensor must be a is of invalid type. Expected Int64 but got %s" % t.dtype)
    nodes = nodes.reshape(-1)
    n, n_major = nodes.numel(), col_ptrs.numel() - 1
    if n and (int(nodes.min()) < 0 or int(nodes.max()) >= n_major):
        raise IndexError("induced_subgraph: node id outside [0, %d)" % n_major)
    if group is not None:
        return _induced_subgraph_grouped(nodes, col_ptrs, row_indices, n_major if id_bound is None else int(id_bound),
                                         group, group_time, edge_time, time_window)
    if group_time is not None or edge_time is not None or time_window is not None:
        raise ValueError("induced_subgraph: group_time / edge_time / time_window come with group")
    if not nodes.is_cuda:
        begin = col_ptrs[nodes]
        deg = col_ptrs[nodes + 1] - begin
        cols = torch.repeat_interleave(torch.arange(n), deg)
        edge = torch.arange(cols.numel()) - torch.repeat_interleave(torch.cumsum(deg, 0) - deg, deg) + begin[cols]
        values, inv = torch.unique(nodes, return_inverse=True)
        first = torch.full((values.numel(),), n, dtype=torch.int64).scatter_reduce_(0, inv, torch.arange(n), "amin")
        src = row_indices[edge]
        at = torch.searchsorted(values, src).clamp_(max=max(values.numel() - 1, 0))
        keep = values[at] == src if n else torch.zeros(0, dtype=torch.bool)
        return first[at[keep]], cols[keep], edge[keep]
    dev = nodes.device
    if n == 0:
        return tuple(torch.empty(0, dtype=torch.int64, device=dev) for _ in range(3))
    col_ptrs, row_indices = col_ptrs.to(dev).contiguous(), row_indices.to(dev).contiguous()
    graph = _cabi.graph_view(col_ptrs, row_indices)
    counts = torch.tensor([n], dtype=torch.int64).to(dev)
    launch = _cabi.ns_induced_count(graph, nodes.contiguous().view(1, -1), counts, 1, 1,
                                    n_major if id_bound is None else int(id_bound))
    rc, edge_index, _ = _cabi.ns_induced_emit(launch)
    return rc[0], rc[1], edge_index


def _induced_subgraph_grouped(nodes, col_ptrs, row_indices, id_bound, group, group_time, edge_time, time_window):
    """induced_subgraph with a group word per entry (see there)"""
    n, n_major, dev = nodes.numel(), col_ptrs.numel() - 1, nodes.device
    group = group.reshape(-1)
    if group.dtype != torch.int64 or group.numel() != n or group.device != dev:
        raise ValueError("induced_subgraph: group must be an int64 tensor with one word per node, on the nodes' device")
    timed = group_time is not None
    if timed != (edge_time is not None) or timed != (time_window is not None):
        raise ValueError("induced_subgraph: group_time, edge_time and time_window come together")
    if timed and (edge_time.dtype != torch.int64 or edge_time.numel() != row_indices.numel() or group_time.dtype != torch.int64):
        raise ValueError("induced_subgraph: edge_time is int64 with one entry per CSC offset, group_time is int64")
    if n and int(group.min()) < 0:
        raise IndexError("induced_subgraph: negative group")
    n_groups = int(group.max()) + 1 if n else 1
    if timed and group_time.numel() < n_groups:
        raise IndexError("induced_subgraph: group_time has %d entries, %d groups" % (group_time.numel(), n_groups))
    if n == 0:
        return tuple(torch.empty(0, dtype=torch.int64, device=dev) for _ in range(3))
    if not nodes.is_cuda:
        begin = col_ptrs[nodes]
        deg = col_ptrs[nodes + 1] - begin
        cols = torch.repeat_interleave(torch.arange(n), deg)
        edge = torch.arange(cols.numel()) - torch.repeat_interleave(torch.cumsum(deg, 0) - deg, deg) + begin[cols]
        values, inv = torch.unique(group * n_major + nodes, return_inverse=True)
        first = torch.full((values.numel(),), n, dtype=torch.int64).scatter_reduce_(0, inv, torch.arange(n), "amin")
        src = group[cols] * n_major + row_indices[edge]
        at = torch.searchsorted(values, src).clamp_(max=values.numel() - 1)
        keep = values[at] == src
        if timed:
            x = group_time.reshape(-1)[group[cols]] - edge_time.reshape(-1)[edge]      # int64 wraps
            keep &= (x >= int(time_window[0])) & (x <= int(time_window[1]))
        return first[at[keep]], cols[keep], edge[keep]
    col_ptrs, row_indices = col_ptrs.to(dev).contiguous(), row_indices.to(dev).contiguous()
    graph = _cabi.graph_view(col_ptrs, row_indices, timestamps=edge_time.to(dev).contiguous().view(-1) if timed else None)
    counts = torch.tensor([n], dtype=torch.int64).to(dev)
    gt = group_time.to(dev).contiguous().view(-1)[:n_groups].contiguous().view(1, -1) if timed else None
    launch = _cabi.NsInducedGrouped(graph, nodes.contiguous().view(1, -1), group.contiguous().view(1, -1), counts, 1, 1,
                                    id_bound, n_groups, group_time=gt, time_window=time_window).count()
    state = launch.state.cpu()
    if int(state[-1:].view(torch.int32)[0]) & 1:                                       # the default capacity is no bound here
        launch = launch.grown(int(launch.chunks_of(state)[0])).count()
    rc, edge_index, _ = _cabi.ns_induced_emit(launch)
    return rc[0], rc[1], edge_index


class _OneCallTypedSlabs:
    """One call's per-type samples and per-relation rows / cols as the single-batch typed slabs tg_ns_typed_unique reads."""

    def __init__(self, samples: List[Tensor], rows: List[Tensor], cols: List[Tensor], rel_src, rel_dst, dev):
        pad = lambda x: (x if x.numel() else torch.zeros(1, dtype=torch.int64, device=dev)).contiguous().view(1, -1)
        self.T, self.R, self.rel_src, self.rel_dst = len(samples), len(rows), rel_src, rel_dst
        self.samples, self.rows, self.cols = [pad(x) for x in samples], [pad(x) for x in rows], [pad(x) for x in cols]
        self.edge_index, self.n_inputs = self.rows, [0] * self.T
        self.counts = torch.tensor([[x.numel() for x in samples] + [x.numel() for x in rows]], dtype=torch.int64).to(dev)


def unique_nodes_hetero(samples: Dict[str, Tensor], rows: Dict[str, Tensor], cols: Dict[str, Tensor], edge_types,
                        num_nodes: Optional[Dict[str, int]] = None):
    """Per-type node dedup and relabel of ONE call's output of neighbor_sampling_heterogenous (a forest per node type) ->
    (nodes, rows_u, cols_u, inverse), dicts keyed as the inputs: per node type `nodes[t]` lists each value of samples[t]
    once, in order of first occurrence, nodes[t][inverse[t]] == samples[t]; per relation rows_u = inverse[src type][rows],
    cols_u = inverse[dst type][cols] (an end that is no position of its list gives -1); edges are not merged.  Relation
    keys are as the operator returns them ("src__rel__dst"); edge_types (the (src, rel, dst) triples) gives each key's two
    node types.  Device tensors run
    tg_ns_typed_unique as a single-batch launch (csrc/ns_unique_typed.hip; one read-back of the unique counts); CPU tensors
    take a torch implementation of the same rule.  num_nodes: per node type, every id is in [0, num_nodes[t]) (at most 2^31
    takes 32-bit hash keys); a type without an entry assumes nothing beyond non-negative int64 ids."""
    ends = {rel_key(et): (et[0], et[2]) for et in edge_types}
    for k in rows:
        if k not in ends or k not in cols:
            raise ValueError("relation %s has no edge type / no cols" % k)
        if rows[k].numel() != cols[k].numel():
            raise ValueError("rows and cols of %s differ in length" % k)
    for t in list(samples.values()) + list(rows.values()) + [cols[k] for k in rows]:
        if t.dtype != torch.int64:
            raise ValueError("Tensor must be a is of invalid type. Expected Int64 but got %s" % t.dtype)
    rels = list(rows)
    flat = {t: x.reshape(-1) for t, x in samples.items()}
    for k in rels:                                                  # a type only a relation names: an empty list
        for t in ends[k]:
            flat.setdefault(t, torch.zeros(0, dtype=torch.int64))
    types = list(flat)
    if not any(x.is_cuda for x in flat.values()):
        empty = torch.zeros(0, dtype=torch.int64)
        parts = {t: unique_nodes(flat[t], empty, empty) for t in types}
        inverse = {t: parts[t][3] for t in types}

        def relabel(inv, end):                                      # an end that is no position of its list gives -1
            end = end.reshape(-1)
            ok = (end >= 0) & (end < inv.numel())
            return torch.where(ok, torch.cat([inv, inv.new_zeros(1)])[torch.where(ok, end, 0)], -1)

        return ({t: parts[t][0] for t in types}, {k: relabel(inverse[ends[k][0]], rows[k]) for k in rels},
                {k: relabel(inverse[ends[k][1]], cols[k]) for k in rels}, inverse)
    dev = next(x.device for x in flat.values() if x.is_cuda)
    tix = {t: i for i, t in enumerate(types)}
    slabs = _OneCallTypedSlabs([flat[t].to(dev) for t in types], [rows[k].reshape(-1).to(dev) for k in rels],
                               [cols[k].reshape(-1).to(dev) for k in rels], [tix[ends[k][0]] for k in rels],
                               [tix[ends[k][1]] for k in rels], dev)
    bounds = [max(int(num_nodes[t]), 1) if num_nodes is not None and t in num_nodes else 1 << 62 for t in types]
    u = _cabi.ns_typed_unique(slabs, 1, bounds)
    n_unique = u.counts[0].tolist()
    return ({t: u.nodes[i][0, :n_unique[i]] for i, t in enumerate(types)},
            {k: u.rows[r][0, :rows[k].numel()] for r, k in enumerate(rels)},
            {k: u.cols[r][0, :rows[k].numel()] for r, k in enumerate(rels)},
            {t: u.inverse[i][0, :flat[t].numel()] for i, t in enumerate(types)})


def _is_hetero(data) -> bool:
    return hasattr(data, "node_types") and hasattr(data, "edge_types")


class NeighborSamplerTransform:
    """examples/neighbor_sampling_typed.py:16-17, :26-27: `transform = NeighborSamplerTransform(data, num_neighbors)`;
    `batch = transform(inputs)` with a tensor (homogeneous) or a dict of tensors (heterogeneous)."""

    def __init__(self, data, num_neighbors: List[int], sampler=None, filter=None, device="cuda"):
        self.data, self.num_neighbors, self.sampler, self.filter = data, list(num_neighbors), sampler, filter
        self.hetero, self.device = _is_hetero(data), torch.device(device)
        if self.hetero:
            self.col_ptrs, self.row_indices, self.perm = to_hetero_csc(data, self.device)
        else:
            self.col_ptrs, self.row_indices, self.perm = to_csc(data, self.device)

    def __call__(self, inputs, inputs_state=None):
        flt = (self.filter, inputs_state) if self.filter is not None else None
        if not self.hetero:
            s, r, c, e, offsets = native.neighbor_sampling_homogenous(self.col_ptrs, self.row_indices,
                                                                      inputs.to(self.device), self.num_neighbors,
                                                                      self.sampler, flt)
            batch = filter_data(self.data, s, r, c, e, self.perm)
            batch.layer_offsets, batch.batch_size = offsets, int(inputs.numel())
            return batch
        inputs = {k: v.to(self.device) for k, v in inputs.items()}
        fan = {rel_key(et): self.num_neighbors for et in self.data.edge_types}
        s, r, c, e, offsets = native.neighbor_sampling_heterogenous(list(self.data.node_types), list(self.data.edge_types),
                                                                    self.col_ptrs, self.row_indices, inputs, fan,
                                                                    len(self.num_neighbors), self.sampler, flt)
        batch = filter_hetero_data(self.data, s, r, c, e, self.perm)
        batch.layer_offsets = offsets
        return batch


class HGTSamplerTransform:
    """examples/hgt_sampling.py:24-25, :30-31: HGT budget sampling over a heterogeneous container; with
    temporal=True the edge stores' int64 `timestamps` and per-call input timestamps / time range are used."""

    def __init__(self, data, num_samples: List[int], temporal: bool = False, device="cuda"):
        self.data, self.num_samples, self.temporal = data, list(num_samples), temporal
        self.device = torch.device(device)
        self.col_ptrs, self.row_indices, self.perm = to_hetero_csc(data, self.device)
        self.row_timestamps = None
        if temporal:  # timestamps follow the CSC edge order
            self.row_timestamps = {rel_key(et): gather_rows(data[et].timestamps.to(self.device), self.perm[rel_key(et)])
                                   for et in data.edge_types}

    def __call__(self, inputs: Dict[str, Tensor], inputs_timestamps=None, timerange=None):
        inputs = {k: v.to(self.device) for k, v in inputs.items()}
        if inputs_timestamps is not None:
            inputs_timestamps = {k: v.to(self.device) for k, v in inputs_timestamps.items()}
        num = {nt: self.num_samples for nt in self.data.node_types}
        s, ts, r, c, e = native.hgt_sampling(list(self.data.node_types), list(self.data.edge_types), self.col_ptrs,
                                             self.row_indices, self.row_timestamps, inputs, inputs_timestamps, num,
                                             len(self.num_samples), timerange)
        batch = filter_hetero_data(self.data, s, r, c, e, self.perm)
        batch.samples_timestamps = ts
        return batch


class NegativeSamplerTransform:
    """examples/negative_sampling.py:16-17: negatives for every input node; the returned container carries the
    gathered node attributes of `samples` and the negative edges (rows = input slot, cols = batch-local id)."""

    def __init__(self, data, num_neg: int, try_count: int, inbound: bool = False, device="cuda"):
        self.data, self.num_neg, self.try_count, self.inbound = data, num_neg, try_count, inbound
        self.hetero, self.device = _is_hetero(data), torch.device(device)
        if self.hetero:
            self.sizes, self.row_ptrs, self.col_indices = {}, {}, {}
            for et in data.edge_types:
                size = (_num_nodes(data[et[0]]), _num_nodes(data[et[2]]))
                k = rel_key(et)
                self.sizes[k] = size
                self.row_ptrs[k], self.col_indices[k], _ = native.to_csr(data[et].edge_index.to(self.device), size)
        else:
            n = _num_nodes(data)
            self.size = (n, n)
            self.row_ptrs, self.col_indices, _ = native.to_csr(data.edge_index.to(self.device), n)

    def __call__(self, inputs):
        if not self.hetero:
            s, r, c, n_in = native.negative_sample_neighbors_homogenous(self.row_ptrs, self.col_indices, self.size,
                                                                        inputs.to(self.device), self.num_neg,
                                                                        self.try_count)
            out = Graph(num_nodes=int(s.numel()), n_id=s, neg_edge_index=torch.stack([r, c]), batch_size=n_in)
            n_nodes = _num_nodes(self.data)
            for key, value in _tensor_items(self.data):
                if key != "edge_index" and value.dim() > 0 and value.shape[0] == n_nodes:
                    setattr(out, key, gather_rows(value.to(self.device), s))
            return out
        inputs = {k: v.to(self.device) for k, v in inputs.items()}
        s, r, c, counts = native.negative_sample_neighbors_heterogenous(list(self.data.node_types),
                                                                        list(self.data.edge_types), self.row_ptrs,
                                                                        self.col_indices, self.sizes, inputs,
                                                                        self.num_neg, self.try_count, self.inbound)
        out = HeteroGraph()
        for nt in self.data.node_types:
            store = out[nt]
            store.n_id, store.num_nodes, store.batch_size = s[nt], int(s[nt].numel()), counts[nt]
            n_nodes = _num_nodes(self.data[nt])
            for key, value in _tensor_items(self.data[nt]):
                if value.dim() > 0 and value.shape[0] == n_nodes:
                    setattr(store, key, gather_rows(value.to(self.device), s[nt]))
        for et in self.data.edge_types:
            out[et].neg_edge_index = torch.stack([r[rel_key(et)], c[rel_key(et)]])
        return out
