"""Mini-batch loader over the batched C ABI: the caller side of the sampling path.

The reference's surface is one call per mini-batch (examples/neighbor_sampling.py:18-24: sample, then PyG's
`filter_data`).  On a GPU that shape is latency-bound, so this loader keeps `prefetch` mini-batches in flight per
launch: one `tg_ns_homo_batched` launch samples them all (batch j of the epoch draws with call id `call_id0 + j`, so
every mini-batch equals what `neighbor_sampling_homogenous` returns for that (seed, call id) -- and the oracle), one
`tg_gather_rows` launch per attribute fetches the feature rows of all their nodes, and the mini-batches are handed
out as lazily built views of that `SuperBatch` (or the super-batch itself: `NeighborLoader.super_batches()`).
Everything stays in HBM; the host learns only the per-batch sizes (one read-back per launch, taken from pinned memory
behind a launch that runs one super-batch ahead on a side stream).  With `time_attr` / `input_time` the same launches run
under a backward temporal filter, uniformly or taking the most recent admitted edges (TG_SAMPLER_RECENT).
ShaDowKHopLoader is NeighborLoader with one subgraph per seed and every edge of the graph inside each (ShaDow-GNN's k-hop
sampler): tg_ns_induced_grouped_count / _emit behind the grouped dedup.

What the loaders share is written once.  _Loader: the length of an epoch, the walk over its launches (_epoch_launches: the
epoch counter, the one shuffle rule, the launches of _epoch_plan) and iteration as the items of super_batches().
_Indexable: a super-batch's len / index / iteration over one `_at(j)`.  SuperBatch: every optional field defaults to
None, _set_flat takes a launch's flat arrays and gathers the attribute rows.  _BlockLoader with _Block / _BlockBatch /
_BlockSuperBatch: the loaders of DGL-style blocks (PinSAGELoader, FullNeighborLoader, LADIESLoader), each with one per-layer hook.
_PooledLoader: the loaders whose launches write into one pooled slab set (the GraphSAINT loaders, ClusterLoader).

The typed-graph loaders (HeteroNeighborLoader, HGTLoader, BudgetLoader, NegativeLoader) are one program, _TypedLoader:
`prefetch` mini-batches of one node type's seeds per launch of a batched operator, one read-back of the counts, every
slab flattened and split per mini-batch, attributes gathered once per launch.  Each loader adds only its operator's
launch object and a few hooks (e_id, extras, panics).  They run on the caller's stream, launch by launch.
HeteroLinkNeighborLoader is HeteroNeighborLoader seeded by the edges of one relation: tg_link_seeds_typed fills the input
tensors of the relation's two node types directly ahead of the sampler.
Node2VecLoader, MetaPath2VecLoader and TemporalWalkLoader hand out skip-gram batches (context windows of walks plus negative
rows; the temporal one also the windows' timestamps) of one tg_rw_skipgram / tg_mp_skipgram / tg_tempo_skipgram launch per
`prefetch` mini-batches; nothing is read back.
GraphSAINTRandomWalkLoader hands out subgraphs: the distinct nodes that short random walks from random roots visit
(tg_saint_rw_nodes) with every edge of the graph between them (the induced pair), and with sample_coverage the two
normalisation vectors of a pre-sample (tg_saint_coverage_add, tg_saint_norm).  GraphSAINTNodeLoader and GraphSAINTEdgeLoader
are GraphSAINT's other two samplers on the same machinery: nodes drawn by degree (tg_saint_node_nodes) and the ends of
edges drawn with probability ~ 1/deg(u) + 1/deg(v) (tg_saint_edge_nodes).
PinSAGELoader hands out DGL-style blocks whose neighbours are the most visited nodes of short random walks with
termination (tg_pinsage_hop), the visit counts as edge weights; a launch's frontiers are grown per mini-batch with the
grouped dedup.
ClusterData / ClusterLoader hand out Cluster-GCN mini-batches: the union of `batch_size` clusters of a fixed node partition
with every edge of the graph between its nodes (tg_cluster_count / tg_cluster_emit: a range table in LDS instead of the
induced pair's hash table).
FullNeighborLoader hands out blocks that hold EVERY in-edge of their destinations (layer-wise inference; PyG's
num_neighbors=[-1]): tg_ns_full_count / tg_ns_full_emit, one read-back per layer and launch.
LADIESLoader hands out blocks of layer-wise importance sampling: one budget of drawn nodes per layer and mini-batch with
rescaled edge weights (tg_ladies_count / tg_ladies_emit), on the same per-layer scheme.
"""
from itertools import accumulate
from typing import Iterator, List, Optional

import torch
from torch import Tensor

from . import _cabi
from . import tch_geometric as _host
from .transforms import (Graph, HeteroGraph, _attr_kind, _is_hetero, _num_nodes, _tensor_items, rel_key, to_csc,
                         to_hetero_csc)


def _checked_inputs(nodes: Optional[Tensor], n_nodes: int, device=None) -> Tensor:
    """The input nodes (None: all of them) on `device` (None: where they are): int64, flat, and inside [0, n_nodes) -- the
    kernels index `ptrs[w]` unchecked (the reference panics on such an id, neighbor_sampling.rs:197)."""
    nodes = torch.arange(n_nodes, device=device) if nodes is None else nodes.to(device=device).reshape(-1).to(torch.int64)
    if nodes.numel() and (int(nodes.min()) < 0 or int(nodes.max()) >= n_nodes):
        raise IndexError("input_nodes outside [0, %d)" % n_nodes)
    return nodes


def _epoch_plan(n: int, batch_size: int, prefetch: int, drop_last: bool):
    """An epoch over n inputs as launches [(start, n_batches, batch_width)]: a launch samples the inputs
    [start, start + n_batches * batch_width) as n_batches mini-batches, the first of them mini-batch start // batch_size
    of the epoch.  Full mini-batches go `prefetch` to a launch; the ragged last one (dropped under drop_last) is a launch of
    its own."""
    n_full = n // batch_size
    plan = [(first * batch_size, min(prefetch, n_full - first), batch_size) for first in range(0, n_full, prefetch)]
    if not drop_last and n_full * batch_size < n:
        plan.append((n_full * batch_size, 1, n - n_full * batch_size))
    return plan


def _ptr_list(counts) -> List[int]:
    """Host-side counts -> their pointer list [0, c0, c0 + c1, ...]."""
    return list(accumulate(counts, initial=0))


def _at_least_1(name: str, value):
    if int(value) < 1:
        raise ValueError("%s must be at least 1, got %r" % (name, value))


def _split_attrs(data, n_nodes: int, n_edges: int, device, edges: bool = True):
    """(node_attrs, edge_attrs) of a homogeneous `data`: [(name, tensor on the device)] of the tensors with one row per
    node and per edge; edges=False leaves the edge attributes where they are (an empty list)."""
    node_attrs, edge_attrs = [], []
    for key, value in _tensor_items(data):
        kind = _attr_kind(key, value, n_nodes, n_edges)
        if kind == "node":
            node_attrs.append((key, value.to(device)))
        elif kind == "edge" and edges:
            edge_attrs.append((key, value.to(device)))
    return node_attrs, edge_attrs


def _shadowed_view(ptrs: Tensor, indices: Tensor, small: bool, **kw):
    """A graph view with its u32 shadows (they halve the bytes per gathered line) where `small` says that
    ids and offsets fit below 2^31."""
    return _cabi.graph_view(ptrs, indices, indices32=indices.to(torch.int32) if small else None,
                            ptrs32=ptrs.to(torch.int32) if small else None, **kw)


def _refuse_reserved(data, fields, whose: str):
    """A node or edge attribute of `data` named like a field the mini-batches carry themselves would be hidden by it."""
    n_nodes, n_edges = _num_nodes(data), int(data.edge_index.shape[1])
    for key, value in _tensor_items(data):
        if key in fields and _attr_kind(key, value, n_nodes, n_edges) in ("node", "edge"):
            raise ValueError("%s mini-batches carry their own `%s`: rename data.%s" % (whose, key, key))


class _Indexable:
    """A container of mini-batches: len, indexing (negative too) and iteration over one `_at(j)`."""
    __slots__ = ()

    def __len__(self):
        return len(self.node_ptr) - 1

    def __getitem__(self, j):
        if j < 0:
            j += len(self)
        if not 0 <= j < len(self):
            raise IndexError(j)
        return self._at(j)

    def __iter__(self):
        return map(self._at, range(len(self)))


class _Loader:
    """What every loader here has: input_nodes, batch_size, drop_last -> the number of mini-batches of an epoch; the walk
    over an epoch's launches; mini-batches as the items of its super-batches."""
    shuffle = False

    def __len__(self) -> int:
        n = self.input_nodes.numel()
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _epoch_launches(self, *inputs):
        """The next epoch over `inputs` (flat tensors of one length, or None: the seeds and whatever is sliced alongside
        them) as its launches: yields (the [G, width] rows of every input, the first mini-batch's number).  Every epoch
        draws afresh, as the reference's global stream does (utils/random.rs:19-22): mini-batch j of epoch e is number
        e * len(self) + j -- reproducible for a fixed (seed, epoch).  Under `shuffle` one permutation, a function of
        (seed, epoch), orders all inputs."""
        epoch = self.epoch                                      # captured: a second iterator is the next epoch
        self.epoch += 1
        batch0, B, n = epoch * len(self), self.batch_size, inputs[0].numel()
        if self.shuffle:
            gen = torch.Generator(device=self.device)
            gen.manual_seed(self.seed * 1000003 + epoch)
            order = torch.randperm(n, device=self.device, generator=gen)
            inputs = [None if t is None else t[order] for t in inputs]
        for start, G, width in _epoch_plan(n, B, self.prefetch, self.drop_last):
            yield tuple(None if t is None else t[start:start + G * width].reshape(G, width) for t in inputs), batch0 + start // B

    def __iter__(self):
        for sb in self.super_batches():
            yield from sb

    def _view(self, ptrs, indices):
        """a graph view of a homogeneous `data`'s edges, with the u32 shadows where E < 2^31"""
        return _shadowed_view(ptrs, indices, self._n_edges < 2 ** 31)

    def _out_graph(self):
        """the CSR (out-edges) of a homogeneous `data`, built with the device ingest -> its view"""
        ei = self.data.edge_index.to(self.device)
        row_ptrs, col_indices, _ = _cabi.coo_to_csx(ei[0], ei[1], self.n_nodes, self.n_nodes, False)
        return self._view(row_ptrs, col_indices)


class SuperBatch(_Indexable):
    """`prefetch` mini-batches sampled by ONE launch, as flat batch-major device tensors plus per-batch offsets -- the unit
    the loader really works in.  `n_id` [sum nodes], `edge_index` [2, sum edges] (batch-local numbering), `e_id`
    [sum edges] (COO edge ids of the source graph), one flat tensor per node / edge attribute, `node_ptr` / `edge_ptr`
    (python lists, length G + 1), `layer_offsets` [G][hops] triples, `call_id0`; from a `unique=True` loader also
    `layer_nodes` [G][hops] (unique nodes known when a hop starts; else None); from a temporal loader `input_time`
    [G, batch_size] (the seeds' times) and `node_time` [sum nodes] (the filter state of every node of n_id: its root's
    time; else None); from a disjoint loader `batch` [sum nodes] (the subgraph -- the seed group -- every node of n_id
    belongs to, numbered inside its mini-batch; else None).  Iterating (or indexing) yields the
    mini-batches as `MiniBatch` views; a consumer that can take the whole super-batch (a model over a batch of
    sub-graphs with `ptr` offsets) pays no per-mini-batch host work at all."""
    __slots__ = ("n_id", "edge_index", "_e_id", "_e_ptr", "_perm", "node_attrs", "edge_attrs", "node_ptr", "edge_ptr",
                 "layer_offsets", "layer_nodes", "layer_edges", "seed_counts", "batch_size", "call_id0", "n_hops", "_views",
                 "_index", "input_time", "node_time", "batch", "root_n_id")

    def __init__(self):
        """Nothing optional is there (n_hops: none) until the loader that fills the super-batch says so."""
        self._e_id = self._views = self.layer_offsets = self.layer_nodes = self.layer_edges = self.seed_counts = None
        self.input_time = self.node_time = self.batch = self.root_n_id = None
        self.n_hops = 0

    def _set_flat(self, n_id, edge_index, e_ptr, node_ptr, edge_ptr, perm, node_attrs, edge_attrs):
        """The flat arrays of a launch with their pointer lists, and the attribute rows [(name, table)] gathered by them
        (the edges' through e_id = perm[e_ptr]; the ids come from a sampler: no range read-back)."""
        self.n_id, self.edge_index, self.node_ptr, self.edge_ptr = n_id, edge_index, node_ptr, edge_ptr
        self._e_ptr, self._perm = e_ptr, perm
        self.node_attrs = {k: _rows_of(v, n_id) for k, v in node_attrs}
        self.edge_attrs = {k: _rows_of(v, self.e_id) for k, v in edge_attrs}

    @property
    def e_id(self):
        """COO edge ids of the sampled edges: a gather through the ingest permutation (one random 8-byte read per edge),
        made when first asked for -- a consumer that only needs n_id / edge_index / x does not pay for it"""
        if self._e_id is None:
            self._e_id = _cabi.gather_rows(self._perm, self._e_ptr)[0]
        return self._e_id

    def views_of(self, j):
        """every tensor view of mini-batch j, cut by the host module in one call (BatchViews): (n_id, edge_index, node
        attributes..., edge attributes...); e_id is cut apart, when asked for"""
        v = self._views
        if v is None:
            names = ["n_id", "edge_index"] + list(self.node_attrs) + list(self.edge_attrs)
            bases = [self.n_id, self.edge_index] + list(self.node_attrs.values()) + list(self.edge_attrs.values())
            dims = [0, 1] + [0] * (len(bases) - 2)
            kinds = [0, 1] + [0] * len(self.node_attrs) + [1] * len(self.edge_attrs)
            self._index = {k: i for i, k in enumerate(names)}
            v = self._views = _host.BatchViews(bases, dims, kinds, self.node_ptr, self.edge_ptr)
        return v.at(j)

    def _at(self, j):
        return MiniBatch(self, j)

    @property
    def num_nodes(self):
        return self.node_ptr[-1]

    @property
    def num_edges(self):
        return self.edge_ptr[-1]


TIME_FIELDS = ("input_time", "node_time")   # what a temporal NeighborLoader adds to a mini-batch
DISJOINT_FIELDS = ("batch",)                # what a disjoint one adds (PyG's `batch` vector)
SHADOW_FIELDS = ("root_n_id",)              # what ShaDowKHopLoader adds (PyG's ShaDowKHopSampler: every seed's own entry)


class MiniBatch:
    """Mini-batch j of a SuperBatch.  Nothing is built until it is asked for: sizes are python ints, tensors are views
    (torch.narrow) made on first access -- handing a mini-batch out costs well under a microsecond of host time instead
    of the ~20 us an eagerly built container with a dozen attributes took (profiles/r01/loader_end_to_end.json)."""
    __slots__ = ("_sb", "_j", "_cache", "__dict__")   # __dict__: a consumer may hang its own attributes on a mini-batch

    def __init__(self, sb, j):
        self._sb, self._j, self._cache = sb, j, None

    num_nodes = property(lambda self: self._sb.node_ptr[self._j + 1] - self._sb.node_ptr[self._j])
    num_edges = property(lambda self: self._sb.edge_ptr[self._j + 1] - self._sb.edge_ptr[self._j])

    @property
    def batch_size(self):
        """the seeds of the mini-batch; under unique=True the distinct ones (they lead n_id)"""
        sc = self._sb.seed_counts
        return self._sb.batch_size if sc is None else sc[self._j]

    @property
    def layer_nodes(self):
        """unique=True: [hops] unique nodes among the positions known when hop h starts ([0] = the unique seeds)"""
        ln = self._sb.layer_nodes
        return None if ln is None else list(ln[self._j][:self._sb.n_hops])

    @property
    def layer_edges(self):
        """induced=True: [hops] induced edges whose target is among the first layer_nodes[h] nodes (a prefix of edge_index)"""
        le = self._sb.layer_edges
        return None if le is None else list(le[self._j][:self._sb.n_hops])

    call_id = property(lambda self: self._sb.call_id0 + self._j)

    @property
    def layer_offsets(self):
        """the forest's (node begin, node end, edge end) per hop; None from an induced=True loader"""
        lo = self._sb.layer_offsets
        return None if lo is None else [tuple(x) for x in lo[self._j][:self._sb.n_hops]]

    def _all(self):  # the views of this mini-batch: one call into the host module on first use, then a tuple
        c = self._cache
        if c is None:
            c = self._cache = self._sb.views_of(self._j)
        return c

    n_id = property(lambda self: self._all()[0])
    edge_index = property(lambda self: self._all()[1])

    @property
    def e_id(self):
        sb, j = self._sb, self._j
        a = sb.edge_ptr[j]
        return sb.e_id.narrow(0, a, sb.edge_ptr[j + 1] - a)

    def __getattr__(self, name):  # node / edge attributes of the source graph (x, y, edge_attr, ...)
        sb = object.__getattribute__(self, "_sb")
        # a temporal loader's mini-batches also carry input_time [batch_size] (the seeds' times) and node_time [num_nodes]
        # (the time every node of n_id was sampled under: its root's).  Not class attributes: from an untimed loader the
        # two names stay what they were, attributes of the source graph if it has them (a temporal loader refuses such a graph)
        if name in TIME_FIELDS and sb.input_time is not None:
            j = object.__getattribute__(self, "_j")
            if name == "input_time":
                return sb.input_time[j]
            a = sb.node_ptr[j]
            return sb.node_time.narrow(0, a, sb.node_ptr[j + 1] - a)
        # a disjoint loader's mini-batches carry batch [num_nodes], the subgraph of every node of n_id; from any other loader
        # the name stays the graph's attribute if it has one, else None
        if name in DISJOINT_FIELDS and sb.batch is not None:
            j = object.__getattribute__(self, "_j")
            a = sb.node_ptr[j]
            return sb.batch.narrow(0, a, sb.node_ptr[j + 1] - a)
        # ShaDowKHopLoader's mini-batches carry root_n_id [batch_size], the position of every seed's own entry in n_id
        if name in SHADOW_FIELDS and getattr(sb, "root_n_id", None) is not None:
            return sb.root_n_id
        if name in sb.node_attrs or name in sb.edge_attrs:
            views = self._all()
            return views[sb._index[name]]
        if name in DISJOINT_FIELDS:
            return None
        raise AttributeError(name)

    def tensor_items(self):
        views = self._all()
        return [(k, views[i]) for k, i in self._sb._index.items()] + [("e_id", self.e_id)]


def _check_labor(labor, layer_dependency, replace, temporal_strategy, disjoint, num_neighbors):
    """What layer-neighbor sampling (labor=True, TG_SAMPLER_LABOR) cannot take: refused before any device work."""
    if layer_dependency and not labor:
        raise ValueError("layer_dependency=True needs labor=True: it is an option of layer-neighbor sampling")
    if not labor:
        return
    if replace:
        raise ValueError("labor=True samples without replacement: replace=True is not supported")
    if temporal_strategy == "last":
        raise ValueError("labor=True does not combine with temporal_strategy='last': the most recent edges are not drawn")
    if disjoint:
        raise ValueError("labor=True does not combine with disjoint=True: nothing is shared between subgraphs")
    if any(int(k) > 64 for k in num_neighbors):
        raise ValueError("labor=True takes num_neighbors up to 64")


class NeighborLoader(_Loader):
    """One launch samples `prefetch` mini-batches; while the caller consumes super-batch i, super-batch i + 1 is already
    being sampled on a side stream into the other of two slab sets (its sizes travel to pinned host memory behind the
    kernel), so neither the launch nor its one read-back sits on the consumer's path.  Launches of >= 2 048 mini-batches
    get the window-ordered form's workspace (kept by the loader, sized for this graph's stage slots); `form` is
    ns_homo_batched's: 0 takes that form by launch and graph size, 1 whenever the launch qualifies, 2 never.

    unique=True hands out PyG-style mini-batches: tg_ns_homo_unique runs behind the sampler on the side stream, `n_id`
    lists each node once (first occurrence first, so the distinct seeds lead), `edge_index` is numbered against it (edges
    are not merged), node attributes are gathered per unique node; `e_id` and the edge attributes are the forest's.
    `batch_size` is the unique-seed count, `layer_nodes[h]` the unique nodes known when hop h starts; `layer_offsets`
    stays the forest's.

    induced=True (needs unique=True) replaces the forest's edges by the induced subgraph of `n_id`, PyG's directed=False:
    every edge of the graph between two nodes of the mini-batch, ordered by target position, then CSC offset.
    tg_ns_induced_count runs on the side stream directly behind the dedup (its edge counts travel to pinned memory with the
    other sizes: still one wait per launch), tg_ns_induced_emit on the caller's stream straight into the flat `edge_index`;
    the workspace the two passes share belongs to the slab set.  `edge_index`, `num_edges`, `e_id` and the edge attributes
    are the induced edges'; `layer_edges[h]` counts those whose target is among the first `layer_nodes[h]` nodes, a prefix
    of `edge_index`; `layer_offsets` is None.  Induced edges are not filtered.

    Temporal (PyG's time_attr / input_time): `time_attr` names an int64 [E] tensor on `data` in edge_index order (carried
    into CSC order once), `input_time` holds one int64 per input node and is sliced and shuffled with input_nodes.  An edge
    of time t is admitted for a seed of time T when 0 <= T - t <= hi (TG_FILTER_RELATIVE, backward; `time_window` = (lo, hi),
    default (0, 2**62)), and the whole subtree of a seed keeps the seed's time.  temporal_strategy="uniform" draws with the
    loader's sampler among the admitted edges (`replace` honoured); "last" takes the num_neighbors most recent ones
    (TG_SAMPLER_RECENT: deterministic, fan-outs <= 64).  Mini-batches gain `input_time` [batch_size] and `node_time`
    [num_nodes]; a `data` that has node or edge attributes of those names is refused (from an untimed loader the names
    stay the graph's attributes, as before).

    disjoint=True (needs unique=True; PyG's disjoint): every seed keeps its own subgraph.  tg_ns_homo_unique_grouped runs in
    tg_ns_homo_unique's place and dedups by (subgraph, node): a node reached from two seeds is listed twice, once per
    subgraph, and `batch` [num_nodes] names the subgraph (here: the seed's position in the mini-batch) of every node of
    n_id, so both ends of every edge share `batch` and `batch_size` is the seed count.  It buys the contract, not speed:
    inside one seed's tree there is little to merge.  A temporal loader takes unique=True only together with disjoint=True
    -- the same node under two seeds of different times is two samples, so plain deduplication stays refused -- and its
    `node_time` is then input_time[batch].  (PyG turns disjoint on by itself when times are given; here it is asked for by
    name, so that unique=True alone keeps meaning the plain dedup.)  A `data` with a node or edge attribute named `batch` is
    refused; induced=True with disjoint is out of scope and refused here: induced edges per subgraph are ShaDowKHopLoader's.

    labor=True samples with layer-neighbor sampling (LABOR-0; TG_SAMPLER_LABOR): every vertex gets one random variate per
    mini-batch and hop, shared by all seeds of the mini-batch, and a frontier vertex keeps the num_neighbors admitted
    neighbours with the smallest ones.  One vertex's neighbours are a uniform subset as without the option; across the
    mini-batch the same vertices are picked again and again, so `n_id` under unique=True is shorter and fewer feature rows
    are gathered.  layer_dependency=True uses the same variates at every hop (fewer distinct nodes still).  The forest has
    the shape it always has, so unique, induced and time_attr (temporal_strategy="uniform") work unchanged; replace=True,
    temporal_strategy="last", disjoint=True and num_neighbors above 64 are refused."""

    def __init__(self, data, num_neighbors: List[int], input_nodes: Optional[Tensor] = None, batch_size: int = 1024,
                 prefetch: int = 16, replace: bool = False, shuffle: bool = False, drop_last: bool = False,
                 seed: int = 0, call_id0: int = 0, device="cuda", form: int = 0, unique: bool = False,
                 induced: bool = False, time_attr: Optional[str] = None, input_time: Optional[Tensor] = None,
                 temporal_strategy: str = "uniform", time_window=None, disjoint: bool = False, labor: bool = False,
                 layer_dependency: bool = False):
        _check_labor(labor, layer_dependency, replace, temporal_strategy, disjoint, num_neighbors)
        self.labor, self.layer_dependency = bool(labor), bool(layer_dependency)
        if induced and not unique:
            raise ValueError("induced=True needs unique=True: the induced edges are numbered against the unique node list")
        if temporal_strategy not in ("uniform", "last"):
            raise ValueError("temporal_strategy must be 'uniform' or 'last', got %r" % (temporal_strategy,))
        if (time_attr is None) != (input_time is None):
            raise ValueError("time_attr and input_time come together: edge times need seed times and the reverse")
        if temporal_strategy == "last" and time_attr is None:
            raise ValueError("temporal_strategy='last' needs time_attr and input_time")
        if time_window is not None and time_attr is None:
            raise ValueError("time_window needs time_attr and input_time")
        self.temporal = time_attr is not None
        if disjoint and not unique:
            raise ValueError("disjoint=True needs unique=True: without deduplication every seed's tree is apart already")
        self.disjoint = bool(disjoint)
        if self.temporal and unique and not self.disjoint:
            raise ValueError("a temporal loader with unique=True needs disjoint=True: plain deduplication would merge slots "
                             "that carry different seed times")
        if self.disjoint and induced and not self.INDUCED_PER_SUBGRAPH:
            raise ValueError("induced=True with disjoint subgraphs is out of scope: the induced edges are found per "
                             "mini-batch, not per subgraph")
        if self.disjoint:
            _refuse_reserved(data, DISJOINT_FIELDS, "a disjoint loader's")
        if self.temporal:                  # everything that can be refused is refused before any device work
            times = getattr(data, time_attr, None)
            n_edges = int(data.edge_index.shape[1])
            if not isinstance(times, Tensor) or times.dtype != torch.int64 or times.numel() != n_edges:
                raise ValueError("data.%s must be an int64 tensor with one entry per edge (%d)" % (time_attr, n_edges))
            n_inputs = _num_nodes(data) if input_nodes is None else input_nodes.numel()
            if not isinstance(input_time, Tensor) or input_time.dtype != torch.int64 or input_time.numel() != n_inputs:
                raise ValueError("%s must be an int64 tensor with one entry per %s (%d)" % (self.TIME_ARG + (n_inputs,)))
            if temporal_strategy == "last" and any(int(k) > 64 for k in num_neighbors):
                raise ValueError("temporal_strategy='last' takes num_neighbors up to 64")
            _refuse_reserved(data, TIME_FIELDS, "a temporal loader's")
            self.time_window = (0, 2 ** 62) if time_window is None else (int(time_window[0]), int(time_window[1]))
        self.temporal_strategy = temporal_strategy
        self.induced = bool(induced)
        self.data, self.fanout = data, [int(k) for k in num_neighbors]
        self.device = torch.device(device)
        self.batch_size, self.prefetch = int(batch_size), max(1, int(prefetch))
        self.sampler = _cabi.SAMPLER_UNIFORM_REPL if replace else _cabi.SAMPLER_UNIFORM
        if temporal_strategy == "last":
            self.sampler = _cabi.SAMPLER_RECENT
        if self.labor:
            self.sampler = _cabi.SAMPLER_LABOR_SHARED if self.layer_dependency else _cabi.SAMPLER_LABOR
        self.shuffle, self.drop_last, self.seed, self.call_id0 = shuffle, drop_last, int(seed), int(call_id0)
        self.form = int(form)               # of many-batch launches (ns_homo_batched's `form`): 0 = by launch size
        self.unique = bool(unique)
        self._unique_ws = None              # the dedup's tables (flat form), sized once for a full launch
        self.n_nodes = _num_nodes(data)
        self.col_ptrs, self.row_indices, self.perm = to_csc(data, self.device)
        # the longest column (one read-back) sets the stage slots' bit widths: without it they assume n_edges, and the
        # slots of a large graph come out two chunks wide, which the staged pipeline of many-batch launches refuses
        self.edge_time = self.input_time = None
        if self.temporal:                   # the edge times in CSC order, once
            times = getattr(data, time_attr).to(self.device).reshape(-1)
            self.edge_time = times[self.perm].contiguous() if times.numel() else times
            self.input_time = input_time.to(self.device).reshape(-1)
        self._graph = _shadowed_view(self.col_ptrs, self.row_indices,
                                     self.n_nodes < 2 ** 31 and self.row_indices.numel() < 2 ** 31,
                                     timestamps=self.edge_time, max_degree="auto")
        self._idx32, self._ptr32 = self._graph._keep[4:]
        self._time_ws = {}               # temporal and labor launches: the workspace per launch shape (full / ragged), kept
        self.input_nodes = _checked_inputs(input_nodes, self.n_nodes, self.device)
        self._n_edges = int(data.edge_index.shape[1])
        self._node_attrs, self._edge_attrs = _split_attrs(data, self.n_nodes, self._n_edges, self.device)
        self._pool = []                     # slab sets of finished iterators (each live iterator owns its own)
        self._ws = None
        self._side = None
        self.epoch = 0

    INDUCED_PER_SUBGRAPH = False    # induced=True with disjoint=True: only a subclass built for it (ShaDowKHopLoader) gets past

    # ---- what a loader whose work items are not the seeds themselves fills in (LinkNeighborLoader)
    WITH_INVERSE = False            # unique=True: keep tg_ns_homo_unique's `inverse` slab (forest position -> n_id position)
    TIME_ARG = ("input_time", "input node")   # what the work items' times are called in a refusal

    def _seed_width(self, width: int) -> int:
        """Seeds of a mini-batch of `width` work items."""
        return width

    def _seed_rows(self, slab, items: Tensor, first_batch: int) -> Tensor:
        """The [G, seeds] rows the sampler starts from for the work items [G, width] of a launch whose first mini-batch is
        first_batch; called on the side stream, directly ahead of the sampler."""
        return items

    def _seed_times(self, slab, times: Tensor) -> Tensor:
        """The [G, seeds] times the sampler filters under for the work items' times [G, width]; called on the side stream
        next to _seed_rows."""
        return times

    def _seed_groups(self, seeds: int):
        """disjoint: (seed_group, n_groups) of a seed row of this width -- the int32 device map seed position -> subgraph,
        None for the identity (one subgraph per seed)."""
        return None, seeds

    def _new_super_batch(self, slab, G: int) -> SuperBatch:
        """The launch's container; called on the caller's stream while the slab set is still the launch's (whatever a
        subclass needs from it is copied here)."""
        return SuperBatch()

    def _times_of(self, sb, slab, G: int, times: Tensor):
        """-> (input_time [G, seeds], the subgraphs' times [G, n_groups]) of a temporal launch, for the super-batch; called
        on the caller's stream behind _new_super_batch."""
        return times, times

    # ---- stage 1 (side stream): sample G mini-batches into slab set `which`, sizes -> pinned host memory
    def _sample(self, slabs, which, seeds: Tensor, first_batch: int, times: Optional[Tensor] = None):
        """`slabs` is the iterator's own set: slots 0 / 1 for full launches (one consumed, one sampled), "ragged" for the
        epoch's last, narrower mini-batch -- so that one neither replaces the big slabs nor is replaced by them"""
        G, B = seeds.shape[0], self._seed_width(seeds.shape[1])
        H = len(self.fanout)
        slab = slabs.get(which)
        if slab is None or slab["out"].n_batches < G or slab["out"].n_seeds != B:
            cap = G if which == "ragged" else max(G, min(self.prefetch, len(self)))
            slab = {"out": _cabi.NsBatchedOut(cap, B, self.fanout, self.device, with_states=self.temporal),
                    "counts": torch.empty((cap, 2), dtype=torch.int64).pin_memory(),
                    "lo": torch.empty((cap, max(H, 1), 3), dtype=torch.int64).pin_memory(),
                    "free": None}
            if self.unique:
                slab["uniq"] = _cabi.NsUniqueOut(slab["out"], in_place=True, with_inverse=self.WITH_INVERSE,
                                                 with_group=self.disjoint)
                slab["ln"] = torch.empty((cap, max(H, 1)), dtype=torch.int64).pin_memory()
            slabs[which] = slab
        time_ws = None
        if self.temporal or self.labor:      # the workspace of THIS sampler / filter, sized for the slab set's full launch
            key = (slab["out"].n_batches, B)
            if key not in self._time_ws:
                mode = _cabi.FILTER_RELATIVE if self.temporal else _cabi.FILTER_NONE
                self._time_ws[key] = _cabi.ns_homo_batched_workspace(self._graph, key[0], B, self.fanout, self.device,
                                                                     sampler=self.sampler, filter_mode=mode)
            time_ws = self._time_ws[key]
        if G >= 2048 and self._ws is None and not self.temporal and not self.labor:   # many batches per launch: the window-ordered form pays
            self._ws = _cabi.ns_homo_workspace(max(G, min(self.prefetch, len(self))), B, self.fanout, self.device,
                                               graph=self._graph)
        cur = torch.cuda.current_stream(self.device)
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        side = self._side
        side.wait_stream(cur)                # the seeds (and an earlier consumer of this slab set) are ahead of us
        if slab["free"] is not None:
            side.wait_event(slab["free"])
        with torch.cuda.stream(side):
            items = seeds.contiguous()
            seeds = self._seed_rows(slab, items, first_batch)
            out = slab["out"]
            if self.temporal:                # backward RELATIVE filter: 0 <= seed time - edge time <= hi, state kept down the tree
                times = times.contiguous()
                seed_times = self._seed_times(slab, times)
                _cabi.ns_homo_batched(self._graph, seeds, self.fanout, self.seed, self.call_id0 + first_batch, out,
                                      sampler=self.sampler, filter_mode=_cabi.FILTER_RELATIVE, forward=False,
                                      window=self.time_window, seeds_state=seed_times, ws=time_ws)
            elif self.labor:                 # layer-neighbor sampling: the flat path with its workspace, at any launch size
                _cabi.ns_homo_batched(self._graph, seeds, self.fanout, self.seed, self.call_id0 + first_batch, out,
                                      sampler=self.sampler, ws=time_ws)
            else:
                _cabi.ns_homo_batched(self._graph, seeds, self.fanout, self.seed, self.call_id0 + first_batch, out,
                                      sampler=self.sampler, ws=self._ws if G >= 2048 else None, form=self.form)
            sizes = out
            if self.unique:                  # dedup + relabel directly behind the sampler; the host reads the unique counts
                sizes = uniq = slab["uniq"]
                if self.disjoint:            # the dedup key is (subgraph, node): one subgraph per group of seeds
                    seed_group, n_groups = self._seed_groups(B)
                    need, least = _cabi.ns_homo_unique_grouped_workspace_bytes(out.cap_nodes, self.n_nodes, n_groups,
                                                                               out.n_batches)
                else:
                    need, least = _cabi.ns_homo_unique_workspace_bytes(out.cap_nodes, self.n_nodes, out.n_batches)
                if need and (self._unique_ws is None or self._unique_ws.numel() * 8 < least):
                    self._unique_ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=self.device)
                if self.disjoint:
                    _cabi.ns_homo_unique_grouped(out, G, self.n_nodes, seed_group=seed_group, n_groups=n_groups,
                                                 ws=self._unique_ws if need else None, result=uniq)
                else:
                    _cabi.ns_homo_unique(out, G, self.n_nodes, ws=self._unique_ws if need else None, result=uniq)
                if H:
                    slab["ln"][:G].copy_(uniq.layer_nodes[:G], non_blocking=True)
                if self.induced:             # pass 1: the edge counts join the sizes the host waits for
                    ind = slab.get("ind")
                    if self.disjoint:        # per subgraph: the grouped pair, under times with the subgraphs' times
                        if ind is None or ind.chunk_cap < self.chunk_cap:
                            if self.temporal and "gt" not in slab:
                                slab["gt"] = torch.empty((out.n_batches, n_groups), dtype=torch.int64, device=self.device)
                            ind = slab["ind"] = _cabi.NsInducedGrouped(
                                self._graph, uniq.nodes, uniq.group, uniq.counts, 2, out.n_batches, self.n_nodes, n_groups,
                                node_marks=uniq.layer_nodes if H else None, group_time=slab.get("gt"),
                                time_window=self.time_window if self.temporal else None, chunk_cap=self.chunk_cap)
                            slab["ist"] = torch.empty(ind.state.numel(), dtype=torch.int64).pin_memory()
                        if self.temporal:
                            slab["gt"][:G].copy_(self._group_times(slab, seed_times))
                    elif ind is None:
                        ind = slab["ind"] = _cabi.NsInduced(self._graph, uniq.nodes, uniq.counts, 2, out.n_batches,
                                                            self.n_nodes, node_marks=uniq.layer_nodes if H else None)
                        slab["ist"] = torch.empty(ind.state.numel(), dtype=torch.int64).pin_memory()
                    ind.count(G)
                    slab["ist"].copy_(ind.state, non_blocking=True)
            slab["counts"][:G].copy_(sizes.counts[:G], non_blocking=True)
            slab["lo"][:G].copy_(out.layer_offsets[:G], non_blocking=True)
            done = torch.cuda.Event()
            done.record(side)
        items.record_stream(side)
        if times is not None:
            times.record_stream(side)
        return (slab, G, B, first_batch, done, times)

    # ---- stage 2 (caller's stream): flatten, gather the attribute rows
    def _finish(self, ticket) -> SuperBatch:
        slab, G, B, first_batch, done, times = ticket
        out = slab["out"]
        done.synchronize()                   # the host needs the sizes; the device work it waits for is long done
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(done)
        counts = slab["counts"][:G]
        n_nodes, n_edges = counts[:, 0].tolist(), counts[:, 1].tolist()
        src = slab["uniq"] if self.unique else out                 # unique: the deduplicated, relabelled view of the slabs
        if self.induced:                     # pass 2 writes the flat arrays itself: no edge slab, no edge compaction
            ind, ist = slab["ind"], slab["ist"]
            if self.disjoint and int(ist[-1]) & 1:   # a mini-batch needs more chunks than the workspace holds: the slow path
                ind, ist = self._grow_induced(slab, G)
            _cabi.induced_status_check(int(ist[-1]) & 0xFFFFFFFF, "%s(induced=True)" % type(self).__name__)
            n_edges = ist[:G].tolist()
            n_id = _flat_rows(src.nodes[:G], src.counts[:G, 0], sum(n_nodes))
            edge_index, e_ptr, _ = _cabi.ns_induced_emit(ind, n_edges)
        else:
            n_id, edge_index, e_ptr = _cabi.ns_homo_compact(src, G, counts, stacked=True)   # copies: the slabs go back to the sampler
        sb = self._new_super_batch(slab, G)
        total = sum(n_nodes)
        if self.disjoint:                    # the group slab trimmed like nodes (a copy: the slab goes back)
            sb.batch = _flat_rows(src.group[:G], src.counts[:G, 0], total)
        if self.temporal:
            sb.input_time, group_times = self._times_of(sb, slab, G, times)
            if self.disjoint:                # time is a function of the subgraph: mini-batch g's node u has group_times[g][batch[u]]
                first = torch.arange(G, device=self.device) * group_times.shape[1]
                first = torch.repeat_interleave(first, src.counts[:G, 0], output_size=total)
                sb.node_time = group_times.reshape(-1)[first + sb.batch]
            else:                            # the states slab trimmed like samples (a copy: the slab goes back)
                sb.node_time = _flat_rows(out.states[:G], out.counts[:G, 0], total)
        free = torch.cuda.Event()
        free.record(cur)
        slab["free"] = free
        sb._set_flat(n_id, edge_index, e_ptr, _ptr_list(n_nodes), _ptr_list(n_edges), self.perm, self._node_attrs, self._edge_attrs)
        if self.induced:
            cap, H = slab["ind"].n_batches, len(self.fanout)
            sb.layer_edges = slab["ist"][cap:cap * (1 + H)].view(cap, H)[:G].tolist()
        else:
            sb.layer_offsets = slab["lo"][:G].tolist()
        if self.unique:
            H = len(self.fanout)
            sb.layer_nodes = slab["ln"][:G, :H].tolist()
            sb.seed_counts = [ln[0] for ln in sb.layer_nodes] if H else n_nodes
        sb.batch_size, sb.call_id0, sb.n_hops = B, self.call_id0 + first_batch, len(self.fanout)
        return sb

    def _group_times(self, slab, seed_times: Tensor) -> Tensor:
        """The [G, n_groups] subgraph times of a launch whose seeds' times are seed_times [G, seeds]; called on the side
        stream.  One subgraph per seed: the seeds' own."""
        return seed_times

    def _grow_induced(self, slab, G: int):
        """The grouped induced count of a launch overflowed its chunk capacity: a launch object with room for the largest
        mini-batch it reported replaces the slab set's (and sets the capacity of every later one), and pass 1 runs again on
        the caller's stream while the slab set is still the launch's.  One more wait; taken at most a few times per loader."""
        old = slab["ind"]
        self.chunk_cap = max(self.chunk_cap, max(old.chunks_of(slab["ist"])[:G]))
        ind = slab["ind"] = old.grown(self.chunk_cap)
        ind.count(G)
        slab["ist"].copy_(ind.state, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return ind, slab["ist"]

    def super_batches(self) -> Iterator[SuperBatch]:
        """The epoch as super-batches of up to `prefetch` mini-batches; the next one is sampled while this one is used."""
        B = self.batch_size                                     # mini-batch j of epoch e uses call id call_id0 + e * len(self) + j
        work = [(seeds, first_batch, times)
                for (seeds, times), first_batch in self._epoch_launches(self.input_nodes, self.input_time)]
        # this iterator's own slabs (two iterators alive at once -- zip(loader, loader), a restart after an abandoned
        # epoch -- must not sample into each other's); they go back to the pool when the iterator ends or is dropped
        slabs = self._pool.pop() if self._pool else {}
        which_of = lambda i: "ragged" if work[i][0].shape[1] != B else i & 1
        pending = None
        try:
            for i in range(len(work)):
                if pending is None:
                    pending = self._sample(slabs, which_of(i), *work[i])
                ticket = pending
                pending = self._sample(slabs, which_of(i + 1), *work[i + 1]) if i + 1 < len(work) else None
                yield self._finish(ticket)
        finally:
            if pending is not None:          # abandoned with a launch in flight: it still writes into these slabs
                pending[4].synchronize()
            self._pool.append(slabs)


def _flat_rows(slab: Tensor, lens: Tensor, total: int) -> Tensor:
    """tg_compact_rows, or an empty tensor when the rows hold nothing (the library refuses a null destination)."""
    if total == 0:
        return torch.empty(0, dtype=torch.int64, device=slab.device)
    return _cabi.compact_rows(slab, lens, total)


class ShaDowKHopLoader(NeighborLoader):
    """ShaDow-GNN's k-hop sampler (PyG's ShaDowKHopSampler) as a loader: every seed gets its own bounded neighbourhood --
    `depth` hops of at most `num_neighbors` sampled neighbours each -- and the mini-batch holds EVERY edge of the graph
    inside each neighbourhood.  It is NeighborLoader([num_neighbors] * depth, unique=True, disjoint=True, induced=True), the
    one combination NeighborLoader itself refuses: tg_ns_induced_grouped_count runs on the side stream behind
    tg_ns_homo_unique_grouped (node list, group words and, under times, the subgraphs' times), tg_ns_induced_grouped_emit
    writes the flat `edge_index` on the caller's stream.

    Mini-batches carry what the disjoint loader's carry (`n_id`, `batch`, node attributes, under times `node_time` and
    `input_time`), `edge_index` / `e_id` / edge attributes / `layer_edges` of the per-subgraph induced edges (both ends of
    every edge share `batch`; ordered by target position, then CSC offset), `root_n_id` [batch_size] -- the position of
    every seed's own entry in `n_id` -- and `batch_size`, the seed count.  Under times (time_attr / input_time /
    temporal_strategy / time_window as NeighborLoader's) the sampled neighbourhood AND the induced edges are admitted only up
    to the seed's time: lo <= T_seed - t_edge <= hi.

    Columns of a disjoint node list are not disjoint (a hub reached from many seeds is scanned once per seed), so the
    induced pair's workspace has a capacity in chunks of 512 column entries per mini-batch: `chunk_cap` (None: the
    ungrouped pair's bound, num nodes + ceil(E / 512)).  A launch that needs more is counted again with the capacity it
    reported and the larger workspace is kept: one extra wait, taken at most a few times per loader.

    Out of scope: the link-level counterpart (enclosing subgraphs around a label edge; tg_ns_induced_grouped_* already takes
    arbitrary groups, so that loader needs no new kernel) and the typed graphs."""
    INDUCED_PER_SUBGRAPH = True

    def __init__(self, data, depth: int, num_neighbors: int, input_nodes: Optional[Tensor] = None, replace: bool = False,
                 batch_size: int = 1024, prefetch: int = 16, shuffle: bool = False, drop_last: bool = False, seed: int = 0,
                 call_id0: int = 0, device="cuda", time_attr: Optional[str] = None, input_time: Optional[Tensor] = None,
                 temporal_strategy: str = "uniform", time_window=None, chunk_cap: Optional[int] = None):
        if int(depth) < 1:
            raise ValueError("depth must be at least 1, got %r" % (depth,))
        if int(num_neighbors) < 1:
            raise ValueError("num_neighbors must be at least 1, got %r" % (num_neighbors,))
        if temporal_strategy == "last" and int(num_neighbors) > 64:
            raise ValueError("temporal_strategy='last' takes num_neighbors up to 64")
        if chunk_cap is not None and not 1 <= int(chunk_cap) <= 2 ** 31:
            raise ValueError("chunk_cap must be in [1, 2^31], got %r" % (chunk_cap,))
        _refuse_reserved(data, SHADOW_FIELDS, "a ShaDowKHopLoader's")   # (`batch`: the parent's check)
        self.depth, self.num_neighbors = int(depth), int(num_neighbors)
        self.chunk_cap = int(chunk_cap) if chunk_cap is not None else 0   # 0: the launch object's default; grows on overflow
        super().__init__(data, [self.num_neighbors] * self.depth, input_nodes=input_nodes, batch_size=batch_size,
                         prefetch=prefetch, replace=replace, shuffle=shuffle, drop_last=drop_last, seed=seed,
                         call_id0=call_id0, device=device, unique=True, induced=True, disjoint=True, time_attr=time_attr,
                         input_time=input_time, temporal_strategy=temporal_strategy, time_window=time_window)

    def _finish(self, ticket) -> SuperBatch:
        sb = super()._finish(ticket)
        # one subgraph per seed and the pair (subgraph, seed) first occurs at the seed's own position: the seeds lead n_id
        sb.root_n_id = torch.arange(sb.batch_size, device=self.device)
        return sb


def _rows_of(table: Tensor, index: Tensor) -> Tensor:
    return _cabi.gather_rows(table, index)[0]                       # the ids come from a sampler: no range read-back


def _fill_store(st, b: int, fields, attrs):
    """Mini-batch b's part of a node type's or a relation's launch-wide fields and attributes, set on its store."""
    for k, parts in fields:
        if parts is not None:
            setattr(st, k, parts[b])
    for k, parts in attrs.items():
        setattr(st, k, parts[b])


class _TypedLoader(_Loader):
    """The program the typed-graph loaders share: seeds of ONE node type, `prefetch` mini-batches per launch of a batched
    operator, ONE read-back per launch, every per-type / per-relation slab flattened by tg_compact_rows and split per
    mini-batch, node attributes gathered per type by n_id and edge attributes per relation by e_id, one graph per
    mini-batch.  Mini-batch j of epoch e draws with call id call_id0 + e * len(loader) + j.  A subclass builds the launch
    object (_new_launch) and may say how its state is read back, what e_id is, what else a mini-batch carries and when a
    panic is raised."""
    EDGE_FIELD = "edge_index"       # the name of a relation's [2, E] tensor on a mini-batch
    REUSE_SLABS = False             # True: full launches copy their seeds into one kept launch object
    SAMPLE_TS = False               # True: the launch has sample_ts slabs, split into `ts_parts`
    input_ts = None

    def __init__(self, data, input_type, input_nodes, batch_size, drop_last, seed, call_id0, device, edge_attrs=True):
        self.data, self.device = data, torch.device(device)
        self.batch_size, self.drop_last, self.seed, self.call_id0 = int(batch_size), drop_last, int(seed), int(call_id0)
        self.hetero = _is_hetero(data)
        if self.hetero:
            self.node_types, self.edge_types = list(data.node_types), list(data.edge_types)
            if input_type not in self.node_types:
                raise ValueError("input_type must name one of the node types %s" % self.node_types)
            stores = [data[t] for t in self.node_types]
        else:                                                       # one unnamed node type, one unnamed relation
            self.node_types, self.edge_types, input_type, stores = [None], [None], None, [data]
        self.input_type = input_type
        self._tix = {t: i for i, t in enumerate(self.node_types)}
        self._it = self._tix[input_type]
        n_in = _num_nodes(stores[self._it])
        self.input_nodes = _checked_inputs(input_nodes, n_in, self.device)   # an input indexes the rows of its type unchecked
        self._node_attrs = [self._attrs_of(st, _num_nodes(st)) for st in stores]
        self._edge_attrs = [self._attrs_of(data[et], int(data[et].edge_index.shape[1])) if edge_attrs else []
                            for et in self.edge_types]
        self.epoch = 0
        self._launch = {}                                           # (calls, seeds per call) -> the kept launch object

    def _attrs_of(self, store, n):
        """The tensors of a store that have one row per node (per edge), on the device."""
        return [(k, v.to(self.device)) for k, v in _tensor_items(store)
                if k != "edge_index" and v.dim() > 0 and v.shape[0] == n]

    def _quotas(self, quotas, name):
        """Per-hop quotas, one list for every node type or a dict per type -> (dict per type, number of hops)."""
        if isinstance(quotas, dict):
            per_type = {k: [int(x) for x in v] for k, v in quotas.items()}
            n_hops = max((len(v) for v in per_type.values()), default=0)
        else:
            n_hops = len(quotas)
            per_type = {nt: [int(x) for x in quotas] for nt in self.node_types}
        for nt, v in per_type.items():
            if len(v) < n_hops:
                raise ValueError("%s[%s] is shorter than the number of hops" % (name, nt))
        return per_type, n_hops

    def _csc_rels(self, fifth):
        """Ingests every relation as a CSC (col_ptrs, row_indices, perm: CSC position -> COO edge id) -> the operators'
        `rels` tuples, with fifth(edge type) as their fifth entry."""
        self.col_ptrs, self.row_indices, self.perm = to_hetero_csc(self.data, self.device)
        return [(self._tix[et[0]], self._tix[et[2]], self.col_ptrs[rel_key(et)], self.row_indices[rel_key(et)], fifth(et))
                for et in self.edge_types]

    # ---- what a subclass fills in
    def _new_launch(self, inputs, input_ts, n_calls):
        """-> the _cabi launch object (problem, slabs, run) for n_calls mini-batches; inputs / input_ts: per node type a
        [n_calls, seeds] tensor or None (input_ts None: no timestamps)."""
        raise NotImplementedError

    def _post_run(self, slabs):
        """Called directly behind slabs.run(...), before the read-back: may launch more work on the slabs and return
        another object with their fields (samples, rows, cols, edge_index, counts) that is read back and flattened in
        their place."""
        return slabs

    def _read_back(self, slabs):
        """The launch's only read-back -> (host counts [n_calls, >= T + R], what _decorate and _check_panic want)."""
        return slabs.counts.cpu(), None

    def _e_id(self, slabs, r, cols, n_edges, total, flat_nodes):
        """COO edge ids of relation r's sampled edges, flat over the launch; None: the mini-batches carry no e_id.  Here
        the operator's edge_index is a CSC position, so e_id = perm[edge_index]."""
        return _rows_of(self.perm[rel_key(self.edge_types[r])], _flat_rows(slabs.edge_index[r], n_edges, total))

    def _decorate(self, g, b, n_seeds, state, ts_parts):
        """The loader's own extras on mini-batch b of the launch."""

    def _check_panic(self, counts, state, first_batch, b):
        """Raises where the reference would have panicked.  Called with b = None after the read-back, before any
        mini-batch of the launch is handed out, and with every b before that mini-batch is."""

    # ---- the skeleton
    def _launch_for(self, seeds: Tensor, seeds_ts: Optional[Tensor]):
        G, B = seeds.shape
        per_type = lambda x: None if x is None else [x if t == self._it else None for t in range(len(self.node_types))]
        if not self.REUSE_SLABS:
            return self._new_launch(per_type(seeds.contiguous()),
                                    per_type(None if seeds_ts is None else seeds_ts.contiguous()), G)
        slabs = self._launch.get((G, B))
        if slabs is None:  # full launches reuse one set of slabs; a shorter last launch gets its own, freed after use
            slabs = self._new_launch(per_type(seeds.clone()), per_type(None if seeds_ts is None else seeds_ts.clone()), G)
            if G == self.prefetch and B == self.batch_size:
                self._launch = {(G, B): slabs}
        else:
            slabs.inputs[self._it].copy_(seeds)
            if seeds_ts is not None:
                slabs.input_ts[self._it].copy_(seeds_ts)
        return slabs

    def _graph_of(self, b, n_seeds, node_parts, edge_parts):
        g = HeteroGraph()
        for nt, (fields, attrs) in zip(self.node_types, node_parts):
            _fill_store(g[nt], b, fields, attrs)
        g[self.input_type].batch_size = n_seeds
        for et, (fields, attrs) in zip(self.edge_types, edge_parts):
            _fill_store(g[et], b, fields, attrs)
        return g

    def _emit(self, seeds: Tensor, seeds_ts: Optional[Tensor], first_batch: int):
        G, B = seeds.shape
        T = len(self.node_types)
        slabs = self._launch_for(seeds, seeds_ts)
        slabs.run(self.seed, self.call_id0 + first_batch)
        slabs = self._post_run(slabs)
        counts, state = self._read_back(slabs)
        self._check_panic(counts, state, first_batch, None)
        flat_nodes, ts_parts, node_parts, edge_parts = [], [], [], []
        for t in range(T):
            n, lens = slabs.counts[:, t], counts[:, t].tolist()
            flat = _flat_rows(slabs.samples[t], n, sum(lens))
            flat_nodes.append(flat)
            if self.SAMPLE_TS:
                ts_parts.append(torch.split(_flat_rows(slabs.sample_ts[t], n, sum(lens)), lens))
            node_parts.append(((("n_id", torch.split(flat, lens)), ("num_nodes", lens)),
                               {k: torch.split(_rows_of(v, flat), lens) for k, v in self._node_attrs[t]}))
        for r in range(len(self.edge_types)):
            n, lens = slabs.counts[:, T + r], counts[:, T + r].tolist()
            tot = sum(lens)
            fr, fc = _flat_rows(slabs.rows[r], n, tot), _flat_rows(slabs.cols[r], n, tot)
            fe = self._e_id(slabs, r, fc, n, tot, flat_nodes)
            edge_parts.append((((self.EDGE_FIELD, torch.split(torch.stack([fr, fc]), lens, dim=1)),
                                ("e_id", None if fe is None else torch.split(fe, lens))),
                               {k: torch.split(_rows_of(v, fe), lens) for k, v in self._edge_attrs[r]}))
        for b in range(G):
            self._check_panic(counts, state, first_batch, b)
            g = self._graph_of(b, B, node_parts, edge_parts)
            self._decorate(g, b, B, state, ts_parts)
            g.call_id = self.call_id0 + first_batch + b
            yield g

    def __iter__(self):
        for (seeds, seeds_ts), first_batch in self._epoch_launches(self.input_nodes, self.input_ts):
            yield from self._emit(seeds, seeds_ts, first_batch)


class _TemporalInputs:
    """What HGTLoader and BudgetLoader add to _TypedLoader alike: temporal=True takes the edge stores' int64 `timestamps`
    as row timestamps and `input_timestamps` (one per input node) as the seeds' timestamps; the operators return a
    timestamp per sampled node, handed out per node type as the mini-batch's samples_timestamps."""
    SAMPLE_TS = True

    def _init_temporal(self, temporal, input_timestamps):
        """-> self.temporal, self._rels (CSC, with row timestamps in CSC edge order when temporal), self.input_ts"""
        self.temporal = temporal
        self._rels = self._csc_rels(lambda et: _rows_of(self.data[et].timestamps.to(self.device).to(torch.int64),
                                                        self.perm[rel_key(et)]) if temporal else None)
        if temporal:
            if input_timestamps is None:
                raise ValueError("temporal=True needs input_timestamps (one per input node)")
            self.input_ts = input_timestamps.to(self.device).reshape(-1).to(torch.int64)
            if self.input_ts.numel() != self.input_nodes.numel():
                raise ValueError("input_timestamps must have one entry per input node")

    def _decorate(self, g, b, n_seeds, state, ts_parts):
        g.samples_timestamps = {nt: ts_parts[t][b] for t, nt in enumerate(self.node_types)}


class HeteroNeighborLoader(_TypedLoader):
    """The heterogeneous counterpart of NeighborLoader: seeds of ONE node type, `prefetch` mini-batches per
    tg_ns_hetero_batched launch (all hops and relations fused, default samplers), per-type / per-relation slabs flattened
    by tg_compact_rows, node attributes gathered per type, edge attributes per relation through the ingest permutation.
    Mini-batch j of the epoch equals neighbor_sampling_heterogenous for (seed, call_id0 + j).

    unique=True hands out PyG-style mini-batches: tg_ns_typed_unique runs directly behind the sampler, in place on the edge
    slabs and before the read-back, so per node type `n_id` lists each node once (first occurrence first: distinct seeds
    lead, in order), node attributes are gathered per unique node and every relation's `edge_index` is numbered against
    the unique lists of its two types (edges are not merged).  `e_id`, the edge attributes and `layer_offsets` stay the
    forest's; `g[input_type].batch_size` is the unique-seed count.  A launch is read back in two copies, as the forest's
    is: `layer_offsets`, and the unique counts with the unique-seed counts in one tensor.  The flat form's workspace, where
    the shape needs one, and the dedup's own outputs are kept by the loader and sized once for a full launch.
    BudgetLoader, HGTLoader and NegativeLoader have no such switch yet: BudgetLoader._e_id reads `cols` as forest
    positions, so wiring them up is a later step."""
    WITH_INVERSE = False            # unique=True: keep tg_ns_typed_unique's `inverse` slabs (forest position -> n_id position)

    def __init__(self, data, num_neighbors: List[int], input_type: str, input_nodes: Optional[Tensor] = None,
                 batch_size: int = 1024, prefetch: int = 16, replace: bool = False, drop_last: bool = False, seed: int = 0,
                 call_id0: int = 0, device="cuda", unique: bool = False):
        super().__init__(data, input_type, input_nodes, batch_size, drop_last, seed, call_id0, device)
        self.fanout, self.prefetch = [int(k) for k in num_neighbors], max(1, int(prefetch))
        self.sampler = _cabi.SAMPLER_UNIFORM_REPL if replace else _cabi.SAMPLER_UNIFORM
        self._rels = self._csc_rels(lambda et: self.fanout)
        self.unique = bool(unique)
        self._id_bounds = [max(_num_nodes(data[t]), 1) for t in self.node_types]
        self._unique_ws = None              # the dedup's tables (flat form), sized once for a full launch
        self._unique_out = None             # its node slabs and counts for a full launch (the edge slabs are the sampler's)
        self._unique_need = 0               # ... and the workspace bytes that launch asks for (0: the LDS form)

    def _new_launch(self, inputs, input_ts, n_calls):
        return _cabi.NsHeteroBatched(len(self.node_types), self._rels, inputs, len(self.fanout), n_calls, self.device,
                                     sampler=self.sampler)

    def _post_run(self, slabs):
        if not self.unique:
            return slabs
        shapes = [x.shape for x in slabs.samples]
        out, need = self._unique_out, self._unique_need             # a full launch's outputs and plan are kept
        if out is None or [x.shape for x in out.nodes] != shapes:
            full = max(slabs.nb, min(self.prefetch, len(self)))
            need = _cabi.ns_typed_unique_workspace_bytes([s[1] for s in shapes], self._id_bounds, full)[0]
            if need and (self._unique_ws is None or self._unique_ws.numel() * 8 < need):    # 0: the LDS form takes none
                self._unique_ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=self.device)
            out = _cabi.NsTypedUniqueOut(slabs, in_place=True, with_inverse=self.WITH_INVERSE)
            if slabs.nb == full and slabs.n_inputs[self._it] == self._seed_width(self.batch_size):
                self._unique_out, self._unique_need = out, need
        return _cabi.ns_typed_unique(slabs, slabs.nb, self._id_bounds, ws=self._unique_ws if need else None,
                                     form=0 if need else 1, result=out.rebind(slabs))

    def _seed_width(self, width: int) -> int:
        """Inputs of the input type in a mini-batch of `width` work items (here the work items are the seeds)."""
        return width

    def _read_back(self, slabs):
        lo = slabs.layer_offsets.cpu().tolist()
        if not self.unique:
            return slabs.counts.cpu(), (lo, None)
        counts, seed_counts = slabs.read_state()                    # the unique counts and the unique seeds in one copy
        return counts, (lo, seed_counts[:, self._it].tolist())

    def _decorate(self, g, b, n_seeds, state, ts_parts):
        lo, seed_counts = state
        for r, et in enumerate(self.edge_types):
            g[et].layer_offsets = [tuple(x) for x in lo[b][r][:len(self.fanout)]]
        if seed_counts is not None:
            g[self.input_type].batch_size = seed_counts[b]


class HGTLoader(_TemporalInputs, _TypedLoader):
    """HGT budget sampling (hgt_sampling) as a loader: seeds of ONE node type, `prefetch` mini-batches per
    tg_hgt_sample_batched launch chain, one read-back of the counts per launch, per-type / per-relation slabs flattened
    by tg_compact_rows, node attributes gathered per type and edge attributes per relation through the ingest
    permutation (as HeteroNeighborLoader).  num_samples: one list of per-hop quotas for every node type (as
    HGTSamplerTransform) or a dict per type.  temporal=True uses the edge stores' int64 `timestamps` as row timestamps,
    `input_timestamps` (one per input node) as the seeds' timestamps and `timerange` = [lo, hi).

    Mini-batch j of the epoch equals hgt_sampling for (seed, call_id0 + j); every epoch draws fresh call ids.  A
    launch's workspace is prefetch x tg_hgt_batched_workspace_bytes(one call): prefetch is clamped so that it stays
    within `max_workspace_bytes` (default 4 GiB; at least one mini-batch per launch)."""

    def __init__(self, data, num_samples, input_type: str, input_nodes: Optional[Tensor] = None, batch_size: int = 1024,
                 prefetch: int = 64, temporal: bool = False, input_timestamps: Optional[Tensor] = None, timerange=None,
                 drop_last: bool = False, seed: int = 0, call_id0: int = 0, max_workspace_bytes: int = 4 << 30,
                 device="cuda"):
        super().__init__(data, input_type, input_nodes, batch_size, drop_last, seed, call_id0, device)
        self.num_samples, self.n_hops = self._quotas(num_samples, "num_samples")
        self.timerange = None if timerange is None else (int(timerange[0]), int(timerange[1]))
        self._init_temporal(temporal, input_timestamps)
        per_call = _cabi.hgt_batched_workspace_bytes(self._problem(self.batch_size), 1)
        self.prefetch = max(1, min(int(prefetch), int(max_workspace_bytes) // per_call))

    def _num_samples(self):
        return [self.num_samples.get(nt) for nt in self.node_types]

    def _problem(self, n_seeds):
        """A host-only problem of the loader's shape (sizes the workspace; nothing is launched)."""
        n_in = [n_seeds if nt == self.input_type else -1 for nt in self.node_types]
        return _cabi.hgt_problem(len(self.node_types), self._rels, n_in, self._num_samples(), self.n_hops)

    def _new_launch(self, inputs, input_ts, n_calls):
        return _cabi.HgtBatched(len(self.node_types), self._rels, inputs, self._num_samples(), self.n_hops, n_calls,
                                self.device, input_ts=input_ts, timerange=self.timerange if self.temporal else None)

    def _check_panic(self, counts, state, first_batch, b):
        if b is None:                                               # the whole launch, before any mini-batch is handed out
            word = len(self.node_types) + len(self.edge_types)
            panicked = [j for j in range(counts.shape[0]) if int(counts[j, word]) != 0]
            if panicked:
                raise RuntimeError("HGTLoader: mini-batch %d: a weight sum was not positive, or a node type that owns a "
                                   "budget has no num_samples entry (the reference panics here)"
                                   % (first_batch + panicked[0]))


class BudgetLoader(_TemporalInputs, _TypedLoader):
    """Temporal heterogeneous budget sampling (budget_sampling) as a loader: seeds of ONE node type, `prefetch`
    mini-batches per tg_budget_sample_batched launch chain, one read-back of the counts per launch, per-type /
    per-relation slabs flattened by tg_compact_rows, node attributes gathered per type and edge attributes per relation.
    num_neighbors: one list of per-hop quotas for every node type or a dict per type.  temporal=True uses the edge
    stores' int64 `timestamps` as row timestamps and `input_timestamps` (one per input node) as the seeds' timestamps;
    `window` = [lo, hi) turns the temporal filter on, with `forward` / `relative` as in budget_sampling.

    The operator's edge_index is the neighbour's index inside its CSC column (a quirk kept from the reference,
    budget_sampling.rs:116), so e_id = perm[col_ptrs[n_id_dst[col]] + edge_index], computed on the device.

    Mini-batch j of the epoch equals budget_sampling for (seed, call_id0 + j); every epoch draws fresh call ids.  A
    launch's device memory is prefetch x (workspace + output slabs + counts of one call): the slabs are sized for the
    worst case and dominate, so prefetch is clamped to keep both within `max_workspace_bytes` (default 4 GiB; at least
    one mini-batch per launch).  Full launches reuse one set of slabs."""
    REUSE_SLABS = True

    def __init__(self, data, num_neighbors, input_type: str, input_nodes: Optional[Tensor] = None, batch_size: int = 1024,
                 prefetch: int = 64, temporal: bool = False, input_timestamps: Optional[Tensor] = None, window=None,
                 forward: bool = False, relative: bool = False, drop_last: bool = False, seed: int = 0, call_id0: int = 0,
                 max_workspace_bytes: int = 4 << 30, device="cuda"):
        super().__init__(data, input_type, input_nodes, batch_size, drop_last, seed, call_id0, device)
        nn, self.n_hops = self._quotas(num_neighbors, "num_neighbors")
        for nt in self.node_types:
            if self.n_hops and nt not in nn:
                raise ValueError("num_neighbors has no entry for node type %s (budget_sampling panics here)" % nt)
        self.num_neighbors = [nn[nt][:self.n_hops] if self.n_hops else [] for nt in self.node_types]
        self.window = None if window is None else (int(window[0]), int(window[1]))
        self.forward, self.relative = bool(forward), bool(relative)
        self._init_temporal(temporal, input_timestamps)
        per_call = _cabi.budget_batched_bytes(self._problem(self.batch_size), 1)
        self.prefetch = max(1, min(int(prefetch), int(max_workspace_bytes) // per_call))

    def _problem(self, n_seeds):
        """A host-only problem of the loader's shape (sizes a launch; nothing is launched)."""
        n_in = [n_seeds if nt == self.input_type else 0 for nt in self.node_types]
        return _cabi.budget_problem(len(self.node_types), self._rels, n_in, self.num_neighbors, self.n_hops)

    def _new_launch(self, inputs, input_ts, n_calls):
        return _cabi.BudgetBatched(len(self.node_types), self._rels, inputs, self.num_neighbors, self.n_hops, n_calls,
                                   self.device, input_ts=input_ts, window=self.window, forward=self.forward,
                                   relative=self.relative)

    def _e_id(self, slabs, r, cols, n_edges, total, flat_nodes):
        # the destination's node id -> its column start in the CSC -> + index inside the column -> COO edge id
        et = self.edge_types[r]
        key, d = rel_key(et), self._tix[et[2]]
        n_dst = slabs.counts[:, d]
        node_off = torch.cumsum(n_dst, 0) - n_dst                   # where call b's nodes start in flat_nodes[d]
        w = _rows_of(flat_nodes[d], cols + torch.repeat_interleave(node_off, n_edges, output_size=total))
        return _rows_of(self.perm[key], _rows_of(self.col_ptrs[key], w) + _flat_rows(slabs.edge_index[r], n_edges, total))


class NegativeLoader(_TypedLoader):
    """Negative sampling (negative_sample_neighbors_homogenous / _heterogenous) as a loader: `prefetch` mini-batches per
    tg_neg_sample_batched launch (one workgroup runs one whole mini-batch in LDS where its shape fits, tchgeo.h), ONE
    read-back per launch (counts and panic words together), slabs flattened by tg_compact_rows and node attributes gathered
    once per launch and split.  Full launches reuse one set of slabs.

    Homogeneous `data`: yields what NegativeSamplerTransform returns for the mini-batch's inputs (n_id, num_nodes,
    neg_edge_index, batch_size, node attributes gathered by n_id) plus `call_id`.  Heterogeneous `data`: the seeds are of ONE
    node type (`input_type`); yields a HeteroGraph with the same fields per node type and neg_edge_index per relation, as
    the transform does for inputs = {input_type: seeds}.

    Mini-batch j of epoch e equals the transform for (seed, call_id0 + e * len(loader) + j).  Where the reference would
    panic in a mini-batch (inbound, a drawn row out of range; negative_sampling.rs:113) the transform's RuntimeError is
    raised when that mini-batch is reached, not earlier.  A launch's device memory is the workspace plus prefetch x the
    slabs of one call; prefetch is clamped to keep it within `max_workspace_bytes` (at least one mini-batch per launch)."""
    EDGE_FIELD, REUSE_SLABS = "neg_edge_index", True

    PANIC = ("inbound negative sampling indexed a CSR row out of range (the reference panics here, "
             "negative_sampling.rs:113)")

    def __init__(self, data, num_neg: int, try_count: int, input_nodes: Optional[Tensor] = None,
                 input_type: Optional[str] = None, batch_size: int = 1024, prefetch: int = 256, inbound: bool = False,
                 drop_last: bool = False, seed: int = 0, call_id0: int = 0, max_workspace_bytes: int = 4 << 30, device="cuda"):
        self.num_neg, self.try_count = int(num_neg), int(try_count)
        if self.num_neg < 0 or self.try_count < 0:
            raise ValueError("num_neg and try_count must be >= 0")
        super().__init__(data, input_type, input_nodes, batch_size, drop_last, seed, call_id0, device, edge_attrs=False)
        # the homogeneous operator has no inbound form (the transform ignores the flag)
        self.inbound = bool(inbound) and self.hetero
        if self.hetero:
            self._rels = []
            for et in self.edge_types:
                size = (_num_nodes(data[et[0]]), _num_nodes(data[et[2]]))
                if size[1] < 1:
                    raise ValueError("relation %s has an empty destination range" % (et,))
                ptrs, idx, _ = _host.to_csr(data[et].edge_index.to(self.device), size)
                self._rels.append((self._tix[et[0]], self._tix[et[2]], ptrs, idx, size[1]))
        else:
            n = _num_nodes(data)
            ptrs, idx, _ = _host.to_csr(data.edge_index.to(self.device), n)
            self._rels = [(0, 0, ptrs, idx, n)]
        per_call = max(1, _cabi.neg_batched_bytes(self._problem(self.batch_size), 1))
        self.prefetch = max(1, min(int(prefetch), int(max_workspace_bytes) // per_call, _cabi.TG_NEG_MAX_CALLS))

    def _problem(self, n_seeds):
        """A host-only problem of the loader's shape (sizes a launch; nothing is launched)."""
        n_in = [n_seeds if t == self._it else -1 for t in range(len(self.node_types))]
        return _cabi.neg_problem(len(self.node_types), self._rels, n_in, self.num_neg, self.try_count, None, self.inbound,
                                 not self.hetero)

    def _new_launch(self, inputs, input_ts, n_calls):
        return _cabi.NegBatched(len(self.node_types), self._rels, inputs, self.num_neg, self.try_count, n_calls,
                                self.device, self.inbound, not self.hetero)

    def _read_back(self, slabs):
        return slabs.read_state()                                   # counts and panic words in one read-back

    def _e_id(self, slabs, r, cols, n_edges, total, flat_nodes):
        return None                                                 # a negative edge is no edge of the graph

    def _check_panic(self, counts, state, first_batch, b):
        if b is not None and int(state[b]) != 0:                    # when the panicking mini-batch is reached
            raise RuntimeError(self.PANIC)

    def _graph_of(self, b, n_seeds, node_parts, edge_parts):
        if self.hetero:
            return super()._graph_of(b, n_seeds, node_parts, edge_parts)
        g = Graph()                                                 # the homogeneous form: one flat container
        _fill_store(g, b, *node_parts[0])
        _fill_store(g, b, *edge_parts[0])
        g.batch_size = n_seeds
        return g

    def _decorate(self, g, b, n_seeds, state, ts_parts):
        if self.hetero:                                             # as the transform: every node type says how many seeds
            for t, nt in enumerate(self.node_types):
                g[nt].batch_size = n_seeds if t == self._it else 0


class SkipGramBatch:
    """One Node2Vec mini-batch: `pos_rw` [nw * R * B, C] context windows of the walks, `neg_rw` [nw * R * K * B, C] windows
    of the negative rows (views of the launch's slabs), `batch_size` = B seeds, `call_id`.  A walk that met a dead end is
    padded with -1, and so are its windows: mask with (pos_rw >= 0).all(1)."""
    __slots__ = ("pos_rw", "neg_rw", "batch_size", "call_id")

    def __init__(self, pos_rw, neg_rw, batch_size, call_id):
        self.pos_rw, self.neg_rw, self.batch_size, self.call_id = pos_rw, neg_rw, batch_size, call_id


class SkipGramSuperBatch(_Indexable):
    """The mini-batches of ONE tg_rw_skipgram launch: `pos_rw` [G, nw * R * B, C], `neg_rw` [G, nw * R * K * B, C], batch-major,
    `batch_size`, `call_id0` (mini-batch g drew with call_id0 + g).  Iterating or indexing yields SkipGramBatch views."""
    __slots__ = ("pos_rw", "neg_rw", "batch_size", "call_id0")

    def __init__(self, pos_rw, neg_rw, batch_size, call_id0):
        self.pos_rw, self.neg_rw, self.batch_size, self.call_id0 = pos_rw, neg_rw, batch_size, call_id0

    def __len__(self):
        return self.pos_rw.shape[0]

    def _at(self, g):
        return SkipGramBatch(self.pos_rw[g], self.neg_rw[g], self.batch_size, self.call_id0 + g)


class Node2VecLoader(_Loader):
    """Node2Vec training batches (the reference's examples/random_walk.py: positive walks, negative rows, context windows)
    as a loader: ONE tg_rw_skipgram launch walks `prefetch` mini-batches, cuts every walk into its context windows in LDS
    and draws the negatives; nothing is read back, so a launch costs the host one call.  `walk_length` counts steps (rows
    of walk_length + 1 nodes, as random_walk), `context_size` <= walk_length + 1, each seed starts `walks_per_node` walks
    and `walks_per_node * num_negative_samples` negative rows.  Windows of a walk that met a dead end carry its -1 padding.

    The CSR is built once, on first use; so is the edge set that answers has_edge in one probe, when p, q make the
    acceptance probabilities differ and the ids fit its 32-bit halves.  Mini-batch j of epoch e equals _cabi.rw_skipgram
    for (seed, call_id0 + e * len(loader) + j); the ragged last mini-batch is a launch of its own.  A launch's device
    memory is prefetch x (the two slabs + the flat form's workspace of one mini-batch): prefetch is clamped to keep it
    within `max_workspace_bytes` (at least one mini-batch per launch).  `form` is tg_rw_skipgram's (0 auto)."""

    def __init__(self, data, walk_length: int, context_size: int, walks_per_node: int = 1, num_negative_samples: int = 1,
                 p: float = 1.0, q: float = 1.0, input_nodes: Optional[Tensor] = None, batch_size: int = 128,
                 prefetch: int = 256, drop_last: bool = False, seed: int = 0, call_id0: int = 0,
                 max_workspace_bytes: int = 4 << 30, device="cuda", form: int = 0):
        self.data, self.device = data, torch.device(device)
        self.n_nodes = _num_nodes(data)
        self.p, self.q = float(p), float(q)
        # refuses a bad shape here, on the host (C > L, R < 1, K < 0, ...)
        self.cfg = _cabi.rw_skipgram_config(walk_length, context_size, walks_per_node, num_negative_samples, self.n_nodes,
                                            self.p, self.q)
        self._batching(batch_size, drop_last, seed, call_id0)
        self.form = int(form)
        self.input_nodes = _checked_inputs(input_nodes, self.n_nodes)
        pos_rows, neg_rows = _cabi.rw_skipgram_capacity(self.cfg, self.batch_size)
        self._clamp_prefetch(prefetch, max_workspace_bytes, (pos_rows + neg_rows) * self.cfg.context_size * 8 +
                             _cabi.rw_skipgram_workspace_bytes(self.cfg, 1, self.batch_size, self.n_nodes, self.form))
        self._graph = self._edge_set = self._ws = None
        self.epoch = 0

    def _batching(self, batch_size, drop_last, seed, call_id0):
        self.batch_size, self.drop_last, self.seed, self.call_id0 = int(batch_size), drop_last, int(seed), int(call_id0)
        if self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")

    def _clamp_prefetch(self, prefetch, max_workspace_bytes, per_call: int):
        """prefetch x the device memory of one mini-batch stays within max_workspace_bytes (at least one per launch)"""
        self.prefetch = max(1, min(int(prefetch), int(max_workspace_bytes) // max(per_call, 1)))

    def _workspace(self, need: int):
        """The kept workspace, grown to at least `need` bytes (None while no launch has needed one)."""
        if need and (self._ws is None or self._ws.numel() * 8 < need):
            self._ws = torch.empty(need // 8, dtype=torch.int64, device=self.device)
        return self._ws

    def plan(self, epoch: int):
        """The launches of an epoch: [(start, n_batches, batch_width, first call id)] over input_nodes."""
        batch0 = epoch * len(self)
        return [(start, G, width, self.call_id0 + batch0 + start // self.batch_size)
                for start, G, width in _epoch_plan(self.input_nodes.numel(), self.batch_size, self.prefetch, self.drop_last)]

    def _prepare(self):
        if self._graph is not None:
            return
        self.input_nodes = self.input_nodes.to(self.device)
        self.row_ptrs, self.col_indices, _ = _host.to_csr(self.data.edge_index.to(self.device), self.n_nodes)
        self._graph = _shadowed_view(self.row_ptrs, self.col_indices,
                                     self.n_nodes < 2 ** 31 and self.col_indices.numel() < 2 ** 31)
        if not (self.p == 1.0 and self.q == 1.0) and self.n_nodes < 2 ** 32 - 1:
            self._edge_set = _cabi.edge_set(self._graph, self.device)

    def _launch(self, seeds: Tensor, call_id: int) -> SkipGramSuperBatch:
        c = self.cfg
        ws = self._workspace(_cabi.rw_skipgram_workspace_bytes(c, seeds.shape[0], seeds.shape[1], self.n_nodes, self.form))
        pos, neg = _cabi.rw_skipgram(self._graph, seeds, c.walk_length, c.context_size, c.walks_per_node,
                                     c.num_negative_samples, self.p, self.q, self.seed, call_id, self.n_nodes,
                                     edge_set=self._edge_set, form=self.form, ws=ws)
        return SkipGramSuperBatch(pos, neg, seeds.shape[1], call_id)

    def super_batches(self) -> Iterator[SkipGramSuperBatch]:
        """The epoch launch by launch: the [G, rows, C] slabs of up to `prefetch` mini-batches."""
        self._prepare()
        launches = self.plan(self.epoch)                             # fresh draws every epoch (see NeighborLoader)
        self.epoch += 1
        for start, G, width, call_id in launches:
            yield self._launch(*self._launch_inputs(start, G, width), call_id)

    def _launch_inputs(self, start: int, G: int, width: int):
        """what _launch takes ahead of the call id: the [G, width] rows of every per-input tensor"""
        return (self.input_nodes[start:start + G * width].reshape(G, width).contiguous(),)


class MetaPath2VecLoader(Node2VecLoader):
    """MetaPath2Vec training batches (PyG's MetaPath2Vec: walks along a metapath of a typed graph, negative rows drawn per
    column type, context windows) as a loader: ONE tg_mp_skipgram launch per `prefetch` mini-batches.  `metapath` is a
    list of edge types (src, rel, dst) of `data`, each ending where the next starts; step l of a walk goes over
    metapath[l mod len(metapath)], so walk_length > len(metapath) needs a path that closes.  PyG's conventions: `start` /
    `end` of every node type in ONE embedding table of `num_embeddings` = `dummy_idx` + 1 rows (types in data.node_types
    order, dummy_idx = the total node count).  global_ids=True emits table rows (local id + start of the column's type)
    and pads an ended walk with dummy_idx, whose row a trainer leaves alone or masks; global_ids=False emits local ids
    and -1.  input_nodes are local ids of metapath[0][0] (default: all of them).

    The CSR of every distinct relation of the metapath is built once, on first use, and shared where a relation repeats.
    The epoch plan, the call ids, the prefetch clamp, plan(), super_batches() and iteration are Node2VecLoader's:
    mini-batch j of epoch e equals _cabi.mp_skipgram for (seed, call_id0 + e * len(loader) + j)."""

    def __init__(self, data, metapath, walk_length: int, context_size: int, walks_per_node: int = 1,
                 num_negative_samples: int = 1, input_nodes: Optional[Tensor] = None, batch_size: int = 128,
                 prefetch: int = 256, drop_last: bool = False, seed: int = 0, call_id0: int = 0, global_ids: bool = True,
                 max_workspace_bytes: int = 4 << 30, device="cuda", form: int = 0):
        self.data, self.device = data, torch.device(device)
        self.node_types, self.metapath = list(data.node_types), [tuple(et) for et in metapath]
        tix = {t: i for i, t in enumerate(self.node_types)}
        M = len(self.metapath)
        if not 1 <= M <= _cabi.TG_MP_MAX_STEPS:
            raise ValueError("metapath must have 1 to %d steps, got %d" % (_cabi.TG_MP_MAX_STEPS, M))
        known = [tuple(et) for et in data.edge_types]
        for m, et in enumerate(self.metapath):
            if et not in known:
                raise ValueError("metapath step %d: %s is not an edge type of the graph" % (m, et))
            nxt = self.metapath[m + 1] if m + 1 < M else None
            if nxt is not None and et[2] != nxt[0]:
                raise ValueError("metapath step %d: broken chain, it ends at %r and step %d starts at %r" % (m, et[2], m + 1, nxt[0]))
        if int(walk_length) > M and self.metapath[-1][2] != self.metapath[0][0]:
            raise ValueError("metapath step %d: open path, it ends at %r, not at %r where step 0 starts, and walk_length = %d > %d "
                             "steps" % (M - 1, self.metapath[-1][2], self.metapath[0][0], int(walk_length), M))
        self.type_count = [_num_nodes(data[t]) for t in self.node_types]
        self.start, self.end, total = {}, {}, 0
        for t, n in zip(self.node_types, self.type_count):
            self.start[t], self.end[t] = total, total + n
            total += n
        self.dummy_idx, self.num_embeddings, self.global_ids = total, total + 1, bool(global_ids)
        self._step_src, self._step_dst = [tix[et[0]] for et in self.metapath], [tix[et[2]] for et in self.metapath]
        self._n_edges = [int(data[et].edge_index.shape[1]) for et in self.metapath]
        self._batching(batch_size, drop_last, seed, call_id0)
        self.form = int(form)
        self._shape = (int(walk_length), int(context_size), int(walks_per_node), int(num_negative_samples))
        # sizes only: refuses a bad shape here, on the host (C > L, R < 1, K < 0, ...); _prepare puts the CSRs behind it
        self.cfg = self._config([_cabi.graph_sizing(self.type_count[s], e) for s, e in zip(self._step_src, self._n_edges)])
        n_in = self.type_count[self._step_src[0]]
        self.input_nodes = _checked_inputs(input_nodes, n_in)
        pos_rows, neg_rows = _cabi.mp_skipgram_capacity(self.cfg, self.batch_size)
        self._clamp_prefetch(prefetch, max_workspace_bytes, (pos_rows + neg_rows) * self.cfg.context_size * 8 +
                             _cabi.mp_skipgram_workspace_bytes(self.cfg, 1, self.batch_size, self.form))
        self._graph = self._ws = None
        self.epoch = 0

    def _config(self, graphs):
        starts = [self.start[t] for t in self.node_types] if self.global_ids else None
        return _cabi.mp_skipgram_config(graphs, self._step_src, self._step_dst, self.type_count, *self._shape,
                                        type_start=starts, pad_value=self.dummy_idx if self.global_ids else -1)

    def _prepare(self):
        if self._graph is not None:
            return
        self.input_nodes = self.input_nodes.to(self.device)
        self._graph = {}                                             # edge type -> its CSR view, built once
        for et, s, d in zip(self.metapath, self._step_src, self._step_dst):
            if et in self._graph:
                continue
            n_src, n_dst = self.type_count[s], self.type_count[d]
            ptrs, idx, _ = _host.to_csr(self.data[et].edge_index.to(self.device), (n_src, n_dst))
            self._graph[et] = _shadowed_view(ptrs, idx, max(n_src, n_dst) < 2 ** 31 and idx.numel() < 2 ** 31)
        self.cfg = self._config([self._graph[et] for et in self.metapath])

    def _launch(self, seeds: Tensor, call_id: int) -> SkipGramSuperBatch:
        ws = self._workspace(_cabi.mp_skipgram_workspace_bytes(self.cfg, seeds.shape[0], seeds.shape[1], self.form))
        pos, neg = _cabi.mp_skipgram(self.cfg, seeds, self.seed, call_id, form=self.form, ws=ws)
        return SkipGramSuperBatch(pos, neg, seeds.shape[1], call_id)


class TemporalSkipGramBatch:
    """One temporal skip-gram mini-batch: `pos_rw` [nw * R * B, C] context windows of the temporal walks, `pos_ts` the
    timestamp of every word of pos_rw (-1: none; None when the loader was built with with_timestamps=False), `neg_rw`
    [nw * R * K * B, C] windows of the negative rows (views of the launch's slabs), `batch_size` = B seeds, `call_id`.  A
    temporal walk restarts instead of ending: there is no padding."""
    __slots__ = ("pos_rw", "pos_ts", "neg_rw", "batch_size", "call_id")

    def __init__(self, pos_rw, pos_ts, neg_rw, batch_size, call_id):
        self.pos_rw, self.pos_ts, self.neg_rw, self.batch_size, self.call_id = pos_rw, pos_ts, neg_rw, batch_size, call_id


class TemporalSkipGramSuperBatch(_Indexable):
    """The mini-batches of ONE tg_tempo_skipgram launch: `pos_rw`, `pos_ts` (or None) [G, nw * R * B, C], `neg_rw` [G, nw * R *
    K * B, C], batch-major, `batch_size`, `call_id0` (mini-batch g drew with call_id0 + g).  Iterating or indexing yields
    TemporalSkipGramBatch views."""
    __slots__ = ("pos_rw", "pos_ts", "neg_rw", "batch_size", "call_id0")

    def __init__(self, pos_rw, pos_ts, neg_rw, batch_size, call_id0):
        self.pos_rw, self.pos_ts, self.neg_rw, self.batch_size, self.call_id0 = pos_rw, pos_ts, neg_rw, batch_size, call_id0

    def __len__(self):
        return self.pos_rw.shape[0]

    def _at(self, g):
        return TemporalSkipGramBatch(self.pos_rw[g], None if self.pos_ts is None else self.pos_ts[g], self.neg_rw[g],
                                     self.batch_size, self.call_id0 + g)


class TemporalWalkLoader(Node2VecLoader):
    """CTDNE-style training batches (temporal walks, their context windows and timestamps, negative rows) as a loader: ONE
    tg_tempo_skipgram launch per `prefetch` mini-batches; nothing is read back.  `walk_length` counts COLUMNS of a walk, as
    tempo_random_walk does (the start node is column 0) -- Node2VecLoader's counts steps, one less.  `context_size` <=
    walk_length; `window` = (lo, hi) is the walk's half-open time window relative to a walker's start time.  Each seed
    starts `walks_per_node` walks and `walks_per_node * num_negative_samples` negative rows.

    `edge_timestamps`: int64 [E] in data.edge_index order (default: data.timestamps); `node_timestamps`: [N], used for an
    edge without a timestamp (default: all -1); `input_timestamps`: one start time per input node (default: all -1 = no
    start time, every edge admissible), sliced exactly as input_nodes.  with_timestamps=False leaves pos_ts out (None).

    The CSR and the timestamps in its edge order are built once, on first use.  The epoch plan, the call ids, the prefetch
    clamp, plan(), super_batches() and iteration are Node2VecLoader's: mini-batch j of epoch e equals
    _cabi.tempo_skipgram for (seed, call_id0 + e * len(loader) + j); the ragged last mini-batch is a launch of its own."""

    def __init__(self, data, walk_length: int, context_size: int, window, walks_per_node: int = 1,
                 num_negative_samples: int = 1, edge_timestamps: Optional[Tensor] = None,
                 node_timestamps: Optional[Tensor] = None, input_nodes: Optional[Tensor] = None,
                 input_timestamps: Optional[Tensor] = None, with_timestamps: bool = True, batch_size: int = 128,
                 prefetch: int = 256, drop_last: bool = False, seed: int = 0, call_id0: int = 0,
                 max_workspace_bytes: int = 4 << 30, device="cuda"):
        self.data, self.device = data, torch.device(device)
        self.n_nodes = _num_nodes(data)
        self.window = (int(window[0]), int(window[1]))
        if self.window[0] >= self.window[1]:
            raise ValueError("window = %r is empty: it is half open, window[0] < window[1]" % (window,))
        self.cfg = _cabi.tempo_skipgram_config(walk_length, context_size, self.window, walks_per_node, num_negative_samples,
                                               self.n_nodes)
        self._batching(batch_size, drop_last, seed, call_id0)
        try:                                                      # the library's own refusals (C > L, R < 1, K < 0, too long ...)
            pos_rows, neg_rows = _cabi.tempo_skipgram_capacity(self.cfg, self.batch_size)
            _cabi.tempo_skipgram_lds_bytes(self.cfg)
        except _cabi.TchGeoError as e:
            raise ValueError(str(e)) from None
        n_edges = int(data.edge_index.shape[1])
        ets = getattr(data, "timestamps", None) if edge_timestamps is None else edge_timestamps
        if ets is None:
            raise ValueError("the graph has no `timestamps`: pass edge_timestamps (int64, one per edge in edge_index order)")
        if ets.numel() != n_edges:
            raise ValueError("edge_timestamps must have one entry per edge (%d), got %d" % (n_edges, ets.numel()))
        if node_timestamps is not None and node_timestamps.numel() != self.n_nodes:
            raise ValueError("node_timestamps must have one entry per node (%d), got %d" % (self.n_nodes, node_timestamps.numel()))
        self._edge_ts_in, self._node_ts_in = ets, node_timestamps
        self.input_nodes = _checked_inputs(input_nodes, self.n_nodes)
        if input_timestamps is None:
            input_timestamps = torch.full((self.input_nodes.numel(),), -1, dtype=torch.int64)
        self.input_ts = input_timestamps.reshape(-1).to(torch.int64)
        if self.input_ts.numel() != self.input_nodes.numel():
            raise ValueError("input_timestamps must have one entry per input node")
        self.with_timestamps = bool(with_timestamps)
        self._clamp_prefetch(prefetch, max_workspace_bytes,
                             ((2 if self.with_timestamps else 1) * pos_rows + neg_rows) * self.cfg.context_size * 8)
        self._graph = None
        self.epoch = 0

    def _prepare(self):
        if self._graph is not None:
            return
        self.input_nodes, self.input_ts = self.input_nodes.to(self.device), self.input_ts.to(self.device)
        self.row_ptrs, self.col_indices, perm = _host.to_csr(self.data.edge_index.to(self.device), self.n_nodes)
        ets = self._edge_ts_in.to(self.device).reshape(-1).to(torch.int64)
        self.edge_ts = ets[perm] if ets.numel() else ets             # into CSR edge order
        self.node_ts = torch.full((self.n_nodes,), -1, dtype=torch.int64, device=self.device) if self._node_ts_in is None \
            else self._node_ts_in.to(self.device).reshape(-1).to(torch.int64).contiguous()
        self._graph = _cabi.graph_view(self.row_ptrs, self.col_indices)

    def _launch_inputs(self, start: int, G: int, width: int):
        return super()._launch_inputs(start, G, width) + (self.input_ts[start:start + G * width].reshape(G, width).contiguous(),)

    def _launch(self, seeds: Tensor, seeds_ts: Tensor, call_id: int) -> TemporalSkipGramSuperBatch:
        pos, pts, neg = _cabi.tempo_skipgram(self._graph, self.node_ts, self.edge_ts, seeds, seeds_ts, self.cfg, self.seed,
                                             call_id, with_ts=self.with_timestamps)
        return TemporalSkipGramSuperBatch(pos, pts, neg, seeds.shape[1], call_id)


class LinkSuperBatch(SuperBatch):
    """A SuperBatch of a LinkNeighborLoader: the G mini-batches of ONE tg_link_seeds + tg_ns_homo_batched launch, plus the
    link fields as batch-major tensors (row g is mini-batch g's, numbered against ITS n_id): `input_id` [G, E],
    `neg_unverified` [G], `batch_size` = E; binary: `edge_label_index` [G, 2, P], `edge_label` [G, P]; triplet:
    `src_index`, `dst_pos_index` [G, E], `dst_neg_index` [G, E, K] (`edge_label` [G, E] only when the user gave labels); from a
    temporal loader `edge_label_time` [G, P] (triplet: [G, E]; else None)."""
    __slots__ = ("neg_sampling", "edge_label_index", "edge_label", "src_index", "dst_pos_index", "dst_neg_index", "input_id",
                 "neg_unverified", "edge_label_time")

    def _at(self, j):
        return LinkMiniBatch(self, j)


def _row_of(name):
    def get(self):
        t = getattr(self._sb, name)
        return None if t is None else t[self._j]
    return property(get)


class LinkMiniBatch(MiniBatch):
    """Mini-batch j of a LinkSuperBatch: a MiniBatch whose seeds are the endpoints of `batch_size` positive edges and their
    negatives; n_id[edge_label_index] (binary) or n_id[src_index], n_id[dst_pos_index], n_id[dst_neg_index] (triplet) are
    the global endpoints.  `neg_unverified` is a device scalar: negatives kept after try_count rejected attempts."""
    __slots__ = ()
    batch_size = property(lambda self: self._sb.batch_size)
    edge_label_index = _row_of("edge_label_index")
    edge_label = _row_of("edge_label")
    src_index = _row_of("src_index")
    dst_pos_index = _row_of("dst_pos_index")
    dst_neg_index = _row_of("dst_neg_index")
    input_id = _row_of("input_id")
    neg_unverified = _row_of("neg_unverified")
    edge_label_time = _row_of("edge_label_time")


class LinkNeighborLoader(NeighborLoader):
    """PyG's link-level loader: a NeighborLoader whose work items are edges.  A mini-batch is `batch_size` positive edges of
    `edge_label_index` ([2, N], default data.edge_index); tg_link_seeds draws `neg_sampling_ratio` = K negatives per positive
    ("binary": random pairs; "triplet": random destinations for the positive's source), each checked against the graph for
    up to `try_count` attempts (try_count = 1: unchecked, as PyG), and lays positives and negatives out as the seed row the
    sampler starts from -- `prefetch` mini-batches per launch, on the side stream, directly ahead of tg_ns_homo_batched.
    Mini-batch j of epoch e uses call id call_id0 + e * len(loader) + j for the negatives and the sampler alike.

    Numbering against n_id: under unique=False seed p sits at n_id[p], so the index tensors are constants shared by all
    mini-batches of one width; under unique=True they are tg_ns_homo_unique's `inverse` of the seed positions, copied out of
    the slab before the sampler gets it back.  `edge_label` (user labels [N]) is carried through only when K = 0.
    `edge_set=True` builds the CSC's edge set once (one probe per check instead of a binary search) when the ids fit.

    Temporal (PyG's time_attr / edge_label_time): `edge_label_time` holds one int64 per label edge and is sliced and
    shuffled with the edges; `time_attr`, `temporal_strategy` and `time_window` are NeighborLoader's.  Both endpoints of
    pair j sample under the pair's time; negative u belongs to positive u // K (in binary mode as in triplet mode) and takes
    its time.  Negatives are still checked against the WHOLE graph, not against time: a pair that becomes an edge only
    after its time is not drawn as a negative.  Mini-batches gain `edge_label_time` [P] (the pairs' times; triplet: [E], the
    positives'), `input_time` [S] (per seed) and `node_time`.  unique=False hands out the temporal forest; unique=True the
    disjoint contract (implied by the times, as in PyG; `disjoint=True` asks for it without times): one subgraph per pair -- binary: seed s belongs to
    subgraph s mod P; triplet: src i, dst_pos i and dst_neg u to subgraphs i, i and u // K -- so src_j and dst_j share a
    subgraph, `batch` names every node's, and edge_label_index and friends come from `inverse` as before."""
    WITH_INVERSE = True
    TIME_ARG = ("edge_label_time", "label edge")

    def __init__(self, data, num_neighbors: List[int], edge_label_index: Optional[Tensor] = None,
                 edge_label: Optional[Tensor] = None, neg_sampling_ratio: int = 1, neg_sampling: str = "binary",
                 try_count: int = 8, batch_size: int = 1024, prefetch: int = 16, replace: bool = False, shuffle: bool = False,
                 drop_last: bool = False, seed: int = 0, call_id0: int = 0, device="cuda", form: int = 0,
                 unique: bool = False, edge_set: bool = False, time_attr: Optional[str] = None,
                 edge_label_time: Optional[Tensor] = None, temporal_strategy: str = "uniform", time_window=None,
                 disjoint: bool = False, labor: bool = False, layer_dependency: bool = False):
        _check_labor(labor, layer_dependency, replace, temporal_strategy,
                     bool(disjoint) or (time_attr is not None and bool(unique)), num_neighbors)
        if (time_attr is None) != (edge_label_time is None):
            raise ValueError("time_attr and edge_label_time come together: edge times need a time per label edge and the reverse")
        if neg_sampling not in ("binary", "triplet"):
            raise ValueError("neg_sampling must be 'binary' or 'triplet'")
        K = int(neg_sampling_ratio)
        if K != neg_sampling_ratio or K < 0:
            raise ValueError("neg_sampling_ratio must be an integer >= 0")
        if K > 0 and edge_label is not None:
            raise ValueError("edge_label with neg_sampling_ratio > 0: shifting user labels past the negatives' 0 is not offered")
        if int(try_count) < 1 or int(batch_size) < 1:
            raise ValueError("try_count and batch_size must be >= 1")
        dev = torch.device(device)
        eli = data.edge_index if edge_label_index is None else edge_label_index
        if eli.dim() != 2 or eli.shape[0] != 2:
            raise ValueError("edge_label_index must be [2, N]")
        if edge_label_time is not None and (not isinstance(edge_label_time, Tensor) or edge_label_time.dtype != torch.int64
                                            or edge_label_time.numel() != eli.shape[1]):
            raise ValueError("edge_label_time must be an int64 tensor with one entry per label edge (%d)" % eli.shape[1])
        if disjoint and not unique:
            raise ValueError("disjoint=True needs unique=True: without deduplication every seed's tree is apart already")
        eli = eli.to(dev).to(torch.int64).contiguous()
        n_nodes = _num_nodes(data)
        if eli.numel() and (int(eli.min()) < 0 or int(eli.max()) >= n_nodes):   # once, as _checked_inputs: no launch yet
            raise IndexError("edge_label_index outside [0, %d)" % n_nodes)
        if edge_label is not None and edge_label.shape[0] != eli.shape[1]:
            raise ValueError("edge_label must have one entry per edge of edge_label_index")
        # the base class sees the work items only as a count (for the times' length); the real ones are set below
        super().__init__(data, num_neighbors, input_nodes=eli.new_zeros(eli.shape[1] if time_attr is not None else 0),
                         batch_size=batch_size, prefetch=prefetch, replace=replace, shuffle=shuffle, drop_last=drop_last,
                         seed=seed, call_id0=call_id0, device=dev, form=form, unique=unique, time_attr=time_attr,
                         input_time=edge_label_time, temporal_strategy=temporal_strategy, time_window=time_window,
                         disjoint=bool(disjoint) or (time_attr is not None and bool(unique)),   # as PyG: times force disjoint
                         labor=labor, layer_dependency=layer_dependency)
        self.edge_label_index = eli
        self.edge_label = None if edge_label is None else edge_label.to(dev)
        self.input_nodes = torch.arange(eli.shape[1], device=dev)    # the work items: positions in edge_label_index
        self.K, self.try_count = K, int(try_count)
        self.neg_sampling = neg_sampling
        self.mode = _cabi.LINK_BINARY if neg_sampling == "binary" else _cabi.LINK_TRIPLET
        self._edge_set = _cabi.edge_set(self._graph, dev) if edge_set and self.n_nodes < 2 ** 32 - 1 else None
        self._consts = {}

    def _seed_width(self, width: int) -> int:
        return _cabi.link_seeds_capacity(width, self.K, self.mode)[0]

    def _seed_rows(self, slab, items: Tensor, first_batch: int) -> Tensor:
        G, E = items.shape
        S, cap = self._seed_width(E), slab["out"].n_batches
        rows = slab.get("link")
        if rows is None or rows.shape != (cap, S):
            rows = slab["link"] = torch.empty((cap, S), dtype=torch.int64, device=self.device)
            slab["unv"] = torch.zeros(cap, dtype=torch.int64, device=self.device)
        slab["items"] = items
        _cabi.link_seeds(self._graph, self.edge_label_index[0][items], self.edge_label_index[1][items], self.K, self.mode,
                         self.try_count, self.seed, self.call_id0 + first_batch, self.n_nodes, edge_set=self._edge_set,
                         out=rows[:G], unverified=slab["unv"][:G])
        return rows[:G]

    def _constants(self, E: int):
        """What all mini-batches of E positives share: the forest's index tensors (seed p sits at n_id[p]) and the labels."""
        c = self._consts.get(E)
        if c is None:
            S, P = _cabi.link_seeds_capacity(E, self.K, self.mode)
            local = torch.arange(S, device=self.device)
            label = torch.cat([torch.ones(E, device=self.device), torch.zeros(P - E, device=self.device)])
            c = self._consts[E] = (local, label)
        return c

    def _group_constants(self, E: int):
        """What all mini-batches of E positives share under times or disjoint subgraphs: (seed_group int32 [S], n_groups,
        of_positive int64 [S]) -- the subgraph of every seed of the row and the positive whose time it samples under.  Pair
        j < E is positive j, negative u = j - E belongs to positive u // K; binary: the row is [src of P pairs | dst of P
        pairs], a subgraph per pair; triplet: [src | dst_pos | dst_neg], a subgraph per positive."""
        c = self._consts.get(("groups", E))
        if c is None:
            K = self.K
            of_pair = torch.cat([torch.arange(E, device=self.device),
                                 torch.div(torch.arange(E * K, device=self.device), max(K, 1), rounding_mode="floor")])
            if self.mode == _cabi.LINK_BINARY:
                P = E + E * K
                group, of_positive, n_groups = torch.arange(P, device=self.device).repeat(2), of_pair.repeat(2), P
            else:
                group = of_positive = torch.cat([torch.arange(E, device=self.device), of_pair])
                n_groups = E
            c = self._consts[("groups", E)] = (group.to(torch.int32).contiguous(), n_groups, of_positive.contiguous())
        return c

    def _seed_groups(self, seeds: int):
        per = 2 * (1 + self.K) if self.mode == _cabi.LINK_BINARY else 2 + self.K    # seeds per positive: _seed_width's inverse
        group, n_groups, _ = self._group_constants(seeds // per)
        return group, n_groups

    def _seed_times(self, slab, times: Tensor) -> Tensor:
        G, E = times.shape
        _, _, of_positive = self._group_constants(E)
        S, cap = of_positive.numel(), slab["out"].n_batches
        rows = slab.get("seed_times")
        if rows is None or rows.shape != (cap, S):
            rows = slab["seed_times"] = torch.empty((cap, S), dtype=torch.int64, device=self.device)
        slab["label_times"] = times
        torch.index_select(times, 1, of_positive, out=rows[:G])     # one gather on the side stream, ahead of the sampler
        return rows[:G]

    def _times_of(self, sb, slab, G: int, times: Tensor):
        # a copy: the seed-time rows go back to the sampler with the slab set
        return slab["seed_times"][:G].clone(), sb.edge_label_time

    def _new_super_batch(self, slab, G: int) -> LinkSuperBatch:
        sb = LinkSuperBatch()
        items = slab["items"]
        E, K = items.shape[1], self.K
        S, P = _cabi.link_seeds_capacity(E, K, self.mode)
        const, label = self._constants(E)
        if self.unique:                      # a copy (clone: a full slice is contiguous already): the slab goes back
            local = slab["uniq"].inverse[:G, :S].clone(memory_format=torch.contiguous_format)
        else:
            local = const.expand(G, S)
        sb.neg_sampling, sb.input_id = self.neg_sampling, items
        sb.neg_unverified = slab["unv"][:G].clone()
        sb.edge_label_index = sb.edge_label = sb.src_index = sb.dst_pos_index = sb.dst_neg_index = sb.edge_label_time = None
        if self.temporal:                    # the pairs' times (triplet: the positives'): the subgraphs' either way
            times = slab["label_times"]
            if self.mode == _cabi.LINK_BINARY:
                times = times.index_select(1, self._group_constants(E)[2][:P])
            sb.edge_label_time = times
        if self.mode == _cabi.LINK_BINARY:
            sb.edge_label_index = local.view(G, 2, P)
            sb.edge_label = label.expand(G, P)
        else:
            sb.src_index, sb.dst_pos_index = local[:, :E], local[:, E:2 * E]
            sb.dst_neg_index = local[:, 2 * E:].reshape(G, E, K)
        if self.edge_label is not None:      # K = 0: the user's labels of these positives
            sb.edge_label = self.edge_label[items]
        return sb

    def _finish(self, ticket) -> LinkSuperBatch:
        sb = super()._finish(ticket)
        sb.batch_size = sb.input_id.shape[1]                         # positive edges, not seeds
        return sb


class HeteroLinkNeighborLoader(HeteroNeighborLoader):
    """LinkNeighborLoader for ONE relation et = (A, rel, B) of a typed graph: a HeteroNeighborLoader whose work items are
    positions in the relation's `edge_label_index` -- PyG's form (edge_type, Tensor[2, N]), or a bare edge_type or
    (edge_type, None) for the relation's own edge_index.  A mini-batch is `batch_size` positive edges;
    tg_link_seeds_typed draws `neg_sampling_ratio` = K negatives per positive ("binary": a random A and a random B;
    "triplet": random B for the positive's source), each checked against the relation for up to `try_count` attempts
    (try_count = 1: unchecked), and writes them straight into the launch's per-type input tensors -- inputs[A] [G, Ws] and
    inputs[B] [G, Wd], or ONE [G, S] tensor when A == B -- directly ahead of tg_ns_hetero_batched on the same stream.
    Equal ids of A and B are unrelated nodes unless A == B: only then is s == d rejected.  Mini-batch j of epoch e uses
    call id call_id0 + e * len(loader) + j for the negatives and the sampler alike.

    A mini-batch is HeteroNeighborLoader's HeteroGraph plus: binary `g[et].edge_label_index` [2, P] (row 0 indexes
    g[A].n_id, row 1 g[B].n_id) and `g[et].edge_label` [P]; triplet `g[A].src_index` [E], `g[B].dst_pos_index` [E],
    `g[B].dst_neg_index` [E, K]; `g[et].input_id` [E], `g.neg_unverified` (a device scalar) and `batch_size` of A and of B:
    the seeds of that type leading its n_id (the row width under the forest, the unique-seed count under unique=True).
    Under unique=False a type's n_id starts with its inputs, so the positions are constants per width; under unique=True
    they are tg_ns_typed_unique's `inverse` at those positions, copied out of the slab.  `edge_label` (user labels [N]) is
    carried through only when K = 0; `edge_set=True` builds the relation's edge set once when both id ranges fit;
    `shuffle=True` permutes the work items per epoch with a generator seeded by (seed, epoch), as NeighborLoader does."""
    WITH_INVERSE = True

    def __init__(self, data, num_neighbors: List[int], edge_label_index, edge_label: Optional[Tensor] = None,
                 neg_sampling_ratio: int = 1, neg_sampling: str = "binary", try_count: int = 8, batch_size: int = 1024,
                 prefetch: int = 16, replace: bool = False, shuffle: bool = False, drop_last: bool = False, seed: int = 0,
                 call_id0: int = 0, device="cuda", unique: bool = False, edge_set: bool = False):
        if not _is_hetero(data):
            raise ValueError("HeteroLinkNeighborLoader takes a typed graph; LinkNeighborLoader is the loader of a homogeneous one")
        if neg_sampling not in ("binary", "triplet"):
            raise ValueError("neg_sampling must be 'binary' or 'triplet'")
        K = int(neg_sampling_ratio)
        if K != neg_sampling_ratio or K < 0:
            raise ValueError("neg_sampling_ratio must be an integer >= 0")
        if K > 0 and edge_label is not None:
            raise ValueError("edge_label with neg_sampling_ratio > 0: shifting user labels past the negatives' 0 is not offered")
        if int(try_count) < 1 or int(batch_size) < 1:
            raise ValueError("try_count and batch_size must be >= 1")
        et, eli = edge_label_index, None
        if isinstance(et, (tuple, list)) and len(et) == 2 and isinstance(et[0], (tuple, list)):
            et, eli = et
        et = tuple(et)
        if et not in [tuple(x) for x in data.edge_types]:
            raise ValueError("edge_label_index must name one of the edge types %s" % list(data.edge_types))
        dev = torch.device(device)
        eli = data[et].edge_index if eli is None else eli
        if eli.dim() != 2 or eli.shape[0] != 2:
            raise ValueError("edge_label_index must be [2, N]")
        eli = eli.to(dev).to(torch.int64).contiguous()
        n_src, n_dst = _num_nodes(data[et[0]]), _num_nodes(data[et[2]])
        for row, n, nt in ((eli[0], n_src, et[0]), (eli[1], n_dst, et[2])):   # once: nothing was launched with them yet
            if row.numel() and (int(row.min()) < 0 or int(row.max()) >= n):
                raise IndexError("edge_label_index: ids of %s outside [0, %d)" % (nt, n))
        if edge_label is not None and edge_label.shape[0] != eli.shape[1]:
            raise ValueError("edge_label must have one entry per edge of edge_label_index")
        super().__init__(data, num_neighbors, et[0], input_nodes=eli.new_empty(0), batch_size=batch_size, prefetch=prefetch,
                         replace=replace, drop_last=drop_last, seed=seed, call_id0=call_id0, device=dev, unique=unique)
        self.edge_type, self.edge_label_index = et, eli
        self.edge_label = None if edge_label is None else edge_label.to(dev)
        self.input_nodes = torch.arange(eli.shape[1], device=dev)    # the work items: positions in edge_label_index
        self.shuffle, self.K, self.try_count, self.neg_sampling = bool(shuffle), K, int(try_count), neg_sampling
        self.mode = _cabi.LINK_BINARY if neg_sampling == "binary" else _cabi.LINK_TRIPLET
        self._ta, self._tb, self.n_src, self.n_dst = self._tix[et[0]], self._tix[et[2]], n_src, n_dst
        self.same_type = self._ta == self._tb
        ptrs, idx = self.col_ptrs[rel_key(et)], self.row_indices[rel_key(et)]
        self._rel_graph = _shadowed_view(ptrs, idx, max(n_src, n_dst) < 2 ** 31 and idx.numel() < 2 ** 31)
        fits = max(n_src, n_dst) < 2 ** 32 - 1
        self._edge_set = _cabi.edge_set(self._rel_graph, dev) if edge_set and fits else None
        self._consts = {}

    def _widths(self, E: int):
        """-> (Ws, Wd): the source and the destination row of a mini-batch of E positives."""
        P = _cabi.link_seeds_capacity(E, self.K, self.mode)[1]
        return (P if self.mode == _cabi.LINK_BINARY else E), P

    def _seed_width(self, width: int) -> int:
        Ws, Wd = self._widths(width)
        return Ws + Wd if self.same_type else Ws

    def _launch_for(self, items: Tensor, seeds_ts):
        G, E = items.shape
        Ws, Wd = self._widths(E)
        new = lambda w: torch.empty((G, w), dtype=torch.int64, device=self.device)
        inputs = [None] * len(self.node_types)
        if self.same_type:                                           # one input row per mini-batch: tg_link_seeds' layout
            inputs[self._ta] = row = new(Ws + Wd)
            src_out, dst_out = row[:, :Ws], row[:, Ws:]
        else:
            inputs[self._ta], inputs[self._tb] = src_out, dst_out = new(Ws), new(Wd)
        unv = torch.zeros(G, dtype=torch.int64, device=self.device)
        _cabi.link_seeds_typed(self._rel_graph, self.edge_label_index[0][items], self.edge_label_index[1][items], self.K,
                               self.mode, self.try_count, self.seed, self._first_call, self.n_src, self.n_dst, self.same_type,
                               edge_set=self._edge_set, src_out=src_out, dst_out=dst_out, unverified=unv)
        slabs = self._new_launch(inputs, None, G)
        slabs.link = (items, unv)
        return slabs

    def _emit(self, seeds: Tensor, seeds_ts, first_batch: int):
        self._first_call = self.call_id0 + first_batch               # for _launch_for, the first thing the skeleton calls:
        yield from super()._emit(seeds, seeds_ts, first_batch)       # set and read before this generator yields anything

    def _constants(self, E: int):
        """What all forest mini-batches of E positives share: positions (an input sits at its own place in its type's
        n_id; the destinations follow the sources when A == B) and the labels."""
        c = self._consts.get(E)
        if c is None:
            Ws, Wd = self._widths(E)
            dev = self.device
            c = self._consts[E] = (torch.arange(Ws, device=dev), torch.arange(Wd, device=dev) + (Ws if self.same_type else 0),
                                   torch.cat([torch.ones(E, device=dev), torch.zeros(Wd - E, device=dev)]))
        return c

    def _read_back(self, slabs):
        lo = slabs.layer_offsets.cpu().tolist()
        counts, seed_counts = slabs.read_state() if self.unique else (slabs.counts.cpu(), None)
        items, unv = (slabs.src if self.unique else slabs).link
        G, E = items.shape
        Ws, Wd = self._widths(E)
        ca, cb, label = self._constants(E)
        if self.unique:                      # copies: a kept NsTypedUniqueOut is written again by the next full launch
            off = Ws if self.same_type else 0
            la = slabs.inverse[self._ta][:, :Ws].clone()
            lb = slabs.inverse[self._tb][:, off:off + Wd].clone()
            seed_counts = seed_counts.tolist()
            sizes = [(seed_counts[b][self._ta], seed_counts[b][self._tb]) for b in range(G)]
        else:
            la, lb = ca.expand(G, Ws), cb.expand(G, Wd)
            sizes = [(Ws + Wd, Ws + Wd) if self.same_type else (Ws, Wd)] * G
        link = dict(items=items, unv=unv, E=E, sizes=sizes, la=la, lb=lb,
                    label=self.edge_label[items] if self.edge_label is not None else label.expand(G, Wd))
        if self.mode == _cabi.LINK_BINARY:
            link["eli"] = torch.stack([la, lb], dim=1)               # [G, 2, P], once per launch
        return counts, (lo, link)

    def _decorate(self, g, b, n_seeds, state, ts_parts):
        lo, link = state
        super()._decorate(g, b, n_seeds, (lo, None), ts_parts)
        A, B, et, E = self.edge_type[0], self.edge_type[2], self.edge_type, link["E"]
        g[A].batch_size, g[B].batch_size = link["sizes"][b]
        st = g[et]
        st.input_id = link["items"][b]
        g.neg_unverified = link["unv"][b]
        if self.mode == _cabi.LINK_BINARY:
            st.edge_label_index, st.edge_label = link["eli"][b], link["label"][b]
        else:
            g[A].src_index = link["la"][b]
            g[B].dst_pos_index, g[B].dst_neg_index = link["lb"][b, :E], link["lb"][b, E:].reshape(E, self.K)
            if self.edge_label is not None:
                st.edge_label = link["label"][b]


SAINT_FIELDS = ("node_norm", "edge_norm")   # what a GraphSAINT loader with sample_coverage > 0 adds to a mini-batch
SAINT_PRESAMPLE_CALL_ID0 = 1 << 62          # the pre-sample's call ids: a range no epoch reaches


class _PooledLoader(_Loader):
    """Loaders whose launches all write into one slab set, on the caller's stream: a live iterator owns a set and gives it
    back to `_pool` when it ends or is dropped, so a second epoch allocates nothing and two live iterators never share.
    A loader supplies `_new_slab`, `_epoch_state` (what an epoch's launches share), `_launch` (mini-batches j .. j + G - 1
    of that epoch into the slab set -> (call_id0 of the super-batch, node counts, edge counts) as the host reads them
    back) and `_emit` (-> what SuperBatch._set_flat takes ahead of `perm`); `perm`, `_node_attrs` and `_edge_attrs` are its
    own."""

    def _init_pool(self):
        self._pool = []                      # slab sets of finished iterators (each live iterator owns its own)
        self.slab_allocations = 0            # slab sets made so far: a second epoch makes none
        self.epoch = 0

    def _take_slab(self):
        if self._pool:
            return self._pool.pop()
        self.slab_allocations += 1
        return self._new_slab()

    def _finish(self, slab, G: int, call_id0: int, n_nodes, n_edges) -> SuperBatch:
        sb = SuperBatch()
        sb._set_flat(*self._emit(slab, G, n_nodes, n_edges), self.perm, self._node_attrs, self._edge_attrs)
        sb.batch_size, sb.call_id0 = self.batch_size, call_id0
        return sb

    def super_batches(self) -> Iterator[SuperBatch]:
        """The epoch as super-batches of up to `prefetch` mini-batches."""
        epoch = self.epoch                   # captured: a second iterator is the next epoch
        self.epoch += 1
        state, n = self._epoch_state(epoch), len(self)
        slab = self._take_slab()
        try:
            for j in range(0, n, self.prefetch):
                G = min(self.prefetch, n - j)
                yield self._finish(slab, G, *self._launch(slab, state, j, G))
        finally:
            self._pool.append(slab)


class _GraphSAINTLoader(_PooledLoader):
    """What GraphSAINT's three samplers share: everything but the step that makes a mini-batch's node list.  The argument
    checks, the CSC, the attributes, the slab sets, a launch's read-back, the pre-sample with its two norms.  A sampler
    supplies `_own_arguments` (its own checks; -> the positions P of a mini-batch and their
    name in the refusal), `_prepare` (its graphs, once), `_workspace_bytes`, `_fill` (the node lists of mini-batches
    call_id .. call_id + G - 1 into slab["nodes"] / slab["counts"], refusals into slab["status"]) and `_status_message`."""

    def __init__(self, data, batch_size: int, num_steps: int, sample_coverage: int = 0, prefetch: int = 16, seed: int = 0,
                 call_id0: int = 0, device="cuda", form: int = 0):
        S = int(num_steps)
        _at_least_1("batch_size", batch_size)    # everything that can be refused is refused before any device work
        self.batch_size = int(batch_size)
        positions, named = self._own_arguments()
        _at_least_1("num_steps", num_steps)
        if int(sample_coverage) < 0:
            raise ValueError("sample_coverage must not be negative, got %r" % (sample_coverage,))
        _at_least_1("prefetch", prefetch)
        if int(form) not in (0, 1, 2):
            raise ValueError("form must be 0 (auto), 1 (LDS) or 2 (flat), got %r" % (form,))
        if positions > 2 ** 30:
            raise ValueError("%s = %d positions exceed 2^30" % (named, positions))
        if not 0 <= int(call_id0) < SAINT_PRESAMPLE_CALL_ID0 // 2:
            raise ValueError("call_id0 must be in [0, 2^61), got %r" % (call_id0,))
        N, E = _num_nodes(data), int(data.edge_index.shape[1])
        if not 1 <= N <= 2 ** 31:
            raise ValueError("the graph must have between 1 and 2^31 nodes, got %d" % N)
        if int(sample_coverage) > 0:
            _refuse_reserved(data, SAINT_FIELDS, "a GraphSAINT loader's")
        self.data, self.num_steps = data, S
        self.sample_coverage, self.prefetch = int(sample_coverage), int(prefetch)
        self.seed, self.call_id0, self.form = int(seed), int(call_id0), int(form)
        self.device = torch.device(device)
        self.n_nodes, self._n_edges = N, E
        self.col_ptrs, self.row_indices, self.perm = to_csc(data, self.device)
        self._graph = self._view(self.col_ptrs, self.row_indices)
        self._prepare()
        self._node_attrs, self._edge_attrs = _split_attrs(data, N, E, self.device)
        self.positions = positions
        self._init_pool()
        self.node_norm = self.edge_norm = None
        self.presampled_launches = self.presampled_batches = 0
        if self.sample_coverage > 0:
            self._presample()

    def __len__(self) -> int:
        return self.num_steps

    def _workspace_bytes(self, cap: int) -> int:
        return _cabi.saint_ne_workspace_bytes(cap, self.positions, self.form)[0]   # the node and the edge sampler's

    def _new_slab(self):
        """what a launch of up to `prefetch` mini-batches writes (an epoch's launches may be narrower; the pre-sample's are
        always `prefetch` wide, so that is the size whatever num_steps is): the node slab, counts + the sampler's status
        word in one tensor, the induced pair's launch object (its counts, status and workspace), the flat form's workspace
        and the pinned image of everything the host reads back"""
        cap, dev = self.prefetch, self.device
        nodes = torch.empty((cap, self.positions), dtype=torch.int64, device=dev)
        state = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
        counts, status = state[:cap], state[-1:].view(torch.int32)[:1]
        need = self._workspace_bytes(cap)
        ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev) if need else None
        ind = _cabi.NsInduced(self._graph, nodes, counts, 1, cap, self.n_nodes)
        host = torch.empty(state.numel() + ind.state.numel(), dtype=torch.int64).pin_memory()
        return dict(nodes=nodes, state=state, counts=counts, status=status, ws=ws, ind=ind, host=host)

    def _epoch_state(self, epoch: int) -> int:
        return self.call_id0 + epoch * self.num_steps            # the call id of the epoch's first mini-batch

    def _launch(self, slab, first: int, j: int, G: int):
        """mini-batches call_id = first + j .. call_id + G - 1 into the slab set -> (call_id, node counts, edge counts), the
        counts as python lists after the launch's one read-back; pass 2 of the induced pair has not run yet"""
        cap, call_id = self.prefetch, first + j
        slab["state"][-1:].zero_()
        self._fill(slab, call_id, G)
        ind = slab["ind"].count(G)
        host = slab["host"]
        host[:cap + 1].copy_(slab["state"], non_blocking=True)
        host[cap + 1:].copy_(ind.state, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        who = type(self).__name__
        status = int(host[cap:cap + 1].view(torch.int32)[0])
        if status:
            raise RuntimeError("%s: %s" % (who, self._status_message(status)))
        _cabi.induced_status_check(int(host[-1:].view(torch.int32)[0]), who)
        return call_id, host[:G].tolist(), host[cap + 1:cap + 1 + G].tolist()

    def _presample(self):
        """whole launches under call ids from 1 << 62 until the node lists' sizes reach N * sample_coverage; their nodes
        and induced edges are counted on the device, the counts become the two norms"""
        dev, G = self.device, self.prefetch
        node_count = torch.zeros(self.n_nodes, dtype=torch.int64, device=dev)
        edge_count = torch.zeros(self._n_edges, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        slab = self._take_slab()
        covered, launches = 0, 0
        while covered < self.n_nodes * self.sample_coverage:
            _, n_nodes, n_edges = self._launch(slab, SAINT_PRESAMPLE_CALL_ID0, launches * G, G)
            _, offsets, _ = _cabi.ns_induced_emit(slab["ind"], n_edges)
            _cabi.saint_coverage_add(slab["nodes"], slab["counts"], node_count, edge_count, edge_ids=offsets, status=status,
                                     n_batches=G)
            covered += sum(n_nodes)
            launches += 1
        self._pool.append(slab)
        self.presampled_launches, self.presampled_batches = launches, launches * G
        self.node_norm, self.edge_norm = _cabi.saint_norm(self._graph, node_count, edge_count, launches * G)
        if int(status.item()):
            raise RuntimeError("%s: an id outside the coverage tables" % type(self).__name__)

    def _emit(self, slab, G: int, n_nodes, n_edges):
        edge_index, e_ptr, _ = _cabi.ns_induced_emit(slab["ind"], n_edges)
        n_id = _flat_rows(slab["nodes"][:G], slab["counts"][:G], sum(n_nodes))   # copies: the slabs go back to the sampler
        return n_id, edge_index, e_ptr, _ptr_list(n_nodes), _ptr_list(n_edges)

    def _finish(self, slab, G: int, call_id: int, n_nodes, n_edges) -> SuperBatch:
        sb = super()._finish(slab, G, call_id, n_nodes, n_edges)
        if self.node_norm is not None:       # like attributes: the view machinery cuts them per mini-batch
            sb.node_attrs["node_norm"] = _rows_of(self.node_norm, sb.n_id)
            sb.edge_attrs["edge_norm"] = _rows_of(self.edge_norm, sb._e_ptr)
        return sb


class GraphSAINTRandomWalkLoader(_GraphSAINTLoader):
    """GraphSAINT's random-walk sampler (PyG's GraphSAINTRandomWalkSampler) as a loader: a mini-batch is a SUBGRAPH -- the
    distinct nodes that `walk_length`-step uniform walks from `batch_size` random roots visit, and every edge of the graph
    between them.  An epoch is `num_steps` mini-batches; mini-batch j of epoch e has call id c = call_id0 + e * num_steps + j,
    its roots are tg_seed_batches(seed, c, 1, batch_size, N) and its walks draw with (seed, c).  A launch takes `prefetch`
    consecutive mini-batches (the epoch's last launch may be narrower): tg_seed_batches, tg_saint_rw_nodes (walks and the
    first-occurrence dedup in one step, `form` as there), tg_ns_induced_count, ONE read-back of the node and edge counts
    and the status words, tg_ns_induced_emit into flat arrays, tg_gather_rows per attribute -- all on the caller's stream.
    The walks follow out-edges on a CSR built once with the device ingest; symmetric=True states that the graph is
    symmetric and walks on the CSC the loader already holds.

    Mini-batches are `MiniBatch` views of a `SuperBatch` (`super_batches()` hands those out): `n_id` (first visit first, so
    the distinct roots lead), `edge_index` (row = source, col = target, numbered against n_id; ordered by target position,
    then CSC offset), `e_id`, node and edge attributes; `batch_size` is the root count.

    sample_coverage > 0: the constructor pre-samples whole launches (call ids from 1 << 62) until the node lists' sizes add
    up to N * sample_coverage, counts how often every node and edge was sampled (tg_saint_coverage_add) and turns the
    counts into GraphSAINT's two normalisation vectors (tg_saint_norm, n_samples = the mini-batches pre-sampled);
    mini-batches then carry `node_norm` [num_nodes] and `edge_norm` [num_edges] like attributes.  A `data` that has node or
    edge attributes of those names is refused."""

    def __init__(self, data, batch_size: int, walk_length: int, num_steps: int, sample_coverage: int = 0, prefetch: int = 16,
                 seed: int = 0, call_id0: int = 0, device="cuda", symmetric: bool = False, form: int = 0):
        self.walk_length, self.symmetric = int(walk_length), bool(symmetric)
        self._walk_length_given = walk_length
        super().__init__(data, batch_size, num_steps, sample_coverage, prefetch, seed, call_id0, device, form)

    def _own_arguments(self):
        if self.walk_length < 1:
            raise ValueError("walk_length must be at least 1, got %r" % (self._walk_length_given,))
        return self.batch_size * (self.walk_length + 1), "batch_size * (walk_length + 1)"

    def _prepare(self):
        # symmetric: the caller's word that in-edges are out-edges
        self._walk_graph = self._graph if self.symmetric else self._out_graph()

    def _workspace_bytes(self, cap: int) -> int:
        return _cabi.saint_rw_workspace_bytes(cap, self.batch_size, self.walk_length, self.form)[0]

    def _fill(self, slab, call_id: int, G: int):
        roots = _cabi.seed_batches(self.seed, call_id, G, self.batch_size, self.n_nodes, self.device)
        _cabi.saint_rw_nodes(self._walk_graph, roots, self.walk_length, self.seed, call_id, form=self.form, ws=slab["ws"],
                             out=(slab["nodes"], slab["counts"]), status=slab["status"])

    def _status_message(self, status: int) -> str:
        return "a root outside the graph"


class GraphSAINTNodeLoader(_GraphSAINTLoader):
    """GraphSAINT's node sampler (PyG's GraphSAINTNodeSampler) as a loader: a mini-batch is the subgraph induced by the
    distinct nodes among `batch_size` draws, each draw a node with probability out-degree / E (the source of a uniform
    edge: tg_saint_node_nodes on the CSC the loader holds; no CSR is needed).  Mini-batch j of epoch e has call id
    call_id0 + e * num_steps + j and draws with (seed, that call id); the pre-sample's call ids start at 1 << 62.
    Everything behind the node list -- launches of `prefetch` mini-batches, the induced pair, the one read-back, the
    `MiniBatch` views, sample_coverage and the two norms -- is GraphSAINTRandomWalkLoader's.  A mini-batch's `batch_size`
    is the draw count; `n_id` is in order of first draw."""

    def _own_arguments(self):
        return self.batch_size, "batch_size"

    def _prepare(self):
        if self._n_edges < 1:
            raise ValueError("the node sampler draws the sources of edges: the graph has none")

    def _fill(self, slab, call_id: int, G: int):
        _cabi.saint_node_nodes(self._graph, self.batch_size, G, self.seed, call_id, id_bound=self.n_nodes, form=self.form,
                               ws=slab["ws"], out=(slab["nodes"], slab["counts"]), status=slab["status"])

    def _status_message(self, status: int) -> str:
        return "a drawn node outside the graph"


class GraphSAINTEdgeLoader(_GraphSAINTLoader):
    """GraphSAINT's edge sampler (PyG's GraphSAINTEdgeSampler) as a loader: a mini-batch is the subgraph induced by the ends
    of `batch_size` drawn EDGES.  An edge (u -> v) is drawn with probability proportional to 1 / deg_in(v) + 1 / deg_out(u),
    the paper's minimum-variance law, as a mixture: a uniform entry of the list [non-empty columns of the CSC | non-empty
    rows of the CSR], then a uniform entry of that column or row (tg_saint_edge_nodes) -- no table over E.  The draws are
    independent, WITH replacement; PyG takes a Gumbel top-k over all E edges for every mini-batch, without replacement.
    The CSR is built once with the device ingest and the two lists once with torch (diff(ptrs) > 0, nonzero);
    symmetric=True states that the graph is symmetric and passes the CSC and its list for both sides.  Call ids, the
    pre-sample, the norms and everything behind the node list are GraphSAINTRandomWalkLoader's.  A mini-batch's
    `batch_size` is the number of edges drawn; `n_id` holds the distinct sources in order of first draw, then the targets
    not among them."""

    def __init__(self, data, batch_size: int, num_steps: int, sample_coverage: int = 0, prefetch: int = 16, seed: int = 0,
                 call_id0: int = 0, device="cuda", symmetric: bool = False, form: int = 0):
        self.symmetric = bool(symmetric)
        super().__init__(data, batch_size, num_steps, sample_coverage, prefetch, seed, call_id0, device, form)

    def _own_arguments(self):
        return 2 * self.batch_size, "2 * batch_size"

    def _prepare(self):
        if self._n_edges < 1:
            raise ValueError("the edge sampler draws edges: the graph has none")
        nonempty = lambda ptrs: torch.nonzero(torch.diff(ptrs) > 0).view(-1)
        self._out = self._graph if self.symmetric else self._out_graph()
        self.cols = nonempty(self.col_ptrs)
        self.rows = self.cols if self.symmetric else nonempty(self._out._keep[0])

    def _fill(self, slab, call_id: int, G: int):
        _cabi.saint_edge_nodes(self._graph, self.cols, self._out, self.rows, self.batch_size, G, self.seed, call_id,
                               id_bound=self.n_nodes, form=self.form, ws=slab["ws"], out=(slab["nodes"], slab["counts"]),
                               status=slab["status"])

    def _status_message(self, status: int) -> str:
        return "a drawn edge outside the graph" if status & 2 else "a listed column or row without entries"


class _Block:
    """One layer of a block mini-batch: `n_id` (the source nodes; its first `n_dst` entries are the destination nodes, the
    previous frontier in order), `edge_index` [2, E] numbered against n_id, and one tensor [E] more under the name a subclass
    declares (PAYLOAD, also its one slot): what `num_edges` counts."""
    __slots__ = ("n_id", "n_dst", "edge_index")

    def __init__(self, n_id, n_dst, edge_index, payload):
        self.n_id, self.n_dst, self.edge_index = n_id, n_dst, edge_index
        setattr(self, self.PAYLOAD, payload)

    @property
    def num_src_nodes(self):
        return self.n_id.numel()

    @property
    def num_edges(self):
        return getattr(self, self.PAYLOAD).numel()


class _BlockBatch:
    """Mini-batch j of a _BlockSuperBatch: `blocks` (of the subclass's BLOCK) outermost first as in DGL ([block_{L-1}, ...,
    block_0]), `n_id` = the outermost block's source nodes, the node attributes of the data gathered by n_id, `batch_size`
    and `input_nodes` (the seeds = the first `batch_size` entries of n_id); under CALL_ID also `call_id`, layer 0's."""
    CALL_ID = False

    def __init__(self, sb, j):
        self.batch_size = sb.seed_ptr[j + 1] - sb.seed_ptr[j]
        self.input_nodes = sb.input_nodes[sb.seed_ptr[j]:sb.seed_ptr[j + 1]]
        if self.CALL_ID:
            self.call_id = sb.call_id0 + j * sb.n_layers
        self.blocks = []
        for lay in reversed(sb.layers):
            n0, n1 = lay["src_ptr"][j], lay["src_ptr"][j + 1]
            e0, e1 = lay["edge_ptr"][j], lay["edge_ptr"][j + 1]
            self.blocks.append(self.BLOCK(lay["n_id"][n0:n1], lay["dst_ptr"][j + 1] - lay["dst_ptr"][j],
                                          lay["edge_index"][:, e0:e1], lay[self.BLOCK.PAYLOAD][e0:e1]))
        self.n_id = self.blocks[0].n_id
        n0, n1 = sb.node_ptr[j], sb.node_ptr[j + 1]
        self._attrs = {k: v[n0:n1] for k, v in sb.node_attrs.items()}

    @property
    def num_nodes(self):
        return self.n_id.numel()

    def __getattr__(self, name):
        attrs = self.__dict__.get("_attrs", {})
        if name in attrs:
            return attrs[name]
        raise AttributeError(name)


class _BlockSuperBatch(_Indexable):
    """The mini-batches of ONE launch as flat batch-major device tensors with python pointer lists: `n_layers`, per layer l
    `layers[l]` = dict(n_id, src_ptr, dst_ptr, edge_index (numbered inside each mini-batch), the payload, edge_ptr); `n_id` /
    `node_ptr` of the last layer, `node_attrs` gathered once by it; `input_nodes` / `seed_ptr`.  Iterating or indexing
    yields views of the subclass's BATCH."""

    def _at(self, j):
        return self.BATCH(self, j)


class _BlockLoader(_Loader):
    """What the loaders of DGL-style blocks share.  Distinct seeds per mini-batch, checked on the host; the CSC with its
    shadows and the node attributes on the device; an epoch as launches of up to `prefetch` mini-batches, shuffled by
    (seed, epoch); a launch as `n_layers` layers over the flat concatenation of its mini-batches' frontiers -- F_{l+1} = F_l
    followed by what layer l adds -- with the node attributes gathered by F_L.  A loader supplies SUPER_BATCH, `_block`
    (layer l of a launch -> its entry of `layers`) and, where the layers pass on more than the frontier, `_launch_state`."""

    def __init__(self, data, n_layers: int, input_nodes, batch_size: int, prefetch: int, shuffle: bool, drop_last: bool,
                 seed: int, device):
        N, B = _num_nodes(data), int(batch_size)
        if not 1 <= N <= 2 ** 31:
            raise ValueError("the graph must have between 1 and 2^31 nodes, got %d" % N)
        nodes = _checked_inputs(None if input_nodes is None else input_nodes.detach().cpu(), N)
        if input_nodes is not None and nodes.numel():
            # a frontier lists a node once: two equal seeds in one mini-batch would be two slots of F_0
            batch_of = torch.zeros_like(nodes) if shuffle else torch.arange(nodes.numel()) // B
            key = torch.sort(batch_of * N + nodes).values
            if bool((key[1:] == key[:-1]).any()):
                raise ValueError("input_nodes holds a node twice " + ("(shuffle=True: anywhere)" if shuffle else
                                                                      "inside one mini-batch"))
        self.data, self.n_layers, self.batch_size = data, n_layers, B
        self.prefetch, self.seed = int(prefetch), int(seed)
        self.shuffle, self.drop_last = bool(shuffle), bool(drop_last)
        self.device = torch.device(device)
        self.n_nodes, self._n_edges = N, int(data.edge_index.shape[1])
        self.input_nodes = nodes.to(self.device)
        self.col_ptrs, self.row_indices, self.perm = to_csc(data, self.device)
        self._graph = self._view(self.col_ptrs, self.row_indices)
        self._node_attrs = _split_attrs(data, N, self._n_edges, self.device, edges=False)[0]
        self.epoch = 0

    def _launch_state(self, sb, G: int, width: int, first_batch: int):
        """What the layers of a launch pass on beside the frontier: handed to every `_block` of the launch."""

    def _launch(self, seeds: Tensor, first_batch: int):
        """seeds [G, width]: mini-batches first_batch .. first_batch + G - 1 of the run (epoch * len(self) + j)"""
        G, width = seeds.shape
        sb = self.SUPER_BATCH()
        sb.n_layers = self.n_layers
        sb.input_nodes = frontier = seeds.reshape(-1).contiguous()
        sb.seed_ptr = ptr = [g * width for g in range(G + 1)]
        state = self._launch_state(sb, G, width, first_batch)
        sb.layers = []
        for l in range(self.n_layers):
            sb.layers.append(self._block(l, frontier, ptr, first_batch, state))
            frontier, ptr = sb.layers[-1]["n_id"], sb.layers[-1]["src_ptr"]
        sb.n_id, sb.node_ptr = frontier, ptr
        sb.node_attrs = {k: _rows_of(v, frontier) for k, v in self._node_attrs}
        return sb

    def super_batches(self):
        """The epoch as launches of up to `prefetch` mini-batches."""
        for (seeds,), first_batch in self._epoch_launches(self.input_nodes):
            yield self._launch(seeds, first_batch)


class _PinSAGESlabs:
    """A launch's frontier followed by a hop's neighbours, as the single-batch slabs tg_ns_homo_unique_grouped reads: the
    counts stay on the device (n = frontier + E samples, E edges; E is the hop's offsets[m])."""

    def __init__(self, frontier: Tensor, nbr: Tensor, par: Tensor, total: Tensor):
        n, dev = frontier.numel(), frontier.device
        self.samples = torch.cat([frontier, nbr]).view(1, -1)
        self.rows = (n + torch.arange(nbr.numel(), dtype=torch.int64, device=dev)).view(1, -1)
        self.cols = par.view(1, -1)
        self.edge_index = self.rows
        self.layer_offsets = torch.zeros((1, 1, 3), dtype=torch.int64, device=dev)
        self.counts = torch.stack([total + n, total]).view(1, 2)
        self.states, self.n_seeds, self.n_hops = None, n, 1

    struct = _cabi.NsBatchedOut.struct


class PinSAGEBlock(_Block):
    """One layer of a PinSAGE mini-batch: a _Block with `edge_index` [2, E] (row = position in n_id of the neighbour, col =
    position of the destination) and `edge_weight` [E] int64, the visit counts."""
    PAYLOAD = "edge_weight"
    __slots__ = (PAYLOAD,)


class PinSAGEBatch(_BlockBatch):
    """Mini-batch j of a PinSAGESuperBatch: a _BlockBatch of PinSAGEBlocks with the `call_id` of layer 0."""
    BLOCK, CALL_ID = PinSAGEBlock, True


class PinSAGESuperBatch(_BlockSuperBatch):
    """A launch of PinSAGELoader: a _BlockSuperBatch whose layers carry `edge_weight`, with `call_id0` (layer 0 of
    mini-batch 0)."""
    BATCH = PinSAGEBatch


class PinSAGELoader(_BlockLoader):
    """PinSAGE's importance sampler (DGL's PinSAGESampler / RandomWalkNeighborSampler) as a loader: the neighbours of a
    node are the k_l nodes that `n_walks` random walks of up to `walk_length` steps from it visit most often (each walk
    ends before a step l >= 1 with probability `termination`), the visit counts are the edge weights
    (tg_pinsage_hop, csrc/pinsage.hip).  The walks follow in-edges on the CSC; walk_out_edges=True builds the CSR once and
    walks along the edges; symmetric=True states that both are the same.

    Mini-batch j of epoch e (0-based across launches) with distinct seeds F_0, for layer l = 0 .. L-1: one hop runs over
    the flat concatenation of the launch's frontiers F_l with per-slot call ids call_id0 + (e * len(loader) + j) * L + l,
    fan-out k_l and draw ids = the slot's index inside its own mini-batch's frontier -- a mini-batch's result does not
    depend on what else is in the launch.  F_{l+1} = F_l followed by the neighbours not yet in F_l, in order of first
    occurrence in the hop's output (tg_ns_homo_unique_grouped over the launch, one group per mini-batch).  Block l holds
    n_id = F_{l+1}, n_dst = |F_l|, edge_index (row = index in n_id of the neighbour, col = index of the frontier slot) and
    edge_weight.  A mini-batch (PinSAGEBatch) carries `blocks` outermost first, `n_id` = F_L, the node attributes of
    `data` gathered by n_id (tg_gather_rows), `batch_size` and `input_nodes`; super_batches() hands out whole launches.

    Host synchronisation: ONE read-back of sizes per layer and launch (the per-mini-batch node and edge counts), on the
    caller's stream.  Duplicate input nodes inside one mini-batch are refused in the constructor (with shuffle=True any
    duplicate); everything that can be refused is refused before any device work."""

    def __init__(self, data, num_neighbors: List[int], input_nodes: Optional[Tensor] = None, batch_size: int = 1024,
                 n_walks: int = 10, walk_length: int = 2, termination: float = 0.5, prefetch: int = 16, seed: int = 0,
                 call_id0: int = 0, shuffle: bool = False, drop_last: bool = False, symmetric: bool = False, device="cuda",
                 walk_out_edges: bool = False):
        fanout = [int(k) for k in num_neighbors]
        if not fanout:
            raise ValueError("num_neighbors must name at least one layer")
        if any(not 1 <= k <= 64 for k in fanout):
            raise ValueError("num_neighbors must be in 1..64 per layer, got %r" % (list(num_neighbors),))
        R, T = int(n_walks), int(walk_length)
        _at_least_1("batch_size", batch_size)
        _at_least_1("n_walks", n_walks)
        _at_least_1("walk_length", walk_length)
        if R * T > _cabi.PINSAGE_MAX_VISITS:
            raise ValueError("n_walks * walk_length = %d visits per node exceed %d" % (R * T, _cabi.PINSAGE_MAX_VISITS))
        alpha = float(termination)
        if not 0.0 <= alpha < 1.0:                       # a NaN fails both comparisons
            raise ValueError("termination must be in [0, 1), got %r" % (termination,))
        _at_least_1("prefetch", prefetch)
        if not 0 <= int(call_id0) < 2 ** 62:
            raise ValueError("call_id0 must be in [0, 2^62), got %r" % (call_id0,))
        super().__init__(data, len(fanout), input_nodes, batch_size, prefetch, shuffle, drop_last, seed, device)
        self.fanout, self.call_id0 = fanout, int(call_id0)
        self.n_walks, self.walk_length, self.termination = R, T, alpha
        self.symmetric, self.walk_out_edges = bool(symmetric), bool(walk_out_edges)
        # out-edges: the CSR, built once
        self._walk_graph = self._out_graph() if self.walk_out_edges and not self.symmetric else self._graph

    SUPER_BATCH = PinSAGESuperBatch

    def _launch_state(self, sb, G: int, width: int, first_batch: int):
        sb.call_id0 = self.call_id0 + first_batch * self.n_layers
        return {"group": torch.arange(G, device=self.device).repeat_interleave(width),   # the mini-batch of every frontier slot: ascending
                "status": torch.zeros(1, dtype=torch.int32, device=self.device)}

    def _block(self, l: int, frontier: Tensor, ptr: List[int], first_batch: int, state):
        """the hop over the launch's frontiers, the grouped dedup and the relabel -> layer l; the next layer's groups go
        into `state`"""
        L, G, group, status = self.n_layers, len(ptr) - 1, state["group"], state["status"]
        o = dict(dtype=torch.int64, device=self.device)
        arange = lambda n: torch.arange(n, **o)
        n = frontier.numel()
        start = torch.tensor(ptr, **o)
        local = arange(n) - start[group]                 # the slot's index inside its own mini-batch's frontier
        call_ids = (self.call_id0 + first_batch * L + l) + group * L
        cnt, offsets, nbr, par, vis = _cabi.pinsage_hop(self._walk_graph, frontier, self.fanout[l], self.n_walks,
                                                        self.walk_length, self.termination, self.seed, 0, call_ids=call_ids,
                                                        ids=local, status=status)
        slabs = _PinSAGESlabs(frontier, nbr, par, offsets[n])
        u = _cabi.ns_homo_unique_grouped(slabs, 1, self.n_nodes, seed_group=group.to(torch.int32), n_groups=G)
        cap = slabs.samples.shape[1]
        g_of = torch.where(arange(cap) < u.counts[0, 0], u.group[0], torch.full((), G, **o))
        sizes = torch.zeros(G + 1, **o).scatter_add_(0, g_of, torch.ones(cap, **o))
        host = torch.cat([sizes[:G], offsets[start], status.to(torch.int64)]).tolist()   # the layer's ONE read-back
        if host[-1]:
            raise RuntimeError("%s: a frontier node outside the graph" % type(self).__name__)
        nptr, eptr = _ptr_list(host[:G]), host[G:2 * G + 1]
        total, n_edges = nptr[-1], eptr[-1]
        order = torch.sort(g_of, stable=True).indices[:total]     # grouped by mini-batch, first occurrence first
        rank = torch.empty(cap, **o)
        rank[order] = arange(total)
        n_id, state["group"] = u.nodes[0][order], g_of[order]
        next_start = torch.tensor(nptr, **o)
        par_e, e_group = par[:n_edges], group[par[:n_edges]]
        row = rank[u.inverse[0, n:n + n_edges]] - next_start[e_group]
        col = par_e - start[e_group]
        return dict(n_id=n_id, src_ptr=nptr, dst_ptr=ptr, edge_index=torch.stack([row, col]),
                    edge_weight=vis[:n_edges].clone(), edge_ptr=eptr)


class FullNeighborBlock(_Block):
    """One layer of a full-neighbour mini-batch: a _Block with `edge_index` [2, m] (row = position in n_id of the source, col
    = position of the destination; EVERY in-edge of every destination, in (destination, CSC offset) order) and `e_id` [m],
    the edges' columns in data.edge_index: data.edge_index[:, e_id] == n_id[edge_index]."""
    PAYLOAD = "e_id"
    __slots__ = (PAYLOAD,)


class FullNeighborBatch(_BlockBatch):
    """Mini-batch j of a FullNeighborSuperBatch: a _BlockBatch of FullNeighborBlocks (nothing is drawn: no call id)."""
    BLOCK = FullNeighborBlock


class FullNeighborSuperBatch(_BlockSuperBatch):
    """A launch of FullNeighborLoader: a _BlockSuperBatch whose layers carry `e_id`."""
    BATCH = FullNeighborBatch


class FullNeighborLoader(_BlockLoader):
    """Every in-edge per layer: the loader of layer-wise inference (PyG's NeighborLoader(num_neighbors=[-1] * L), DGL's
    MultiLayerFullNeighborSampler(L)) over tg_ns_full_count / tg_ns_full_emit (csrc/ns_full.hip).  Nothing is sampled:
    a mini-batch is a function of the graph and its seeds.

    Mini-batch j with distinct seeds F_0, for layer l = 0 .. L-1: one pair of calls runs over the flat concatenation of the
    launch's frontiers F_l (one list per mini-batch).  F_{l+1} = F_l followed by the sources of its in-edges that are not
    in it yet, in order of first occurrence in (destination, CSC offset) order; ALL of F_{l+1} is the next layer's
    frontier.  Block l (FullNeighborBlock) holds n_id = F_{l+1}, n_dst = |F_l|, edge_index [2, m] and e_id with
    data.edge_index[:, e_id] == n_id[edge_index]; every destination has its whole in-degree.  A mini-batch
    (FullNeighborBatch) carries `blocks` outermost first, `n_id` = F_L, the node attributes of `data` gathered by n_id
    (tg_gather_rows), `batch_size` and `input_nodes`; super_batches() hands out whole launches (`prefetch` mini-batches)
    as flat tensors with pointer lists.

    Host synchronisation: ONE read-back per layer and launch (node counts, edge counts, chunk counts and the status word in
    one copy, between the two passes), on the caller's stream.  The table and chunk capacities of a layer are kept from
    launch to launch; a launch that needs more than the kept capacity repeats the layer's first pass ONCE, sized by the
    exact counts it has just read plus a quarter (a second read-back for that layer; `growths` counts them).  A mini-batch whose layer has 2^31
    edges or more, or more than 2^30 nodes, raises RuntimeError naming the mini-batch.

    Out of scope: a -1 inside NeighborLoader's num_neighbors and mixed fan-outs such as [-1, 10] (NeighborLoader is
    unchanged and keeps refusing fan-outs <= 0 and > 255), temporal filters, typed graphs.  Duplicate input nodes inside
    one mini-batch are refused in the constructor (with shuffle=True any duplicate); everything that can be refused is
    refused before any device work.  Shuffling is a function of (seed, epoch)."""

    def __init__(self, data, num_layers: int = 1, input_nodes: Optional[Tensor] = None, batch_size: int = 1024,
                 prefetch: int = 16, shuffle: bool = False, drop_last: bool = False, seed: int = 0, device="cuda"):
        L = int(num_layers)
        if not 1 <= L <= _cabi.TG_MAX_HOPS:
            raise ValueError("num_layers must be in 1..%d, got %r" % (_cabi.TG_MAX_HOPS, num_layers))
        _at_least_1("batch_size", batch_size)
        _at_least_1("prefetch", prefetch)
        if _is_hetero(data):
            raise ValueError("FullNeighborLoader takes a homogeneous graph (typed graphs are out of scope)")
        super().__init__(data, L, input_nodes, batch_size, prefetch, shuffle, drop_last, seed, device)
        self.num_layers = L
        N, E, B = self.n_nodes, self._n_edges, self.batch_size
        # the kept capacities per layer (distinct nodes, chunks per mini-batch): a guess from the mean degree that grows
        mean = (E + N - 1) // N
        self._node_cap = [min(_cabi.NS_FULL_MAX_NODES, B * (2 + 2 * mean))] * L
        self._chunk_cap = [2 * B + self._node_cap[0] // 512] * L
        self._ws = None
        self.growths = 0

    SUPER_BATCH = FullNeighborSuperBatch

    def _layer(self, l: int, frontier: Tensor, ptr: List[int], first_batch: int):
        """the pair over the launch's lists -> (host n_out, host m, the counted NsFull)"""
        dev, G = self.device, len(ptr) - 1
        node_ptr = torch.tensor(ptr, dtype=torch.int64, device=dev)
        max_nodes = max(ptr[g + 1] - ptr[g] for g in range(G))
        for attempt in (0, 1):
            node_cap, chunk_cap = max(self._node_cap[l], max_nodes), max(self._chunk_cap[l], 1)
            op = _cabi.NsFull(self._graph, self.n_nodes, max_nodes, node_cap, chunk_cap, G, dev, ws=self._ws)
            self._ws = op.ws
            op.count(frontier, node_ptr)
            host = op.state.tolist()                      # the layer's ONE read-back (a second one after a growth)
            n_out, m, chunks, status = host[:G], host[G:2 * G], host[2 * G:3 * G], host[-1] & 0xFFFFFFFF
            _cabi.ns_full_status_check(status, type(self).__name__)
            if not status & 1:
                return n_out, m, op
            for g in range(G):
                n = ptr[g + 1] - ptr[g]
                if m[g] >= 2 ** 31 or n + min(m[g], self.n_nodes) > _cabi.NS_FULL_MAX_NODES:
                    raise RuntimeError("%s: layer %d of mini-batch %d has %d edges over %d nodes: past the limits of one "
                                       "batch (2^31 edges, 2^30 nodes); use a smaller batch_size" %
                                       (type(self).__name__, l, first_batch + g, m[g], n))
            if attempt:
                raise RuntimeError("%s: layer %d still refused after growing to the sizes it reported" % (type(self).__name__, l))
            # what the launch needs, and a quarter more: the next launch's largest mini-batch is rarely the same size
            need = max(ptr[g + 1] - ptr[g] + min(m[g], self.n_nodes) for g in range(G))
            self._node_cap[l] = min(_cabi.NS_FULL_MAX_NODES, need + need // 4)
            self._chunk_cap[l] = min(_cabi.NS_FULL_MAX_CHUNKS, max(chunks) + max(chunks) // 4)
            self.growths += 1

    def _block(self, l: int, frontier: Tensor, ptr: List[int], first_batch: int, state):
        n_out, m, op = self._layer(l, frontier, ptr, first_batch)
        o = dict(dtype=torch.int64, device=self.device)
        nptr, eptr = _ptr_list(n_out), _ptr_list(m)
        node_off = torch.cumsum(op.n_nodes, 0) - op.n_nodes
        edge_off = torch.cumsum(op.n_edges, 0) - op.n_edges
        n_id = torch.empty(nptr[-1], **o)
        rc = torch.empty((2, eptr[-1]), **o)
        offs = torch.empty(eptr[-1], **o)
        op.emit(node_off, edge_off, n_id, rc[0], rc[1], offs)
        return dict(n_id=n_id, src_ptr=nptr, dst_ptr=ptr, edge_index=rc, e_id=self.perm[offs], edge_ptr=eptr)


class LADIESBlock(_Block):
    """One layer of a layer-wise mini-batch: a _Block with `edge_index` [2, m] (row = position in n_id of the source, col =
    position of the destination; the in-edges whose source the layer drew, in (destination, CSC offset) order),
    `edge_weight` [m] float32 (the rescaled adjacency entry: a destination's weighted sum is an unbiased estimate of its
    full row) and `e_id` [m], the edges' columns in data.edge_index: data.edge_index[:, e_id] == n_id[edge_index]."""
    PAYLOAD = "edge_weight"
    __slots__ = (PAYLOAD, "e_id")


class LADIESBatch(_BlockBatch):
    """Mini-batch j of a LADIESSuperBatch: a _BlockBatch of LADIESBlocks with the `call_id` of layer 0; every block also
    carries its slice of the layer's `e_id`."""
    BLOCK, CALL_ID = LADIESBlock, True

    def __init__(self, sb, j):
        super().__init__(sb, j)
        for blk, lay in zip(self.blocks, reversed(sb.layers)):
            blk.e_id = lay["e_id"][lay["edge_ptr"][j]:lay["edge_ptr"][j + 1]]


class LADIESSuperBatch(_BlockSuperBatch):
    """A launch of LADIESLoader: a _BlockSuperBatch whose layers carry `edge_weight` and `e_id`, with `call_id0` (layer 0 of
    mini-batch 0)."""
    BATCH = LADIESBatch


class LADIESLoader(_BlockLoader):
    """Layer-wise importance sampling (FastGCN's estimator with LADIES' layer-dependent law, Zou et al. 2019) over
    tg_ladies_count / tg_ladies_emit (csrc/ladies.hip): every layer draws ONE budget of num_samples[l] nodes for the whole
    mini-batch, with replacement, a node's probability proportional to the squared norm of its column in the frontier's
    rows of the normalised adjacency; the kept edges are rescaled so that the aggregation stays unbiased.  A block is
    bounded by its budget where node-wise sampling grows by fanout^L.

    Mini-batch j of the run (epoch * len(loader) + its number in the epoch) with distinct seeds F_0, for layer l = 0 .. L-1:
    one pair of calls runs over the flat concatenation of the launch's frontiers F_l (one list per mini-batch) under call id
    call_id0 + j * L + l -- a mini-batch does not depend on what else is in the launch.  F_{l+1} = F_l followed by the drawn
    nodes that are not in it, ordered by their first drawing slot.  Block l (LADIESBlock) holds n_id = F_{l+1}, n_dst =
    |F_l|, edge_index [2, m], edge_weight and e_id.  Without weight_attr the adjacency is the row-normalised one (every
    in-edge of a destination of in-degree d weighs 1/d); weight_attr names a float tensor [E] of `data` with the caller's
    entries (a normalised Laplacian's; values above 1 count as 1 in the draw's law, values <= 0 and NaN as 0), which
    row_normalize=True first divides by their destination's sum (float64, index_add_).  A mini-batch (LADIESBatch) carries
    `blocks` outermost first, `n_id` = F_L, the node attributes of `data` gathered by n_id, `batch_size`, `input_nodes`
    and `call_id`; super_batches() hands out whole launches.

    Host synchronisation: ONE read-back per layer and launch, between the two passes; the capacities grow as
    FullNeighborLoader's do (`growths` counts the repeated first passes).  Duplicate input nodes inside one mini-batch are
    refused in the constructor (with shuffle=True any duplicate); everything that can be refused is refused before any
    device work.  Shuffling is a function of (seed, epoch)."""

    def __init__(self, data, num_samples: List[int], input_nodes: Optional[Tensor] = None, batch_size: int = 1024,
                 prefetch: int = 16, shuffle: bool = True, drop_last: bool = False, seed: int = 0,
                 weight_attr: Optional[str] = None, row_normalize: bool = False, device="cuda"):
        from . import _cabi_ladies
        budgets = [int(s) for s in num_samples]
        if not budgets:
            raise ValueError("num_samples must name at least one layer")
        if any(not 1 <= s <= _cabi_ladies.LADIES_MAX_SAMPLES for s in budgets):
            raise ValueError("num_samples must be in 1..%d per layer, got %r" % (_cabi_ladies.LADIES_MAX_SAMPLES, list(num_samples)))
        _at_least_1("batch_size", batch_size)
        _at_least_1("prefetch", prefetch)
        if _is_hetero(data):
            raise ValueError("LADIESLoader takes a homogeneous graph (typed graphs are out of scope)")
        E = int(data.edge_index.shape[1])
        weights = None
        if weight_attr is not None:
            weights = getattr(data, weight_attr, None)
            if not isinstance(weights, Tensor):
                raise ValueError("weight_attr: data has no tensor %r" % (weight_attr,))
            if weights.dim() != 1 or weights.numel() != E or not weights.is_floating_point():
                raise ValueError("weight_attr: data.%s must be a floating-point tensor of shape [%d], got %s %s" %
                                 (weight_attr, E, weights.dtype, tuple(weights.shape)))
        super().__init__(data, len(budgets), input_nodes, batch_size, prefetch, shuffle, drop_last, seed, device)
        self._ops = _cabi_ladies
        self.num_samples, self.call_id0 = budgets, 0
        self.weight_attr, self.row_normalize = weight_attr, bool(row_normalize)
        self.weights = self.col_sum = None
        if weights is not None:
            w = weights.to(self.device)[self.perm].to(torch.float64)           # CSC order
            if self.row_normalize:
                col = torch.repeat_interleave(torch.arange(self.n_nodes, device=self.device), self.col_ptrs[1:] - self.col_ptrs[:-1])
                self.col_sum = torch.zeros(self.n_nodes, dtype=torch.float64, device=self.device).index_add_(0, col, w)
                w = torch.where(self.col_sum[col] > 0, w / self.col_sum[col], torch.zeros_like(w))
            self.weights = w.to(torch.float32).contiguous()
        N, B, L = self.n_nodes, self.batch_size, self.n_layers
        mean = (E + N - 1) // N
        grown = [B]
        for s in budgets:
            grown.append(grown[-1] + s)                                       # a frontier's bound per layer
        self._node_cap = [min(_cabi_ladies.LADIES_MAX_NODE_CAP, grown[l] * (2 + 2 * mean)) for l in range(L)]
        self._chunk_cap = [2 * grown[l] + self._node_cap[l] // 512 for l in range(L)]
        self._ws = None
        self.growths = 0

    SUPER_BATCH = LADIESSuperBatch

    def _launch_state(self, sb, G: int, width: int, first_batch: int):
        sb.call_id0 = self.call_id0 + first_batch * self.n_layers

    def _layer(self, l: int, frontier: Tensor, ptr: List[int], first_batch: int):
        """the count pass over the launch's lists -> (host n_out, host kept edges, the counted Ladies)"""
        ops, dev, G, L, who = self._ops, self.device, len(ptr) - 1, self.n_layers, type(self).__name__
        node_ptr = torch.tensor(ptr, dtype=torch.int64, device=dev)
        max_nodes = max(ptr[g + 1] - ptr[g] for g in range(G))
        if max_nodes > ops.LADIES_MAX_NODES:
            raise RuntimeError("%s: layer %d has a frontier of %d nodes, more than 2^22" % (who, l, max_nodes))
        for attempt in (0, 1):
            node_cap, chunk_cap = max(self._node_cap[l], max_nodes), max(self._chunk_cap[l], 1)
            op = ops.Ladies(self._graph, self.n_nodes, max_nodes, node_cap, chunk_cap, self.num_samples[l], G, dev,
                            weights=self.weights, ws=self._ws)
            self._ws = op.ws
            op.count(frontier, node_ptr, self.seed, self.call_id0 + first_batch * L + l, call_stride=L)
            host = op.state.tolist()                      # the layer's ONE read-back (a second one after a growth)
            n_out, m, chunks, status = host[:G], host[G:2 * G], host[4 * G:5 * G], host[-1] & 0xFFFFFFFF
            ops.ladies_status_check(status, who)
            if not status & 1:
                return n_out, m, op
            for g in range(G):                            # a refused list reports ALL its triples in n_edges
                n = ptr[g + 1] - ptr[g]
                if not n_out[g] and (m[g] >= 2 ** 31 or n + min(m[g], self.n_nodes) > ops.LADIES_MAX_NODE_CAP):
                    raise RuntimeError("%s: layer %d of mini-batch %d has %d edges over %d nodes: past the limits of one "
                                       "batch (2^31 edges, 2^30 nodes); use a smaller batch_size" % (who, l, first_batch + g, m[g], n))
            if attempt:
                raise RuntimeError("%s: layer %d still refused after growing to the sizes it reported" % (who, l))
            # what the refused lists need, and a quarter more: the next launch's largest mini-batch is rarely the same size
            need = max([node_cap] + [ptr[g + 1] - ptr[g] + min(m[g], self.n_nodes) for g in range(G) if not n_out[g]])
            self._node_cap[l] = min(ops.LADIES_MAX_NODE_CAP, need + need // 4)
            self._chunk_cap[l] = min(ops.LADIES_MAX_CHUNKS, max(chunks) + max(chunks) // 4)
            self.growths += 1

    def _block(self, l: int, frontier: Tensor, ptr: List[int], first_batch: int, state):
        n_out, m, op = self._layer(l, frontier, ptr, first_batch)
        o = dict(dtype=torch.int64, device=self.device)
        nptr, eptr = _ptr_list(n_out), _ptr_list(m)
        node_off = torch.cumsum(op.n_nodes, 0) - op.n_nodes
        edge_off = torch.cumsum(op.n_edges, 0) - op.n_edges
        E = eptr[-1]                                      # a launch may keep no edge at all: the buffers still exist
        n_id = torch.empty(max(nptr[-1], 1), **o)[:nptr[-1]]
        rc = torch.empty((2, max(E, 1)), **o)[:, :E]
        offs = torch.empty(max(E, 1), **o)[:E]
        weight = torch.empty(max(E, 1), dtype=torch.float32, device=self.device)[:E]
        op.emit(node_off, edge_off, n_id, None, None, rc[0], rc[1], offs, weight)
        return dict(n_id=n_id, src_ptr=nptr, dst_ptr=ptr, edge_index=rc, edge_weight=weight, e_id=self.perm[offs], edge_ptr=eptr)


def range_partition(num_nodes: int, num_parts: int) -> Tensor:
    """part [N] (CPU int64): P contiguous id ranges whose sizes differ by at most one, node v in cluster v * P // N.  A
    stand-in for a real partitioner in examples and tests; it knows nothing about the edges."""
    N, P = int(num_nodes), int(num_parts)
    if N < 0 or P < 1:
        raise ValueError("range_partition: num_nodes >= 0 and num_parts >= 1 expected, got %r, %r" % (num_nodes, num_parts))
    return (torch.arange(N, dtype=torch.int64) * P) // max(N, 1)


def random_partition(num_nodes: int, num_parts: int, seed: int = 0) -> Tensor:
    """part [N] (CPU int64): every node in a cluster drawn uniformly from [0, P) by a CPU generator seeded with `seed`."""
    N, P = int(num_nodes), int(num_parts)
    if N < 0 or P < 1:
        raise ValueError("random_partition: num_nodes >= 0 and num_parts >= 1 expected, got %r, %r" % (num_nodes, num_parts))
    g = torch.Generator()
    g.manual_seed(int(seed))
    return torch.randint(0, P, (N,), generator=g, dtype=torch.int64)


def cluster_epoch_order(num_parts: int, seed: int, epoch: int, shuffle: bool = True) -> Tensor:
    """The order ClusterLoader visits the clusters in during epoch `epoch` (CPU int64 [P]): torch.randperm from a CPU
    generator seeded with (seed * 1000003 + epoch) mod 2^63, or arange without shuffle."""
    if not shuffle:
        return torch.arange(int(num_parts), dtype=torch.int64)
    g = torch.Generator()
    g.manual_seed((int(seed) * 1000003 + int(epoch)) % (1 << 63))
    return torch.randperm(int(num_parts), generator=g)


class ClusterData:
    """A graph renumbered by a node partition (PyG's ClusterData without the partitioner): `part` [N] gives every node's
    cluster in [0, num_parts) -- from METIS (pymetis, torch-sparse), a saved file, or range_partition / random_partition.
    One-off setup on `device` with the plumbing that exists: a stable sort of `part` is `node_perm` (new id -> original id;
    `node_inv` the other way), tg_ind2ptr over the sorted cluster ids is `partptr` (cluster c = new ids [partptr[c],
    partptr[c+1])), the device ingest of the renumbered edge list gives the CSC (`col_ptrs`, `row_indices`) and `perm`
    (CSC offset -> original edge number), with int32 shadows when E < 2^31.  Attributes stay in the original numbering:
    mini-batches address them through n_id and e_id."""

    def __init__(self, data, part: Tensor, num_parts: Optional[int] = None, device="cuda"):
        N, E = _num_nodes(data), int(data.edge_index.shape[1])
        if not 1 <= N <= 2 ** 31:                # everything that needs no device is refused before any device work
            raise ValueError("the graph must have between 1 and 2^31 nodes, got %d" % N)
        if not isinstance(part, Tensor) or part.dim() != 1 or part.is_floating_point() or part.dtype == torch.bool:
            raise ValueError("part must be an integer tensor [num_nodes]")
        if part.numel() != N:
            raise ValueError("part has %d entries for %d nodes" % (part.numel(), N))
        if num_parts is not None and int(num_parts) < 1:
            raise ValueError("num_parts must be at least 1, got %r" % (num_parts,))
        lo, hi = int(part.min()), int(part.max())    # on the device only when `part` lives there
        P = hi + 1 if num_parts is None else int(num_parts)
        if lo < 0 or hi >= P:
            raise ValueError("part holds cluster ids outside [0, %d): min %d, max %d" % (P, lo, hi))
        self.data, self.num_parts, self.n_nodes, self.n_edges = data, P, N, E
        self.device = dev = torch.device(device)
        part = part.to(dev, torch.int64)
        sorted_part, self.node_perm = torch.sort(part, stable=True)
        self.node_inv = torch.empty_like(self.node_perm)
        self.node_inv[self.node_perm] = torch.arange(N, dtype=torch.int64, device=dev)
        self.partptr = _cabi.ind2ptr(sorted_part.contiguous(), P)
        ei = data.edge_index.to(dev)
        self.col_ptrs, self.row_indices, self.perm = _cabi.coo_to_csx(self.node_inv[ei[0]], self.node_inv[ei[1]], N, N, True)
        self.graph = _shadowed_view(self.col_ptrs, self.row_indices, E < 2 ** 31)
        self.node_attrs, self.edge_attrs = _split_attrs(data, N, E, dev)

    def __len__(self) -> int:
        return self.num_parts


class ClusterLoader(_PooledLoader):
    """Cluster-GCN's mini-batches (PyG's ClusterLoader, DGL's ClusterGCNSampler) over a ClusterData: a mini-batch is the
    union of `batch_size` clusters with EVERY edge of the graph between its nodes, the between-cluster ones included.  An
    epoch visits every cluster once, in cluster_epoch_order(P, seed, epoch, shuffle); mini-batch j takes
    order[j * batch_size : (j + 1) * batch_size], the last one is shorter (dropped under drop_last).  A launch takes
    `prefetch` consecutive mini-batches: tg_cluster_count, ONE read-back of the node and edge counts and the status word,
    tg_cluster_emit into exact flat arrays, tg_gather_rows per attribute -- all on the caller's stream.

    Mini-batches are `MiniBatch` views of a `SuperBatch` (`super_batches()` hands those out): `n_id` (ORIGINAL node ids,
    cluster after cluster in the list's order, inside a cluster in the stable order of the partition), `edge_index` (row =
    source, col = target, numbered against n_id; ordered by target position, then CSC offset), `e_id` (original edge
    numbers), node and edge attributes; `batch_size` is the cluster count asked for."""

    def __init__(self, cluster_data: ClusterData, batch_size: int = 1, shuffle: bool = True, drop_last: bool = False,
                 prefetch: int = 16, seed: int = 0, device=None):
        q = int(batch_size)
        if q < 1:                            # everything that can be refused is refused before any device work
            raise ValueError("batch_size must be at least 1 cluster, got %r" % (batch_size,))
        if q > _cabi.CLUSTER_MAX_PARTS_PER_BATCH:
            raise ValueError("batch_size must be at most %d clusters, got %r" % (_cabi.CLUSTER_MAX_PARTS_PER_BATCH, batch_size))
        _at_least_1("prefetch", prefetch)
        if not isinstance(cluster_data, ClusterData):
            raise ValueError("cluster_data must be a ClusterData, got %s" % type(cluster_data).__name__)
        cd = self.cluster_data = cluster_data
        if device is not None and torch.device(device).type != cd.device.type:
            raise ValueError("the ClusterData lives on %s, not on %s" % (cd.device, device))
        self.device = cd.device
        self.batch_size, self.shuffle, self.drop_last = q, bool(shuffle), bool(drop_last)
        self.prefetch, self.seed = int(prefetch), int(seed)
        self.input_nodes = torch.empty(cd.num_parts, dtype=torch.int8)   # _Loader.__len__: the inputs are the clusters
        self.perm, self._node_attrs, self._edge_attrs = cd.perm, cd.node_attrs, cd.edge_attrs
        self._init_pool()

    def _new_slab(self):
        """what a launch of up to `prefetch` mini-batches needs: the cluster lists and their lengths on the device, the
        pair's launch object (its counts, status and workspace) and the pinned images of what crosses the bus"""
        cap, q, dev, cd = self.prefetch, self.batch_size, self.device, self.cluster_data
        lists = torch.zeros(cap * q + cap, dtype=torch.int64, device=dev)   # lists and lengths: one upload
        clusters, n_clusters = lists[:cap * q].view(cap, q), lists[cap * q:]
        ind = _cabi.ClusterInduced(cd.graph, cd.partptr, clusters, n_clusters, cd.node_perm)
        return dict(lists=lists, ind=ind, host_lists=torch.zeros(cap * q + cap, dtype=torch.int64).pin_memory(),
                    host=torch.empty(ind.state.numel(), dtype=torch.int64).pin_memory())

    def _epoch_state(self, epoch: int) -> Tensor:
        return cluster_epoch_order(self.cluster_data.num_parts, self.seed, epoch, self.shuffle)

    def _launch(self, slab, order: Tensor, j0: int, G: int):
        """mini-batches j0 .. j0 + G - 1 of the epoch -> (j0, node counts, edge counts), the counts as python lists after the
        launch's one read-back; pass 2 has not run yet"""
        cap, q = self.prefetch, self.batch_size
        hl = slab["host_lists"]              # its last upload is behind the last launch's read-back
        hl.zero_()
        part = order[j0 * q:(j0 + G) * q]
        hl[:part.numel()] = part             # row g of the [cap, q] slab starts at g * q: full rows, then the ragged last
        for g in range(G):
            hl[cap * q + g] = min(q, order.numel() - (j0 + g) * q)
        slab["lists"].copy_(hl, non_blocking=True)
        ind = slab["ind"].count(G)
        host = slab["host"]
        host.copy_(ind.state, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        _cabi.cluster_status_check(int(host[-1:].view(torch.int32)[0]), type(self).__name__)
        return j0, host[:G].tolist(), host[cap:cap + G].tolist()

    def _emit(self, slab, G: int, n_nodes, n_edges):
        return slab["ind"].emit(n_nodes, n_edges)           # n_id, edge_index, e_ptr and the two pointer lists
