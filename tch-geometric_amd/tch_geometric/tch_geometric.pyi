"""Type stubs of the native module (operator surface of the reference: src/python.rs:785-803).

Tensors are int64 unless noted; they may live on a HIP device (adjacency stays resident in HBM) or on
the CPU (uploaded per call).  Relation dicts are keyed "src__rel__dst" (neighbor_sampling.rs:257).

Limits the reference does not have: per-hop fan-out at most 4096 for the unweighted, unfiltered samplers and at most
1024 under a temporal filter or the weighted sampler (ValueError beyond; the C ABI's batched launch tg_ns_homo_batched
takes fan-outs up to 255 and 8 hops, TG_MAX_HOPS: the operators route larger fan-outs to the flat per-hop kernels and
deeper calls hop by hop); heterogeneous sampling at most 8 node types / 16 relations in the fused launch (more fall back
to one launch per relation and hop).  RecentEdgeSampler (additive: the reference has no such class; the k most recent
admitted edges, PyG's temporal_strategy="last", deterministic) takes fan-outs up to 64 and at most 8 hops, homogeneous
sampling only; a filter passed with it must carry the sampler's own timestamps tensor (ValueError otherwise).  A call of
up to 2048 inputs is one launch of the batched driver; a larger one runs hop by hop (tg_ns_hop_recent, one size read-back
per hop), as the other samplers do.  LaborEdgeSampler(layer_dependency=False) (additive: layer-neighbor sampling, LABOR-0;
TG_SAMPLER_LABOR / _LABOR_SHARED, csrc/ns_hop_labor.hip) takes the same two routes under the same limits (fan-outs up to
64, at most 8 hops, homogeneous only: ValueError otherwise): every vertex gets one variate per call and hop, an input keeps
the num_neighbors admitted neighbours with the smallest ones.  loader.NeighborLoader(..., labor=False,
layer_dependency=False) and LinkNeighborLoader take it per mini-batch; it works with unique, induced and time_attr
(temporal_strategy="uniform") and refuses replace=True, temporal_strategy="last", disjoint=True and fan-outs above 64.

neighbor_sampling_homogenous returns the reference's forest (a vertex reached along two paths holds two slots of
`samples`, rows[e] == n_seeds + e).  The PyG-style form -- each node once, edges numbered against that list -- is made
behind it, not inside it: transforms.unique_nodes(samples, rows, cols) -> (nodes, rows_u, cols_u, inverse) for one call
(tg_ns_homo_unique, csrc/ns_unique.hip), loader.NeighborLoader(..., unique=True) for mini-batches.  Likewise per node
type for neighbor_sampling_heterogenous: transforms.unique_nodes_hetero(samples, rows, cols, edge_types, num_nodes=None)
-> (nodes, rows_u, cols_u, inverse) dicts (tg_ns_typed_unique, csrc/ns_unique_typed.hip),
loader.HeteroNeighborLoader(..., unique=True) for mini-batches.

random_walk returns the [n, walk_length + 1] walks of one call.  Node2Vec training batches -- the walks cut into context
windows plus negative rows, many mini-batches per launch -- come from Node2VecLoader (exported by the package;
tg_rw_skipgram, csrc/rw_skipgram.hip): it yields objects with pos_rw [rows, context_size], neg_rw, batch_size, call_id.
MetaPath2VecLoader (tg_mp_skipgram, csrc/mp_skipgram.hip) yields the same objects for walks along a metapath of a typed
graph, with ids offset into one embedding table (PyG's MetaPath2Vec: start / end per type, dummy_idx, num_embeddings).

Link-level mini-batches -- positive edges, checked negatives, the neighbourhood of all their endpoints, and
edge_label_index numbered against n_id -- come from LinkNeighborLoader (exported by the package; tg_link_seeds,
csrc/link_seeds.hip), and for one relation (A, rel, B) of a typed graph from HeteroLinkNeighborLoader
(tg_link_seeds_typed): edge_label_index's two rows are numbered against the n_id of A and of B.

Node-level temporal mini-batches come from loader.NeighborLoader(..., time_attr=None, input_time=None,
temporal_strategy="uniform", time_window=None): `time_attr` names an int64 [E] tensor on `data` (edge_index order),
`input_time` one int64 per input node; an edge of time t is admitted for a seed of time T when 0 <= T - t <= hi
(time_window = (lo, hi), default (0, 2**62)) and a seed's whole subtree keeps its time.  "uniform" draws among the admitted
edges (replace honoured), "last" takes the num_neighbors most recent (RecentEdgeSampler's kernel).  Mini-batches gain
input_time [batch_size] and node_time [num_nodes] (a graph with attributes of those names is refused; from an untimed
loader the names stay the graph's own attributes).

Disjoint mini-batches (PyG's disjoint=True: one subgraph per seed, the dedup key is (subgraph, node), `batch` [num_nodes]
names every node's subgraph) come from loader.NeighborLoader(..., unique=True, disjoint=True), with or without times; a
temporal NeighborLoader with unique=True and no disjoint=True raises ValueError (plain dedup would merge seed times).  The operator is tg_ns_homo_unique_grouped (csrc/ns_unique.hip):
_cabi.ns_homo_unique_grouped(out, n_batches, id_bound, seed_group=None, n_groups=None, form=0, ws=None, in_place=False,
result=None, with_inverse=True) -> an NsUniqueOut(..., with_group=True) whose `group` slab is the batch vector, with
_cabi.ns_homo_unique_grouped_form(cap_nodes, id_bound, n_groups, lds_limit_bytes=0) -> (form, lds_bytes),
_cabi.ns_homo_unique_grouped_workspace_bytes(cap_nodes, id_bound, n_groups, n_batches) -> (bytes, bytes_min) and
_cabi.ns_homo_unique_grouped_workspace(cap_nodes, id_bound, n_groups, n_batches, device, form=0); for one call
transforms.unique_nodes(samples, rows, cols, id_bound=None, seed_group=None, n_seeds=None) -> with seed_group (an int
tensor [n_seeds]) (nodes, rows_u, cols_u, inverse, batch), without it the four-tuple as before.

Temporal link-level mini-batches come from LinkNeighborLoader(..., time_attr=None, edge_label_time=None,
temporal_strategy="uniform", time_window=None, disjoint=False): `edge_label_time` holds one int64 per label edge; both
endpoints of a pair sample under the pair's time, a negative under its positive's (negative u belongs to positive u // K);
negatives are checked against the whole graph, not against time.  Mini-batches gain edge_label_time [P] (triplet: [E]),
input_time [S], node_time and, under unique=True (one subgraph per pair; triplet: per positive), batch.  induced=True
with disjoint subgraphs raises ValueError.

Induced edges per subgraph (ShaDow-GNN's k-hop sampler, PyG's ShaDowKHopSampler) come from ShaDowKHopLoader(data, depth,
num_neighbors, input_nodes=None, replace=False, batch_size=1024, prefetch=16, ..., time_attr=None, input_time=None,
temporal_strategy="uniform", time_window=None, chunk_cap=None) (exported by the package): NeighborLoader's unique=True,
disjoint=True, induced=True in one, which NeighborLoader itself refuses.  Mini-batches carry the disjoint loader's fields,
the induced edges of every seed's own neighbourhood (both ends of an edge share `batch`; under times only edges with
lo <= T_seed - t <= hi) and root_n_id [batch_size].  The operators are tg_ns_induced_grouped_count / _emit
(csrc/ns_induced.hip): _cabi.NsInducedGrouped(graph, nodes, group, counts, counts_stride, n_batches, id_bound, n_groups,
node_marks=None, group_time=None, time_window=None, chunk_cap=None, ws=None) with count() / emit() / grown(chunk_cap) and
_cabi.ns_induced_grouped_workspace_bytes(graph, pitch_nodes, id_bound, n_groups, chunk_cap, n_batches) -> (bytes,
bytes_min); for one list transforms.induced_subgraph(nodes, col_ptrs, row_indices, id_bound=None, group=None,
group_time=None, edge_time=None, time_window=None) -> (rows, cols, edge_index)."""
from typing import Dict, List, Optional, Tuple, Union

from torch import Tensor

from .utils import LaborEdgeSampler, RecentEdgeSampler, TemporalEdgeFilter, UniformEdgeSampler, WeightedEdgeSampler

NodeType = str
RelType = str
EdgeType = Tuple[str, str, str]
LayerOffset = Tuple[int, int, int]
EdgeSampler = Union[UniformEdgeSampler, WeightedEdgeSampler, RecentEdgeSampler, LaborEdgeSampler]   # the last two are additive
HomoFilter = Tuple[TemporalEdgeFilter, Tensor]
HeteroFilter = Tuple[TemporalEdgeFilter, Dict[NodeType, Tensor]]

def seed(seed: int) -> None: ...                      # additive: the reference cannot be seeded from Python
def rng_state() -> Tuple[int, int]: ...
def set_rng_state(seed: int, call_counter: int) -> None: ...
def backend_version() -> str: ...
class PanicException(RuntimeError): ...               # raised where the reference panics (pyo3_runtime.PanicException there)
def graph_cache_info() -> Dict[str, int]: ...         # additive: CPU-resident adjacency tensors are uploaded once and
def graph_cache_clear() -> None: ...                  # kept on the device (keyed on storage identity + content version);
                                                      # also the edge sets that answer has_edge for random_walk with
                                                      # p != q (built by the first call of >= 2^20 walker steps on a graph)

def to_csc(row_col: Tensor, size: Union[int, Tuple[int, int]]) -> Tuple[Tensor, Tensor, Tensor]: ...
def to_csr(row_col: Tensor, size: Union[int, Tuple[int, int]]) -> Tuple[Tensor, Tensor, Tensor]: ...

def neighbor_sampling_homogenous(
    col_ptrs: Tensor, row_indices: Tensor, inputs: Tensor, num_neighbors: List[int],
    sampler: Optional[EdgeSampler] = None, filter: Optional[HomoFilter] = None,
) -> Tuple[Tensor, Tensor, Tensor, Tensor, List[LayerOffset]]: ...

def neighbor_sampling_heterogenous(
    node_types: List[NodeType], edge_types: List[EdgeType], col_ptrs: Dict[RelType, Tensor],
    row_indices: Dict[RelType, Tensor], inputs: Dict[NodeType, Tensor], num_neighbors: Dict[RelType, List[int]],
    num_hops: int, sampler: Optional[EdgeSampler] = None, filter: Optional[HeteroFilter] = None,
) -> Tuple[Dict[NodeType, Tensor], Dict[RelType, Tensor], Dict[RelType, Tensor], Dict[RelType, Tensor],
           Dict[RelType, List[LayerOffset]]]: ...

def hgt_sampling(
    node_types: List[NodeType], edge_types: List[EdgeType], col_ptrs: Dict[RelType, Tensor],
    row_indices: Dict[RelType, Tensor], row_timestamps: Optional[Dict[RelType, Tensor]],
    inputs: Dict[NodeType, Tensor], input_timestamps: Optional[Dict[NodeType, Tensor]],
    num_samples: Dict[NodeType, List[int]], num_hops: int, timerange: Optional[Tuple[int, int]] = None,
) -> Tuple[Dict[NodeType, Tensor], Dict[NodeType, Tensor], Dict[RelType, Tensor], Dict[RelType, Tensor],
           Dict[RelType, Tensor]]: ...

def random_walk(row_ptrs: Tensor, col_indices: Tensor, start: Tensor, walk_length: int, p: float,
                q: float) -> Tensor: ...

def tempo_random_walk(
    row_ptrs: Tensor, col_indices: Tensor, node_timestamps: Tensor, edge_timestamps: Tensor, start: Tensor,
    start_timestamps: Tensor, walk_length: int, window: Tuple[int, int],
) -> Tuple[Tensor, Tensor]: ...

def negative_sample_neighbors_homogenous(
    row_ptrs: Tensor, col_indices: Tensor, graph_size: Tuple[int, int], inputs: Tensor, num_neg: int, try_count: int,
) -> Tuple[Tensor, Tensor, Tensor, int]: ...

def negative_sample_neighbors_heterogenous(
    node_types: List[NodeType], edge_types: List[EdgeType], row_ptrs: Dict[RelType, Tensor],
    col_indices: Dict[RelType, Tensor], sizes: Dict[RelType, Tuple[int, int]], inputs: Dict[NodeType, Tensor],
    num_neg: int, try_count: int, inbound: bool,
) -> Tuple[Dict[NodeType, Tensor], Dict[RelType, Tensor], Dict[RelType, Tensor], Dict[NodeType, int]]: ...

def budget_sampling(
    node_types: List[NodeType], edge_types: List[EdgeType], col_ptrs: Dict[RelType, Tensor],
    row_indices: Dict[RelType, Tensor], row_timestamps: Optional[Dict[RelType, Tensor]],
    inputs: Dict[NodeType, Tensor], input_timestamps: Optional[Dict[NodeType, Tensor]],
    num_neighbors: Dict[NodeType, List[int]], num_hops: int, window: Optional[Tuple[int, int]], forward: bool,
    relative: bool,
) -> Tuple[Dict[NodeType, Tensor], Dict[NodeType, Tensor], Dict[RelType, Tensor], Dict[RelType, Tensor],
           Dict[RelType, Tensor]]: ...

def biased_tempo_random_walk(
    row_ptrs: Tensor, col_indices: Tensor, node_timestamps: Tensor, edge_timestamps: Tensor, start: Tensor,
    start_timestamps: Tensor, walk_length: int, bias_type: str, forward: bool, retry_count: int,
) -> Tuple[Tensor, Tensor]: ...
