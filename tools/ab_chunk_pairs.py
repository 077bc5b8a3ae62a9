"""A/B of library builds on the count / emit pairs over chunked columns (csrc/chunk_scan.h; the method and the command line:
tools/ab_loop.py).  A case is one count + one emit on RMAT-(24 - SHIFT) with 16 edges per node, at the shape of the operator
section of the pair's loader benchmark, and at a small shape where the unit rule (cs_short_quarter, cs_short_fill) decides:
  ns_induced          16 batches behind tg_ns_homo_unique, 1 024 seeds x [15, 10] (bench_induced_loader.py) | 16 seeds x [5, 3]
  ns_induced_grouped  16 batches behind tg_ns_homo_unique_grouped, 1 024 seeds x [10, 10], untimed (bench_shadow_loader.py) |
                      16 seeds x [5, 3]
  cluster             16 lists of 32 of 2^14 ranges of consecutive ids (bench_cluster_loader.py) | 16 lists of 2
  ns_full             16 frontiers of 1 024 distinct nodes, sized exactly (bench_full_neighbor_loader.py) | 16 of 16
The full pair's emit consumes the workspace, so a call is always the pair.  Prints one JSON object."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tch-geometric_amd"))
import ab_loop  # noqa: E402
from tch_geometric import _cabi  # noqa: E402

dev = torch.device("cuda:0")
scale = 24 - int(os.environ.get("SHIFT", "0"))
n, G = 1 << scale, 16
row, col = _cabi.rmat_edges(scale, n * 16, 0x5EED0000 + scale, dev)
ptrs, idx, _ = _cabi.coo_to_csx(row, col, n, n, True)
del row, col
g = _cabi.graph_view(ptrs, idx, indices32=idx.to(torch.int32), ptrs32=ptrs.to(torch.int32))
cases = {}                                                   # name -> a call that runs count, then emit, once


def pair(launch, emit_args):
    def call():
        launch.count()
        launch.emit(*emit_args)
    return call


def edge_arrays(launch):
    """a counted launch's exact outputs: edge_off, rows, cols, edge_index"""
    total = int(launch.n_edges.sum())
    rc = torch.empty((2, max(total, 1)), dtype=torch.int64, device=dev)
    return torch.cumsum(launch.n_edges, 0) - launch.n_edges, rc[0], rc[1], torch.empty(max(total, 1), dtype=torch.int64, device=dev)


for tag, B, fan in (("loader", 1024, [15, 10]), ("small", 16, [5, 3])):
    seeds = _cabi.seed_batches(0xBA7C4, 0, G, B, n, dev)
    slabs = _cabi.NsBatchedOut(G, B, fan, dev)
    _cabi.ns_homo_batched(g, seeds, fan, 0, 0, slabs)
    uniq = _cabi.ns_homo_unique(slabs, G, n, with_inverse=False)
    launch = _cabi.NsInduced(g, uniq.nodes, uniq.counts, 2, G, n, node_marks=uniq.layer_nodes).count()
    cases["ns_induced/" + tag] = pair(launch, edge_arrays(launch))
    fan = [10, 10] if tag == "loader" else fan
    slabs = _cabi.NsBatchedOut(G, B, fan, dev)
    _cabi.ns_homo_batched(g, seeds, fan, 0, 0, slabs)
    ug = _cabi.ns_homo_unique_grouped(slabs, G, n, with_inverse=False)
    launch = _cabi.NsInducedGrouped(g, ug.nodes, ug.group, ug.counts, 2, G, n, B, node_marks=ug.layer_nodes).count()
    state = launch.state.cpu()
    if int(state[-1]) & 1:                                   # a disjoint list past the default capacity: the loader's retry
        launch = launch.grown(max(launch.chunks_of(state))).count()
    cases["ns_induced_grouped/" + tag] = pair(launch, edge_arrays(launch))

parts = 1 << 14
partptr = torch.arange(parts + 1, dtype=torch.int64, device=dev) * (n // parts)
gen = torch.Generator(device=dev)
gen.manual_seed(7)
for tag, q in (("loader", 32), ("small", 2)):
    clusters = torch.randperm(parts, device=dev, generator=gen)[:G * q].view(G, q).contiguous()
    launch = _cabi.ClusterInduced(g, partptr, clusters).count()
    nodes = torch.empty(int(launch.n_nodes.sum()), dtype=torch.int64, device=dev)
    args = (torch.cumsum(launch.n_nodes, 0) - launch.n_nodes,) + edge_arrays(launch)
    cases["cluster/" + tag] = (lambda l=launch, a=args, nd=nodes: (l.count(), l.emit_into(a[0], a[1], nd, a[2], a[3], a[4])))

for tag, width in (("loader", 1024), ("small", 16)):
    lists = torch.randperm(n, device=dev, generator=gen)[:G * width].view(G, width)
    deg = ptrs[lists + 1] - ptrs[lists]
    need = int((width + torch.clamp(deg.sum(1), max=n)).max())
    op = _cabi.NsFull(g, n, width, need, max(int(((deg + 511) // 512).sum(1).max()), 1), G, dev)
    flat, node_ptr = lists.reshape(-1).contiguous(), torch.arange(G + 1, device=dev) * width
    n_nodes, n_edges, _, status = op.count(flat, node_ptr)
    assert int(status.cpu()[0]) == 0
    nodes_out = torch.empty(int(n_nodes.sum()), dtype=torch.int64, device=dev)
    trip = torch.empty((3, int(n_edges.sum())), dtype=torch.int64, device=dev)
    args = (torch.cumsum(n_nodes, 0) - n_nodes, torch.cumsum(n_edges, 0) - n_edges, nodes_out, trip[0], trip[1], trip[2])
    cases["ns_full/" + tag] = (lambda o=op, f=flat, p=node_ptr, a=args: (o.count(f, p), o.emit(*a)))

ab_loop.run(cases)
