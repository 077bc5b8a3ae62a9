"""ClusterLoader on RMAT-24 (16 edges per node, directed) under range_partition into 2^14 clusters of 1 024 consecutive ids,
32 clusters per mini-batch, prefetch 16, with a [2^24, 128] float32 feature matrix, in one process.  A range partition of
an R-MAT graph is NOT a METIS partition: the edges a mini-batch keeps say nothing about what a real partitioner would
keep; the scan's work (the CSC entries of the batch's columns) is the same either way.  Prints one JSON line (the kept run:
profiles/bench_cluster_loader.json):
  pair         (and pair_wide, the same at 1 024 clusters per list) tg_cluster_count / tg_cluster_emit on one launch of 16 mini-batches against tg_ns_induced_count / _emit on
               the same expanded node lists (HIP events, ms per call; ROUNDS interleaved medians and their spread), whether
               the two wrote equal words, the entries scanned, entries/s and the share of the 8 TB/s roof at the bytes
               actually read per entry (the entry's 32-bit id, plus one 32-bit column end per column, spread over its entries)
  loader       the loader end to end in mini-batches/s, against
  composition  the hand composition it replaces: torch.cat of the clusters' ranges, NsInduced.count, the read-back,
               ns_induced_emit and the gathers, 16 mini-batches a launch -- ROUNDS passes each, interleaved."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tch-geometric_amd"))
from tch_geometric import _cabi  # noqa: E402
from tch_geometric.loader import ClusterData, ClusterLoader, cluster_epoch_order, range_partition  # noqa: E402
from tch_geometric.transforms import Graph  # noqa: E402

dev = torch.device("cuda:0")
SCALE = int(os.environ.get("SCALE", "24"))
PARTS = 1 << int(os.environ.get("PART_SCALE", "14"))
Q = int(os.environ.get("Q", "32"))
D = int(os.environ.get("DIM", "128"))
Q_WIDE = int(os.environ.get("Q_WIDE", "1024"))        # the pair alone is also timed at the widest list
BATCHES = int(os.environ.get("BATCHES", "2048"))       # mini-batches of a loader pass (whole epochs, one after the other)
SLOW_BATCHES = int(os.environ.get("SLOW_BATCHES", "256"))   # mini-batches of a composition pass
ROUNDS = int(os.environ.get("ROUNDS", "5"))
PREFETCH, SEED, ROOF = 16, 7, 8e12
n = 1 << SCALE
row, col = _cabi.rmat_edges(SCALE, n * 16, 0x5EED0000 + SCALE, dev)
data = Graph(edge_index=torch.stack([row, col]), num_nodes=n)
del row, col
data.x = torch.empty((n, D), dtype=torch.float32, device=dev)
data.x.view(torch.int32)[:] = 1
cd = ClusterData(data, range_partition(n, PARTS), PARTS, device=dev)
E = cd.n_edges
res = {"config": "RMAT-%d, %d directed edges, range_partition into %d clusters of %d consecutive ids (not a METIS partition), "
                 "%d clusters per mini-batch, prefetch %d, %d f32 features, %d mini-batches per loader pass, %d per composition pass, %d interleaved passes"
                 % (SCALE, E, PARTS, n // PARTS, Q, PREFETCH, D, BATCHES, SLOW_BATCHES, ROUNDS)}


def timed(fn, warm=2, reps=5, inner=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(inner):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]) / inner)
    return statistics.median(ms)


def summary(ms):
    return {"ms_median_of_medians": round(statistics.median(ms), 4), "ms_medians": [round(x, 4) for x in ms],
            "spread_max_over_min": round(max(ms) / min(ms), 4)}


def rates(ps):
    r = sorted(nb / dt for dt, nb in ps)
    return {"mini_batches_per_s_median": round(statistics.median(r), 1), "mini_batches_per_s_best": round(r[-1], 1),
            "spread_max_over_min": round(r[-1] / r[0], 4)}


# ---- the pair against the hash pair on one launch
partptr_host = cd.partptr.cpu()


def expanded(lists_host):
    """the node slab and counts of the hand composition: the clusters' ranges, one after the other"""
    rows = [torch.cat([torch.arange(int(partptr_host[c]), int(partptr_host[c + 1]), device=dev) for c in l.tolist()])
            for l in lists_host]
    width = max(r.numel() for r in rows)
    slab = torch.zeros((len(rows), width), dtype=torch.int64, device=dev)
    for b, r in enumerate(rows):
        slab[b, :r.numel()] = r
    return slab, torch.tensor([r.numel() for r in rows], dtype=torch.int64, device=dev)


def pair_at(q):
    """one launch of PREFETCH lists of q clusters: both pairs on the same lists, outputs compared, passes interleaved"""
    G = PREFETCH
    order = torch.cat([cluster_epoch_order(PARTS, SEED, e) for e in range(-(-G * q // PARTS))])
    lists = order[:G * q].view(G, q).contiguous()
    clusters = lists.to(dev)
    cl = _cabi.ClusterInduced(cd.graph, cd.partptr, clusters, None, None)
    cl.count()
    nodes_c, rc_c, e_c, noff, eoff = cl.emit()
    slab, counts = expanded(lists)
    ind = _cabi.NsInduced(cd.graph, slab, counts, 1, G, n)
    ind.count()
    rc_h, e_h, off_h = _cabi.ns_induced_emit(ind)
    equal = bool(torch.equal(rc_c, rc_h) and torch.equal(e_c, e_h) and off_h == eoff
                 and torch.equal(nodes_c, torch.cat([slab[b, :int(counts[b])] for b in range(G)])))
    lo, hi = cd.partptr[clusters.reshape(-1)], cd.partptr[clusters.reshape(-1) + 1]
    scanned = int((cd.col_ptrs[hi] - cd.col_ptrs[lo]).sum())
    columns = int((hi - lo).sum())
    node_off_c = torch.cumsum(cl.n_nodes, 0) - cl.n_nodes
    edge_off_c = torch.cumsum(cl.n_edges, 0) - cl.n_edges
    edge_off_h = torch.cumsum(ind.n_edges, 0) - ind.n_edges
    run = {"cluster_count": cl.count,
           "cluster_emit": lambda: cl.emit_into(node_off_c, edge_off_c, nodes_c, rc_c[0], rc_c[1], e_c),
           "cluster_emit_without_nodes": lambda: cl.emit_into(node_off_c, edge_off_c, None, rc_c[0], rc_c[1], e_c),
           "induced_count": ind.count,
           "induced_emit": lambda: ind.emit(edge_off_h, rc_h[0], rc_h[1], e_h)}
    ms = {k: [] for k in run}
    names = list(run)
    for r in range(ROUNDS):
        for k in (names if r % 2 == 0 else names[::-1]):
            ms[k].append(timed(run[k]))
    # what the new scan reads per entry: its 32-bit id; pass 2 also a 32-bit column end per column of a chunk with a hit
    bytes_per_entry = {"cluster_count": 4.0, "cluster_emit": 4 + 4 * columns / max(scanned, 1),
                       "cluster_emit_without_nodes": 4 + 4 * columns / max(scanned, 1)}
    pair = {"clusters_per_batch": q, "batches_per_call": G, "nodes_per_call": noff[-1], "induced_edges_per_call": eoff[-1],
            "scanned_entries_per_call": scanned, "columns_per_call": columns, "outputs_equal": equal,
            "workspace_bytes_cluster": _cabi.cluster_workspace_bytes(cd.graph, PARTS, q, G)[0],
            "workspace_bytes_induced": _cabi.ns_induced_workspace_bytes(cd.graph, slab.shape[1], n, G)[0]}
    for k in run:
        pair[k] = summary(ms[k])
        per_s = scanned / (pair[k]["ms_median_of_medians"] * 1e-3)
        pair[k]["scanned_entries_per_s"] = round(per_s, 0)
        if k in bytes_per_entry:
            pair[k]["bytes_read_per_entry_at_most"] = round(bytes_per_entry[k], 3)
            pair[k]["share_of_8TBps_roof"] = round(per_s * bytes_per_entry[k] / ROOF, 4)
    pair["count_induced_over_cluster"] = round(pair["induced_count"]["ms_median_of_medians"] / pair["cluster_count"]["ms_median_of_medians"], 3)
    pair["emit_induced_over_cluster"] = round(pair["induced_emit"]["ms_median_of_medians"] / pair["cluster_emit"]["ms_median_of_medians"], 3)
    print(json.dumps(pair), file=sys.stderr, flush=True)
    return pair


res["pair"] = pair_at(Q)
res["pair_wide"] = pair_at(Q_WIDE)                     # the same at the widest list: enough entries to see the scan itself


# ---- the loader against the hand composition
def loader_pass(loader):
    torch.cuda.synchronize()
    nb = 0
    t0 = time.perf_counter()
    while nb < BATCHES:
        for sb in loader.super_batches():
            _ = (sb.n_id, sb.edge_index, sb.e_id, sb.node_attrs["x"])
            nb += len(sb)
            if nb >= BATCHES:
                break
    torch.cuda.synchronize()
    return time.perf_counter() - t0, nb


comp_ws = [None]


def composition_pass(epoch):
    """what a caller composed by hand before: the ranges concatenated per mini-batch, the hash pair over them, the gathers"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    order = cluster_epoch_order(PARTS, SEED, epoch)
    nb = 0
    for j0 in range(0, SLOW_BATCHES, PREFETCH):
        slab, counts = expanded(order[j0 * Q:(j0 + PREFETCH) * Q].view(PREFETCH, Q))
        ind = _cabi.NsInduced(cd.graph, slab, counts, 1, PREFETCH, n, ws=comp_ws[0])
        comp_ws[0] = ind.ws
        ind.count()
        rc, e, off = _cabi.ns_induced_emit(ind)
        n_id = _cabi.gather_rows(cd.node_perm, _cabi.compact_rows(slab, counts, int(counts.sum())))[0]
        _ = (_cabi.gather_rows(data.x, n_id)[0], _cabi.gather_rows(cd.perm, e)[0])
        nb += PREFETCH
    torch.cuda.synchronize()
    return time.perf_counter() - t0, nb


loader = ClusterLoader(cd, batch_size=Q, shuffle=True, prefetch=PREFETCH, seed=SEED)
loader_pass(loader)                                    # un-timed: slabs, pinned buffers, workspaces, the allocator's pools
composition_pass(0)
passes = {"loader": [], "composition": []}
for r in range(ROUNDS):
    passes["loader"].append(loader_pass(loader))
    passes["composition"].append(composition_pass(r + 1))
res["loader"], res["composition"] = rates(passes["loader"]), rates(passes["composition"])
res["loader_over_composition_median"] = round(res["loader"]["mini_batches_per_s_median"] /
                                              res["composition"]["mini_batches_per_s_median"], 3)
print(json.dumps(res))
