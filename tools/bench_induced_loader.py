"""NeighborLoader(unique=True, induced=True) against NeighborLoader(unique=True) on RMAT-24, fan-out [15, 10], batch 1 024,
prefetch 16, with a [2^24, 128] float32 feature matrix, in one process.  Prints one JSON line (the kept run:
profiles/bench_induced_loader.json):
  loader    both loaders end to end in mini-batches/s -- ROUNDS passes each, interleaved, median and best -- and the
            edges a mini-batch carries: induced against forest
  passes    tg_ns_induced_count and tg_ns_induced_emit alone on one launch of 16 deduplicated batches (HIP events, ms per
            call), the scanned CSC entries (the sum of the degrees of the batches' nodes) and scanned entries/s, the
            workspace
  hub       pass 1 on one column of 1 000 003 entries (the hub and 1 000 of its sources) beside pass 1 on as many entries
            spread over columns of 16: the ratio says whether a hub column serialises"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tch-geometric_amd"))
from tch_geometric import _cabi  # noqa: E402
from tch_geometric.loader import NeighborLoader  # noqa: E402
from tch_geometric.transforms import Graph  # noqa: E402

dev = torch.device("cuda:0")
SCALE = int(os.environ.get("SCALE", "24"))
D = int(os.environ.get("DIM", "128"))
BATCHES = int(os.environ.get("BATCHES", "256"))        # mini-batches of a timed pass
ROUNDS = int(os.environ.get("ROUNDS", "3"))
B, FAN, PREFETCH = 1024, [15, 10], 16
n = 1 << SCALE
row, col = _cabi.rmat_edges(SCALE, n * 16, 0x5EED0000 + SCALE, dev)
ei = torch.stack([row, col])
del row, col
seeds = _cabi.seed_batches(0xBA7C4, 0, BATCHES + PREFETCH, B, n, dev).reshape(-1)
res = {"config": "RMAT-%d, fan-out %s, batch %d, prefetch %d, %d f32 features, %d mini-batches per pass, %d interleaved passes"
                 % (SCALE, FAN, B, PREFETCH, D, BATCHES, ROUNDS)}


def one_pass(loader):
    it = iter(loader)
    for _ in range(PREFETCH):                          # the first launch of the epoch is not steady state
        next(it)
    torch.cuda.synchronize()
    edges = nodes = nb = 0
    t0 = time.perf_counter()
    for b in it:
        edges += b.num_edges
        nodes += b.num_nodes
        nb += 1
        _ = (b.n_id, b.edge_index, b.x)
        if nb >= BATCHES:
            break
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del it
    return dt, nb, edges, nodes


def timed(fn, warm=3, reps=5, inner=5):
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
    return statistics.median(ms), min(ms)


data = Graph(edge_index=ei, num_nodes=n)
data.x = torch.empty((n, D), dtype=torch.float32, device=dev)
data.x.view(torch.int32)[:] = 1
kw = dict(input_nodes=seeds, batch_size=B, prefetch=PREFETCH, unique=True)
loaders = {"unique": NeighborLoader(data, FAN, **kw), "induced": NeighborLoader(data, FAN, induced=True, **kw)}
for ld in loaders.values():                            # un-timed: slabs, pinned buffers, workspaces, the allocator's pools
    one_pass(ld)
passes = {k: [] for k in loaders}
for _ in range(ROUNDS):
    for k, ld in loaders.items():
        passes[k].append(one_pass(ld))
entry = {}
for k, ps in passes.items():
    rate = sorted(nb / dt for dt, nb, _, _ in ps)
    dt, nb, edges, nodes = ps[-1]
    entry[k] = {"mini_batches_per_s_median": round(statistics.median(rate), 1), "mini_batches_per_s_best": round(rate[-1], 1),
                "nodes_per_mini_batch": round(nodes / nb), "edges_per_mini_batch": round(edges / nb)}
entry["induced_over_unique_median"] = round(entry["induced"]["mini_batches_per_s_median"] /
                                            entry["unique"]["mini_batches_per_s_median"], 4)
entry["induced_edges_over_forest_edges"] = round(entry["induced"]["edges_per_mini_batch"] /
                                                 entry["unique"]["edges_per_mini_batch"], 3)
res["loader"] = entry
print(json.dumps({"loader": entry}), file=sys.stderr, flush=True)
graph = loaders["induced"]._graph
ptrs = loaders["induced"].col_ptrs
del loaders, data
torch.cuda.empty_cache()

# ---- the two passes alone, on one launch of the loader's shape
G = PREFETCH
out = _cabi.NsBatchedOut(G, B, FAN, dev)
_cabi.ns_homo_batched(graph, seeds[:G * B].reshape(G, B).contiguous(), FAN, 0, 0, out)
uniq = _cabi.ns_homo_unique(out, G, n, with_inverse=False)
launch = _cabi.NsInduced(graph, uniq.nodes, uniq.counts, 2, G, n, node_marks=uniq.layer_nodes)
launch.count()
state = launch.state.cpu()
m = state[:G]
total = int(m.sum())
off = torch.cumsum(launch.n_edges, 0) - launch.n_edges
rc = torch.empty((2, total), dtype=torch.int64, device=dev)
eidx = torch.empty(total, dtype=torch.int64, device=dev)
counts = uniq.counts.cpu()
scanned = 0
for b in range(G):
    v = uniq.nodes[b, :int(counts[b, 0])]
    scanned += int((ptrs[v + 1] - ptrs[v]).sum())
p1, p1_best = timed(launch.count)
p2, p2_best = timed(lambda: launch.emit(off, rc[0], rc[1], eidx))
need, least = _cabi.ns_induced_workspace_bytes(graph, out.cap_nodes, n, G)
res["passes"] = {"batches_per_call": G, "pitch_nodes": out.cap_nodes, "status": int(state[-1]),
                 "nodes_per_call": int(counts[:, 0].sum()), "forest_edges_per_call": int(counts[:, 1].sum()),
                 "induced_edges_per_call": total, "scanned_entries_per_call": scanned,
                 "scanned_entries_per_mini_batch": scanned // G,
                 "count_ms_median": p1, "count_ms_best": p1_best, "emit_ms_median": p2, "emit_ms_best": p2_best,
                 "count_G_scanned_entries_per_s": round(scanned / p1 / 1e6, 3),
                 "emit_G_scanned_entries_per_s": round(scanned / p2 / 1e6, 3),
                 "workspace_bytes": need, "workspace_bytes_one_batch": least}
print(json.dumps({"passes": res["passes"]}), file=sys.stderr, flush=True)
del out, uniq, launch, rc, eidx, graph, ptrs, ei
torch.cuda.empty_cache()

# ---- one hub column against the same number of entries in short columns
nv, deg = 200000, 1000003
gen = torch.Generator(device=dev)
gen.manual_seed(7)
src = torch.sort(torch.randint(1, nv, (deg,), device=dev, generator=gen)).values
hub_ptrs = torch.full((nv + 1,), deg, dtype=torch.int64, device=dev)
hub_ptrs[0] = 0
hub_nodes = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.unique(src)[:1000]]).view(1, -1)
short_ptrs = torch.clamp(torch.arange(nv + 1, device=dev) * 16, max=deg)        # 62 500 columns of 16 and one of 3
short_nodes = torch.arange((deg + 15) // 16, device=dev).view(1, -1)


def pass1(p, nodes):
    g = _cabi.graph_view(p, src, indices32=src.to(torch.int32), ptrs32=p.to(torch.int32))
    cnt = torch.tensor([nodes.shape[1]], dtype=torch.int64).to(dev)
    ln = _cabi.NsInduced(g, nodes, cnt, 1, 1, nv)
    med, best = timed(ln.count, inner=10)
    return {"nodes": nodes.shape[1], "scanned_entries": deg, "induced_edges": int(ln.n_edges[0]), "status": int(ln.status[0]),
            "count_ms_median": med, "count_ms_best": best}


res["hub"] = {"one_column": pass1(hub_ptrs, hub_nodes), "columns_of_16": pass1(short_ptrs, short_nodes)}
res["hub"]["one_column_over_columns_of_16"] = round(res["hub"]["one_column"]["count_ms_median"] /
                                                    res["hub"]["columns_of_16"]["count_ms_median"], 3)
print(json.dumps(res))
