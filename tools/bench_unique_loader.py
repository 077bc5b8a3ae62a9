"""NeighborLoader(unique=True) against NeighborLoader(unique=False) on RMAT-24, fan-out [15, 10], batch 1 024, prefetch 16,
with a [2^24, D] float32 feature matrix (D = 128 and 32), in one process.  Prints one JSON line (the kept run:
profiles/bench_unique_loader.json):
  loader    per D: both loaders end to end (sampling, dedup where asked for, one read-back per launch, compaction, the
            feature gather; the consumer builds the n_id / edge_index / x views) in mini-batches/s and sampled edges/s --
            ROUNDS passes each, interleaved forest / unique, median and best -- and the bytes of x a mini-batch carries
  dedup     tg_ns_homo_unique alone on one launch of 16 sampled batches (HIP events, ms per call), the form taken, the
            workspace, and the measured n_unique / n_nodes"""
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
DIMS = [int(x) for x in os.environ.get("DIMS", "128,32").split(",")]
BATCHES = int(os.environ.get("BATCHES", "16384"))      # mini-batches of a timed pass
ROUNDS = int(os.environ.get("ROUNDS", "5"))
B, FAN, PREFETCH = 1024, [15, 10], 16
n = 1 << SCALE
row, col = _cabi.rmat_edges(SCALE, n * 16, 0x5EED0000 + SCALE, dev)
ei = torch.stack([row, col])
del row, col
seeds = _cabi.seed_batches(0xBA7C4, 0, BATCHES + PREFETCH, B, n, dev).reshape(-1)
res = {"config": "RMAT-%d, fan-out %s, batch %d, prefetch %d, %d mini-batches per pass, %d interleaved passes"
                 % (SCALE, FAN, B, PREFETCH, BATCHES, ROUNDS)}


def one_pass(loader, D):
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
        _ = (b.n_id, b.edge_index, b.x) if D else (b.n_id, b.edge_index)
        if nb >= BATCHES:
            break
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del it
    return dt, nb, edges, nodes


res["loader"] = {}
for D in DIMS:
    data = Graph(edge_index=ei, num_nodes=n)
    if D:
        data.x = torch.empty((n, D), dtype=torch.float32, device=dev)
        data.x.view(torch.int32)[:] = 1
    loaders = {"forest": NeighborLoader(data, FAN, input_nodes=seeds, batch_size=B, prefetch=PREFETCH),
               "unique": NeighborLoader(data, FAN, input_nodes=seeds, batch_size=B, prefetch=PREFETCH, unique=True)}
    for ld in loaders.values():                        # un-timed: slabs, pinned buffers, workspace, the allocator's pools
        one_pass(ld, D)
    passes = {k: [] for k in loaders}
    for _ in range(ROUNDS):
        for k, ld in loaders.items():
            passes[k].append(one_pass(ld, D))
    entry = {}
    for k, ps in passes.items():
        rate = sorted(nb / dt for dt, nb, _, _ in ps)
        dt, nb, edges, nodes = ps[-1]
        entry[k] = {"mini_batches_per_s_median": round(statistics.median(rate)), "mini_batches_per_s_best": round(rate[-1]),
                    "G_sampled_edges_per_s_median": round(statistics.median(e / t for t, _, e, _ in ps) / 1e9, 3),
                    "nodes_per_mini_batch": round(nodes / nb), "edges_per_mini_batch": round(edges / nb),
                    "x_bytes_per_mini_batch": round(nodes / nb) * D * 4}
    entry["unique_over_forest_median"] = round(entry["unique"]["mini_batches_per_s_median"] /
                                               entry["forest"]["mini_batches_per_s_median"], 3)
    entry["n_unique_over_n_nodes"] = round(entry["unique"]["nodes_per_mini_batch"] / entry["forest"]["nodes_per_mini_batch"], 4)
    res["loader"]["D%d" % D] = entry
    print(json.dumps({"D%d" % D: entry}), file=sys.stderr, flush=True)
    del loaders, data
    torch.cuda.empty_cache()

# ---- the dedup call alone, on one launch of the loader's shape
G = PREFETCH
ptrs, idx, _ = _cabi.coo_to_csx(ei[0].contiguous(), ei[1].contiguous(), n, n, True)
graph = _cabi.graph_view(ptrs, idx, indices32=idx.to(torch.int32), ptrs32=ptrs.to(torch.int32))
out = _cabi.NsBatchedOut(G, B, FAN, dev)
_cabi.ns_homo_batched(graph, seeds[:G * B].reshape(G, B).contiguous(), FAN, 0, 0, out)
form, lds, bound = _cabi.ns_homo_unique_form(out.cap_nodes, n)
total, least = _cabi.ns_homo_unique_workspace_bytes(out.cap_nodes, n, G)
ws = _cabi.ns_homo_unique_workspace(out.cap_nodes, n, G, dev)
uniq = _cabi.NsUniqueOut(out, in_place=False, with_inverse=False)
for _ in range(10):
    _cabi.ns_homo_unique(out, G, n, ws=ws, result=uniq)
torch.cuda.synchronize()
ms = []
for _ in range(5):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(20):
        _cabi.ns_homo_unique(out, G, n, ws=ws, result=uniq)
    ev[1].record()
    torch.cuda.synchronize()
    ms.append(ev[0].elapsed_time(ev[1]) / 20)
cf, cu = out.counts.cpu(), uniq.counts.cpu()
res["dedup"] = {"batches_per_call": G, "cap_nodes": out.cap_nodes, "form": form, "lds_bound_cap_nodes": bound,
                "workspace_bytes": total, "workspace_bytes_one_batch": least, "ms_per_call_median": statistics.median(ms),
                "ms_per_call_best": min(ms), "positions_per_call": int(cf[:, 0].sum()), "edges_per_call": int(cf[:, 1].sum()),
                "n_unique_over_n_nodes": float(cu[:, 0].sum()) / float(cf[:, 0].sum())}
print(json.dumps(res))
