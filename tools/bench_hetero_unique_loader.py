"""HeteroNeighborLoader(unique=True) against HeteroNeighborLoader(unique=False) on the cfg4-style synthetic graph of
tools/bench_hetero.py (3 node types A = 2^23, B = 2^22, C = 2^22; 5 relations x 20 M rectangular R-MAT edges), seeds of
type A, fan-out [15, 10], batch 1 024, prefetch 16, in one process.  Prints one JSON line (the kept run:
profiles/bench_hetero_unique_loader.json):
  loader    per D (the width of a float32 `x` on every node type; 0 = no attributes): both loaders end to end (sampling,
            dedup where asked for, the read-back, compaction, the feature gathers) in mini-batches/s -- ROUNDS passes each,
            interleaved forest / unique, median and best -- the nodes and x bytes a mini-batch carries, and the mean
            n_unique / n_nodes per node type
  dedup     tg_ns_typed_unique alone on one launch of 16 sampled batches (HIP events, ms per launch), the form taken and
            the workspace"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tch-geometric_amd"))
from tch_geometric import _cabi  # noqa: E402
from tch_geometric.loader import HeteroNeighborLoader  # noqa: E402
from tch_geometric.transforms import HeteroGraph  # noqa: E402

dev = torch.device("cuda:0")
SHIFT = int(os.environ.get("SHIFT", "0"))              # > 0: a smaller graph (every scale lowered by SHIFT)
scales = {"A": 23 - SHIFT, "B": 22 - SHIFT, "C": 22 - SHIFT}
edge_types = [("A", "e0", "A"), ("A", "e1", "B"), ("B", "e2", "A"), ("B", "e3", "C"), ("C", "e4", "A")]
E = int(os.environ.get("EDGES", 20_000_000 >> SHIFT))
DIMS = [int(x) for x in os.environ.get("DIMS", "128,0").split(",")]
BATCHES = int(os.environ.get("BATCHES", "256"))        # mini-batches of a timed pass
ROUNDS = int(os.environ.get("ROUNDS", "3"))
B, FAN, PREFETCH = 1024, [15, 10], 16
node_types = ["A", "B", "C"]
edges = {et: torch.stack(_cabi.rmat_edges_rect(scales[et[0]], scales[et[2]], E, 0xC0F4 + r, dev))
         for r, et in enumerate(edge_types)}
seeds = _cabi.seed_batches(0xBA7C4, 0, BATCHES + PREFETCH, B, 1 << scales["A"], dev).reshape(-1)
res = {"config": "3 ntypes (2^%d, 2^%d, 2^%d), 5 etypes x %d edges, seeds of type A, fan-out %s, batch %d, prefetch %d, "
                 "%d mini-batches per pass, %d interleaved passes"
                 % (scales["A"], scales["B"], scales["C"], E, FAN, B, PREFETCH, BATCHES, ROUNDS)}


def graph(D):
    data = HeteroGraph()
    for t in node_types:
        data[t].num_nodes = 1 << scales[t]
        if D:
            data[t].x = torch.empty((1 << scales[t], D), dtype=torch.float32, device=dev)
            data[t].x.view(torch.int32)[:] = 1
    for et in edge_types:
        data[et].edge_index = edges[et]
    return data


def one_pass(loader, D):
    it = iter(loader)
    for _ in range(PREFETCH):                          # the first launch of the epoch is not steady state
        next(it)
    torch.cuda.synchronize()
    nodes, nb = {t: 0 for t in node_types}, 0
    t0 = time.perf_counter()
    for g in it:
        for t in node_types:
            nodes[t] += g[t].num_nodes
            _ = (g[t].n_id, g[t].x) if D else g[t].n_id
        nb += 1
        if nb >= BATCHES:
            break
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del it
    return dt, nb, nodes


res["loader"] = {}
for D in DIMS:
    data = graph(D)
    kw = dict(input_type="A", input_nodes=seeds, batch_size=B, prefetch=PREFETCH)
    loaders = {"forest": HeteroNeighborLoader(data, FAN, **kw), "unique": HeteroNeighborLoader(data, FAN, unique=True, **kw)}
    for ld in loaders.values():                        # un-timed: the allocator's pools, the workspace
        one_pass(ld, D)
    passes = {k: [] for k in loaders}
    for _ in range(ROUNDS):
        for k, ld in loaders.items():
            passes[k].append(one_pass(ld, D))
    entry = {}
    for k, ps in passes.items():
        rate = sorted(nb / dt for dt, nb, _ in ps)
        dt, nb, nodes = ps[-1]
        per = {t: round(nodes[t] / nb) for t in node_types}
        entry[k] = {"mini_batches_per_s_median": round(statistics.median(rate), 1), "mini_batches_per_s_best": round(rate[-1], 1),
                    "nodes_per_mini_batch": per, "x_bytes_per_mini_batch": sum(per.values()) * D * 4}
    entry["unique_over_forest_median"] = round(entry["unique"]["mini_batches_per_s_median"] /
                                               entry["forest"]["mini_batches_per_s_median"], 3)
    entry["n_unique_over_n_nodes"] = {t: round(entry["unique"]["nodes_per_mini_batch"][t] /
                                               max(entry["forest"]["nodes_per_mini_batch"][t], 1), 4) for t in node_types}
    res["loader"]["D%d" % D] = entry
    print(json.dumps({"D%d" % D: entry}), file=sys.stderr, flush=True)
    rels, bounds = loaders["unique"]._rels, loaders["unique"]._id_bounds
    del loaders, data
    torch.cuda.empty_cache()

# ---- the dedup launch alone, on one launch of the loader's shape (out of place: every repetition reads the same forest)
G = PREFETCH
hb = _cabi.NsHeteroBatched(3, rels, [seeds[:G * B].reshape(G, B).contiguous(), None, None], 2, G, dev)
hb.run(0, 0)
pitches = [x.shape[1] for x in hb.samples]
form, lds = _cabi.ns_typed_unique_form(pitches, bounds)
total, least = _cabi.ns_typed_unique_workspace_bytes(pitches, bounds, G)
ws = torch.empty(total // 8 + 1, dtype=torch.int64, device=dev) if total else None
uniq = _cabi.NsTypedUniqueOut(hb, in_place=False, with_inverse=False)
for _ in range(5):
    _cabi.ns_typed_unique(hb, G, bounds, ws=ws, form=form, result=uniq)
torch.cuda.synchronize()
ms = []
for _ in range(5):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(10):
        _cabi.ns_typed_unique(hb, G, bounds, ws=ws, form=form, result=uniq)
    ev[1].record()
    torch.cuda.synchronize()
    ms.append(ev[0].elapsed_time(ev[1]) / 10)
cf, cu = hb.counts.cpu(), uniq.counts.cpu()
res["dedup"] = {"batches_per_launch": G, "pitch_nodes": pitches, "form": form, "lds_bytes_of_the_lds_form": lds,
                "workspace_bytes": total, "workspace_bytes_one_batch": least, "ms_per_launch_median": statistics.median(ms),
                "ms_per_launch_best": min(ms), "positions_per_launch": int(cf[:, :3].sum()),
                "edges_per_launch": int(cf[:, 3:].sum()),
                "n_unique_over_n_nodes": {t: float(cu[:, i].sum()) / max(float(cf[:, i].sum()), 1.0)
                                          for i, t in enumerate(node_types)}}
print(json.dumps(res))
