"""The grouped dedup (tg_ns_homo_unique_grouped, PyG's disjoint=True) and the loaders built on it, on RMAT-24 with uniform
int64 edge times and seed times in [0, 1000): fan-outs [15, 10], batch 1024, prefetch 16, one process, interleaved passes,
medians with the spread.  Writes profiles/bench_disjoint_loader.json (OUT names another file) and prints the same JSON line:
  operator   tg_ns_homo_unique_grouped with identity groups against tg_ns_homo_unique on the same 16 sampled batches, both
             in the flat form with all tables at once, out of place, outputs and workspace allocated once (HIP events, ms)
  ratio      n_unique / n_nodes of those batches under the plain dedup and under the disjoint one
  neighbor   NeighborLoader mini-batches/s: temporal unique=True, disjoint=True against temporal unique=False, both strategies,
             untimed unique=True (plain dedup) and untimed disjoint=True
  link       LinkNeighborLoader (K = 1, binary, try_count 8) mini-batches/s: temporal with both `unique` settings against
             the untimed loader with both
Every loader pass takes every super-batch's n_id and edge_index.  SCALE / BATCHES / ROUNDS shrink it for a dry run."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tch-geometric_amd"))
from tch_geometric import _cabi  # noqa: E402
from tch_geometric.loader import LinkNeighborLoader, NeighborLoader  # noqa: E402
from tch_geometric.transforms import Graph  # noqa: E402

dev = torch.device("cuda:0")
SCALE = int(os.environ.get("SCALE", "24"))
BATCHES = int(os.environ.get("BATCHES", "128"))        # mini-batches of a timed pass
ROUNDS = int(os.environ.get("ROUNDS", "5"))
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "bench_disjoint_loader.json"))
FAN, B, PREFETCH, TMAX = [15, 10], 1024, 16, 1000
n = 1 << SCALE
row, col = _cabi.rmat_edges(SCALE, n * 16, 0x5EED0000 + SCALE, dev)
gen = torch.Generator(device=dev).manual_seed(0x7E4D1)
data = Graph(edge_index=torch.stack([row, col]), num_nodes=n,
             time=torch.randint(0, TMAX, (row.numel(),), generator=gen, device=dev))
del row, col
seeds = _cabi.seed_batches(0xBA7C4, 0, BATCHES, B, n, dev).reshape(-1)
seeds_t = torch.randint(0, TMAX, (seeds.numel(),), generator=gen, device=dev)
res = {"config": "RMAT-%d, edge times and seed times uniform in [0, %d), fan-outs %s, batch %d, prefetch %d, %d mini-batches per "
                 "pass, %d interleaved passes" % (SCALE, TMAX, FAN, B, PREFETCH, BATCHES, ROUNDS)}


def event_ms(call, reps=10):
    call()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        call()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def summary(v, digits=4, best=min):
    return {"median": round(statistics.median(v), digits), "best": round(best(v), digits),
            "spread_max_over_min": round(max(v) / min(v), 3)}


# ---- the operator alone: one full launch's slabs, sampled once ----
temporal = dict(time_attr="time", input_time=seeds_t)
nkw = dict(input_nodes=seeds, batch_size=B, prefetch=PREFETCH)
first = NeighborLoader(data, FAN, **nkw)
G = min(PREFETCH, BATCHES)
out = _cabi.NsBatchedOut(G, B, FAN, dev)
_cabi.ns_homo_batched(first._graph, seeds[:G * B].reshape(G, B), FAN, 0, 0, out)
cap = out.samples.shape[1]
plain, grouped = _cabi.NsUniqueOut(out), _cabi.NsUniqueOut(out, with_group=True)
ws_p = _cabi.ns_homo_unique_workspace(cap, n, G, dev, form=2)
ws_g = _cabi.ns_homo_unique_grouped_workspace(cap, n, B, G, dev, form=2)
calls = {"plain": lambda: _cabi.ns_homo_unique(out, G, n, form=2, ws=ws_p, result=plain),
         "grouped_identity": lambda: _cabi.ns_homo_unique_grouped(out, G, n, form=2, ws=ws_g, result=grouped)}
ms = {k: [] for k in calls}
for _ in range(ROUNDS):
    for k, call in calls.items():
        ms[k].append(event_ms(call))
op = {k: dict(summary(v), unit="ms per launch of %d batches" % G) for k, v in ms.items()}
op["grouped_over_plain"] = round(op["grouped_identity"]["median"] / op["plain"]["median"], 3)
op["key_bits"] = {"plain": 32 if n <= 1 << 31 else 64, "grouped_identity": 32 if n * B <= 1 << 31 else 64}
op["positions_per_batch"], op["workspace_bytes"] = cap, {"plain": ws_p.numel() * 8, "grouped_identity": ws_g.numel() * 8}
res["operator"] = op
n_nodes = out.counts[:G, 0].sum().item()
res["ratio"] = {"n_unique_over_n_nodes_plain": round(plain.counts[:G, 0].sum().item() / n_nodes, 4),
                "n_unique_over_n_nodes_disjoint": round(grouped.counts[:G, 0].sum().item() / n_nodes, 4)}
print(json.dumps({"operator": op, "ratio": res["ratio"]}), file=sys.stderr, flush=True)
del out, plain, grouped, ws_p, ws_g, calls


# ---- loader throughput ----
def loader_pass(loader):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nb = 0
    for sb in loader.super_batches():
        nb += len(sb)
        sb.n_id, sb.edge_index
    torch.cuda.synchronize()
    return time.perf_counter() - t0, nb


def rates(loaders):
    for ld in loaders.values():                        # un-timed: slabs, workspaces, the allocator's pools
        loader_pass(ld)
    passes = {k: [] for k in loaders}
    for _ in range(ROUNDS):
        for k, ld in loaders.items():
            passes[k].append(loader_pass(ld))
    return {k: dict(summary([nb / dt for dt, nb in ps], 1, max), unit="mini-batches/s") for k, ps in passes.items()}


nl = {"untimed_unique": NeighborLoader(data, FAN, unique=True, **nkw),
      "untimed_disjoint": NeighborLoader(data, FAN, unique=True, disjoint=True, **nkw)}
for strategy in ("uniform", "last"):
    nl["temporal_%s_forest" % strategy] = NeighborLoader(data, FAN, temporal_strategy=strategy, **temporal, **nkw)
    nl["temporal_%s_disjoint" % strategy] = NeighborLoader(data, FAN, temporal_strategy=strategy, unique=True, disjoint=True, **temporal,
                                                         **nkw)
entry = rates(nl)
for strategy in ("uniform", "last"):
    entry["%s_disjoint_over_forest" % strategy] = round(entry["temporal_%s_disjoint" % strategy]["median"]
                                                        / entry["temporal_%s_forest" % strategy]["median"], 3)
entry["untimed_disjoint_over_unique"] = round(entry["untimed_disjoint"]["median"] / entry["untimed_unique"]["median"], 3)
res["neighbor"] = entry
print(json.dumps({"neighbor": entry}), file=sys.stderr, flush=True)
del nl, first

pick = torch.randint(0, data.edge_index.shape[1], (BATCHES * B,), device=dev, generator=gen)
eli = data.edge_index[:, pick].contiguous()
elt = torch.randint(0, TMAX, (pick.numel(),), generator=gen, device=dev)
lkw = dict(edge_label_index=eli, neg_sampling_ratio=1, neg_sampling="binary", try_count=8, batch_size=B, prefetch=PREFETCH)
ll = {"untimed_forest": LinkNeighborLoader(data, FAN, **lkw),
      "untimed_unique": LinkNeighborLoader(data, FAN, unique=True, **lkw),
      "temporal_forest": LinkNeighborLoader(data, FAN, time_attr="time", edge_label_time=elt, **lkw),
      "temporal_disjoint": LinkNeighborLoader(data, FAN, unique=True, time_attr="time", edge_label_time=elt, **lkw)}
entry = rates(ll)
entry["temporal_disjoint_over_forest"] = round(entry["temporal_disjoint"]["median"] / entry["temporal_forest"]["median"], 3)
res["link"] = entry
with open(OUT, "w") as f:
    f.write(json.dumps(res, indent=1) + "\n")
print(json.dumps(res))
