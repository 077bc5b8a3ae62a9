"""Layer-neighbor sampling (TG_SAMPLER_LABOR) and NeighborLoader(labor=True) on RMAT-24: fan-outs [15, 10] and [10, 10, 10],
batch 1024, prefetch 16, 128 f32 features, one process, interleaved passes, medians with the spread.  Prints one JSON line
(the kept run: profiles/bench_labor_loader.json):
  distinct  nodes per mini-batch under unique=True for uniform, labor and labor + layer_dependency, and n_unique / n_nodes
            against the forest's size: the number the sampler exists for
  hop       tg_ns_hop_labor over the loader's hop-1 frontier (16 x 1024 x 15 slots drawn by degree, so hubs repeat), without
            and under a backward RELATIVE filter, against tg_ns_hop_recent (the parent's kernel, the yardstick; random int64
            times) and the plain flat hop tg_ns_hop on the same frontier: ms, inspected edges/s and what that is in bytes/s at
            4 (indices32) or 12 (ids + times) bytes per edge.  Timed around the _cabi wrappers, which allocate their outputs
  long      the same labor hop with TG_LABOR_LONG_COLUMN at 2 048 / 8 192 / 32 768
  hub       one column of 1 000 003 entries against the same entries in 62 501 columns of 16, for labor and for recent
  loader    mini-batches/s with the features gathered, unique=True and unique=False, labor against uniform, and the
            feature-gather bytes per mini-batch of each
SCALE / BATCHES / ROUNDS shrink it for a dry run."""
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
BATCHES = int(os.environ.get("BATCHES", "64"))         # mini-batches of a timed pass
ROUNDS = int(os.environ.get("ROUNDS", "5"))
CHANNELS = int(os.environ.get("CHANNELS", "128"))
FANS, B, PREFETCH, TMAX, WINDOW = ([15, 10], [10, 10, 10]), 1024, 16, 1000, (0, 2 ** 62)
n = 1 << SCALE
row, col = _cabi.rmat_edges(SCALE, n * 16, 0x5EED0000 + SCALE, dev)
gen = torch.Generator(device=dev).manual_seed(0x1AB0)
data = Graph(edge_index=torch.stack([row, col]), num_nodes=n, x=torch.randn((n, CHANNELS), generator=gen, device=dev))
del row, col
seeds = _cabi.seed_batches(0xBA7C4, 0, BATCHES, B, n, dev).reshape(-1)
res = {"config": "RMAT-%d, batch %d, prefetch %d, %d f32 features, %d mini-batches per pass, %d interleaved passes"
                 % (SCALE, B, PREFETCH, CHANNELS, BATCHES, ROUNDS),
       "timing": "hop, long and hub: HIP events around the _cabi wrappers, which allocate their outputs (and the labor hop's "
                 "workspace) per call: not pure kernel times"}
KINDS = {"uniform": {}, "labor": dict(labor=True), "labor_layer_dependency": dict(labor=True, layer_dependency=True)}


def make(fan, unique, **kw):
    return NeighborLoader(data, fan, input_nodes=seeds, batch_size=B, prefetch=PREFETCH, unique=unique, **kw)


def event_ms(call, reps=5):
    call()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        call()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def interleaved(calls):
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, call in calls.items():
            ms[k].append(event_ms(call))
    return {k: {"ms_median": round(statistics.median(v), 4), "ms_best": round(min(v), 4),
                "spread_max_over_min": round(max(v) / min(v), 3)} for k, v in ms.items()}


def loader_pass(loader):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nb = nodes = 0
    for sb in loader.super_batches():
        nb += len(sb)
        nodes += int(sb.n_id.numel())
    torch.cuda.synchronize()
    return time.perf_counter() - t0, nb, nodes


# ---- distinct nodes per mini-batch, and loader throughput with the features gathered ----
res["distinct"], res["loader"] = {}, {}
for fan in FANS:
    loaders = {(k, u): make(fan, u, **kw) for k, kw in KINDS.items() for u in (True, False)}
    for ld in loaders.values():                        # un-timed: slabs, workspaces, the allocator's pools
        loader_pass(ld)
    passes = {key: [] for key in loaders}
    for _ in range(ROUNDS):
        for key, ld in loaders.items():
            passes[key].append(loader_pass(ld))
    dist, thr = {}, {}
    for (k, u), ps in passes.items():
        rate = sorted(nb / dt for dt, nb, _ in ps)
        per_mb = statistics.mean(p[2] / p[1] for p in ps)
        thr["%s_unique=%s" % (k, u)] = {"mini_batches_per_s_median": round(statistics.median(rate), 1),
                                        "mini_batches_per_s_best": round(rate[-1], 1),
                                        "spread_max_over_min": round(rate[-1] / rate[0], 3),
                                        "nodes_per_mini_batch": round(per_mb, 1),
                                        "feature_gather_MB_per_mini_batch": round(per_mb * CHANNELS * 4 / 1e6, 2)}
        if u:
            forest = statistics.mean(p[2] / p[1] for p in passes[(k, False)])
            dist[k] = {"distinct_nodes_per_mini_batch": round(per_mb, 1), "forest_nodes_per_mini_batch": round(forest, 1),
                       "n_unique_over_n_nodes": round(per_mb / forest, 4)}
    for k in ("labor", "labor_layer_dependency"):
        dist[k]["distinct_over_uniform"] = round(dist[k]["distinct_nodes_per_mini_batch"] /
                                                 dist["uniform"]["distinct_nodes_per_mini_batch"], 4)
        for u in (True, False):
            thr["%s_over_uniform_unique=%s" % (k, u)] = round(thr["%s_unique=%s" % (k, u)]["mini_batches_per_s_median"] /
                                                              thr["uniform_unique=%s" % u]["mini_batches_per_s_median"], 3)
    res["distinct"][str(fan)], res["loader"][str(fan)] = dist, thr
    print(json.dumps({"fan": fan, "distinct": dist, "loader": thr}), file=sys.stderr, flush=True)
    ref = loaders[("labor", False)]
    ptrs, idx, idx32, ptr32 = ref.col_ptrs, ref.row_indices, ref._idx32, ref._ptr32
    del loaders, passes
del data
torch.cuda.empty_cache()

# ---- one hop over the loader's hop-1 frontier ([15, 10]: hop 0's samples of a full launch) ----
FAN = FANS[0]
G = min(PREFETCH, BATCHES)
times = torch.randint(0, TMAX, (idx.numel(),), generator=gen, device=dev)
graph = _cabi.graph_view(ptrs, idx, timestamps=times, indices32=idx32, ptrs32=ptr32, max_degree="auto")
out = _cabi.NsBatchedOut(G, B, FAN[:1], dev)
_cabi.ns_homo_batched(graph, seeds[:G * B].reshape(G, B), FAN[:1], 0, 0, out)
counts = out.counts.cpu()
frontier = torch.cat([out.samples[b, B:int(counts[b, 0])] for b in range(G)]).contiguous()
fstates = torch.randint(0, TMAX, (frontier.numel(),), generator=gen, device=dev)
deg = (ptrs[1:] - ptrs[:-1])[frontier]
inspected = int(deg.sum())
K = FAN[1]
hop = interleaved({
    "labor": lambda: _cabi.ns_hop_labor(graph, frontier, K, 0, 0, layer=1),
    "labor_filtered": lambda: _cabi.ns_hop_labor(graph, frontier, K, 0, 0, layer=1, states=fstates,
                                                 filter_mode=_cabi.FILTER_RELATIVE, window=WINDOW),
    "recent": lambda: _cabi.ns_hop_recent(graph, frontier, K),
    "recent_filtered": lambda: _cabi.ns_hop_recent(graph, frontier, K, states=fstates, filter_mode=_cabi.FILTER_RELATIVE,
                                                   window=WINDOW),
    "plain_flat_hop": lambda: _cabi.ns_hop(graph, frontier, K, 0)})
for k, bytes_per_edge in (("labor", 4), ("labor_filtered", 12), ("recent", 8), ("recent_filtered", 8)):
    rate = inspected / (hop[k]["ms_median"] * 1e-3)
    hop[k]["inspected_edges_per_s"] = float("%.4g" % rate)
    hop[k]["GB_per_s_at_%dB_per_edge" % bytes_per_edge] = round(rate * bytes_per_edge / 1e9, 1)
hop["frontier_vertices"], hop["edges_inspected"], hop["longest_column"] = frontier.numel(), inspected, int(deg.max())
hop["columns_above_8192"] = int((deg > 8192).sum())
hop["labor_over_recent_ms"] = round(hop["labor"]["ms_median"] / hop["recent"]["ms_median"], 3)
hop["labor_over_plain_ms"] = round(hop["labor"]["ms_median"] / hop["plain_flat_hop"]["ms_median"], 3)
res["hop"] = hop
print(json.dumps({"hop": hop}), file=sys.stderr, flush=True)


def with_threshold(t):
    def call():
        _cabi.ns_hop_labor_long_column(t)
        _cabi.ns_hop_labor(graph, frontier, K, 0, 0, layer=1)
    return call


res["long"] = interleaved({"long_column_%d" % t: with_threshold(t) for t in (2048, 8192, 32768, 1 << 40)})
_cabi.ns_hop_labor_long_column(0)
print(json.dumps({"long": res["long"]}), file=sys.stderr, flush=True)
del out, frontier, fstates, graph, times

# ---- hub check: one column of 1 000 003 entries against the same entries in 62 501 columns of 16 ----
HUB = 1000003
cols16 = (HUB + 15) // 16
hub_ts = torch.randint(0, TMAX, (HUB,), generator=gen, device=dev)
hub_idx = torch.randint(0, n, (HUB,), generator=gen, device=dev)
p_one = torch.tensor([0, HUB], device=dev)
p_many = torch.clamp(torch.arange(cols16 + 1, device=dev) * 16, max=HUB)
kw = dict(timestamps=hub_ts, indices32=hub_idx.to(torch.int32))
g_one = _cabi.graph_view(p_one, hub_idx, ptrs32=p_one.to(torch.int32), **kw)
g_many = _cabi.graph_view(p_many, hub_idx, ptrs32=p_many.to(torch.int32), **kw)
v_one, v_many = torch.zeros(1, dtype=torch.int64, device=dev), torch.arange(cols16, device=dev)
one, many = "one_column_of_%d" % HUB, "%d_columns_of_16" % cols16
hub = interleaved({"labor_" + one: lambda: _cabi.ns_hop_labor(g_one, v_one, K, 0, 0),
                   "labor_" + many: lambda: _cabi.ns_hop_labor(g_many, v_many, K, 0, 0),
                   "recent_" + one: lambda: _cabi.ns_hop_recent(g_one, v_one, K),
                   "recent_" + many: lambda: _cabi.ns_hop_recent(g_many, v_many, K)})
for s in ("labor", "recent"):
    hub[s + "_one_column_over_many_ms"] = round(hub["%s_%s" % (s, one)]["ms_median"] / hub["%s_%s" % (s, many)]["ms_median"], 2)
res["hub"] = hub
print(json.dumps(res))
