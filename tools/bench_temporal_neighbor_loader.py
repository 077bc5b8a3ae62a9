"""The most-recent-k sampler and the temporal NeighborLoader on RMAT-24 with uniform int64 edge times and seed times in
[0, 1000): fan-outs [15, 10], batch 1024, prefetch 16, one process, interleaved passes, medians with the spread.  Prints one
JSON line (the kept run: profiles/bench_temporal_neighbor_loader.json):
  hop      one hop of tg_ns_hop_recent against tg_ns_hop_scan (the yardstick) over the same frontier (the loader's hop 1:
           16 x 1024 x 15 slots drawn by degree, so hubs repeat) and the same backward RELATIVE filter: ms, the ratio, the
           edges inspected and each hop's rate as a fraction of the 8 TB/s roof at 8 bytes per inspected edge.  The timed
           calls are the _cabi wrappers, as a caller sees them: each allocates its outputs, tg_ns_hop_scan's also sizes
           and allocates its workspace and zeroes a status word -- host work inside the events that differs between the
           two and, if anything, counts against the yardstick; these are not pure kernel times
  hub      tg_ns_hop_recent over one column of 1 000 003 entries against the same entries in 62 501 columns of 16: the ratio
           is what scanning a hub on ONE wavefront costs
  loader   NeighborLoader mini-batches/s for temporal_strategy "last", "uniform" and untimed, all unique=False
The kernel's registers, scratch and LDS are the compiler's to report (-Rpass-analysis=kernel-resource-usage), not this tool's.
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
BATCHES = int(os.environ.get("BATCHES", "128"))        # mini-batches of a timed pass
ROUNDS = int(os.environ.get("ROUNDS", "5"))
FAN, B, PREFETCH, TMAX, WINDOW = [15, 10], 1024, 16, 1000, (0, 2 ** 62)
HBM_ROOF = 8e12
n = 1 << SCALE
row, col = _cabi.rmat_edges(SCALE, n * 16, 0x5EED0000 + SCALE, dev)
gen = torch.Generator(device=dev).manual_seed(0x7E4D1)
data = Graph(edge_index=torch.stack([row, col]), num_nodes=n,
             time=torch.randint(0, TMAX, (row.numel(),), generator=gen, device=dev))
del row, col
seeds = _cabi.seed_batches(0xBA7C4, 0, BATCHES, B, n, dev).reshape(-1)
seeds_t = torch.randint(0, TMAX, (seeds.numel(),), generator=gen, device=dev)
res = {"config": "RMAT-%d, edge times and seed times uniform in [0, %d), fan-outs %s, batch %d, prefetch %d, %d mini-batches per "
                 "pass, %d interleaved passes" % (SCALE, TMAX, FAN, B, PREFETCH, BATCHES, ROUNDS),
       "timing": "hop and hub: HIP events around the _cabi wrappers, which allocate their outputs per call (the scan hop's also "
                 "sizes and allocates its workspace and zeroes its status word): not pure kernel times"}

loaders = {"last": NeighborLoader(data, FAN, input_nodes=seeds, batch_size=B, prefetch=PREFETCH, time_attr="time",
                                  input_time=seeds_t, temporal_strategy="last"),
           "uniform": NeighborLoader(data, FAN, input_nodes=seeds, batch_size=B, prefetch=PREFETCH, time_attr="time",
                                     input_time=seeds_t, temporal_strategy="uniform"),
           "untimed": NeighborLoader(data, FAN, input_nodes=seeds, batch_size=B, prefetch=PREFETCH)}
graph, ptrs = loaders["last"]._graph, loaders["last"].col_ptrs


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


# ---- one hop: the loader's hop-1 frontier (hop 0's samples of a full launch), both hops under the loader's filter ----
G = min(PREFETCH, BATCHES)
out = _cabi.NsBatchedOut(G, B, FAN[:1], dev, with_states=True)
ws = _cabi.ns_homo_batched_workspace(graph, G, B, FAN[:1], dev, sampler=_cabi.SAMPLER_RECENT, filter_mode=_cabi.FILTER_RELATIVE)
_cabi.ns_homo_batched(graph, seeds[:G * B].reshape(G, B), FAN[:1], 0, 0, out, sampler=_cabi.SAMPLER_RECENT,
                      filter_mode=_cabi.FILTER_RELATIVE, window=WINDOW, seeds_state=seeds_t[:G * B].reshape(G, B), ws=ws)
counts = out.counts.cpu()
frontier = torch.cat([out.samples[b, B:int(counts[b, 0])] for b in range(G)]).contiguous()
fstates = torch.cat([out.states[b, B:int(counts[b, 0])] for b in range(G)]).contiguous()
deg = (ptrs[1:] - ptrs[:-1])[frontier]
inspected = int(deg.sum())
hop = interleaved({
    "recent": lambda: _cabi.ns_hop_recent(graph, frontier, FAN[1], states=fstates, filter_mode=_cabi.FILTER_RELATIVE,
                                          window=WINDOW),
    "scan": lambda: _cabi.ns_hop_scan(graph, frontier, fstates, FAN[1], 0, _cabi.FILTER_RELATIVE, WINDOW)})
for k in hop:
    hop[k]["fraction_of_8TBps_roof_at_8B_per_inspected_edge"] = round(inspected * 8 / (hop[k]["ms_median"] * 1e-3) / HBM_ROOF, 4)
hop["frontier_vertices"], hop["edges_inspected"], hop["longest_column"] = frontier.numel(), inspected, int(deg.max())
hop["recent_over_scan_ms"] = round(hop["recent"]["ms_median"] / hop["scan"]["ms_median"], 3)
res["hop"] = hop
print(json.dumps({"hop": hop}), file=sys.stderr, flush=True)
del out, ws, frontier, fstates

# ---- hub check: one column of 1 000 003 entries against the same entries in 62 501 columns of 16 ----
HUB = 1000003
cols16 = (HUB + 15) // 16
hub_ts = torch.randint(0, TMAX, (HUB,), generator=gen, device=dev)
hub_idx = torch.randint(0, n, (HUB,), generator=gen, device=dev)
p_one = torch.tensor([0, HUB], device=dev)
p_many = torch.clamp(torch.arange(cols16 + 1, device=dev) * 16, max=HUB)
g_one = _cabi.graph_view(p_one, hub_idx, timestamps=hub_ts)
g_many = _cabi.graph_view(p_many, hub_idx, timestamps=hub_ts)
v_one, v_many = torch.zeros(1, dtype=torch.int64, device=dev), torch.arange(cols16, device=dev)
hubr = interleaved({"one_column_of_%d" % HUB: lambda: _cabi.ns_hop_recent(g_one, v_one, FAN[1]),
                    "%d_columns_of_16" % cols16: lambda: _cabi.ns_hop_recent(g_many, v_many, FAN[1])})
a, b = hubr["one_column_of_%d" % HUB]["ms_median"], hubr["%d_columns_of_16" % cols16]["ms_median"]
hubr["one_column_over_many_ms"] = round(a / b, 2)
hubr["one_wavefront_GB_per_s"] = round(HUB * 8 / (a * 1e-3) / 1e9, 2)
res["hub"] = hubr
print(json.dumps({"hub": hubr}), file=sys.stderr, flush=True)


# ---- loader throughput ----
def loader_pass(loader):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nb = 0
    for sb in loader.super_batches():
        nb += len(sb)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, nb


for ld in loaders.values():                            # un-timed: slabs, workspaces, the allocator's pools
    loader_pass(ld)
passes = {k: [] for k in loaders}
for _ in range(ROUNDS):
    for k, ld in loaders.items():
        passes[k].append(loader_pass(ld))
entry = {}
for k, ps in passes.items():
    rate = sorted(nb / dt for dt, nb in ps)
    entry[k] = {"mini_batches_per_s_median": round(statistics.median(rate), 1), "mini_batches_per_s_best": round(rate[-1], 1),
                "spread_max_over_min": round(rate[-1] / rate[0], 3)}
entry["last_over_uniform"] = round(entry["last"]["mini_batches_per_s_median"] / entry["uniform"]["mini_batches_per_s_median"], 3)
entry["last_over_untimed"] = round(entry["last"]["mini_batches_per_s_median"] / entry["untimed"]["mini_batches_per_s_median"], 3)
res["loader"] = entry
print(json.dumps(res))
