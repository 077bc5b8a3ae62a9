"""tg_pinsage_hop and PinSAGELoader on RMAT-24 with reverse edges, in one process (the kept run:
profiles/bench_pinsage_loader.json).  Prints one JSON line:
  hop          the fused hop over a frontier of 16 x 1 024 seeds at (R, T, alpha, k) = (10, 2, 0.5, 3) -- DGL's example --,
               (200, 3, 0.5, 50) and (64, 64, 0.15, 64) at the limit of 4 096 visits, against the composition it replaces:
               _cabi.random_walk over the repeated frontier, a torch truncation (torch.rand draws: the same law, not the same
               numbers), sort, unique_consecutive and a segmented top-k.  HIP events around the calls, ROUNDS interleaved
               medians and their spread; steps per second (the steps are counted on the composition's truncated walks).
  phases       which phase bounds the hop, by this tool's own switch: the same hop at termination 0.99 (every walk ends
               after its first step: about 1 / T of the look-ups, the same rows to sort) and at termination 0 (every step is
               taken), beside _cabi.random_walk alone (the walking phase with its rows written to HBM).
  hub          62 501 frontier slots on ONE column of 1 000 003 entries against one slot on each of 62 501 columns of 16
               (T = 1: a step reads one entry, whatever the column's length).
  loader       PinSAGELoader mini-batches/s at L = 2, [3, 3], batch 1 024, prefetch 16, 128 f32 features, beside
               NeighborLoader(unique=True) with [3, 3] from the same run (a point of reference, not a target), and the
               distinct nodes per mini-batch of both."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tch-geometric_amd"))
from tch_geometric import _cabi  # noqa: E402
from tch_geometric.loader import NeighborLoader, PinSAGELoader  # noqa: E402
from tch_geometric.transforms import Graph  # noqa: E402

dev = torch.device("cuda:0")
SCALE = int(os.environ.get("SCALE", "24"))
D = int(os.environ.get("DIM", "128"))
BATCHES = int(os.environ.get("BATCHES", "64"))
ROUNDS = int(os.environ.get("ROUNDS", "3"))
B, PREFETCH, SEED = 1024, 16, 7
CONFIGS = {"R10_T2_a0.5_k3": (10, 2, 0.5, 3), "R200_T3_a0.5_k50": (200, 3, 0.5, 50), "R64_T64_a0.15_k64": (64, 64, 0.15, 64)}
RW_YARDSTICK = 23.8e9                                   # tg_random_walk's steps per second (README)
n = 1 << SCALE
row, col = _cabi.rmat_edges(SCALE, n * 16, 0x5EED0000 + SCALE, dev)
ei = torch.stack([torch.cat([row, col]), torch.cat([col, row])])
del row, col
data = Graph(edge_index=ei, num_nodes=n)
data.x = torch.empty((n, D), dtype=torch.float32, device=dev)
data.x.view(torch.int32)[:] = 1
seeds = _cabi.seed_batches(SEED, 0, 1, BATCHES * B, n, dev)[0]
seeds = torch.unique(seeds)[:BATCHES * B]                # a frontier lists a node once
seeds = seeds[torch.randperm(seeds.numel(), device=dev)][:(seeds.numel() // B) * B].contiguous()
res = {"config": "RMAT-%d with reverse edges (%d edges), batch %d, prefetch %d, %d f32 features, %d mini-batches per loader "
                 "pass, %d interleaved passes" % (SCALE, ei.shape[1], B, PREFETCH, D, seeds.numel() // B, ROUNDS),
       "timing": "hop, phases and hub: HIP events around the _cabi wrappers, which allocate their outputs per call"}


def event_ms(call, reps=3):
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


loaders = {"pinsage": PinSAGELoader(data, [3, 3], input_nodes=seeds, batch_size=B, n_walks=10, walk_length=2, termination=0.5,
                                    prefetch=PREFETCH, seed=SEED, symmetric=True, device=dev),
           "neighbor_unique": NeighborLoader(data, [3, 3], input_nodes=seeds, batch_size=B, prefetch=PREFETCH, seed=SEED,
                                             unique=True, device=dev)}
graph = loaders["pinsage"]._walk_graph
steps_taken = {}


def composition(frontier, R, T, alpha, k, name=None):
    """what a caller composed before: the walk matrix in HBM, a truncation, sort, run lengths, a segmented top-k"""
    m, V = frontier.numel(), R * T
    walks = _cabi.random_walk(graph, frontier.repeat_interleave(R), T, 1.0, 1.0, SEED, 0)[:, 1:]
    if T > 1:
        alive = torch.cumprod((torch.rand((m * R, T - 1), device=dev) >= alpha).to(torch.int64), 1).bool()
        walks[:, 1:] = torch.where(alive, walks[:, 1:], torch.full((), -1, dtype=torch.int64, device=dev))
    flat = walks.reshape(-1)
    keep = flat >= 0
    slot = torch.arange(m, device=dev).repeat_interleave(V)
    key = torch.sort(slot[keep] * n + flat[keep]).values
    if name is not None:
        steps_taken[name] = int(key.numel())
    uniq, counts = torch.unique_consecutive(key, return_counts=True)
    us, uid = uniq // n, uniq % n
    order = torch.sort((us * (V + 1) + (V - counts)) * n + uid).indices
    us, uid, counts = us[order], uid[order], counts[order]
    seg, seg_len = torch.unique_consecutive(us, return_counts=True)
    seg_start = torch.cumsum(seg_len, 0) - seg_len
    rank = torch.arange(us.numel(), device=dev) - seg_start.repeat_interleave(seg_len)
    top = rank < k
    return uid[top], us[top], counts[top]


def loader_pass(loader):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nb = nodes = 0
    for sb in loader.super_batches():
        _ = sb.node_attrs["x"]
        nb += len(sb)
        nodes += int(sb.n_id.numel())
    torch.cuda.synchronize()
    return time.perf_counter() - t0, nb, nodes


# ---- the loader ----
for ld in loaders.values():                            # un-timed: slabs, workspaces, the allocator's pools
    loader_pass(ld)
passes = {k: [] for k in loaders}
for _ in range(ROUNDS):
    for k, ld in loaders.items():
        passes[k].append(loader_pass(ld))
res["loader"] = {}
for k, ps in passes.items():
    rate = sorted(nb / dt for dt, nb, _ in ps)
    res["loader"][k] = {"mini_batches_per_s_median": round(statistics.median(rate), 1),
                        "mini_batches_per_s_best": round(rate[-1], 1), "spread_max_over_min": round(rate[-1] / rate[0], 3),
                        "distinct_nodes_per_mini_batch": round(statistics.mean(p[2] / p[1] for p in ps), 1)}
res["loader"]["pinsage_over_neighbor_unique"] = round(res["loader"]["pinsage"]["mini_batches_per_s_median"] /
                                                      res["loader"]["neighbor_unique"]["mini_batches_per_s_median"], 4)
print(json.dumps({"loader": res["loader"]}), file=sys.stderr, flush=True)
del loaders["neighbor_unique"], data
torch.cuda.empty_cache()

# ---- the hop alone, against the composition, and its phases ----
frontier = seeds[:PREFETCH * B].contiguous()
res["hop"], res["phases"] = {}, {}
for name, (R, T, alpha, k) in CONFIGS.items():
    composition(frontier, R, T, alpha, k, name)
    hop = interleaved({"fused": lambda: _cabi.pinsage_hop(graph, frontier, k, R, T, alpha, SEED, 0),
                       "composition": lambda: composition(frontier, R, T, alpha, k)})
    hop["fused_over_composition_ms"] = round(hop["fused"]["ms_median"] / hop["composition"]["ms_median"], 4)
    hop["frontier"], hop["walkers"], hop["steps_taken"] = frontier.numel(), frontier.numel() * R, steps_taken[name]
    rate = steps_taken[name] / (hop["fused"]["ms_median"] * 1e-3)
    hop["fused_steps_per_s"] = float("%.4g" % rate)
    hop["fused_steps_per_s_over_random_walk_yardstick"] = round(rate / RW_YARDSTICK, 4)
    res["hop"][name] = hop
    start = frontier.repeat_interleave(R)
    ph = interleaved({"hop_termination_0.99": lambda: _cabi.pinsage_hop(graph, frontier, k, R, T, 0.99, SEED, 0),
                      "hop_termination_0": lambda: _cabi.pinsage_hop(graph, frontier, k, R, T, 0.0, SEED, 0),
                      "random_walk_alone": lambda: _cabi.random_walk(graph, start, T, 1.0, 1.0, SEED, 0)})
    ph["note"] = "termination 0.99: about one step per walk and the same rows to sort, so close to the selecting phase alone"
    res["phases"][name] = ph
    print(json.dumps({name: {"hop": hop, "phases": ph}}), file=sys.stderr, flush=True)
    del start
    torch.cuda.empty_cache()

# ---- hub check: every slot on one column of 1 000 003 entries against one slot per column of 16 ----
HUB = 1000003
cols16 = (HUB + 15) // 16
gen = torch.Generator(device=dev).manual_seed(11)
hub_idx = torch.randint(0, cols16, (HUB,), generator=gen, device=dev)
p_one = torch.full((cols16 + 1,), HUB, dtype=torch.int64, device=dev)
p_one[0] = 0                                            # column 0 holds every entry, the others none
p_many = torch.clamp(torch.arange(cols16 + 1, device=dev) * 16, max=HUB)
kw = dict(indices32=hub_idx.to(torch.int32))
g_one = _cabi.graph_view(p_one, hub_idx, ptrs32=p_one.to(torch.int32), **kw)
g_many = _cabi.graph_view(p_many, hub_idx, ptrs32=p_many.to(torch.int32), **kw)
v_one, v_many = torch.zeros(cols16, dtype=torch.int64, device=dev), torch.arange(cols16, device=dev)
one, many = "%d_slots_on_one_column_of_%d" % (cols16, HUB), "%d_columns_of_16" % cols16
hub = interleaved({one: lambda: _cabi.pinsage_hop(g_one, v_one, 3, 10, 1, 0.5, SEED, 0),
                   many: lambda: _cabi.pinsage_hop(g_many, v_many, 3, 10, 1, 0.5, SEED, 0)})
hub["one_column_over_many_ms"] = round(hub[one]["ms_median"] / hub[many]["ms_median"], 3)
res["hub"] = hub
print(json.dumps(res))
