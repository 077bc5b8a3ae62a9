"""TemporalWalkLoader against what a trainer can do without it, on RMAT-24 with the reverse edges added and uniform int64
edge timestamps in [0, 1000): L = 20 columns, context 10, 10 walks per node, 1 negative row per walk, batch 128, prefetch
256, start times uniform in [0, 1000), window (0, 200), in one process.  Prints one JSON line (the kept run:
profiles/bench_temporal_walk_loader.json):
  loader       ROUNDS interleaved passes each, median / best / spread (max over min) in mini-batches/s, of
               (a) TemporalWalkLoader end to end, launch by launch (super_batches) and mini-batch by mini-batch as views;
               (b) the per-mini-batch composition it replaces: one _cabi.tempo_random_walk, strided slices + cat for the
                   nodes and for the timestamps, torch.randint, slices + cat;
               (c) the best without the fused launch: ONE _cabi.tempo_random_walk over all G * W walkers of a launch, then the
                   same torch window composition on the whole tensors;
               the bytes a mini-batch's three slabs hold and (a)'s write rate as a fraction of 8 TB/s
  launch       HIP events around single calls of the loader's launch shape: tg_tempo_skipgram (with and without pos_ts) and
               tg_tempo_random_walk over the same walkers (the walk alone, which bounds the fused launch from below)
With TILES=16x1,16x4,4x1,1x1 (walkers x wavefronts per workgroup) it prints a second JSON line (the kept run:
profiles/bench_temporal_walk_loader_tiles.json): the same launch under every workgroup shape (TG_TEMPO_SKIPGRAM_TILE,
TG_TEMPO_SKIPGRAM_WAVES), interleaved, ms per launch."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tch-geometric_amd"))
from tch_geometric import _cabi  # noqa: E402
from tch_geometric.loader import TemporalWalkLoader  # noqa: E402
from tch_geometric.transforms import Graph  # noqa: E402

dev = torch.device("cuda:0")
SCALE = int(os.environ.get("SCALE", "24"))
BATCHES = int(os.environ.get("BATCHES", "2048"))       # mini-batches of a timed pass
ROUNDS = int(os.environ.get("ROUNDS", "5"))
TILES = [tuple(int(v) for v in x.split("x")) for x in os.environ.get("TILES", "").split(",") if x]   # walkers x wavefronts
L, C, R, K, B, PREFETCH = 20, 10, 10, 1, 128, 256
TMAX, WINDOW = 1000, (0, 200)
HBM_ROOF = 8e12
nw, W, U = L - C + 1, R * B, R * K * B
n = 1 << SCALE
row, col = _cabi.rmat_edges(SCALE, n * 16, 0x5EED0000 + SCALE, dev)
ei = torch.stack([torch.cat([row, col]), torch.cat([col, row])])
del row, col
gen = torch.Generator(device=dev).manual_seed(0x7E4D0)
data = Graph(edge_index=ei, num_nodes=n, timestamps=torch.randint(0, TMAX, (ei.shape[1],), generator=gen, device=dev))
seeds = _cabi.seed_batches(0xBA7C4, 0, BATCHES, B, n, dev).reshape(-1)
seeds_ts = torch.randint(0, TMAX, (seeds.numel(),), generator=gen, device=dev)
slab_bytes = nw * C * 8 * (2 * W + U)                  # pos_rw, pos_ts, neg_rw of one mini-batch
res = {"config": "RMAT-%d + reverse edges, edge timestamps uniform in [0, %d), start times likewise, window %s, L %d columns, "
                 "context %d, %d walks per node, %d negative, batch %d, prefetch %d, %d mini-batches per pass, %d interleaved "
                 "passes" % (SCALE, TMAX, WINDOW, L, C, R, K, B, PREFETCH, BATCHES, ROUNDS),
       "slab_bytes_per_mini_batch": slab_bytes, "loader": {}, "launch": {}}

loader = TemporalWalkLoader(data, L, C, WINDOW, walks_per_node=R, num_negative_samples=K, input_nodes=seeds,
                            input_timestamps=seeds_ts, batch_size=B, prefetch=PREFETCH)
loader._prepare()
del ei
data.edge_index = data.timestamps = None               # the loader holds the CSR and the timestamps in its order
torch.cuda.empty_cache()
graph, node_ts, edge_ts = loader._graph, loader.node_ts, loader.edge_ts
res["walkers_per_workgroup"], res["lds_bytes_per_workgroup"] = _cabi.tempo_skipgram_lds_bytes(loader.cfg)


def loader_pass(whole_launches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nb = 0
    if whole_launches:
        for sb in loader.super_batches():
            nb += len(sb)
    else:
        for b in loader:
            _ = (b.pos_rw, b.pos_ts, b.neg_rw)
            nb += 1
    torch.cuda.synchronize()
    return time.perf_counter() - t0, nb


def windows(x, dim):
    """cat([x[..., k:k + C] for k in range(nw)], dim): the window composition on [.., rows, L]"""
    return torch.cat([x[..., k:k + C] for k in range(nw)], dim=dim)


def composition_pass():
    """(b) the same mini-batches from the one-call operator: what a trainer on the parent commit writes"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for j in range(BATCHES):
        batch, batch_ts = seeds[j * B:(j + 1) * B], seeds_ts[j * B:(j + 1) * B]
        rw, ts = _cabi.tempo_random_walk(graph, node_ts, edge_ts, batch.repeat(R), batch_ts.repeat(R), L, WINDOW, 0, j)
        pos_rw, pos_ts = windows(rw, 0), windows(ts, 0)
        neg_start = batch.repeat(R * K)
        nrw = torch.cat([neg_start.view(-1, 1), torch.randint(n, (neg_start.numel(), L - 1), device=dev)], dim=-1)
        neg_rw = windows(nrw, 0)
    torch.cuda.synchronize()
    assert pos_rw.shape == pos_ts.shape == (nw * W, C) and neg_rw.shape == (nw * U, C)
    return time.perf_counter() - t0, BATCHES


def one_walk_per_launch_pass():
    """(c) one tempo_random_walk over all G * W walkers of a launch, then the window composition on the whole tensors"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nb = 0
    for start, G, width, call_id in loader.plan(0):
        s = seeds[start:start + G * width].view(G, width)
        st = seeds_ts[start:start + G * width].view(G, width)
        rw, ts = _cabi.tempo_random_walk(graph, node_ts, edge_ts, s.repeat(1, R).reshape(-1), st.repeat(1, R).reshape(-1), L,
                                         WINDOW, 0, call_id)
        pos_rw, pos_ts = windows(rw.view(G, R * width, L), 1), windows(ts.view(G, R * width, L), 1)
        neg_start = s.repeat(1, R * K)
        nrw = torch.cat([neg_start.unsqueeze(-1), torch.randint(n, (G, R * K * width, L - 1), device=dev)], dim=-1)
        neg_rw = windows(nrw, 1)
        nb += G
    torch.cuda.synchronize()
    assert pos_rw.shape == pos_ts.shape == (G, nw * R * width, C) and neg_rw.shape == (G, nw * R * K * width, C)
    return time.perf_counter() - t0, nb


runs = {"loader_launches": lambda: loader_pass(True), "loader_mini_batches": lambda: loader_pass(False),
        "composition_per_mini_batch": composition_pass, "one_walk_per_launch": one_walk_per_launch_pass}
for f in runs.values():                                # un-timed: the allocator's pools, the first launches
    f()
passes = {k: [] for k in runs}
for _ in range(ROUNDS):
    for k, f in runs.items():
        passes[k].append(f())
entry = {}
for k, ps in passes.items():
    rate = sorted(nb / dt for dt, nb in ps)
    med = statistics.median(rate)
    entry[k] = {"mini_batches_per_s_median": round(med), "mini_batches_per_s_best": round(rate[-1]),
                "spread_max_over_min": round(rate[-1] / rate[0], 3)}
    if k.startswith("loader"):
        entry[k]["TB_written_per_s_median"] = round(med * slab_bytes / 1e12, 3)
        entry[k]["fraction_of_8TBps_roof"] = round(med * slab_bytes / HBM_ROOF, 3)
for k in ("loader_launches", "loader_mini_batches"):
    for other in ("composition_per_mini_batch", "one_walk_per_launch"):
        entry["%s_over_%s" % (k, other)] = round(entry[k]["mini_batches_per_s_median"] /
                                                 entry[other]["mini_batches_per_s_median"], 2)
res["loader"] = entry
print(json.dumps({"loader": entry}), file=sys.stderr, flush=True)

# ---- single launches of the loader's shape, HIP events ----
g_seeds = seeds[:PREFETCH * B].reshape(PREFETCH, B).contiguous()
g_ts = seeds_ts[:PREFETCH * B].reshape(PREFETCH, B).contiguous()
flat_s, flat_ts = g_seeds.repeat(1, R).reshape(-1), g_ts.repeat(1, R).reshape(-1)


def event_ms(call, reps=10):
    for _ in range(3):
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
    return {k: {"ms_per_launch_median": round(statistics.median(v), 4), "ms_per_launch_best": round(min(v), 4),
                "spread_max_over_min": round(max(v) / min(v), 3)} for k, v in ms.items()}


outs = {True: _cabi.tempo_skipgram(graph, node_ts, edge_ts, g_seeds, g_ts, loader.cfg, 0, 0, with_ts=True),
        False: _cabi.tempo_skipgram(graph, node_ts, edge_ts, g_seeds, g_ts, loader.cfg, 0, 0, with_ts=False)}
fused = lambda with_ts: _cabi.tempo_skipgram(graph, node_ts, edge_ts, g_seeds, g_ts, loader.cfg, 0, 0, with_ts=with_ts,
                                             out=outs[with_ts])
res["launch"] = interleaved({"tempo_skipgram": lambda: fused(True), "tempo_skipgram_without_pos_ts": lambda: fused(False),
                             "tempo_random_walk_same_walkers": lambda: _cabi.tempo_random_walk(
                                 graph, node_ts, edge_ts, flat_s, flat_ts, L, WINDOW, 0, 0)})
med = res["launch"]["tempo_skipgram"]["ms_per_launch_median"]
res["launch"]["tempo_skipgram"]["fraction_of_8TBps_roof"] = round(PREFETCH * slab_bytes / (med * 1e-3) / HBM_ROOF, 3)
res["launch"]["fused_over_walk_alone_ms"] = round(
    med / res["launch"]["tempo_random_walk_same_walkers"]["ms_per_launch_median"], 3)
print(json.dumps(res))

if TILES:
    def with_tile(tile, waves):
        def call():
            os.environ["TG_TEMPO_SKIPGRAM_TILE"], os.environ["TG_TEMPO_SKIPGRAM_WAVES"] = str(tile), str(waves)
            fused(True)
        return call
    ab = interleaved({"tile%dx%d" % tw: with_tile(*tw) for tw in TILES})
    for k in ("TG_TEMPO_SKIPGRAM_TILE", "TG_TEMPO_SKIPGRAM_WAVES"):
        os.environ.pop(k, None)
    for t, w in TILES:
        ab["tile%dx%d" % (t, w)]["lds_bytes_per_workgroup"] = t * (((2 * L) | 1) + 1) * 8
    ab["tempo_random_walk_same_walkers"] = res["launch"]["tempo_random_walk_same_walkers"]
    print(json.dumps({"config": res["config"] + "; one launch of %d mini-batches per workgroup shape (walkers x wavefronts), %d "
                                                "interleaved rounds of 10 launches" % (PREFETCH, ROUNDS), "tiles": ab}))
