"""Batched budget_sampling on BASELINE cfg4 (built as tools/bench_misc.py builds it: A = 2^23, B = C = 2^22 nodes, five
relations x 20 M R-MAT edges; 1 024 seeds of type A, [15, 10] per type, 2 hops), first without a filter, then with a
window on synthetic timestamps (row timestamps on every relation, one per seed).  Prints one JSON line:
  per_call   tg.budget_sampling, one call per launch chain (the operator surface)
  batched    tg_budget_sample_batched at N calls per launch (HIP events): ms per launch, calls/s, nodes + edges per second,
             the workspace and the output slabs, and the roofline by bench.py's byte rule for budget updates (16 B + 8 B x
             min(deg, 50) per (node, relation into its type), for every node a hop expands; the timestamps a window
             reads are not counted)
  loader     BudgetLoader end to end at its default prefetch (sampling, read-back, compaction, e_id; no attributes)."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tch-geometric_amd"))
import tch_geometric as tg  # noqa: E402
from tch_geometric import _cabi  # noqa: E402

HBM_PEAK_GBS = 8000.0
dev = torch.device("cuda:0")
scales = {"A": 23, "B": 22, "C": 22}
node_types = ["A", "B", "C"]
edge_types = [("A", "e0", "A"), ("A", "e1", "B"), ("B", "e2", "A"), ("B", "e3", "C"), ("C", "e4", "A")]
E = int(os.environ.get("EDGES", 20_000_000))
SIZES = [int(x) for x in os.environ.get("SIZES", "1,16,64,256,512").split(",")]
TS_RANGE, WINDOW = 1000, (0, 500)      # the window keeps a neighbour up to 500 time units older than its node
P, I, RTS, COO = {}, {}, {}, {}
gen = torch.Generator(device=dev)
gen.manual_seed(0x7157)
for r, (s, nm, d) in enumerate(edge_types):
    row, col = _cabi.rmat_edges_rect(scales[s], scales[d], E, 0xC0F4 + r, dev)
    key = "%s__%s__%s" % (s, nm, d)
    P[key], I[key], _ = _cabi.coo_to_csx(row, col, 1 << scales[s], 1 << scales[d], True)
    RTS[key] = torch.randint(0, TS_RANGE, (E,), generator=gen, device=dev)
    COO[edge_types[r]] = torch.stack([row, col])
del row, col
tix = {t: i for i, t in enumerate(node_types)}
keys = ["%s__%s__%s" % et for et in edge_types]
nn = {t: [15, 10] for t in node_types}
res = {"config": "cfg4: 3 ntypes (2^23, 2^22, 2^22), 5 etypes x %d edges, 1024 seeds of type A, [15, 10] per type, 2 hops; "
                 "window: row and seed timestamps uniform in [0, %d), window %s backward" % (E, TS_RANGE, list(WINDOW))}


def rels(temporal):
    return [(tix[s], tix[d], P[k], I[k], RTS[k] if temporal else None) for (s, _, d), k in zip(edge_types, keys)]


def alg_bytes_per_call(seeds, seeds_ts, kw, n=8):
    """bench.py's byte rule over the nodes every hop expands: the inputs, then what hop 0 appended -- the lists of the
    same calls run with one hop (hop 0 draws the same there).  Mean over n calls."""
    one = _cabi.BudgetBatched(3, rels(kw["window"] is not None), [seeds[:n], None, None], [[nn[t][0]] for t in node_types],
                              1, n, dev, input_ts=None if seeds_ts is None else [seeds_ts[:n], None, None], **kw)
    one.run(7, 0)
    c = one.counts.cpu()
    total = 0
    for b in range(n):
        for (s_, r_, d_), k in zip(edge_types, keys):
            w = one.samples[tix[d_]][b, :int(c[b, tix[d_]])]
            deg = (P[k][w + 1] - P[k][w]).clamp(max=50)
            total += 16 * w.numel() + 8 * int(deg.sum())
    return total / n


for name, kw in (("plain", dict(window=None)), ("window", dict(window=WINDOW, forward=False, relative=False))):
    temporal = kw["window"] is not None
    out = res[name] = {}
    # ---- one call per launch chain
    tg.seed(1)
    seeds1 = _cabi.seed_batches(0xBA7C4, 1, 1, 1024, 1 << 23, dev)[0].contiguous()
    ts1 = torch.randint(0, TS_RANGE, (1024,), generator=gen, device=dev) if temporal else None
    call = lambda: tg.budget_sampling(node_types, edge_types, P, I, RTS if temporal else None, {"A": seeds1},
                                      {"A": ts1} if temporal else None, nn, 2, kw["window"], False, False)
    for _ in range(3):
        o = call()
    torch.cuda.synchronize()
    reps = 100
    t0 = time.perf_counter()
    for _ in range(reps):
        o = call()
    torch.cuda.synchronize()
    ms1 = (time.perf_counter() - t0) / reps * 1e3
    out["per_call"] = {"ms_per_call": ms1, "calls_per_s": 1e3 / ms1, "nodes": sum(int(v.numel()) for v in o[0].values()),
                       "edges": sum(int(v.numel()) for v in o[2].values())}
    # ---- batched
    seeds = _cabi.seed_batches(0xBA7C4, 100, max(SIZES), 1024, 1 << 23, dev)
    seeds_ts = torch.randint(0, TS_RANGE, seeds.shape, generator=gen, device=dev) if temporal else None
    ab = alg_bytes_per_call(seeds, seeds_ts, kw)
    out["alg_bytes_per_call"] = ab
    out["batched"] = {}
    for N in SIZES:
        bb = _cabi.BudgetBatched(3, rels(temporal), [seeds[:N], None, None], [nn[t] for t in node_types], 2, N, dev,
                                 input_ts=None if seeds_ts is None else [seeds_ts[:N], None, None], **kw)
        bb.run(7, 0)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        reps = max(5, min(50, 4096 // N))
        ev[0].record()
        for i in range(reps):
            bb.run(7, (i + 1) * N)
        ev[1].record()
        torch.cuda.synchronize()
        ms = ev[0].elapsed_time(ev[1]) / reps
        n_ne = int(bb.counts.sum())
        out["batched"][str(N)] = {"ms_per_launch": ms, "calls_per_s": N / ms * 1e3, "nodes_plus_edges_per_s": n_ne / ms * 1e3,
                                  "workspace_bytes": bb.workspace_bytes, "slab_bytes": bb.launch_bytes - bb.workspace_bytes,
                                  "roofline_frac": ab * N / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
        del bb
        torch.cuda.empty_cache()
    best = max(v["calls_per_s"] for v in out["batched"].values())
    out["speedup_vs_per_call"] = best / out["per_call"]["calls_per_s"]
    if "256" in out["batched"]:
        out["speedup_at_256"] = out["batched"]["256"]["calls_per_s"] / out["per_call"]["calls_per_s"]

# ---- loader
from tch_geometric.loader import BudgetLoader  # noqa: E402
from tch_geometric.transforms import HeteroGraph  # noqa: E402
n_batches = int(os.environ.get("LOADER_BATCHES", 1024))
if n_batches:
    data = HeteroGraph()
    for t in node_types:
        data[t].num_nodes = 1 << scales[t]
    for et in edge_types:
        data[et].edge_index = COO[et]
    nodes = _cabi.seed_batches(0xBA7C4, 7, n_batches, 1024, 1 << 23, dev).reshape(-1)
    loader = BudgetLoader(data, [15, 10], "A", input_nodes=nodes, batch_size=1024, seed=3, device=dev)   # default prefetch
    sum(1 for _ in BudgetLoader(data, [15, 10], "A", input_nodes=nodes[:4096], batch_size=1024, seed=3, device=dev))  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = sum(1 for _ in loader)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res["loader"] = {"prefetch": loader.prefetch, "mini_batches": n, "s": dt, "mini_batches_per_s": n / dt}
print(json.dumps(res))
