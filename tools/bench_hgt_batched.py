"""Batched hgt_sampling on BASELINE cfg4 (built as tools/bench_hetero.py builds it: A = 2^23, B = C = 2^22 nodes, five
relations x 20 M R-MAT edges; 1 024 seeds of type A, [512, 512] per type, 2 hops).  Prints one JSON line:
  per_call   tg.hgt_sampling, one call per launch chain (the operator surface)
  batched    tg_hgt_sample_batched at N calls per launch (HIP events): ms per launch, calls/s, nodes + edges per second,
             the workspace, and the roofline by bench.py's cfg4_hgt byte rule (16 B + 8 B x min(deg, 50) per node and
             relation into its type, per budget update and again per output node)
  loader     HGTLoader end to end at its default prefetch (sampling, read-back, compaction, no attributes)."""
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
P, I, COO = {}, {}, {}
for r, (s, _, d) in enumerate(edge_types):
    row, col = _cabi.rmat_edges_rect(scales[s], scales[d], E, 0xC0F4 + r, dev)
    key = "%s__%s__%s" % (s, edge_types[r][1], d)
    P[key], I[key], _ = _cabi.coo_to_csx(row, col, 1 << scales[s], 1 << scales[d], True)
    COO[edge_types[r]] = torch.stack([row, col])
del row, col
tix = {t: i for i, t in enumerate(node_types)}
rels = [(tix[s], tix[d], P["%s__%s__%s" % (s, r, d)], I["%s__%s__%s" % (s, r, d)], None) for s, r, d in edge_types]
ns = {t: [512, 512] for t in node_types}
res = {"config": "cfg4: 3 ntypes (2^23, 2^22, 2^22), 5 etypes x %d edges, 1024 seeds of type A, [512, 512] per type, "
                 "2 hops" % E}


def alg_bytes(samples, n_seeds):
    """bench.py's cfg4_hgt rule for one call (samples: per type its node list)."""
    total = 0
    for s_, r_, d_ in edge_types:
        p_ = P["%s__%s__%s" % (s_, r_, d_)]
        w_ = samples[tix[d_]]
        deg = (p_[w_ + 1] - p_[w_]).clamp(max=50)
        upd = w_.numel() - min(ns[d_][-1], max(w_.numel() - (n_seeds if d_ == "A" else 0), 0))
        total += int((16 * upd + 8 * deg[:upd].sum()).item()) + int((16 * w_.numel() + 8 * deg.sum()).item())
    return total


# ---- one call per launch chain
tg.seed(1)
seeds1 = _cabi.seed_batches(0xBA7C4, 1, 1, 1024, 1 << 23, dev)[0].contiguous()
call = lambda: tg.hgt_sampling(node_types, edge_types, P, I, None, {"A": seeds1}, None, ns, 2)
for _ in range(3):
    out = call()
torch.cuda.synchronize()
reps = 50
t0 = time.perf_counter()
for _ in range(reps):
    out = call()
torch.cuda.synchronize()
ms1 = (time.perf_counter() - t0) / reps * 1e3
nodes = sum(int(v.numel()) for v in out[0].values())
edges = sum(int(v.numel()) for v in out[2].values())
b1 = alg_bytes([out[0][t] for t in node_types], 1024)
res["per_call"] = {"ms_per_call": ms1, "calls_per_s": 1e3 / ms1, "nodes": nodes, "edges": edges,
                   "roofline_frac": b1 / (ms1 * 1e-3) / 1e9 / HBM_PEAK_GBS}

# ---- batched
res["batched"] = {}
for N in SIZES:
    seeds = _cabi.seed_batches(0xBA7C4, 100, N, 1024, 1 << 23, dev)
    hb = _cabi.HgtBatched(3, rels, [seeds, None, None], [ns[t] for t in node_types], 2, N, dev)
    hb.run(7, 0)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    reps = max(3, min(20, 2048 // N))
    ev[0].record()
    for i in range(reps):
        hb.run(7, (i + 1) * N)
    ev[1].record()
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / reps
    c = hb.counts.cpu()
    n_ne = int(c[:, :8].sum())
    ab = sum(alg_bytes([hb.samples[t][b, :int(c[b, t])] for t in range(3)], 1024) for b in range(min(N, 8))) * N / min(N, 8)
    res["batched"][str(N)] = {"ms_per_launch": ms, "calls_per_s": N / ms * 1e3, "nodes_plus_edges_per_s": n_ne / ms * 1e3,
                              "workspace_bytes": hb.workspace_bytes, "panics": int(c[:, 8].sum()),
                              "roofline_frac": ab / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
    del hb
    torch.cuda.empty_cache()
best = max(v["calls_per_s"] for v in res["batched"].values())
res["speedup_vs_per_call"] = best / res["per_call"]["calls_per_s"]

# ---- loader
from tch_geometric.loader import HGTLoader  # noqa: E402
from tch_geometric.transforms import HeteroGraph  # noqa: E402
data = HeteroGraph()
for t in node_types:
    data[t].num_nodes = 1 << scales[t]
for et in edge_types:
    data[et].edge_index = COO[et]
n_batches = int(os.environ.get("LOADER_BATCHES", 1024))
nodes = _cabi.seed_batches(0xBA7C4, 7, n_batches, 1024, 1 << 23, dev).reshape(-1)
loader = HGTLoader(data, [512, 512], "A", input_nodes=nodes, batch_size=1024, seed=3, device=dev)   # default prefetch
torch.cuda.synchronize()
t0 = time.perf_counter()
n = sum(1 for _ in loader)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
res["loader"] = {"prefetch": loader.prefetch, "mini_batches": n, "s": dt, "mini_batches_per_s": n / dt}
print(json.dumps(res))
