"""Batched negative sampling, 1 024 inputs x 5 negatives x 5 tries per call: homogeneous on the CSR of RMAT-24 and
heterogeneous on BASELINE cfg4 (built as tools/bench_misc.py builds it: A = 2^23, B = C = 2^22 nodes, five relations x
20 M R-MAT edges; inputs of type A).  Prints one JSON line, per graph:
  per_call   the operator surface (negative_sample_neighbors_*), one call per launch chain, same process
  batched    tg_neg_sample_batched at N calls per launch (HIP events): ms per launch, calls/s, negatives/s, the LDS a
             workgroup asks for and the form taken (1 = one workgroup runs one call in LDS, 0 = call by call)
  loader     NegativeLoader end to end at its default prefetch (sampling, one read-back per launch, compaction; no
             attributes)."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tch-geometric_amd"))
import tch_geometric as tg  # noqa: E402
from tch_geometric import _cabi  # noqa: E402
from tch_geometric.loader import NegativeLoader  # noqa: E402
from tch_geometric.transforms import Graph, HeteroGraph  # noqa: E402

dev = torch.device("cuda:0")
SIZES = [int(x) for x in os.environ.get("SIZES", "1,16,64,256,1024").split(",")]
LOADER_BATCHES = int(os.environ.get("LOADER_BATCHES", 65536))
B, NUM_NEG, TRIES = 1024, 5, 5
res = {"config": "%d inputs x %d negatives x %d tries per call" % (B, NUM_NEG, TRIES)}


def per_call(fn, reps=200):
    for _ in range(5):
        out = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, out


def batched(n_types, rels, seeds, homogeneous):
    out = {}
    for N in SIZES:
        nb = _cabi.NegBatched(n_types, rels, [seeds[:N]] + [None] * (n_types - 1), NUM_NEG, TRIES, N, dev,
                              homogeneous=homogeneous)
        for i in range(10):                      # warm-up: code object, LDS attribute, clocks
            nb.run(7, i * N)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        reps = max(10, min(200, 16384 // N))
        ev[0].record()
        for i in range(reps):
            nb.run(7, (i + 1) * N)
        ev[1].record()
        torch.cuda.synchronize()
        ms = ev[0].elapsed_time(ev[1]) / reps
        counts, panic = nb.read_state()
        negatives = int(counts[:, n_types:].sum())
        out[str(N)] = {"ms_per_launch": ms, "us_per_call": ms / N * 1e3, "calls_per_s": N / ms * 1e3,
                       "negatives_per_s": negatives / ms * 1e3, "lds_bytes": nb.lds_bytes, "form": nb.form,
                       "workspace_bytes": nb.workspace_bytes, "slab_bytes": nb.launch_bytes - nb.workspace_bytes}
        assert not bool(panic.any())
        del nb
        torch.cuda.empty_cache()
    return out


def finish(out, data, nodes, **kw):
    ms1 = out["per_call"]["ms_per_call"]
    for v in out["batched"].values():
        v["per_call_over_batched"] = ms1 * 1e3 / v["us_per_call"]
    if LOADER_BATCHES:
        sum(1 for _ in NegativeLoader(data, NUM_NEG, TRIES, input_nodes=nodes[:4 * B], batch_size=B, seed=3, device=dev, **kw))
        loader = NegativeLoader(data, NUM_NEG, TRIES, input_nodes=nodes, batch_size=B, seed=3, device=dev, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = sum(1 for _ in loader)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out["loader"] = {"prefetch": loader.prefetch, "mini_batches": n, "s": dt, "mini_batches_per_s": n / dt}


# ---- homogeneous: CSR of RMAT-24
n = 1 << 24
row, col = _cabi.rmat_edges(24, n * 16, 0x5EED0000 + 24, dev)
ptrs, idx, _ = _cabi.coo_to_csx(row, col, n, n, False)
tg.seed(1)
inputs = _cabi.seed_batches(0x4E47, 0, 1, B, n, dev)[0].contiguous()
ms, o = per_call(lambda: tg.negative_sample_neighbors_homogenous(ptrs, idx, (n, n), inputs, NUM_NEG, TRIES))
homo = res["homogeneous_rmat24"] = {"per_call": {"ms_per_call": ms, "calls_per_s": 1e3 / ms, "negatives": int(o[1].numel()),
                                                 "negatives_per_s": int(o[1].numel()) / ms * 1e3}}
seeds = _cabi.seed_batches(0x4E47, 100, max(SIZES), B, n, dev)
homo["batched"] = batched(1, [(0, 0, ptrs, idx, n)], seeds, True)
finish(homo, Graph(edge_index=torch.stack([row, col]), num_nodes=n),
       _cabi.seed_batches(0x4E47, 7, max(LOADER_BATCHES, 4), B, n, dev).reshape(-1))
del row, col, ptrs, idx, seeds
torch.cuda.empty_cache()

# ---- heterogeneous: cfg4
scales = {"A": 23, "B": 22, "C": 22}
node_types = ["A", "B", "C"]
edge_types = [("A", "e0", "A"), ("A", "e1", "B"), ("B", "e2", "A"), ("B", "e3", "C"), ("C", "e4", "A")]
tix = {t: i for i, t in enumerate(node_types)}
PR, IR, sizes, rels = {}, {}, {}, []
data = HeteroGraph()
for t in node_types:
    data[t].num_nodes = 1 << scales[t]
for r, (s, nm, d) in enumerate(edge_types):
    rw, cl = _cabi.rmat_edges_rect(scales[s], scales[d], 20_000_000, 0xC0F4 + r, dev)
    key = "%s__%s__%s" % (s, nm, d)
    PR[key], IR[key], _ = _cabi.coo_to_csx(rw, cl, 1 << scales[s], 1 << scales[d], False)
    sizes[key] = (1 << scales[s], 1 << scales[d])
    rels.append((tix[s], tix[d], PR[key], IR[key], 1 << scales[d]))
    data[(s, nm, d)].edge_index = torch.stack([rw, cl])
del rw, cl
seeds1 = _cabi.seed_batches(0xBA7C4, 1, 1, B, 1 << 23, dev)[0].contiguous()
ms, o = per_call(lambda: tg.negative_sample_neighbors_heterogenous(node_types, edge_types, PR, IR, sizes, {"A": seeds1},
                                                                   NUM_NEG, TRIES, False))
neg = sum(int(v.numel()) for v in o[1].values())
het = res["heterogeneous_cfg4"] = {"per_call": {"ms_per_call": ms, "calls_per_s": 1e3 / ms, "negatives": neg,
                                                "negatives_per_s": neg / ms * 1e3}}
seeds = _cabi.seed_batches(0xBA7C4, 100, max(SIZES), B, 1 << 23, dev)
het["batched"] = batched(3, rels, seeds, False)
finish(het, data, _cabi.seed_batches(0xBA7C4, 7, max(LOADER_BATCHES, 4), B, 1 << 23, dev).reshape(-1), input_type="A")
print(json.dumps(res))
