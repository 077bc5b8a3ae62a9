"""Node2VecLoader against the composition it replaces, on RMAT-24 with the reverse edges added (walkers do not die early):
T = 20 steps, context 10, 10 walks per node, 1 negative row per walk, batch 128, prefetch 256, for p = q = 1 and for
p = 1, q = 1.5, in one process.  Prints one JSON line (the kept run: profiles/bench_node2vec_loader.json):
  loader       per (p, q): Node2VecLoader end to end, mini-batch views and whole launches (super_batches), against the
               composition built from the one-call operators only -- per mini-batch one _cabi.random_walk, PyG's strided
               slices + cat, torch.randint and its slices + cat -- ROUNDS passes each, interleaved, median and best, in
               mini-batches/s; the bytes a mini-batch's two slabs hold and the write rate as a fraction of 8 TB/s
  forms        one launch of the loader's shape in each form of tg_rw_skipgram (1 LDS uint32, 2 LDS int64, 3 flat), HIP
               events, ms per launch, and the ratio flat / LDS"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tch-geometric_amd"))
from tch_geometric import _cabi  # noqa: E402
from tch_geometric.loader import Node2VecLoader  # noqa: E402
from tch_geometric.transforms import Graph  # noqa: E402

dev = torch.device("cuda:0")
SCALE = int(os.environ.get("SCALE", "24"))
BATCHES = int(os.environ.get("BATCHES", "4096"))       # mini-batches of a timed pass
ROUNDS = int(os.environ.get("ROUNDS", "5"))
T, C, R, K, B, PREFETCH = 20, 10, 10, 1, 128, 256
HBM_ROOF = 8e12
L, nw = T + 1, T + 1 - C + 1
n = 1 << SCALE
row, col = _cabi.rmat_edges(SCALE, n * 16, 0x5EED0000 + SCALE, dev)
ei = torch.stack([torch.cat([row, col]), torch.cat([col, row])])
del row, col
data = Graph(edge_index=ei, num_nodes=n)
seeds = _cabi.seed_batches(0xBA7C4, 0, BATCHES, B, n, dev).reshape(-1)
slab_bytes = nw * R * B * C * 8 * (1 + K)
res = {"config": "RMAT-%d + reverse edges, T %d, context %d, %d walks per node, %d negative, batch %d, prefetch %d, "
                 "%d mini-batches per pass, %d interleaved passes" % (SCALE, T, C, R, K, B, PREFETCH, BATCHES, ROUNDS),
       "slab_bytes_per_mini_batch": slab_bytes, "loader": {}, "forms": {}}


def loader_pass(loader, whole_launches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nb = 0
    if whole_launches:
        for sb in loader.super_batches():
            nb += len(sb)
    else:
        for b in loader:
            _ = (b.pos_rw, b.neg_rw)
            nb += 1
    torch.cuda.synchronize()
    return time.perf_counter() - t0, nb


def composition_pass(graph, edge_set, p, q):
    """the same mini-batches from the one-call operators: what a trainer on the parent commit writes"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for j in range(BATCHES):
        batch = seeds[j * B:(j + 1) * B]
        start = batch.repeat(R)
        rw = _cabi.random_walk(graph, start, T, p, q, 0, j, edge_set=edge_set)
        pos_rw = torch.cat([rw[:, k:k + C] for k in range(nw)], dim=0)
        neg_start = batch.repeat(R * K)
        nrw = torch.cat([neg_start.view(-1, 1), torch.randint(n, (neg_start.numel(), T), device=dev)], dim=-1)
        neg_rw = torch.cat([nrw[:, k:k + C] for k in range(nw)], dim=0)
    torch.cuda.synchronize()
    assert pos_rw.shape == (nw * R * B, C) and neg_rw.shape == (nw * R * K * B, C)
    return time.perf_counter() - t0, BATCHES


for p, q in ((1.0, 1.0), (1.0, 1.5)):
    loader = Node2VecLoader(data, T, C, walks_per_node=R, num_negative_samples=K, p=p, q=q, input_nodes=seeds, batch_size=B,
                            prefetch=PREFETCH)
    loader._prepare()
    runs = {"loader_mini_batches": lambda: loader_pass(loader, False), "loader_launches": lambda: loader_pass(loader, True),
            "composition": lambda: composition_pass(loader._graph, loader._edge_set, p, q)}
    for f in runs.values():                            # un-timed: the allocator's pools, the first launches
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
                    "TB_written_per_s_median": round(med * slab_bytes / 1e12, 3),
                    "fraction_of_8TBps_roof": round(med * slab_bytes / HBM_ROOF, 3)}
    for k in ("loader_mini_batches", "loader_launches"):
        entry[k + "_over_composition"] = round(entry[k]["mini_batches_per_s_median"] /
                                               entry["composition"]["mini_batches_per_s_median"], 2)
    # one launch in each form
    g_seeds = seeds[:PREFETCH * B].reshape(PREFETCH, B).contiguous()
    forms = {}
    for form in (1, 2, 3):
        cfg = loader.cfg
        nbytes = _cabi.rw_skipgram_workspace_bytes(cfg, PREFETCH, B, n, form)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev) if nbytes else None
        out = None
        call = lambda: _cabi.rw_skipgram(loader._graph, g_seeds, T, C, R, K, p, q, 0, 0, n, edge_set=loader._edge_set,
                                         form=form, ws=ws, out=out)
        out = call()
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(ROUNDS):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(10):
                call()
            ev[1].record()
            torch.cuda.synchronize()
            ms.append(ev[0].elapsed_time(ev[1]) / 10)
        med = statistics.median(ms)
        forms["form%d" % form] = {"ms_per_launch_median": round(med, 4), "ms_per_launch_best": round(min(ms), 4),
                                  "workspace_bytes": nbytes,
                                  "fraction_of_8TBps_roof": round(PREFETCH * slab_bytes / (med * 1e-3) / HBM_ROOF, 3)}
        del ws, out
    forms["flat_over_lds32_ms"] = round(forms["form3"]["ms_per_launch_median"] / forms["form1"]["ms_per_launch_median"], 2)
    forms["lds64_over_lds32_ms"] = round(forms["form2"]["ms_per_launch_median"] / forms["form1"]["ms_per_launch_median"], 2)
    key = "p%g_q%g" % (p, q)
    res["loader"][key], res["forms"][key] = entry, forms
    print(json.dumps({key: {"loader": entry, "forms": forms}}), file=sys.stderr, flush=True)
    del loader, runs
    torch.cuda.empty_cache()
print(json.dumps(res))
