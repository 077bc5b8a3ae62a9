"""MetaPath2VecLoader against the composition it replaces, on the cfg4-style synthetic graph of
tools/bench_hetero_link_loader.py (3 node types A = 2^23, B = 2^22, C = 2^22; 5 relations x 20 M rectangular R-MAT edges):
T = 20 steps, context 10, 10 walks per node, 1 negative row per walk, batch 128, prefetch 256, along the closed metapath of
2 relations A-e1-B-e2-A and the one of 4 relations A-e1-B-e3-C-e4-A-e0-A, in one process.  Prints one JSON line (the kept
run: profiles/bench_metapath2vec_loader.json):
  loader       per metapath: MetaPath2VecLoader end to end, mini-batch views and whole launches (super_batches), against
               the composition a trainer writes from torch ops -- per mini-batch and step a degree look-up in the step's
               CSR, a torch.rand-based neighbour pick, then torch.randint negatives per column type, the offset add, PyG's
               strided slices + cat -- ROUNDS passes each, interleaved, median and best, in mini-batches/s; the bytes a
               mini-batch's two slabs hold and the write rate as a fraction of 8 TB/s; the share of positive words that
               are dummy_idx (walks that met a row without out-edges)
  forms        one launch of the loader's shape (256 mini-batches) in each form of tg_mp_skipgram (1 LDS uint32, 2 LDS
               int64, 3 flat), HIP events, ms per launch, and the ratio flat / LDS"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tch-geometric_amd"))
from tch_geometric import _cabi  # noqa: E402
from tch_geometric.loader import MetaPath2VecLoader  # noqa: E402
from tch_geometric.transforms import HeteroGraph  # noqa: E402

dev = torch.device("cuda:0")
SHIFT = int(os.environ.get("SHIFT", "0"))              # > 0: a smaller graph (every scale lowered by SHIFT)
scales = {"A": 23 - SHIFT, "B": 22 - SHIFT, "C": 22 - SHIFT}
node_types = ["A", "B", "C"]
edge_types = [("A", "e0", "A"), ("A", "e1", "B"), ("B", "e2", "A"), ("B", "e3", "C"), ("C", "e4", "A")]
N_EDGES = int(os.environ.get("EDGES", 20_000_000 >> SHIFT))
BATCHES = int(os.environ.get("BATCHES", "1024"))       # mini-batches of a timed pass
ROUNDS = int(os.environ.get("ROUNDS", "5"))
T, C, R, K, B, PREFETCH = 20, 10, 10, 1, 128, 256
HBM_ROOF = 8e12
L, nw = T + 1, T + 1 - C + 1
METAPATHS = {"A-e1-B-e2-A": [edge_types[1], edge_types[2]],
             "A-e1-B-e3-C-e4-A-e0-A": [edge_types[1], edge_types[3], edge_types[4], edge_types[0]]}
data = HeteroGraph()
for t in node_types:
    data[t].num_nodes = 1 << scales[t]
for r, et in enumerate(edge_types):
    data[et].edge_index = torch.stack(_cabi.rmat_edges_rect(scales[et[0]], scales[et[2]], N_EDGES, 0xC0F4 + r, dev))
seeds = _cabi.seed_batches(0xBA7C4, 0, BATCHES, B, 1 << scales["A"], dev).reshape(-1)
slab_bytes = nw * R * B * C * 8 * (1 + K)
res = {"config": "3 ntypes (2^%d, 2^%d, 2^%d), 5 etypes x %d edges, T %d, context %d, %d walks per node, %d negative, batch %d, "
                 "prefetch %d, %d mini-batches per pass, %d interleaved passes"
                 % (scales["A"], scales["B"], scales["C"], N_EDGES, T, C, R, K, B, PREFETCH, BATCHES, ROUNDS),
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


def composition_pass(loader, csr):
    """the same kind of mini-batches from torch ops: what a trainer on the parent commit writes (PyG's MetaPath2Vec)"""
    path, M = loader.metapath, len(loader.metapath)
    col_types = [path[0][0]] + [path[l % M][2] for l in range(T)]
    start = [loader.start[t] for t in col_types]
    count = [loader.end[t] - loader.start[t] for t in col_types]
    dummy = loader.dummy_idx
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for j in range(BATCHES):
        batch = seeds[j * B:(j + 1) * B]
        cur = batch.repeat(R)
        alive = torch.ones_like(cur, dtype=torch.bool)
        cols = [cur + start[0]]
        for l in range(T):
            ptrs, idx = csr[path[l % M]]
            b = ptrs[cur]
            deg = ptrs[cur + 1] - b                                        # the degree look-up
            alive = alive & (deg > 0)
            pick = (torch.rand(cur.numel(), device=dev) * deg).to(torch.int64).clamp_(max=N_EDGES - 1)
            cur = torch.where(alive, idx[(b + pick).clamp_(max=N_EDGES - 1)], torch.zeros_like(cur))
            cols.append(torch.where(alive, cur + start[l + 1], dummy))     # the offset add, dummy_idx behind an ended walk
        rw = torch.stack(cols, dim=-1)
        pos_rw = torch.cat([rw[:, k:k + C] for k in range(nw)], dim=0)
        neg_start = batch.repeat(R * K)
        ncols = [neg_start + start[0]] + [torch.randint(count[m], (neg_start.numel(),), device=dev) + start[m]
                                          for m in range(1, L)]            # randint per column type
        nrw = torch.stack(ncols, dim=-1)
        neg_rw = torch.cat([nrw[:, k:k + C] for k in range(nw)], dim=0)
    torch.cuda.synchronize()
    assert pos_rw.shape == (nw * R * B, C) and neg_rw.shape == (nw * R * K * B, C)
    return time.perf_counter() - t0, BATCHES


for key, path in METAPATHS.items():
    loader = MetaPath2VecLoader(data, path, T, C, walks_per_node=R, num_negative_samples=K, input_nodes=seeds, batch_size=B,
                                prefetch=PREFETCH)
    loader._prepare()
    csr = {et: g._keep[:2] for et, g in loader._graph.items()}             # the loader's own CSRs (ptrs, indices)
    runs = {"loader_mini_batches": lambda: loader_pass(loader, False), "loader_launches": lambda: loader_pass(loader, True),
            "composition": lambda: composition_pass(loader, csr)}
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
        nbytes = _cabi.mp_skipgram_workspace_bytes(loader.cfg, PREFETCH, B, form)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev) if nbytes else None
        out = None
        call = lambda: _cabi.mp_skipgram(loader.cfg, g_seeds, 0, 0, form=form, ws=ws, out=out)
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
                                  "workspace_bytes": nbytes, "lds_bytes": _cabi.mp_skipgram_lds_bytes(L, 4 if form == 1 else 8)
                                  if form < 3 else 0,
                                  "fraction_of_8TBps_roof": round(PREFETCH * slab_bytes / (med * 1e-3) / HBM_ROOF, 3)}
        del ws, out
    pos, _ = _cabi.mp_skipgram(loader.cfg, g_seeds, 0, 0)
    # R-MAT rows without out-edges end walks early: an ended walker makes no more look-ups, its windows are still written
    entry["pos_words_padded_share"] = round(float((pos == loader.dummy_idx).float().mean()), 3)
    del pos
    forms["flat_over_lds32_ms"] = round(forms["form3"]["ms_per_launch_median"] / forms["form1"]["ms_per_launch_median"], 2)
    forms["lds64_over_lds32_ms"] = round(forms["form2"]["ms_per_launch_median"] / forms["form1"]["ms_per_launch_median"], 2)
    res["loader"][key], res["forms"][key] = entry, forms
    print(json.dumps({key: {"loader": entry, "forms": forms}}), file=sys.stderr, flush=True)
    del loader, runs, csr
    torch.cuda.empty_cache()
print(json.dumps(res))
