"""GraphSAINTRandomWalkLoader on RMAT-24 with reverse edges (symmetric, so the walks run on the CSC), prefetch 16, with a
[2^24, 128] float32 feature matrix, in one process, at two shapes: batch 6 000 x walk length 2 (PyG's usual shape; 18 000
positions: the flat form) and batch 2 000 x walk length 4 (10 000 positions: the LDS form).  Prints one JSON line (the kept
run: profiles/bench_saint_loader.json):
  rw_nodes     tg_saint_rw_nodes alone on one launch of 16 mini-batches, by form (HIP events, ms per call; ROUNDS
               interleaved medians and their spread), the distinct nodes it lists and the workspace
  stages       the other steps of the same launch alone: tg_ns_induced_count, tg_ns_induced_emit, the feature gather
  loader       the loader end to end in mini-batches/s, against
  composition  the per-mini-batch composition it replaces: _cabi.random_walk, torch.unique, transforms.induced_subgraph and
               the gathers, one mini-batch at a time -- ROUNDS passes each, interleaved, median, best and spread."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tch-geometric_amd"))
from tch_geometric import _cabi  # noqa: E402
from tch_geometric.loader import GraphSAINTRandomWalkLoader  # noqa: E402
from tch_geometric.transforms import Graph, induced_subgraph  # noqa: E402

dev = torch.device("cuda:0")
SCALE = int(os.environ.get("SCALE", "24"))
D = int(os.environ.get("DIM", "128"))
BATCHES = int(os.environ.get("BATCHES", "64"))         # mini-batches of a loader pass
SLOW_BATCHES = int(os.environ.get("SLOW_BATCHES", "16"))   # mini-batches of a composition pass
ROUNDS = int(os.environ.get("ROUNDS", "3"))
PREFETCH, SEED = 16, 7
SHAPES = {"B6000_T2": (6000, 2), "B2000_T4": (2000, 4)}
n = 1 << SCALE
row, col = _cabi.rmat_edges(SCALE, n * 16, 0x5EED0000 + SCALE, dev)
ei = torch.stack([torch.cat([row, col]), torch.cat([col, row])])
del row, col
data = Graph(edge_index=ei, num_nodes=n)
data.x = torch.empty((n, D), dtype=torch.float32, device=dev)
data.x.view(torch.int32)[:] = 1
res = {"config": "RMAT-%d with reverse edges (%d edges), prefetch %d, %d f32 features, %d mini-batches per loader pass, %d per "
                 "composition pass, %d interleaved passes" % (SCALE, ei.shape[1], PREFETCH, D, BATCHES, SLOW_BATCHES, ROUNDS)}


def timed(fn, warm=2, reps=5, inner=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(inner):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]) / inner)
    return statistics.median(ms)


def summary(ms):
    return {"ms_median_of_medians": round(statistics.median(ms), 4), "ms_medians": [round(x, 4) for x in ms],
            "spread_max_over_min": round(max(ms) / min(ms), 4)}


def rates(ps):
    r = sorted(nb / dt for dt, nb in ps)
    return {"mini_batches_per_s_median": round(statistics.median(r), 1), "mini_batches_per_s_best": round(r[-1], 1),
            "spread_max_over_min": round(r[-1] / r[0], 4)}


def loader_pass(loader):
    torch.cuda.synchronize()
    nb = 0
    t0 = time.perf_counter()
    for sb in loader.super_batches():
        _ = (sb.n_id, sb.edge_index, sb.node_attrs["x"])
        nb += len(sb)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, nb


def composition_pass(loader, B, T, call_id0):
    """what a caller composed per mini-batch before: walk matrix, torch.unique (sorts, synchronises, reads a size back),
    the induced transform (one more read-back), the gathers"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for j in range(SLOW_BATCHES):
        c = call_id0 + j
        roots = _cabi.seed_batches(SEED, c, 1, B, n, dev)[0]
        walks = _cabi.random_walk(loader._walk_graph, roots, T, 1.0, 1.0, SEED, c)
        flat = walks.t().reshape(-1)
        nodes = torch.unique(flat[flat >= 0])
        rows, cols, e = induced_subgraph(nodes, loader.col_ptrs, loader.row_indices)
        _ = (_cabi.gather_rows(data.x, nodes)[0], _cabi.gather_rows(loader.perm, e)[0])
    torch.cuda.synchronize()
    return time.perf_counter() - t0, SLOW_BATCHES


loaders = {k: GraphSAINTRandomWalkLoader(data, B, T, BATCHES, prefetch=PREFETCH, seed=SEED, symmetric=True, device=dev)
           for k, (B, T) in SHAPES.items()}
for k, ld in loaders.items():                          # un-timed: slabs, pinned buffers, workspaces, the allocator's pools
    loader_pass(ld)
    composition_pass(ld, *SHAPES[k], 1 << 40)
passes = {k: {"loader": [], "composition": []} for k in loaders}
for r in range(ROUNDS):
    for k, ld in loaders.items():
        passes[k]["loader"].append(loader_pass(ld))
        passes[k]["composition"].append(composition_pass(ld, *SHAPES[k], (1 << 40) + (r + 1) * SLOW_BATCHES))
for k, ps in passes.items():
    entry = {"loader": rates(ps["loader"]), "composition": rates(ps["composition"])}
    entry["loader_over_composition_median"] = round(entry["loader"]["mini_batches_per_s_median"] /
                                                    entry["composition"]["mini_batches_per_s_median"], 3)
    res[k] = entry
print(json.dumps({k: res[k] for k in loaders}), file=sys.stderr, flush=True)

# ---- the steps of one launch alone
for k, (B, T) in SHAPES.items():
    ld = loaders[k]
    G, P = PREFETCH, _cabi.saint_rw_capacity(B, T)
    roots = _cabi.seed_batches(SEED, 0, G, B, n, dev)
    nodes = torch.empty((G, P), dtype=torch.int64, device=dev)
    counts = torch.zeros(G, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    auto = _cabi.saint_rw_form(B, T)[0]
    forms = [f for f in (1, 2) if f == 2 or auto == 1]
    ws = {f: (torch.empty(_cabi.saint_rw_workspace_bytes(G, B, T, f)[0] // 8 + 1, dtype=torch.int64, device=dev) if f == 2 else None)
          for f in forms}
    run = {f: (lambda f=f: _cabi.saint_rw_nodes(ld._walk_graph, roots, T, SEED, 0, form=f, ws=ws[f], out=(nodes, counts),
                                                status=status)) for f in forms}
    ms = {f: [] for f in forms}
    outs = {}
    for f in forms:
        nodes.fill_(-7)
        run[f]()
        outs[f] = (nodes.clone(), counts.clone())
    for r in range(ROUNDS):
        for f in (forms if r % 2 == 0 else forms[::-1]):
            ms[f].append(timed(run[f]))
    entry = {"auto_form": auto, "positions": P, "batches_per_call": G, "nodes_per_call": int(counts.sum()),
             "workspace_bytes_flat": _cabi.saint_rw_workspace_bytes(G, B, T, 2)[0], "status": int(status.item())}
    for f in forms:
        entry["form_%d" % f] = summary(ms[f])
    if len(forms) == 2:
        entry["forms_write_equal_words"] = all(torch.equal(a, b) for a, b in zip(outs[1], outs[2]))
        entry["form_1_over_form_2"] = round(entry["form_1"]["ms_median_of_medians"] / entry["form_2"]["ms_median_of_medians"], 4)
    res[k]["rw_nodes"] = entry
    ind = _cabi.NsInduced(ld._graph, nodes, counts, 1, G, n)
    ind.count()
    n_edges = ind.state.cpu()[:G].tolist()
    total = sum(n_edges)
    off = torch.cumsum(ind.n_edges, 0) - ind.n_edges
    rc = torch.empty((2, max(total, 1)), dtype=torch.int64, device=dev)
    eidx = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
    n_id = _cabi.compact_rows(nodes, counts, int(counts.sum()))
    scanned = int((ld.col_ptrs[n_id + 1] - ld.col_ptrs[n_id]).sum())
    res[k]["stages"] = {
        "induced_edges_per_call": total, "scanned_entries_per_call": scanned,
        "induced_count": summary([timed(ind.count) for _ in range(ROUNDS)]),
        "induced_emit": summary([timed(lambda: ind.emit(off, rc[0], rc[1], eidx)) for _ in range(ROUNDS)]),
        "gather_x": summary([timed(lambda: _cabi.gather_rows(data.x, n_id)) for _ in range(ROUNDS)])}
    del ind, rc, eidx, ws
print(json.dumps(res))
