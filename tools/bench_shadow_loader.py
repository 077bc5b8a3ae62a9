"""ShaDowKHopLoader on RMAT-24, depth 2, NUM_NEIGHBORS per hop, batch 1 024, prefetch 16, with a [2^24, 128] float32
feature matrix, in one process.  Prints one JSON line (the kept run: profiles/bench_shadow_loader.json):
  loader    ShaDowKHopLoader untimed and timed ("uniform"), NeighborLoader(unique=True, disjoint=True) and
            NeighborLoader(unique=True, induced=True) end to end in mini-batches/s -- ROUNDS passes each, interleaved,
            median, best and spread -- and the nodes / edges a mini-batch carries
  passes    tg_ns_induced_grouped_count and _emit alone on one launch of 16 batches behind tg_ns_homo_unique_grouped,
            untimed and timed (HIP events, ms per call), the scanned CSC entries and scanned entries/s, the chunks a
            mini-batch needs against the default capacity, the workspace
  ungrouped tg_ns_induced_count / _emit on one launch of 16 plainly deduplicated batches: ROUNDS interleaved medians and
            their spread (max / min).  With PARENT_LIB=<a libtchgeo_hip.so built from the parent commit> the same calls go
            to that library too, in the same process on the same lists, workspace and output arrays (so that placement is
            equal), interleaved with this one's in alternating order: csrc/ns_induced.hip is shared by the two pairs, and
            the ungrouped one must not have moved by more than its own spread."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tch-geometric_amd"))
from tch_geometric import _cabi  # noqa: E402
from tch_geometric.loader import NeighborLoader, ShaDowKHopLoader  # noqa: E402
from tch_geometric.transforms import Graph  # noqa: E402

dev = torch.device("cuda:0")
SCALE = int(os.environ.get("SCALE", "24"))
D = int(os.environ.get("DIM", "128"))
BATCHES = int(os.environ.get("BATCHES", "128"))        # mini-batches of a timed pass
ROUNDS = int(os.environ.get("ROUNDS", "3"))
K = int(os.environ.get("NUM_NEIGHBORS", "10"))
PARENT_LIB = os.environ.get("PARENT_LIB")
B, DEPTH, PREFETCH, WINDOW = 1024, 2, 16, (0, 500)
FAN = [K] * DEPTH
n = 1 << SCALE
row, col = _cabi.rmat_edges(SCALE, n * 16, 0x5EED0000 + SCALE, dev)
ei = torch.stack([row, col])
del row, col
seeds = _cabi.seed_batches(0xBA7C4, 0, BATCHES + PREFETCH, B, n, dev).reshape(-1)
gen = torch.Generator(device=dev)
gen.manual_seed(5)
edge_time = torch.randint(0, 1000, (ei.shape[1],), device=dev, generator=gen)
seed_time = torch.randint(500, 1500, (seeds.numel(),), device=dev, generator=gen)
res = {"config": "RMAT-%d, depth %d, %d neighbours per hop, batch %d, prefetch %d, %d f32 features, %d mini-batches per pass, "
                 "%d interleaved passes, time window %s" % (SCALE, DEPTH, K, B, PREFETCH, D, BATCHES, ROUNDS, list(WINDOW))}


def one_pass(loader):
    it = iter(loader)
    for _ in range(PREFETCH):                          # the first launch of the epoch is not steady state
        next(it)
    torch.cuda.synchronize()
    edges = nodes = nb = 0
    t0 = time.perf_counter()
    for b in it:
        edges += b.num_edges
        nodes += b.num_nodes
        nb += 1
        _ = (b.n_id, b.edge_index, b.x)
        if nb >= BATCHES:
            break
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del it
    return dt, nb, edges, nodes


def timed(fn, warm=3, reps=5, inner=5):
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


data = Graph(edge_index=ei, num_nodes=n)
data.x = torch.empty((n, D), dtype=torch.float32, device=dev)
data.x.view(torch.int32)[:] = 1
data_t = Graph(edge_index=ei, num_nodes=n)              # the timed loader's: its mini-batches also gather `time` per edge
data_t.x, data_t.time = data.x, edge_time
kw = dict(input_nodes=seeds, batch_size=B, prefetch=PREFETCH)
tkw = dict(time_attr="time", input_time=seed_time, temporal_strategy="uniform", time_window=WINDOW)
loaders = {"shadow": ShaDowKHopLoader(data, DEPTH, K, **kw),
           "shadow_timed_uniform": ShaDowKHopLoader(data_t, DEPTH, K, **kw, **tkw),
           "disjoint": NeighborLoader(data, FAN, unique=True, disjoint=True, **kw),
           "induced": NeighborLoader(data, FAN, unique=True, induced=True, **kw)}
for ld in loaders.values():                            # un-timed: slabs, pinned buffers, workspaces, the allocator's pools
    one_pass(ld)
passes = {k: [] for k in loaders}
for _ in range(ROUNDS):
    for k, ld in loaders.items():
        passes[k].append(one_pass(ld))
entry = {}
for k, ps in passes.items():
    rate = sorted(nb / dt for dt, nb, _, _ in ps)
    dt, nb, edges, nodes = ps[-1]
    entry[k] = {"mini_batches_per_s_median": round(statistics.median(rate), 1), "mini_batches_per_s_best": round(rate[-1], 1),
                "spread_max_over_min": round(rate[-1] / rate[0], 4),
                "nodes_per_mini_batch": round(nodes / nb), "edges_per_mini_batch": round(edges / nb)}
for k in ("disjoint", "induced"):
    entry["shadow_over_%s_median" % k] = round(entry["shadow"]["mini_batches_per_s_median"] /
                                               entry[k]["mini_batches_per_s_median"], 4)
entry["chunk_cap_after"] = {k: loaders[k].chunk_cap for k in ("shadow", "shadow_timed_uniform")}   # 0: the default never overflowed
res["loader"] = entry
print(json.dumps({"loader": entry}), file=sys.stderr, flush=True)
graph = loaders["shadow_timed_uniform"]._graph         # with timestamps (CSC order) and the u32 shadows
keep = loaders["shadow_timed_uniform"]                 # owns the arrays the view points into
ptrs = keep.col_ptrs
del loaders, data, data_t
torch.cuda.empty_cache()

# ---- the grouped passes alone, on one launch of the loader's shape
G = PREFETCH
out = _cabi.NsBatchedOut(G, B, FAN, dev)
first = seeds[:G * B].reshape(G, B).contiguous()
_cabi.ns_homo_batched(graph, first, FAN, 0, 0, out)
ug = _cabi.ns_homo_unique_grouped(out, G, n, with_inverse=False)
group_time = seed_time[:G * B].reshape(G, B).contiguous()
res["passes"] = {}
for name, tk in (("untimed", {}), ("timed", dict(group_time=group_time, time_window=WINDOW))):
    launch = _cabi.NsInducedGrouped(graph, ug.nodes, ug.group, ug.counts, 2, G, n, B, node_marks=ug.layer_nodes, **tk)
    launch.count()
    state = launch.state.cpu()
    chunks = launch.chunks_of(state)
    total = int(state[:G].sum())
    off = torch.cumsum(launch.n_edges, 0) - launch.n_edges
    rc = torch.empty((2, max(total, 1)), dtype=torch.int64, device=dev)
    eidx = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
    counts = ug.counts.cpu()
    scanned = 0
    for b in range(G):
        v = ug.nodes[b, :int(counts[b, 0])]
        scanned += int((ptrs[v + 1] - ptrs[v]).sum())
    p1 = [timed(launch.count) for _ in range(ROUNDS)]
    p2 = [timed(lambda: launch.emit(off, rc[0], rc[1], eidx)) for _ in range(ROUNDS)]
    need, least = _cabi.ns_induced_grouped_workspace_bytes(graph, out.cap_nodes, n, B, 0, G)
    res["passes"][name] = {
        "batches_per_call": G, "pitch_nodes": out.cap_nodes, "status": int(state[-1]), "nodes_per_call": int(counts[:, 0].sum()),
        "forest_edges_per_call": int(counts[:, 1].sum()), "induced_edges_per_call": total,
        "scanned_entries_per_call": scanned, "count": summary(p1), "emit": summary(p2),
        "count_G_scanned_entries_per_s": round(scanned / statistics.median(p1) / 1e6, 3),
        "emit_G_scanned_entries_per_s": round(scanned / statistics.median(p2) / 1e6, 3),
        "chunks_per_mini_batch_max": max(chunks), "chunks_per_mini_batch_mean": round(sum(chunks) / G),
        "default_chunk_cap": launch.chunk_cap, "workspace_bytes": need, "workspace_bytes_one_batch": least}
    del launch, rc, eidx
print(json.dumps({"passes": res["passes"]}), file=sys.stderr, flush=True)
del ug
torch.cuda.empty_cache()

# ---- the ungrouped pair on plainly deduplicated lists: this library and, when given, the parent commit's, interleaved
_cabi.ns_homo_batched(graph, first, FAN, 0, 0, out)
uniq = _cabi.ns_homo_unique(out, G, n, with_inverse=False)
libs = {"this": _cabi.lib}
if PARENT_LIB:
    libs["parent"] = C.CDLL(PARENT_LIB)


# one launch object and one set of flat outputs for every library: the ungrouped workspace layout is the same in both, so
# the calls touch the same addresses and a difference is the code's, not the placement's
ln = _cabi.NsInduced(graph, uniq.nodes, uniq.counts, 2, G, n, node_marks=uniq.layer_nodes)
ln.count()
total = int(ln.state.cpu()[:G].sum())
off = torch.cumsum(ln.n_edges, 0) - ln.n_edges
rc = torch.empty((2, total), dtype=torch.int64, device=dev)
eidx = torch.empty(total, dtype=torch.int64, device=dev)
stream = _cabi.stream_ptr(dev)


def pair_of(lib):
    """count / emit closures that call `lib`"""
    def count():
        _cabi.check(lib.tg_ns_induced_count(C.byref(ln.graph), C.byref(ln.struct), C.c_int64(G), C.c_int64(n), _cabi.ptr(ln.n_edges),
                                            _cabi.ptr(ln.edge_marks), _cabi.ptr(ln.status), _cabi.ptr(ln.ws),
                                            C.c_int64(ln.ws.numel() * 8), stream))

    def emit():
        _cabi.check(lib.tg_ns_induced_emit(C.byref(ln.graph), C.byref(ln.struct), C.c_int64(G), C.c_int64(n), _cabi.ptr(off),
                                           _cabi.ptr(rc[0]), _cabi.ptr(rc[1]), _cabi.ptr(eidx), _cabi.ptr(ln.ws),
                                           C.c_int64(ln.ws.numel() * 8), stream))
    return count, emit


pairs = {k: pair_of(lib) for k, lib in libs.items()}
outputs = {}
for k, (count, emit) in pairs.items():                 # what each library writes, from poisoned arrays
    ln.state.fill_(-7), rc.fill_(-7), eidx.fill_(-7)
    ln.state[-1:].zero_()
    count(), emit()
    outputs[k] = (ln.state.clone(), rc.clone(), eidx.clone())
ms = {k: {"count": [], "emit": []} for k in pairs}
for r in range(ROUNDS):
    for k in (list(pairs) if r % 2 == 0 else list(pairs)[::-1]):   # interleaved, the order alternating
        count, emit = pairs[k]
        ms[k]["count"].append(timed(count))
        ms[k]["emit"].append(timed(emit))
res["ungrouped"] = {k: {"count": summary(v["count"]), "emit": summary(v["emit"])} for k, v in ms.items()}
res["ungrouped"]["induced_edges_per_call"] = total
if PARENT_LIB:
    res["ungrouped"]["outputs_equal_parent"] = all(torch.equal(a, b) for a, b in zip(outputs["this"], outputs["parent"]))
    for p in ("count", "emit"):
        a, b = res["ungrouped"]["this"][p], res["ungrouped"]["parent"][p]
        ratio = a["ms_median_of_medians"] / b["ms_median_of_medians"]
        spread = max(a["spread_max_over_min"], b["spread_max_over_min"])
        res["ungrouped"]["%s_this_over_parent" % p] = round(ratio, 4)
        res["ungrouped"]["%s_within_spread" % p] = bool(1 / spread <= ratio <= spread)
print(json.dumps(res))
