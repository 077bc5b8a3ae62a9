"""GraphSAINTNodeLoader and GraphSAINTEdgeLoader on RMAT-24 with reverse edges (symmetric, so the edge sampler takes the CSC
and its list for both sides), prefetch 16, with a [2^24, 128] float32 feature matrix, in one process.  Prints one JSON line
(the kept run: profiles/bench_saint_ne_loader.json):
  node_nodes / edge_nodes   tg_saint_node_nodes at B = 6 000 and tg_saint_edge_nodes at B = 4 000 alone on one launch of 16
               mini-batches, by form where it fits (HIP events, ms per call; ROUNDS interleaved medians and their spread),
               against the torch composition of the same step, one mini-batch at a time: randint (node) or the mixture by
               hand (edge), the gathers, torch.unique and the re-sort to first-occurrence order.  The composition is timed
               on torch's own random numbers; fed the kernel's picks (Philox restated in torch) it must produce the
               kernel's words, which is asserted here
  stages       the other steps of the same launch alone: tg_ns_induced_count, tg_ns_induced_emit, the feature gather, and
               the share of the launch spent in the two induced scans
  loaders      both loaders end to end in mini-batches/s beside GraphSAINTRandomWalkLoader (6 000 roots, T = 2) in the same
               run -- ROUNDS passes each, interleaved, median, best and spread."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tch-geometric_amd"))
from tch_geometric import _cabi  # noqa: E402
from tch_geometric.loader import GraphSAINTEdgeLoader, GraphSAINTNodeLoader, GraphSAINTRandomWalkLoader  # noqa: E402
from tch_geometric.transforms import Graph  # noqa: E402

dev = torch.device("cuda:0")
SCALE = int(os.environ.get("SCALE", "24"))
D = int(os.environ.get("DIM", "128"))
BATCHES = int(os.environ.get("BATCHES", "64"))         # mini-batches of a loader pass
ROUNDS = int(os.environ.get("ROUNDS", "3"))
PREFETCH, SEED = 16, 7
B_NODE, B_EDGE, B_WALK, T_WALK = 6000, 4000, 6000, 2
TAG_NODE, TAG_EDGE = 16, 17
n = 1 << SCALE
row, col = _cabi.rmat_edges(SCALE, n * 16, 0x5EED0000 + SCALE, dev)
ei = torch.stack([torch.cat([row, col]), torch.cat([col, row])])
del row, col
data = Graph(edge_index=ei, num_nodes=n)
data.x = torch.empty((n, D), dtype=torch.float32, device=dev)
data.x.view(torch.int32)[:] = 1
res = {"config": "RMAT-%d with reverse edges (%d edges), prefetch %d, %d f32 features, %d mini-batches per loader pass, "
                 "%d interleaved passes" % (SCALE, ei.shape[1], PREFETCH, D, BATCHES, ROUNDS)}


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


# ---- the kernel's picks in torch: Philox4x32-10 and floor(x * n / 2^64) on 32-bit words held in int64 -------------------------
M32 = 0xFFFFFFFF


def mulhilo(a, b):
    """a: a 32-bit constant, b: int64 tensor of 32-bit words -> (high, low) words of the product"""
    lo = (a & 0xFFFF) * b                                  # < 2^48
    hi = (a >> 16) * b                                     # < 2^48
    full_lo = (lo + ((hi & 0xFFFF) << 16))                 # < 2^49: the low 48 bits and a carry
    return ((hi >> 16) + (full_lo >> 32)) & M32, full_lo & M32


def philox(c, k0, k1):
    c0, c1, c2, c3 = c
    for _ in range(10):
        h0, l0 = mulhilo(0xD2511F53, c0)
        h1, l1 = mulhilo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def slot_words(call_id, B, tag):
    """the four words of slot i's draw (SEED, call_id, tag, id = i, 0, 0) -> int64 [4, B]"""
    z = torch.zeros(1, dtype=torch.int64, device=dev)
    key = philox((z + (call_id & M32), z + (call_id >> 32), z + tag, z + 0x74636867), SEED & M32, SEED >> 32)
    i = torch.arange(B, dtype=torch.int64, device=dev)
    return philox((torch.zeros_like(i), torch.zeros_like(i), i, torch.zeros_like(i)), key[0], key[1])


def bounded(w_lo, w_hi, m):
    """floor((w_hi << 32 | w_lo) * m / 2^64), m < 2^31 (a number or a tensor)"""
    return (w_hi * m + ((w_lo * m) >> 32)) >> 32


def first_occurrence(flat):
    """the distinct values of `flat` ordered by first position: unique plus the re-sort"""
    uniq, inv = torch.unique(flat, return_inverse=True)
    first = torch.full((uniq.numel(),), flat.numel(), dtype=torch.int64, device=dev)
    first.scatter_reduce_(0, inv, torch.arange(flat.numel(), device=dev), "amin")
    return uniq[torch.argsort(first)]


def compose_node(indices, B, call_id=None):
    e = torch.randint(0, indices.numel(), (B,), device=dev) if call_id is None else \
        bounded(*slot_words(call_id, B, TAG_NODE)[:2], indices.numel())
    return first_occurrence(indices[e])


def compose_edge(ptrs, indices, cols, B, call_id=None):
    """both sides are the CSC and its list (a symmetric graph)"""
    m = 2 * cols.numel()
    if call_id is None:
        t = torch.randint(0, m, (B,), device=dev)
    else:
        w = slot_words(call_id, B, TAG_EDGE)
        t = bounded(w[0], w[1], m)
    side = t >= cols.numel()
    major = cols[torch.where(side, t - cols.numel(), t)]
    b, e = ptrs[major], ptrs[major + 1]
    k = (torch.rand(B, device=dev) * (e - b)).long() if call_id is None else bounded(w[2], w[3], e - b)
    other = indices[b + k]
    return first_occurrence(torch.cat([torch.where(side, major, other), torch.where(side, other, major)]))


loaders = {
    "node_B%d" % B_NODE: GraphSAINTNodeLoader(data, B_NODE, BATCHES, prefetch=PREFETCH, seed=SEED, device=dev),
    "edge_B%d" % B_EDGE: GraphSAINTEdgeLoader(data, B_EDGE, BATCHES, prefetch=PREFETCH, seed=SEED, symmetric=True, device=dev),
    "walk_B%d_T%d" % (B_WALK, T_WALK): GraphSAINTRandomWalkLoader(data, B_WALK, T_WALK, BATCHES, prefetch=PREFETCH, seed=SEED,
                                                                  symmetric=True, device=dev)}
for ld in loaders.values():                            # un-timed: slabs, pinned buffers, workspaces, the allocator's pools
    loader_pass(ld)
passes = {k: [] for k in loaders}
for r in range(ROUNDS):
    for k, ld in loaders.items():
        passes[k].append(loader_pass(ld))
res["loaders"] = {k: rates(ps) for k, ps in passes.items()}
print(json.dumps(res["loaders"]), file=sys.stderr, flush=True)

# ---- the fused step alone against the composition, and the other steps of the same launch
G = PREFETCH
for key, B, P in (("node_nodes", B_NODE, B_NODE), ("edge_nodes", B_EDGE, 2 * B_EDGE)):
    ld = loaders["node_B%d" % B_NODE] if key == "node_nodes" else loaders["edge_B%d" % B_EDGE]
    nodes = torch.empty((G, P), dtype=torch.int64, device=dev)
    counts = torch.zeros(G, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    auto = _cabi.saint_ne_form(P)[0]
    forms = [f for f in (1, 2) if f == 2 or auto == 1]
    ws = {f: (torch.empty(_cabi.saint_ne_workspace_bytes(G, P, f)[0] // 8 + 1, dtype=torch.int64, device=dev) if f == 2 else None)
          for f in forms}
    if key == "node_nodes":
        run = {f: (lambda f=f: _cabi.saint_node_nodes(ld._graph, B, G, SEED, 0, id_bound=n, form=f, ws=ws[f], out=(nodes, counts),
                                                      status=status)) for f in forms}
        compose = lambda c=None: compose_node(ld.row_indices, B, c)
    else:
        run = {f: (lambda f=f: _cabi.saint_edge_nodes(ld._graph, ld.cols, ld._graph, ld.cols, B, G, SEED, 0, id_bound=n, form=f,
                                                      ws=ws[f], out=(nodes, counts), status=status)) for f in forms}
        compose = lambda c=None: compose_edge(ld.col_ptrs, ld.row_indices, ld.cols, B, c)
    outs = {}
    for f in forms:
        nodes.fill_(-7)
        run[f]()
        outs[f] = (nodes.clone(), counts.clone())
    for g in range(G):                                 # the composition on the kernel's picks writes the kernel's words
        want = compose(g)
        assert int(outs[forms[0]][1][g]) == want.numel() and torch.equal(outs[forms[0]][0][g, :want.numel()], want), (key, g)
    composition = lambda: [compose() for _ in range(G)]
    ms = {f: [] for f in forms}
    ms["composition"] = []
    order = forms + ["composition"]
    for r in range(ROUNDS):
        for f in (order if r % 2 == 0 else order[::-1]):
            ms[f].append(timed(run[f] if f != "composition" else composition))
    entry = {"auto_form": auto, "positions": P, "batches_per_call": G, "nodes_per_call": int(counts.sum()),
             "workspace_bytes_flat": _cabi.saint_ne_workspace_bytes(G, P, 2)[0], "status": int(status.item()),
             "composition_on_the_kernels_picks_writes_equal_words": True,
             "torch_composition": summary(ms["composition"])}
    for f in forms:
        entry["form_%d" % f] = summary(ms[f])
    if len(forms) == 2:
        entry["forms_write_equal_words"] = all(torch.equal(a, b) for a, b in zip(outs[1], outs[2]))
    fused = entry["form_%d" % (auto if auto in forms else 2)]["ms_median_of_medians"]
    entry["composition_over_auto_form"] = round(entry["torch_composition"]["ms_median_of_medians"] / fused, 2)
    res[key] = entry
    ind = _cabi.NsInduced(ld._graph, nodes, counts, 1, G, n)
    ind.count()
    n_edges = ind.state.cpu()[:G].tolist()
    total = sum(n_edges)
    off = torch.cumsum(ind.n_edges, 0) - ind.n_edges
    rc = torch.empty((2, max(total, 1)), dtype=torch.int64, device=dev)
    eidx = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
    n_id = _cabi.compact_rows(nodes, counts, int(counts.sum()))
    stages = {
        "induced_edges_per_call": total,
        "scanned_entries_per_call": int((ld.col_ptrs[n_id + 1] - ld.col_ptrs[n_id]).sum()),
        "induced_count": summary([timed(ind.count) for _ in range(ROUNDS)]),
        "induced_emit": summary([timed(lambda: ind.emit(off, rc[0], rc[1], eidx)) for _ in range(ROUNDS)]),
        "gather_x": summary([timed(lambda: _cabi.gather_rows(data.x, n_id)) for _ in range(ROUNDS)])}
    scans = stages["induced_count"]["ms_median_of_medians"] + stages["induced_emit"]["ms_median_of_medians"]
    stages["launch_ms"] = round(fused + scans + stages["gather_x"]["ms_median_of_medians"], 4)
    stages["induced_scans_share_of_launch"] = round(scans / stages["launch_ms"], 4)
    res[key]["stages"] = stages
    del ind, rc, eidx, ws
print(json.dumps(res))
