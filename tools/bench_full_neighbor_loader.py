"""FullNeighborLoader and tg_ns_full_count / tg_ns_full_emit on RMAT-24 (16 edges per node, directed), in one process.
Prints one JSON line (the kept run: profiles/bench_full_neighbor_loader.json):
  pair         the pair alone on LISTS lists of LIST_NODES random distinct nodes (HIP events, ms per call; ROUNDS interleaved
               medians and their spread): count, emit (every emit behind an un-timed count: pass 2 consumes the workspace),
               scanned entries/s and the share of the 8 TB/s roof at the bytes the kernels ASK for per entry (stated in the
               output; the lines that move are more: every probe is a random line),
               against tg_ns_induced_count / _emit on the same lists, which scan the same columns (the yardstick), and
               against the torch composition it replaces, one list at a time, after their outputs compared equal word for word
  hub          one column of 1 000 003 entries against 62 501 columns of 16: count + emit of either frontier
  loader       FullNeighborLoader(num_layers=1), batch 1 024, prefetch 16, 128 f32 features, in mini-batches/s against
  composition  the torch composition per mini-batch plus the same gathers -- ROUNDS passes each, interleaved
  two_layers   num_layers=2 at a batch size small enough for the limits: nodes and edges per mini-batch."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tch-geometric_amd"))

SCALE = int(os.environ.get("SCALE", "24"))
D = int(os.environ.get("DIM", "128"))
LISTS = int(os.environ.get("LISTS", "16"))
LIST_NODES = int(os.environ.get("LIST_NODES", "1024"))
BATCH, PREFETCH = int(os.environ.get("BATCH", "1024")), int(os.environ.get("PREFETCH", "16"))
BATCHES = int(os.environ.get("BATCHES", "512"))              # mini-batches of a loader pass
SLOW_BATCHES = int(os.environ.get("SLOW_BATCHES", "32"))     # mini-batches of a composition pass
ROUNDS = int(os.environ.get("ROUNDS", "5"))
BATCH2 = int(os.environ.get("BATCH2", "16"))                 # num_layers=2
ROOF = 8e12
BYTES_COUNT = 2 * (4 + 4 + 4)          # two scans: the entry's 32-bit id, a 32-bit key and a 32-bit value of the table
BYTES_EMIT = 2 * (4 + 4 + 4) + 3 * 8   # two scans again, and three int64 words written per entry


def torch_full(ptrs, indices, v):
    """the composition the pair replaces, for ONE list -> (out_nodes, rows, cols, csc offsets); two read-backs (m, n_out)"""
    dev, n = v.device, v.numel()
    begin = ptrs[v]
    deg = ptrs[v + 1] - begin
    before = torch.cumsum(deg, 0) - deg
    m = int(deg.sum())
    cols = torch.repeat_interleave(torch.arange(n, device=dev), deg, output_size=m)
    e = torch.arange(m, device=dev) + (begin - before)[cols]
    src = indices[e]
    every = torch.cat([v, src])
    ids, inverse = torch.unique(every, return_inverse=True)
    first = torch.full((ids.numel(),), n + m, dtype=torch.int64, device=dev)
    first.scatter_reduce_(0, inverse, torch.arange(n + m, device=dev), "amin")
    new = torch.sort(first[first >= n]).values
    out = torch.cat([v, every[new]])
    pos = torch.where(first < n, first, n + torch.searchsorted(new, first))
    return out, pos[inverse[n:]], cols, e


def timed(fn, before=None, warm=2, reps=7):
    """ms of one fn() by HIP events, the median of `reps`; before() runs un-timed ahead of every fn()"""
    ms = []
    for r in range(warm + reps):
        if before is not None:
            before()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        if r >= warm:
            ms.append(ev[0].elapsed_time(ev[1]))
    return statistics.median(ms)


def summary(ms):
    return {"ms_median_of_medians": round(statistics.median(ms), 4), "ms_medians": [round(x, 4) for x in ms],
            "spread_max_over_min": round(max(ms) / min(ms), 4)}


def rates(ps):
    r = sorted(nb / dt for dt, nb in ps)
    return {"mini_batches_per_s_median": round(statistics.median(r), 1), "mini_batches_per_s_best": round(r[-1], 1),
            "spread_max_over_min": round(r[-1] / r[0], 4)}


def interleaved(run):
    ms = {k: [] for k in run}
    names = list(run)
    for r in range(ROUNDS):
        for k in (names if r % 2 == 0 else names[::-1]):
            ms[k].append(run[k]())
    return {k: summary(v) for k, v in ms.items()}


def sized(_cabi, graph, ptrs, lists, id_bound, dev):
    """an NsFull exactly large enough for `lists` (a [G, width] tensor), its flat inputs and its outputs' prefixes"""
    G, width = lists.shape
    deg = ptrs[lists + 1] - ptrs[lists]
    m = deg.sum(1)
    need = int((width + torch.clamp(m, max=id_bound)).max())
    chunks = int(((deg + 511) // 512).sum(1).max())
    op = _cabi.NsFull(graph, id_bound, width, need, max(chunks, 1), G, dev)
    return op, lists.reshape(-1).contiguous(), torch.arange(G + 1, device=dev) * width, int(m.sum())


def emitted(op, flat, node_ptr, dev):
    """count, the read-back, emit into exact arrays -> (nodes_out, triples [3, M], node_off, edge_off, host counts)"""
    n_nodes, n_edges, _, status = op.count(flat, node_ptr)
    host_n, host_m = n_nodes.tolist(), n_edges.tolist()
    assert int(status.cpu()[0]) == 0
    node_off, edge_off = torch.cumsum(n_nodes, 0) - n_nodes, torch.cumsum(n_edges, 0) - n_edges
    nodes_out = torch.empty(sum(host_n), dtype=torch.int64, device=dev)
    trip = torch.empty((3, sum(host_m)), dtype=torch.int64, device=dev)
    op.emit(node_off, edge_off, nodes_out, trip[0], trip[1], trip[2])
    return nodes_out, trip, node_off, edge_off, host_n, host_m


def main():
    from tch_geometric import _cabi
    from tch_geometric.loader import FullNeighborLoader
    from tch_geometric.transforms import Graph
    dev = torch.device("cuda:0")
    n = 1 << SCALE
    row, col = _cabi.rmat_edges(SCALE, n * 16, 0x5EED0000 + SCALE, dev)
    data = Graph(edge_index=torch.stack([row, col]), num_nodes=n)
    del row, col
    data.x = torch.empty((n, D), dtype=torch.float32, device=dev)
    data.x.view(torch.int32)[:] = 1
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    inputs = torch.randperm(n, device=dev, generator=gen)[:max(BATCHES, LISTS) * max(BATCH, LIST_NODES)]
    loader = FullNeighborLoader(data, 1, input_nodes=inputs[:BATCHES * BATCH], batch_size=BATCH, prefetch=PREFETCH, device=dev)
    graph, ptrs, indices, perm = loader._graph, loader.col_ptrs, loader.row_indices, loader.perm
    E = indices.numel()
    res = {"config": "RMAT-%d, %d directed edges, longest column %d; %d lists of %d random distinct nodes for the pair; loader: "
                     "batch %d, prefetch %d, %d f32 features, %d mini-batches per loader pass, %d per composition pass, %d "
                     "interleaved passes" % (SCALE, E, int((ptrs[1:] - ptrs[:-1]).max()), LISTS, LIST_NODES, BATCH, PREFETCH, D,
                                             BATCHES, SLOW_BATCHES, ROUNDS)}

    # ---- the pair alone, against the induced pair on the same lists and against the torch composition
    lists = inputs[:LISTS * LIST_NODES].view(LISTS, LIST_NODES)
    op, flat, node_ptr, scanned = sized(_cabi, graph, ptrs, lists, n, dev)
    nodes_out, trip, node_off, edge_off, host_n, host_m = emitted(op, flat, node_ptr, dev)
    equal, n_at, m_at = True, 0, 0
    for b in range(LISTS):                                 # word for word, before any time is taken
        out, rows, cols, e = torch_full(ptrs, indices, lists[b])
        equal = equal and torch.equal(out, nodes_out[n_at:n_at + host_n[b]])
        equal = equal and torch.equal(torch.stack([rows, cols, e]), trip[:, m_at:m_at + host_m[b]])
        n_at, m_at = n_at + host_n[b], m_at + host_m[b]
    counts = torch.full((LISTS,), LIST_NODES, dtype=torch.int64, device=dev)
    ind = _cabi.NsInduced(graph, lists.contiguous(), counts, 1, LISTS, n)
    ind.count()
    m_ind = ind.n_edges.tolist()
    ind_off = torch.cumsum(ind.n_edges, 0) - ind.n_edges
    ind_trip = torch.empty((3, sum(m_ind)), dtype=torch.int64, device=dev)
    count = lambda: op.count(flat, node_ptr)
    emit = lambda: op.emit(node_off, edge_off, nodes_out, trip[0], trip[1], trip[2])

    def both():
        count()
        emit()

    def composition_lists():
        for b in range(LISTS):
            torch_full(ptrs, indices, lists[b])

    pair = interleaved({"full_count": lambda: timed(count),
                        "full_emit": lambda: timed(emit, before=count),
                        "full_count_and_emit": lambda: timed(both),
                        "induced_count": lambda: timed(ind.count),
                        "induced_emit": lambda: timed(lambda: ind.emit(ind_off, ind_trip[0], ind_trip[1], ind_trip[2])),
                        "torch_composition": lambda: timed(composition_lists, warm=1, reps=3)})
    for k, nbytes in (("full_count", BYTES_COUNT), ("full_emit", BYTES_EMIT), ("induced_count", None), ("induced_emit", None)):
        per_s = scanned / (pair[k]["ms_median_of_medians"] * 1e-3)
        pair[k]["scanned_entries_per_s"] = round(per_s, 0)
        if nbytes:
            pair[k]["bytes_asked_per_entry"] = nbytes
            pair[k]["share_of_8TBps_roof"] = round(per_s * nbytes / ROOF, 4)
    ms = lambda k: pair[k]["ms_median_of_medians"]
    pair.update({"lists": LISTS, "nodes_per_list": LIST_NODES, "scanned_entries_per_call": scanned,
                 "out_nodes_per_call": sum(host_n), "induced_edges_per_call": sum(m_ind),
                 "outputs_equal_torch_composition": bool(equal),
                 "workspace_bytes_full": _cabi.ns_full_workspace_bytes(graph, n, op.max_nodes, op.node_cap, op.chunk_cap, LISTS)[0],
                 "workspace_bytes_induced": _cabi.ns_induced_workspace_bytes(graph, LIST_NODES, n, LISTS)[0],
                 "count_full_over_induced": round(ms("full_count") / ms("induced_count"), 3),
                 "emit_full_over_induced": round(ms("full_emit") / ms("induced_emit"), 3),
                 "composition_over_full_pair": round(ms("torch_composition") / ms("full_count_and_emit"), 3)})
    res["pair"] = pair
    print(json.dumps(pair), file=sys.stderr, flush=True)
    del op, ind, ind_trip, trip, nodes_out

    # ---- the hub check: one column of 1 000 003 entries against 62 501 columns of 16
    n_hub, long, short = 1 << 20, 1000003, 62501
    deg = torch.zeros(n_hub, dtype=torch.int64, device=dev)
    deg[0], deg[1:short + 1] = long, 16
    hptrs = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(deg, 0)])
    hidx = torch.randint(0, n_hub, (int(hptrs[-1]),), device=dev, generator=gen)
    hgraph = _cabi.graph_view(hptrs, hidx, indices32=hidx.to(torch.int32), ptrs32=hptrs.to(torch.int32))
    hub = {}
    runs = {}
    for name, frontier in (("one_column_of_1000003", torch.zeros((1, 1), dtype=torch.int64, device=dev)),
                           ("62501_columns_of_16", torch.arange(1, short + 1, device=dev).view(1, -1))):
        hop, hflat, hnode_ptr, hm = sized(_cabi, hgraph, hptrs, frontier, n_hub, dev)
        hnodes, htrip, hnoff, heoff, hn, _ = emitted(hop, hflat, hnode_ptr, dev)
        hub[name] = {"entries": hm, "out_nodes": sum(hn)}

        def both_hub(hop=hop, a=(hflat, hnode_ptr), o=(hnoff, heoff, hnodes, htrip)):
            hop.count(*a)
            hop.emit(o[0], o[1], o[2], o[3][0], o[3][1], o[3][2])
        runs[name] = lambda f=both_hub: timed(f)
    for name, s in interleaved(runs).items():
        hub[name]["count_and_emit"] = s
        hub[name]["entries_per_s"] = round(hub[name]["entries"] / (s["ms_median_of_medians"] * 1e-3), 0)
    hub["hub_over_flat_ms"] = round(hub["one_column_of_1000003"]["count_and_emit"]["ms_median_of_medians"] /
                                    hub["62501_columns_of_16"]["count_and_emit"]["ms_median_of_medians"], 3)
    res["hub"] = hub
    print(json.dumps(hub), file=sys.stderr, flush=True)
    del hgraph, hptrs, hidx, runs

    # ---- the loader against the composition
    def loader_pass():
        torch.cuda.synchronize()
        nb = 0
        t0 = time.perf_counter()
        for sb in loader.super_batches():
            _ = (sb.n_id, sb.layers[0]["edge_index"], sb.layers[0]["e_id"], sb.node_attrs["x"])
            nb += len(sb)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, nb

    def composition_pass(r):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start = (r * SLOW_BATCHES) % max(1, BATCHES - SLOW_BATCHES + 1)
        for j in range(start, start + SLOW_BATCHES):
            out, rows, cols, e = torch_full(ptrs, indices, inputs[j * BATCH:(j + 1) * BATCH])
            _ = (_cabi.gather_rows(data.x, out)[0], perm[e])
        torch.cuda.synchronize()
        return time.perf_counter() - t0, SLOW_BATCHES

    loader_pass()                                          # un-timed: the kept capacities, the workspace, the allocator's pools
    composition_pass(0)
    growths = loader.growths
    passes = {"loader": [], "composition": []}
    for r in range(ROUNDS):
        passes["loader"].append(loader_pass())
        passes["composition"].append(composition_pass(r + 1))
    res["loader"], res["composition"] = rates(passes["loader"]), rates(passes["composition"])
    res["loader"]["growths_first_pass"], res["loader"]["growths_timed_passes"] = growths, loader.growths - growths
    res["loader_over_composition_median"] = round(res["loader"]["mini_batches_per_s_median"] /
                                                  res["composition"]["mini_batches_per_s_median"], 3)

    # ---- two layers at a small batch: what a mini-batch holds
    two = FullNeighborLoader(data, 2, input_nodes=inputs[:64 * BATCH2], batch_size=BATCH2, prefetch=4, device=dev)
    sizes = [(mb.blocks[1].num_src_nodes, mb.blocks[1].num_edges, mb.num_nodes, mb.blocks[0].num_edges) for mb in two]
    col = lambda i: [s[i] for s in sizes]
    res["two_layers"] = {"batch_size": BATCH2, "mini_batches": len(sizes),
                         "layer0_nodes_mean": round(statistics.mean(col(0)), 1), "layer0_edges_mean": round(statistics.mean(col(1)), 1),
                         "layer1_nodes_mean": round(statistics.mean(col(2)), 1), "layer1_nodes_max": max(col(2)),
                         "layer1_edges_mean": round(statistics.mean(col(3)), 1), "layer1_edges_max": max(col(3)),
                         "growths": two.growths}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
