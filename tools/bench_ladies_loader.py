"""LADIESLoader and tg_ladies_count / tg_ladies_emit on RMAT-24 (16 edges per node, directed), in one process.  Prints one
JSON line (the kept run: profiles/bench_ladies_loader.json):
  pair     the pair alone on LISTS lists of LIST_NODES random distinct nodes at s = 512 (HIP events, ms per call; ROUNDS
           interleaved medians and their spread): count, emit, against tg_ns_full_count / _emit on the same frontiers in the
           same process, unchanged (the yardstick: the layer-wise pair scans the columns five times to their four and draws)
  hub      one column of 1 000 003 entries against 62 501 columns of 16: count + emit of either frontier
  loader   LADIESLoader(num_samples=[512, 512]), batch 1 024, prefetch 16, 128 f32 features: mini-batches/s and distinct nodes
           per mini-batch, beside NeighborLoader([15, 10], unique=True) and labor=True in the same run.
           and against the torch composition that writes the same words, one list at a time, after every word (edge_weight as
           bits) compared equal.  The composition is handed its picks t_j (tests/helpers_ladies.draw_t on the host, from the
           total S it agrees on with the kernel): Philox and the 128-bit product are not what a composition would be made of
The timing helpers and the exact sizing of the full-neighbour pair are tools/bench_full_neighbor_loader.py's."""
import json
import os
import statistics
import sys
import time

import torch

import bench_full_neighbor_loader as bf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
SCALE, D, LISTS, LIST_NODES = bf.SCALE, bf.D, bf.LISTS, bf.LIST_NODES
BATCH, PREFETCH, ROUNDS = bf.BATCH, bf.PREFETCH, bf.ROUNDS
BATCHES = int(os.environ.get("BATCHES", "256"))              # mini-batches of a loader pass
S = int(os.environ.get("SAMPLES", "512"))


def _find(keys, values, queries):
    """values[i] where queries equal keys[i] (keys distinct), -1 elsewhere"""
    if not keys.numel():
        return torch.full_like(queries, -1)
    ks, ki = torch.sort(keys)
    at = torch.searchsorted(ks, queries).clamp(max=ks.numel() - 1)
    return torch.where(ks[at] == queries, values[ki[at]], torch.full_like(queries, -1))


def torch_ladies(ptrs, indices, v, s, t):
    """the composition the pair replaces, for ONE list of distinct nodes under the picks t [s] (int64) -> (out_nodes,
    node_count, node_weight, rows, cols, csc offsets, edge_weight, S, n_cand); one read-back (m)"""
    dev, n = v.device, v.numel()
    arange = lambda k: torch.arange(k, device=dev)
    begin = ptrs[v]
    deg = ptrs[v + 1] - begin
    before = torch.cumsum(deg, 0) - deg
    m = int(deg.sum())
    cols = torch.repeat_interleave(arange(n), deg, output_size=m)
    e = arange(m) + (begin - before)[cols]
    src = indices[e]
    d = deg.clamp(min=1)
    q = torch.clamp((1 << 40) // (d * d), min=1)[cols]
    ids, inverse = torch.unique(src, return_inverse=True)
    nc = ids.numel()
    first = torch.full((nc,), m, dtype=torch.int64, device=dev).scatter_reduce_(0, inverse, arange(m), "amin")
    order = torch.argsort(first)                           # candidates by first occurrence
    rank = torch.empty_like(order)
    rank[order] = arange(nc)
    cand, inv = ids[order], rank[inverse]
    W = torch.zeros(nc, dtype=torch.int64, device=dev).scatter_add_(0, inv, q)
    S = W.sum()
    sel = torch.searchsorted(torch.cumsum(W, 0) - W, t, right=True) - 1
    c = torch.bincount(sel, minlength=nc)
    first_slot = torch.full((nc,), s, dtype=torch.int64, device=dev).scatter_reduce_(0, sel, arange(s), "amin")
    pos = _find(v, arange(n), cand)                        # a candidate that is a frontier node: its position
    new = torch.nonzero((c > 0) & (pos < 0)).view(-1)
    new = new[torch.argsort(first_slot[new])]              # the others, by their first selecting slot
    pos[new] = n + arange(new.numel())
    who = torch.cat([_find(cand, arange(nc), v), new])     # the candidate at every position of out_nodes
    zero = torch.zeros_like(who)
    seen = who >= 0
    node_count = torch.where(seen, c[who.clamp(min=0)], zero)
    node_weight = torch.where(seen, W[who.clamp(min=0)], zero)
    kept = c[inv] > 0
    u, kc = inv[kept], cols[kept]
    ew = ((c[u].double() * S.double()) / (float(s) * W[u].double())) * (1.0 / deg.double())[kc]
    return torch.cat([v, cand[new]]), node_count, node_weight, pos[u], kc, e[kept], ew.float(), S, nc


def ladies_sized(ops, graph, ptrs, lists, id_bound, s, dev):
    """a Ladies exactly large enough for `lists` (a [G, width] tensor), its flat inputs"""
    G, width = lists.shape
    deg = ptrs[lists + 1] - ptrs[lists]
    m = deg.sum(1)
    need = int((width + torch.clamp(m, max=id_bound)).max())
    chunks = int(((deg + 511) // 512).sum(1).max())
    op = ops.Ladies(graph, id_bound, width, need, max(chunks, 1), s, G, dev)
    return op, lists.reshape(-1).contiguous(), torch.arange(G + 1, device=dev) * width, int(m.sum())


def ladies_outputs(op, flat, node_ptr, dev):
    n_nodes, n_edges, n_cand, total, _, status = op.count(flat, node_ptr, 7, 0)
    host_n, host_m = n_nodes.tolist(), n_edges.tolist()
    assert int(status.cpu()[0]) == 0
    node_off, edge_off = torch.cumsum(n_nodes, 0) - n_nodes, torch.cumsum(n_edges, 0) - n_edges
    per_node = torch.empty((3, sum(host_n)), dtype=torch.int64, device=dev)
    trip = torch.empty((3, max(sum(host_m), 1)), dtype=torch.int64, device=dev)
    ew = torch.empty(max(sum(host_m), 1), dtype=torch.float32, device=dev)
    emit = lambda: op.emit(node_off, edge_off, per_node[0], per_node[1], per_node[2], trip[0], trip[1], trip[2], ew)
    emit()
    op.bench_outputs = (per_node, trip, ew, total.tolist())
    return emit, host_n, host_m, n_cand.tolist()


def main():
    from tch_geometric import _cabi, _cabi_ladies
    from tch_geometric.loader import LADIESLoader, NeighborLoader
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
    loader = LADIESLoader(data, [S, S], input_nodes=inputs[:BATCHES * BATCH], batch_size=BATCH, prefetch=PREFETCH, shuffle=False,
                          device=dev)
    graph, ptrs, indices = loader._graph, loader.col_ptrs, loader.row_indices
    res = {"config": "RMAT-%d, %d directed edges, longest column %d; %d lists of %d random distinct nodes for the pair at s = %d; "
                     "loader: num_samples [%d, %d], batch %d, prefetch %d, %d f32 features, %d mini-batches per pass, %d interleaved "
                     "passes" % (SCALE, indices.numel(), int((ptrs[1:] - ptrs[:-1]).max()), LISTS, LIST_NODES, S, S, S, BATCH,
                                 PREFETCH, D, BATCHES, ROUNDS)}

    # ---- the pair alone, against the full-neighbour pair on the same frontiers
    lists = inputs[:LISTS * LIST_NODES].view(LISTS, LIST_NODES)
    op, flat, node_ptr, scanned = ladies_sized(_cabi_ladies, graph, ptrs, lists, n, S, dev)
    emit, host_n, host_m, host_cand = ladies_outputs(op, flat, node_ptr, dev)
    count = lambda: op.count(flat, node_ptr, 7, 0)
    # the composition's picks, and every word of its outputs against the pair's, before any time is taken
    import numpy as np
    from helpers_ladies import draw_t
    per_node, trip, ew, totals = op.bench_outputs
    picks = [torch.from_numpy(draw_t(7, b, S, totals[b]).astype(np.int64)).to(dev) for b in range(LISTS)]
    n_at, m_at = 0, 0
    for b in range(LISTS):
        out, cnt, wgt, rows, cols, e, w, S_b, nc = torch_ladies(ptrs, indices, lists[b], S, picks[b])
        assert int(S_b) == totals[b] and nc == host_cand[b] and out.numel() == host_n[b] and rows.numel() == host_m[b], b
        assert torch.equal(torch.stack([out, cnt, wgt]), per_node[:, n_at:n_at + host_n[b]]), b
        assert torch.equal(torch.stack([rows, cols, e]), trip[:, m_at:m_at + host_m[b]]), b
        assert torch.equal(w.view(torch.int32), ew[m_at:m_at + host_m[b]].view(torch.int32)), b
        n_at, m_at = n_at + host_n[b], m_at + host_m[b]

    def composition_lists():
        for b in range(LISTS):
            torch_ladies(ptrs, indices, lists[b], S, picks[b])
    fop, fflat, fnode_ptr, _ = bf.sized(_cabi, graph, ptrs, lists, n, dev)
    fnodes, ftrip, fnoff, feoff, fn, fm = bf.emitted(fop, fflat, fnode_ptr, dev)
    fcount = lambda: fop.count(fflat, fnode_ptr)
    femit = lambda: fop.emit(fnoff, feoff, fnodes, ftrip[0], ftrip[1], ftrip[2])
    pair = bf.interleaved({"ladies_count": lambda: bf.timed(count),
                           "ladies_emit": lambda: bf.timed(emit),
                           "full_count": lambda: bf.timed(fcount),
                           "full_emit": lambda: bf.timed(femit, before=fcount),
                           "torch_composition": lambda: bf.timed(composition_lists, warm=1, reps=3)})
    ms = lambda k: pair[k]["ms_median_of_medians"]
    for k in ("ladies_count", "ladies_emit", "full_count", "full_emit"):
        pair[k]["scanned_entries_per_s"] = round(scanned / (ms(k) * 1e-3), 0)
    pair.update({"lists": LISTS, "nodes_per_list": LIST_NODES, "n_samples": S, "scanned_entries_per_call": scanned,
                 "candidates_per_call": sum(host_cand), "out_nodes_per_call": sum(host_n), "kept_edges_per_call": sum(host_m),
                 "full_out_nodes_per_call": sum(fn), "full_edges_per_call": sum(fm),
                 "workspace_bytes_ladies": _cabi_ladies.ladies_workspace_bytes(graph, n, op.max_nodes, op.node_cap, op.chunk_cap,
                                                                             S, LISTS)[0],
                 "workspace_bytes_full": _cabi.ns_full_workspace_bytes(graph, n, fop.max_nodes, fop.node_cap, fop.chunk_cap, LISTS)[0],
                 "outputs_equal_torch_composition": True,      # asserted above, edge_weight as bits
                 "composition_over_ladies_pair": round(ms("torch_composition") / (ms("ladies_count") + ms("ladies_emit")), 3),
                 "count_ladies_over_full": round(ms("ladies_count") / ms("full_count"), 3),
                 "emit_ladies_over_full": round(ms("ladies_emit") / ms("full_emit"), 3),
                 "pair_ladies_over_full": round((ms("ladies_count") + ms("ladies_emit")) / (ms("full_count") + ms("full_emit")), 3)})
    res["pair"] = pair
    print(json.dumps(pair), file=sys.stderr, flush=True)
    del op, fop, fnodes, ftrip

    # ---- the hub check: one column of 1 000 003 entries against 62 501 columns of 16
    n_hub, long, short = 1 << 20, 1000003, 62501
    deg = torch.zeros(n_hub, dtype=torch.int64, device=dev)
    deg[0], deg[1:short + 1] = long, 16
    hptrs = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(deg, 0)])
    hidx = torch.randint(0, n_hub, (int(hptrs[-1]),), device=dev, generator=gen)
    hgraph = _cabi.graph_view(hptrs, hidx, indices32=hidx.to(torch.int32), ptrs32=hptrs.to(torch.int32))
    hub, runs = {}, {}
    for name, frontier in (("one_column_of_1000003", torch.zeros((1, 1), dtype=torch.int64, device=dev)),
                           ("62501_columns_of_16", torch.arange(1, short + 1, device=dev).view(1, -1))):
        hop, hflat, hnode_ptr, hm = ladies_sized(_cabi_ladies, hgraph, hptrs, frontier, n_hub, S, dev)
        hemit, hn, hk, hc = ladies_outputs(hop, hflat, hnode_ptr, dev)
        hub[name] = {"entries": hm, "candidates": sum(hc), "out_nodes": sum(hn), "kept_edges": sum(hk)}

        def both_hub(hop=hop, a=(hflat, hnode_ptr), e=hemit):
            hop.count(a[0], a[1], 7, 0)
            e()
        runs[name] = lambda f=both_hub: bf.timed(f)
    for name, s in bf.interleaved(runs).items():
        hub[name]["count_and_emit"] = s
        hub[name]["entries_per_s"] = round(hub[name]["entries"] / (s["ms_median_of_medians"] * 1e-3), 0)
    hub["hub_over_flat_ms"] = round(hub["one_column_of_1000003"]["count_and_emit"]["ms_median_of_medians"] /
                                    hub["62501_columns_of_16"]["count_and_emit"]["ms_median_of_medians"], 3)
    res["hub"] = hub
    print(json.dumps(hub), file=sys.stderr, flush=True)
    del hgraph, hptrs, hidx, runs

    # ---- the loaders: mini-batches/s and distinct nodes per mini-batch
    loaders = {"ladies_512_512": loader,
               "neighbor_15_10_unique": NeighborLoader(data, [15, 10], input_nodes=inputs[:BATCHES * BATCH], batch_size=BATCH,
                                                       prefetch=PREFETCH, unique=True, device=dev),
               "neighbor_15_10_labor": NeighborLoader(data, [15, 10], input_nodes=inputs[:BATCHES * BATCH], batch_size=BATCH,
                                                      prefetch=PREFETCH, unique=True, labor=True, device=dev)}
    nodes = {k: [] for k in loaders}

    def one_pass(name):
        torch.cuda.synchronize()
        nb, t0 = 0, time.perf_counter()
        for sb in loaders[name].super_batches():
            ptr = getattr(sb, "node_ptr", None)
            if ptr is None:
                nodes[name].extend(mb.num_nodes for mb in sb)
            else:
                ptr = ptr.tolist() if isinstance(ptr, torch.Tensor) else ptr
                nodes[name].extend(b - a for a, b in zip(ptr[:-1], ptr[1:]))
            nb += len(sb)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, nb

    passes = {k: [] for k in loaders}
    for k in loaders:
        one_pass(k)                                        # un-timed: capacities, workspaces, the allocator's pools
        nodes[k].clear()
    for r in range(ROUNDS):
        for k in (list(loaders) if r % 2 == 0 else list(loaders)[::-1]):
            passes[k].append(one_pass(k))
    res["loaders"] = {}
    for k in loaders:
        res["loaders"][k] = bf.rates(passes[k])
        res["loaders"][k]["distinct_nodes_per_mini_batch_mean"] = round(statistics.mean(nodes[k]), 1)
        res["loaders"][k]["distinct_nodes_per_mini_batch_max"] = max(nodes[k])
    res["loaders"]["ladies_512_512"]["growths"] = loader.growths
    print(json.dumps(res))


if __name__ == "__main__":
    main()
