"""tg_cn_links on RMAT-24 (16 edges per node, directed, its CSC), in one process.  Prints one JSON line (the kept run:
profiles/bench_cn.json):
  random   LINKS random links (both ends uniform over the vertices), cn_cap 256, both tables: links/s and row entries/s (the
           entries of both ends' rows, what a merge would read) of _WAVE, _GROUP and AUTO, HIP events, ROUNDS interleaved
           medians and their spread
  hubs     HUB_LINKS links whose ends are both drawn from the vertices with at least HUB_DEGREE entries, the same way, and
           AUTO under several wave_max
  torch    what a user does today, on the same device and the same links: per batch of links the keys v * N + w for w in
           row(u), looked up with torch.searchsorted in the graph's sorted key array, counts by index_add_ and the members by
           a mask.  Parallel entries are not folded and no score is summed, which favours it; the total of its hits is
           printed beside the kernel's total of distinct members
No device setting is touched.  The timing helpers are tools/bench_full_neighbor_loader.py's."""
import json
import os
import sys

import torch

import bench_full_neighbor_loader as bf

SCALE = bf.SCALE
LINKS = int(os.environ.get("LINKS", str(1 << 20)))
HUB_LINKS = int(os.environ.get("HUB_LINKS", str(1 << 14)))
HUB_DEGREE = int(os.environ.get("HUB_DEGREE", "2048"))
CAP = int(os.environ.get("CN_CAP", "256"))
TORCH_ENTRIES = 1 << 26                                    # expanded entries per batch of the composition


def torch_cn(ptrs, indices, keys, n, u, v):
    """the composition: -> (count [L], members flat); no read-back but the batching's"""
    dev, L = u.device, u.numel()
    begin = ptrs[u]
    deg = ptrs[u + 1] - begin
    before = torch.cumsum(deg, 0) - deg
    m = int(deg.sum())
    slot = torch.repeat_interleave(torch.arange(L, device=dev), deg, output_size=m)
    w = indices[torch.arange(m, device=dev) + (begin - before)[slot]]
    q = v[slot] * n + w
    at = torch.searchsorted(keys, q).clamp(max=keys.numel() - 1)
    hit = (keys[at] == q) & (w != u[slot]) & (w != v[slot])
    return torch.zeros(L, dtype=torch.int64, device=dev).index_add_(0, slot, hit.to(torch.int64)), w[hit]


def torch_batches(ptrs, u):
    """cuts of the links so that a batch expands to at most TORCH_ENTRIES entries (found once, outside the timing)"""
    deg = (ptrs[u + 1] - ptrs[u]).cpu().tolist()
    cuts, acc = [0], 0
    for i, d in enumerate(deg):
        if acc + d > TORCH_ENTRIES and i > cuts[-1]:
            cuts.append(i)
            acc = 0
        acc += d
    return cuts + [len(deg)]


def main():
    from tch_geometric import _cabi, _cabi_cn as ops
    dev = torch.device("cuda:0")
    n = 1 << SCALE
    row, col = _cabi.rmat_edges(SCALE, n * 16, 0x5EED0000 + SCALE, dev)
    ptrs, indices, _ = _cabi.coo_to_csx(row, col, n, n, True)
    del row, col
    graph = _cabi.graph_view(ptrs, indices, indices32=indices.to(torch.int32), ptrs32=ptrs.to(torch.int32))
    deg = ptrs[1:] - ptrs[:-1]
    keys = torch.repeat_interleave(torch.arange(n, device=dev), deg) * n + indices       # ascending: the CSC's own order
    tables = ops.cn_tables(ptrs, indices)
    gen = torch.Generator(device=dev)
    gen.manual_seed(13)
    hubs = torch.nonzero(deg >= HUB_DEGREE).view(-1)
    work = {"random": torch.randint(0, n, (2, LINKS), device=dev, generator=gen),
            "hubs": hubs[torch.randint(0, hubs.numel(), (2, HUB_LINKS), device=dev, generator=gen)]}
    res = {"config": "RMAT-%d CSC, %d entries, longest row %d, %d vertices with >= %d entries; %d random links, %d hub links, "
                     "cn_cap %d, 2 tables, u32 shadows; %d interleaved rounds"
                     % (SCALE, indices.numel(), int(deg.max()), hubs.numel(), HUB_DEGREE, LINKS, HUB_LINKS, CAP, bf.ROUNDS),
           "constants": {"TG_CN_WINDOW": ops.CN_WINDOW, "TG_CN_WAVE_MAX": ops.CN_WAVE_MAX, "TG_CN_GROUP_TILES": ops.CN_GROUP_TILES}}
    for name, links in work.items():
        u, v = links[0].contiguous(), links[1].contiguous()
        L = u.numel()
        entries = int((deg[u] + deg[v]).sum())
        shorter = int(torch.minimum(deg[u], deg[v]).sum())
        runs, outs = {}, {}
        forms = [("wave", dict(form=ops.FORM_WAVE)), ("group", dict(form=ops.FORM_GROUP)), ("auto", dict(form=ops.FORM_AUTO))]
        if name == "hubs":
            forms += [("auto_wave_max_%d" % wm, dict(form=ops.FORM_AUTO, wave_max=wm)) for wm in (256, 1024, 16384)]
        for key, kw in forms:
            outs[key] = ops.cn_links(graph, u, v, CAP, tables=tables, **kw)
            runs[key] = lambda kw=kw, o=outs[key]: bf.timed(lambda: ops.cn_links(graph, u, v, CAP, tables=tables, out=o, ws=o["ws"],
                                                                                  status=o["status"], **kw))
        first = outs[forms[0][0]]
        for key, _ in forms[1:]:                               # equal words in every form
            for word in ("count", "adjacent", "score"):
                assert torch.equal(first[word], outs[key][word]), (name, key, word)
        cuts = torch_batches(ptrs, u)

        def composition():
            return [torch_cn(ptrs, indices, keys, n, u[a:b], v[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        hits = sum(int(c.sum()) for c, _ in composition())
        runs["torch_searchsorted"] = lambda: bf.timed(composition, warm=1, reps=3)
        part = bf.interleaved(runs)
        for key, s in part.items():
            sec = s["ms_median_of_medians"] * 1e-3
            s["links_per_s"], s["row_entries_per_s"] = round(L / sec, 0), round(entries / sec, 0)
        part.update({"links": L, "row_entries": entries, "shorter_row_entries": shorter, "torch_batches": len(cuts) - 1,
                     "common_neighbours": int(first["count"].sum()), "torch_hits_with_parallel_entries": hits,
                     "links_cut_by_cap": int((first["count"] > CAP).sum()),
                     "torch_over_auto": round(part["torch_searchsorted"]["ms_median_of_medians"] /
                                              part["auto"]["ms_median_of_medians"], 3)})
        res[name] = part
        print(json.dumps({name: part}), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
