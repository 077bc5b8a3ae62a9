"""tg_seal_nodes_capped on RMAT-24 (16 edges per node, directed, its CSC, u32 shadows), in one process.  Prints one JSON line (the
kept run: profiles/bench_seal_capped.json), h = 2, caps [100, 100], node_cap 202:
  random   LINKS random links: links/s and row entries/s (the rows of every vertex of N, which the rounds walk) of the capped
           call, HIP events, ROUNDS interleaved medians and their spread
  hubs     HUB_LINKS links between vertices with at least HUB_DEGREE entries, the same way
  uncut    the links of `random` that tg_seal_nodes does not refuse at the same node_cap (the refused share is printed):
           tg_seal_nodes and the capped call on them, interleaved, and their ratio; then the same pair on the links of
           these that the capped call does not cut either (equal words: what the Philox per entry costs)
--seal-nodes-only times tg_seal_nodes alone on the `uncut` links and imports nothing newer than _cabi_seal: run it on a checkout
of an older commit and on this one, in turns, to compare tg_seal_nodes between them.  --label names the tree in the output.
No device setting is touched.  The timing helpers are tools/bench_full_neighbor_loader.py's."""
import argparse
import json
import os
import sys

import torch

import bench_full_neighbor_loader as bf

SCALE = bf.SCALE
LINKS = int(os.environ.get("LINKS", str(1 << 16)))
HUB_LINKS = int(os.environ.get("HUB_LINKS", str(1 << 12)))
HUB_DEGREE = int(os.environ.get("HUB_DEGREE", "2048"))
CAPS, SEED = [100, 100], 7


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--seal-nodes-only", action="store_true")
    parser.add_argument("--label", default="unlabelled")
    args = parser.parse_args()
    from tch_geometric import _cabi, _cabi_seal
    dev = torch.device("cuda:0")
    n = 1 << SCALE
    row, col = _cabi.rmat_edges(SCALE, n * 16, 0x5EED0000 + SCALE, dev)
    ptrs, indices, _ = _cabi.coo_to_csx(row, col, n, n, True)
    del row, col
    graph = _cabi.graph_view(ptrs, indices, indices32=indices.to(torch.int32), ptrs32=ptrs.to(torch.int32))
    deg = ptrs[1:] - ptrs[:-1]
    gen = torch.Generator(device=dev)
    gen.manual_seed(13)
    hubs = torch.nonzero(deg >= HUB_DEGREE).view(-1)
    sizes = _cabi_seal.Seal(len(CAPS), 2 + sum(CAPS))

    def distinct(links):
        return links[:, links[0] != links[1]].contiguous()

    def entries(out):
        inside = torch.arange(sizes.node_cap, device=dev)[None, :] < out["count"][:, None]
        return int(deg[out["nodes"][inside]].sum())

    def seal_nodes(u, v, out=None):
        return _cabi_seal.seal_nodes(graph, u, v, sizes, distances=False,
                                     **({} if out is None else dict(out=out, ws=out["ws"], status=out["status"])))

    work = {"random": distinct(torch.randint(0, n, (2, LINKS), device=dev, generator=gen)),
            "hubs": distinct(hubs[torch.randint(0, hubs.numel(), (2, HUB_LINKS), device=dev, generator=gen)])}
    res = {"tree": args.label,
           "config": "RMAT-%d CSC, %d entries, longest row %d, %d vertices with >= %d entries; h = 2, caps %s, node_cap %d, u32 "
                     "shadows; %d interleaved rounds" % (SCALE, indices.numel(), int(deg.max()), hubs.numel(), HUB_DEGREE, CAPS,
                                                         sizes.node_cap, bf.ROUNDS)}
    links = work["random"]
    kept = links[:, seal_nodes(links[0], links[1])["count"] > 0].contiguous()
    u, v = kept[0], kept[1]
    a = seal_nodes(u, v)
    if args.seal_nodes_only:
        part = bf.interleaved({"seal_nodes": lambda: bf.timed(lambda: seal_nodes(u, v, a))})
        part.update(links=kept.shape[1], refused_share=round(1 - kept.shape[1] / links.shape[1], 4), row_entries=entries(a))
        res["uncut"] = part
        print(json.dumps(res))
        return
    from tch_geometric import _cabi_seal_capped as ops

    def capped(u, v, out=None):
        return ops.seal_nodes_capped(graph, u, v, sizes, CAPS, SEED, out=out, distances=False,
                                     **({} if out is None else dict(ws=out["ws"], status=out["status"])))

    for name, ls in work.items():
        out = capped(ls[0], ls[1])
        part = bf.interleaved({"capped": lambda ls=ls, out=out: bf.timed(lambda: capped(ls[0], ls[1], out))})
        sec, walked = part["capped"]["ms_median_of_medians"] * 1e-3, entries(out)
        part.update(links=ls.shape[1], row_entries=walked, links_per_s=round(ls.shape[1] / sec, 0),
                    row_entries_per_s=round(walked / sec, 0), links_cut=int((out["cut"] != 0).sum()))
        res[name] = part
        print(json.dumps({name: part}), file=sys.stderr, flush=True)
    b = capped(u, v)
    same = b["cut"] == 0                                                         # equal words wherever no hop was cut
    assert torch.equal(a["count"][same], b["count"][same]) and torch.equal(a["nodes"][same, :2], b["nodes"][same, :2])
    for name, pick in (("uncut", kept), ("uncut_by_both", kept[:, same].contiguous())):
        pu, pv = pick[0], pick[1]
        oa, ob = seal_nodes(pu, pv), capped(pu, pv)
        part = bf.interleaved({"seal_nodes": lambda: bf.timed(lambda: seal_nodes(pu, pv, oa)),
                               "capped": lambda: bf.timed(lambda: capped(pu, pv, ob))})
        part.update(links=pick.shape[1], links_cut_by_the_capped_call=int((ob["cut"] != 0).sum()), row_entries=entries(oa),
                    refused_share_of_random=round(1 - kept.shape[1] / links.shape[1], 4),
                    capped_over_seal_nodes=round(part["capped"]["ms_median_of_medians"] /
                                                 part["seal_nodes"]["ms_median_of_medians"], 3))
        res[name] = part
    print(json.dumps(res))


if __name__ == "__main__":
    main()
