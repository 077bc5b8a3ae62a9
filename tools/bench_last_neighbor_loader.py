"""The streaming last-k neighbour state (tg_lastn_*, LastNeighborLoader, TemporalEventLoader) on RMAT-24's edges taken as an
event stream in a random order, k = 10, 200 events per step, 3 seeds per event (src, dst, one negative), in one process.
Prints one JSON line (the kept run: profiles/bench_last_neighbor_loader.json; a path argument writes it there too):
  calls     one tg_lastn_sample of a step's 600 seeds and one tg_lastn_insert of its 200 events (HIP events, ms per call;
            ROUNDS interleaved medians and their spread), the insert under both forms
  replay    tg_lastn_replay, ms per step at 1 / 16 / 256 steps per call
  pyg       the torch composition of PyG's LastNeighborLoader (lookup + insert) per step, after its outputs compared equal
            to LastNeighborLoader's as sets (PyG sorts n_id) on steps where no node exceeds `size` entries
  recent    tg_ns_homo_batched_ws with TG_SAMPLER_RECENT on the static CSC of the whole stream under the filter
            e_id < step start: the offline route the state stands beside
  loader    TemporalEventLoader mini-batches/s at prefetch 1 / 16 / 256
  hub       a step whose 200 events all touch one node against a spread step: insert and sample
The timing helpers are tools/bench_full_neighbor_loader.py's."""
import json
import os
import sys
import time

import torch

import bench_full_neighbor_loader as bf

SCALE = bf.SCALE
K, STEP = int(os.environ.get("SIZE", "10")), int(os.environ.get("STEP", "200"))
EVENTS = int(os.environ.get("EVENTS", str(256 * 200 * 4)))       # the prefix of the stream the timed passes walk
WARM_EVENTS = int(os.environ.get("WARM_EVENTS", "2000000"))      # inserted before anything is timed: the rings are in use


def pyg_insert(st, src, dst):
    """torch_geometric/nn/models/tgn.py LastNeighborLoader.insert, on st = dict(nbr, e_id [n, size], assoc [n], cur)"""
    size = st["nbr"].shape[1]
    nbrs, nodes = torch.cat([src, dst]), torch.cat([dst, src])
    e_id = torch.arange(st["cur"], st["cur"] + src.numel(), device=src.device).repeat(2)
    st["cur"] += src.numel()
    nodes, perm = nodes.sort()
    nbrs, e_id = nbrs[perm], e_id[perm]
    n_id = nodes.unique()
    st["assoc"][n_id] = torch.arange(n_id.numel(), device=n_id.device)
    dense = torch.arange(nodes.numel(), device=nodes.device) % size + st["assoc"][nodes] * size
    d_e = e_id.new_full((n_id.numel() * size,), -1)
    d_e[dense] = e_id
    d_n = e_id.new_empty(n_id.numel() * size)
    d_n[dense] = nbrs
    all_e = torch.cat([st["e_id"][n_id], d_e.view(-1, size)], dim=-1)
    all_n = torch.cat([st["nbr"][n_id], d_n.view(-1, size)], dim=-1)
    top_e, perm = all_e.topk(size, dim=-1)
    st["e_id"][n_id], st["nbr"][n_id] = top_e, torch.gather(all_n, 1, perm)


def pyg_lookup(st, n_id):
    size = st["nbr"].shape[1]
    nbrs, e_id = st["nbr"][n_id], st["e_id"][n_id]
    nodes = n_id.view(-1, 1).repeat(1, size)
    mask = e_id >= 0
    nbrs, nodes, e_id = nbrs[mask], nodes[mask], e_id[mask]
    n_id = torch.cat([n_id, nbrs]).unique()
    st["assoc"][n_id] = torch.arange(n_id.numel(), device=n_id.device)
    return n_id, torch.stack([st["assoc"][nbrs], st["assoc"][nodes]]), e_id


def triples(n_id, edge_index, e_id):
    """the lookup's edges as sorted rows (query node, e_id, neighbour): what both loaders must agree on"""
    rows = torch.stack([n_id[edge_index[1]], e_id, n_id[edge_index[0]]], dim=1)
    return torch.unique(rows, dim=0)


def main():
    from tch_geometric import _cabi, _cabi_lastn
    from tch_geometric.last_neighbor import LastNeighborLoader, TemporalEventLoader
    dev = torch.device("cuda:0")
    n = 1 << SCALE
    row, col = _cabi.rmat_edges(SCALE, n * 16, 0x5EED0000 + SCALE, dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    order = torch.randperm(row.numel(), device=dev, generator=gen)
    src, dst = row[order].contiguous(), col[order].contiguous()      # the stream: event j is (src[j], dst[j]) with e_id j
    del row, col, order
    E = src.numel()
    assert WARM_EVENTS + EVENTS <= E
    G_MAX = EVENTS // STEP
    neg = torch.randint(0, n, (G_MAX, STEP), device=dev, generator=gen)
    a0 = WARM_EVENTS
    seeds = torch.cat([src[a0:a0 + EVENTS].view(G_MAX, STEP), dst[a0:a0 + EVENTS].view(G_MAX, STEP), neg], dim=1).contiguous()
    res = {"config": "RMAT-%d's %d edges as a stream in a random order, k = %d, %d events per step, %d seeds per step; %d "
                     "events inserted before the timed window of %d; %d interleaved passes" % (SCALE, E, K, STEP, 3 * STEP,
                                                                                              WARM_EVENTS, EVENTS, bf.ROUNDS)}
    ln = _cabi_lastn.LastN(n, K, dev)

    def warm(state):
        state.reset()
        for a in range(0, WARM_EVENTS, 1 << 21):
            b = min(a + (1 << 21), WARM_EVENTS)
            state.insert(src[a:b], dst[a:b], e_base=a)
    warm(ln)
    base = ln.state_dict()
    res["state_bytes"] = ln.state_bytes

    # ---- the outputs against PyG's algorithm, on steps where no node has more than k entries
    ours, pyg = LastNeighborLoader(n, K, device=dev), dict(nbr=torch.empty((n, K), dtype=torch.int64, device=dev),
                                                           e_id=torch.full((n, K), -1, dtype=torch.int64, device=dev),
                                                           assoc=torch.empty(n, dtype=torch.int64, device=dev), cur=0)
    compared = 0
    for g in range(G_MAX):
        s, d = src[a0 + g * STEP:a0 + (g + 1) * STEP], dst[a0 + g * STEP:a0 + (g + 1) * STEP]
        if int(torch.bincount(torch.cat([s, d])).max()) > K:
            continue
        got, want = ours(seeds[g]), pyg_lookup(pyg, seeds[g])
        assert torch.equal(torch.sort(got[0]).values, want[0]) and torch.equal(triples(*got), triples(*want)), g
        ours.insert(s, d)
        pyg_insert(pyg, s, d)
        compared += 1
        if compared == 24:
            break
    assert compared == 24
    res["outputs_equal_pyg_composition_on_steps"] = compared
    del ours

    # ---- single calls
    out1 = _cabi.NsBatchedOut(1, 3 * STEP, [K], dev)
    s0, d0 = src[a0:a0 + STEP], dst[a0:a0 + STEP]
    calls = bf.interleaved({
        "sample_600_seeds": lambda: bf.timed(lambda: ln.sample(seeds[:1], [K], out=out1)),
        "insert_200_events_lds": lambda: bf.timed(lambda: ln.insert(s0, d0, e_base=a0, form=1)),
        "insert_200_events_grid": lambda: bf.timed(lambda: ln.insert(s0, d0, e_base=a0, form=2)),
        "pyg_composition_step": lambda: bf.timed(lambda: (pyg_lookup(pyg, seeds[0]), pyg_insert(pyg, s0, d0)))})
    res["calls"] = calls
    print(json.dumps(calls), file=sys.stderr, flush=True)

    # ---- replay per step
    replay = {}
    for G in (1, 16, 256):
        G = min(G, G_MAX)
        outG = _cabi.NsBatchedOut(G, 3 * STEP, [K], dev)
        fn = lambda G=G, outG=outG: ln.replay(src[a0:a0 + G * STEP], dst[a0:a0 + G * STEP], seeds[:G], [K], STEP, e_base=a0, out=outG)
        replay["steps_per_call_%d" % G] = (G, lambda fn=fn: bf.timed(fn))
    timed = bf.interleaved({k: v[1] for k, v in replay.items()})
    for k, (G, _) in replay.items():
        timed[k]["ms_per_step"] = round(timed[k]["ms_median_of_medians"] / G, 5)
    res["replay"] = timed
    print(json.dumps(timed), file=sys.stderr, flush=True)

    # ---- the offline route: RECENT on the CSC of the whole stream under e_id < step start
    # (both directions of every event, as the state holds them: column v = the entries of node v, timestamps = e_id)
    ptrs, idx, perm = _cabi.coo_to_csx(torch.cat([src, dst]), torch.cat([dst, src]), n, n, True)
    ts = (perm % E).contiguous()
    graph = _cabi.graph_view(ptrs, idx, timestamps=ts, max_degree="auto")
    outR = _cabi.NsBatchedOut(1, 3 * STEP, [K], dev, with_states=True)
    wsR = _cabi.ns_homo_batched_workspace(graph, 1, 3 * STEP, [K], dev, sampler=_cabi.SAMPLER_RECENT, filter_mode=_cabi.FILTER_STATIC)
    zeros = torch.zeros((1, 3 * STEP), dtype=torch.int64, device=dev)
    recent = lambda: _cabi.ns_homo_batched(graph, seeds[:1], [K], 1, 2, outR, sampler=_cabi.SAMPLER_RECENT,
                                           filter_mode=_cabi.FILTER_STATIC, window=(0, a0 - 1), seeds_state=zeros, ws=wsR)
    ln.load_state_dict(base)
    recent()
    ln.sample(seeds[:1], [K], out=out1)
    torch.cuda.synchronize()
    cnt = out1.counts.cpu()[0].tolist()
    assert outR.counts.cpu()[0].tolist() == cnt                      # the same neighbourhoods
    assert torch.equal(graph._keep[3][outR.edge_index[0, :cnt[1]]], out1.edge_index[0, :cnt[1]])
    res["recent_on_static_csc"] = bf.interleaved({"recent_600_seeds": lambda: bf.timed(recent),
                                                  "lastn_sample_600_seeds": lambda: bf.timed(lambda: ln.sample(seeds[:1], [K], out=out1))})
    res["recent_on_static_csc"]["outputs_equal"] = True
    res["recent_on_static_csc"]["longest_column"] = int(graph.max_degree)
    print(json.dumps(res["recent_on_static_csc"]), file=sys.stderr, flush=True)
    res["recent_on_static_csc"]["csc_entries"] = 2 * E
    del graph, ptrs, idx, perm, ts, outR, wsR

    # ---- the hub check
    hub_node = int(torch.bincount(dst[:1 << 22]).argmax())
    hs, hd = torch.randint(0, n, (STEP,), device=dev, generator=gen), torch.full((STEP,), hub_node, device=dev)
    hseeds = torch.full((1, 3 * STEP), hub_node, device=dev)
    res["hub"] = bf.interleaved({
        "insert_all_on_one_node": lambda: bf.timed(lambda: ln.insert(hs, hd, e_base=a0, form=1)),
        "insert_spread": lambda: bf.timed(lambda: ln.insert(s0, d0, e_base=a0, form=1)),
        "sample_one_node_600_times": lambda: bf.timed(lambda: ln.sample(hseeds, [K], out=out1)),
        "sample_spread": lambda: bf.timed(lambda: ln.sample(seeds[:1], [K], out=out1))})
    print(json.dumps(res["hub"]), file=sys.stderr, flush=True)
    del ln

    # ---- the loader
    t = torch.arange(EVENTS)
    loaders = {"prefetch_%d" % p: TemporalEventLoader(src[a0:a0 + EVENTS], dst[a0:a0 + EVENTS], t, n, K, STEP, prefetch=p, device=dev)
               for p in (1, 16, 256)}

    def one_pass(name):
        torch.cuda.synchronize()
        nb, t0 = 0, time.perf_counter()
        for _ in loaders[name]:
            nb += 1
        torch.cuda.synchronize()
        return time.perf_counter() - t0, nb
    passes = {k: [] for k in loaders}
    for k in loaders:
        one_pass(k)
    for r in range(bf.ROUNDS):
        for k in (list(loaders) if r % 2 == 0 else list(loaders)[::-1]):
            passes[k].append(one_pass(k))
    res["loader"] = {k: bf.rates(passes[k]) for k in loaders}
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
