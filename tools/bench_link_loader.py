"""LinkNeighborLoader against the composition it replaces, on RMAT-24: fan-out [15, 10], 1 024 positive edges per mini-batch,
K = 1 negative each, binary, try_count 8, prefetch 16, in one process.  Prints one JSON line (the kept run:
profiles/bench_link_loader.json):
  link_seeds   one tg_link_seeds launch of 16 mini-batches alone (HIP events, ms, median and best of ROUNDS timings of 20
               launches), with the binary search and with the edge set, for try_count 8 and try_count 1 (no look-up), and
               the share of negatives left unverified
  loaders      LinkNeighborLoader with unique=False and unique=True, with and without the edge set, and the baseline --
               per epoch one torch.randint of unchecked negatives, cat with the positives into the same seed rows, then
               NeighborLoader(input_nodes=rows, batch_size=S), with unique=False and unique=True: the same sampler (and
               dedup) launches -- ROUNDS passes each, interleaved, median / best / worst in mini-batches/s; every
               mini-batch's n_id and edge_index are taken; over_baseline compares with the baseline of the same `unique`"""
import copy
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tch-geometric_amd"))
from tch_geometric import _cabi  # noqa: E402
from tch_geometric.loader import LinkNeighborLoader, NeighborLoader  # noqa: E402
from tch_geometric.transforms import Graph  # noqa: E402

dev = torch.device("cuda:0")
SCALE = int(os.environ.get("SCALE", "24"))
BATCHES = int(os.environ.get("BATCHES", "256"))        # mini-batches of a timed pass
ROUNDS = int(os.environ.get("ROUNDS", "5"))
FANOUT, E, K, TRIES, PREFETCH = [15, 10], 1024, 1, 8, 16
n = 1 << SCALE
row, col = _cabi.rmat_edges(SCALE, n * 16, 0x5EED0000 + SCALE, dev)
data = Graph(edge_index=torch.stack([row, col]), num_nodes=n)
del row, col
gen = torch.Generator(device=dev)
gen.manual_seed(1)
pick = torch.randint(0, data.edge_index.shape[1], (BATCHES * E,), device=dev, generator=gen)
eli = data.edge_index[:, pick].contiguous()
S, P = _cabi.link_seeds_capacity(E, K, _cabi.LINK_BINARY)
res = {"config": "RMAT-%d, fan-out %s, %d positive edges per mini-batch, K = %d, binary, try_count %d, prefetch %d, %d "
                 "mini-batches per pass, %d interleaved passes" % (SCALE, FANOUT, E, K, TRIES, PREFETCH, BATCHES, ROUNDS),
       "seeds_per_mini_batch": S, "link_seeds": {}, "loaders": {}}

kw = dict(edge_label_index=eli, neg_sampling_ratio=K, neg_sampling="binary", try_count=TRIES, batch_size=E,
          prefetch=PREFETCH, device=dev)
forest = LinkNeighborLoader(data, FANOUT, edge_set=True, **kw)


def variant(unique, edge_set):
    """the same graph and CSC (ingested once) under another configuration"""
    v = copy.copy(forest)
    v.unique, v._pool, v._side, v._consts, v.epoch = unique, [], None, {}, 0
    if not edge_set:
        v._edge_set = None
    return v


base = NeighborLoader(data, FANOUT, input_nodes=eli.new_zeros(S), batch_size=S, prefetch=PREFETCH, device=dev)

# ---- the kernel alone
src, dst = eli[0, :PREFETCH * E].reshape(PREFETCH, E).contiguous(), eli[1, :PREFETCH * E].reshape(PREFETCH, E).contiguous()
for name, es, tries in (("binary_search", None, TRIES), ("edge_set", forest._edge_set, TRIES), ("unchecked", None, 1)):
    out = unv = None
    call = lambda: _cabi.link_seeds(forest._graph, src, dst, K, _cabi.LINK_BINARY, tries, 0, 0, n, edge_set=es, out=out,
                                    unverified=unv)
    out, unv = call()
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(ROUNDS):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(20):
            call()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]) / 20)
    res["link_seeds"][name] = {"ms_per_launch_median": round(statistics.median(ms), 4), "ms_per_launch_best": round(min(ms), 4),
                               "unverified_share": round(int(unv.sum()) / (PREFETCH * K * E), 6)}
print(json.dumps(res["link_seeds"]), file=sys.stderr, flush=True)


def loader_pass(loader):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nb = 0
    for mb in loader:
        _ = (mb.n_id, mb.edge_index)
        nb += 1
    torch.cuda.synchronize()
    return time.perf_counter() - t0, nb


def baseline_pass():
    """what a trainer writes without the feature: unchecked negatives, the same seed rows, the node-seeded loader"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    neg = torch.randint(n, (2, BATCHES, K * E), device=dev)
    rows = torch.cat([eli[0].view(BATCHES, E), neg[0], eli[1].view(BATCHES, E), neg[1]], dim=1)
    base.input_nodes = rows.reshape(-1)
    nb = 0
    for mb in base:
        _ = (mb.n_id, mb.edge_index)
        nb += 1
    torch.cuda.synchronize()
    return time.perf_counter() - t0, nb


base_forest, base_unique = base, copy.copy(base)
base_unique.unique, base_unique._pool, base_unique._side = True, [], None


def baseline_of(loader):
    def run():
        global base
        base = loader
        return baseline_pass()
    return run


runs = {"baseline_randint_cat_NeighborLoader": baseline_of(base_forest),
        "baseline_randint_cat_NeighborLoader_unique": baseline_of(base_unique)}
for unique in (False, True):
    for edge_set in (False, True):
        v = variant(unique, edge_set)
        runs["link_%s_%s" % ("unique" if unique else "forest", "edge_set" if edge_set else "binary_search")] = \
            (lambda v=v: loader_pass(v))
for f in runs.values():                                # un-timed: the allocator's pools, the slabs, the first launches
    f()
passes = {k: [] for k in runs}
for _ in range(ROUNDS):
    for k, f in runs.items():
        passes[k].append(f())
for k, ps in passes.items():
    assert all(nb == BATCHES for _, nb in ps)
    rate = sorted(nb / dt for dt, nb in ps)
    med = statistics.median(rate)
    res["loaders"][k] = {"mini_batches_per_s_median": round(med), "mini_batches_per_s_best": round(rate[-1]),
                         "mini_batches_per_s_worst": round(rate[0]), "ms_per_launch_of_16_median": round(16e3 / med, 3)}
for k in list(res["loaders"]):                         # each against the baseline that does the same work behind the sampler
    b = res["loaders"]["baseline_randint_cat_NeighborLoader" + ("_unique" if "unique" in k else "")]
    res["loaders"][k]["over_baseline"] = round(res["loaders"][k]["mini_batches_per_s_median"] / b["mini_batches_per_s_median"], 3)
print(json.dumps(res))
