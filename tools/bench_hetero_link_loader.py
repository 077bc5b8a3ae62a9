"""HeteroLinkNeighborLoader against the composition it replaces, on the cfg4-style synthetic graph of
tools/bench_hetero_unique_loader.py (3 node types A = 2^23, B = 2^22, C = 2^22; 5 relations x 20 M rectangular R-MAT
edges): the labelled relation is (A, e1, B), fan-out [15, 10], 1 024 positive edges per mini-batch, K = 1 negative each,
binary, try_count 8, prefetch 16, in one process.  Prints one JSON line (the kept run:
profiles/bench_hetero_link_loader.json):
  link_seeds_typed  one tg_link_seeds_typed launch of 16 mini-batches alone (HIP events, ms, median and best of ROUNDS
                    timings of 20 launches), with the binary search, with the edge set and unchecked (try_count 1), and
                    the share of negatives left unverified
  loaders           HeteroLinkNeighborLoader with unique=False and unique=True, with and without the edge set, and the
                    baseline -- the same loader with its seed launch replaced by what a trainer writes without it: a
                    torch.randint of unchecked negatives per node type, cat with the positives into the two input
                    tensors; the same tg_ns_hetero_batched (and dedup) launches behind it -- ROUNDS passes each,
                    interleaved, median / best / worst in mini-batches/s; every type's n_id and every relation's
                    edge_index are taken; over_baseline compares with the baseline of the same `unique`"""
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
from tch_geometric.loader import HeteroLinkNeighborLoader  # noqa: E402
from tch_geometric.transforms import HeteroGraph  # noqa: E402

dev = torch.device("cuda:0")
SHIFT = int(os.environ.get("SHIFT", "0"))              # > 0: a smaller graph (every scale lowered by SHIFT)
scales = {"A": 23 - SHIFT, "B": 22 - SHIFT, "C": 22 - SHIFT}
node_types = ["A", "B", "C"]
edge_types = [("A", "e0", "A"), ("A", "e1", "B"), ("B", "e2", "A"), ("B", "e3", "C"), ("C", "e4", "A")]
N_EDGES = int(os.environ.get("EDGES", 20_000_000 >> SHIFT))
BATCHES = int(os.environ.get("BATCHES", "256"))        # mini-batches of a timed pass
ROUNDS = int(os.environ.get("ROUNDS", "5"))
REL = ("A", "e1", "B")
FANOUT, E, K, TRIES, PREFETCH = [15, 10], 1024, 1, 8, 16
data = HeteroGraph()
for t in node_types:
    data[t].num_nodes = 1 << scales[t]
for r, et in enumerate(edge_types):
    data[et].edge_index = torch.stack(_cabi.rmat_edges_rect(scales[et[0]], scales[et[2]], N_EDGES, 0xC0F4 + r, dev))
gen = torch.Generator(device=dev)
gen.manual_seed(1)
pick = torch.randint(0, N_EDGES, (BATCHES * E,), device=dev, generator=gen)
eli = data[REL].edge_index[:, pick].contiguous()
res = {"config": "3 ntypes (2^%d, 2^%d, 2^%d), 5 etypes x %d edges, labelled relation %s, fan-out %s, %d positive edges per "
                 "mini-batch, K = %d, binary, try_count %d, prefetch %d, %d mini-batches per pass, %d interleaved passes"
                 % (scales["A"], scales["B"], scales["C"], N_EDGES, "-".join(REL), FANOUT, E, K, TRIES, PREFETCH, BATCHES,
                    ROUNDS),
       "link_seeds_typed": {}, "loaders": {}}

kw = dict(neg_sampling_ratio=K, neg_sampling="binary", try_count=TRIES, batch_size=E, prefetch=PREFETCH, device=dev)
forest = HeteroLinkNeighborLoader(data, FANOUT, (REL, eli), edge_set=True, **kw)
n_src, n_dst = forest.n_src, forest.n_dst


class Composition(HeteroLinkNeighborLoader):
    """the baseline: unchecked torch.randint negatives per node type, cat with the positives, the same launches behind"""

    def _launch_for(self, items, seeds_ts):
        G, width = items.shape
        src = torch.cat([self.edge_label_index[0][items], torch.randint(n_src, (G, K * width), device=dev)], dim=1)
        dst = torch.cat([self.edge_label_index[1][items], torch.randint(n_dst, (G, K * width), device=dev)], dim=1)
        slabs = self._new_launch([src, dst, None], None, G)
        slabs.link = (items, torch.zeros(G, dtype=torch.int64, device=dev))
        return slabs


def variant(unique, edge_set, cls=HeteroLinkNeighborLoader):
    """the same graph and CSCs (ingested once) under another configuration"""
    v = copy.copy(forest)
    v.__class__ = cls
    v.unique, v._consts, v._unique_out, v._unique_ws, v._unique_need, v.epoch = unique, {}, None, None, 0, 0
    if not edge_set:
        v._edge_set = None
    return v


# ---- the kernel alone
src = eli[0, :PREFETCH * E].reshape(PREFETCH, E).contiguous()
dst = eli[1, :PREFETCH * E].reshape(PREFETCH, E).contiguous()
for name, es, tries in (("binary_search", None, TRIES), ("edge_set", forest._edge_set, TRIES), ("unchecked", None, 1)):
    so = do = unv = None
    call = lambda: _cabi.link_seeds_typed(forest._rel_graph, src, dst, K, _cabi.LINK_BINARY, tries, 0, 0, n_src, n_dst, False,
                                          edge_set=es, src_out=so, dst_out=do, unverified=unv)
    so, do, unv = call()
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
    res["link_seeds_typed"][name] = {"ms_per_launch_median": round(statistics.median(ms), 4),
                                     "ms_per_launch_best": round(min(ms), 4),
                                     "unverified_share": round(int(unv.sum()) / (PREFETCH * K * E), 6)}
print(json.dumps(res["link_seeds_typed"]), file=sys.stderr, flush=True)


def loader_pass(loader):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nb = 0
    for g in loader:
        _ = [g[t].n_id for t in node_types], [g[et].edge_index for et in edge_types]
        nb += 1
    torch.cuda.synchronize()
    return time.perf_counter() - t0, nb


runs = {"baseline_randint_cat_NsHeteroBatched": variant(False, False, Composition),
        "baseline_randint_cat_NsHeteroBatched_unique": variant(True, False, Composition)}
for unique in (False, True):
    for edge_set in (False, True):
        runs["link_%s_%s" % ("unique" if unique else "forest", "edge_set" if edge_set else "binary_search")] = \
            variant(unique, edge_set)
for ld in runs.values():                               # un-timed: the allocator's pools, the workspace, the first launches
    loader_pass(ld)
passes = {k: [] for k in runs}
for _ in range(ROUNDS):
    for k, ld in runs.items():
        passes[k].append(loader_pass(ld))
for k, ps in passes.items():
    assert all(nb == BATCHES for _, nb in ps)
    rate = sorted(nb / dt for dt, nb in ps)
    med = statistics.median(rate)
    res["loaders"][k] = {"mini_batches_per_s_median": round(med, 1), "mini_batches_per_s_best": round(rate[-1], 1),
                         "mini_batches_per_s_worst": round(rate[0], 1), "ms_per_launch_of_16_median": round(16e3 / med, 3)}
for k in list(res["loaders"]):                         # each against the baseline that does the same work behind the sampler
    b = res["loaders"]["baseline_randint_cat_NsHeteroBatched" + ("_unique" if "unique" in k else "")]
    res["loaders"][k]["over_baseline"] = round(res["loaders"][k]["mini_batches_per_s_median"] / b["mini_batches_per_s_median"], 3)
print(json.dumps(res))
