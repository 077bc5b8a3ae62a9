"""A/B of library builds on the node dedup operators (the method and the command line: tools/ab_loop.py).  Cases, on RMAT-20
with 16 edges per node and seeds from seed_batches:
  ns_homo_unique, ns_homo_unique_grouped (identity groups)   flat form: 16 batches x 1 024 seeds x [15, 10] (169 984
      positions, the loader's shape); LDS form: 2 048 batches x 128 seeds x [5, 3] (2 688 positions)
  ns_typed_unique   one sampled hetero launch, set up as tools/bench_hetero_unique_loader.py's `dedup` section (SHIFT > 0:
      a smaller graph), in its auto form and forced flat
Prints one JSON object."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tch-geometric_amd"))
import ab_loop  # noqa: E402
from tch_geometric import _cabi  # noqa: E402
from tch_geometric.loader import HeteroNeighborLoader  # noqa: E402
from tch_geometric.transforms import HeteroGraph  # noqa: E402

dev = torch.device("cuda:0")
cases = {}                                                   # name -> a call that launches the operator once
scale = 20
n = 1 << scale
row, col = _cabi.rmat_edges(scale, n * 16, 0x5EED0000 + scale, dev)
ptrs, idx, _ = _cabi.coo_to_csx(row, col, n, n, True)
g = _cabi.graph_view(ptrs, idx, indices32=idx.to(torch.int32), ptrs32=ptrs.to(torch.int32))
keep = []
for tag, form, G, B, fan in (("flat", 2, 16, 1024, [15, 10]), ("lds", 1, 2048, 128, [5, 3])):
    slabs = _cabi.NsBatchedOut(G, B, fan, dev)
    _cabi.ns_homo_batched(g, _cabi.seed_batches(0xBA7C4, 0, G, B, n, dev), fan, 0, 0, slabs)
    cap = slabs.samples.shape[1]
    plain = dict(form=form, ws=_cabi.ns_homo_unique_workspace(cap, n, G, dev, form), result=_cabi.NsUniqueOut(slabs))
    grouped = dict(form=form, ws=_cabi.ns_homo_unique_grouped_workspace(cap, n, B, G, dev, form),
                   result=_cabi.NsUniqueOut(slabs, with_group=True))
    cases["ns_homo_unique/" + tag] = lambda s=slabs, G=G, kw=plain: _cabi.ns_homo_unique(s, G, n, **kw)
    cases["ns_homo_unique_grouped/" + tag] = lambda s=slabs, G=G, kw=grouped: _cabi.ns_homo_unique_grouped(s, G, n, **kw)

SHIFT = int(os.environ.get("SHIFT", "0"))
scales = {"A": 23 - SHIFT, "B": 22 - SHIFT, "C": 22 - SHIFT}
data = HeteroGraph()
for t in scales:
    data[t].num_nodes = 1 << scales[t]
for r, et in enumerate([("A", "e0", "A"), ("A", "e1", "B"), ("B", "e2", "A"), ("B", "e3", "C"), ("C", "e4", "A")]):
    data[et].edge_index = torch.stack(_cabi.rmat_edges_rect(scales[et[0]], scales[et[2]], 20_000_000 >> SHIFT, 0xC0F4 + r, dev))
G, B = 16, 1024
seeds = _cabi.seed_batches(0xBA7C4, 0, G, B, 1 << scales["A"], dev)
ld = HeteroNeighborLoader(data, [15, 10], unique=True, input_type="A", input_nodes=seeds.reshape(-1), batch_size=B, prefetch=G)
rels, bounds = ld._rels, ld._id_bounds
hb = _cabi.NsHeteroBatched(3, rels, [seeds.contiguous(), None, None], 2, G, dev)
hb.run(0, 0)
pitches = [x.shape[1] for x in hb.samples]
auto = _cabi.ns_typed_unique_form(pitches, bounds)[0]
least = _cabi.ns_typed_unique_workspace_bytes(pitches, bounds, G)[1]
tws = torch.empty(least * G // 8 + 1, dtype=torch.int64, device=dev)
uniq = _cabi.NsTypedUniqueOut(hb, in_place=False, with_inverse=False)
cases["ns_typed_unique/auto(form %d)" % auto] = lambda: _cabi.ns_typed_unique(hb, G, bounds, ws=tws, form=auto, result=uniq)
cases["ns_typed_unique/flat"] = lambda: _cabi.ns_typed_unique(hb, G, bounds, ws=tws, form=2, result=uniq)

ab_loop.run(cases)
