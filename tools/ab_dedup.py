"""A/B of library builds on the node dedup operators INSIDE one process, on the same slabs and workspaces (why one process:
tools/ab_same_process.py): `python tools/ab_dedup.py parent.so parent.so new.so [--out FILE]` (paths relative to the repo
root; "-" = the default build).  Three alternating rounds, HIP events, ms per call.  Cases, on RMAT-20 with 16 edges per
node and seeds from seed_batches:
  ns_homo_unique, ns_homo_unique_grouped (identity groups)   flat form: 16 batches x 1 024 seeds x [15, 10] (169 984
      positions, the loader's shape); LDS form: 2 048 batches x 128 seeds x [5, 3] (2 688 positions)
  ns_typed_unique   one sampled hetero launch, set up as tools/bench_hetero_unique_loader.py's `dedup` section (SHIFT > 0:
      a smaller graph), in its auto form and forced flat
With the SAME build given first and second, the gap between those two medians is the noise floor of the run; every later
build's median is held against the first build's median + twice that gap.  Prints one JSON object."""
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tch-geometric_amd"))
from tch_geometric import _cabi  # noqa: E402
from tch_geometric.loader import HeteroNeighborLoader  # noqa: E402
from tch_geometric.transforms import HeteroGraph  # noqa: E402

dev = torch.device("cuda:0")
args = sys.argv[1:]
out_path = args.pop(args.index("--out") + 1) if "--out" in args else None
paths = [a for a in args if a != "--out"]
default, libs = _cabi.lib, []
for i, path in enumerate(paths):
    h = default if path == "-" else C.CDLL(os.path.join(ROOT, path))
    h.tg_version.restype = h.tg_last_error.restype = C.c_char_p
    libs.append(("%d:%s" % (i, path), h))

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

ms = {c: {name: [] for name, _ in libs} for c in cases}
for rnd in range(3):
    for name, h in libs:
        _cabi.lib = h
        for c, call in cases.items():
            for _ in range(3):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                call()
            e1.record()
            torch.cuda.synchronize()
            ms[c][name].append(e0.elapsed_time(e1) / 20)
_cabi.lib = default
res = {}
for c in cases:
    med = {name: round(statistics.median(v), 5) for name, v in ms[c].items()}
    entry = {"ms_per_call_median": med, "ms_per_call_rounds": {k: [round(x, 5) for x in v] for k, v in ms[c].items()}}
    if len(libs) >= 3 and paths[0] == paths[1]:
        (a, _), (b, _) = libs[0], libs[1]
        gap = abs(med[a] - med[b])
        entry["noise_floor_ms"] = round(gap, 5)
        entry["verdict"] = {name: "ok" if med[name] <= med[a] + 2 * gap else "slower by %.5f ms" % (med[name] - med[a])
                            for name, _ in libs[2:]}
    res[c] = entry
text = json.dumps(res, indent=1)
print(text)
if out_path:
    open(out_path, "w").write(text + "\n")
