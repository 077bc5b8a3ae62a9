"""Same-process A/B of tg_ns_out.rows_prefilled: the default bench launch (RMAT-24, 16 384 batches of 1 024 seeds, [15, 10],
staged pipeline) on ONE set of slabs, the struct field on against off, three alternating rounds -- the kernels apart from
placement.  `python tools/ab_rows_prefilled.py`; G=<batches> for another launch size.  Per variant and round: ms per launch
(HIP events around four launches) and the per-stage HIP-event times of one more launch (tg_ns_win_stage_timing).  One JSON
line per (round, variant)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tch-geometric_amd"))
from tch_geometric import _cabi  # noqa: E402

dev = torch.device("cuda:0")
G, B, fan, scale = int(os.environ.get("G", 16384)), 1024, [15, 10], 24
n = 1 << scale
out = _cabi.NsBatchedOut(G, B, fan, dev)          # rows filled and marked
row, col = _cabi.rmat_edges(scale, n * 16, 0x5EED0000 + scale, dev)
ptrs, idx, _ = _cabi.coo_to_csx(row, col, n, n, True)
del row, col
g = _cabi.graph_view(ptrs, idx, indices32=idx.to(torch.int32), ptrs32=ptrs.to(torch.int32), max_degree="auto")
ws = _cabi.ns_homo_workspace(G, B, fan, dev, staged=True, graph=g)
seeds = _cabi.seed_batches(0xBA7C4, 0, G, B, n, dev)
_cabi.ns_win_tuning_set(staged=1, stage_parts=1)
assert out.struct().rows_prefilled == B + 1


class Off:
    """the same slabs, the field forced to 0: the launch writes `rows` (the same values) as before the field existed"""

    def __getattr__(self, k):
        return getattr(out, k)

    def struct(self):
        s = out.struct()
        s.rows_prefilled = 0
        return s


def launch(o):
    _cabi.ns_homo_batched(g, seeds, fan, 0, 0, o, ws=ws, form=1)


for rnd in range(3):
    for name, o in (("rows_written", Off()), ("rows_prefilled", out)):
        for _ in range(2):
            launch(o)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(4):
            launch(o)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 4
        _cabi.ns_win_stage_timing(True)
        launch(o)
        stages = _cabi.ns_win_stage_times()
        _cabi.ns_win_stage_timing(False)
        print(json.dumps({"round": rnd, "variant": name, "ms_per_launch": round(ms, 3),
                          "stage_ms": [(k, round(v, 3)) for k, v in stages]}), flush=True)
assert out.struct().rows_prefilled == B + 1 and torch.equal(out.rows[G - 1], torch.arange(out.rows.shape[1], device=dev) + B)
