"""The stream-order contract of include/tchgeo.h's first convention for the layer-wise pair: tg_ladies_count, tg_ladies_emit and
the wrappers Ladies.count / Ladies.emit are stream-ordered and never synchronise, allocate or free.  The detector is
helpers_stream's (a case runs behind a blocker on a side stream, over decoy inputs and zero-filled buffers); CASES is the
table tests/test_ladies_contract_cpu.py holds against include/tchgeo_ladies.h and _cabi_ladies.py."""
import pytest
import torch

import helpers_stream as hs
from helpers_stream import ASYNC, Case
from test_gpu_stream_order import _graph, _pick, _prefix, _sized, _view

pytestmark = pytest.mark.gpu
MODULES = ("tch_geometric._cabi_ladies",)


def _ladies_case(weighted):
    def make(dev):
        d = _graph(dev, "r10")
        g = torch.Generator().manual_seed(5)
        more = dict(nodes=torch.randperm(d["n"], generator=g)[:205].to(dev), node_ptr=torch.tensor([0, 40, 105, 205], device=dev))
        if weighted:
            more["w32"] = (d["w"] / 4.5).to(torch.float32)
        return _pick(d, "ptrs", "idx", **more)

    def chain(inp, T, totals):
        from tch_geometric import _cabi_ladies
        n, dev = inp["ptrs"].numel() - 1, inp["nodes"].device
        op = _cabi_ladies.Ladies(_view(inp), n, 128, 4096, 0, 64, 3, dev, weights=inp.get("w32"))
        n_nodes, n_edges, _, _, _, _ = op.count(inp["nodes"], inp["node_ptr"], 17, 300)
        if totals is None:
            totals = (int(n_nodes.sum()), int(n_edges.sum()))
        per_node = T.empty((3, max(totals[0], 1)), dtype=torch.int64, device=dev)
        trip = T.empty((3, max(totals[1], 1)), dtype=torch.int64, device=dev)
        ew = T.empty(max(totals[1], 1), dtype=torch.float32, device=dev)
        op.emit(_prefix(n_nodes), _prefix(n_edges), per_node[0], per_node[1], per_node[2], trip[0], trip[1], trip[2], ew)
        return (op.state, per_node, trip, ew), totals
    name = "ladies_weighted" if weighted else "ladies"
    remember, call = _sized(name, chain)
    return Case(name, ["tg_ladies_count", "tg_ladies_emit", "Ladies.count", "Ladies.emit"], ASYNC, remember(make), call,
                vary=["nodes"], modules=MODULES)


CASES = [_ladies_case(False), _ladies_case(True)]
EXEMPT = {}


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_stream_order(case):
    r = hs.check(case)
    print("%s: host enqueue %.3f ms, %d outputs" % (case.id, r["host_ms"], r["n_outputs"]))
