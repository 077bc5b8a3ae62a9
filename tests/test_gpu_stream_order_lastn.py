"""The stream-order contract of include/tchgeo.h's first convention for the streaming last-k neighbour state: tg_lastn_reset,
tg_lastn_insert (both forms), tg_lastn_sample, tg_lastn_replay and the wrappers LastN.reset / .insert / .sample / .replay are
stream-ordered and never synchronise, allocate or free.  The detector is helpers_stream's (a case runs behind a blocker on a
side stream, over decoy inputs and zero-filled buffers); CASES is the table tests/test_lastn_contract_cpu.py holds against
include/tchgeo_lastn.h and _cabi_lastn.py."""
import pytest
import torch

import helpers_stream as hs
from helpers_stream import ASYNC, Case

pytestmark = pytest.mark.gpu
MODULES = ("tch_geometric._cabi_lastn",)
N, K = 500, 6


def _inputs(n_events):
    def make(dev):
        g = torch.Generator().manual_seed(7)
        return dict(src=torch.randint(0, N, (n_events,), generator=g).to(dev), dst=torch.randint(0, N, (n_events,), generator=g).to(dev),
                    seeds=torch.randint(0, N, (4, 33), generator=g).to(dev))
    return make


def _slabs(ln, out):
    return (ln.state, ln.status, out.samples, out.cols, out.edge_index, out.layer_offsets, out.counts)


def _insert_sample_case(name, n_events, form):
    def call(inp, T):
        from tch_geometric import _cabi_lastn
        ln = _cabi_lastn.LastN(N, K, inp["src"].device)              # reset
        half = n_events // 2
        ln.insert(inp["src"][:half].contiguous(), inp["dst"][:half].contiguous(), form=form)
        ln.insert(inp["src"][half:].contiguous(), inp["dst"][half:].contiguous(), e_base=half, symmetric=False, form=form)
        return _slabs(ln, ln.sample(inp["seeds"], [3, 2]))
    return Case(name, ["tg_lastn_reset", "tg_lastn_insert", "tg_lastn_sample", "LastN.reset", "LastN.insert", "LastN.sample"],
                ASYNC, _inputs(n_events), call, vary=["src", "dst", "seeds"], modules=MODULES)


def _replay_case(name, n_events, step):
    def call(inp, T):
        from tch_geometric import _cabi_lastn
        ln = _cabi_lastn.LastN(N, K, inp["src"].device)
        G = -(-n_events // step)
        seeds = inp["seeds"].reshape(-1)[:G * 8].reshape(G, 8).contiguous()
        return _slabs(ln, ln.replay(inp["src"], inp["dst"], seeds, [3, 2], step))
    return Case(name, ["tg_lastn_reset", "tg_lastn_replay", "LastN.reset", "LastN.replay"], ASYNC, _inputs(n_events), call,
                vary=["src", "dst", "seeds"], modules=MODULES)


CASES = [_insert_sample_case("lastn_lds", 900, 1), _insert_sample_case("lastn_grid", 900, 2),
         _replay_case("lastn_replay", 900, 100), _replay_case("lastn_replay_grid", 5000, 2500)]
EXEMPT = {}


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_stream_order(case):
    r = hs.check(case)
    print("%s: host enqueue %.3f ms, %d outputs" % (case.id, r["host_ms"], r["n_outputs"]))
