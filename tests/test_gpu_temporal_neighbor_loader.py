"""NeighborLoader with time_attr / input_time: "last" equals the NumPy restatement of TG_SAMPLER_RECENT, "uniform" equals
_cabi.ns_homo_batched under the same filter, seed and call id; epochs are reproducible, attributes are gathered as in the
untimed loader, and a default-argument loader yields what the plain batched launch yields."""
import numpy as np
import pytest
import torch

import orc
from helpers import load_karate
from helpers_recent import recent_ns_homo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FAN, BATCH, PREFETCH, SEED, CALL0 = [3, 2], 8, 3, 21, 500
WINDOW = (0, 2 ** 62)


@pytest.fixture(scope="module")
def karate():
    """karate with a seeded int64 time per edge (edge_index order), features, and one time per node as input_time"""
    from tch_geometric.transforms import Graph
    ei, n = load_karate()
    rs = np.random.default_rng(17)
    time = rs.integers(0, 40, ei.shape[1]).astype(np.int64)
    x = rs.standard_normal((n, 5)).astype(np.float32)
    ea = rs.standard_normal((ei.shape[1], 2)).astype(np.float32)
    data = Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=n, x=torch.from_numpy(x).to(DEV),
                 edge_attr=torch.from_numpy(ea).to(DEV), time=torch.from_numpy(time).to(DEV))
    ptrs, idx, perm = orc.to_csc(ei, n)
    input_time = rs.integers(5, 45, n).astype(np.int64)
    return dict(data=data, n=n, ei=ei, time=time, x=x, ea=ea, ptrs=ptrs, idx=idx, perm=perm, ts_csc=time[perm],
                input_time=input_time)


def _loader(k, strategy, **kw):
    from tch_geometric.loader import NeighborLoader
    return NeighborLoader(k["data"], FAN, batch_size=BATCH, prefetch=PREFETCH, seed=SEED, call_id0=CALL0, time_attr="time",
                          input_time=torch.from_numpy(k["input_time"]), temporal_strategy=strategy, device=DEV, **kw)


def _epoch(loader):
    out = []
    for b in loader:
        out.append(dict(n_id=b.n_id.cpu(), edge_index=b.edge_index.cpu(), e_id=b.e_id.cpu(), lo=b.layer_offsets,
                        input_time=b.input_time.cpu(), node_time=b.node_time.cpu(), x=b.x.cpu(), edge_attr=b.edge_attr.cpu(),
                        call_id=b.call_id, batch_size=b.batch_size))
    return out


def _roots(cols, n_seeds, n_nodes):
    root = np.arange(n_nodes)
    for e, c in enumerate(cols):                            # rows[e] = n_seeds + e: parents come first
        root[n_seeds + e] = root[c]
    return root


@pytest.mark.parametrize("shuffle", [False, True])
def test_last_equals_the_restatement(karate, shuffle):
    k = karate
    loader = _loader(k, "last", shuffle=shuffle)
    batches = _epoch(loader)
    assert len(batches) == len(loader) == 5                 # 34 seeds: four full mini-batches and a ragged one of 2
    seen = []
    for j, b in enumerate(batches):
        B = b["batch_size"]
        assert B == (8 if j < 4 else 2) and b["call_id"] == CALL0 + j
        seeds, t0 = b["n_id"][:B].numpy(), b["input_time"].numpy()
        assert np.array_equal(t0, k["input_time"][seeds])   # input_time is sliced and shuffled with input_nodes
        seen += seeds.tolist()
        s, r, c, e, lo, counts, st = recent_ns_homo(k["ptrs"], k["idx"], k["ts_csc"], seeds, FAN, t0, 1, False, WINDOW)
        assert torch.equal(b["n_id"], torch.from_numpy(s)) and b["lo"] == lo
        assert torch.equal(b["edge_index"], torch.from_numpy(np.stack([r, c])))
        assert torch.equal(b["e_id"], torch.from_numpy(k["perm"][e]))
        assert torch.equal(b["node_time"], torch.from_numpy(st))
        # e_id maps back to edges of the source graph no later than the root's time; node_time is the root's everywhere
        root = _roots(c, B, len(s))
        assert np.array_equal(st, t0[root])
        assert np.all(k["time"][b["e_id"].numpy()] <= t0[root[r]])
        assert np.array_equal(k["ei"][0][b["e_id"].numpy()], s[r]) and np.array_equal(k["ei"][1][b["e_id"].numpy()], s[c])
        assert np.array_equal(b["x"].numpy(), k["x"][s]) and np.array_equal(b["edge_attr"].numpy(), k["ea"][b["e_id"].numpy()])
    assert sorted(seen) == list(range(k["n"]))
    assert (seen != list(range(k["n"]))) == shuffle


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("replace", [False, True])
def test_uniform_equals_the_batched_launch_under_the_same_filter(karate, replace, shuffle):
    from tch_geometric import _cabi
    k = karate
    batches = _epoch(_loader(k, "uniform", replace=replace, shuffle=shuffle))
    seen = torch.cat([b["n_id"][:b["batch_size"]] for b in batches]).tolist()
    assert sorted(seen) == list(range(k["n"])) and (seen != list(range(k["n"]))) == shuffle
    P, I = torch.from_numpy(k["ptrs"]).to(DEV), torch.from_numpy(k["idx"]).to(DEV)
    g = _cabi.graph_view(P, I, timestamps=torch.from_numpy(k["ts_csc"]).to(DEV))
    for j, b in enumerate(batches):
        B = b["batch_size"]
        seeds = b["n_id"][:B].to(DEV).reshape(1, B)             # the epoch's order, shuffled or not
        assert torch.equal(b["input_time"], torch.from_numpy(k["input_time"])[b["n_id"][:B]])   # sliced with the seeds
        st = b["input_time"].to(DEV).reshape(1, B)
        out = _cabi.NsBatchedOut(1, B, FAN, DEV, with_states=True)
        _cabi.ns_homo_batched(g, seeds, FAN, SEED, CALL0 + j, out, sampler=1 if replace else 0,
                              filter_mode=_cabi.FILTER_RELATIVE, forward=False, window=WINDOW, seeds_state=st)
        torch.cuda.synchronize()
        s, r, c, e, lo = out.batch(0)
        assert torch.equal(b["n_id"], s.cpu()) and b["lo"] == lo
        assert torch.equal(b["edge_index"], torch.stack([r, c]).cpu())
        assert torch.equal(b["e_id"], torch.from_numpy(k["perm"])[e.cpu()])
        assert torch.equal(b["node_time"], out.states[0, :len(s)].cpu())
        # ... which is the oracle's under that filter
        o = orc.ns_homo(k["ptrs"], k["idx"], seeds[0].cpu().numpy(), FAN, orc.rng_philox(SEED, CALL0 + j),
                        sampler=1 if replace else 0, filter_mode=1, forward=False, window=WINDOW, timestamps=k["ts_csc"],
                        inputs_state=st[0].cpu().numpy())
        assert np.array_equal(b["n_id"].numpy(), o[0]) and np.array_equal(b["e_id"].numpy(), k["perm"][o[3]])


@pytest.mark.parametrize("strategy", ["last", "uniform"])
def test_epochs_are_reproducible_and_windows_hold(karate, strategy):
    k = karate
    a = _epoch(_loader(k, strategy, shuffle=True, time_window=(0, 10)))
    b = _epoch(_loader(k, strategy, shuffle=True, time_window=(0, 10)))
    assert len(a) == len(b) == 5
    for x, y in zip(a, b):
        for key in ("n_id", "edge_index", "e_id", "input_time", "node_time", "x", "edge_attr"):
            assert torch.equal(x[key], y[key]), key
        assert x["lo"] == y["lo"]
        age = x["node_time"][x["edge_index"][1]].numpy() - k["time"][x["e_id"].numpy()]
        assert np.all((age >= 0) & (age <= 10))
    assert sum(len(x["e_id"]) for x in a) > 0


def test_default_arguments_are_the_loader_of_before(karate):
    """all four temporal arguments at their defaults: the mini-batches are the plain batched launch's, and carry no times"""
    from tch_geometric import _cabi
    from tch_geometric.loader import NeighborLoader
    k = karate
    loader = NeighborLoader(k["data"], FAN, batch_size=BATCH, prefetch=PREFETCH, seed=SEED, call_id0=CALL0, device=DEV)
    assert loader.temporal is False and loader.sampler == _cabi.SAMPLER_UNIFORM
    P, I = torch.from_numpy(k["ptrs"]).to(DEV), torch.from_numpy(k["idx"]).to(DEV)
    g = _cabi.graph_view(P, I)
    n = 0
    for j, b in enumerate(loader):
        B = b.batch_size
        seeds = torch.arange(j * BATCH, j * BATCH + B, device=DEV).reshape(1, B)
        out = _cabi.NsBatchedOut(1, B, FAN, DEV)
        _cabi.ns_homo_batched(g, seeds, FAN, SEED, CALL0 + j, out)
        torch.cuda.synchronize()
        s, r, c, e, lo = out.batch(0)
        assert torch.equal(b.n_id, s) and torch.equal(b.edge_index, torch.stack([r, c])) and b.layer_offsets == lo
        assert torch.equal(b.e_id.cpu(), torch.from_numpy(k["perm"])[e.cpu()])
        for name in ("input_time", "node_time"):             # the graph has no such attributes: nothing by these names
            with pytest.raises(AttributeError):
                getattr(b, name)
        assert torch.equal(b.time.cpu(), torch.from_numpy(k["time"])[b.e_id.cpu()])   # `time` is an edge attribute like any other
        n += 1
    assert n == 5


def test_an_untimed_loader_hands_out_the_graphs_own_time_attributes(karate):
    """a graph may carry node attributes called node_time / input_time (examples/_data.py's temporal dataset does): from
    a loader without time_attr they are gathered like any other attribute, as before; a temporal loader, whose mini-batches
    have fields of those names, refuses such a graph"""
    from tch_geometric.loader import LinkNeighborLoader, NeighborLoader
    from tch_geometric.transforms import Graph
    k = karate
    rs = np.random.default_rng(23)
    node_time, input_time = rs.integers(0, 50, k["n"]), rs.integers(0, 50, (k["n"], 2))
    data = Graph(edge_index=torch.from_numpy(k["ei"]).to(DEV), num_nodes=k["n"], time=torch.from_numpy(k["time"]).to(DEV),
                 node_time=torch.from_numpy(node_time).to(DEV), input_time=torch.from_numpy(input_time).to(DEV))
    n = 0
    for b in NeighborLoader(data, FAN, batch_size=BATCH, prefetch=PREFETCH, seed=SEED, device=DEV):
        s = b.n_id.cpu().numpy()
        assert np.array_equal(b.node_time.cpu().numpy(), node_time[s])
        assert np.array_equal(b.input_time.cpu().numpy(), input_time[s])
        assert dict(b.tensor_items())["node_time"] is not None
        n += 1
    assert n == 5
    for b in LinkNeighborLoader(data, FAN, batch_size=50, prefetch=2, seed=SEED, device=DEV):
        assert np.array_equal(b.node_time.cpu().numpy(), node_time[b.n_id.cpu().numpy()])
    with pytest.raises(ValueError, match="node_time|input_time"):
        NeighborLoader(data, FAN, time_attr="time", input_time=torch.from_numpy(k["input_time"]), device=DEV)
