"""NeighborLoader(labor=True) and LinkNeighborLoader(labor=True): every mini-batch equals the NumPy restatement of
TG_SAMPLER_LABOR (helpers_labor.py) under the mini-batch's call id, followed by the dedup rule (helpers_unique) and the
induced-subgraph rule (helpers_induced) where asked for; and on an R-MAT graph a mini-batch lists fewer distinct nodes."""
import numpy as np
import pytest
import torch

import helpers_link as hl
import orc
from helpers import load_karate
from helpers_induced import induced_rule
from helpers_labor import SAMPLER_LABOR, SAMPLER_LABOR_SHARED, labor_ns_homo
from helpers_unique import unique_rule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FAN, BATCH, PREFETCH, SEED, CALL0 = [3, 2], 8, 3, 21, 500
WINDOW = (0, 2 ** 62)


@pytest.fixture(scope="module")
def karate():
    from tch_geometric.transforms import Graph
    ei, n = load_karate()
    rs = np.random.default_rng(17)
    time = rs.integers(0, 40, ei.shape[1]).astype(np.int64)
    x = rs.standard_normal((n, 5)).astype(np.float32)
    data = Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=n, x=torch.from_numpy(x).to(DEV),
                 time=torch.from_numpy(time).to(DEV))
    ptrs, idx, perm = orc.to_csc(ei, n)
    input_time = rs.integers(5, 45, n).astype(np.int64)
    return dict(data=data, n=n, ei=ei, time=time, x=x, ptrs=ptrs, idx=idx, perm=perm, ts_csc=time[perm], input_time=input_time)


def _loader(k, **kw):
    from tch_geometric.loader import NeighborLoader
    return NeighborLoader(k["data"], FAN, batch_size=BATCH, prefetch=PREFETCH, seed=SEED, call_id0=CALL0, device=DEV,
                          labor=True, **kw)


@pytest.mark.parametrize("dependency", [False, True])
@pytest.mark.parametrize("shuffle", [False, True])
def test_forest_equals_the_restatement_over_two_epochs(karate, dependency, shuffle):
    from tch_geometric import _cabi
    k = karate
    loader = _loader(k, layer_dependency=dependency, shuffle=shuffle)
    sampler = SAMPLER_LABOR_SHARED if dependency else SAMPLER_LABOR
    assert loader.sampler == (_cabi.SAMPLER_LABOR_SHARED if dependency else _cabi.SAMPLER_LABOR) == sampler
    assert len(loader) == 5                                 # 34 seeds: four full mini-batches and a ragged one of 2
    orders = []
    for epoch in range(2):
        seen = []
        for j, b in enumerate(loader):
            B = b.batch_size
            assert B == (8 if j < 4 else 2) and b.call_id == CALL0 + epoch * 5 + j
            seeds = b.n_id[:B].cpu().numpy()
            seen += seeds.tolist()
            s, r, c, e, lo, _, _ = labor_ns_homo(k["ptrs"], k["idx"], None, seeds, FAN, SEED, b.call_id, sampler)
            assert torch.equal(b.n_id.cpu(), torch.from_numpy(s)) and b.layer_offsets == lo
            assert torch.equal(b.edge_index.cpu(), torch.from_numpy(np.stack([r, c])))
            assert torch.equal(b.e_id.cpu(), torch.from_numpy(k["perm"][e]))
            assert np.array_equal(b.x.cpu().numpy(), k["x"][s])
        assert sorted(seen) == list(range(k["n"])) and (seen != list(range(k["n"]))) == shuffle
        orders.append(seen)
    assert (orders[0] != orders[1]) == shuffle
    assert len(loader._time_ws) == 2                        # one workspace per launch shape (full / ragged), kept


@pytest.mark.parametrize("induced", [False, True])
def test_unique_and_induced_equal_the_rules_behind_the_restatement(karate, induced):
    k = karate
    loader = _loader(k, unique=True, induced=induced, shuffle=True)
    n = 0
    for j, b in enumerate(loader):
        B = BATCH if j < 4 else 2
        seeds = b.n_id[:b.batch_size].cpu().numpy()        # distinct seeds lead; karate's inputs are distinct
        assert b.batch_size == B
        s, r, c, e, lo, _, _ = labor_ns_homo(k["ptrs"], k["idx"], None, seeds, FAN, SEED, CALL0 + j)
        nodes, _, rows_u, cols_u, layer_nodes = unique_rule(s, r, c, [x[0] for x in lo])
        assert torch.equal(b.n_id.cpu(), torch.from_numpy(nodes)) and b.layer_nodes == layer_nodes
        assert np.array_equal(b.x.cpu().numpy(), k["x"][nodes])
        if induced:
            rows, cols, eidx = induced_rule(nodes, k["ptrs"], k["idx"])
            assert np.array_equal(b.edge_index.cpu().numpy(), np.stack([rows, cols]))
            assert np.array_equal(b.e_id.cpu().numpy(), k["perm"][eidx])
        else:
            assert np.array_equal(b.edge_index.cpu().numpy(), np.stack([rows_u, cols_u]))
            assert np.array_equal(b.e_id.cpu().numpy(), k["perm"][e])
        n += 1
    assert n == 5


def test_with_time_attr_the_filter_is_on_the_real_times(karate):
    k = karate
    loader = _loader(k, time_attr="time", input_time=torch.from_numpy(k["input_time"]), time_window=(0, 15), shuffle=True)
    n_edges = 0
    for j, b in enumerate(loader):
        B = b.batch_size
        seeds, t0 = b.n_id[:B].cpu().numpy(), b.input_time.cpu().numpy()
        assert np.array_equal(t0, k["input_time"][seeds])
        s, r, c, e, lo, _, st = labor_ns_homo(k["ptrs"], k["idx"], k["ts_csc"], seeds, FAN, SEED, CALL0 + j, SAMPLER_LABOR, t0, 1,
                                              False, (0, 15))
        assert torch.equal(b.n_id.cpu(), torch.from_numpy(s)) and b.layer_offsets == lo
        assert torch.equal(b.edge_index.cpu(), torch.from_numpy(np.stack([r, c])))
        assert torch.equal(b.e_id.cpu(), torch.from_numpy(k["perm"][e]))
        assert torch.equal(b.node_time.cpu(), torch.from_numpy(st))
        age = st[c] - k["time"][b.e_id.cpu().numpy()]
        assert np.all((age >= 0) & (age <= 15))
        n_edges += len(e)
    assert n_edges > 0


@pytest.mark.parametrize("unique", [False, True], ids=["forest", "unique"])
def test_link_loader_passes_the_option_through(karate, unique):
    from tch_geometric.loader import LinkNeighborLoader
    k = karate
    loader = LinkNeighborLoader(k["data"], FAN, neg_sampling_ratio=1, try_count=4, batch_size=30, prefetch=2, seed=SEED,
                                call_id0=CALL0, device=DEV, unique=unique, labor=True, layer_dependency=True)
    assert loader.labor and loader.layer_dependency
    eli = loader.edge_label_index.cpu().numpy()
    E_all = eli.shape[1]
    n = 0
    for j, mb in enumerate(loader):
        positions = np.arange(j * 30, min((j + 1) * 30, E_all))
        rows, _ = hl.seed_rows(k["ptrs"], k["idx"], eli[0][positions][None], eli[1][positions][None], 1, loader.mode,
                               loader.try_count, SEED, CALL0 + j, k["n"])
        s, r, c, e, lo, _, _ = labor_ns_homo(k["ptrs"], k["idx"], None, rows[0], FAN, SEED, CALL0 + j, SAMPLER_LABOR_SHARED)
        if unique:
            s, _, r, c, _ = unique_rule(s, r, c)
        assert np.array_equal(mb.n_id.cpu().numpy(), s)
        assert np.array_equal(mb.edge_index.cpu().numpy(), np.stack([r, c]))
        n += 1
    assert n == len(loader) == -(-E_all // 30) and E_all % 30 != 0     # the last mini-batch is ragged


def test_fewer_distinct_nodes_on_rmat():
    """R-MAT scale 12 x 16 edges, [10, 10], 256 seeds per mini-batch, unique=True: the mean n_id length.
    The NumPy restatement of this very loop (same graph and seeds; labor_hop with one call id per mini-batch against
    labor_hop with a call id of its own for every frontier slot, which is an independent uniform k-subset per slot) gave
    1 881.5 distinct nodes per mini-batch with independent draws, 1 254.25 with shared variates (0.67x) and 1 214.25 with
    layer_dependency.  Only "smaller" is asserted."""
    from tch_geometric.loader import NeighborLoader
    from tch_geometric.transforms import Graph
    n = 1 << 12
    row, col = orc.rmat_edges(12, n * 16, 0x5EED)
    data = Graph(edge_index=torch.from_numpy(np.stack([row, col])).to(DEV), num_nodes=n)
    nodes = torch.from_numpy(np.random.default_rng(1).permutation(n)[:1024])
    mean = {}
    for labor in (False, True):
        loader = NeighborLoader(data, [10, 10], input_nodes=nodes, batch_size=256, prefetch=4, seed=3, device=DEV, unique=True,
                                labor=labor)
        sizes = [b.num_nodes for b in loader]
        assert len(sizes) == 4
        mean[labor] = sum(sizes) / len(sizes)
    print("distinct nodes per mini-batch: uniform %.1f, labor %.1f" % (mean[False], mean[True]))
    assert mean[True] < mean[False]
