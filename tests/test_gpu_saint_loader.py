"""GraphSAINTRandomWalkLoader on the karate graph and on a random multigraph with sinks: every mini-batch's n_id equals the
restatement (roots through _cabi.seed_batches, walks through _cabi.random_walk, helpers_saint.node_list), its edge_index /
e_id equal helpers_induced.induced_rule applied to that n_id, attributes follow; ragged last launch, two epochs, a rebuilt
loader, the symmetric route, the pooled slabs, and with sample_coverage the two norms against the restated pre-sample."""
import numpy as np
import pytest
import torch

from helpers import load_karate
from helpers_induced import induced_rule
from helpers_saint import coverage_counts, node_list, norms, presample_launches, random_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, CALL0, STEPS, PREFETCH = 21, 300, 7, 3


def make(ei, n):
    from tch_geometric.transforms import Graph
    rs = np.random.default_rng(n)
    x = rs.standard_normal((n, 3)).astype(np.float32)
    w = rs.standard_normal((ei.shape[1], 2)).astype(np.float32)
    data = Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=n, x=torch.from_numpy(x).to(DEV),
                 edge_attr=torch.from_numpy(w).to(DEV))
    return dict(data=data, ei=ei, n=n, x=x, w=w)


@pytest.fixture(scope="module", params=["karate", "random"])
def case(request):
    if request.param == "karate":
        ei, n = load_karate()
        return dict(make(ei, n), B=6, T=2)
    return dict(make(random_graph(300, 2000, 0.1, seed=1), 300), B=20, T=3)


def build(k, **kw):
    from tch_geometric.loader import GraphSAINTRandomWalkLoader
    args = dict(prefetch=PREFETCH, seed=SEED, call_id0=CALL0, device=DEV)
    args.update(kw)
    return GraphSAINTRandomWalkLoader(k["data"], k["B"], k["T"], STEPS, **args)


def restated_n_id(k, loader, call_id):
    from tch_geometric import _cabi
    roots = _cabi.seed_batches(SEED, call_id, 1, k["B"], k["n"], DEV)
    walks = _cabi.random_walk(loader._walk_graph, roots[0], k["T"], 1.0, 1.0, SEED, call_id)
    return node_list(walks.cpu().numpy())


def check_batch(k, loader, mb, call_id, host):
    """one mini-batch against the restatement -> (n_id, CSC offsets of its edges)"""
    hp, hi, perm = host
    n_id = mb.n_id.cpu().numpy()
    assert mb.call_id == call_id and mb.batch_size == k["B"]
    assert np.array_equal(n_id, restated_n_id(k, loader, call_id))
    assert mb.num_nodes == n_id.size and len(set(n_id.tolist())) == n_id.size
    rows, cols, e = induced_rule(n_id, hp, hi)
    assert np.array_equal(mb.edge_index.cpu().numpy(), np.stack([rows, cols])) and mb.num_edges == rows.size
    e_id = mb.e_id.cpu().numpy()
    assert np.array_equal(e_id, perm[e])
    assert np.array_equal(k["ei"][0][e_id], n_id[rows]) and np.array_equal(k["ei"][1][e_id], n_id[cols])   # row = source
    assert np.array_equal(mb.x.cpu().numpy(), k["x"][n_id])
    assert np.array_equal(mb.edge_attr.cpu().numpy(), k["w"][e_id])
    assert mb.layer_offsets is None and mb.layer_nodes is None and mb.layer_edges is None
    return n_id, e


def host_of(loader):
    return tuple(t.cpu().numpy() for t in (loader.col_ptrs, loader.row_indices, loader.perm))


def test_two_epochs_ragged_launch_rebuilt_loader_and_pool(case):
    k = case
    loader = build(k)
    assert len(loader) == STEPS and loader.node_norm is None
    host = host_of(loader)
    epochs = []
    for epoch in range(2):
        sizes, seen = [], []
        for sb in loader.super_batches():
            sizes.append(len(sb))
            assert sb.call_id0 == CALL0 + epoch * STEPS + len(seen) and sb.num_nodes == sb.n_id.numel()
            for mb in sb:
                n_id, _ = check_batch(k, loader, mb, CALL0 + epoch * STEPS + len(seen), host)
                with pytest.raises(AttributeError):
                    mb.node_norm
                seen.append(n_id)
        assert sizes == [3, 3, 1]                                       # the ragged last launch
        if epoch == 0:
            assert loader.slab_allocations == 1
            slab_ptr = loader._pool[0]["nodes"].data_ptr()
        epochs.append(seen)
    assert any(not np.array_equal(a, b) for a, b in zip(*epochs))       # the epochs differ
    assert loader.slab_allocations == 1 and loader._pool[0]["nodes"].data_ptr() == slab_ptr   # later epochs reuse the slabs
    again = build(k)
    for epoch in range(2):                                              # a rebuilt loader repeats them
        got = [mb.n_id.cpu().numpy() for mb in again]
        assert len(got) == STEPS and all(np.array_equal(a, b) for a, b in zip(got, epochs[epoch]))
    it1, it2 = iter(loader), iter(loader)                               # two live iterators own a slab set each
    a, b = next(it1), next(it2)
    assert a.call_id == CALL0 + 2 * STEPS and b.call_id == CALL0 + 3 * STEPS and loader.slab_allocations == 2
    check_batch(k, loader, a, a.call_id, host)
    check_batch(k, loader, b, b.call_id, host)


@pytest.mark.parametrize("form", [1, 2])
def test_forms_agree(case, form):
    k = case
    want = [mb.n_id.cpu().numpy() for mb in build(k)]
    got = [mb.n_id.cpu().numpy() for mb in build(k, form=form)]
    assert len(got) == STEPS and all(np.array_equal(a, b) for a, b in zip(got, want))


def test_symmetric_route_equals_the_csr_route(case):
    k = case
    ei = np.concatenate([k["ei"], k["ei"][::-1]], axis=1)               # every edge both ways
    sym = dict(make(ei, k["n"]), B=k["B"], T=k["T"])
    a, b = build(sym), build(sym, symmetric=True)
    assert b._walk_graph is b._graph and a._walk_graph is not a._graph
    host = host_of(a)
    for j, (x, y) in enumerate(zip(a, b)):
        check_batch(sym, a, x, CALL0 + j, host)
        assert torch.equal(x.n_id, y.n_id) and torch.equal(x.edge_index, y.edge_index) and torch.equal(x.e_id, y.e_id)


def test_sample_coverage_norms(case):
    from tch_geometric.loader import SAINT_PRESAMPLE_CALL_ID0
    k = case
    coverage = 5
    loader = build(k, sample_coverage=coverage)
    hp, hi, perm = host = host_of(loader)
    E = hi.size
    # the pre-sample restated: whole launches of PREFETCH mini-batches from call id 1 << 62
    node_lists, edge_lists, sums = [], [], []
    for launch in range(loader.presampled_launches):
        total = 0
        for g in range(PREFETCH):
            n_id = restated_n_id(k, loader, SAINT_PRESAMPLE_CALL_ID0 + launch * PREFETCH + g)
            node_lists.append(n_id)
            edge_lists.append(induced_rule(n_id, hp, hi)[2])
            total += n_id.size
        sums.append(total)
    assert presample_launches(sums, k["n"], coverage) == loader.presampled_launches >= 2
    assert loader.presampled_batches == loader.presampled_launches * PREFETCH
    nc, ec = coverage_counts(node_lists, edge_lists, k["n"], E)
    want_n, want_e = norms(hp, nc, ec, loader.presampled_batches)
    got_n, got_e = loader.node_norm.cpu().numpy(), loader.edge_norm.cpu().numpy()
    assert np.array_equal(got_n.view(np.uint32), want_n.view(np.uint32))
    assert np.array_equal(got_e.view(np.uint32), want_e.view(np.uint32))
    assert loader.slab_allocations == 1
    for j, mb in enumerate(loader):                                     # the epoch's call ids are untouched by the pre-sample
        n_id, e = check_batch(k, loader, mb, CALL0 + j, host)
        assert np.array_equal(mb.node_norm.cpu().numpy(), want_n[n_id])
        assert np.array_equal(mb.edge_norm.cpu().numpy(), want_e[e])
    assert loader.slab_allocations == 1                                 # the epoch took the pre-sample's slab set
