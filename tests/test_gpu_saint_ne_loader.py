"""GraphSAINTNodeLoader and GraphSAINTEdgeLoader on a random multigraph with sinks: every mini-batch's n_id equals the
NumPy restatement (helpers_saint_ne) under the stated call ids, its edge_index / e_id equal helpers_induced.induced_rule
applied to that n_id, attributes follow; ragged last launch, two epochs, prefetch 1 against 4, two live iterators, the
pooled slabs, with sample_coverage the two norms against the restated pre-sample, and the symmetric route."""
import numpy as np
import pytest
import torch

import helpers_saint_ne as H
from helpers_induced import induced_rule
from helpers_saint import coverage_counts, norms, presample_launches, random_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, CALL0, STEPS, PREFETCH, B, N = 23, 500, 7, 3, 40, 300


def make(ei, n):
    from tch_geometric.transforms import Graph
    rs = np.random.default_rng(n)
    x = rs.standard_normal((n, 3)).astype(np.float32)
    w = rs.standard_normal((ei.shape[1], 2)).astype(np.float32)
    data = Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=n, x=torch.from_numpy(x).to(DEV),
                 edge_attr=torch.from_numpy(w).to(DEV))
    return dict(data=data, ei=ei, n=n, x=x, w=w)


@pytest.fixture(scope="module")
def graph():
    return make(random_graph(N, 2000, 0.1, seed=1), N)


def build(k, which, **kw):
    import tch_geometric
    args = dict(prefetch=PREFETCH, seed=SEED, call_id0=CALL0, device=DEV)
    args.update(kw)
    return getattr(tch_geometric, {"node": "GraphSAINTNodeLoader", "edge": "GraphSAINTEdgeLoader"}[which])(k["data"], B, STEPS, **args)


def host_of(loader):
    return tuple(t.cpu().numpy() for t in (loader.col_ptrs, loader.row_indices, loader.perm))


def restated_n_id(k, loader, which, call_id):
    """the node list of one mini-batch from the loader's own arrays"""
    hp, hi, _ = host_of(loader)
    if which == "node":
        lists, status = H.node_lists(hi, 1, B, SEED, call_id, k["n"])
    else:
        csr = tuple(t.cpu().numpy() for t in loader._out._keep[:2])
        lists, status = H.edge_lists((hp, hi), H.nonempty(hp), csr, H.nonempty(csr[0]), 1, B, SEED, call_id, k["n"])
    assert status == 0
    return lists[0]


def check_batch(k, loader, which, mb, call_id, host):
    """one mini-batch against the restatement -> (n_id, CSC offsets of its edges)"""
    hp, hi, perm = host
    n_id = mb.n_id.cpu().numpy()
    assert mb.call_id == call_id and mb.batch_size == B
    assert np.array_equal(n_id, restated_n_id(k, loader, which, call_id))
    assert mb.num_nodes == n_id.size and len(set(n_id.tolist())) == n_id.size
    rows, cols, e = induced_rule(n_id, hp, hi)
    assert np.array_equal(mb.edge_index.cpu().numpy(), np.stack([rows, cols])) and mb.num_edges == rows.size
    e_id = mb.e_id.cpu().numpy()
    assert np.array_equal(e_id, perm[e])
    assert np.array_equal(k["ei"][0][e_id], n_id[rows]) and np.array_equal(k["ei"][1][e_id], n_id[cols])   # row = source
    assert np.array_equal(mb.x.cpu().numpy(), k["x"][n_id])
    assert np.array_equal(mb.edge_attr.cpu().numpy(), k["w"][e_id])
    return n_id, e


@pytest.mark.parametrize("which", ["node", "edge"])
def test_two_epochs_ragged_launch_prefetch_iterators_and_pool(graph, which):
    k = graph
    loader = build(k, which)
    assert len(loader) == STEPS and loader.node_norm is None and loader.positions == (B if which == "node" else 2 * B)
    if which == "edge":                                                 # the lists: the non-empty majors, made once
        assert np.array_equal(loader.cols.cpu().numpy(), H.nonempty(loader.col_ptrs.cpu().numpy()))
        assert np.array_equal(loader.rows.cpu().numpy(), H.nonempty(loader._out._keep[0].cpu().numpy()))
        assert loader.rows.numel() < N and loader._out is not loader._graph
    host = host_of(loader)
    epochs = []
    for epoch in range(2):
        sizes, seen = [], []
        for sb in loader.super_batches():
            sizes.append(len(sb))
            assert sb.call_id0 == CALL0 + epoch * STEPS + len(seen) and sb.num_nodes == sb.n_id.numel()
            for mb in sb:
                n_id, _ = check_batch(k, loader, which, mb, CALL0 + epoch * STEPS + len(seen), host)
                with pytest.raises(AttributeError):
                    mb.node_norm
                seen.append(n_id)
        assert sizes == [3, 3, 1]                                       # the ragged last launch
        if epoch == 0:
            assert loader.slab_allocations == 1
        epochs.append(seen)
    assert any(not np.array_equal(a, b) for a, b in zip(*epochs))       # the epochs differ
    assert loader.slab_allocations == 1                                 # epoch 2 reused the slabs
    for prefetch in (1, 4):                                             # the launch width changes no mini-batch
        got = [mb.n_id.cpu().numpy() for mb in build(k, which, prefetch=prefetch)]
        assert len(got) == STEPS and all(np.array_equal(a, b) for a, b in zip(got, epochs[0]))
    for form in (1, 2):
        got = [mb.n_id.cpu().numpy() for mb in build(k, which, form=form)]
        assert all(np.array_equal(a, b) for a, b in zip(got, epochs[0]))
    it1, it2 = iter(loader), iter(loader)                               # two live iterators own a slab set each
    a, b = next(it1), next(it2)
    assert a.call_id == CALL0 + 2 * STEPS and b.call_id == CALL0 + 3 * STEPS and loader.slab_allocations == 2
    check_batch(k, loader, which, a, a.call_id, host)
    check_batch(k, loader, which, b, b.call_id, host)


@pytest.mark.parametrize("which", ["node", "edge"])
def test_sample_coverage_norms(graph, which):
    from tch_geometric.loader import SAINT_PRESAMPLE_CALL_ID0
    k = graph
    coverage = 2
    loader = build(k, which, sample_coverage=coverage)
    hp, hi, perm = host = host_of(loader)
    node_lists, edge_lists, sums = [], [], []
    for launch in range(loader.presampled_launches):                    # whole launches of PREFETCH from call id 1 << 62
        total = 0
        for g in range(PREFETCH):
            n_id = restated_n_id(k, loader, which, SAINT_PRESAMPLE_CALL_ID0 + launch * PREFETCH + g)
            node_lists.append(n_id)
            edge_lists.append(induced_rule(n_id, hp, hi)[2])
            total += n_id.size
        sums.append(total)
    assert presample_launches(sums, k["n"], coverage) == loader.presampled_launches >= 2
    assert loader.presampled_batches == loader.presampled_launches * PREFETCH
    nc, ec = coverage_counts(node_lists, edge_lists, k["n"], hi.size)
    want_n, want_e = norms(hp, nc, ec, loader.presampled_batches)
    got_n, got_e = loader.node_norm.cpu().numpy(), loader.edge_norm.cpu().numpy()
    assert np.array_equal(got_n.view(np.uint32), want_n.view(np.uint32))
    assert np.array_equal(got_e.view(np.uint32), want_e.view(np.uint32))
    assert loader.slab_allocations == 1
    for j, mb in enumerate(loader):                                     # the epoch's call ids are untouched by the pre-sample
        n_id, e = check_batch(k, loader, which, mb, CALL0 + j, host)
        assert np.array_equal(mb.node_norm.cpu().numpy(), want_n[n_id])
        assert np.array_equal(mb.edge_norm.cpu().numpy(), want_e[e])
    assert loader.slab_allocations == 1                                 # the epoch took the pre-sample's slab set
    import tch_geometric
    from tch_geometric.transforms import Graph
    hidden = Graph(edge_index=k["data"].edge_index, num_nodes=N, node_norm=torch.zeros(N, device=DEV))
    with pytest.raises(ValueError, match="node_norm"):
        type(loader)(hidden, B, STEPS, sample_coverage=coverage, device=DEV)
    assert isinstance(loader, tch_geometric.loader._GraphSAINTLoader)


def test_symmetric_equals_the_explicit_two_view_call(graph):
    """on a symmetrised graph the CSC is its own CSR: symmetric=True (one view, one list, both sides) gives the mini-batches
    of the route that builds the CSR -- and equals the C ABI called with the CSC and its list twice"""
    from tch_geometric import _cabi
    k = graph
    ei = np.concatenate([k["ei"], k["ei"][::-1]], axis=1)               # every edge both ways
    sym = make(ei, N)
    a, b = build(sym, "edge"), build(sym, "edge", symmetric=True)
    assert b._out is b._graph and b.rows is b.cols and a._out is not a._graph
    assert torch.equal(a.cols, a.rows) and torch.equal(a.cols, b.cols)
    host = host_of(a)
    got = []
    for j, (x, y) in enumerate(zip(a, b)):
        check_batch(sym, a, "edge", x, CALL0 + j, host)
        assert torch.equal(x.n_id, y.n_id) and torch.equal(x.edge_index, y.edge_index) and torch.equal(x.e_id, y.e_id)
        got.append(y.n_id)
    nodes, counts = _cabi.saint_edge_nodes(b._graph, b.cols, b._graph, b.cols, B, STEPS, SEED, CALL0, id_bound=N)
    torch.cuda.synchronize()
    for j in range(STEPS):
        assert torch.equal(nodes[j, :int(counts[j])], got[j])
