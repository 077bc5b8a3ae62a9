"""SketchData and SubgraphSketchLoader: the sketch and every mini-batch's integers equal the restatement (helpers_sketch) on the
CSC; `structure` and the cardinalities equal a float64 NumPy evaluation of the same formulas from the same integers within a
bound derived from float32's unit roundoff; two epochs, prefetch 1 against 4, shuffling with drop_last, two live iterators."""
import math

import numpy as np
import pytest
import torch

import helpers_sketch as hk
from helpers_induced import csc_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, B, L, H, NP, P, SEED = 300, 16, 100, 2, 128, 8, 11
MREG, EPS = 1 << P, 2.0 ** -24


@pytest.fixture(scope="module")
def world():
    from tch_geometric import SketchData
    from tch_geometric.transforms import Graph
    rs = np.random.default_rng(8)
    half = np.concatenate([rs.integers(0, N - 1, (2, 700)), np.stack([np.full(200, 7), rs.integers(0, N - 1, 200)]),
                           [[0, 0, 4], [1, 1, 4]]], axis=1)              # a hub, a parallel edge, a self loop; N - 1 is isolated
    ei = np.concatenate([half, half[::-1]], axis=1).astype(np.int64)     # symmetric
    sd = SketchData(Graph(edge_index=torch.from_numpy(ei).to(DEV), num_nodes=N), H, NP, P, SEED, device=DEV)
    ptrs, indices, _ = csc_of(ei, N)
    hops = [hk.init(N, NP, P, SEED)]
    for _ in range(H):
        hops.append(hk.propagate(ptrs, indices, *hops[-1])[:2])
    links = rs.integers(0, N, (2, L)).astype(np.int64)   # 100 links: 6 mini-batches of 16 and a ragged one of 4
    links[:, :3] = [[0, 7, 4], [1, N - 1, 4]]            # a parallel edge, the hub against the isolated vertex, u == v
    return dict(sd=sd, hops=hops, links=links, label=(np.arange(L) % 2).astype(np.float32), ref=hk.links(hops, links[0], links[1]))


def loader(w, **kw):
    from tch_geometric import SubgraphSketchLoader
    kw = dict(dict(edge_label_index=torch.from_numpy(w["links"]), edge_label=torch.from_numpy(w["label"]), batch_size=B,
                   prefetch=4), **kw)
    return SubgraphSketchLoader(w["sd"], **kw)


def test_the_sketch_and_its_cardinalities(world):
    sd = world["sd"]
    assert np.array_equal(sd.sketch.cpu().numpy().view(np.uint32), np.stack([hk.pack(M, R) for M, R in world["hops"]]))
    for hop in range(H + 1):
        R = world["hops"][hop][1]
        want = hk.card([hk.registers(r)[0] for r in R], [hk.registers(r)[1] for r in R], MREG)
        got = sd.cardinality(hop).cpu().numpy()
        assert got.dtype == np.float32 and np.all(np.abs(got - want) <= 5 * EPS * np.maximum(want, MREG * math.log(MREG)))
    assert abs(float(sd.cardinality(0)[0]) - 1.0) < 0.01 and abs(float(sd.cardinality(2)[N - 1]) - 1.0) < 0.01


def same(w, mb, picked, labelled=True):
    """mini-batch mb against the restatement over the links at the positions `picked`"""
    ref = w["ref"]
    assert np.array_equal(mb.edge_label_index.cpu().numpy(), w["links"][:, picked]) and mb.batch_size == len(picked)
    assert np.array_equal(mb.edge_label.cpu().numpy(), w["label"][picked]) if labelled else mb.edge_label is None
    for name in ("match", "usum", "uzero", "nsum", "nzero"):
        assert np.array_equal(getattr(mb, name).cpu().numpy().view(ref[name].dtype), ref[name][picked]), name
    # float64 from the same integers
    union, single = hk.card(ref["usum"][picked], ref["uzero"][picked], MREG), hk.card(ref["nsum"][picked], ref["nzero"][picked], MREG)
    for S, Z in ((ref["usum"][picked], ref["uzero"][picked]), (ref["nsum"][picked], ref["nzero"][picked])):
        E = 0.7213 / (1 + 1.079 / MREG) * MREG * MREG / (S.astype(np.float64) / 2.0 ** 33)
        assert np.all((np.abs(E - 2.5 * MREG) > 8 * EPS * E) | (Z == 0))      # no value sits on the seam between the two branches
    I = np.zeros((len(picked), H + 1, H + 1))
    I[:, 1:, 1:] = ref["match"][picked] / NP * union
    A = I[:, 1:, 1:] - I[:, :-1, 1:] - I[:, 1:, :-1] + I[:, :-1, :-1]
    ring = single - np.concatenate([np.zeros((len(picked), 2, 1)), single[:, :, :-1]], axis=2)
    Bf = np.stack([ring[:, 0] - A.sum(2), ring[:, 1] - A.sum(1)], 1)
    # The bound, per link, in units of EPS x C with C = max(every cardinality of the link, m ln m).  A cardinality takes at
    # most 5 roundings of relative size EPS against C (S to float32, the constant, the division; or the constant ln m, a log
    # within 2 ulp, the subtraction, the product): 5.  I = match / n_perm x card adds 2: 7.  A is four I and three additions of
    # terms below 4 C: 4 x 7 + 3 x 4 = 40.  B is two cardinalities and their difference (11), h <= 3 A (120), h - 1 additions of
    # terms below 3 x 4 C (24) and the last subtraction of terms below 13 C: 168.  The float64 side's own error is below EPS^2.
    C = np.maximum(np.maximum(union.max((1, 2)), single.max((1, 2))), MREG * math.log(MREG))
    got = mb.structure.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (len(picked), H * (H + 2))
    assert np.all(np.abs(got[:, :H * H] - A.reshape(-1, H * H)) <= 40 * EPS * C[:, None])
    assert np.all(np.abs(got[:, H * H:] - Bf.reshape(-1, 2 * H)) <= 168 * EPS * C[:, None])
    for s, name in enumerate(("src_card", "dst_card")):
        assert np.all(np.abs(getattr(mb, name).cpu().numpy() - single[:, s]) <= 5 * EPS * C[:, None]), name


@pytest.mark.parametrize("prefetch", [1, 4])
def test_two_epochs_full_and_ragged_mini_batches(world, prefetch):
    ld = loader(world, prefetch=prefetch)
    assert len(ld) == 7
    for epoch in range(2):
        seen = 0
        for j, mb in enumerate(ld):
            same(world, mb, np.arange(j * B, min((j + 1) * B, L)))
            assert mb.call_id == epoch * 7 + j
            seen += 1
        assert seen == 7
    assert ld.slab_allocations == 1                      # the second epoch reused the slab set


def test_shuffle_with_drop_last_and_two_live_iterators(world):
    ld = loader(world, shuffle=True, drop_last=True, seed=5, edge_label=None)
    assert len(ld) == 6
    orders = []
    for epoch in range(2):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(5 * 1000003 + epoch)
        orders.append(torch.randperm(L, device=DEV, generator=gen).cpu().numpy())
    first, second = iter(ld), iter(ld)                   # epochs 0 and 1, interleaved: neither sees the other's slabs
    for j in range(6):
        same(world, next(first), orders[0][j * B:(j + 1) * B], labelled=False)
        same(world, next(second), orders[1][j * B:(j + 1) * B], labelled=False)
    assert ld.slab_allocations == 2
