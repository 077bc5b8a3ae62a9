"""Batched negative sampling on the GPU: every call of a tg_neg_sample_batched launch equals the oracle (philox-mode) at call
id first + b and the single operator run alone at that call id, word for word -- samples, rows, cols and counts -- and
writes nothing past its counts.  Both forms (one workgroup per call in LDS; call by call), per-call panic words, and the
NegativeLoader."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
from helpers import load_fake_dataset, load_fake_hetero, load_karate, rel_key

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENT = -7


@pytest.fixture(scope="module")
def tg():
    import tch_geometric
    return tch_geometric


@pytest.fixture(scope="module")
def cabi():
    from tch_geometric import _cabi
    return _cabi


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(cabi, nb, seed, first):
    """fills the slabs with a sentinel, runs the launch -> host copies (samples [T], rows [R], cols [R], counts, panic)"""
    for slab in nb.samples + nb.rows + nb.cols:
        slab.fill_(SENT)
    nb.run(seed, first)
    torch.cuda.synchronize()
    counts, panic = nb.read_state()
    return ([s.cpu().numpy() for s in nb.samples], [r.cpu().numpy() for r in nb.rows], [c.cpu().numpy() for c in nb.cols],
            counts.numpy(), panic.numpy())


def _row_is(slab_row, want, what):
    n = len(want)
    assert np.array_equal(slab_row[:n], want), what
    assert (slab_row[n:] == SENT).all(), "%s: written past its count" % (what,)


def _check_homo(tg, cabi, ptrs, idx, node_count, inputs, num_neg, tries, seed, first, form=None, pad=3, oracle_calls=None):
    """inputs: [n_calls, n_in] host array.  Every call against the single operator; against the oracle too (all calls, or
    the listed ones)."""
    n, (N, B) = len(ptrs) - 1, inputs.shape
    P, I = _cu(ptrs), _cu(idx)
    d_in = _cu(inputs)
    nb = cabi.NegBatched(1, [(0, 0, P, I, node_count)], [d_in], num_neg, tries, N, DEV, homogeneous=True, pad=pad)
    if form is not None:
        assert nb.form == form, (nb.form, nb.lds_bytes)
    assert nb.node_pitch[0] == max(B + B * num_neg + pad, 1) and nb.edge_pitch[0] == max(B * num_neg + pad, 1)
    S, R, Cc, counts, panic = _run(cabi, nb, seed, first)
    assert not panic.any()
    for b in range(N):
        tg.set_rng_state(seed, first + b)
        s, r, c, sc = tg.negative_sample_neighbors_homogenous(P, I, (n, node_count), d_in[b], num_neg, tries)
        assert sc == B and counts[b].tolist() == [s.numel(), r.numel()], b
        _row_is(S[0][b], s.cpu().numpy(), ("samples", b))
        _row_is(R[0][b], r.cpu().numpy(), ("rows", b))
        _row_is(Cc[0][b], c.cpu().numpy(), ("cols", b))
        if oracle_calls is None or b in oracle_calls:
            o = orc.neg_homo(ptrs, idx, (n, node_count), inputs[b], num_neg, tries, orc.rng_philox(seed, first + b))
            assert o[3] == B
            _row_is(S[0][b], o[0], ("samples vs oracle", b))
            _row_is(R[0][b], o[1], ("rows vs oracle", b))
            _row_is(Cc[0][b], o[2], ("cols vs oracle", b))
    return nb


def _rmat12():
    n = 1 << 12
    row, col = orc.rmat_edges(12, n * 16, 21)
    ptrs, idx, _ = orc.to_csr(np.stack([row, col]), n)
    return n, ptrs, idx


def test_homogeneous_karate_256_calls(tg, cabi):
    """negative_sampling.rs:146-171's configuration (34 inputs x 10 x 5), 256 calls with different inputs per call."""
    ei, n = load_karate()
    ptrs, idx, _ = orc.to_csr(ei, n)
    rs = np.random.default_rng(3)
    inputs = np.stack([rs.permutation(n) for _ in range(256)]).astype(np.int64)
    _check_homo(tg, cabi, ptrs, idx, n, inputs, 10, 5, seed=31, first=1000, form=1)


def test_homogeneous_rmat_heavy_duplication_256_calls(tg, cabi):
    """tests/test_gpu_negative.py's heavy-duplication case: 3 000 inputs drawn from 64 distinct values, per call its own
    draw.  60 000 items may run call by call (whatever the device says is accepted, and checked against form()); the same
    duplication at 512 inputs x 7 over a node range of 50 must be fused."""
    n, ptrs, idx = _rmat12()
    inputs = orc.seed_batches(2, 40, 256, 3000, 64).astype(np.int64)
    assert inputs.shape == (256, 3000) and len(np.unique(inputs)) <= 64
    nb = _check_homo(tg, cabi, ptrs, idx, n, inputs, 20, 4, seed=8, first=77)
    assert nb.form == cabi.neg_batched_form(nb.problem)[0]
    small = orc.seed_batches(2, 900, 256, 512, 64).astype(np.int64)
    _check_homo(tg, cabi, ptrs, idx, 50, small, 7, 3, seed=8, first=5000, form=1)


@pytest.mark.parametrize("num_neg,tries,size,n_in", [(7, 3, None, 700), (1, 1, None, 700), (20, 4, 50, 150)])
def test_homogeneous_parameter_corners(tg, cabi, num_neg, tries, size, n_in):
    """The (num_neg, try_count, node range) corners of tests/test_gpu_negative.py, 12 calls per launch, inputs from 64
    distinct values, at sizes that fit the fused kernel (150 x 20 = 3 000 items over a node range of 50: many repeats)."""
    n, ptrs, idx = _rmat12()
    inputs = orc.seed_batches(2, 7, 12, n_in, 64).astype(np.int64)
    _check_homo(tg, cabi, ptrs, idx, size or n, inputs, num_neg, tries, seed=8, first=3, form=1)


def test_homogeneous_degenerate_shapes(tg, cabi):
    """num_neg = 0, try_count = 0, the two-node graph where nothing is admissible, n_inputs = 0: each a launch of several
    calls."""
    n, ptrs, idx = _rmat12()
    inputs = orc.seed_batches(5, 0, 6, 100, n).astype(np.int64)
    nb = _check_homo(tg, cabi, ptrs, idx, n, inputs, 0, 4, seed=1, first=9, form=1)
    assert nb.counts.cpu().tolist() == [[100, 0]] * 6
    nb = _check_homo(tg, cabi, ptrs, idx, n, inputs, 3, 0, seed=1, first=9, form=1)
    assert nb.counts.cpu().tolist() == [[100, 0]] * 6
    p2, i2 = np.array([0, 1, 2], dtype=np.int64), np.array([1, 0], dtype=np.int64)     # 2 nodes, linked both ways
    nb = _check_homo(tg, cabi, p2, i2, 2, np.array([[0, 1], [1, 0], [1, 1], [0, 0]], dtype=np.int64), 3, 4, seed=2, first=0,
                     form=1)
    assert nb.counts.cpu().tolist() == [[2, 0]] * 4
    nb = _check_homo(tg, cabi, p2, i2, 2, np.zeros((5, 0), dtype=np.int64), 3, 4, seed=2, first=0, form=1)
    assert nb.counts.cpu().tolist() == [[0, 0]] * 5


def _hetero_graph(inbound):
    counts, edges = load_fake_hetero()
    node_types, edge_types = sorted(counts), sorted(edges)
    if inbound:
        edge_types = [e for e in edge_types if counts[e[2]] <= counts[e[0]]]
        node_types = sorted({e[0] for e in edge_types} | {e[2] for e in edge_types})
    P, I, S = {}, {}, {}
    for et in edge_types:
        k = rel_key(et)
        P[k], I[k], _ = orc.to_csr(edges[et], (counts[et[0]], counts[et[2]]))
        S[k] = (counts[et[0]], counts[et[2]])
    return counts, node_types, edge_types, P, I, S


@pytest.mark.parametrize("inbound", [False, True])
def test_heterogeneous_128_calls(tg, cabi, inbound):
    """negative_sampling.rs:173-233's configuration (3 negatives, 10 tries) on the fake hetero fixture: inputs with
    duplicates, a type without an `inputs` entry (outbound), 128 calls: per type and per relation equal to orc.neg_hetero
    and to the single operator."""
    counts, node_types, edge_types, P, I, S = _hetero_graph(inbound)
    tix = {t: i for i, t in enumerate(node_types)}
    N, rs = 128, np.random.default_rng(12)
    inputs = {t: (np.arange(0, 200, 2)[None, :] % 60 + rs.integers(0, 40, (N, 1))).astype(np.int64) for t in node_types}
    if not inbound:
        del inputs[node_types[-1]]
    Pd, Id = {k: _cu(v) for k, v in P.items()}, {k: _cu(v) for k, v in I.items()}
    rels = [(tix[et[0]], tix[et[2]], Pd[rel_key(et)], Id[rel_key(et)], S[rel_key(et)][1]) for et in edge_types]
    d_in = {t: _cu(v) for t, v in inputs.items()}
    nb = cabi.NegBatched(len(node_types), rels, [d_in.get(t) for t in node_types], 3, 10, N, DEV, inbound=inbound, pad=2)
    assert nb.form == 1
    Sm, R, Cc, cnt, panic = _run(cabi, nb, 404, 60)
    assert not panic.any()
    T = len(node_types)
    for b in range(N):
        call_in = {t: v[b] for t, v in inputs.items()}
        o = orc.neg_hetero(node_types, edge_types, P, I, S, call_in, 3, 10, inbound, orc.rng_philox(404, 60 + b))
        tg.set_rng_state(404, 60 + b)
        s, r, c, sc = tg.negative_sample_neighbors_heterogenous(node_types, edge_types, Pd, Id, S,
                                                                {t: v[b] for t, v in d_in.items()}, 3, 10, inbound)
        assert sc == o[3]
        for t, nt in enumerate(node_types):
            assert cnt[b, t] == len(o[0][nt]) == s[nt].numel()
            _row_is(Sm[t][b], o[0][nt], ("samples", nt, b))
            assert np.array_equal(s[nt].cpu().numpy(), o[0][nt])
        for q, et in enumerate(edge_types):
            k = rel_key(et)
            assert cnt[b, T + q] == len(o[1][k]) == r[k].numel()
            _row_is(R[q][b], o[1][k], ("rows", k, b))
            _row_is(Cc[q][b], o[2][k], ("cols", k, b))
            assert np.array_equal(r[k].cpu().numpy(), o[1][k]) and np.array_equal(c[k].cpu().numpy(), o[2][k])


def test_forms_agree_with_the_query_and_call_by_call_equals_the_oracle(tg, cabi):
    """40 000 inputs x 5 is past the fused limit: the launch runs call by call and still equals the oracle; form() says
    what ran for it and for the two shapes that must be fused on gfx950.  The call-by-call form's workspace covers a
    single call's."""
    n, ptrs, idx = _rmat12()
    inputs = orc.seed_batches(11, 0, 3, 40000, n).astype(np.int64)
    nb = _check_homo(tg, cabi, ptrs, idx, n, inputs, 5, 5, seed=6, first=21, form=0)
    assert cabi.neg_batched_form(nb.problem) == (0, nb.lds_bytes)
    single = C.c_int64(0)
    cabi.check(cabi.lib.tg_neg_workspace_bytes(C.byref(nb.problem), C.byref(single)))
    assert nb.workspace_bytes >= single.value > 0
    # the two shapes a training loop asks for
    P, I = _cu(ptrs), _cu(idx)
    homo = cabi.neg_problem(1, [(0, 0, P, I, n)], [1024], 5, 5, homogeneous=True)
    form, lds = cabi.neg_batched_form(homo)
    assert form == 1 and 0 < lds <= 160 * 1024 and cabi.neg_batched_workspace_bytes(homo, 256) == 0
    cfg4 = cabi.neg_problem(3, [(s, d, P, I, n) for s, d in [(0, 0), (0, 1), (1, 0), (1, 2), (2, 0)]], [1024, -1, -1], 5, 5)
    assert cabi.neg_batched_form(cfg4)[0] == 1
    got = _check_homo(tg, cabi, ptrs, idx, n, orc.seed_batches(11, 5, 4, 1024, n).astype(np.int64), 5, 5, seed=6, first=2,
                      form=1)
    assert got.lds_bytes == lds


def test_short_workspace_is_refused_on_the_device(cabi):
    """A call-by-call shape with 8 bytes less than tg_neg_batched_workspace_bytes is refused by name before anything is
    launched: every output word keeps its sentinel.  The exact size is accepted."""
    n, ptrs, idx = _rmat12()
    inputs = orc.seed_batches(11, 0, 2, 40000, n).astype(np.int64)
    nb = cabi.NegBatched(1, [(0, 0, _cu(ptrs), _cu(idx), n)], [_cu(inputs)], 5, 5, 2, DEV, homogeneous=True)
    assert nb.form == 0 and nb.workspace_bytes >= 8
    for slab in nb.samples + nb.rows + nb.cols:
        slab.fill_(SENT)
    nb.state.fill_(SENT)
    rng = cabi.TgRng(6, 21)
    rc = cabi.lib.tg_neg_sample_batched(C.byref(nb.problem), C.c_int64(2), C.byref(rng), C.byref(nb.out), cabi.ptr(nb.workspace),
                                        C.c_int64(nb.workspace_bytes - 8), cabi.stream_ptr(DEV))
    msg = cabi.lib.tg_last_error().decode()
    assert rc == 1 and "tg_neg_sample_batched" in msg and "workspace too small" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert all(bool((slab == SENT).all()) for slab in nb.samples + nb.rows + nb.cols) and bool((nb.state == SENT).all())
    nb.run(6, 21)
    torch.cuda.synchronize()
    counts, panic = nb.read_state()
    assert not panic.any() and counts[:, 0].min() >= 40000


def test_panic_is_reported_per_call(tg, cabi):
    """The single-relation inbound case of test_negative_heterogeneous_inbound_panic_is_reported with few items per call
    (2 inputs x 1 negative x 1 try, 64 calls): some calls draw a row past the CSR and panic, others do not.  panic[b] is
    'the oracle raised for call b' for all 64, and every other call equals the oracle."""
    counts, edges = load_fake_hetero()
    et = ("v0", "e0", "v2")                          # 897 src rows, 982 dst nodes
    p, i, _ = orc.to_csr(edges[et], (counts["v0"], counts["v2"]))
    k, size = rel_key(et), (counts["v0"], counts["v2"])
    N, seed = 64, 77
    inputs = np.stack([(np.arange(2) * 7 + 3 * b) % 897 for b in range(N)]).astype(np.int64)
    want = []
    for b in range(N):
        try:
            want.append(orc.neg_hetero(["v0", "v2"], [et], {k: p}, {k: i}, {k: size}, {"v0": inputs[b]}, 1, 1, True,
                                       orc.rng_philox(seed, 100 + b)))
        except RuntimeError:
            want.append(None)
    n_panic = sum(w is None for w in want)
    assert n_panic >= 8 and N - n_panic >= 8, n_panic           # the premise, under the oracle alone (seed 77: 10 of 64)
    nb = cabi.NegBatched(2, [(0, 1, _cu(p), _cu(i), size[1])], [_cu(inputs), None], 1, 1, N, DEV, inbound=True, pad=1)
    assert nb.form == 1
    Sm, R, Cc, cnt, panic = _run(cabi, nb, seed, 100)
    assert panic.tolist() == [int(w is None) for w in want]
    for b, o in enumerate(want):
        if o is None:
            continue
        assert cnt[b].tolist() == [len(o[0]["v0"]), len(o[0]["v2"]), len(o[1][k])]
        _row_is(Sm[0][b], o[0]["v0"], ("samples v0", b))
        _row_is(Sm[1][b], o[0]["v2"], ("samples v2", b))
        _row_is(R[0][b], o[1][k], ("rows", b))
        _row_is(Cc[0][b], o[2][k], ("cols", b))


def test_at_scale_rmat20_512_calls_one_launch(tg, cabi):
    """RMAT-20 CSR built on the device, 1 024 inputs x 5 x 5, 512 calls in ONE launch: all 512 equal the single operator at
    their call ids; 8 of them are replayed by the oracle."""
    n = 1 << 20
    row, col = cabi.rmat_edges(20, n * 16, 0x5EED0014, DEV)
    P, I, _ = cabi.coo_to_csx(row, col, n, n, False)
    del row, col
    seeds = cabi.seed_batches(0xBA7C4, 300, 512, 1024, n, DEV)
    ptrs, idx = P.cpu().numpy(), I.cpu().numpy()
    _check_homo(tg, cabi, ptrs, idx, n, seeds.cpu().numpy(), 5, 5, seed=99, first=1 << 33, form=1, pad=0,
                oracle_calls=(0, 1, 63, 64, 255, 256, 300, 511))


# ---------------------------------------------------------------- NegativeLoader
def _same_homo(got, want, x, B, cid):
    n_id = want.n_id.cpu().numpy()
    assert np.array_equal(got.n_id.cpu().numpy(), n_id) and got.num_nodes == want.num_nodes == len(n_id)
    assert np.array_equal(got.neg_edge_index.cpu().numpy(), want.neg_edge_index.cpu().numpy())
    assert got.batch_size == want.batch_size == B and got.call_id == cid
    assert np.array_equal(got.x.cpu().numpy(), x[n_id]) and np.array_equal(want.x.cpu().numpy(), x[n_id])


def test_negative_loader_homogeneous(tg, cabi):
    """len, drop_last, the ragged last mini-batch, mini-batch j == NegativeSamplerTransform at (seed, call_id0 + j) with
    the gathered attribute, other call ids in the second epoch, prefetch clamped by max_workspace_bytes."""
    from tch_geometric.loader import NegativeLoader
    from tch_geometric.transforms import Graph, NegativeSamplerTransform
    ei, n = load_fake_dataset()
    x = np.random.default_rng(9).standard_normal((n, 5)).astype(np.float32)      # the fixture holds edges only
    data = Graph(edge_index=_cu(ei), num_nodes=n, x=_cu(x))
    nodes = torch.from_numpy(np.random.default_rng(10).integers(0, n, 230))
    tf = NegativeSamplerTransform(data, 4, 3)
    loader = NegativeLoader(data, 4, 3, input_nodes=nodes, batch_size=32, prefetch=3, seed=5, call_id0=40)
    assert len(loader) == 8 and loader.prefetch == 3
    assert len(NegativeLoader(data, 4, 3, input_nodes=nodes, batch_size=32, drop_last=True)) == 7
    first_epoch = []
    for epoch in range(2):
        n_seen = 0
        for j, got in enumerate(loader):
            seeds = nodes[j * 32:(j + 1) * 32]
            cid = 40 + epoch * 8 + j
            tg.set_rng_state(5, cid)
            _same_homo(got, tf(seeds.to(DEV)), x, len(seeds), cid)
            if epoch == 0:
                first_epoch.append(got.neg_edge_index.cpu().numpy())
            elif got.neg_edge_index.shape == first_epoch[j].shape:
                assert not np.array_equal(got.neg_edge_index.cpu().numpy(), first_epoch[j])    # other draws
            n_seen += 1
        assert n_seen == 8 and len(seeds) == 230 - 7 * 32                         # the ragged one came last
    dl = NegativeLoader(data, 4, 3, input_nodes=nodes, batch_size=32, prefetch=3, drop_last=True, seed=5, call_id0=40)
    got = list(dl)
    assert len(got) == 7 and [g.call_id for g in got] == list(range(40, 47))
    # a launch's memory: prefetch x one call's slabs (+ workspace); a small budget clamps prefetch, never below one
    per_call = cabi.neg_batched_bytes(loader._problem(32), 1)
    small = NegativeLoader(data, 4, 3, input_nodes=nodes, batch_size=32, prefetch=64, max_workspace_bytes=5 * per_call + 1,
                           seed=5, call_id0=40)
    assert small.prefetch == 5
    assert NegativeLoader(data, 4, 3, input_nodes=nodes, batch_size=32, prefetch=64, max_workspace_bytes=1).prefetch == 1
    for j, g in enumerate(small):
        tg.set_rng_state(5, 40 + j)
        _same_homo(g, tf(nodes[j * 32:(j + 1) * 32].to(DEV)), x, min(32, 230 - j * 32), 40 + j)
    with pytest.raises(IndexError):
        NegativeLoader(data, 4, 3, input_nodes=torch.tensor([0, n]))


def test_negative_loader_homogeneous_ignores_inbound(tg, cabi):
    """The homogeneous operator has no inbound form and the transform ignores the flag; so does the loader."""
    from tch_geometric.loader import NegativeLoader
    from tch_geometric.transforms import Graph, NegativeSamplerTransform
    ei, n = load_fake_dataset()
    x = np.random.default_rng(9).standard_normal((n, 5)).astype(np.float32)
    data = Graph(edge_index=_cu(ei), num_nodes=n, x=_cu(x))
    nodes = torch.arange(100)
    tf = NegativeSamplerTransform(data, 4, 3, inbound=True)
    got = list(NegativeLoader(data, 4, 3, input_nodes=nodes, batch_size=32, prefetch=2, inbound=True, seed=5, call_id0=9))
    assert len(got) == 4
    for j, g in enumerate(got):
        tg.set_rng_state(5, 9 + j)
        _same_homo(g, tf(nodes[j * 32:(j + 1) * 32].to(DEV)), x, min(32, 100 - j * 32), 9 + j)


def _hetero_data(node_types, edge_types, counts, edges):
    from tch_geometric.transforms import HeteroGraph
    rs = np.random.default_rng(4)
    data, feats = HeteroGraph(), {}
    for nt in node_types:
        feats[nt] = rs.standard_normal((counts[nt], 6)).astype(np.float32)
        data[nt].x, data[nt].num_nodes = _cu(feats[nt]), counts[nt]
    for et in edge_types:
        data[et].edge_index = _cu(edges[et])
    return data, feats


def test_negative_loader_heterogeneous(tg, cabi):
    """Seeds of one node type over the fake hetero fixture (with a seeded attribute x per type): every mini-batch of two
    epochs equals NegativeSamplerTransform at (seed, call_id0 + j), per node type and per relation."""
    from tch_geometric.loader import NegativeLoader
    from tch_geometric.transforms import NegativeSamplerTransform
    counts, edges = load_fake_hetero()
    node_types, edge_types = sorted(counts), sorted(edges)
    data, feats = _hetero_data(node_types, edge_types, counts, edges)
    nt0 = node_types[0]
    nodes = torch.from_numpy(np.random.default_rng(6).integers(0, counts[nt0], 150))
    tf = NegativeSamplerTransform(data, 3, 10)
    loader = NegativeLoader(data, 3, 10, input_nodes=nodes, input_type=nt0, batch_size=32, prefetch=2, seed=7, call_id0=11)
    assert len(loader) == 5 and loader.prefetch == 2
    for epoch in range(2):
        n_seen = 0
        for j, got in enumerate(loader):
            seeds = nodes[j * 32:(j + 1) * 32]
            cid = 11 + epoch * 5 + j
            tg.set_rng_state(7, cid)
            want = tf({nt0: seeds.to(DEV)})
            for nt in node_types:
                n_id = want[nt].n_id.cpu().numpy()
                assert np.array_equal(got[nt].n_id.cpu().numpy(), n_id), (epoch, j, nt)
                assert got[nt].num_nodes == want[nt].num_nodes == len(n_id)
                assert got[nt].batch_size == want[nt].batch_size == (len(seeds) if nt == nt0 else 0)
                assert np.array_equal(got[nt].x.cpu().numpy(), feats[nt][n_id])
            for et in edge_types:
                assert np.array_equal(got[et].neg_edge_index.cpu().numpy(), want[et].neg_edge_index.cpu().numpy()), (epoch, j, et)
            assert got.call_id == cid
            n_seen += 1
        assert n_seen == 5
    with pytest.raises(ValueError):
        NegativeLoader(data, 3, 10, input_nodes=nodes, input_type="nope")


def test_negative_loader_raises_at_the_panicking_mini_batch(tg, cabi):
    """Inbound sampling over ("v0", "e0", "v2") (982 destination ids, 897 CSR rows): mini-batches of 2 seeds x 1 x 1; the
    mini-batches before the first one whose oracle call panics are delivered and equal the transform, then the transform's
    RuntimeError is raised -- although the whole launch (16 mini-batches) had run by then."""
    from tch_geometric.loader import NegativeLoader
    from tch_geometric.transforms import NegativeSamplerTransform
    counts, edges = load_fake_hetero()
    et = ("v0", "e0", "v2")
    data, feats = _hetero_data(["v0", "v2"], [et], counts, edges)
    p, i, _ = orc.to_csr(edges[et], (counts["v0"], counts["v2"]))
    k, size = rel_key(et), (counts["v0"], counts["v2"])
    nodes = torch.from_numpy(np.concatenate([(np.arange(2) * 7 + 3 * b) % 897 for b in range(64)]))
    first_panic = None
    for b in range(64):
        try:
            orc.neg_hetero(["v0", "v2"], [et], {k: p}, {k: i}, {k: size}, {"v0": nodes[2 * b:2 * b + 2].numpy()}, 1, 1, True,
                           orc.rng_philox(77, 100 + b))
        except RuntimeError:
            first_panic = b
            break
    assert first_panic is not None and first_panic >= 1          # seed 77: some mini-batches come before it
    tf = NegativeSamplerTransform(data, 1, 1, inbound=True)
    loader = NegativeLoader(data, 1, 1, input_nodes=nodes, input_type="v0", batch_size=2, prefetch=16, inbound=True, seed=77,
                            call_id0=100)
    delivered = 0
    with pytest.raises(RuntimeError, match="reference panics"):
        for j, got in enumerate(loader):
            assert j < first_panic
            tg.set_rng_state(77, 100 + j)
            want = tf({"v0": nodes[2 * j:2 * j + 2].to(DEV)})
            for nt in ("v0", "v2"):
                assert np.array_equal(got[nt].n_id.cpu().numpy(), want[nt].n_id.cpu().numpy())
            assert np.array_equal(got[et].neg_edge_index.cpu().numpy(), want[et].neg_edge_index.cpu().numpy())
            delivered += 1
    assert delivered == first_panic
    tg.set_rng_state(77, 100 + first_panic)
    with pytest.raises(RuntimeError, match="reference panics"):
        tf({"v0": nodes[2 * first_panic:2 * first_panic + 2].to(DEV)})
