"""The scaffold the loaders share (tch_geometric.loader), on hand-made CPU tensors: the block containers, the epoch walk,
the skip-gram super-batches and the pointer-list helper.  No GPU and no native library call."""
import pytest
import torch

N_IN, BATCH, PREFETCH, SEED = 23, 5, 2, 7


def _loader_module():
    from tch_geometric import loader
    return loader


# ---- block containers: 3 mini-batches x 2 layers, uneven pointer lists, mini-batch 1 has no edge in layer 0
SEED_PTR = [0, 2, 3, 6]
SRC_PTR = [[0, 4, 5, 10], [0, 6, 9, 16]]            # layer l's sources; layer 0's destinations are the seeds
EDGE_PTR = [[0, 3, 3, 7], [0, 5, 6, 11]]
CALL_ID0 = 40
FAMILIES = [("PinSAGESuperBatch", "PinSAGEBatch", "PinSAGEBlock", "edge_weight", True),
            ("FullNeighborSuperBatch", "FullNeighborBatch", "FullNeighborBlock", "e_id", False)]


def _block_super_batch(family):
    sup, _, _, payload, _ = family
    sb = getattr(_loader_module(), sup)()
    sb.n_layers, sb.call_id0 = 2, CALL_ID0
    sb.input_nodes, sb.seed_ptr = torch.arange(100, 106), SEED_PTR
    sb.layers, dst_ptr = [], SEED_PTR
    for l in range(2):
        n, e = SRC_PTR[l][-1], EDGE_PTR[l][-1]
        sb.layers.append({"n_id": 1000 * (l + 1) + torch.arange(n), "src_ptr": SRC_PTR[l], "dst_ptr": dst_ptr,
                          "edge_index": torch.stack([torch.arange(e), 50 + torch.arange(e)]) + 100 * l,
                          payload: 7000 * (l + 1) + torch.arange(e), "edge_ptr": EDGE_PTR[l]})
        dst_ptr = SRC_PTR[l]
    sb.n_id, sb.node_ptr = sb.layers[-1]["n_id"], SRC_PTR[-1]
    sb.node_attrs = {"x": torch.arange(16 * 3).view(16, 3).float(), "y": torch.arange(16) * 2}
    return sb


@pytest.mark.parametrize("family", FAMILIES, ids=[f[3] for f in FAMILIES])
def test_block_super_batch_indexing(family):
    sb = _block_super_batch(family)
    batch_cls = getattr(_loader_module(), family[1])
    assert len(sb) == 3
    listed = list(sb)
    assert len(listed) == 3 and all(type(b) is batch_cls for b in listed)
    for j in range(3):
        for got in (sb[j], sb[j - 3], listed[j]):
            assert torch.equal(got.n_id, sb.n_id[SRC_PTR[1][j]:SRC_PTR[1][j + 1]])
            assert torch.equal(got.input_nodes, sb.input_nodes[SEED_PTR[j]:SEED_PTR[j + 1]])
    assert torch.equal(sb[-1].n_id, listed[2].n_id)
    for bad in (3, -4):
        with pytest.raises(IndexError):
            sb[bad]


@pytest.mark.parametrize("family", FAMILIES, ids=[f[3] for f in FAMILIES])
def test_block_batches_equal_the_slices(family):
    _, _, block_name, payload, has_call_id = family
    sb = _block_super_batch(family)
    block_cls = getattr(_loader_module(), block_name)
    dst_ptrs = [SEED_PTR, SRC_PTR[0]]
    for j, mb in enumerate(sb):
        assert mb.batch_size == SEED_PTR[j + 1] - SEED_PTR[j]
        assert len(mb.blocks) == 2 and all(type(b) is block_cls for b in mb.blocks)
        for pos, l in enumerate((1, 0)):                     # outermost first: blocks[0] is layer 1
            blk, lay = mb.blocks[pos], sb.layers[l]
            n0, n1, e0, e1 = SRC_PTR[l][j], SRC_PTR[l][j + 1], EDGE_PTR[l][j], EDGE_PTR[l][j + 1]
            assert torch.equal(blk.n_id, lay["n_id"][n0:n1])
            assert torch.equal(blk.edge_index, lay["edge_index"][:, e0:e1]) and blk.edge_index.shape == (2, e1 - e0)
            assert torch.equal(getattr(blk, payload), lay[payload][e0:e1])
            assert blk.n_dst == dst_ptrs[l][j + 1] - dst_ptrs[l][j]
            assert blk.num_src_nodes == n1 - n0 and blk.num_edges == e1 - e0
            other = "e_id" if payload == "edge_weight" else "edge_weight"
            assert not hasattr(blk, other) and not hasattr(blk, "__dict__")
        assert mb.blocks[1].num_edges == (0 if j == 1 else EDGE_PTR[0][j + 1] - EDGE_PTR[0][j])
        assert torch.equal(mb.n_id, mb.blocks[0].n_id) and mb.num_nodes == SRC_PTR[1][j + 1] - SRC_PTR[1][j]
        n0, n1 = SRC_PTR[1][j], SRC_PTR[1][j + 1]
        assert torch.equal(mb.x, sb.node_attrs["x"][n0:n1]) and torch.equal(mb.y, sb.node_attrs["y"][n0:n1])
        with pytest.raises(AttributeError):
            mb.z
        if has_call_id:
            assert mb.call_id == CALL_ID0 + j * 2
        else:
            assert not hasattr(mb, "call_id")


def test_block_takes_its_payload_by_position():
    m = _loader_module()
    a = m.PinSAGEBlock(torch.arange(4), 2, torch.zeros(2, 3, dtype=torch.int64), torch.tensor([5, 6, 7]))
    b = m.FullNeighborBlock(torch.arange(4), 2, torch.zeros(2, 3, dtype=torch.int64), torch.tensor([5, 6, 7]))
    assert a.edge_weight.tolist() == b.e_id.tolist() == [5, 6, 7] and a.num_edges == b.num_edges == 3 and a.n_dst == b.n_dst == 2


# ---- the epoch walk
def _walker(n=N_IN, shuffle=False, drop_last=False, seed=SEED):
    m = _loader_module()
    ld = m._Loader()
    ld.input_nodes = torch.arange(n) * 3 + 1
    ld.batch_size, ld.prefetch, ld.drop_last, ld.shuffle, ld.seed = BATCH, PREFETCH, drop_last, shuffle, seed
    ld.device, ld.epoch = torch.device("cpu"), 0
    return ld


@pytest.mark.parametrize("drop_last", [False, True])
def test_epoch_walk_without_shuffle_is_the_plan(drop_last):
    m = _loader_module()
    ld = _walker(drop_last=drop_last)
    paired = ld.input_nodes * 10
    plan = m._epoch_plan(N_IN, BATCH, PREFETCH, drop_last)
    assert len(ld) == (4 if drop_last else 5) and len(plan) == (2 if drop_last else 3)
    for epoch in range(2):
        launches = list(ld._epoch_launches(ld.input_nodes, paired, None))
        assert ld.epoch == epoch + 1 and len(launches) == len(plan)
        for ((rows, rows_paired, nothing), first_batch), (start, G, width) in zip(launches, plan):
            assert nothing is None and rows.shape == rows_paired.shape == (G, width)
            assert torch.equal(rows.reshape(-1), ld.input_nodes[start:start + G * width])
            assert torch.equal(rows_paired, rows * 10)
            assert first_batch == epoch * len(ld) + start // BATCH
    if not drop_last:
        assert launches[-1][0][0].shape == (1, N_IN - 4 * BATCH)       # the ragged last mini-batch: a launch of its own


@pytest.mark.parametrize("drop_last", [False, True])
def test_epoch_walk_with_shuffle_is_a_function_of_seed_and_epoch(drop_last):
    kept = N_IN // BATCH * BATCH if drop_last else N_IN
    orders = []
    for epoch in range(2):
        gen = torch.Generator(device="cpu")
        gen.manual_seed(SEED * 1000003 + epoch)
        orders.append(torch.randperm(N_IN, generator=gen))
    assert not torch.equal(orders[0], orders[1])
    for _ in range(2):                                       # a rebuilt loader walks the same epochs
        ld = _walker(shuffle=True, drop_last=drop_last)
        paired = ld.input_nodes * 10
        for epoch in range(2):
            launches = list(ld._epoch_launches(ld.input_nodes, paired))
            rows = torch.cat([r.reshape(-1) for (r, _), _ in launches])
            rows_paired = torch.cat([p.reshape(-1) for (_, p), _ in launches])
            assert torch.equal(rows, ld.input_nodes[orders[epoch]][:kept])
            assert torch.equal(rows_paired, rows * 10)
            assert [fb for _, fb in launches] == [epoch * len(ld) + s // BATCH
                                                  for s, _, _ in _loader_module()._epoch_plan(N_IN, BATCH, PREFETCH, drop_last)]
            if not drop_last:
                assert sorted(rows.tolist()) == ld.input_nodes.tolist()
    other_seed = _walker(shuffle=True, drop_last=drop_last, seed=SEED + 1)
    first = torch.cat([r.reshape(-1) for (r,), _ in other_seed._epoch_launches(other_seed.input_nodes)])
    assert not torch.equal(first, other_seed.input_nodes[orders[0]][:kept])


def test_two_live_epoch_walks_take_consecutive_epochs():
    ld = _walker()
    a, b = ld._epoch_launches(ld.input_nodes), ld._epoch_launches(ld.input_nodes)
    assert ld.epoch == 0                                     # an epoch starts when its first launch is asked for
    (_, first_a), (_, first_b) = next(a), next(b)
    assert (first_a, first_b, ld.epoch) == (0, len(ld), 2)
    assert [fb for _, fb in a] == [2, 4] and [fb for _, fb in b] == [len(ld) + 2, len(ld) + 4]
    assert next(ld._epoch_launches(ld.input_nodes))[1] == 2 * len(ld)


# ---- skip-gram super-batches
@pytest.mark.parametrize("with_ts", [None, False, True], ids=["node2vec", "temporal-without-ts", "temporal-with-ts"])
def test_skipgram_super_batch_indexing(with_ts):
    m = _loader_module()
    G, C = 3, 4
    pos, neg = torch.arange(G * 6 * C).view(G, 6, C), 1000 + torch.arange(G * 12 * C).view(G, 12, C)
    pts = pos + 500 if with_ts else None
    if with_ts is None:
        sb, batch_cls = m.SkipGramSuperBatch(pos, neg, 5, 70), m.SkipGramBatch
    else:
        sb, batch_cls = m.TemporalSkipGramSuperBatch(pos, pts, neg, 5, 70), m.TemporalSkipGramBatch
    assert not hasattr(sb, "__dict__") and len(sb) == G
    listed = list(sb)
    assert len(listed) == G
    for g in range(G):
        for got in (sb[g], sb[g - G], listed[g]):
            assert type(got) is batch_cls and got.batch_size == 5 and got.call_id == 70 + g
            assert torch.equal(got.pos_rw, pos[g]) and torch.equal(got.neg_rw, neg[g])
            if with_ts is not None:
                assert got.pos_ts is None if not with_ts else torch.equal(got.pos_ts, pts[g])
    for bad in (G, -G - 1):
        with pytest.raises(IndexError):
            sb[bad]


# ---- helpers
def test_ptr_list():
    ptr = _loader_module()._ptr_list
    assert ptr([]) == [0]
    assert ptr([0, 0, 0]) == [0, 0, 0, 0]
    assert ptr([3, 0, 5, 1]) == [0, 3, 3, 8, 9]
    assert ptr((n for n in (2, 2))) == [0, 2, 4] and type(ptr([1])) is list


def test_super_batch_starts_empty():
    m = _loader_module()
    for sb in (m.SuperBatch(), m.LinkSuperBatch()):
        for name in ("layer_offsets", "layer_nodes", "layer_edges", "seed_counts", "input_time", "node_time", "batch", "root_n_id"):
            assert getattr(sb, name) is None
        assert sb.n_hops == 0 and not hasattr(sb, "__dict__")
